"""activation_recompute="mlp" on the oracle op backend (CPU): exact gradients against "none", what the context holds, the row ranges of the backward's
recompute launches, and the public interface (validation, "none" is the parent's run, trainer step / resume / two gloo ranks).
tests/test_recompute_gpu.py runs the same shapes on HipOps.  Cases and harness: tests/recompute_cases.py."""
import itertools
import json
import os
import sys

import pytest
import torch

import ratio_cases as rc
import recompute_cases as rcc
from helpers import GOLDEN, load_case
from oracle.ref_ops import RefOps
from time_r1_amd.config import qwen2_vl_7b, qwen2_5_vl_7b
from time_r1_amd.grpo import GRPOCore
from time_r1_amd.model import Engine
from time_r1_amd.trainer import GRPOConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ exact gradients
@pytest.mark.parametrize("variant", ["qwen2_vl", "qwen2_5_vl"])
@pytest.mark.parametrize("reuse_prefill", [True, False], ids=["prefill+continuation", "full-sequence"])
@pytest.mark.parametrize("shape", list(rcc.SHAPES))
def test_gradients_and_outputs_equal_the_none_run_bit_for_bit(shape, reuse_prefill, variant):
    ops = RefOps()
    for beta, fix_vit in itertools.product((0.0, 0.04), (True, False)):
        kw = dict(variant=variant, beta=beta, fix_vit=fix_vit, reuse_prefill=reuse_prefill)
        none = rcc.micro_steps(ops, rcc.SHAPES[shape], "none", **kw)
        mlp = rcc.micro_steps(ops, rcc.SHAPES[shape], "mlp", **kw)
        rcc.assert_equal_runs(mlp, none, (shape, kw))


@pytest.mark.parametrize("fix_vit", [True, False])
def test_a_replayed_update_with_an_entropy_bonus_is_exact_too(fix_vit):
    """num_iterations = 2 at the core: the first pass (prefill + continuation), the weights move, then forward_logps(replay=True) - the full-sequence path into the
    pooled slot-0 buffers - and the ratio loss, with entropy_coef != 0 in both passes."""
    ops = RefOps()
    kw = dict(beta=0.04, fix_vit=fix_vit, replay=True, entropy_coef=0.01)
    none = rcc.micro_steps(ops, rcc.SHAPES["tail"], "none", **kw)
    mlp = rcc.micro_steps(ops, rcc.SHAPES["tail"], "mlp", **kw)
    assert "replay_grad" in mlp[0] and not torch.equal(mlp[0]["replay_grad"], mlp[0]["grad"])
    rcc.assert_equal_runs(mlp, none, "replay")


# ------------------------------------------------------------------------------------------------------------ saved state
def test_bytes_per_row_and_layer_at_7b_width():
    for cfg in (qwen2_vl_7b(), qwen2_5_vl_7b()):
        L = cfg.text.n_layers
        assert Engine(cfg, None, None).ctx_bytes(1) == 157704 * L
        assert Engine(cfg, None, None, activation_recompute="none").ctx_bytes(19650) == 157704 * L * 19650
        eng = Engine(cfg, None, None, activation_recompute="mlp")
        assert eng.ctx_bytes(1) == 29704 * L and eng.ctx_bytes(19650) == 29704 * L * 19650
        # the one transient set: xn, xn2, gu, a of ONE layer = what the mode drops per layer
        assert eng.recompute_set_bytes(1) == 157704 - 29704
        assert eng.ctx_bytes(19650) < Engine.CTX_STASH_GB * 1e9 < Engine(cfg, None, None).ctx_bytes(19650)     # configuration 4 leaves the stash regime


@pytest.mark.parametrize("reuse_prefill", [True, False], ids=["prefill+continuation", "full-sequence"])
@pytest.mark.parametrize("mode", ["none", "mlp"])
@pytest.mark.parametrize("shape", ["tail", "no-tail"])
def test_the_context_holds_exactly_ctx_bytes(shape, mode, reuse_prefill):
    """bf16 activations on the oracle backend, so the formula's 2 bytes per element are the tensors' own: the bytes of the distinct tensors of the per-layer
    records (K is the cache's and lse is per head: neither is in the formula) equal ctx_bytes(M); a replay's context (pooled buffers) too."""
    seen = []

    def on_ctx(eng, st):
        ctx, M = st.llm_ctx, st.layout.M
        held = {}
        for L in ctx["layers"]:
            for k in rcc.RECOMPUTED:
                assert (k in L) == (mode == "none"), (k, sorted(L))
            for k, v in L.items():
                if torch.is_tensor(v) and k not in ("k", "lse"):
                    assert v.shape[0] == M
                    held[v.data_ptr()] = v.numel() * v.element_size()
        seen.append((sum(held.values()), eng.ctx_bytes(M), M))
    P, G, C = rcc.SHAPES[shape]
    rcc.micro_steps(RefOps(torch.bfloat16), (P, G, C), mode, reuse_prefill=reuse_prefill, replay=True, on_ctx=on_ctx)
    assert len(seen) == 2
    t = rcc.CONFIGS["qwen2_vl"]().text
    per_row = {"none": 2 * (4 * t.hidden + t.kv_dim + 2 * t.q_dim + 3 * t.intermediate) + 8, "mlp": 2 * (2 * t.hidden + t.kv_dim + 2 * t.q_dim) + 8}[mode]
    for held, formula, M in seen:
        assert M == P + G * C and held == formula == M * t.n_layers * per_row, (held, formula, M * t.n_layers * per_row)


def test_pooled_buffer_sets_have_no_recomputed_buffers():
    ops = RefOps(torch.bfloat16)
    for mode in ("none", "mlp"):
        cfg, pol, eng, core = rcc.build(ops, mode)
        bufs, stash = eng.alloc_ctx_bufs(166, slot=0, prefill_rows=70)
        assert not stash and len(bufs) == cfg.text.n_layers
        for L in bufs:
            assert set(L) == (set(Engine.SAVED) | {"rstd1", "rstd2"}) - (set(rcc.RECOMPUTED) if mode == "mlp" else set())
    # switching the mode on a live engine drops the other mode's pooled sets
    eng.set_activation_recompute("none")
    assert "xn" in eng.alloc_ctx_bufs(166, slot=0)[0]


def test_stash_and_unstash_work_on_the_keys_that_exist(monkeypatch):
    """The large-sequence regime forced at a small size (CTX_STASH_GB = 0): slot 1 gets a stash of the prompt rows, unstash_ctx moves it into the full set."""
    ops = RefOps(torch.bfloat16)
    monkeypatch.setattr(Engine, "CTX_STASH_GB", 0.0)
    cfg, pol, eng, core = rcc.build(ops, "mlp")
    bufs, stash = eng.alloc_ctx_bufs(166, slot=1, prefill_rows=70)
    assert stash and bufs[0]["h"].shape[0] == 70 and not set(bufs[0]) & set(rcc.RECOMPUTED)
    for L in bufs:
        for v in L.values():
            v.fill_(1.0)
    pctx = eng.unstash_ctx(dict(bufs=bufs, stash=True), 70, 166)
    assert not pctx["stash"] and pctx["bufs"][0]["h"].shape[0] == 166 and float(pctx["bufs"][1]["q"][:70].float().min()) == 1.0


# ------------------------------------------------------------------------------------------------------------ row ranges
def _glu_rows(shape, mode, reuse_prefill):
    """-> ({layer: [rows of each forward gemm_glu call]}, the same of the backward) of one micro-step on the policy's weights."""
    ops = RefOps()
    P, G, C = rcc.SHAPES[shape]
    cfg, pol, eng, core = rcc.build(ops, mode, G=G, C=C, reuse_prefill=reuse_prefill)
    layer_of = {pol.train.w("l%d.gu.w" % i).data_ptr(): i for i in range(cfg.text.n_layers)}
    rows = {False: {}, True: {}}
    state = {"bwd": False}
    glu, bwd = ops.gemm_glu, eng.llm_bwd

    def spy_glu(x, w, *a, **k):
        rows[state["bwd"]].setdefault(layer_of[w.data_ptr()], []).append(int(x.shape[0]))
        if state["bwd"]:
            assert k.get("save_gu", True) and k.get("a_out") is not None and k.get("gu_out") is not None      # into the transient set
        else:
            assert k.get("save_gu", True) == (mode == "none")
        return glu(x, w, *a, **k)

    def spy_bwd(*a, **k):
        state["bwd"] = True
        try:
            return bwd(*a, **k)
        finally:
            state["bwd"] = False
    ops.gemm_glu, eng.llm_bwd = spy_glu, spy_bwd
    toks, mask, adv = rcc.forced_inputs(G, C)
    st = core.prepare(*rcc.prompt_for(cfg, P))
    if reuse_prefill:
        core.rollout(st)
    else:
        from time_r1_amd.positions import PackedLayout
        st.layout = PackedLayout(st.P, G, C)
    st.completion_ids = toks
    core.forward_logps(st)
    core.loss_backward(st, mask, adv, 1.0)
    return rows[False], rows[True]


@pytest.mark.parametrize("shape,reuse_prefill,want", [
    ("tail", True, {0: [70, 96], 1: [1, 96]}),                       # the tail layer's prompt piece is ONE row (P - 1); the continuation runs all of its rows
    ("tail", False, {0: [166], 1: [97]}),
    ("no-tail", True, {0: [20, 96], 1: [20, 96]}),
    ("no-tail", False, {0: [116], 1: [116]}),
    ("short-continuation", True, {0: [70, 48], 1: [1, 48]}),         # 48 rows: the other side of gemm_glu's 64-row switch from the 118-row sequence
    ("short-continuation", False, {0: [118], 1: [49]}),
])
def test_the_backward_recomputes_over_the_forwards_row_ranges(shape, reuse_prefill, want):
    fwd, bwd = _glu_rows(shape, "mlp", reuse_prefill)
    assert fwd == want, fwd
    assert bwd == fwd, (bwd, fwd)
    fwd_none, bwd_none = _glu_rows(shape, "none", reuse_prefill)
    assert fwd_none == want and bwd_none == {}


# ------------------------------------------------------------------------------------------------------------ interface
def test_validation_names_the_two_values():
    cfg = rcc.CONFIGS["qwen2_vl"]()
    for bad in ("full", "MLP", "", True):
        for make in (lambda: GRPOConfig(activation_recompute=bad), lambda: Engine(cfg, None, None, activation_recompute=bad), lambda: rcc.build(RefOps(), bad)):
            with pytest.raises(ValueError, match='"none" or "mlp"'):
                make()
    with pytest.raises(ValueError, match='"none" or "mlp"'):
        GRPOConfig(activation_recompute=None)
    assert GRPOConfig().activation_recompute == "none" and GRPOConfig(activation_recompute="mlp").activation_recompute == "mlp"
    # GRPOCore(activation_recompute=None), the default, keeps the engine's own setting
    cfg, pol, eng, core = rcc.build(RefOps(), "mlp", through="engine")
    assert eng.activation_recompute == "mlp" and GRPOCore(eng, None, 4, 24, beta=0.0).eng.recompute_mlp
    assert rcc.build(RefOps(), "mlp", through="core")[2].recompute_mlp and not rcc.build(RefOps(), None)[2].recompute_mlp


def _op_calls(mode, reuse_prefill):
    spy = rcc.Spy(RefOps())
    rcc.micro_steps(spy, rcc.SHAPES["tail"], mode, beta=0.04, reuse_prefill=reuse_prefill)
    return [list(c) for c in spy.calls]


@pytest.mark.parametrize("reuse_prefill", [True, False], ids=["prefill+continuation", "full-sequence"])
def test_none_issues_the_parents_op_calls(reuse_prefill):
    """tests/golden/recompute_none_op_calls.json: (op name, rows of its first tensor) of every op call of one micro-step, recorded on the commit before the option
    existed.  The default and an explicit "none" issue exactly that sequence; "mlp" differs from it only by the recompute launches inside the backward."""
    gold = json.load(open(os.path.join(GOLDEN, "recompute_none_op_calls.json")))["reuse_prefill" if reuse_prefill else "full_sequence"]
    assert _op_calls(None, reuse_prefill) == gold
    assert _op_calls("none", reuse_prefill) == gold
    mlp = _op_calls("mlp", reuse_prefill)
    rebuilt = ("rmsnorm_fwd", "gemm_glu")
    assert [c for c in mlp if c[0] not in rebuilt] == [c for c in gold if c[0] not in rebuilt]
    # per layer and forward launch (two after a prefill + continuation): the ln2 norm, the gate/up GEMM and the ln1 norm
    assert len(mlp) - len(gold) == 2 * 3 * (2 if reuse_prefill else 1)


def test_gradient_checkpointing_alone_changes_nothing(tmp_path):
    fx = load_case("clip_beta")
    runs = {}
    for name, over in (("plain", {}), ("flag", dict(gradient_checkpointing=True)), ("mlp", dict(gradient_checkpointing=True, activation_recompute="mlp"))):
        tr = rc.tiny_trainer(RefOps(), fx, tmp_path / name, mu=1, ga=2, n_rows=2, **over)
        assert tr.engine.activation_recompute == ("mlp" if name == "mlp" else "none")
        rec = rc.run_recorded(tr)
        runs[name] = (rec["masters"], tr.state.log_history)
    assert len(runs["plain"][0]) == 1
    for name in ("flag", "mlp"):
        assert torch.equal(rcc.bits(runs[name][0][0]), rcc.bits(runs["plain"][0][0])), name
        strip = lambda log: {k: v for k, v in log.items() if not k.startswith("perf/") and "per_sec" not in k and k != "train_runtime"}
        assert [strip(l) for l in runs[name][1]] == [strip(l) for l in runs["plain"][1]], name


def test_trainer_steps_and_resume_match_none_bit_for_bit(tmp_path):
    """num_iterations = 2, GA = 2, 4 rows: 4 optimizer steps (2 of them replays) with sampled rollouts; then checkpoint-2 of the "mlp" run resumed in "mlp"."""
    fx = load_case("clip_beta")
    masters = {}
    for mode in ("none", "mlp"):
        tr = rc.tiny_trainer(RefOps(), fx, tmp_path / mode, mu=2, save_steps=2, activation_recompute=mode)
        masters[mode] = rc.run_recorded(tr)["masters"]
        assert tr.state.global_step == 4
    for a, b in zip(masters["mlp"], masters["none"]):
        assert torch.equal(rcc.bits(a), rcc.bits(b))
    tr = rc.tiny_trainer(RefOps(), fx, tmp_path / "resumed", mu=2, activation_recompute="mlp")
    rec = rc.run_recorded(tr, ckpt=str(tmp_path / "mlp" / "checkpoint-2"))
    assert tr.state.global_step == 4 and len(rec["masters"]) == 2
    tr0 = rc.tiny_trainer(RefOps(), fx, tmp_path / "resumed-none", mu=2)
    rec0 = rc.run_recorded(tr0, ckpt=str(tmp_path / "none" / "checkpoint-2"))
    assert torch.equal(rcc.bits(rec["masters"][-1]), rcc.bits(rec0["masters"][-1]))


def test_the_setting_parses_from_the_command_line(monkeypatch):
    sys.path.insert(0, ROOT)
    import train_grpo
    seen = {}

    class Stop(Exception):
        pass

    def trainer(model=None, reward_funcs=None, metric_funcs=None, args=None, **kw):
        seen["args"] = args
        raise Stop()
    monkeypatch.setattr(train_grpo, "init_from_env", lambda *a, **k: None)
    monkeypatch.setattr(train_grpo, "load_json_dataset_tg", lambda *a, **k: [])
    monkeypatch.setattr(train_grpo, "TimeR1_Trainer", trainer)
    base = ["train_grpo.py", "--model_name_or_path", "m", "--train_data_path", "d"]
    for extra, want in (([], ("none", False)), (["--activation_recompute", "mlp", "--gradient_checkpointing", "true"], ("mlp", True))):
        monkeypatch.setattr(sys, "argv", base + extra)
        with pytest.raises(Stop):
            train_grpo.main()
        assert (seen["args"].activation_recompute, seen["args"].gradient_checkpointing) == want
    monkeypatch.setattr(sys, "argv", base + ["--activation_recompute", "layer"])
    with pytest.raises(ValueError, match='"none" or "mlp"'):
        train_grpo.main()


# ------------------------------------------------------------------------------------------------------------ two gloo ranks
def _gloo_worker(rank, world, port, q, mode):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import ratio_cases
    from helpers import load_case as load
    fx = load("clip_beta")
    tr = ratio_cases.tiny_trainer(RefOps(), fx, "/tmp/tr1_recompute_gloo_%s_%d" % (mode, rank), mu=1, ga=1, n_rows=2, activation_recompute=mode,
                                  grad_wire_dtype="fp32", shard_optimizer=False)
    assert tr.dp.enabled and tr.dp.world == 2 and tr.engine.activation_recompute == mode
    tr.args.learning_rate = 1e-3
    tr.accumulation_window([[tr.train_dataset[rank]]])          # the last micro-step of the window: layer ranges go to the all-reduce from inside llm_bwd
    assert tr.optimizer.sync.active and len(tr.optimizer.sync.pending) >= tr.cfg.text.n_layers
    tr.optimizer.step()
    q.put((rank, tr.params.train.master.numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_match_none_bit_for_bit():
    import socket
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    out = {}
    for mode in ("none", "mlp"):
        q = ctx.Queue()
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q, mode)) for r in range(2)]
        for p in procs:
            p.start()
        res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda x: x[0])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        assert (res[0][1] == res[1][1]).all()
        out[mode] = torch.from_numpy(res[0][1])
    assert torch.equal(rcc.bits(out["mlp"]), rcc.bits(out["none"]))
