"""LoRA (TimeR1_Trainer's peft_config), CPU side: the fp32 merge chain of tests/lora_cases.py against fp64, the engine's adapter gradients against fp64 autograd on
the UNMERGED form, and the trainer on the oracle op backend (RefOps): construction, the step-0 equalities, what stays frozen, resume, replays,
two ranks over gloo, the adapter file, the refusals, the command line.  tests/test_lora_gpu.py runs the HIP kernels and the HIP trainer on the same cases."""
import json
import os
import sys

import pytest
import torch

import lora_cases as lc
import ref_sync_cases as sc
from helpers import load_case, ref_ops_without
from oracle.ref_ops import RefOps
from time_r1_amd.lora import LoraSpec, TARGET_MODULES
from time_r1_amd.trainer import GRPOConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the merge chain
def test_merge_composite_against_fp64():
    """Within one bf16 ulp everywhere, and RNE of the fp64 value wherever that is further than (r + 3) 2^-24 c relative from a bf16 tie (c: the element's
    cancellation).  The share excluded by that margin stays under 1 % over all cases (about 2^-9 at r = 64 by arithmetic)."""
    total = excluded = 0
    per_r = {}
    for out, in_, r, s in lc.merge_cases():
        w0, a, bt = lc.merge_data(out, in_, r)
        got = lc.merge_composite(w0, a, bt, s)
        y, c = lc.merge64(w0, a, bt, s)
        want, dist, ulp = sc.bf16_rne64(y)
        assert float(c.max()) <= lc.MAX_CANCELLATION, (out, in_, r, s, float(c.max()))
        assert bool(((got.double() - y).abs() <= ulp).all()), (out, in_, r, s)
        clear = dist > (r + 3) * 2.0 ** -24 * c
        assert bool(torch.equal(sc.bits(got)[clear], sc.bits(want)[clear])), (out, in_, r, s, int((sc.bits(got)[clear] != sc.bits(want)[clear]).sum()))
        t, e = per_r.get(r, (0, 0))
        per_r[r] = (t + y.numel(), e + int((~clear).sum()))
        total, excluded = total + y.numel(), excluded + int((~clear).sum())
    for r, (t, e) in sorted(per_r.items()):
        print("r=%d: %d of %d elements within the margin of a tie (%.4f %%)" % (r, e, t, 100.0 * e / t))
    print("all cases: %d of %d excluded (%.4f %%)" % (excluded, total, 100.0 * excluded / total))
    assert excluded / total < 0.01


def test_cases_tell_a_fused_multiply_add_from_the_pinned_chain():
    """The kernel's contract is one rounding per multiplication and per addition.  The shared cases (above all the `big` adapters, where the adapter term dominates the
    sum) must hold elements on which a contracted chain rounds to another bf16 value, or the GPU's bit-for-bit check could not see a contraction."""
    differ = 0
    for out, in_, r, s in lc.merge_cases():
        if s == 0.0:
            continue
        for big, seed in lc.MERGE_DATA:
            w0, a, bt = lc.merge_data(out, in_, r, seed=seed, big=big)
            differ += int((sc.bits(lc.merge_fused_variant(w0, a, bt, s)) != sc.bits(lc.merge_composite(w0, a, bt, s))).sum())
    print("%d elements differ under contraction" % differ)
    assert differ >= 8, differ


def test_zero_scale_and_zero_adapter_return_the_base_weights():
    for out, in_ in lc.MERGE_SHAPES:
        w0, a, bt = lc.merge_data(out, in_, 16)
        assert sc.identity_ok(lc.merge_composite(w0, a, bt, 0.0), w0, lc.merge_acc(a, bt))
        assert torch.equal(lc.merge_composite(w0, a, torch.zeros_like(bt), 2.0), w0)


# ------------------------------------------------------------------------------------------------------------------ spec / refusals
def test_spec_accepts_peft_field_names_from_objects_and_dicts():
    class Cfg:
        r, lora_alpha, target_modules, lora_dropout, bias, use_rslora, use_dora, init_lora_weights = 16, 32, {"q_proj", "v_proj"}, 0.0, "none", False, False, True
    s = LoraSpec.from_config(Cfg())
    assert (s.r, s.r_store, s.targets, s.scale) == (16, 16, ("q_proj", "v_proj"), 2.0)
    s = LoraSpec.from_config(dict(r=8, lora_alpha=16, target_modules="all-linear", use_rslora=True))
    assert s.targets == TARGET_MODULES and s.r_store == 16 and abs(s.scale - 16 / 8 ** 0.5) < 1e-12
    assert LoraSpec.from_config(dict(r=64, lora_alpha=64, target_modules=["down_proj", "q_proj", "q_proj"])).targets == ("q_proj", "down_proj")
    assert LoraSpec.from_config(s) is s


@pytest.mark.parametrize("bad,exc", [
    (dict(r=4), ValueError), (dict(r=12), ValueError), (dict(r=128), ValueError), (dict(target_modules=["q_proj", "lm_head"]), ValueError),
    (dict(target_modules=[]), ValueError), (dict(target_modules=None), ValueError), (dict(target_modules="visual.qkv"), ValueError),
    (dict(lora_dropout=0.05), NotImplementedError), (dict(bias="all"), NotImplementedError), (dict(use_dora=True), NotImplementedError)])
def test_spec_refusals(bad, exc):
    with pytest.raises(exc):
        LoraSpec.from_config({**dict(r=16, lora_alpha=32, target_modules=["q_proj"]), **bad})


def test_trainer_refusals(tmp_path):
    fx = load_case("clip_beta")
    with pytest.raises(NotImplementedError, match="sync_ref_model"):
        lc.tiny_lora_trainer(RefOps(), fx, tmp_path, lc.QV, sync_ref_model=True, ref_model_sync_steps=2)
    with pytest.raises(ValueError, match="shard_optimizer"):
        lc.tiny_lora_trainer(RefOps(), fx, tmp_path, lc.QV, shard_optimizer=True)
    with pytest.raises(NotImplementedError, match="lora_merge / lora_wgrad"):
        lc.tiny_lora_trainer(ref_ops_without("lora_merge", "lora_wgrad"), fx, tmp_path, lc.QV)      # the ref_mixup convention: a backend without the ops is named
    with pytest.raises(NotImplementedError, match="lora_dropout"):
        lc.tiny_lora_trainer(RefOps(), fx, tmp_path, dict(lc.QV, lora_dropout=0.1))
    tr = lc.tiny_lora_trainer(RefOps(), fx, tmp_path, lc.QV, deepspeed="scripts/zero3.json")      # a deepspeed path resolves to the replicated optimizer
    assert not tr.optimizer.sharded and tr.optimizer.lazy_zero is None
    tr.args.sync_ref_model = True                      # settings changed after construction are checked again when train() starts
    with pytest.raises(NotImplementedError, match="sync_ref_model"):
        tr.train()


def test_model_params_can_be_built_without_training_state():
    from oracle.ref_ops import RefOps
    from time_r1_amd.config import tiny_test
    from time_r1_amd.params import ModelParams
    p = ModelParams(tiny_test(), RefOps(), optimizer_state=False, with_grad=False)
    a = p.train
    assert a.grad is None and a.master is None and a.m is None and a.v is None and float(a.w16.abs().max()) > 0
    q = ModelParams(tiny_test(), RefOps())
    assert q.train.grad is not None and torch.equal(q.train.w16, a.w16)
    q.drop_training_state()
    assert q.train.grad is None and q.train.master is None and q.train.m is None and q.train.v is None


# ------------------------------------------------------------------------------------------------------------------ engine: adapter gradients
@pytest.mark.parametrize("recompute", ["none", "mlp"])
@pytest.mark.parametrize("reuse_prefill", [True, False], ids=["prefill+continuation", "full-sequence"])
@pytest.mark.parametrize("targets,r", [("all-linear", 16), ("all-linear", 8), (["q_proj", "v_proj"], 16), (["q_proj", "v_proj"], 8)], ids=["all-r16", "all-r8", "qv-r16", "qv-r8"])
def test_adapter_gradients_against_fp64_autograd_on_the_unmerged_form(targets, r, reuse_prefill, recompute):
    """Bt random (with Bt = 0 every dA is zero).  Tolerance: the CPU engine-gradient tests' (tests/test_trainer_host_logic.py)."""
    lora, res = lc.engine_adapter_grads(RefOps(), targets, r, recompute, reuse_prefill)
    assert len(res) == 2 * lora.cfg.text.n_layers * len(lora.spec.targets)
    for name, (mine, gold) in res.items():
        gold = gold.float()
        assert float(gold[:r].abs().max()) > 0, name
        assert torch.allclose(mine, gold, atol=2e-5 * max(1.0, gold.abs().max().item()), rtol=2e-3), (name, float((mine - gold).abs().max()))
        if r == 8:
            assert float(mine[8:].abs().max()) == 0.0, "the padding rows of a rank-8 adapter get no gradient"


# ------------------------------------------------------------------------------------------------------------------ trainer
def test_construction_step_zero_and_what_stays_frozen(tmp_path):
    fx = load_case("clip_beta")
    from helpers import golden_params
    ops = RefOps()
    _, pol, _ = golden_params(ops, fx)
    loaded = pol.train.w16.clone()
    tr = lc.tiny_lora_trainer(ops, fx, tmp_path / "lora", lc.QV, pol=pol)
    a = tr.params.train
    assert torch.equal(a.w16, loaded), "Bt = 0: the first merge returns the loaded weights"
    assert a.grad is None and a.master is None and a.m is None and a.v is None
    assert tr.ref_model is tr.lora.base and torch.equal(tr.lora.base.w16, loaded)
    assert tr.lora.numel() == 2 * 8 * ((128 + 128) + (128 + 64)) and tr.lora.train.numel >= 2 * tr.lora.numel()      # r = 8 stored as 16 rows
    A = tr.lora.train.view(tr.lora.train.master, "l0.q.A")
    assert float(A[:8].abs().max()) > 0 and float(A[:8].abs().max()) <= 1 / 128 ** 0.5 and float(A[8:].abs().max()) == 0
    assert float(tr.lora.train.view(tr.lora.train.master, "l1.v.Bt").abs().max()) == 0
    # the frozen parts' backward ops are never called; the full-parameter trainer on the same rows calls every one of them
    spied = ("gelu_bwd", "layernorm_bwd", "embed_bwd")
    calls = {}

    def spy(trn, tag):
        for n in spied:
            orig = getattr(trn.ops, n)
            setattr(trn.ops, n, lambda *x, _o=orig, _k=(tag, n), **k: (calls.__setitem__(_k, calls.get(_k, 0) + 1), _o(*x, **k))[1])
    spy(tr, "lora")
    snaps, first = lc.run_snapshots(tr)
    full = lc.tiny_lora_trainer(RefOps(), fx, tmp_path / "full", None)
    spy(full, "full")
    _, first_full = lc.run_snapshots(full)
    assert all(calls.get(("full", n), 0) > 0 for n in spied) and not any(calls.get(("lora", n), 0) for n in spied), calls
    assert torch.equal(first["logp"], first_full["logp"]), "step 0: the merged policy is the loaded one"
    assert tr.state.log_history[0]["kl"] == 0.0 and tr.state.log_history[1]["kl"] > 0, "the reference is the base copy"
    assert [s["step"] for s in snaps] == [1, 2, 3]
    m = lc.targeted_mask(tr)
    end = snaps[-1]
    assert torch.equal(end["base"], loaded), "W0 never moves"
    assert torch.equal(end["w"][~m], loaded[~m]), "embedding, norms, biases, lm_head, merger and the untargeted projections keep their bits"
    off, shape = a.offsets["l0.o.w"]
    assert not bool(m[off: off + shape[0] * shape[1]].any()) and bool(m[a.offsets["l0.qkv.w"][0]])
    assert bool((end["w"][m] != loaded[m]).any())
    assert float(tr.lora.train.view(tr.lora.train.master, "l0.q.A")[8:].abs().max()) == 0.0, "rank 8: the padding rows stay zero through AdamW"


def test_merged_weights_are_the_fp32_merge_of_the_saved_adapter(tmp_path):
    """save_model writes the merged model.safetensors and, beside it, the adapter in peft's key layout (unpadded, lora_B transposed back): merging the saved
    adapter in fp32 onto the base weights and casting once gives the saved weights."""
    from safetensors.torch import load_file
    fx = load_case("clip_beta")
    tr = lc.tiny_lora_trainer(RefOps(), fx, tmp_path, lc.QV, n_rows=2)
    lc.run_snapshots(tr)
    tr.save_model(str(tmp_path / "out"))
    ad = load_file(str(tmp_path / "out" / "adapter_model.safetensors"))
    cfg = json.load(open(tmp_path / "out" / "adapter_config.json"))
    assert cfg["r"] == 8 and cfg["lora_alpha"] == 16 and cfg["target_modules"] == ["q_proj", "v_proj"] and cfg["peft_type"] == "LORA" and cfg["bias"] == "none"
    t = tr.cfg.text
    assert len(ad) == 2 * 2 * t.n_layers
    ka = "base_model.model.model.language_model.layers.1.self_attn.v_proj.lora_A.weight"
    kb = "base_model.model.model.language_model.layers.1.self_attn.v_proj.lora_B.weight"
    assert ad[ka].shape == (8, t.hidden) and ad[kb].shape == (t.kv_dim, 8) and ad[ka].dtype == torch.float32
    merged = load_file(str(tmp_path / "out" / "model.safetensors"))["model.language_model.layers.1.self_attn.v_proj.weight"]
    w0 = tr.lora.base.w("l1.qkv.w")[t.q_dim + t.kv_dim:]
    want = w0.float() + cfg["lora_alpha"] / cfg["r"] * (ad[kb] @ ad[ka])
    assert float((ad[kb] @ ad[ka]).abs().max()) > 0
    assert torch.allclose(merged.float(), want, atol=1e-6, rtol=0)          # (the kernel's chain and a matmul order the r products differently: fp32 rounding)
    # round trip: the exported tensors are the masters' first r rows
    sd, _ = tr.lora.export_adapter()
    a = tr.lora.train
    assert torch.equal(sd[ka], a.view(a.master, "l1.v.A")[:8]) and torch.equal(sd[kb].t(), a.view(a.master, "l1.v.Bt")[:8])


def test_resume_continues_bit_for_bit(tmp_path):
    fx = load_case("clip_beta")
    ops = RefOps()
    tr = lc.tiny_lora_trainer(ops, fx, tmp_path / "a", lc.ALL_LINEAR, n_rows=4, save_steps=2)
    snaps, _ = lc.run_snapshots(tr)
    d = tmp_path / "a" / "checkpoint-2"
    for f in ("model.safetensors", "adapter_model.safetensors", "adapter_config.json", "reference_policy.pt", "optimizer_rank0.pt"):
        assert os.path.exists(d / f), f
    assert torch.equal(torch.load(d / "reference_policy.pt", weights_only=False)["ref_w16"], snaps[0]["base"]), "reference_policy.pt holds W0"
    opt = torch.load(d / "optimizer_rank0.pt", weights_only=False)
    assert opt["master"].numel() == tr.lora.train.numel and opt["shard"] is None, "optimizer_rank*.pt holds the adapter state"
    tr2 = lc.tiny_lora_trainer(ops, fx, tmp_path / "b", lc.ALL_LINEAR, n_rows=4)
    snaps2, _ = lc.run_snapshots(tr2, ckpt=str(d))
    assert [s["step"] for s in snaps2] == [3, 4]
    for k in ("w", "base", "master"):
        assert torch.equal(snaps2[0][k], snaps[2][k]) and torch.equal(snaps2[1][k], snaps[3][k]), k
    keys = ("loss", "kl", "reward", "reward_std", "grad_norm", "generation_entropy", "completion_length")
    assert [{k: l[k] for k in keys} for l in tr2.state.log_history[-2:]] == [{k: l[k] for k in keys} for l in tr.state.log_history[-2:]]


def test_resume_from_a_model_only_checkpoint_is_refused(tmp_path):
    """save_only_model=True writes no optimizer_rank*.pt, which under LoRA is the adapter state: resuming from it would load the merged weights and then merge
    them away with W0 + fresh adapters at the first step.  It raises before anything is loaded."""
    fx = load_case("clip_beta")
    ops = RefOps()
    tr = lc.tiny_lora_trainer(ops, fx, tmp_path / "a", lc.QV, n_rows=1, save_steps=1, save_only_model=True)
    lc.run_snapshots(tr)
    d = tmp_path / "a" / "checkpoint-1"
    assert os.path.exists(d / "model.safetensors") and not os.path.exists(d / "optimizer_rank0.pt")
    tr2 = lc.tiny_lora_trainer(ops, fx, tmp_path / "b", lc.QV, n_rows=2)
    w = tr2.params.train.w16.clone()
    with pytest.raises(ValueError, match="optimizer_rank0.pt"):
        tr2.train(resume_from_checkpoint=str(d))
    assert torch.equal(tr2.params.train.w16, w) and tr2.state.global_step == 0


def test_two_updates_per_rollout_merge_between_the_replays(tmp_path):
    fx = load_case("clip_beta")
    tr = lc.tiny_lora_trainer(RefOps(), fx, tmp_path, lc.ALL_LINEAR, mu=2, ga=1, n_rows=2)
    merges, versions = [], []
    orig = tr.lora.merge
    tr.lora.merge = lambda *a, **k: (orig(*a, **k), merges.append(tr.state.global_step), versions.append(tr.params.train.version))[0]
    snaps, _ = lc.run_snapshots(tr)
    assert [s["step"] for s in snaps] == [1, 2, 3, 4] and merges == [0, 1, 2, 3], "one merge behind every optimizer step, replays included"
    assert versions == sorted(set(versions)), "every merge bumps the arena's version"
    assert not torch.equal(snaps[0]["w"], snaps[1]["w"]), "the replay ran on the re-merged weights and moved them again"
    assert "policy_kl_old" in tr.state.log_history[1] and tr.state.log_history[1]["policy_kl_old"] > 0


def _worker(rank, world, port, q, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import lora_cases as lc
    from helpers import load_case
    tr = lc.tiny_lora_trainer(RefOps(), load_case("clip_beta"), os.path.join(out, "r%d" % rank), lc.ALL_LINEAR, n_rows=2)
    assert tr.dp.enabled and tr.dp.world == 2 and not tr.optimizer.sharded and tr.lora.train.shard is None
    snaps, _ = lc.run_snapshots(tr)                # 2 rows over 2 ranks: one optimizer step, each rank on its own row
    assert [s["step"] for s in snaps] == [1]
    q.put((rank, snaps[0]["master"].numpy().copy(), snaps[0]["w"].numpy().copy(), tr.last_completions))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_identical_adapters_and_merged_weights(tmp_path):
    import socket
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][3] != res[1][3], "the ranks trained on different rows"
    assert (res[0][1] == res[1][1]).all() and (res[0][2] == res[1][2]).all()
    assert float(abs(res[0][1]).max()) > 0


def test_ft_trainer_accepts_a_peft_config_too(tmp_path):
    from time_r1_amd.trainer import TimeR1_Trainer_ft
    tr = lc.tiny_lora_trainer(RefOps(), load_case("clip_beta"), tmp_path, lc.QV, cls=TimeR1_Trainer_ft)
    assert tr.lora is not None and tr.engine.lora is tr.lora and tr.params.train.grad is None


def test_the_lora_flags_parse_from_the_command_line(monkeypatch):
    sys.path.insert(0, ROOT)
    import train_grpo
    seen = {}

    class Stop(Exception):
        pass

    def trainer(model=None, reward_funcs=None, metric_funcs=None, args=None, **kw):
        seen["kw"] = kw
        raise Stop()
    monkeypatch.setattr(train_grpo, "init_from_env", lambda *a, **k: None)
    monkeypatch.setattr(train_grpo, "load_json_dataset_tg", lambda *a, **k: [])
    monkeypatch.setattr(train_grpo, "TimeR1_Trainer", trainer)
    base = ["train_grpo.py", "--model_name_or_path", "m", "--train_data_path", "d"]
    monkeypatch.setattr(sys, "argv", base + ["--use_peft", "--lora_r", "64", "--lora_alpha", "128", "--lora_target_modules", "all-linear", "--use_rslora", "true"])
    with pytest.raises(Stop):
        train_grpo.main()
    s = LoraSpec.from_config(seen["kw"]["peft_config"])
    assert (s.r, s.lora_alpha, s.targets, s.use_rslora) == (64, 128.0, TARGET_MODULES, True)
    monkeypatch.setattr(sys, "argv", base + ["--use_peft", "true", "--lora_target_modules", "q_proj", "o_proj"])
    with pytest.raises(Stop):
        train_grpo.main()
    s = LoraSpec.from_config(seen["kw"]["peft_config"])
    assert (s.r, s.lora_alpha, s.targets) == (16, 32.0, ("q_proj", "o_proj"))
    monkeypatch.setattr(sys, "argv", base)
    with pytest.raises(Stop):
        train_grpo.main()
    assert "peft_config" not in seen["kw"]


def test_the_two_symbols_are_declared_and_exported():
    import ctypes
    from time_r1_amd import hip
    decls = hip.parse_header()
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in ("tr1_lora_merge", "tr1_lora_wgrad"):
        assert name in decls and hasattr(raw, name), name
    assert len(decls) == 103
    from time_r1_amd.ops import HipOps
    assert HipOps.LORA_WGRAD_MCHUNK == 256 and HipOps.lora_wgrad_splits(257, 8) == (2, 256) and HipOps.lora_wgrad_splits(256, 8) == (1, 256)
    assert HipOps.lora_wgrad_splits(5074, 18944) == (3, 1792)
