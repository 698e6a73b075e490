"""fix_vit=False (the reference's default, main.py:44-49): the patch embedding, every vision block and the merger train (reference
timer1_trainer.py:267-288).  CPU, oracle ops injected through `ops=` (RefOps.quickgelu_bwd is the one op only a training tower asks
for).  The golden captures hold the reference's gradient norms of every tower tensor (the generator built the
trainer without freezing anything, and the captured reference tower equals the policy tower, which is what fix_vit=False gives at step 0)."""
import os
import sys

import pytest
import torch

from helpers import frames_for, CASES, load_case, golden_params, golden_inputs, golden_rewards, HF_GRAD_KEYS, pick_grad
from oracle.ref_ops import RefOps
from oracle.text import FakeProcessor
from oracle import ref_model as RM
from oracle import ref_grpo as RG
import time_r1_amd  # noqa: F401
from time_r1_amd.config import tiny_test, tiny_test_25, PRESETS
from time_r1_amd.params import ModelParams, Arena, arena_specs, SEG_ALIGN
from time_r1_amd.trainer import TimeR1_Trainer, TimeR1_Trainer_ft, GRPOConfig
from time_r1_amd import rewards as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tower_hf_grads(cfg, get):
    """HF key -> this repo's slice of every tower tensor; get(name) returns the arena view (gradient or weight)."""
    v = cfg.vision
    out = {"model.visual.patch_embed.proj.weight": get("patch.w")[:, : v.patch_dim]}
    for i in range(v.depth):
        p, h = "v%d." % i, "model.visual.blocks.%d." % i
        pairs = [("n1.w", "norm1.weight"), ("n2.w", "norm2.weight"), ("qkv.w", "attn.qkv.weight"), ("qkv.b", "attn.qkv.bias"),
                 ("proj.w", "attn.proj.weight"), ("proj.b", "attn.proj.bias")]
        if v.variant == "qwen2_5_vl":
            i0, ip = v.mlp_dim, v.mlp_dim_padded
            gu, gb = get(p + "gu.w"), get(p + "gu.b")
            out[h + "mlp.gate_proj.weight"], out[h + "mlp.up_proj.weight"] = gu[:i0], gu[ip:ip + i0]
            out[h + "mlp.gate_proj.bias"], out[h + "mlp.up_proj.bias"] = gb[:i0], gb[ip:ip + i0]
            out[h + "mlp.down_proj.weight"], out[h + "mlp.down_proj.bias"] = get(p + "down.w")[:, :i0], get(p + "down.b")
        else:
            pairs += [("n1.b", "norm1.bias"), ("n2.b", "norm2.bias"), ("fc1.w", "mlp.fc1.weight"), ("fc1.b", "mlp.fc1.bias"),
                      ("fc2.w", "mlp.fc2.weight"), ("fc2.b", "mlp.fc2.bias")]
        for a, b in pairs:
            out[h + b] = get(p + a)
    return out


def golden_tower_norms(fx):
    return {k: v for k, v in fx["grad_norms"].items() if "visual.blocks" in k or "patch_embed" in k}


def tower_pads(cfg, get):
    """The pad regions of the tower (gradient or weights): patch.w columns >= patch_dim and Qwen2.5-VL's MLP width padding."""
    v = cfg.vision
    out = [get("patch.w")[:, v.patch_dim:]]
    if v.variant == "qwen2_5_vl" and v.mlp_dim_padded != v.mlp_dim:
        i0, ip = v.mlp_dim, v.mlp_dim_padded
        for i in range(v.depth):
            p = "v%d." % i
            out += [get(p + "gu.w")[i0:ip], get(p + "gu.w")[ip + i0:], get(p + "gu.b")[i0:ip], get(p + "gu.b")[ip + i0:], get(p + "down.w")[:, i0:]]
    return out


def tower_names(params):
    return [n for n in params.vit.names() if n == "patch.w" or n.startswith("v")]


def pads_zero(cfg, get):
    return all(float(t.abs().max()) == 0.0 for t in tower_pads(cfg, get))


# ------------------------------------------------------------------------------------------------------------ oracle vs the reference
@pytest.mark.parametrize("case", CASES)
def test_oracle_tower_gradients_match_reference_golden(case):
    """The oracle's autograd through the tower is the tensor-level yardstick of the tower gradients: pinned to the reference's norms."""
    fx = load_case(case)
    cfg, pol, ref = golden_params(RefOps(), fx)
    W = RM.weights_from_params(pol, requires_grad=True)
    for n in pol.frozen.names():
        W[n].requires_grad_(True)
    Wr = RM.weights_from_params(ref)
    pv, grid = golden_inputs(fx)
    rew, _ = golden_rewards(fx)
    out = RG.grpo_step(W, Wr, cfg, fx["prompt_ids"], pv, grid, fx["completion_ids"], rew, fx["beta"], fx["use_grpo"], rope_mode="hf5")
    out["loss"].backward()
    gold = golden_tower_norms(fx)
    mine = tower_hf_grads(cfg, lambda n: W[n].grad)
    assert set(mine) == set(gold) and len(gold) == (25 if cfg.vision.variant == "qwen2_vl" else 37)
    for k, g in gold.items():
        assert abs(float(mine[k].norm()) - g) <= 1e-4 * g, (k, float(mine[k].norm()), g)


# ------------------------------------------------------------------------------------------------------------ arena layout
@pytest.mark.parametrize("make", [tiny_test, tiny_test_25])
def test_train_vit_layout(make):
    cfg = make()
    ops = RefOps()
    a, b, c = ModelParams(cfg, ops), ModelParams(cfg, ops, train_vit=False), ModelParams(cfg, ops, train_vit=True)
    for x, y in ((a.train, b.train), (a.frozen, b.frozen)):
        assert x.offsets == y.offsets and x.segments == y.segments
    assert c.vit is c.train and a.vit is a.frozen and c.frozen.numel == 0 and c.frozen.names() == []
    for n in a.train.names():                          # LLM / merger offsets unchanged; the tower follows the merger, same order
        assert c.train.offsets[n] == a.train.offsets[n], n
    assert c.train.names() == a.train.names() + a.frozen.names()
    for n in a.train.names():                          # same weights by name (init_random draws in spec order)
        assert torch.equal(a.train.w(n), c.train.w(n)), n
    for n in a.frozen.names():
        assert torch.equal(a.frozen.w(n), c.train.w(n)), n
    t = c.train
    assert t.segments[0][1] == 0 and t.segments[-1][2] == t.numel
    assert all(s[2] == n[1] for s, n in zip(t.segments, t.segments[1:]))
    assert all(s[1] % SEG_ALIGN == 0 for s in t.segments) and len({s[0] for s in t.segments}) == len(t.segments)
    for world in (1, 2, 4, 8):
        cover = torch.zeros(t.numel, dtype=torch.int32)
        for r in range(world):
            loc = 0
            for ca, cb, la in t.chunks(r, world):
                assert la == loc and (cb - ca) % 64 == 0
                loc += cb - ca
                cover[ca:cb] += 1
            assert loc == t.numel // world
        assert bool((cover == 1).all())
    # relayout copies by name both ways; the HF export and the loaders agree across layouts
    d = a.relayout(True)
    assert d.train_vit and torch.equal(d.train.w16, c.train.w16) and torch.equal(d.train.master, c.train.master)
    e = c.relayout(False)
    assert torch.equal(e.train.w16, a.train.w16) and torch.equal(e.frozen.w16, a.frozen.w16)
    ea, ec = a.export_hf_state_dict(), c.export_hf_state_dict()
    assert ea.keys() == ec.keys() and all(torch.equal(ea[k], ec[k]) for k in ea)
    f = ModelParams(cfg, ops, init="none", train_vit=True)
    f.load_hf_state_dict(ea)
    assert torch.equal(f.train.w16, c.train.w16)


class _NoAlloc:
    act_dtype = torch.bfloat16

    def zeros(self, *shape, dtype=None):
        return torch.empty(0)


@pytest.mark.parametrize("name", ["qwen2-vl-7b", "qwen2.5-vl-7b"])
def test_train_vit_layout_at_7b_from_specs(name):
    """The 7B layouts compared from the spec lists (a CPU ModelParams at 7B would need over 100 GB)."""
    cfg = PRESETS[name]()
    trf, fzf = arena_specs(cfg, False)
    trv, fzv = arena_specs(cfg, True)
    A, F, V = Arena(_NoAlloc(), trf, False), Arena(_NoAlloc(), fzf, False), Arena(_NoAlloc(), trv, False)
    assert fzv == [] and [n for n, _ in trv] == [n for n, _ in trf + fzf]
    for n, (off, shape) in A.offsets.items():
        assert V.offsets[n] == (off, shape)
    assert V.segments[:len(A.segments)] == A.segments
    base = A.numel
    for n, (off, shape) in F.offsets.items():
        assert V.offsets[n] == (off + base, shape), n
    assert [(k, a + base, b + base) for k, a, b in F.segments] == V.segments[len(A.segments):]
    for world in (2, 4, 8):
        assert all((b - a) % (world * 64) == 0 for _, a, b in V.segments)


# ------------------------------------------------------------------------------------------------------------ the trainer
def make_vit_trainer(fx, fix_vit=False, cls=TimeR1_Trainer, ops=None, **over):
    ops = ops or RefOps()
    cfg, pol, ref = golden_params(ops, fx)
    args = GRPOConfig(output_dir="/tmp/tr1_vit_test", num_generations=fx["G"], max_completion_length=fx["C"], beta=fx["beta"], use_grpo=fx["use_grpo"],
                      rope_index_mode="hf5", temperature=1.0, logging_steps=1, save_strategy="no", fix_vit=fix_vit, **over)
    tr = cls(pol, [R.iou_timestamp_reward_v2, R.format_reward], list(R.metric_funcs_registry.values()), args=args, train_dataset=None,
             processing_class=FakeProcessor(cfg), ops=ops)
    if fx["beta"] != 0:
        tr.ref_model.w16.copy_(ref.relayout(tr.params.train_vit).train.w16)       # the captured reference tower IS the policy tower
    return cfg, tr


def golden_row(fx, tr):
    row = dict(fx["row"])
    row["_forced_completion_ids"] = fx["completion_ids"].numpy()
    tr._video_inputs = lambda ex: ([frames_for(fx)], [2.0])
    return row


@pytest.mark.parametrize("case", CASES)
def test_trainer_fix_vit_false_matches_reference_golden(case):
    fx = load_case(case)
    cfg, tr = make_vit_trainer(fx)
    assert tr.params.train_vit and tr.params.frozen.numel == 0
    loss = tr.compute_loss(tr.model, [golden_row(fx, tr)])
    assert abs(float(loss) - float(fx["loss"])) < 2e-5
    for k, v in fx["metrics"].items():
        assert abs(tr._metrics[k][0] - v[0]) < 5e-5, (k, tr._metrics[k], v)
    g = tr.params.train
    for hk, gold in fx["grads"].items():
        if hk in HF_GRAD_KEYS:
            mine = pick_grad(cfg, g.g, hk)
            assert torch.allclose(mine, gold, atol=2e-5 * max(1.0, gold.abs().max().item()), rtol=2e-3), hk
    gold = golden_tower_norms(fx)
    mine = tower_hf_grads(cfg, g.g)
    assert set(mine) == set(gold)
    for k, gn in gold.items():
        assert abs(float(mine[k].norm()) - gn) <= 1e-4 * gn, (k, float(mine[k].norm()), gn)
    assert pads_zero(cfg, g.g)
    # the LLM and merger gradients are those of a fix_vit=True run (same offsets: the tower follows the merger)
    _, tr0 = make_vit_trainer(fx, fix_vit=True, ops=RefOps())
    tr0.compute_loss(tr0.model, [golden_row(fx, tr0)])
    n0 = tr0.params.train.numel
    assert torch.equal(g.grad[:n0], tr0.params.train.grad)


def test_fix_vit_false_parses_from_the_command_line(monkeypatch):
    sys.path.insert(0, ROOT)
    import train_grpo
    assert GRPOConfig().fix_vit is True                      # the default stays
    seen = {}

    class Stop(Exception):
        pass

    def trainer(model=None, reward_funcs=None, metric_funcs=None, args=None, **kw):
        seen["args"] = args
        raise Stop()
    monkeypatch.setattr(train_grpo, "init_from_env", lambda *a, **k: None)
    monkeypatch.setattr(train_grpo, "load_json_dataset_tg", lambda *a, **k: [])
    monkeypatch.setattr(train_grpo, "TimeR1_Trainer", trainer)
    monkeypatch.setattr(sys, "argv", ["train_grpo.py", "--fix_vit", "false", "--model_name_or_path", "m", "--train_data_path", "d"])
    with pytest.raises(Stop):
        train_grpo.main()
    assert seen["args"].fix_vit is False


def test_ft_trainer_and_every_model_form_build_the_training_layout(tmp_path):
    fx = load_case("q25_grpo_beta")
    cfg, tr = make_vit_trainer(fx, cls=TimeR1_Trainer_ft)
    assert tr.params.train_vit and tr.ref_model.numel == tr.params.train.numel
    ops = RefOps()
    args = GRPOConfig(output_dir=str(tmp_path), fix_vit=False, save_strategy="no")
    assert TimeR1_Trainer(cfg, [R.format_reward], [], args=args, processing_class=FakeProcessor(cfg), ops=ops).params.train_vit
    tr.save_model(str(tmp_path / "m"))
    tr3 = TimeR1_Trainer(str(tmp_path / "m"), [R.format_reward], [], args=args, processing_class=FakeProcessor(cfg), ops=ops)
    assert tr3.params.train_vit and torch.equal(tr3.params.train.w16, tr.params.train.w16)


def test_preset_and_loaded_hf_module_build_the_training_layout(tmp_path):
    """The two model forms the test above leaves out: a preset name and a loaded transformers module (reference timer1_trainer.py:184-206)."""
    transformers = pytest.importorskip("transformers")
    from safetensors.torch import load_file
    ops = RefOps()
    args = GRPOConfig(output_dir=str(tmp_path), fix_vit=False, save_strategy="no", seed=3)
    cfg = PRESETS["tiny25"]()
    tr = TimeR1_Trainer("tiny25", [R.format_reward], [], args=args, processing_class=FakeProcessor(cfg), ops=ops)
    want = ModelParams(cfg, ops, seed=3, train_vit=True)
    assert tr.params.train_vit and tr.params.frozen.numel == 0 and torch.equal(tr.params.train.w16, want.train.w16)
    fx = load_case("grpo_beta")
    cfg, tr0 = make_vit_trainer(fx, fix_vit=True)
    d = str(tmp_path / "m")
    tr0.save_model(d)
    m = transformers.AutoModelForImageTextToText.from_config(transformers.AutoConfig.from_pretrained(d))
    m.load_state_dict({k: v.float() for k, v in load_file(os.path.join(d, "model.safetensors")).items()}, strict=True)
    tr2 = TimeR1_Trainer(m, [R.format_reward], [], args=args, processing_class=FakeProcessor(cfg), ops=ops)
    assert tr2.params.train_vit and tr2.params.frozen.numel == 0
    bf = lambda x: x.to(torch.bfloat16).float()          # save_model writes 16-bit weights
    assert torch.equal(bf(tr2.params.train.w16), bf(tr0.params.relayout(True).train.w16))


def test_two_optimizer_windows_update_the_tower_and_keep_pads_zero():
    fx = load_case("q25_grpo_beta")
    cfg, tr = make_vit_trainer(fx, learning_rate=1e-3, weight_decay=0.1)
    w0 = tr.params.train.w16.clone()
    t0 = tr.params.train.range_of("patch")[0]
    for _ in range(2):
        row = golden_row(fx, tr)
        full = {}
        step = tr.optimizer.step

        def grab(lr=None):
            full["n"] = float(tr.params.train.grad.norm())
            return step(lr=lr)
        tr.optimizer.step = grab
        gn = tr.optimizer_window([[row]])
        del tr.optimizer.step
        assert abs(float(gn) - full["n"]) <= 1e-4 * full["n"]        # the clipping norm covers the tower's gradients (fp32 sums in another order)
    init = ModelParams(cfg, RefOps(), init="none", train_vit=True)
    init.train.w16.copy_(w0)
    for n in tower_names(tr.params):
        assert not torch.equal(tr.params.vit.w(n), init.train.w(n)), n
    assert pads_zero(cfg, tr.params.vit.w)
    assert torch.equal(tr.ref_model.w16[t0:], w0[t0:])          # the reference tower stays at the initial weights


# ------------------------------------------------------------------------------------------------------------ data parallel / resume
def _worker_vit(rank, world, port, q, shard):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from test_dp_gloo import _rows
    from test_vit_train_host import make_vit_trainer
    fx = load_case("grpo_beta")
    cfg, tr = make_vit_trainer(fx, grad_wire_dtype="fp32", shard_optimizer=shard)
    tr._video_inputs = lambda ex: ([ex["_frames"]], [2.0])
    tr.args.learning_rate = 1e-3
    a = tr.params.train
    norms = []
    for step in range(2):
        row = _rows(fx)[rank]
        row["_forced_completion_ids"] = (row["_forced_completion_ids"] + 5 * step) % 480 + 2
        tr.accumulation_window([[row]])
        norms.append(float(tr.optimizer.step()))
    q.put((rank, a.w16.float().numpy().copy(), norms))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_equals_replicated_with_fix_vit_false():
    from test_dp_gloo import _spawn2
    sharded = _spawn2(_worker_vit, True)
    plain = _spawn2(_worker_vit, False)
    assert torch.equal(sharded[0][1], sharded[1][1]) and torch.equal(plain[0][1], plain[1][1])
    assert abs(sharded[0][2][0] - plain[0][2][0]) < 1e-5 * max(1.0, plain[0][2][0])
    assert torch.allclose(sharded[0][1].float(), plain[0][1].float(), atol=1e-6, rtol=1e-5)


def test_resume_equals_straight_run_with_fix_vit_false(tmp_path):
    from test_trainer_host_logic import _dataset
    fx = load_case("grpo_beta")

    def run(out, max_steps, ckpt=None):
        cfg, tr = make_vit_trainer(fx, gradient_accumulation_steps=2)
        tr.args.output_dir = str(out)
        tr.args.num_train_epochs = 1
        tr.args.max_steps = max_steps
        tr.args.save_strategy = "steps"
        tr.args.save_steps = 1
        tr.args.learning_rate = 1e-4
        tr.train_dataset = _dataset(fx, 4)
        tr.train(resume_from_checkpoint=ckpt)
        return tr
    straight = run(tmp_path / "a", 2)
    run(tmp_path / "b", 1)
    resumed = run(tmp_path / "b", 2, ckpt=str(tmp_path / "b" / "checkpoint-1"))
    assert torch.equal(resumed.params.train.w16, straight.params.train.w16)
    assert torch.equal(resumed.ref_model.w16, straight.ref_model.w16)
