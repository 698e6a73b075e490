"""fix_vit=False on the HIP path: the two new kernels (QuickGELU backward, padded-head unpad), the tower backward on the padded heads
against the oracle's fp32 autograd (the project's bf16-vs-fp32 bound: 6 % relative L2 per tensor), and the trainer on the golden cases."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from helpers import frames_for, CASES, load_case, golden_params, HF_GRAD_KEYS, pick_grad  # noqa: E402
from test_vit_train_host import tower_hf_grads, golden_tower_norms, pads_zero, golden_row, tower_names  # noqa: E402


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def test_quickgelu_bwd_within_one_ulp(hip_ops):
    ops = hip_ops
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64 * 1024, generator=g) * 4
    x[:16] = torch.tensor([-300., -90., -40., -12., -3., -1e-3, -0., 0., 1e-3, 3., 12., 40., 90., 300., 1e4, -1e4])
    dy = torch.randn(x.shape, generator=g)
    xb, dyb = x.to(torch.bfloat16), dy.to(torch.bfloat16)
    got = ops.quickgelu_bwd(xb.to(ops.device), dyb.to(ops.device)).float().cpu()
    v = xb.double()
    s = torch.sigmoid(1.702 * v)
    want = (dyb.double() * (s + 1.702 * v * s * (1 - s))).float()
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp(min=1e-30))) - 7)
    assert bool(torch.isfinite(got).all())
    assert bool(((got - want).abs() <= ulp).all()), float(((got - want).abs() / ulp).max())


@pytest.mark.parametrize("half,hoff", [(40, 48), (32, 48), (40, 64), (56, 64)])
@pytest.mark.parametrize("rotate", [False, True])
def test_heads_unpad_bit_identical_to_compact_plus_rope_backward(hip_ops, half, hoff, rotate):
    ops = hip_ops
    T, H, hd = 301, 4, 2 * half
    g = torch.Generator().manual_seed(half + hoff)
    x = torch.zeros(T, H, 128)
    x[:, :, :half] = torch.randn(T, H, half, generator=g)
    x[:, :, hoff:hoff + half] = torch.randn(T, H, half, generator=g)
    x128 = x.reshape(T, H * 128).to(torch.bfloat16).to(ops.device)
    ang = torch.rand(T, half, generator=g) * 50
    cos, sin = ang.cos().to(ops.device), ang.sin().to(ops.device)
    v = x128.view(T, H, 128)
    comp = torch.cat([v[:, :, :half], v[:, :, hoff:hoff + half]], -1).reshape(T, H * hd).contiguous()
    want = ops.rope_apply(comp, H, hd, cos, sin, backward=True) if rotate else comp
    W = 3 * H * hd + 64
    buf = ops.zeros(T, W)
    out = buf[:, H * hd:2 * H * hd]                      # a column view with ld = W
    ops.vit_heads_unpad(x128, H, half, hoff, out, *((cos, sin) if rotate else (None, None)))
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))
    assert float(buf[:, :H * hd].abs().max()) == 0.0 and float(buf[:, 2 * H * hd:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ the tower backward
def _tower(ops, variant, E, H, grid, depth=2):
    import time_r1_amd  # noqa: F401
    from time_r1_amd.config import tiny_test, tiny_test_25, VisionConfig
    from time_r1_amd.params import ModelParams
    from time_r1_amd.model import Engine
    q25 = variant == "qwen2_5_vl"
    cfg = tiny_test_25() if q25 else tiny_test()
    cfg.vision = VisionConfig(depth=depth, embed_dim=E, num_heads=H, mlp_dim=(E * 3420 // 1280) if q25 else 4 * E, out_hidden=128, variant=variant,
                              **({"window_size": 112, "fullatt_block_indexes": (1,)} if q25 else {}))
    params = ModelParams(cfg, ops, seed=5, train_vit=True)
    return cfg, params, Engine(cfg, ops, params)


def _pixels(ops, v, grid, seed=3):
    n = sum(t * h * w for t, h, w in grid)
    pix = torch.randn(n, v.patch_dim, generator=torch.Generator().manual_seed(seed))
    pp = ops.zeros(n, v.patch_dim_padded)
    pp[:, : v.patch_dim] = pix.to(pp.device).to(pp.dtype)
    return pp


def _merger_ref(cfg, W, feats, perm):
    """The merger on given features (window order for Qwen2.5-VL), output rows in natural order: the oracle's dfeats."""
    v = cfg.vision
    N, E = feats.shape
    if v.variant == "qwen2_5_vl":
        y = W["merger.ln.w"] * (feats * torch.rsqrt(feats.pow(2).mean(-1, keepdim=True) + v.ln_eps))
    else:
        y = F.layer_norm(feats, (E,), W["merger.ln.w"], W["merger.ln.b"], v.ln_eps)
    y = F.gelu(y.reshape(N // v.merge_unit, E * v.merge_unit) @ W["merger.fc1.w"].t() + W["merger.fc1.b"])
    out = y @ W["merger.fc2.w"].t() + W["merger.fc2.b"]
    if perm is not None:
        out = torch.zeros_like(out).index_copy(0, perm.long().to(out.device), out)
    return out


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp(min=1e-20))


def _tower_grads_vs_oracle(ops, cfg, params, eng, grid, tol=0.06):
    from oracle import ref_model as RM
    v = cfg.vision
    pp = _pixels(ops, v, grid)
    feats0, _ = eng.vit_features(pp, grid)
    feats, perm, ctx = eng.vit_features(pp, grid, save=True)
    assert torch.equal(_bits(feats), _bits(feats0)), "save mode must not change the features"
    out, mctx = eng.merger_fwd(params.train, feats, save=True, perm=perm)
    R = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)) * 0.05
    params.train.grad.zero_()
    dfeats = eng.merger_bwd(mctx, R.to(ops.device).to(torch.bfloat16))
    eng.vit_bwd(ctx, dfeats)
    torch.cuda.synchronize()
    W = RM.weights_from_params(params, requires_grad=True)
    want = RM.vision_tower(W, cfg, pp[:, : v.patch_dim].float().cpu(), grid)
    (want * R.to(torch.bfloat16).float()).sum().backward()
    errs = {}
    for n in tower_names(params):
        errs[n] = _rel(params.train.g(n).cpu(), W[n].grad)
    fl = feats.float().cpu().requires_grad_(True)
    Wd = {k: t.detach() for k, t in W.items()}
    (_merger_ref(cfg, Wd, fl, perm) * R.to(torch.bfloat16).float()).sum().backward()
    errs["dfeats"] = _rel(dfeats.cpu(), fl.grad)
    bad = {k: e for k, e in errs.items() if not e < tol}
    assert not bad, bad
    assert pads_zero(cfg, params.train.g)
    return errs


@pytest.mark.parametrize("variant", ["qwen2_vl", "qwen2_5_vl"])
@pytest.mark.parametrize("E,H", [(256, 4), (1280, 16)])
def test_tower_backward_on_padded_heads_matches_oracle(hip_ops, variant, E, H):
    cfg, params, eng = _tower(hip_ops, variant, E, H, [(2, 8, 12)])
    assert hip_ops.vit_pad128_ok(H, cfg.vision.head_dim) and eng._vit_pad128(2 * 8 * 12) is not None
    _tower_grads_vs_oracle(hip_ops, cfg, params, eng, [(2, 8, 12)])


@pytest.mark.parametrize("variant", ["qwen2_vl", "qwen2_5_vl"])
def test_tower_backward_at_full_size(hip_ops, variant):
    """Config-3 geometry (grid 16 x 22 x 38, N_v = 13 376), 2 blocks of the real width, padded heads: every tower gradient and dfeats within 6 % of the
    oracle's fp32 autograd.  The oracle's dense [heads, N, N] attention (~12 GB per block) runs on the device here (torch as the checker)."""
    from oracle import ref_model as RM
    ops = hip_ops
    grid = [(16, 22, 38)]
    cfg, params, eng = _tower(ops, variant, 1280, 16, grid)
    v = cfg.vision
    pp = _pixels(ops, v, grid)
    assert pp.shape[0] == 13376 and eng._vit_pad128(pp.shape[0]) is not None
    feats, perm, ctx = eng.vit_features(pp, grid, save=True)
    out, mctx = eng.merger_fwd(params.train, feats, save=True, perm=perm)
    R = (torch.randn(out.shape, generator=torch.Generator().manual_seed(7)) * 0.05).to(torch.bfloat16).to(ops.device)
    params.train.grad.zero_()
    dfeats = eng.merger_bwd(mctx, R)
    eng.vit_bwd(ctx, dfeats)
    torch.cuda.synchronize()
    del ctx, mctx
    names = tower_names(params)
    with torch.device(ops.device):
        W = {n: params.train.w(n).detach().float().clone().requires_grad_(n in names) for n in params.train.names()}
        want = RM.vision_tower(W, cfg, pp[:, : v.patch_dim].float(), grid)
        (want * R.float()).sum().backward()
        del want
        errs = {n: _rel(params.train.g(n), W[n].grad) for n in names}
        fl = feats.detach().float().requires_grad_(True)
        Wd = {k: t.detach() for k, t in W.items()}
        (_merger_ref(cfg, Wd, fl, perm) * R.float()).sum().backward()
        errs["dfeats"] = _rel(dfeats, fl.grad)
    bad = {k: e for k, e in errs.items() if not e < 0.06}
    assert not bad, bad
    assert pads_zero(cfg, params.train.g)


@pytest.mark.parametrize("variant", ["qwen2_vl", "qwen2_5_vl"])
def test_padded_tower_follows_the_optimizer_step(hip_ops, variant):
    """The stale-cache check on the padded path every real config takes: GRPOCore + AdamWFlat over two windows on a tower of 4 heads of 64 on 128-wide
    padded heads.  The padded proj weights are derived once per weight version and the optimizer rewrites the weights through HIP kernels torch never
    sees, so the cache key carries Arena.version.  Second window: the policy features equal a fresh engine's (no cache) bit for bit and the oracle's at
    the updated weights; the reference tower (its own cache entry) still gives the first window's features, bit for bit."""
    from oracle import ref_model as RM
    from time_r1_amd.grpo import GRPOCore, eos_mask, group_advantages
    from time_r1_amd.model import Engine
    from time_r1_amd.optim import AdamWFlat
    from time_r1_amd.synthetic import synthetic_prompt
    ops = hip_ops
    g3 = (2, 8, 12)
    cfg, params, eng = _tower(ops, variant, 256, 4, [g3])
    v = cfg.vision
    N = g3[0] * g3[1] * g3[2]
    G, C = 4, 6
    core = GRPOCore(eng, params.train.clone_weights_only(), G, C, beta=0.04, use_grpo=True, seed=3, rope_index_mode="hf4")
    opt = AdamWFlat(params, ops, lr=1e-3)
    ids, pix, grid = synthetic_prompt(cfg, g3, 9, 7, seed=2, text_vocab=400)
    first = None
    for w in range(2):
        st = core.prepare(ids, pix, grid)
        assert eng._vit_pad128(N) is not None
        if w == 0:
            first = st.feats.clone()
        else:
            fresh, _ = Engine(cfg, ops, params).vit_features(st.pixels, st.grid)
            assert not torch.equal(_bits(st.feats), _bits(first)), "the tower did not move"
            assert torch.equal(_bits(st.feats), _bits(fresh)), "the policy tower ran on stale padded proj weights"
            got, _ = eng.merger_fwd(params.train, st.feats, save=False, perm=st.vis_perm)
            want = RM.vision_tower(RM.weights_from_params(params), cfg, st.pixels[:, : v.patch_dim].float().cpu(), st.grid)
            assert _rel(got.cpu(), want) < 0.03
            ref_feats, _ = eng.vit_features(st.pixels, st.grid, arena=core.ref_arena)
            assert torch.equal(_bits(ref_feats), _bits(first)), "the reference tower must keep the initial weights"
        core.rollout(st)
        core.forward_logps(st)
        mask = torch.tensor(eos_mask(st.completion_ids.cpu().numpy(), cfg.eos_token_id))
        _, adv, _ = group_advantages(torch.rand(G, 2, generator=torch.Generator().manual_seed(5 + w)), G)
        core.loss_backward(st, mask.to(ops.device), adv.to(ops.device), 1.0)
        opt.step()
    torch.cuda.synchronize()
    assert pads_zero(cfg, params.train.w)


# ------------------------------------------------------------------------------------------------------------ the trainer
def _make(fx, ops, fix_vit):
    import time_r1_amd  # noqa: F401
    from time_r1_amd.trainer import TimeR1_Trainer, GRPOConfig
    from time_r1_amd import rewards as R
    from oracle.text import FakeProcessor
    cfg, pol, ref = golden_params(ops, fx)
    args = GRPOConfig(output_dir="/tmp/tr1_gpu_vit", num_generations=fx["G"], max_completion_length=fx["C"], beta=fx["beta"], use_grpo=fx["use_grpo"],
                      rope_index_mode="hf5", temperature=1.0, save_strategy="no", fix_vit=fix_vit)
    tr = TimeR1_Trainer(pol, [R.iou_timestamp_reward_v2, R.format_reward], [], args=args, processing_class=FakeProcessor(cfg), ops=ops)
    if fx["beta"] != 0:
        tr.ref_model.w16.copy_(ref.relayout(tr.params.train_vit).train.w16)
    return cfg, tr


@pytest.mark.parametrize("case", CASES)
def test_hip_trainer_fix_vit_false_vs_reference_golden(hip_ops, case):
    fx = load_case(case)
    cfg, tr = _make(fx, hip_ops, False)
    loss = tr.compute_loss(tr.model, [golden_row(fx, tr)])
    assert abs(float(loss) - float(fx["loss"])) < 5e-3
    for k, v in fx["metrics"].items():
        tol = 5e-3 if k in ("kl",) else (0.05 if k == "generation_entropy" else 1e-6)
        assert abs(tr._metrics[k][0] - v[0]) <= tol, (k, tr._metrics[k], v)
    g = tr.params.train
    for hk, gold in fx["grads"].items():
        if hk in HF_GRAD_KEYS:
            assert _rel(pick_grad(cfg, g.g, hk).cpu(), gold) < 0.06, hk
    gold = golden_tower_norms(fx)
    mine = tower_hf_grads(cfg, g.g)
    bad = {k: (float(mine[k].norm()), gn) for k, gn in gold.items() if not abs(float(mine[k].norm()) - gn) <= 0.06 * gn}
    assert not bad, bad
    assert pads_zero(cfg, g.g)
    # LLM and merger gradients: bit-identical to the fix_vit=True run
    _, tr0 = _make(fx, hip_ops, True)
    tr0.compute_loss(tr0.model, [golden_row(fx, tr0)])
    n0 = tr0.params.train.numel
    assert torch.equal(g.grad[:n0].cpu(), tr0.params.train.grad.cpu())


@pytest.mark.parametrize("case", ["grpo_beta", "q25_grpo_beta"])
def test_two_trainer_windows_update_the_tower(hip_ops, case):
    """Two optimizer windows of the trainer on the golden cases (their 64-wide towers take the unpadded path; the padded path's cache is checked by
    test_padded_tower_follows_the_optimizer_step): the tower's master weights move, pads stay zero, the returned norm is the whole gradient arena's,
    the second window's features follow the updated weights, and with beta != 0 the reference log-probs keep the initial tower."""
    from oracle import ref_model as RM
    fx = load_case(case)
    cfg, tr = _make(fx, hip_ops, False)
    tr.args.learning_rate = 1e-3
    v = cfg.vision
    w0 = tr.params.train.w16.clone()
    a = tr.params.train
    init = {n: a.view(a.master, n).clone() for n in tower_names(tr.params)}      # fp32 master: a step of 1e-3 moves no bf16 norm weight of 1.0
    for step in range(2):
        row = golden_row(fx, tr)
        full = {}
        orig = tr.optimizer.step

        def grab(lr=None):
            full["n"] = float(tr.params.train.grad.norm())
            return orig(lr=lr)
        tr.optimizer.step = grab
        gn = tr.optimizer_window([[row]])
        del tr.optimizer.step
        assert abs(float(gn) - full["n"]) <= 1e-3 * full["n"], (float(gn), full["n"])
        if step == 0:
            continue
        # second window's features (policy tower at the weights after step 1) against the oracle tower at those weights
        st = tr.core.prepare(fx["prompt_ids"], *_golden_pixels(fx))
        got, _ = tr.engine.merger_fwd(tr.params.train, st.feats, save=False, perm=st.vis_perm)
        want = RM.vision_tower(RM.weights_from_params(tr.params), cfg, st.pixels[:, : v.patch_dim].float().cpu(), st.grid)
        assert _rel(got.cpu(), want) < 0.03
    if fx["beta"] != 0:          # the reference log-probs after two updates: those of a fresh trainer at the initial weights, bit for bit
        _, fresh = _make(fx, hip_ops, False)
        assert torch.equal(_ref_logp(tr, fx), _ref_logp(fresh, fx))
    for n, t in init.items():
        assert not torch.equal(a.view(a.master, n), t), n
    assert pads_zero(cfg, tr.params.vit.w)
    t0 = tr.params.train.range_of("patch")[0]
    assert torch.equal(tr.ref_model.w16[t0:], w0[t0:])


def _golden_pixels(fx):
    from helpers import golden_inputs
    pv, grid = golden_inputs(fx)
    return pv, grid


def _ref_logp(tr, fx):
    import numpy as np
    from time_r1_amd.positions import PackedLayout
    st = tr.core.prepare(fx["prompt_ids"], *_golden_pixels(fx))
    st.layout = PackedLayout(st.P, fx["G"], fx["C"])
    st.completion_ids = tr.ops.tensor(np.asarray(fx["completion_ids"].numpy(), dtype=np.int32), torch.int32)
    tr.core.forward_logps(st)
    return st.ref_logp.float().cpu()
