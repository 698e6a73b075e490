"""The entropy options of the GRPO objective on the MI355X: tr1_logp_entropy_bwd and tr1_entropy_quantile_weight against the fp64 references of
tests/entropy_cases.py, the head's backward with a gradient at the entropy (materialised and chunked), GRPOCore's token selection, the torch op under autograd
and the trainer on HipOps.  Every check prints the worst error it saw (`pytest -s`).

Worst seen on MI355X: logp_entropy_bwd 0.327 of TOL_DLOGITS over the 17 cases (6.7e-3 absolute), the pairing test 0.322, the torch op
0.251; head gradients 0.016 relative L2 with dent against 0.005 for dlogp alone (bound 0.06); no token left out of any selection comparison; the logged-loss
identity to 6.9e-7 (bound 1e-5)."""
import pytest
import torch

import entropy_cases as ec
import vocab_cases as vc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
I32 = torch.int32
DEV = "cuda:0"


def bits(t):
    return t.contiguous().view(torch.int16)


def share(got, ref, tol, what):
    ratio, err = vc.worst(got, ref, tol)
    print("OBS %-62s max err %.3e  (%.3f of atol %g + rtol %g |ref|)" % (what, err, ratio, tol[0], tol[1]))
    assert ratio <= 1.0, "%s: max err %.4g is %.3g x the tolerance (atol %g, rtol %g)" % (what, err, ratio, tol[0], tol[1])
    return ratio


# ------------------------------------------------------------------------------------------------------------ A. logp_entropy_bwd
# TOL_DLOGITS = atol 1e-3, rtol 1e-2: fp32 arithmetic ahead of ONE rounding to bf16 (2^-9 relative) against rtol 1e-2.
@pytest.mark.parametrize("name,kw", vc.bwd_cases(), ids=[c[0] for c in vc.bwd_cases()])
def test_logp_entropy_bwd(hip_ops, name, kw):
    store, x, tg, kinds = vc.stat_rows(**kw)
    R, V, col0 = kw["R"], kw["V"], kw.get("col0", 0)
    dlogp, dent = vc.bwd_dlogp(R, kw["seed"]), ec.bwd_dent(R, kw["seed"])
    stats = vc.ref_stats(x, tg)
    ref = ec.ref_dlogits_ent(x, tg, dlogp, dent, stats)
    store_d = store.to(DEV)
    view = store_d[:, col0:col0 + V]
    tg_d, lse_d, ent_d, dlogp_d, dent_d = tg.to(DEV), stats[2].float().to(DEV), stats[1].float().to(DEV), dlogp.to(DEV), dent.to(DEV)
    out = hip_ops.logp_entropy_bwd(view, tg_d, lse_d, ent_d, dlogp_d, dent_d, inplace=False)
    assert out.data_ptr() != view.data_ptr()
    if store.shape[1] != V:
        assert out.stride(0) != view.stride(0), "this case runs ld_out != ld"
    assert torch.equal(store_d.cpu().view(torch.int16), store.view(torch.int16)), "inplace=False leaves the logits alone"
    share(out, ref, vc.TOL_DLOGITS, "ent bwd %s dlogits" % name)
    # the contracts with tr1_logp_bwd (out of place, on the untouched logits)
    plain = hip_ops.logp_bwd(view, tg_d, lse_d, dlogp_d, inplace=False)
    null = hip_ops.logp_entropy_bwd(view, tg_d, lse_d, ent_d, dlogp_d, None, inplace=False)
    assert torch.equal(bits(null), bits(plain)), "a null dent is tr1_logp_bwd, bit for bit"
    o, p = out.float().cpu(), plain.float().cpu()
    z_ent, z_lp = dent == 0, dlogp == 0
    assert bool((o[z_ent] == p[z_ent]).all()), "rows with dent == 0 equal tr1_logp_bwd's rows in value"
    assert bool((o[z_ent & z_lp] == 0).all()), "dlogp == 0 and dent == 0 must give exactly 0"
    if R >= 24:
        assert bool(z_ent.any()) and bool((z_ent & z_lp).any()) and bool((z_lp & ~z_ent).any())
        live = ~z_ent
        assert float((o[live] - p[live]).abs().max()) > 1e-3, "the entropy term is there"
    # in place (the only form the engine uses): bit-equal to the out-of-place result, nothing outside the view touched
    same = hip_ops.logp_entropy_bwd(view, tg_d, lse_d, ent_d, dlogp_d, dent_d, inplace=True)
    assert same.data_ptr() == view.data_ptr()
    assert torch.equal(bits(same), bits(out)), "in-place and out-of-place results differ"
    after = store_d.cpu()
    outside = torch.ones(store.shape[1], dtype=torch.bool)
    outside[col0:col0 + V] = False
    assert torch.equal(after[:, outside].view(torch.int16), store[:, outside].view(torch.int16)), "wrote outside the [R, V] view"


def test_logp_entropy_bwd_refuses_V_not_multiple_of_8(hip_ops):
    from time_r1_amd.hip import HipError
    for V in (1001, 2047):
        store, x, tg, _ = vc.stat_rows(R=3, V=V, seed=5)
        view = store.to(DEV)[:, :V]
        z, o = torch.zeros(3, device=DEV), torch.ones(3, device=DEV)
        with pytest.raises(HipError):
            hip_ops.logp_entropy_bwd(view, tg.to(DEV), z, o, o, o, inplace=False)
        with pytest.raises(HipError):
            hip_ops.logp_entropy_bwd(view, tg.to(DEV), z, o, o, None, inplace=False)


def test_logp_entropy_bwd_pairs_fused_lse_with_recomputed_logits(hip_ops):
    """The chunked backward of the head: LSE AND entropy from the fused lm_head forward, a chunk's logits recomputed by gemm_nt, the backward in place on them."""
    M, V, K = 257, 33024, 192
    hn, w, tg, logits, _ = vc.lmhead_case(M, V, K)
    dlogp, dent = vc.bwd_dlogp(M, 17), ec.bwd_dent(M, 17)
    hn_d, w_d, tg_d, dlogp_d, dent_d = hn.to(DEV), w.to(DEV), tg.to(DEV), dlogp.to(DEV), dent.to(DEV)
    _, ent, lse = hip_ops.lmhead_lse(hn_d, w_d, tg_d)
    for a, b in ((0, 128), (128, M)):
        lg = hip_ops.gemm_nt(hn_d[a:b], w_d)
        lg_before = lg.clone()
        dl = hip_ops.logp_entropy_bwd(lg, tg_d[a:b].contiguous(), lse[a:b].contiguous(), ent[a:b].contiguous(), dlogp_d[a:b].contiguous(),
                                      dent_d[a:b].contiguous(), inplace=True)
        assert dl.data_ptr() == lg.data_ptr()
        ref = ec.ref_dlogits_ent(lg_before.cpu(), tg[a:b], dlogp[a:b], dent[a:b])
        share(dl, ref, vc.TOL_DLOGITS, "ent bwd pairing rows %d..%d" % (a, b))


# ------------------------------------------------------------------------------------------------------------ B. entropy_quantile_weight
@pytest.mark.parametrize("G,C", ec.QUANTILE_SHAPES)
def test_entropy_quantile_weight(hip_ops, G, C):
    """Every mask (vc.grpo_case's, with two empty rows, all masked) x both entropy sets (uniform; half zeros with -1e-7 and -0.0) x every rho; NaN at the masked
    positions: the selection equals the fp64 reference's, stats3 = (threshold, kept, live), a second call gives the same bits."""
    left = 0
    for mname, mask in ec.quantile_masks(G, C).items():
        for kind in ("uniform", "zeros"):
            ent = ec.quantile_entropies(mask, kind)
            ent_d, mask_d = ent.to(DEV), mask.to(DEV)
            for rho in ec.RHOS:
                w, st = hip_ops.entropy_quantile_weight(ent_d, mask_d, rho)
                w2, st2 = hip_ops.entropy_quantile_weight(ent_d, mask_d, rho)
                assert w.shape == ent.shape and w.dtype == torch.float32
                assert torch.equal(w.view(I32), w2.view(I32)) and torch.equal(st.view(I32), st2.view(I32)), "two calls, two results"
                n = ec.compare_quantile(w, st, ent, mask, rho, (G, C, mname, kind, rho))
                if kind == "uniform":
                    assert n == 0, "uniform entropies: fp32 order statistics reproduce the fp64 mask with none left out"
                left += n
                if mname == "none":
                    assert bool((w == 0).all()) and bool((st == 0).all())
    print("OBS quantile G=%d C=%d: %d tokens near a threshold left out" % (G, C, left))


def test_entropy_quantile_weight_refuses_bad_arguments(hip_ops):
    from time_r1_amd.hip import HipError
    e, m = torch.zeros(2, 8, device=DEV), torch.ones(2, 8, dtype=I32, device=DEV)
    for rho in (0.0, -0.5, 1.5):
        with pytest.raises(HipError):
            hip_ops.entropy_quantile_weight(e, m, rho)
    n = (1 << 20) + 8
    with pytest.raises(HipError):
        hip_ops.entropy_quantile_weight(torch.zeros(1, n, device=DEV), torch.ones(1, n, dtype=I32, device=DEV), 0.5)


# ------------------------------------------------------------------------------------------------------------ C. torch op under autograd
def test_entropy_gradient_through_the_torch_op(hip_ops):
    """d ent.sum() and d (lp a + ent b).sum() / d logits through T.logp_entropy against autograd of log_softmax on the fp32 logits, TOL_DLOGITS."""
    import time_r1_amd.torch_ops as T
    R, V = 37, 2048
    _, x, tg, _ = vc.stat_rows(R=R, V=V, seed=21)
    a, b = vc.bwd_dlogp(R, 21).to(DEV), ec.bwd_dent(R, 21).to(DEV)
    for what, f in (("ent.sum()", lambda lp, ent: ent.sum()), ("(lp a + ent b).sum()", lambda lp, ent: (lp * a + ent * b).sum())):
        lg = x.contiguous().to(DEV).requires_grad_(True)
        f(*T.logp_entropy(lg, tg.to(DEV))).backward()
        lf = x.float().to(DEV).requires_grad_(True)
        ls = torch.log_softmax(lf, -1)
        f(ls.gather(1, tg.to(DEV).long()[:, None])[:, 0], -(ls.exp() * ls).sum(-1)).backward()
        assert lg.grad.dtype == BF16 and float(lf.grad.abs().max()) > 0.05
        share(lg.grad, lf.grad, vc.TOL_DLOGITS, "torch op: d %s / d logits" % what)
    # a graph that never uses the entropy still runs logp_bwd
    x_d, tg_d = x.contiguous().to(DEV), tg.to(DEV)
    lg = x_d.clone().requires_grad_(True)
    lp, _ = T.logp_entropy(lg, tg_d)
    (lp * a).sum().backward()
    lse = hip_ops.logp_entropy_fwd(x_d, tg_d)[2]
    assert torch.equal(bits(lg.grad), bits(hip_ops.logp_bwd(x_d, tg_d, lse, a, inplace=False)))


# ------------------------------------------------------------------------------------------------------------ D. head_fwd + head_bwd(dent)
G_, C_, HID, V_ = 3, 50, 128, 2048


def _head_setup(hip_ops):
    from time_r1_amd.config import tiny_test
    from time_r1_amd.model import Engine
    from time_r1_amd.params import ModelParams
    cfg = tiny_test(vocab=V_)
    params = ModelParams(cfg, hip_ops, seed=3)
    w = params.lm_head_w()
    w.copy_((w.float() * 12.0).to(BF16))            # logits of standard deviation ~3: a distribution whose entropy has a gradient worth the name
    eng = Engine(cfg, hip_ops, params)
    g = torch.Generator().manual_seed(5)
    P, R = 9, G_ * C_
    M = P + R
    h_last = torch.randn(M, HID, generator=g).to(BF16)
    # the packed layout's prediction rows: the last prompt row G times, then every completion row but each completion's last
    rest = torch.cat([P + gi * C_ + torch.arange(C_ - 1) for gi in range(G_)])
    pred = torch.cat([torch.full((G_,), P - 1), rest]).to(I32)
    tg = torch.randint(0, V_, (R,), generator=g).to(I32)
    return cfg, params, eng, h_last, pred, tg


def _head_reference(cfg, params, h_last, pred, tg, dlogp, dent):
    """fp64 autograd of gather -> RMSNorm -> lm_head -> (logp, H), loss = sum dlogp logp + sum dent H -> (dh, d lm_head, d norm weight)."""
    h = h_last.double().clone().requires_grad_(True)
    W = params.lm_head_w().double().cpu().clone().requires_grad_(True)
    nw = params.train.w("norm").double().cpu().clone().requires_grad_(True)
    hp = h[pred.long()]
    hn = nw * (hp * torch.rsqrt(hp.pow(2).mean(-1, keepdim=True) + cfg.text.rms_eps))
    ls = torch.log_softmax(hn @ W.t(), -1)
    lp = ls.gather(1, tg.long()[:, None])[:, 0]
    H = -(ls.exp() * ls).sum(-1)
    (lp * dlogp.double() + H * dent.double()).sum().backward()
    return h.grad, W.grad, nw.grad


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


@pytest.mark.parametrize("chunk", [4096, 64], ids=["materialised", "chunks-64-64-22"])
def test_head_backward_with_an_entropy_gradient(hip_ops, chunk):
    """dh, the lm_head gradient and the final-norm gradient of head_fwd + head_bwd(dent) against fp64 autograd, within the 6 % relative L2 that
    tests/test_trainer_gpu.py holds bf16 gradients to; the dlogp-only call of the same test beside it.  chunk = 64: the fused forward (no logits kept) and the
    recompute branch over chunks of 64, 64 and 22 rows."""
    cfg, params, eng, h_last, pred, tg = _head_setup(hip_ops)
    eng.HEAD_CHUNK_ROWS = chunk
    R = G_ * C_
    dlogp, dent, zero = vc.bwd_dlogp(R, 31) * 0.1, ec.bwd_dent(R, 31), torch.zeros(R)
    tr = params.train
    for what, dl, de in (("dlogp only", dlogp, None), ("dent only", zero, dent), ("dlogp and dent", dlogp, dent)):
        tr.grad.zero_()
        logp, ent, ctx = eng.head_fwd(tr, h_last.to(DEV), pred.to(DEV), tg.to(DEV), save=True)
        assert (ctx["logits"] is None) == (chunk < R) and ctx["ent"] is ent
        dh = eng.head_bwd(ctx, dl.to(DEV), G_, dent=None if de is None else de.to(DEV))
        ref = _head_reference(cfg, params, h_last, pred, tg, dl, zero if de is None else de)
        errs = [rel_l2(dh, ref[0]), rel_l2(params.lm_head_g(), ref[1]), rel_l2(tr.g("norm"), ref[2])]
        print("OBS head %-14s %-16s rel L2: dh %.4f  lm_head %.4f  norm %.4f" % ("chunk %d" % chunk, what, *errs))
        for name, e in zip(("dh", "lm_head", "norm"), errs):
            assert e < 0.06, (what, name, e)
        assert float(ent.min()) > 0.5, "the rows must have an entropy to differentiate"


# ------------------------------------------------------------------------------------------------------------ E. GRPOCore: the selection is a tok_weight
@pytest.mark.parametrize("path", ["clip", "use_grpo", "objective"])
def test_core_selection_equals_an_explicit_tok_weight(hip_ops, path):
    """GRPOCore(top_entropy_quantile=rho).loss_backward leaves the gradient arena of a default GRPOCore handed tok_weight = the fp64 reference mask, bit for bit;
    with an importance cap (a tok_weight of the caller's) the two multiply."""
    from time_r1_amd.config import tiny_test
    from time_r1_amd.grpo import GRPOCore, policy_objective
    from time_r1_amd.model import Engine
    from time_r1_amd.params import ModelParams
    from time_r1_amd.positions import PackedLayout
    from time_r1_amd.synthetic import synthetic_prompt
    cfg = tiny_test()
    pol, ref = ModelParams(cfg, hip_ops, seed=1), ModelParams(cfg, hip_ops, seed=2, optimizer_state=False)
    eng = Engine(cfg, hip_ops, pol)
    G, C, rho = 3, 50, 0.3
    ids, pix, grid = synthetic_prompt(cfg, (4, 6, 8), 9, 7, seed=2, text_vocab=400)
    kw = dict(beta=0.04, use_grpo=path == "use_grpo", seed=3, rope_index_mode="hf4",
              objective=policy_objective(loss_type="dr_grpo", importance_sampling_level="sequence") if path == "objective" else None)
    gen = torch.Generator().manual_seed(9)
    toks = torch.randint(2, 400, (G, C), generator=gen).to(I32)
    mask = vc.grpo_case(G, C)[2]
    adv = torch.randn(G, generator=gen)
    cap = (torch.rand(G, C, generator=gen) * 2).clamp(max=1.5)
    for tokw in (None, cap):
        grads = []
        for sel in (True, False):
            core = GRPOCore(eng, ref.train, G, C, top_entropy_quantile=rho if sel else 1.0, **kw)
            st = core.prepare(ids, pix, grid)
            st.layout = PackedLayout(st.P, G, C)
            st.completion_ids = toks.to(DEV)
            core.forward_logps(st)
            w_ref, thr, kept, n = ec.ref_quantile_weight(st.entropy.float().cpu(), mask, rho)
            assert 0 < kept < n
            tw = None if tokw is None else tokw.to(DEV)
            if not sel:
                tw = w_ref.to(DEV) if tw is None else tw * w_ref.to(DEV)
            pol.train.grad.zero_()
            out, _ = core.loss_backward(st, mask.to(DEV), adv.to(DEV), 0.5, **({} if tw is None else {"tok_weight": tw}))
            grads.append((pol.train.grad.clone(), out.clone()))
        (ga, oa), (gb, ob) = grads
        assert float(ga.abs().max()) > 0
        assert torch.equal(oa.view(I32), ob.view(I32)), (path, tokw is not None)
        assert torch.equal(ga.view(I32), gb.view(I32)), (path, tokw is not None, float((ga - gb).abs().max()))


# ------------------------------------------------------------------------------------------------------------ F. trainer on HipOps
def test_defaults_are_the_parent_run_on_hip(hip_ops, tmp_path):
    ec.check_defaults_are_the_parent_run(hip_ops, tmp_path)


def test_entropy_bonus_in_the_logged_loss_on_hip(hip_ops, tmp_path):
    ec.check_entropy_bonus_in_the_logged_loss(hip_ops, tmp_path)


def test_top_entropy_quantile_changes_the_step_on_hip(hip_ops, tmp_path):
    ec.check_top_entropy_quantile_changes_the_step(hip_ops, tmp_path)


def test_two_iterations_with_both_options_on_hip(hip_ops, tmp_path):
    ec.check_two_iterations_with_both_options(hip_ops, tmp_path)


def test_all_truncated_completions_leave_the_weights_bit_unchanged_on_hip(hip_ops, tmp_path):
    ec.check_all_truncated_leaves_the_weights_alone(hip_ops, tmp_path)
