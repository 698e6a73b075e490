"""GPU: the vocabulary-side HIP kernels (csrc/loss.hip, csrc/sampler.hip, the lmhead_lse tail of csrc/gemm.hip) against the fp64 references of tests/vocab_cases.py.

Cases, references and tolerances live in vocab_cases.py; tests/test_vocab_side_ref.py shows on the CPU that the fp32 oracle sits within a tenth of
every tolerance on the same cases.  The tolerances are the project's own (tests/test_ops_gpu.py); every check prints the worst error it saw
(`pytest -s`), and the figures of the MI355X run are repeated next to each tolerance below.
"""
import pytest
import torch

import vocab_cases as vc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
I32 = torch.int32
DEV = "cuda:0"


def check(got, ref, tol, what):
    ratio, err = vc.worst(got, ref, tol)
    print("OBS %-62s max err %.3e  (%.3f of atol %g + rtol %g |ref|)" % (what, err, ratio, tol[0], tol[1]))
    assert ratio <= 1.0, "%s: max err %.4g is %.3g x the tolerance (atol %g, rtol %g)" % (what, err, ratio, tol[0], tol[1])


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------------------ A. logp_entropy_fwd
# TOL_STATS = atol 1e-3, rtol 1e-4.  Worst seen on MI355X over all 23 cases: logp 5.7e-6, entropy 1.2e-5, lse 4.0e-6 (at most 0.008 of the tolerance).
@pytest.mark.parametrize("name,kw", vc.stat_cases(), ids=[c[0] for c in vc.stat_cases()])
def test_logp_entropy_fwd(hip_ops, name, kw):
    store, x, tg, kinds = vc.stat_rows(**kw)
    col0, V = kw.get("col0", 0), kw["V"]
    store_d = store.to(DEV)
    got = hip_ops.logp_entropy_fwd(store_d[:, col0:col0 + V], tg.to(DEV))
    ref = vc.ref_stats(x, tg)
    for a, b, what in zip(got, ref, ("logp", "entropy", "lse")):
        check(a, b, vc.TOL_STATS, "fwd %s %s" % (name, what))
    assert torch.equal(store_d.cpu().view(torch.int16), store.view(torch.int16)), "the forward does not write its input"


# ------------------------------------------------------------------------------------------------------------ B. lmhead_lse
# fused vs fp64 of the bf16-rounded product: TOL_STATS.  Worst seen on MI355X over the 10 shapes: logp 1.5e-6, entropy 3.2e-6, lse 1.3e-6
# (0.002 of the tolerance; the materialised path against fp64: 1.5e-6, 1.2e-5, 1.3e-6).
# fused vs the materialised HIP path: TOL_FUSED = atol 2e-3, rtol 1e-4.  Worst seen on MI355X: logp 1.9e-6, entropy 1.2e-5, lse 1.9e-6 (0.005 of it).
@pytest.mark.parametrize("M,V,K,bm", vc.LMHEAD_SHAPES, ids=["%dx%d-tile%d" % (s[0], s[1], s[3]) for s in vc.LMHEAD_SHAPES])
def test_lmhead_lse(hip_ops, M, V, K, bm):
    """Every tile height of the fused lm_head (224 / 256 / 288 / 320 rows; the CPU file replays the launcher's choice for these shapes), on peaked,
    constant and two-level rows, with targets on the slice and tile edges."""
    hn, w, tg, logits, kinds = vc.lmhead_case(M, V, K)
    hn_d, w_d, tg_d = hn.to(DEV), w.to(DEV), tg.to(DEV)
    fused = hip_ops.lmhead_lse(hn_d, w_d, tg_d)
    assert fused is not None, "shape outside the fused kernel's range"
    ref = vc.ref_stats(logits, tg)
    for a, b, what in zip(fused, ref, ("logp", "entropy", "lse")):
        check(a, b, vc.TOL_STATS, "lm_head fused vs fp64 %dx%d %s" % (M, V, what))
    lg = hip_ops.gemm_nt(hn_d, w_d)
    # the operands make fp32 accumulation exact in any order (vocab_cases.lmhead_case), so the bf16 logits are the same numbers everywhere
    assert torch.equal(bits(lg).cpu(), bits(logits)), "gemm_nt: bf16 logits differ from the exactly representable product"
    mat = hip_ops.logp_entropy_fwd(lg, tg_d)
    for a, b, c, what in zip(fused, mat, ref, ("logp", "entropy", "lse")):
        check(a, b, vc.TOL_FUSED, "lm_head fused vs materialised %dx%d %s" % (M, V, what))
        check(b, c, vc.TOL_STATS, "lm_head materialised vs fp64 %dx%d %s" % (M, V, what))


# ------------------------------------------------------------------------------------------------------------ C. logp_bwd
# TOL_DLOGITS = atol 1e-3, rtol 1e-2 (bf16 output).  Worst seen on MI355X over the 17 cases: 6.7e-3 at a target element of magnitude 2.2 (0.31 of the tolerance).
# sum-to-zero: bound derived in vocab_cases.sum_to_zero_bound.  Worst seen on MI355X: |sum| 7.1e-3, 0.40 of the bound.
@pytest.mark.parametrize("name,kw", vc.bwd_cases(), ids=[c[0] for c in vc.bwd_cases()])
def test_logp_bwd(hip_ops, name, kw):
    store, x, tg, kinds = vc.stat_rows(**kw)
    R, V, col0 = kw["R"], kw["V"], kw.get("col0", 0)
    dlogp = vc.bwd_dlogp(R, kw["seed"])
    lse64 = vc.ref_stats(x, tg)[2]
    ref = vc.ref_dlogits(x, tg, dlogp, lse64)
    store_d = store.to(DEV)
    view = store_d[:, col0:col0 + V]
    tg_d, lse_d, dlogp_d = tg.to(DEV), lse64.float().to(DEV), dlogp.to(DEV)
    out = hip_ops.logp_bwd(view, tg_d, lse_d, dlogp_d, inplace=False)
    assert out.data_ptr() != view.data_ptr()
    if store.shape[1] != V:
        assert out.stride(0) != view.stride(0), "this case runs ld_out != ld"
    assert torch.equal(store_d.cpu().view(torch.int16), store.view(torch.int16)), "inplace=False leaves the logits alone"
    check(out, ref, vc.TOL_DLOGITS, "bwd %s dlogits" % name)
    # in place (the only form the engine uses): the output aliases the input; bit-equal to the out-of-place result, nothing outside the view touched
    same = hip_ops.logp_bwd(view, tg_d, lse_d, dlogp_d, inplace=True)
    assert same.data_ptr() == view.data_ptr()
    assert torch.equal(bits(same), bits(out)), "in-place and out-of-place results differ"
    after = store_d.cpu()
    outside = torch.ones(store.shape[1], dtype=torch.bool)
    outside[col0:col0 + V] = False
    assert torch.equal(after[:, outside].view(torch.int16), store[:, outside].view(torch.int16)), "wrote outside the [R, V] view"
    # properties, in fp64 on the host from the bf16 output
    o = out.double().cpu()
    zero = dlogp == 0
    assert (o[zero] == 0).all(), "dlogp == 0 must give exactly 0"
    rows = torch.arange(R)
    p_t = torch.exp(x.double()[rows, tg.long()] - lse64)
    check(o[rows, tg.long()], dlogp.double() * (1 - p_t), vc.TOL_DLOGITS, "bwd %s dlogits[target] = g (1 - p)" % name)
    s, bound = o.sum(1).abs(), vc.sum_to_zero_bound(ref, dlogp)
    live = ~zero
    share = float((s[live] / bound[live]).max()) if live.any() else 0.0
    print("OBS %-62s max |sum_v dlogits| %.3e  (%.3f of the bound)" % ("bwd %s sum-to-zero" % name, float(s.max()), share))
    assert (s <= bound).all(), "rows %s: |sum_v dlogits| %s above the bound %s" % (torch.nonzero(s > bound).flatten().tolist(), s[s > bound], bound[s > bound])


def test_logp_bwd_refuses_V_not_multiple_of_8(hip_ops):
    from time_r1_amd.hip import HipError
    for V in (1001, 2047):
        store, x, tg, _ = vc.stat_rows(R=3, V=V, seed=5)
        view = store.to(DEV)[:, :V]
        with pytest.raises(HipError):
            hip_ops.logp_bwd(view, tg.to(DEV), torch.zeros(3, device=DEV), torch.ones(3, device=DEV), inplace=False)


# TOL_DLOGITS.  Worst seen on MI355X: 7.1e-3 on a gradient of magnitude 2 (0.32 of the tolerance).
def test_logp_bwd_pairs_fused_lse_with_recomputed_logits(hip_ops):
    """The chunked backward of the head: LSE from the fused lm_head forward, a chunk's logits recomputed by gemm_nt, logp_bwd in place on them."""
    M, V, K = 257, 33024, 192
    hn, w, tg, logits, _ = vc.lmhead_case(M, V, K)
    dlogp = vc.bwd_dlogp(M, 17)
    hn_d, w_d, tg_d, dlogp_d = hn.to(DEV), w.to(DEV), tg.to(DEV), dlogp.to(DEV)
    _, _, lse = hip_ops.lmhead_lse(hn_d, w_d, tg_d)
    for a, b in ((0, 128), (128, M)):
        lg = hip_ops.gemm_nt(hn_d[a:b], w_d)
        lg_before = lg.clone()
        dl = hip_ops.logp_bwd(lg, tg_d[a:b].contiguous(), lse[a:b].contiguous(), dlogp_d[a:b].contiguous(), inplace=True)
        assert dl.data_ptr() == lg.data_ptr()
        ref = vc.ref_dlogits(lg_before.cpu(), tg[a:b], dlogp[a:b])
        check(dl, ref, vc.TOL_DLOGITS, "bwd pairing rows %d..%d" % (a, b))


# ------------------------------------------------------------------------------------------------------------ D. grpo_loss
# TOL_GRPO = atol 1e-5, rtol 1e-4; dlogp against the autograd gradient of the fp64 loss.  Worst seen on MI355X over the 48 cases, as a share of the
# tolerance (the k3 term reaches 5e8, so rtol carries the comparison): dlogp 0.018, out3 0.004, row_len 0 (exact), row_kl 0.013.
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("beta", [0.0, 0.04])
@pytest.mark.parametrize("use_grpo", [True, False])
@pytest.mark.parametrize("G,C", vc.GRPO_SHAPES)
def test_grpo_loss(hip_ops, G, C, use_grpo, beta, grad_scale):
    logp, ref_lp, mask, adv = vc.grpo_case(G, C)
    rp = ref_lp if beta else None
    ref = vc.ref_grpo(logp, rp, mask, adv, beta, use_grpo, grad_scale)
    got = hip_ops.grpo_loss(logp.to(DEV), rp.to(DEV) if rp is not None else None, mask.to(DEV), adv.to(DEV), beta, use_grpo, grad_scale)
    for a, b, what in zip(got, ref, ("dlogp", "out3", "row_len", "row_kl")):
        check(a, b, vc.TOL_GRPO, "grpo (%d, %d) grpo=%d beta=%g gs=%g %s" % (G, C, use_grpo, beta, grad_scale, what))
    assert (got[0].cpu()[~mask.bool()] == 0).all(), "dlogp at masked positions must be exactly 0"


def test_grpo_loss_refuses_more_than_64_rows(hip_ops):
    from time_r1_amd.hip import HipError
    G, C = 65, 4
    with pytest.raises(HipError):
        hip_ops.grpo_loss(torch.zeros(G, C, device=DEV), None, torch.ones(G, C, dtype=I32, device=DEV), torch.zeros(G, device=DEV), 0.0, True, 1.0)


# ------------------------------------------------------------------------------------------------------------ E. sampler
# Every draw: the token is kept by top-k and the Philox uniform (bit-equal to the host's) lies in its fp64 CDF interval with CDF_SLACK = 1e-4.
# Worst distance of a uniform outside its interval seen on MI355X over 12 992 draws: 1.5e-7 (sweep, top_k = 0, T = 0.7).
def run_draws(hip_ops, logits_d, temperature, top_k, seeds, n_steps, **kw):
    """Sweep (seed, step): -> [(seed, step, tokens [rows] list, u [rows] list)]; asserts that a call writes column `step` only and that the
    uniforms are the host's, bit for bit."""
    rows = logits_d.shape[0]
    G = kw.get("group_rows", 0)
    out = []
    dirty = torch.zeros((), dtype=torch.bool, device=DEV)
    for seed in seeds:
        tok = torch.full((rows, n_steps), -7, dtype=I32, device=DEV)
        us = []
        for step in range(n_steps):
            before = tok.clone()
            u = torch.zeros(rows, device=DEV)
            hip_ops.sample_tokens(logits_d, temperature, top_k, seed, torch.tensor([step], dtype=I32, device=DEV), tok, None, -1, 0, False, u_out=u, **kw)
            other = torch.ones(n_steps, dtype=torch.bool, device=DEV)
            other[step] = False
            dirty |= (tok != before)[:, other].any()
            us.append(u)
        tok_c = tok.cpu()
        for step in range(n_steps):
            u_c = us[step].cpu()
            for r in range(rows):
                want = vc.philox_u(seed + (r // G) * kw.get("seed_stride", 0), r % G, step) if G else vc.philox_u(seed, r, step)
                assert float(u_c[r]) == want, ("philox uniform", seed, step, r, float(u_c[r]), want)
            out.append((seed, step, tok_c[:, step].tolist(), u_c.tolist()))
    assert not bool(dirty), "a call wrote a column other than *step"
    return out


def judge(draws, cdfs, what, expect=None):
    worst = 0.0
    for seed, step, toks, us in draws:
        for r, (t, u) in enumerate(zip(toks, us)):
            keep, cdf = cdfs[r]
            e = vc.draw_error(keep, cdf, t, u)
            assert e is None, (what, "seed %d step %d row %d" % (seed, step, r), e)
            lo = float(cdf[t - 1]) if t > 0 else 0.0
            worst = max(worst, lo - u, u - float(cdf[t]))
            if expect is not None:
                expect(r, t, u)
    print("OBS %-62s %d draws, worst distance outside the CDF interval %.3e (slack %g)" % (what, sum(len(d[2]) for d in draws), worst, vc.CDF_SLACK))


@pytest.mark.parametrize("top_k,T", vc.SWEEP_CONFIGS)
def test_sampler_sweep_full_vocabulary(hip_ops, top_k, T):
    """2048 draws per configuration at V = 152064 (16 rows x 8 steps x 16 seeds), each judged exactly."""
    logits = vc.sweep_rows(vc.SWEEP_ROWS, vc.V_FULL)
    cdfs = [vc.token_cdf(logits[r], T, top_k) for r in range(vc.SWEEP_ROWS)]
    draws = run_draws(hip_ops, logits.to(DEV), T, top_k, vc.SWEEP_SEEDS, vc.SWEEP_STEPS)
    assert sum(len(d[2]) for d in draws) >= 2048
    judge(draws, cdfs, "sampler sweep top_k=%d T=%g" % (top_k, T))


_CRAFTED = vc.crafted_cases()


@pytest.mark.parametrize("name", sorted(_CRAFTED))
def test_sampler_crafted(hip_ops, name):
    c = _CRAFTED[name]
    logits = c["logits"]
    rows, V = logits.shape
    if "store" in c:
        logits_d = c["store"].to(DEV)[:, c["col0"]:c["col0"] + V]
        assert logits_d.data_ptr() % 16 != 0 and logits_d.stride(0) % 8 == 0
        assert torch.equal(bits(logits_d).cpu(), bits(logits))
    else:
        logits_d = logits.to(DEV)
    cdfs = [vc.token_cdf(logits[r], c["temperature"], c["top_k"]) for r in range(rows)]
    if "kept" in c:
        assert all(int(k.sum()) == c["kept"] for k, _ in cdfs)
    only = c.get("only")

    def expect(r, t, u):
        assert only is None or t == only, (name, r, t, u)

    draws = run_draws(hip_ops, logits_d, c["temperature"], c["top_k"], vc.CRAFTED_SEEDS, vc.CRAFTED_STEPS)
    judge(draws, cdfs, "sampler " + name, expect)


@pytest.mark.parametrize("V,fn", [(vc.V_FULL, vc.fused_boundaries), (vc.V_UNFUSED, vc.unfused_boundaries)], ids=["fused", "unfused-V163848"])
def test_sampler_boundary_pairs(hip_ops, V, fn):
    """All mass on two tokens on either side of each boundary of the inverse-CDF search: the token is decided by u <= p alone."""
    logits, meta = vc.pair_case(V, fn(V))
    cdfs = [vc.token_cdf(logits[r], 1.0, 0) for r in range(len(meta))]
    first = [0] * len(meta)
    second = [0] * len(meta)

    def expect(r, t, u):
        _, a, b = meta[r]
        want = vc.pair_expect(logits[r], a, b, 1.0, u)
        assert want is None or t == want, (meta[r], "drew %d, u = %.9g" % (t, u))
        first[r] += t == a
        second[r] += t == b

    draws = run_draws(hip_ops, logits.to(DEV), 1.0, 0, vc.CRAFTED_SEEDS, 8)
    judge(draws, cdfs, "sampler boundary pairs V=%d" % V, expect)
    assert all(f + s == 32 for f, s in zip(first, second))
    assert sum(1 for f in first if f) > 0.9 * len(meta) and sum(1 for s in second if s) > 0.9 * len(meta), "both tokens of (nearly) every pair are drawn"


@pytest.mark.parametrize("top_k", [0, 50])
def test_sampler_one_row_expanded_to_G(hip_ops, top_k):
    """ld == 0: the form the rollout uses for the first token (one logits row shown to G rows)."""
    G = 8
    one = vc.sweep_rows(1, vc.V_FULL, seed=21)
    one_d = one.to(DEV)
    exp = one_d.expand(G, vc.V_FULL)
    assert exp.stride(0) == 0
    cdfs = [vc.token_cdf(one[0], 0.9, top_k)] * G
    d_exp = run_draws(hip_ops, exp, 0.9, top_k, vc.CRAFTED_SEEDS[:2], 4)
    d_con = run_draws(hip_ops, exp.contiguous(), 0.9, top_k, vc.CRAFTED_SEEDS[:2], 4)
    assert d_exp == d_con, "expanded row and its contiguous copy draw different tokens"
    judge(d_exp, cdfs, "sampler ld == 0 top_k=%d" % top_k)
    assert any(len(set(d[2])) > 1 for d in d_exp), "the G rows draw with their own uniforms"


@pytest.mark.parametrize("V", [vc.V_FULL, 1001])
def test_sampler_grouped_seed_equals_separate_launches(hip_ops, V):
    """B prompts x G rows in one launch (group_rows = G, seed_stride = 7919) == B launches with seed + 7919 b."""
    B, G, seed = 3, 4, 20240607
    logits = vc.sweep_rows(B * G, V, seed=22)
    logits_d = logits.to(DEV)
    cdfs = [vc.token_cdf(logits[r], 0.9, 50) for r in range(B * G)]
    one = run_draws(hip_ops, logits_d, 0.9, 50, (seed,), 4, group_rows=G, seed_stride=7919)
    judge(one, cdfs, "sampler grouped seed V=%d" % V)
    for b in range(B):
        sep = run_draws(hip_ops, logits_d[b * G:(b + 1) * G], 0.9, 50, (seed + 7919 * b,), 4)
        for (_, step, toks, us), (_, step2, toks2, us2) in zip(one, sep):
            assert step == step2 and toks[b * G:(b + 1) * G] == toks2 and us[b * G:(b + 1) * G] == us2, (b, step)


@pytest.mark.parametrize("V", [vc.V_FULL, 1001])
def test_sampler_step_form_over_consecutive_calls(hip_ops, V):
    """tr1_sample_tokens_step with a workspace zeroed once: 20 decode calls, rows finishing on the way, equal call by call to the plain entry point."""
    rows, eos, pad, seed = 8, 3, 1, 777
    C = vc.STEP_CALLS
    tok_a = torch.full((rows, C), -7, dtype=I32, device=DEV)
    tok_b = tok_a.clone()
    fin_a = torch.zeros(rows, dtype=I32, device=DEV)
    fin_b = fin_a.clone()
    nid = torch.full((rows,), -7, dtype=I32, device=DEV)
    n_checked, mixed = 0, 0
    for call in range(C):
        logits = vc.step_form_logits(call, rows, V, eos)
        logits_d = logits.to(DEV)
        step = torch.tensor([call], dtype=I32, device=DEV)
        was_done = fin_b.cpu().bool()
        u_a, u_b = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
        hip_ops.sample_tokens(logits_d, 1.0, 50, seed, step, tok_a, fin_a, eos, pad, True, u_out=u_a)
        hip_ops.sample_tokens(logits_d, 1.0, 50, seed, step, tok_b, fin_b, eos, pad, True, u_out=u_b, next_ids=nid)
        ws = hip_ops._ws[("sampler_step", rows)]
        assert not bool(ws.any()), "call %d left the cached workspace dirty" % call
        assert torch.equal(tok_a, tok_b) and torch.equal(fin_a, fin_b) and torch.equal(u_a, u_b), "call %d: step form differs from the plain entry point" % call
        assert torch.equal(nid, tok_b[:, call]), "next_ids is the written column"
        assert (tok_b[:, call + 1:] == -7).all()
        t, f, u = tok_b[:, call].cpu(), fin_b.cpu().bool(), u_b.cpu()
        assert (f | ~was_done).all(), "a finished row stays finished"
        mixed += bool(was_done.any() and not was_done.all())
        for r in range(rows):
            if was_done[r]:
                assert int(t[r]) == pad and int(nid[r]) == pad
                continue
            assert float(u[r]) == vc.philox_u(seed, r, call)
            e = vc.draw_error(*vc.token_cdf(logits[r], 1.0, 50), int(t[r]), float(u[r]))
            assert e is None, (call, r, e)
            assert bool(f[r]) == (int(t[r]) == eos)
            n_checked += 1
    assert mixed >= 3 and bool(fin_b.all()), "rows finish on the way, all by the end"
    print("OBS sampler step form V=%d: %d live draws checked over %d calls" % (V, n_checked, C))
