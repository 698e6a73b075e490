"""CPU: the fp32 oracle (oracle/ref_ops.py) against the fp64 references of tests/vocab_cases.py, on every case tests/test_vocab_side_gpu.py uses.

The trainer goldens lean on the oracle, and the GPU file compares the HIP kernels with the fp64 references at the project's tolerances.  Here the
oracle has to sit within ONE TENTH of each tolerance on every case: the cases are then well-posed (a GPU miss cannot be the reference's own
rounding), and the oracle itself is checked at the rows a trained policy produces - peaked, constant, two-level, wide.  The tile-height table of
the fused lm_head cases is replayed against the launcher's cost model, so it cannot silently rot.
"""
import re
import os

import numpy as np
import pytest
import torch

import vocab_cases as vc

BF16 = torch.bfloat16
TENTH = vc.ORACLE_SHARE


def within(got, ref, tol, share, what):
    ratio, err = vc.worst(got, ref, tol)
    print("%s: max err %.3g = %.3g of the tolerance" % (what, err, ratio))
    assert ratio <= share, "%s: max err %.4g is %.3g of the tolerance (allowed %.2g)" % (what, err, ratio, share)


# ---------------------------------------------------------------------------------------------------------------- A / C
@pytest.mark.parametrize("name,kw", vc.stat_cases(), ids=[c[0] for c in vc.stat_cases()])
def test_oracle_logp_entropy(ref_ops, name, kw):
    store, x, tg, kinds = vc.stat_rows(**kw)
    assert float(x.float().abs().max()) <= vc.LOGIT_LIMIT and torch.isfinite(x.float()).all()
    assert ((tg >= 0) & (tg < kw["V"])).all()
    ref = vc.ref_stats(x, tg)
    got = ref_ops.logp_entropy_fwd(x.float(), tg)
    for a, b, what in zip(got, ref, ("logp", "entropy", "lse")):
        within(a, b, vc.TOL_STATS, TENTH, "%s %s" % (name, what))
    for r, kind in enumerate(kinds):
        if kind == "const":
            assert abs(float(ref[1][r]) - np.log(kw["V"])) < 1e-9, "a constant row has entropy ln V"
        if kind == "peak_hit":
            assert float(ref[0][r]) > -1e-3 and float(ref[1][r]) < 1e-2
        if kind == "peak_tail":
            assert float(ref[0][r]) < -18.0


def test_stat_rows_cover_every_kind_and_lane():
    _, _, tg, kinds = vc.stat_rows(R=64, V=2048, seed=3)
    assert set(kinds) == set(vc.ROW_KINDS)
    free = [int(tg[r]) % 8 for r, k in enumerate(kinds) if k == "normal"]
    assert sorted(set(free)) == list(range(8)), "targets of the plain rows sit in every lane of a 16-byte chunk"
    assert {c[1]["V"] for c in vc.stat_cases()} == set(vc.STAT_V) and {c[1]["R"] for c in vc.stat_cases()} == set(vc.STAT_ROWS)
    assert any(c[1].get("ld", 0) > c[1]["V"] for c in vc.stat_cases())


@pytest.mark.parametrize("name,kw", vc.bwd_cases(), ids=[c[0] for c in vc.bwd_cases()])
def test_oracle_logp_bwd(ref_ops, name, kw):
    assert kw["V"] % 8 == 0
    store, x, tg, kinds = vc.stat_rows(**kw)
    dlogp = vc.bwd_dlogp(kw["R"], kw["seed"])
    lse = vc.ref_stats(x, tg)[2]
    ref = vc.ref_dlogits(x, tg, dlogp, lse)
    got = ref_ops.logp_bwd(x.float(), tg, lse.float(), dlogp, inplace=False)
    within(got, ref, vc.TOL_DLOGITS, TENTH, name + " dlogits")
    rows = torch.arange(kw["R"])
    p_t = torch.exp(x.double()[rows, tg.long()] - lse)
    assert torch.allclose(ref[rows, tg.long()], dlogp.double() * (1 - p_t), rtol=1e-12, atol=1e-15)
    assert float(ref.sum(1).abs().max()) < 1e-9, "the exact gradient of a row sums to 0"
    assert (ref[dlogp == 0] == 0).all()
    if kw["R"] >= 37:
        assert (dlogp == 0).any() and (dlogp > 0).any() and (dlogp < 0).any()
    # the bound of the sum-to-zero property holds for the correctly rounded gradient
    s = ref.to(BF16).double().sum(1).abs()
    assert (s <= vc.sum_to_zero_bound(ref, dlogp)).all()


# ---------------------------------------------------------------------------------------------------------------- B
def test_lmhead_tile_height_replay_matches_the_launcher_source():
    """The replay is only worth something while it is the launcher's rule: pin the constants it copies."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "time-r1_amd", "csrc", "gemm.hip")).read()
    body = src[src.index('extern "C" int tr1_lmhead_lse_fwd'):]
    body = body[:body.index("lse_combine_kernel")]
    flat, whole = re.sub(r"\s+", " ", body), re.sub(r"\s+", " ", src)
    # the one table, the one cost and the one picker of the 8-wave tile height (first = 256: 256, 224, 288, 320 - the order of the replay)
    assert whole.count("static const double NT8P_EFF[4] = {0.94, 1.0, 1.025, 1.03};") == 1 and whole.count("{0.94, 1.0, 1.025, 1.03}") == 1
    assert "static double nt8p_cost(int64_t M, int64_t n_tiles, int64_t rows, double eff) { const int64_t t = ((M + rows - 1) / rows) * n_tiles; return (double)((t + 255) / 256) * 256.0 * (double)(rows * BN2) / eff; }" in whole
    assert "static int nt8p_pick_rt(int64_t M, int64_t n_tiles, int first) { int rt = first / 32; double best = nt8p_cost(M, n_tiles, first, NT8P_EFF[rt - 7]); for (int r = 7; r <= 10; ++r) { const double c = nt8p_cost(M, n_tiles, r * 32, NT8P_EFF[r - 7]); if (c < best) { best = c; rt = r; } } return rt; }" in whole
    # the lm_head's call: start at 256, whole and ragged 256-column tiles
    assert "const int64_t t2n = (N + BN2 - 1) / BN2;" in flat and "nt8p_pick_rt(M, t2n, 256)" in flat and flat.count("nt8p_pick_rt(") == 1
    assert re.search(r"#define BN2 256\b", src)


def test_lmhead_shapes_hit_every_tile_height():
    for M, V, K, bm in vc.LMHEAD_SHAPES:
        assert vc.lmhead_tile_rows(M, V) == bm, "(%d, %d): the launcher now picks %d-row tiles, the table says %d - re-pick the shapes" % (
            M, V, vc.lmhead_tile_rows(M, V), bm)
        assert V % 64 == 0 and K % 64 == 0 and V >= 256
    assert {s[3] for s in vc.LMHEAD_SHAPES} == {224, 256, 288, 320}
    assert vc.lmhead_tile_rows(321, 33024) == 224 and 321 - 224 == 97            # a second, 97-row tile
    assert 151936 % 256 != 0                                                   # ragged last column tile
    # what the present op test runs: only 224 and 320
    old = [(48, 512), (300, 1024), (7, 256), (1600, 152064), (64, 320), (33, 448), (1600, 151936)]
    assert {vc.lmhead_tile_rows(*s) for s in old} == {224, 320}


@pytest.mark.parametrize("M,V,K,bm", vc.LMHEAD_SHAPES, ids=["%dx%d" % s[:2] for s in vc.LMHEAD_SHAPES])
def test_oracle_lmhead(ref_ops, M, V, K, bm):
    hn, w, tg, logits, kinds = vc.lmhead_case(M, V, K)
    assert set(kinds) >= {"normal", "peak_hit", "peak_tail", "const", "two_level"}
    assert float(logits.float().abs().max()) <= vc.LOGIT_LIMIT, float(logits.float().abs().max())
    assert vc.lmhead_product_is_exact(hn, w, torch.arange(0, M, max(1, M // 12))), "fp32 accumulation of these operands must be exact"
    if bm < M:
        assert int(tg[bm - 1]) != int(tg[bm]) and kinds[bm - 1] == kinds[bm] == "normal"
    for c in (0, 63, 64, V - 64, V - 1, V - 100):
        assert (tg == c).any(), c
    ref = vc.ref_stats(logits, tg)
    got = ref_ops.logp_entropy_fwd(logits.float(), tg)
    for a, b, what in zip(got, ref, ("logp", "entropy", "lse")):
        within(a, b, vc.TOL_STATS, TENTH, "lm_head %dx%d %s" % (M, V, what))
    for r in range(min(M, 40)):
        if kinds[r] == "peak_hit":
            assert float(ref[0][r]) > -1e-3, (r, float(ref[0][r]))
        if kinds[r] == "const":
            assert abs(float(ref[1][r]) - np.log(V)) < 1e-9
        if kinds[r] == "two_level":
            assert abs(float(ref[2][r]) - 60.0) < 1e-9


# ---------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("beta", [0.0, 0.04])
@pytest.mark.parametrize("use_grpo", [True, False])
@pytest.mark.parametrize("G,C", vc.GRPO_SHAPES)
def test_oracle_grpo_loss(ref_ops, G, C, use_grpo, beta, grad_scale):
    logp, ref_lp, mask, adv = vc.grpo_case(G, C)
    assert torch.isfinite(torch.exp(ref_lp - logp)).all(), "masked positions stay finite in fp32"
    live = mask.bool()
    if G * C > 8:
        assert float((ref_lp - logp)[live].abs().max()) > 0.9 * vc.GRPO_MAX_DIFF
    rp = ref_lp if beta else None
    ref = vc.ref_grpo(logp, rp, mask, adv, beta, use_grpo, grad_scale)
    got = ref_ops.grpo_loss(logp, rp, mask, adv, beta, use_grpo, grad_scale)
    for a, b, what in zip(got, ref, ("dlogp", "out3", "row_len", "row_kl")):
        within(a, b, vc.TOL_GRPO, TENTH, "grpo (%d, %d) %s" % (G, C, what))
    assert (ref[0][~live] == 0).all(), "no gradient at masked positions"
    # the masked positions do not enter the loss: the same grid with harmless values there gives the same numbers
    ref2 = vc.ref_grpo(torch.where(live, logp, torch.zeros_like(logp)), None if rp is None else torch.where(live, rp, torch.zeros_like(rp)), mask, adv,
                       beta, use_grpo, grad_scale)
    for a, b in zip(ref, ref2):
        assert torch.equal(a, b)


def test_grpo_masks_have_the_listed_forms():
    _, _, mask, _ = vc.grpo_case(8, 200)
    m = mask.bool()
    assert int(m[0].sum()) == 1, "a row of length 1"
    is_prefix = [bool((m[r].long().diff() <= 0).all()) for r in range(8)]
    assert not is_prefix[1] and all(is_prefix[2:]), "one mask with holes, prefixes elsewhere"
    assert int(m[7].sum()) == 200
    _, _, mask, _ = vc.grpo_case(1, 1)
    assert mask.tolist() == [[1]]


# ---------------------------------------------------------------------------------------------------------------- E
def test_philox_matches_the_oracle():
    from oracle.ref_ops import philox_uniform
    for seed in vc.SWEEP_SEEDS + vc.CRAFTED_SEEDS:
        for row in (0, 1, 15, 63):
            for step in (0, 3, 7, 19):
                u = vc.philox_u(seed, row, step)
                assert u == float(np.float32(philox_uniform(seed, row, step))) and 0.0 < u < 1.0, "the oracle's uniform, stored in fp32"


def _oracle_draws(ref_ops, logits, temperature, top_k, seeds, steps, C, check=None):
    rows, V = logits.shape
    cdfs = [vc.token_cdf(logits[r], temperature, top_k) for r in range(rows)]
    for seed in seeds:
        tok = torch.full((rows, C), -7, dtype=torch.int32)
        for step in steps:
            u = torch.zeros(rows)
            ref_ops.sample_tokens(logits.float(), temperature, top_k, seed, torch.tensor([step], dtype=torch.int32), tok, None, -1, 0, False, u_out=u)
            for r in range(rows):
                ur = vc.philox_u(seed, r, step)
                assert float(u[r]) == ur
                e = vc.draw_error(cdfs[r][0], cdfs[r][1], int(tok[r, step]), ur)
                assert e is None, (seed, step, r, e)
                if check:
                    check(r, int(tok[r, step]), ur)
    return cdfs


@pytest.mark.parametrize("top_k,T", vc.SWEEP_CONFIGS)
def test_oracle_sampler_sweep(ref_ops, top_k, T):
    """The oracle on the sweep's rows (a sample of the GPU file's 2048 draws per configuration: the full-vocabulary oracle costs milliseconds per draw)."""
    logits = vc.sweep_rows(vc.SWEEP_ROWS, vc.V_FULL)
    assert vc.SWEEP_ROWS * vc.SWEEP_STEPS * len(vc.SWEEP_SEEDS) >= 2048
    _oracle_draws(ref_ops, logits, T, top_k, vc.SWEEP_SEEDS[:2], (0, vc.SWEEP_STEPS - 1), vc.SWEEP_STEPS)


_CRAFTED = vc.crafted_cases()


@pytest.mark.parametrize("name", sorted(_CRAFTED))
def test_oracle_sampler_crafted(ref_ops, name):
    c = _CRAFTED[name]
    logits = c["logits"]
    only = c.get("only")

    def check(r, tok, u):
        if only is not None:
            assert tok == only, (r, tok, u)

    cdfs = _oracle_draws(ref_ops, logits, c["temperature"], c["top_k"], vc.CRAFTED_SEEDS[:2], (0, vc.CRAFTED_STEPS - 1), vc.CRAFTED_STEPS, check)
    if "kept" in c:
        for keep, _ in cdfs:
            assert int(keep.sum()) == c["kept"]
    if only is not None:
        for keep, cdf in cdfs:
            assert float(cdf[only] - (cdf[only - 1] if only else 0.0)) > 1 - 1e-12, "all mass on one token"


@pytest.mark.parametrize("V,fn", [(vc.V_FULL, vc.fused_boundaries), (vc.V_UNFUSED, vc.unfused_boundaries)], ids=["fused", "unfused"])
def test_oracle_sampler_boundary_pairs(ref_ops, V, fn):
    bounds = fn(V)
    logits, meta = vc.pair_case(V, bounds)
    assert (V <= vc.SAMP_FUSED_MAXV) == (fn is vc.fused_boundaries) and V % 8 == 0
    if fn is vc.fused_boundaries:
        nch = V // 8
        seg = (nch + 15) // 16
        names = " ".join(n for n, _ in bounds)
        assert "seg15" in names and "it%d" % ((seg + 63) // 64 - 1) in names, "a wave-segment boundary and the last iteration of a segment are covered"
    sides = set()
    sel = list(range(len(meta)))
    lg, sub = logits[sel], [meta[i] for i in sel]

    def check(r, tok, u):
        _, a, b = sub[r]
        want = vc.pair_expect(lg[r], a, b, 1.0, u)
        assert want is None or tok == want, (sub[r], tok, u)
        sides.add(tok == a)

    _oracle_draws(ref_ops, lg, 1.0, 0, vc.CRAFTED_SEEDS[:1], (0, 1), vc.CRAFTED_STEPS, check)
    assert sides == {True, False}, "draws land on both sides of the split"
    for name, a, b in meta:
        assert 0 <= a < b < V


def test_step_form_logits_finish_rows_on_the_way():
    for call in (0, 5, 19):
        x = vc.step_form_logits(call, rows=8, V=4096)
        p = torch.softmax(x.double(), -1)[:, 3]
        if call >= 5:
            assert float(p[call % 8]) > 0.999999
            assert float(p.sum()) < 1.01
        else:
            assert float(p.max()) < 0.5
