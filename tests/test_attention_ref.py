"""CPU: the attention cases of tests/attn_cases.py are what tests/test_attention_gpu.py takes them for.

  * the fp32 oracle (oracle/ref_ops.py attn_fwd / attn_bwd, on which tests/test_ops_gpu.py rests) sits within a tenth of every derived bound against the
    fp64 reference - a miss on the GPU cannot be the oracle's rounding;
  * an fp32 emulation of the kernels' rounding points (bf16 P and dS, fp32 everything else, lazy running maximum, bf16 outputs) stays within every bound
    and uses a good part of it - the bounds are attainable, not slack;
  * every mask mutant (one edge of every row moved by one key) is caught by the bounds on at least 90 % of the rows whose visible set it changes;
  * the mechanisms the cases are named for occur: replayed from the masks and scores the way tests/test_gemm_tile_heights.py replays the GEMM launcher.
Every check prints its figures (`pytest -s`)."""
import pytest
import torch

import attn_cases as ac

ALL = ac.CASE_NAMES + ac.DECODE_NAMES


def _shares(triples):
    return [ac.share(got, ref, tol)[0] for got, ref, tol in triples]


@pytest.mark.parametrize("name", ALL)
def test_scores_stay_within_64_nats_and_the_poison_is_in_place(name):
    c, r = ac.case(name), ac.ref_fwd_of(name)
    s = r.s[torch.isfinite(r.s)]
    assert s.numel() == 0 or float(s.abs().max()) <= 64.0, "visible scores up to %.1f nats" % float(s.abs().max())
    assert bool(torch.isnan(c.k[c.S:].float()).all()) and bool(torch.isnan(c.v[c.S:].float()).all()) and c.k.shape[0] > c.S
    big = float(torch.tensor(1e4).to(torch.bfloat16))
    assert bool((c.k[:c.S][c.poison].float().abs() == big).all()) and bool((c.v[:c.S][c.poison].float().abs() == big).all())
    assert not bool((c.poison & ~c.unseen).any())
    assert bool(torch.isfinite(c.k[:c.S].float()).all()) and bool(torch.isfinite(r.O).all())


def test_every_family_and_a_mixed_wave_occur():
    """Every family in every case of 45 tokens or more; 32-row waves that hold more than one family, and the hot / cold alternation inside one wave."""
    for name in ac.CASE_NAMES:
        c = ac.case(name)
        if c.T >= 45:
            assert set(c.fam.tolist()) == set(range(9)), name
    c = ac.case("long-prefix")
    fam_of_row = c.fam.repeat_interleave(c.group)
    waves = fam_of_row[:fam_of_row.numel() // 32 * 32].view(-1, 32)
    assert int((waves.min(1).values != waves.max(1).values).sum()) > waves.shape[0] // 2
    assert bool(((waves == 7).sum(1) >= 2 * c.group).any())


@pytest.mark.parametrize("name", ALL)
def test_oracle_fp32_within_a_tenth_of_every_bound(ref_ops, name):
    c, r = ac.case(name), ac.ref_fwd_of(name)
    pre, lo, hi = [x.int() for x in (c.pre, c.lo, c.hi)]
    q, k, v = c.q.float(), c.k[:c.S].float(), c.v[:c.S].float()
    o, lse = ref_ops.attn_fwd(q, k, v.t().contiguous(), pre, lo, hi, c.nh, c.nkv, c.S, c.hd, c.scale)
    # the backward at the oracle's OWN O / lse (its autograd backward is the gradient of its own forward)
    dq, dk, dv = ref_ops.attn_bwd(q, k, v, o, c.do.float(), lse, pre, lo, hi, c.nh, c.nkv, c.S, c.hd, c.scale)
    b = ac.ref_bwd(c, o, lse)
    sh = _shares([(o, r.O, r.tol_O), (lse, r.lse, r.tol_lse), (dq, b.dQ, b.tol_dQ), (dk, b.dK, b.tol_dK), (dv, b.dV, b.tol_dV)])
    print("OBS oracle %-20s share of bound: O %.4f  lse %.4f  dQ %.4f  dK %.4f  dV %.4f" % (name, *sh))
    assert max(sh) <= 0.1, sh


@pytest.mark.parametrize("name", ALL)
def test_emulated_rounding_points_stay_within_the_bounds(name):
    c, r = ac.case(name), ac.ref_fwd_of(name)
    o, lse, _ = ac.emulate_fwd(c)
    o16, lse32 = ac.bf(r.O), r.lse.float()
    b = ac.ref_bwd(c, o16, lse32)
    dq, dk, dv = ac.emulate_bwd(c, o16, lse32)
    sh = _shares([(o, r.O, r.tol_O), (lse, r.lse, r.tol_lse), (dq, b.dQ, b.tol_dQ), (dk, b.dK, b.tol_dK), (dv, b.dV, b.tol_dV)])
    print("OBS emulation %-20s share of bound: O %.3f  lse %.3f  dQ %.3f  dK %.3f  dV %.3f" % (name, *sh))
    assert max(sh) <= 1.0, sh
    assert bool((dk.float()[c.unseen] == 0).all()) and bool((dv.float()[c.unseen] == 0).all())


def test_the_bounds_are_attainable():
    """Over the cases the emulation uses more than half of every bound that a bf16 rounding point sets (the LSE bound is an fp32 worst case)."""
    worst = [0.0] * 4
    for name in ("causal-200", "tile-edges-128-64", "long-prefix", "segments-128"):
        c, r = ac.case(name), ac.ref_fwd_of(name)
        o16, lse32 = ac.bf(r.O), r.lse.float()
        b = ac.ref_bwd(c, o16, lse32)
        dq, dk, dv = ac.emulate_bwd(c, o16, lse32)
        sh = _shares([(ac.emulate_fwd(c)[0], r.O, r.tol_O), (dq, b.dQ, b.tol_dQ), (dk, b.dK, b.tol_dK), (dv, b.dV, b.tol_dV)])
        worst = [max(a, x) for a, x in zip(worst, sh)]
    print("OBS emulation, largest shares: O %.3f  dQ %.3f  dK %.3f  dV %.3f" % tuple(worst))
    assert min(worst) >= 0.5, worst


@pytest.mark.parametrize("name", ALL)
def test_every_mask_mutant_is_caught(name):
    """pre +- 1, lo +- 1, hi +- 1 on every row: of the (head, token) rows whose visible set changes, at least 90 % are off by 2 x a bound - in the LSE or in some
    element of O; decode launches run without the LSE (need_lse=False), so there O alone has to do it, on the edge-weighted rows."""
    c, r = ac.case(name), ac.ref_fwd_of(name)
    decode = name in ac.DECODE_NAMES
    for which, d in ac.MUTANTS:
        changed, caught = ac.mutant_catch(c, r, which, d, use_lse=not decode, rows=(c.fam == 8) if decode else None)
        print("OBS mutant %-20s %s%+d: %d of %d changed rows caught" % (name, which, d, caught, changed))
        assert caught >= 0.9 * changed, (which, d, caught, changed)
    if decode:
        assert int((c.fam == 8).sum()) >= 2


LAZY_BOTH = ("causal-200", "rows257", "tile-edges-128-64", "clamped", "segments-128", "continuation", "long-causal", "long-prefix")
WAVES_ALL_THREE = ("causal-200", "tile-edges-128-64", "lo-in-prefix-tile", "gap", "clamped", "segments-128", "long-prefix")
QMETA_SKIPS = ("gap", "gap-d64", "segments", "segments-128", "long-prefix", "causal-200")


@pytest.mark.parametrize("name", sorted(set(LAZY_BOTH + WAVES_ALL_THREE)))
def test_replay_lazy_maximum_and_wave_decisions(name):
    """attn_fwd32_kernel's per-wave decisions, replayed by emulate_fwd: the lazy maximum is KEPT on some tile although a row's maximum rose, and REPLACED on some
    tile of a wave whose rows all had a maximum already; some wave x tile visit is any && !full, some full, some !any."""
    st = ac.emulate_fwd(ac.case(name))[2]
    print("OBS replay %-20s %s" % (name, st))
    if name in LAZY_BOTH:
        assert st["kept"] > 0 and st["replaced"] > 0, st
    if name in WAVES_ALL_THREE:
        assert st["any_not_full"] > 0 and st["full"] > 0 and st["not_any"] > 0, st


def test_replay_lazy_maximum_off_gives_the_same_numbers_within_the_bounds():
    """The lazy rule only moves the reference point of exp2: with it switched off the emulation rescales on every rise and still sits within the bounds."""
    c, r = ac.case("long-causal"), ac.ref_fwd_of("long-causal")
    o, lse, st = ac.emulate_fwd(c, lazy=0.0)
    assert st["kept"] == 0
    assert max(_shares([(o, r.O, r.tol_O), (lse, r.lse, r.tol_lse)])) <= 1.0


def test_replay_backward_launch():
    """dkdv_qsplit: QS == 1 up to 64 packed rows, QS > 1 above; the qmeta summary lets the dK / dV kernels skip (query tile, key block) visits."""
    assert ac.replay_bwd(ac.case("causal-64"))[0] == 1 and ac.replay_bwd(ac.case("causal-1"))[0] == 1
    assert ac.replay_bwd(ac.case("causal-65"))[0] == 2 and ac.replay_bwd(ac.case("long-prefix"))[0] == 8
    for name in QMETA_SKIPS:
        qs, skipped, made = ac.replay_bwd(ac.case(name))
        print("OBS replay bwd %-20s QS %d, %d visits skipped, %d made" % (name, qs, skipped, made))
        assert skipped > 0 and made > 0


def test_replay_tile_ranges():
    """att_tile_range on the blocks of the named cases: `lo-in-prefix-tile` clamps start2 to pre_tiles, `gap` leaves whole tiles out between the groups,
    `clamped` takes both clamps, and two cases have rows with 6 key tiles or more."""
    c = ac.case("lo-in-prefix-tile")
    assert int(c.lo[c.pre > 0].min()) // 64 < (int(c.pre.max()) + 63) // 64
    assert ac.tile_range(70, 70, 129, 130) == [0, 1, 2]
    c = ac.case("gap")
    tiles = ac.tile_range(int(c.pre.max()), int(c.lo[-1]), int(c.hi[-1]), c.S)
    assert tiles == [0, 5] and bool(c.poison[128:191].all()) and not bool(c.poison[191])      # (191 = lo - 1 of the next group keeps its score)
    c = ac.case("clamped")
    assert c.S == 203 and c.S % 8 == 3 and bool((c.hi >= c.S).any()) and bool((c.pre > c.S).any())
    assert ac.tile_range(c.S + 9, 0, c.S + 5, c.S) == [0, 1, 2, 3]
    long_cases = [n for n in ac.CASE_NAMES if int(ac.case(n).vis.sum(1).max()) >= 6 * 64]
    assert len(long_cases) >= 2, long_cases
    assert max(ac.case(n).S for n in ALL) <= 704 and max(ac.case(n).T * ac.case(n).group for n in ALL) <= 2500


def test_unfrag_inverts_the_documented_layout():
    rows, nh = 21, 3
    x = torch.arange(rows * nh * 128, dtype=torch.float32).view(rows, nh * 128)
    of = torch.zeros((rows + 15) // 16 * 16 * nh * 128)
    for m in range(rows):
        for k in range(nh * 128):
            of[((m // 16) * (nh * 4) + k // 32) * 512 + (m % 16) * 32 + k % 32] = x[m, k]
    assert torch.equal(ac.unfrag(of, rows, nh), x)
