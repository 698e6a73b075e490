"""CPU: the fp32 oracle (oracle/ref_ops.py) against the fp64 references of tests/optim_cases.py on the cases the GPU file runs, and the host-side
logic those cases lean on: the replay of the weight-gradient launcher's tile choice, the exact-sum data, the lazy-zero partition of the arena.

The oracle must sit at or below optim_cases.ORACLE_SHARE (0.75) of every derived bound: a HIP kernel that then misses a bound is not missing it
because of the reference's own rounding.
"""
import os

import numpy as np
import pytest
import torch

import optim_cases as oc

BF16 = torch.bfloat16
F32 = torch.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "time-r1_amd", "csrc")

CASES = oc.adamw_cases()


# ---------------------------------------------------------------------------------------------------------------- A
def test_bound_constants_are_the_documented_rounding_counts():
    u = 2.0 ** -24
    assert (oc.E_GG, oc.R_M, oc.R_V, oc.R_D, oc.C_P) == (7 * u, 9 * u, 17 * u, 26 * u, 2.0)
    assert oc.R_M == (1 + 1 + 7) * u + 0 * u and oc.R_V == (1 + 2 + 2 * 7 + 0) * u + 0 * u
    assert 8.5 + 1 + 1 + 1 + 1 == 12.5 and 12.5 + 4 + 9 == 25.5 <= oc.R_D / u
    # the hyper-parameters are fp32 values, and 1 - beta is exact in fp32
    for b in (oc.B1, oc.B2):
        assert float(np.float32(b)) == b and float(np.float32(1.0) - np.float32(b)) == 1.0 - b
    # lr * wd < 2^-25 at lr 1e-6, wd 0.01: the decay factor is exactly 1 in fp32 (documented, inside the ulp term)
    assert oc.f32(1e-6) * oc.f32(0.01) < 2.0 ** -25 and float(np.float32(1.0) - np.float32(oc.f32(1e-6)) * np.float32(oc.f32(0.01))) == 1.0


def test_case_table_covers_what_it_claims():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert {c["lr"] for c in CASES} >= {oc.f32(1e-6), oc.f32(2e-5), oc.f32(1e-3)}
    assert {(c["lr"], c["wd"]) for c in CASES} >= {(oc.f32(a), oc.f32(b)) for a in (1e-6, 2e-5) for b in (0.0, 0.01)}
    assert {c["step"] for c in CASES} >= {1, 2, 1000, 100000}
    assert {c["state"] for c in CASES} == {"first", "trained", "tiny"}
    assert {c["n"] for c in CASES} >= {1, 3, 4, 5, 1023, 4096 * 256 * 4 + 3, 3 * 4096 * 256 * 4 + 1}
    assert {c["offs"][:4] for c in CASES} >= {(1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3)}
    assert any(c["offs"][4] % 2 and c["offs"][5] % 2 for c in CASES)
    by = {c["name"]: c for c in CASES}
    # the clip cases do what their names say
    gm, mx = 0.5, 1.0
    norm = lambda ss: gm * float(np.sqrt(np.float64(ss))) + 1e-6
    assert norm(by["clip-below"]["clip"]) < mx < norm(by["clip-just-below"]["clip"])        # the 1e-6 already tips the nearest neighbour of 4 over
    assert norm(by["clip-just-above"]["clip"]) > mx and norm(by["clip-above"]["clip"]) > mx
    assert by["clip-just-below"]["clip"] < 4.0 < by["clip-just-above"]["clip"]
    assert oc.ref_coef(by["clip-below"]["clip"], mx, gm) == gm and oc.ref_coef(0.0, mx, gm) == gm
    assert oc.ref_coef(by["clip-above"]["clip"], mx, gm) < gm and oc.ref_coef(1e30, mx, gm) < 1e-14
    assert by["clip-maxnorm0"]["max_norm"] == 0.0 and by["clip-none"]["clip"] is None and by["clip-gm0.125"]["gm"] == 0.125
    # the "given" sumsq of the trained state clips (norm 0.5 sqrt(n) 1e-2 = 0.5 at n = 10007 does not; the 100003-element settings do)
    p, m, v, g, ss = oc.adamw_inputs(by["lr1e-6-wd0.01-step2-trained"])
    assert 0.5 * float(ss.sqrt()) > 1.0
    # tiny gradients: v' about 1e-12
    p, m, v, g, ss = oc.adamw_inputs(by["lr1e-6-wd0-step2-tiny"])
    ref = oc.ref_adamw(p, m, v, g, oc.f32(1e-6), 0.0, 2, None, 1.0, 1.0)
    assert 1e-13 < float(ref["v"].median()) < 1e-11
    # in some elements the two terms of m' cancel to below a tenth of their size, and the update cancels most of p
    p, m, v, g, ss = oc.adamw_inputs(by["lr1e-3-wd0.01-step1000-trained"])
    ref = oc.ref_adamw(p, m, v, g, oc.f32(1e-3), oc.f32(0.01), 1000, ss, 1.0, 0.5)
    assert bool((ref["m"].abs() < 0.1 * ref["terms"]).any()) and bool((ref["p"].abs() < 0.1 * p.double().abs()).any())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_oracle_adamw_step_within_share_of_bounds(ref_ops, case):
    """The fp32 oracle on views at the case's offsets: at most 0.75 of every bound, p16 = bf16(master), gradient zeroed, sentinels intact."""
    out = oc.run_adamw(ref_ops, case)
    r = oc.check_adamw(out, case, oc.ORACLE_SHARE)
    print("OBS oracle %-40s p %.3f  m %.3f  v %.3f of the bound" % (case["name"], r["p"], r["m"], r["v"]))
    assert float(out["g"].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["lr1e-6-wd0.01-step2-trained", "clip-gm0.125", "n5", "offs123057"])
def test_oracle_adamw_g16_and_keep_gradient(ref_ops, name):
    case = [c for c in CASES if c["name"] == name][0]
    a = oc.run_adamw(ref_ops, case, zero_grad=False)
    assert torch.equal(oc.bits32(a["g"]), oc.bits32(a["g_before"]))
    oc.check_adamw(a, case, oc.ORACLE_SHARE)
    b = oc.run_adamw(ref_ops, case, zero_grad=False, use_g16=True)
    assert torch.equal(oc.bits32(b["g"]), oc.bits32(b["g_before"])) and float(b["g"][0]) == 7.0
    oc.check_adamw(b, case, oc.ORACLE_SHARE)
    p, m, v, g, ss = oc.adamw_inputs(case)
    c = oc.run_adamw(ref_ops, case, inputs=(p, m, v, g.to(BF16).float(), ss))
    for k in ("p", "m", "v"):
        assert torch.equal(oc.bits32(b[k]), oc.bits32(c[k])), k
    assert torch.equal(oc.bits16(b["p16"]), oc.bits16(c["p16"]))


def test_a_wrong_step_misses_the_bounds():
    """At production settings (lr 1e-6, where a whole update is about the size of an absolute tolerance of 1e-6): a skipped update, a doubled one, a
    missing bias correction - each is far outside the derived bound."""
    case = [c for c in CASES if c["name"] == "lr1e-6-wd0.01-step2-trained"][0]
    p, m, v, g, ss = oc.adamw_inputs(case)
    ref = oc.ref_adamw(p, m, v, g, case["lr"], case["wd"], case["step"], ss, case["max_norm"], case["gm"])
    delta = p.double() * (1 - case["lr"] * case["wd"]) - ref["p"]
    bc1 = 1 - oc.B1 ** case["step"]
    for what, wrong in (("skipped", ref["p"] + delta), ("twice", ref["p"] - delta), ("no bias correction 1", ref["p"] + delta * (1 - bc1))):
        r = oc.adamw_ratios(wrong.float(), ref["m"].float(), ref["v"].float(), ref)
        assert r["p"] > 20, (what, r)


@pytest.mark.parametrize("rot", oc.BF16_ROTATIONS)
def test_bf16_patterns(ref_ops, rot):
    """The table's expected patterns are round-to-nearest-even (torch's own conversion), and lr = wd = 0 with an empty state leaves p bit for bit."""
    p, want = oc.bf16_case(rot)
    assert torch.equal(oc.bits16(p.to(BF16)), want)
    case = oc._case("bf16-rot%d" % rot, oc.BF16_N, lr=0.0, wd=0.0, step=1, clip=None, gm=1.0)
    z = torch.zeros(oc.BF16_N)
    out = oc.run_adamw(ref_ops, case, inputs=(p, z, z.clone(), z.clone(), None))
    assert torch.equal(oc.bits32(out["p"]), oc.bits32(p)) and torch.equal(oc.bits16(out["p16"]), want)


def test_bf16_patterns_reach_every_lane_and_the_tail():
    k = len(oc.BF16_PATTERNS)
    body = (oc.BF16_N // 4) * 4
    lanes, tail = set(), set()
    for rot in oc.BF16_ROTATIONS:
        idx = (torch.arange(oc.BF16_N) + rot) % k
        lanes |= {(int(j), i % 4) for i, j in enumerate(idx[:body])}
        tail |= {int(j) for j in idx[body:]}
    assert lanes == {(j, l) for j in range(k) for l in range(4)} and tail == set(range(k)) and oc.BF16_N - body == 3


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("name,dtype,n,off", oc.sumsq_cases(), ids=[c[0] for c in oc.sumsq_cases()])
def test_exact_sum_data_stays_below_2_24_and_the_oracle_counts_it(ref_ops, name, dtype, n, off):
    x = oc.int_data(n, 100 + n % 97 + off, dtype)
    s = oc.exact_sumsq(x)
    assert n < 8 or s > 0
    assert torch.equal(x.float(), x.float().round()) and float(x.float().abs().max()) <= 2
    out = torch.tensor([oc.OUT0])
    ref_ops.sumsq_accum(x, out)
    assert float(out) == oc.OUT0 + s
    pos = oc.planted_positions(n, dtype)
    w = 4 if dtype == F32 else 8
    assert set(range((n // w) * w, n)) <= set(pos) and all(0 <= q < n for q in pos)
    if n > oc.GRID_PASS:
        assert (oc.SUMSQ_PASS_F32 if dtype == F32 else oc.SUMSQ_PASS_BF16) in pos or n // w * w <= oc.SUMSQ_PASS_BF16


def test_planted_positions_enter_a_later_grid_trip():
    n = 3 * oc.GRID_PASS + 1
    assert {oc.SUMSQ_PASS_F32, 2 * oc.SUMSQ_PASS_F32, 5 * oc.SUMSQ_PASS_F32, n - 1, n - 2} <= set(oc.planted_positions(n, F32))
    assert {oc.SUMSQ_PASS_BF16, 2 * oc.SUMSQ_PASS_BF16, n - 1, n - 2} <= set(oc.planted_positions(n, BF16))
    src = open(os.path.join(CSRC, "optim.hip")).read()
    # the grid caps the trip lengths are computed from
    assert "tr1_grid_1d(n / 4 + 1, 256, 2048)" in src and "tr1_grid_1d(n / 8 + 1, 256, 2048)" in src and src.count("tr1_grid_1d(n / 4 + 1, 256, 4096)") == 2


@pytest.mark.parametrize("n", oc.PARTIALS_N)
def test_partials_data_is_exact(n):
    buf, s = oc.partials_case(n)
    assert buf.numel() == n + 256 + oc.PAD and 0 <= s < oc.EXACT_LIMIT and (n < 8 or s > 0)


@pytest.mark.parametrize("case", oc.periodic_cases(), ids=[c[0] for c in oc.periodic_cases()])
def test_oracle_periodic_sum_and_zero(ref_ops, case):
    name, base, stride, count, ranges = case
    assert len(ranges) <= 8 and all(0 <= a <= b <= stride for a, b in ranges)
    for kind in ("in", "out", "mixed"):
        arena, mask, s = oc.periodic_arena(case, kind)
        assert (s == 0) == (kind == "out") and int(mask.sum()) == count * sum(b - a for a, b in ranges)
        out = torch.tensor([oc.OUT0])
        ref_ops.sumsq_ranges_periodic(arena, base, stride, count, ranges, out)
        assert float(out) == oc.OUT0 + s
    arena, mask, s = oc.periodic_arena(case, "mixed")
    before = arena.clone()
    ref_ops.zero_ranges_periodic(arena, base, stride, count, ranges)
    assert torch.equal(oc.bits32(arena[~mask]), oc.bits32(before[~mask])) and bool((oc.bits32(arena[mask]) == 0).all())


def test_periodic_cases_cover_what_they_claim():
    cs = oc.periodic_cases()
    assert {len(c[4]) for c in cs} >= {1, 3, 8} and {c[3] for c in cs} >= {1, 28, 80}
    assert all(c[1] % 4 for c in cs)
    assert any(a == b for c in cs for a, b in c[4]) and any(b - a > 64 * 256 for c in cs for a, b in c[4])


def test_wgrad_tile_height_replay_matches_the_launcher_source():
    """The replay is only worth something while it is the launcher's rule: pin the constants it copies."""
    flat, src = oc.launcher_source("tr1_wgrad_f32_sumsq", os.path.join(CSRC, "gemm.hip"))
    flat = flat[:flat.index("*n_partials = blocks * 8;") + 30]
    assert "const int64_t t2n = (N + BN2 - 1) / BN2;" in flat
    # K-major: start at 256 (256, 224, 288, 320); NT: start at 224 (224, 256, 288, 320) - the two branches of the replay
    assert "nt8p_pick_rt(M, t2n, b_kmajor ? 256 : 224)" in flat and flat.count("nt8p_pick_rt(") == 1
    assert "*n_partials = blocks * 8;" in flat
    import re
    whole = re.sub(r"\s+", " ", src)
    # the one table, the one cost and the one picker of the 8-wave tile height
    assert whole.count("static const double NT8P_EFF[4] = {0.94, 1.0, 1.025, 1.03};") == 1 and whole.count("{0.94, 1.0, 1.025, 1.03}") == 1
    assert "static double nt8p_cost(int64_t M, int64_t n_tiles, int64_t rows, double eff) { const int64_t t = ((M + rows - 1) / rows) * n_tiles; return (double)((t + 255) / 256) * 256.0 * (double)(rows * BN2) / eff; }" in whole
    assert "static int nt8p_pick_rt(int64_t M, int64_t n_tiles, int first) { int rt = first / 32; double best = nt8p_cost(M, n_tiles, first, NT8P_EFF[rt - 7]); for (int r = 7; r <= 10; ++r) { const double c = nt8p_cost(M, n_tiles, r * 32, NT8P_EFF[r - 7]); if (c < best) { best = c; rt = r; } } return rt; }" in whole
    assert re.search(r"#define BN2 256\b", src)


def test_wgrad_shapes_hit_every_tile_height():
    for N, K, Mp, T, bm in oc.WGRAD_SHAPES:
        for kmajor in (False, True):
            got = oc.wgrad_tile_rows(N, K, kmajor)
            assert got == bm, "(%d, %d, kmajor %d): the launcher now picks %d-row tiles, the table says %d - re-pick the shapes" % (N, K, kmajor, got, bm)
        assert N >= 512 and K >= 256 and K % 8 == 0 and Mp % 64 == 0 and T < Mp
        assert N % bm and K % 256, "partial tiles in both directions"
        from time_r1_amd.ops import HipOps
        assert 8 * ((N + bm - 1) // bm) * ((K + 255) // 256) <= HipOps.wgrad_sumsq_partials(N, K)
    assert {s[4] for s in oc.WGRAD_SHAPES} == {224, 256, 288, 320}


@pytest.mark.parametrize("shape", oc.WGRAD_SHAPES, ids=["%dx%d" % s[:2] for s in oc.WGRAD_SHAPES])
def test_wgrad_data_is_exact(shape):
    N, K, Mp, T, bm = shape
    dy, x, gw0, over, acc = oc.wgrad_case(N, K, Mp, T)
    for t in (dy[:T], x[:T], gw0):
        assert torch.equal(t, t.round()) and torch.equal(t.to(BF16).float(), t)
    assert float(dy[T:].abs().max()) == 0.0 and not torch.isfinite(x[T:]).all()
    for gw in (over, acc):
        s = oc.exact_sumsq(gw)
        assert s > (1 << 18) and torch.equal(gw.float().double(), gw)
    assert int((over != 0).sum()) > 1000 * ((N + bm - 1) // bm) * ((K + 255) // 256) // 8


@pytest.mark.parametrize("seed", range(200))
def test_lazy_zero_plan_partitions_the_arena(seed):
    """AdamW's own zeroing spans + the periodic small ranges + the kept matrices cover every index of the arena exactly once, and the spans the fused
    launches walk cover it exactly once on their own (what _norm_from_sink adds up: prefix and suffix, the small ranges, the matrices' epilogue sums)."""
    from time_r1_amd.optim import AdamWFlat
    n, lz = oc.random_plan(seed)
    o = AdamWFlat.__new__(AdamWFlat)
    o.lazy_zero, o.lazy_zero_ok = lz, None
    spans, small = o._zero_spans(n)
    assert len(small) <= 8
    walk = torch.zeros(n, dtype=torch.int32)
    for x, y, z in spans:
        assert 0 <= x < y <= n
        walk[x:y] += 1
    assert bool((walk == 1).all())
    assert [z for x, y, z in spans if x == lz["base"]] == [False]
    cover = oc.zero_plan_cover(n, spans, small, lz)
    assert bool((cover == 1).all()), (n, lz, spans, small)
    o.lazy_zero_ok = lambda: False          # plan withdrawn: one span, everything zeroed
    assert o._zero_spans(n) == ([(0, n, True)], None)


def test_random_plans_are_varied():
    plans = [oc.random_plan(s)[1] for s in range(200)]
    assert {p["count"] for p in plans} == {1, 2, 5, 28}
    assert any(p["keep"] and p["keep"][0][0] == 0 for p in plans) and any(p["keep"] and p["keep"][-1][1] == p["stride"] for p in plans)
    assert any(a[1] == b[0] for p in plans for a, b in zip(p["keep"], p["keep"][1:])) and any(p["base"] % 4 for p in plans)
    assert any(len(p["keep"]) == 7 for p in plans)
