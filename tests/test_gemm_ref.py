"""CPU: the cases of tests/gemm_cases.py are what they claim and the checker of tests/test_gemm_gpu.py is not blind.

1. Replays.  Every case names the kernel / tile height (and, for split-K, the split and its shares) it is there for; the launchers' choices are replayed
   (optim_cases._replay = nt8p_pick_rt, test_gemm_tile_heights.nt_takes_8wave = the NT dispatch, gemm_cases.splitk_pick = splitk_pick, whose text is pinned to
   csrc/gemm.hip) and a case that no longer reaches it fails with "re-pick".  The set of (form, kernel / height) pairs the issue lists must be reached.
2. Inputs.  Regime A: of the values before the bf16 rounding at least 5 % are not representable, at least 2 % are exact ties that round down to even and
   at least 2 % ties that round up; at most 0.5 % of a transcendental output lies within its evaluation error of a rounding boundary.
3. Mutants.  The checker rejects the reference with one fault planted, for every fault in every case it applies to.
Cases of more than 2048 rows are looked at on their first 352 and last 353 rows here (a fault rejected on some rows is rejected)."""
import pytest
import torch

import gemm_cases as gc
import optim_cases as oc

CASES = gc.CASES


def _subset(case):
    M = gc.dims(case)[0]
    if M <= gc.BIG_ROWS:
        return None
    return torch.cat([torch.arange(gc.MUT_ROWS), torch.arange(M - gc.MUT_ROWS - 1, M)])


def test_every_case_reaches_the_kernel_it_is_there_for():
    seen = set()
    for c in CASES:
        r = gc.reached(c)
        if c["form"] == "splitk":
            assert r == (c["reach"], c["S"], c["shares"]), "%s: the launcher gives %s - re-pick" % (c["name"], r)
            assert sum(c["shares"]) == c["K"] // 64 and c["S"] <= c["K"] // 64
            r = r[0]
        else:
            assert r == c["reach"], "%s reaches %s, not %s - re-pick" % (c["name"], r, c["reach"])
        if c["regime"] == "A":
            seen.add((c["form"] + ("-kmajor" if c.get("kmajor") else ""), r))
    want = {("nt", 128), ("splitk", 224), ("splitk-kmajor", 224), ("nnacc", 224)}
    want |= {(f, h) for f in ("nt", "nn", "qgelu", "glu", "rope", "vit", "glubwd") for h in (224, 256, 288, 320)}
    assert seen == want, "not reached: %s; not listed: %s" % (sorted(want - seen), sorted(seen - want))


def test_the_case_set_covers_what_the_issue_lists():
    A = [c for c in CASES if c["regime"] == "A"]
    nt128 = [c for c in A if c["form"] == "nt" and c["reach"] == 128]
    assert {c["K"] for c in nt128} == {64, 128, 192, 320}
    assert {c["M"] for c in nt128} == {1, 127, 129, 300} and {c["N"] for c in nt128} == {8, 136, 200, 264}
    assert {(c["out"], c["bias"], c["res"]) for c in nt128} >= {("bf16", False, False), ("bf16", True, False), ("bf16", False, True), ("bf16", True, True),
                                                                ("f32", False, False), ("f32", True, True), ("acc", True, False), ("acc", False, True)}
    assert all(c["K"] <= 192 or c["out"] == "acc" for c in nt128 if c["M"] <= 64) and any(c["M"] <= 64 and c["out"] == "acc" and c["K"] == 320 for c in nt128)
    for f in ("nn", "qgelu"):       # the 8-wave k loop, K-major and plain operand: the prologue alone, both buffers, both branches at both parities
        assert {c["K"] for c in A if c["form"] == f and c["M"] == 545} == {64, 128, 192, 320}
    assert all(c["K"] == 192 for c in A if c["form"] != "splitk" and c["reach"] in (256, 288, 320))
    assert {(c["K"], c["out"]) for c in A if c["form"] == "nnacc"} == {(192, "f32"), (192, "acc"), (320, "f32"), (320, "acc")}
    assert all(c["b_rows"] == c["K"] - 13 for c in A if c["form"] == "nnacc")
    assert {c["I"] for c in A if c["form"] == "glu" and c["M"] == 545} == {8, 136, 200, 264} and any(c["form"] == "glu" and c["M"] == 65 for c in A)
    assert {(c["nh"], c["nkv"]) for c in A if c["form"] == "rope" and c["M"] == 545} == {(2, 2), (4, 2), (6, 2)}
    assert {c["half"] for c in A if c["form"] == "vit" and c["M"] == 545} == {16, 40, 56}
    assert all((c["nh"] * c["half"]) % 128 == 0 for c in A if c["form"] == "vit")
    assert any(c["M"] == 257 for c in A if c["form"] == "rope") and any(c["M"] == 257 for c in A if c["form"] == "vit")
    bw = [c for c in A if c["form"] == "glubwd"]
    assert {c["M"] for c in bw if c["I"] == 264} >= {640, 641, 650, 672}
    odd288 = [c for c in bw if c["reach"] == 288]
    assert odd288 and all(((c["M"] + 287) // 288) % 2 == 1 and (c["M"] + 287) // 288 * 288 < (c["M"] + 63) // 64 * 64 for c in odd288)
    sk = [c for c in A if c["form"] == "splitk"]
    for km in (False, True):
        mine = [c for c in sk if c["kmajor"] == km]
        assert {2, 8} <= {c["S"] for c in mine}
        assert any(len(set(c["shares"])) > 1 for c in mine) and any(1 in c["shares"] for c in mine)
        assert all(c["M"] == 300 and c["N"] == 264 and c["bias"] and c["res"] for c in mine)
    B = [c for c in CASES if c["regime"] == "B"]
    assert all(c["K"] <= 512 for c in B)
    assert {c["form"] for c in B} >= {"nt", "glu", "qgelu", "rope", "vit", "glubwd"} and any(c["out"] in ("f32", "acc") for c in B)


def test_the_splitk_replay_copies_the_launcher():
    body, src = oc.launcher_source("tr1_gemm_splitk_bf16", gc.GEMM_HIP)
    flat = " ".join(src.split())
    for text in gc.SPLITK_TEXT + gc.KERNEL_SHARE_TEXT:
        assert text in flat, text
    for text in gc.SPLITK_LAUNCHER_TEXT:
        assert text in body, text
    assert "static const double NT8P_EFF[4] = {0.94, 1.0, 1.025, 1.03};" in flat and gc.EFF == (0.94, 1.0, 1.025, 1.03)
    assert 'extern "C" int64_t tr1_gemm_splitk_max_splits(void) { return 8; }' in flat
    # S never exceeds the k tiles, with the forcing line included
    for nk in range(2, 40):
        for max_s in range(2, 9):
            _, S, shares = gc.splitk_pick(300, 264, 64 * nk, max_s)
            assert 2 <= S <= min(nk, max_s) and len(shares) == S and min(shares) >= 1 and sum(shares) == nk


def test_the_rounding_helpers():
    src = torch.tensor([a for a, _ in oc.BF16_PATTERNS if (a & 0x7F800000) != 0x7F800000 and 0x00800000 <= (a & 0x7FFFFFFF) < 0x7F000000], dtype=torch.int64)
    v = src.to(torch.int32).view(torch.float32).double()
    want = torch.tensor([b for a, b in oc.BF16_PATTERNS if (a & 0x7F800000) != 0x7F800000 and 0x00800000 <= (a & 0x7FFFFFFF) < 0x7F000000], dtype=torch.int32)
    assert torch.equal(gc.bits16(gc.rne(v)).to(torch.int32) & 0xFFFF, want)
    assert torch.equal(gc.bits16(gc.rne_exact(v)), gc.bits16(gc.rne(v)))
    x = torch.tensor([1.00390625 + 2.0 ** -30, 1.00390625 - 2.0 ** -30, 1.00390625, 1.01171875, -1.01171875], dtype=torch.float64)   # around ties: fp64 values that
    assert gc.rne(x).double().tolist() == [1.0078125, 1.0, 1.0, 1.015625, -1.015625]                                                # double rounding would get wrong
    assert gc.trunc_bf16(x).double().tolist() == [1.0, 1.0, 1.0, 1.0078125, -1.0078125]
    assert gc.away_bf16(x).double().tolist()[2:] == [1.0078125, 1.015625, -1.015625]
    got = torch.tensor([1.0078125, 1.0078125, 1.015625], dtype=torch.bfloat16)
    ok, exc = gc.window_ok(got, torch.tensor([1.00390625 - 1e-9, 1.00390625 - 1e-6, 1.004], dtype=torch.float64), torch.full((3,), 1e-8, dtype=torch.float64))
    assert ok.tolist() == [True, False, False] and exc.tolist() == [True, False, False]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_inputs_exercise_the_rounding_and_the_checker_rejects_every_mutant(case):
    inp = gc.build(case)
    rows = _subset(case)
    ref = gc.reference(case, gc._rows(case, inp, rows))
    A = case["regime"] == "A"
    if A and case["out"] == "bf16":
        nr, down, up = gc.rounding_shares(ref["aux"]["pre"])
        print("OBS %-40s not representable %.3f, ties down %.3f, up %.3f" % (case["name"], nr, down, up))
        assert nr >= 0.05 and down >= 0.02 and up >= 0.02, (case["name"], nr, down, up)
    if A:
        for k, share in gc.window_shares(case, inp, rows).items():
            print("OBS %-40s %s: %.5f of the elements within E of a rounding boundary" % (case["name"], k, share))
            assert share <= gc.EXCUSE_CAP, (case["name"], k, share)
        if case["form"] in ("glu", "qgelu"):
            assert float(ref["aux"]["pre"].abs().max()) <= 16.0
        if case["form"] in ("rope", "vit"):
            cs = torch.stack([inp["cos"], inp["sin"]], -1)
            for pair in ((1.0, 0.0), (0.0, 1.0), (0.0, -1.0)):
                assert bool((cs == torch.tensor(pair, dtype=torch.float64)).all(-1).all(-1).any()), "no row with (c, s) = %s" % (pair,)
    # the reference itself passes its checker
    good = gc.fake_outputs(case, inp, None, rows)
    gc.check(case, inp, good, rows)
    for mut in gc.MUTANTS:
        if not gc.applies(mut, case):
            continue
        bad = gc.fake_outputs(case, inp, mut, rows)
        with pytest.raises(AssertionError):
            gc.check(case, inp, bad, rows)
            print("BLIND %s %s" % (case["name"], mut))


def test_every_mutant_applies_somewhere():
    for mut in gc.MUTANTS:
        assert any(gc.applies(mut, c) for c in CASES if c["regime"] == "A"), mut
