"""GPU: the training GEMMs of csrc/gemm.hip and their fused epilogues against the fp64 references of tests/gemm_cases.py, through the C ABI.

Cases, references, the derivation of every bound and the checker live in gemm_cases.py; tests/test_gemm_ref.py shows on the CPU that every case reaches the
kernel and tile height it names, that the inputs exercise the bf16 rounding (values that are not representable, ties of both kinds) and that the checker
rejects fifteen planted faults.  Regime A (dyadic operands) compares bit patterns; the transcendental outputs may differ from the rounded fp64 value only
where that value lies within the fp32 evaluation error of a rounding boundary, and the number of elements passed that way is printed (`pytest -s`, lines
starting with OBS) and capped at 0.5 %.  Regime B (gaussian operands, K <= 512) holds the derived worst-case bound of fp32 accumulation.

Seen on MI355X: every regime-A comparison bit-exact (128 x 128 kernel, 8-wave kernel at 224 / 256 / 288 / 320 rows through every entry point, K-major operand,
split-K at S = 2, 6, 8 with equal, unequal and one-tile shares).  Passed by the window, regime A: QuickGELU 0 of 41.0 M elements, SwiGLU 0 of 20.7 M, SwiGLU
backward gate half 795 and up half 246 of 41.7 M each (1.9e-5 and 0.6e-5; cap 5e-3).  Regime B, error as a share of the bound: bf16 output 0.94 .. 0.99
(the bound is half a bf16 step at a value just above a power of two), fp32 output 0.005 .. 0.008; epilogues: 0 .. 28 elements per output outside the rounded
fp64 value, all inside the window.

Checked against an edited copy of gemm.hip (not kept): QuickGELU on the unrounded projection fails qgelu-A-545x264x192 (the one case run); without the branch that zero-fills the 32
columns past a row-tile end, dgu^T fails at M = 641, 650, 672 and passes at M = 640 (no padding).

Every operand is a strided view between values that must not be read (3e38, inf: a read shows as inf / NaN), every output a view inside a sentinel frame
that must keep its bits; the split-K workspace starts as NaN."""
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PLAIN = [c for c in gc.CASES if c["form"] != "splitk"]
SPLITK = [c for c in gc.CASES if c["form"] == "splitk"]


def _report(case, excused, outs):
    n = {k: v.numel() for k, v in outs.items()}
    if case["regime"] == "A":
        what = "bit-exact" if not excused else "GEMM part bit-exact; activation passed by the window: " + ", ".join("%s %d" % kv for kv in sorted(excused.items()))
    else:
        what = ", ".join(("%s %.3f" if isinstance(v, float) else "%s %d excused") % (k, v) for k, v in sorted(excused.items()))
    print("OBS gemm %-44s %s  (%s elements)" % (case["name"], what, "+".join(str(v) for v in n.values())))


@pytest.mark.parametrize("case", PLAIN, ids=lambda c: c["name"])
def test_gemm_against_fp64(hip_ops, case):
    inp = gc.build(case)
    outs = gc.launch(hip_ops, case, inp, DEV)
    excused = gc.check(case, inp, outs)
    _report(case, excused, outs)


@pytest.mark.parametrize("case", SPLITK, ids=lambda c: c["name"])
def test_splitk_against_fp64_twice(hip_ops, case):
    """The same launch into two differently poisoned outputs and NaN workspaces (the second with room for a fraction of one more plane, which must not change the
    split): both bit-equal to the exact value, hence to each other."""
    inp = gc.build(case)
    first = gc.launch(hip_ops, case, inp, DEV, poison=0)
    second = gc.launch(hip_ops, case, inp, DEV, poison=1, ws_extra=case["M"] * case["N"] // 2)
    assert torch.equal(gc.bits16(first["c"]), gc.bits16(second["c"])), case["name"] + ": two runs differ"
    gc.check(case, inp, first, poison=0)
    gc.check(case, inp, second, poison=1)
    print("OBS gemm %-44s bit-exact twice: S = %d, k tiles per share %s" % (case["name"], case["S"], case["shares"]))


@pytest.mark.parametrize("kmajor", [0, 1], ids=["nt", "kmajor"])
def test_splitk_rejects_a_single_k_tile(hip_ops, kmajor):
    """K = 64 cannot be split: the launcher returns an error before any launch (a share of no tiles would still stage one, past the end of every row)."""
    from time_r1_amd import hip
    M, N, K = 300, 264, 64
    a = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros((K, N) if kmajor else (N, K), dtype=torch.bfloat16, device=DEV)
    c = torch.full((M, N), 5.0, dtype=torch.bfloat16, device=DEV)
    ws = torch.full((2 * M * N,), 7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(hip.HipError, match="K >= 128"):
        hip_ops.L.call("tr1_gemm_splitk_bf16", a.data_ptr(), b.data_ptr(), c.data_ptr(), 0, 0, M, N, K, a.stride(0), b.stride(0), c.stride(0), 0, kmajor,
                       ws.data_ptr(), ws.numel(), hip_ops._s())
    torch.cuda.synchronize()
    assert bool((c == 5.0).all()) and bool((ws == 7.0).all()), "nothing may have been launched"
