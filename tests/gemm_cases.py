"""Cases, fp64 references, checker and mutants for the training GEMMs of csrc/gemm.hip: the 128 x 128 kernel (gemm_nt_kernel), the phased 8-wave kernel
(gemm_nt8p_kernel) at its four tile heights and with the K-major operand, the fused epilogues EPI 2 / 3 / 4 / 5 / 7 and the split-K form (EPI 6 with
splitk_reduce_kernel).  Shared by tests/test_gemm_ref.py (CPU: the conditions on the inputs, the replays of the launchers' choices, the mutants) and
tests/test_gemm_gpu.py (the HIP kernels on the same cases).  Plain torch on the CPU, written from the formulas; nothing here calls oracle/ref_ops.py.

A. DYADIC operands (the pin).  A[m, k] = ia 2^(ea[m] + p), B[n, k] = ib 2^eb[n] with dense integers ia, ib in [-8, 8] and exponents ea, eb in -2 .. 2, so
every output element has its own unit G[m, n] = 2^(ea[m] + eb[n] + p).  bias[n] = i 2^(eb[n] + p + 2) (a multiple of every row's unit, at most 128 units),
residual[m, n] = i G[m, n], C0[m, n] = i G[m, n].  In units of G every product is an integer of at most 64, so sum_k |a_k b_k| + |bias| + |residual| + |C0|
<= 64 K + 144 < 2^24 (asserted; K up to 2^18): every fp32 partial sum, in any order, split or MFMA grouping, is an integer below 2^24 units and therefore
exact.  The value before rounding is ONE number, S + bias + residual, taken from an fp64 matmul (exact as well); a bf16 output is its round-to-nearest-even,
an fp32 output the number itself.  Comparisons are on bit patterns.  p is a per-case power of two that keeps the gate of an activation within |g| <= 16.
   The rotary forms take cos / sin from {0, +-1, +-1/2, +-1/4, +-3/4}: RNE(p_a) c - RNE(p_b) s is then exact in fp32 too (asserted), with or without
contraction into an fma, and q / k / v are bit-exact.  (The sign of a zero is not compared: -0 == +0.)

B. GAUSSIAN operands (K <= 512), randn rounded to bf16 once.  fp32 accumulation of K products and the bias / residual additions, in any order, is off by at
most E = (K + 2) 2^-24 (sum_k |a_k b_k| + |bias| + |residual|) from the fp64 value c (first order, counts rounded up).  fp32 output: |got - c| <= E, plus
one rounding 2^-24 |C0 + c| when accumulating.  bf16 output: |got - c| <= U (|c| + E) + E with U = 2^-8.  Where an epilogue consumes the rounded projection
without storing it, both bf16 neighbours of c are admissible inputs when c lies within E of the boundary between them.

Transcendental epilogues.  The kernel evaluates the activation in fp32 on bf16 inputs and rounds once (RNE) to bf16.  With v the fp64 value and E a bound of
the fp32 evaluation error, the stored bf16 is RNE(v) - or the other neighbour, but then only if v lies within E of the boundary between the two.  The checker
accepts exactly that ("window": where E reaches half a bf16 step at v, a value that cancels, any RNE of an fp32 within E of v), counts the elements it passes by the window, and test_gemm_ref.py asserts from v alone that at most 0.5 % of a regime-A
output could be passed that way (regime B adds the GEMM's E to the window; at K = 192 .. 512 that window is a few per cent wide by construction, so the cap
is asserted for regime A and the count is printed for B).  Regime B, sums that cancel: where E reaches half a bf16 step of c more than two roundings of the
projection are admissible; those elements (about 3 % at K = 256) are held to the plain bound instead - the output is the RNE of an fp32 value within
D = L (E + U (|c| + E)) + E_f of f(c), L the slope of the epilogue in the projection (1.1 for QuickGELU, |u F| and |g sg| for the backward, |cos|, |sin| for
the rotation).  u = 2^-24, first order:
  __expf(x) = exp2(fl(x log2 e)) on v_exp_f32: the argument carries <= |x| log2e 1.5u absolute (the constant's and the product's rounding), a relative
       error <= 1.04 |x| u, bounded by 1.5 |x| u, in the result; the hardware exp2 adds 1 ulp <= 2u relative - ASSUMED (no documented figure).  Taken
       with a margin of two over that sum:  r_exp(x) = (4 + 3 |x|) u.
  a division is counted 2.5u (correctly rounded in the default build; the margin covers an rcp-based lowering), every other operation u.
  sg = 1 / (1 + e), e = __expf(-g), w = e / (1 + e) = 1 - sigmoid(g):   r_sg = w r_exp(g) + 3.5u   (e's error weighted into the sum, the sum, the division)
  silu(g) = g / (1 + e):  the same count                                 E = |v| r_sg
  SwiGLU (EPI 2): s = RNE(silu(g)), a = RNE(s u); s u is exact in fp32 (two bf16 factors).  a is accepted iff a == RNE(s' u) for an admissible s': RNE of the
       fp64 silu, or its other neighbour when inside the window.
  QuickGELU (EPI 5) on x = RNE(projection + bias): t = fl(-1.702f x) (u relative, i.e. |t| u more in e), y = x / (1 + __expf(t)), W = 1 / (1 + exp(1.702f x)):
       E = |v| (W (r_exp(t) + |t| u) + 3.5u), the reference uses the fp32 value of 1.702.
  SwiGLU backward (EPI 3, store_acc256_glubwd) on d = RNE(da):  ru = d (g sg): E_u = |v| (r_sg + 2u).
       rg = (d u) F, F = sg (1 + g (1 - sg)); d u is exact.  F cancels near g = -1.278, so its error is carried as an ABSOLUTE one:
       d1 = sg r_sg + u |1 - sg|;  d2 = |g| d1 + u |g (1 - sg)|;  d3 = d2 + u |1 + g (1 - sg)|;  dF = sg r_sg |1 + g (1 - sg)| + sg d3 + u |F|;
       E_g = |d u| dF + u |d u F|.
  rotary, regime B (real fp32 cos / sin): x c - y s in fp32 is off by at most 2u (|x c| + |y s|).
"""
import functools
import os

import numpy as np
import torch

import optim_cases as oc
from optim_cases import BF16, F32, F64, PLANT_BIG, bits16, bits32, frame_intact, framed

U = 2.0 ** -24
U_BF16 = 2.0 ** -8
EXCUSE_CAP = 0.005
GEMM_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "time-r1_amd", "csrc", "gemm.hip")
QG_C = float(np.float32(1.702))
ROT_SET = (0.0, 1.0, -1.0, 0.5, -0.5, 0.25, -0.25, 0.75, -0.75)


# ---------------------------------------------------------------------------------------------------------------- rounding
def _key(b):
    """bf16 -> an integer that orders like the value; neighbours differ by 1; +-0 -> 0."""
    i = bits16(b).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _from_key(k):
    i = torch.where(k < 0, (-k) | 0x8000, k)
    return torch.where(i >= 0x8000, i - 0x10000, i).to(torch.int16).view(BF16)


def exact32(v):
    return bool((v.to(F32).double() == v).all())


def rne_exact(v):
    """RNE to bf16 of fp64 values that fp32 represents exactly (then fp32 -> bf16 is the single rounding)."""
    return v.to(F32).to(BF16)


def rne(v):
    """RNE to bf16 of any fp64 value: the nearest of the three bf16 around the double-rounded one, ties to the even pattern."""
    b = v.to(F32).to(BF16)
    k = _key(b)
    best, bd = b, (b.double() - v).abs()
    for c in (_from_key(k - 1), _from_key(k + 1)):
        d = (c.double() - v).abs()
        take = (d < bd) | ((d == bd) & ((bits16(c) & 1) == 0) & ((bits16(best) & 1) == 1))
        best, bd = torch.where(take, c, best), torch.where(take, d, bd)
    return best


def trunc_bf16(v):
    """Mutant: the low 16 bits of the fp32 pattern dropped."""
    return (bits32(v.to(F32)) & -65536).view(F32).to(BF16)


def away_bf16(v):
    """Mutant: round half away from zero (add half an ulp to the magnitude, then truncate)."""
    return ((bits32(v.to(F32)) + 0x8000) & -65536).view(F32).to(BF16)


def rounding_shares(pre):
    """Of values exact in fp32: share not representable in bf16, share of exact ties that round down to even, that round up to even."""
    i = bits32(pre.to(F32))
    low, odd = i & 0xFFFF, (i >> 16) & 1
    n = float(pre.numel())
    tie = low == 0x8000
    return float((low != 0).sum()) / n, float((tie & (odd == 0)).sum()) / n, float((tie & (odd == 1)).sum()) / n


def other_neighbour(v, r):
    """The bf16 next to r = RNE(v) on v's side, and the boundary between the two."""
    alt = _from_key(_key(r) + torch.where(v >= r.double(), 1, -1))
    return alt, (alt.double() + r.double()) / 2


def window_ok(got, v, E):
    """-> (ok, excused): got == RNE(v), or got is the neighbour across a boundary that v lies within E of."""
    r = rne(v)
    kg, kr = _key(got), _key(r)
    same = kg == kr
    exc = ~same & ((kg - kr).abs() == 1) & (((got.double() + r.double()) / 2 - v).abs() <= E)
    if not bool((same | exc).all()):        # a value that cancels (E of at least half a bf16 step at v): any bf16 that is the RNE of an fp32 within E of v
        exc = exc | (~same & _wide(v, E) & _loose(got, v, E))
    return same | exc, exc


def near_share(v, E):
    """Share of elements whose fp64 value lies within E of a bf16 rounding boundary (what the window could excuse)."""
    r = rne(v)
    k = _key(r)
    up, dn = (_from_key(k + 1).double() + r.double()) / 2, (_from_key(k - 1).double() + r.double()) / 2
    return float((torch.minimum((up - v).abs(), (v - dn).abs()) <= E).sum()) / v.numel()


# ---------------------------------------------------------------------------------------------------------------- activations (fp64 + fp32 error bounds)
def r_exp(x):
    return (4.0 + 3.0 * x.abs()) * U


def silu64(g):
    """-> (v, E) of g / (1 + exp(-g))."""
    w = torch.sigmoid(-g)
    v = g * torch.sigmoid(g)
    return v, v.abs() * (w * r_exp(g) + 3.5 * U)


def quickgelu64(x):
    t = QG_C * x
    v = x * torch.sigmoid(t)
    return v, v.abs() * (torch.sigmoid(-t) * (r_exp(t) + t.abs() * U) + 3.5 * U)


def glubwd64(d, g, u):
    """-> (vg, Eg, vu, Eu) of the two formulas of store_acc256_glubwd on d = RNE(da), g, u (fp64 views of bf16 values)."""
    sg, w = torch.sigmoid(g), torch.sigmoid(-g)
    r_sg = w * r_exp(g) + 3.5 * U
    vu = d * (g * sg)
    Eu = vu.abs() * (r_sg + 2 * U)
    inner = 1.0 + g * w
    F = sg * inner
    d1 = sg * r_sg + U * w
    d2 = g.abs() * d1 + U * (g * w).abs()
    d3 = d2 + U * inner.abs()
    dF = sg * r_sg * inner.abs() + sg * d3 + U * F.abs()
    P = d * u
    return P * F, P.abs() * dF + U * (P * F).abs(), vu, Eu


def swiglu_check(a, g, u):
    """a (bf16) against RNE(s' u) for the admissible s' -> (ok, excused)."""
    v, E = silu64(g)
    s0 = rne(v)
    s1, mid = other_neighbour(v, s0)
    adm = (v - mid).abs() <= E
    a0, a1 = rne_exact(s0.double() * u), rne_exact(s1.double() * u)
    k = _key(a)
    same = k == _key(a0)
    exc = ~same & adm & (k == _key(a1))
    return same | exc, exc


# ---------------------------------------------------------------------------------------------------------------- replays of the launchers
EFF = (0.94, 1.0, 1.025, 1.03)


def tile_rows(M, cols, first=256):
    """nt8p_pick_rt for M rows x ceil(cols / 256) column tiles (optim_cases._replay; first = 224: the NT dispatch, 256: every other form)."""
    return oc._replay(M, cols, first == 256)


def nt_kernel(M, N, K, accumulate):
    """What tr1_gemm_nt_bf16 launches: "skinny" (out of scope), 128 (gemm_nt_kernel) or the 8-wave tile height."""
    import test_gemm_tile_heights as th
    if M <= 64 and not accumulate and K >= 256:
        return "skinny"
    return tile_rows(M, N, 224) if th.nt_takes_8wave(M, N) else 128


def splitk_pick(M, N, K, max_s):
    """Replay of splitk_pick + the launcher's `S >= 2` -> (tile rows, S, k tiles of every share)."""
    t2n, nk = (N + 255) // 256, K // 64
    best, brt, bs = 1e300, 8, 1
    for r in range(7, 11):
        S = 1
        while S <= max_s and S <= nk:
            blocks = ((M + r * 32 - 1) // (r * 32)) * t2n * S
            rounds, kshare = float((blocks + 255) // 256), float((nk + S - 1) // S)
            c = rounds * (r * 32) * kshare / EFF[r - 7] + (0.02 * S * float(M * N) / 256.0 / 64.0 if S > 1 else 0.0)
            if c < best:
                best, brt, bs = c, r, S
            S += 1
    S = max(bs, 2)
    q, r = divmod(nk, S)
    return brt * 32, S, [q + (1 if z < r else 0) for z in range(S)]


SPLITK_TEXT = ("for (int r = 7; r <= 10; ++r) for (int S = 1; S <= max_s && S <= nk; ++S) {",
               "const int64_t tiles = ((M + r * 32 - 1) / (r * 32)) * t2n, blocks = tiles * S;",
               "const double rounds = (double)((blocks + 255) / 256), kshare = (double)((nk + S - 1) / S);",
               "const double c = rounds * (r * 32) * kshare / NT8P_EFF[r - 7] + (S > 1 ? 0.02 * S * (double)(M * N) / 256.0 / 64.0 : 0.0);",
               "if (c < best) { best = c; brt = r; bs = S; }")
SPLITK_LAUNCHER_TEXT = ("const int64_t max_s = ws_floats / (M * N);", "splitk_pick(M, N, K, (int)(max_s < 8 ? max_s : 8), &rt, &S);", "if (S < 2) S = 2;",
                        'TR1_CHECK_ARG(K >= 2 * BK, "gemm_splitk: K >= 128 required', 'TR1_CHECK_ARG(S <= K / BK,')
KERNEL_SHARE_TEXT = ("const int nk_all = (int)(K / BK), q = nk_all / ep.i0, r = nk_all - q * ep.i0;",
                     "const int64_t k0 = (int64_t)(kz * q + (kz < r ? kz : r)) * BK;", "K = (int64_t)(q + (kz < r ? 1 : 0)) * BK;")


# ---------------------------------------------------------------------------------------------------------------- cases
def C(form, name, regime="A", **kw):
    d = dict(form=form, regime=regime, bias=False, res=False, out="bf16")
    d.update(kw)
    d["name"] = "%s-%s-%s" % (form, regime, name)
    return d


def _nt(M, N, K, out="bf16", bias=False, res=False, reach=128, regime="A"):
    tag = "%dx%dx%d-%s%s%s" % (M, N, K, out, "-bias" if bias else "", "-res" if res else "")
    return C("nt", tag, regime, M=M, N=N, K=K, out=out, bias=bias, res=res, reach=reach)


def cases():
    """Every case: `reach` is the kernel / tile height the case claims (test_gemm_ref.py replays the launcher: "re-pick" when it no longer holds)."""
    c = []
    # ---- the 128 x 128 kernel through tr1_gemm_nt_bf16: K = 64 / 128 / 192 / 320 (1, 2, 3, 5 k tiles), ragged M and N, every output form
    c += [_nt(1, 8, 64), _nt(1, 136, 320, "acc"), _nt(127, 136, 128, bias=True), _nt(129, 200, 192, res=True), _nt(300, 264, 320, bias=True, res=True),
          _nt(300, 264, 64, "f32", True, True), _nt(129, 264, 128, "f32"), _nt(300, 200, 192, "acc", bias=True), _nt(127, 8, 320, "acc", res=True),
          _nt(1, 264, 192, bias=True, res=True), _nt(300, 136, 320), _nt(127, 200, 64, bias=True, res=True)]
    # ---- the 8-wave kernel through the NT dispatch, one shape per tile height, three k tiles
    c += [_nt(7169, 1032, 192, bias=True, res=True, reach=224), _nt(11425, 1032, 192, "f32", bias=True, reach=256),
          _nt(13057, 1032, 192, "acc", res=True, reach=288), _nt(14689, 1032, 192, reach=320)]
    # ---- K-major operand (tr1_gemm_nn_bf16) and the plain NT operand of the 8-wave kernel (QuickGELU form): the k loop at 1, 2, 3, 5 k tiles
    for K in (64, 128, 192, 320):
        c.append(C("nn", "545x264x%d" % K, M=545, N=264, K=K, reach=224))
        c.append(C("qgelu", "545x264x%d" % K, M=545, N=264, K=K, bias=(K != 128), reach=224))
    for M, h in ((11425, 256), (13057, 288), (14689, 320)):
        c.append(C("nn", "%dx1032x192" % M, M=M, N=1032, K=192, reach=h))
        c.append(C("qgelu", "%dx1032x192" % M, M=M, N=1032, K=192, bias=True, reach=h))
    # ---- K-major fp32 forms (the weight gradient's shape: K = padded tokens, the last 13 rows of B unreadable)
    for Mp in (192, 320):
        for out in ("f32", "acc"):
            c.append(C("nnacc", "545x264x%d-%s" % (Mp, out), M=545, N=264, K=Mp, b_rows=Mp - 13, out=out, reach=224))
    # ---- gate/up + SwiGLU (EPI 2)
    for I in (8, 136, 200, 264):
        c.append(C("glu", "545xI%dx192" % I, M=545, I=I, K=192, bias=(I in (136, 264)), save_gu=(I != 200), reach=224))
    c.append(C("glu", "65xI264x128", M=65, I=264, K=128, bias=False, save_gu=True, reach=224))
    for M, h in ((11425, 256), (13057, 288), (14689, 320)):
        c.append(C("glu", "%dxI520x192" % M, M=M, I=520, K=192, bias=(h == 288), save_gu=True, reach=h))
    # ---- q|k|v + bias + M-RoPE (EPI 4)
    for nh, nkv in ((2, 2), (4, 2), (6, 2)):
        c.append(C("rope", "545-h%d-kv%d-192" % (nh, nkv), M=545, nh=nh, nkv=nkv, K=192, bias=True, reach=224))
    c.append(C("rope", "257-h4-kv2-128", M=257, nh=4, nkv=2, K=128, bias=True, reach=224))
    for M, h in ((11425, 256), (13057, 288), (14689, 320)):
        c.append(C("rope", "%d-h6-kv2-192" % M, M=M, nh=6, nkv=2, K=192, bias=True, reach=h))
    # ---- vision q|k|v + bias + rotary into padded heads (EPI 7)
    for half, nh in ((16, 8), (40, 16), (56, 16)):
        c.append(C("vit", "545-half%d-h%d-192" % (half, nh), M=545, nh=nh, half=half, K=192, bias=True, reach=224))
    c.append(C("vit", "257-half40-h16-64", M=257, nh=16, half=40, K=64, bias=True, reach=224))
    for M, h in ((3809, 256), (4353, 288), (4897, 320)):
        c.append(C("vit", "%d-half40-h16-192" % M, M=M, nh=16, half=40, K=192, bias=True, reach=h))
    # ---- down-projection dgrad + SwiGLU backward (EPI 3) with dgu^T
    for M in (640, 641, 650, 672):
        c.append(C("glubwd", "%dxI264x192" % M, M=M, I=264, K=192, reach=224))
    c.append(C("glubwd", "545xI264x320", M=545, I=264, K=320, reach=224))
    for M, h in ((11425, 256), (13516, 288), (14689, 320)):
        c.append(C("glubwd", "%dxI1032x192" % M, M=M, I=1032, K=192, reach=h))
    # ---- split-K (EPI 6 + splitk_reduce_kernel): (k tiles, workspace planes) -> S and the shares by the replay
    for nk, max_s, S, shares in ((2, 2, 2, [1, 1]), (3, 2, 2, [2, 1]), (8, 8, 8, [1] * 8), (15, 8, 8, [2] * 7 + [1]), (17, 8, 6, [3] * 5 + [2])):
        for km in (False, True):
            c.append(C("splitk", "300x264-nk%d-ws%d-%s" % (nk, max_s, "kmajor" if km else "nt"), M=300, N=264, K=64 * nk, kmajor=km, max_s=max_s, S=S,
                       shares=shares, bias=True, res=True, reach=224))
    # ---- regime B (K <= 512)
    c += [_nt(300, 264, 512, bias=True, res=True, regime="B"), _nt(300, 264, 320, "f32", bias=True, regime="B"), _nt(129, 200, 192, "acc", res=True, regime="B"),
          _nt(7169, 1032, 128, bias=True, reach=224, regime="B")]
    c.append(C("nn", "545x264x320", "B", M=545, N=264, K=320, reach=224))
    c.append(C("glu", "545xI264x256", "B", M=545, I=264, K=256, bias=True, save_gu=True, reach=224))
    c.append(C("qgelu", "545x264x256", "B", M=545, N=264, K=256, bias=True, reach=224))
    c.append(C("rope", "545-h4-kv2-256", "B", M=545, nh=4, nkv=2, K=256, bias=True, reach=224))
    c.append(C("vit", "545-half40-h16-128", "B", M=545, nh=16, half=40, K=128, bias=True, reach=224))
    c.append(C("glubwd", "641xI264x256", "B", M=641, I=264, K=256, reach=224))
    return c


CASES = cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
BIG_ROWS = 2048                    # cases with more rows: the CPU-only checks (shares, mutants) look at the first and last MUT_ROWS rows
MUT_ROWS = 352


def dims(case):
    """-> (M, N of the GEMM, K)."""
    f = case["form"]
    if f in ("glu",):
        return case["M"], 2 * case["I"], case["K"]
    if f == "glubwd":
        return case["M"], case["I"], case["K"]
    if f == "rope":
        return case["M"], (case["nh"] + 2 * case["nkv"]) * 128, case["K"]
    if f == "vit":
        return case["M"], 6 * case["nh"] * case["half"], case["K"]
    return case["M"], case["N"], case["K"]


def reached(case):
    """What the launcher does with the case, replayed."""
    M, N, K = dims(case)
    if case["form"] == "nt":
        return nt_kernel(M, N, K, case["out"] == "acc")
    if case["form"] == "splitk":
        rows, S, shares = splitk_pick(M, N, K, case["max_s"])
        return rows, S, shares
    return tile_rows(M, N, 256)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _ints(shape, gen, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case["name"])) % 100003


@functools.lru_cache(maxsize=2)
def _build(name):
    """The case's inputs.  Regime A, bf16 output: the first seed whose values before rounding meet the shares that test_gemm_ref.py asserts (a 1 x 8 output
    needs a few tries to hold a tie of each kind; every case of more than a few hundred outputs takes its first seed)."""
    case = BY_NAME[name]
    for attempt in range(500):
        inp = _make(case, _seed(case) + 7919 * attempt)
        if case["regime"] != "A" or case["out"] != "bf16":
            return inp
        pre = inp["S"] + (inp["bias"] if inp["bias"] is not None else 0.0) + (inp["res"] if inp["res"] is not None else 0.0)
        nr, down, up = rounding_shares(pre)
        if nr >= 0.05 and down >= 0.02 and up >= 0.02:
            return inp
    raise AssertionError("%s: no seed meets the rounding shares" % name)


def _make(case, seed):
    name = case["name"]
    f, A_ = case["form"], case["regime"] == "A"
    M, N, K = dims(case)
    gen = torch.Generator().manual_seed(seed)
    kv = case.get("b_rows", K)                                      # valid k range
    if A_:
        ea, eb = _ints((M,), gen, -2, 2), _ints((N,), gen, -2, 2)
        a, b = _ints((M, K), gen) * torch.exp2(ea)[:, None], _ints((N, K), gen) * torch.exp2(eb)[:, None]
        G = torch.exp2(ea)[:, None] * torch.exp2(eb)[None, :]
        bias = _ints((N,), gen) * torch.exp2(eb + 2) if case["bias"] else None
        res = _ints((M, N), gen) * G if case["res"] else None
        c0 = _ints((M, N), gen) * G if case["out"] == "acc" else None
        assert 64 * K + 128 + 8 + 8 < oc.EXACT_LIMIT, "the exactness condition of regime A"
    else:
        assert K <= 512
        rb = lambda *s: torch.randn(*s, generator=gen).to(BF16).double()
        a, b = rb(M, K), rb(N, K) * (0.25 if f in ("glu", "qgelu") else 1.0)
        bias = rb(N) if case["bias"] else None
        res = rb(M, N) * 4 if case["res"] else None
        c0 = torch.randn(M, N, generator=gen).to(F32).double() * 8 if case["out"] == "acc" else None
    a[:, kv:] = 0
    S = a[:, :kv] @ b[:, :kv].t()
    inp = dict(a=a, b=b, bias=bias, res=res, c0=c0, kv=kv)
    if A_ and f in ("glu", "qgelu"):                                # the gate / the activation's argument within |.| <= 16: one power of two on A and the bias
        pre = S + (bias if bias is not None else 0.0)
        p = float(2.0 ** np.floor(np.log2(16.0 / float(pre.abs().max()))))
        a *= p
        S *= p
        if bias is not None:
            bias *= p
    if f in ("rope", "vit"):
        w = 64 if f == "rope" else case["half"]
        if A_:
            tab = torch.tensor(ROT_SET, dtype=F64)
            cs, sn = tab[torch.randint(0, 9, (M, w), generator=gen)], tab[torch.randint(0, 9, (M, w), generator=gen)]
            for r, (cc, ss) in enumerate(((1.0, 0.0), (0.0, 1.0), (0.0, -1.0))):
                for row in (r, M - 1 - r, 230 + r):                 # whole rows, in the first tile, the last one and across the 224-row edge
                    cs[row], sn[row] = cc, ss
        else:
            ang = torch.rand(M, w, generator=gen, dtype=F64) * 6.283185307179586
            cs, sn = torch.cos(ang).to(F32).double(), torch.sin(ang).to(F32).double()
        inp.update(cos=cs, sin=sn)
    if f == "glubwd":
        I = case["I"]
        g = (torch.randn(M, I, generator=gen) * 2.5).clamp(-16, 16)
        inp["gu"] = torch.cat([g, torch.randn(M, I, generator=gen)], 1).to(BF16).double()
    for k_ in ("a", "b", "bias", "res"):
        if inp[k_] is not None:
            assert torch.equal(inp[k_].to(BF16).double(), inp[k_]), "%s: operand %s is not bf16" % (name, k_)
    inp["S"], inp["M_full"] = S, M
    inp["sumabs"] = None if A_ else a[:, :kv].abs() @ b[:, :kv].abs().t()
    return inp


def build(case):
    return _build(case["name"])


# ---------------------------------------------------------------------------------------------------------------- reference (and its mutants)
MUTANTS = ("ktile_dropped", "ktile_twice", "trunc", "half_away", "bias_after_rounding", "residual_dropped", "acc_ignores_c0", "chunks_exchanged",
           "row_from_m16", "gate_up_exchanged", "silu_not_rounded", "partner_sign_flipped", "v_rotated", "one_tile_share_lost", "dgut_pad_unwritten")


def applies(mut, case):
    f, M, N = case["form"], dims(case)[0], dims(case)[1]
    bf = case["out"] == "bf16"
    if mut == "half_away" and case["regime"] == "B":      # differs from RNE at exact ties only: gaussian sums have none
        return False
    return {"ktile_dropped": True, "ktile_twice": True, "trunc": bf, "half_away": bf,
            "bias_after_rounding": bf and case["bias"], "residual_dropped": case["res"], "acc_ignores_c0": case["out"] == "acc",
            "chunks_exchanged": N >= 16, "row_from_m16": M > 16, "gate_up_exchanged": f in ("glu", "glubwd"), "silu_not_rounded": f == "glu",
            "partner_sign_flipped": f in ("rope", "vit"), "v_rotated": f in ("rope", "vit"), "one_tile_share_lost": f == "splitk" and 1 in case["shares"],
            "dgut_pad_unwritten": f == "glubwd" and M % 64 != 0}[mut]


def _init_rows(inp, cols, poison):
    """The initial content of a bf16 output view, for the rows the inputs were restricted to."""
    full = init_of((inp["M_full"], cols), BF16, poison)
    return full if inp.get("rows") is None else full[inp["rows"]]


def _rows(case, inp, rows):
    """The inputs restricted to a subset of the rows of A (everything else of a row goes with it)."""
    if rows is None:
        return inp
    out = dict(inp, rows=rows)
    for k_ in ("a", "res", "c0", "S", "sumabs", "cos", "sin", "gu"):
        if inp.get(k_) is not None:
            out[k_] = inp[k_][rows]
    return out


def vit_cols(case):
    """Columns of a padded 128-wide head row that hold the a half and the b half."""
    half, nh = case["half"], case["nh"]
    off = 48 if half <= 48 else 64
    h = torch.arange(nh)[:, None] * 128
    d = torch.arange(half)[None, :]
    return (h + d).reshape(-1), (h + off + d).reshape(-1)


def init_of(shape, dtype, poison=0):
    """What an output view holds before the launch (and must still hold wherever the kernel has nothing to store)."""
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=F64) * (3 + 2 * poison)) % 89 + 500.0 + 64.0 * poison).to(dtype).view(*shape)


def reference(case, inp, mut=None, poison=0):
    """-> dict(out = {name: the expected content of every output view}, aux = what the window checks need).  With `mut` the same computation with one fault
    planted: what a kernel with that fault would leave."""
    f, A_ = case["form"], case["regime"] == "A"
    a, b, bias, res, c0, kv = inp["a"], inp["b"], inp["bias"], inp["res"], inp["c0"], inp["kv"]
    M, N = a.shape[0], b.shape[0]
    S = inp["S"]
    if mut in ("ktile_dropped", "ktile_twice", "one_tile_share_lost"):
        nk = (kv + 63) // 64
        t = nk // 2
        if mut == "one_tile_share_lost":
            t = sum(case["shares"][: case["shares"].index(1)])
        part = a[:, t * 64: min(t * 64 + 64, kv)] @ b[:, t * 64: min(t * 64 + 64, kv)].t()
        S = S + part if mut == "ktile_twice" else S - part
    rnd0 = {"trunc": trunc_bf16, "half_away": away_bf16}.get(mut, rne_exact if A_ else rne)
    rnd = (lambda x: rne(rnd0(x).double() + bias)) if mut == "bias_after_rounding" else rnd0       # the projection as a bf16-output epilogue stores it
    pre = S
    if bias is not None and mut != "bias_after_rounding":
        pre = pre + bias
    if res is not None and mut != "residual_dropped":
        pre = pre + res
    out, aux = {}, dict(pre=pre)
    if A_ and mut is None:
        assert exact32(pre), "%s: the value before rounding is not an fp32" % case["name"]
    if f in ("nt", "nn", "nnacc", "splitk"):
        if case["out"] == "bf16":
            y = rnd(pre)
        else:
            y = (pre + (c0 if (c0 is not None and mut != "acc_ignores_c0") else 0.0)).to(F32)
        out["c"] = y
    elif f == "qgelu":
        x = rnd(pre).double()
        v, E = quickgelu64(x)
        out["c"] = rne(v)
        aux.update(x=x)
    elif f == "glu":
        I = case["I"]
        gu = rnd(pre)
        g, u = gu[:, :I].double(), gu[:, I:].double()
        if mut == "gate_up_exchanged":
            g, u = u, g
        s = silu64(g)[0]
        out["a"] = rne((s if mut == "silu_not_rounded" else rne(s).double()) * u)
        if case["save_gu"]:
            out["gu"] = gu
        aux.update(gu=gu)
    elif f in ("rope", "vit"):
        p = rnd(pre).double()
        cs, sn = inp["cos"], inp["sin"]
        if f == "rope":
            nh, nkv = case["nh"], case["nkv"]
            secs = (("q", 0, nh), ("k", nh * 128, nkv), ("v", (nh + nkv) * 128, nkv))
            for nm, c_0, n_h in secs:
                blk = p[:, c_0: c_0 + n_h * 128].reshape(M, n_h, 2, 64)
                out[nm] = _rotate(blk[:, :, 0], blk[:, :, 1], cs[:, None], sn[:, None], nm == "v" and mut != "v_rotated", mut, A_ and mut is None).reshape(M, n_h * 128)
        else:
            nh, half = case["nh"], case["half"]
            ca, cb = vit_cols(case)
            blk = p.reshape(M, 3, nh, 2, half)
            for si, nm in enumerate("qkv"):
                o = _rotate(blk[:, si, :, 0], blk[:, si, :, 1], cs[:, None], sn[:, None], nm == "v" and mut != "v_rotated", mut, A_ and mut is None)  # [M, nh, 2, half]
                full = _init_rows(inp, nh * 128, poison)
                full[:, ca] = o[:, :, 0].reshape(M, -1)
                full[:, cb] = o[:, :, 1].reshape(M, -1)
                out[nm] = full
        aux.update(p=p)
    elif f == "glubwd":
        I = case["I"]
        d = rnd(pre).double()
        g, u = inp["gu"][:, :I], inp["gu"][:, I:]
        vg, Eg, vu, Eu = glubwd64(d, g, u)
        halves = [rne(vg), rne(vu)]
        if mut == "gate_up_exchanged":
            halves.reverse()
        out["dgu"] = torch.cat(halves, 1)
        aux.update(d=d)
    for k_ in list(out):                                              # faults of the store: applied to every output
        if mut == "chunks_exchanged" and out[k_].shape[1] >= 16:
            y = out[k_].clone()
            y[:, 0:8], y[:, 8:16] = out[k_][:, 8:16], out[k_][:, 0:8]
            out[k_] = y
        if mut == "row_from_m16":
            y = out[k_].clone()
            y[:-16] = out[k_][16:]
            out[k_] = y
    return dict(out=out, aux=aux)


def _rotate(xa, xb, c, s, plain, mut, exact):
    """[M, heads, w] halves -> [M, heads, 2, w] bf16: (xa c - xb s | xb c + xa s), or the halves themselves."""
    if plain:
        return torch.stack([xa, xb], 2).to(BF16)
    oa = xa * c - xb * s
    ob = (xb * c - xa * s) if mut == "partner_sign_flipped" else (xb * c + xa * s)
    if exact:
        assert exact32(oa) and exact32(ob) and exact32(xa * c) and exact32(xb * s), "the rotation is not exact in fp32"
    return torch.stack([rne(oa), rne(ob)], 2)


def dgu_t_of(case, dgu, ld_t, mut=None, poison=0):
    """dgu^T [2I, ld_t]: the transpose, exact zeros in columns [M, ld_t)."""
    M = dgu.shape[0]
    t = init_of((dgu.shape[1], ld_t), BF16, poison) if mut == "dgut_pad_unwritten" else torch.zeros(dgu.shape[1], ld_t, dtype=BF16)
    t[:, :M] = dgu.t()
    return t


# ---------------------------------------------------------------------------------------------------------------- checker
def _bits(t):
    return bits32(t) if t.dtype == F32 else bits16(t)


def gemm_E(case, inp):
    """Regime B: the fp32 accumulation bound (K + 2) 2^-24 (sum |a b| + |bias| + |residual|)."""
    s = inp["sumabs"].clone()
    if inp["bias"] is not None:
        s += inp["bias"].abs()
    if inp["res"] is not None:
        s += inp["res"].abs()
    return (inp["kv"] + 2) * U * s


def _cands(c64, E):
    """The admissible bf16 roundings of an fp32 value within E of c64: RNE(c64), and its other neighbour where c64 is within E of the boundary."""
    r = rne(c64)
    alt, mid = other_neighbour(c64, r)
    return r, alt, (c64 - mid).abs() <= E


def _wide(c64, E):
    """Regime B: E is at least half a bf16 step at c64 (a sum that cancels: |c| far below sum |a b|), so more than two roundings of the projection are
    admissible.  Such elements are held to the plain error bound of their output instead (`_loose`)."""
    r = rne(c64)
    k = _key(r)
    step = torch.minimum((_from_key(k + 1).double() - r.double()).abs(), (r.double() - _from_key(k - 1).double()).abs())
    return E >= 0.5 * step


def _dev(c64, E):
    """How far the bf16 projection can lie from c64: the fp32 value within E, its rounding within U (|c| + E)."""
    return E + U_BF16 * (c64.abs() + E)


def _loose(got, v, D):
    """got = RNE of an fp32 value within D of v."""
    return (got.double() - v).abs() <= D + U_BF16 * (v.abs() + D)


def _any_window(got, cands, fn):
    """got (bf16) against fn(x) -> (v, E) over candidate inputs [(x, admissible)] -> (ok, excused); excused = not the first candidate's RNE."""
    ok = torch.zeros(got.shape, dtype=torch.bool)
    first = None
    for x, adm in cands:
        v, E = fn(x)
        o, _ = window_ok(got, v, E)
        ok |= o & adm
        if first is None:
            first = _key(got) == _key(rne(v))
    return ok, ok & ~first


def check(case, inp, outs, rows=None, poison=0):
    """outs: {name: tensor on the CPU, the whole output view after the launch} -> {name: excused count}.  Raises AssertionError on the first output that is
    wrong.  Regime A: bit patterns (window only for the transcendental outputs); regime B: the derived bounds."""
    f, A_, nm = case["form"], case["regime"] == "A", case["name"]
    sub = _rows(case, inp, rows)
    ref = reference(case, sub, poison=poison)
    exp, aux = ref["out"], ref["aux"]
    excused = {}

    def exact(k_, got=None, want=None):
        got, want = outs[k_] if got is None else got, exp[k_] if want is None else want
        assert got.shape == want.shape and got.dtype == want.dtype, (nm, k_, got.shape, want.shape)
        bad = _bits(got) != _bits(want)
        if got.dtype == BF16:
            bad &= ~((got == 0) & (want == 0))
        assert not bool(bad.any()), "%s: %s differs from the exact value in %d of %d places (first at %s)" % (
            nm, k_, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())

    def windowed(k_, ok, exc, n=None):
        assert bool(ok.all()), "%s: %s is neither the rounded fp64 value nor excused by the window in %d of %d places (first at %s)" % (
            nm, k_, int((~ok).sum()), ok.numel(), (~ok).nonzero()[0].tolist())
        excused[k_] = int(exc.sum())
        if A_:
            assert excused[k_] <= EXCUSE_CAP * ok.numel(), "%s: %s: %d of %d elements passed by the window (cap 0.5 %%)" % (nm, k_, excused[k_], ok.numel())

    E = None if A_ else gemm_E(case, sub)
    pre = aux["pre"]
    if f in ("nt", "nn", "nnacc", "splitk"):
        if A_:
            exact("c")
        else:
            got = outs["c"].double()
            assert torch.isfinite(got).all(), "%s: non-finite output" % nm
            if case["out"] == "bf16":
                err, bnd = (got - pre).abs(), U_BF16 * (pre.abs() + E) + E
            else:
                c64 = pre + (sub["c0"] if sub["c0"] is not None else 0.0)
                err, bnd = (got - c64).abs(), E + (U * c64.abs() if sub["c0"] is not None else 0.0)
            r = oc.worst(err, bnd)
            excused["c.share_of_bound"] = r
            assert r <= 1.0, "%s: error is %.3f of the bound" % (nm, r)
    elif f == "qgelu":
        if A_:
            ok, exc = _any_window(outs["c"], [(aux["x"], True)], quickgelu64)
        else:
            r, alt, adm = _cands(pre, E)
            ok, exc = _any_window(outs["c"], [(r.double(), True), (alt.double(), adm)], quickgelu64)
            v, Ef = quickgelu64(pre)                    # |d/dx x sigmoid(1.702 x)| <= 1.1
            wide = _wide(pre, E) & ~ok & _loose(outs["c"], v, 1.1 * _dev(pre, E) + Ef * (1 + 2 * U_BF16))
            ok, exc = ok | wide, exc | wide
        windowed("c", ok, exc)
    elif f == "glu":
        I = case["I"]
        if case["save_gu"]:
            if A_:
                exact("gu")
            else:
                ok, exc = window_ok(outs["gu"], pre, E)
                wide = _wide(pre, E) & ~ok & ((outs["gu"].double() - pre).abs() <= _dev(pre, E))
                windowed("gu", ok | wide, exc | wide)
            gu = outs["gu"].double()
            ok, exc = swiglu_check(outs["a"], gu[:, :I], gu[:, I:])         # on the projection the kernel stored (checked above)
        elif A_:
            gu = aux["gu"].double()
            ok, exc = swiglu_check(outs["a"], gu[:, :I], gu[:, I:])
        else:
            raise AssertionError("regime B needs the stored projection")
        windowed("a", ok, exc)
    elif f in ("rope", "vit"):
        if A_:
            for k_ in "qkv":
                exact(k_)
        else:
            _check_rotary_b(case, sub, outs, pre, E, windowed, exact, poison)
    elif f == "glubwd":
        I = case["I"]
        g, u = sub["gu"][:, :I], sub["gu"][:, I:]
        if A_:
            cands = [(aux["d"], True)]
        else:
            r, alt, adm = _cands(pre, E)
            cands = [(r.double(), True), (alt.double(), adm)]
        for k_, sl, pick in (("dgu.gate", slice(0, I), slice(0, 2)), ("dgu.up", slice(I, 2 * I), slice(2, 4))):
            ok, exc = _any_window(outs["dgu"][:, sl], cands, lambda d: glubwd64(d, g, u)[pick])
            if not A_:                                  # both outputs are linear in d: the slope from d = 1, the evaluation error at the largest |d|
                v = glubwd64(pre, g, u)[pick][0]
                slope, Ef = glubwd64(torch.ones_like(pre), g, u)[pick][0].abs(), glubwd64(pre.abs() + _dev(pre, E), g, u)[pick][1]
                wide = _wide(pre, E) & ~ok & _loose(outs["dgu"][:, sl], v, slope * _dev(pre, E) + Ef)
                ok, exc = ok | wide, exc | wide
            windowed(k_, ok, exc)
        if "dgu_t" in outs:
            want = dgu_t_of(case, outs["dgu"], outs["dgu_t"].shape[1])
            bad = bits16(outs["dgu_t"]) != bits16(want)
            assert not bool(bad.any()), "%s: dgu^T is not the transpose of dgu with zeros in columns [M, ld_t) in %d places (first at %s)" % (
                nm, int(bad.sum()), bad.nonzero()[0].tolist())
    return excused


def _check_rotary_b(case, sub, outs, pre, E, windowed, exact, poison):
    """Regime B of EPI 4 / 7: every pair (x, y) of admissible roundings of the two projections, x c - y s within 2u (|x c| + |y s|) of the fp32 result."""
    f, M = case["form"], pre.shape[0]
    r, alt, adm = _cands(pre, E)
    wide_all, dev_all = _wide(pre, E), _dev(pre, E)
    cs, sn = sub["cos"][:, None], sub["sin"][:, None]
    if f == "rope":
        nh, nkv = case["nh"], case["nkv"]
        secs = (("q", 0, nh), ("k", nh * 128, nkv), ("v", (nh + nkv) * 128, nkv))
        pick = lambda t, c_0, n_h: t[:, c_0: c_0 + n_h * 128].reshape(M, n_h, 2, 64)
        got_of = lambda nm_, n_h: outs[nm_].reshape(M, n_h, 2, 64)
    else:
        nh, half = case["nh"], case["half"]
        ca, cb = vit_cols(case)
        secs = tuple((nm_, si, nh) for si, nm_ in enumerate("qkv"))
        pick = lambda t, si, n_h: t.reshape(M, 3, nh, 2, half)[:, si]
        got_of = lambda nm_, n_h: torch.stack([outs[nm_][:, ca].reshape(M, nh, half), outs[nm_][:, cb].reshape(M, nh, half)], 2)
        live = torch.zeros(nh * 128, dtype=torch.bool)
        live[ca] = True
        live[cb] = True
        for nm_ in "qkv":
            init = _init_rows(sub, nh * 128, poison)
            assert torch.equal(bits16(outs[nm_][:, ~live]), bits16(init[:, ~live])), "%s: pad columns of %s changed" % (case["name"], nm_)
    for nm_, c_0, n_h in secs:
        R, AL, AD = pick(r, c_0, n_h).double(), pick(alt, c_0, n_h).double(), pick(adm, c_0, n_h)
        got = got_of(nm_, n_h)
        W, D, P = pick(wide_all, c_0, n_h), pick(dev_all, c_0, n_h), pick(pre, c_0, n_h)
        if nm_ == "v":
            ok, exc = window_ok(got, P, pick(E, c_0, n_h))
            wide = W & ~ok & ((got.double() - P).abs() <= D)
            windowed(nm_, ok | wide, exc | wide)
            continue
        for hi, sign, nm2 in ((0, -1.0, nm_ + ".a"), (1, 1.0, nm_ + ".b")):
            ok = torch.zeros(got[:, :, hi].shape, dtype=torch.bool)
            first = None
            for xa, aa in ((R[:, :, 0], True), (AL[:, :, 0], AD[:, :, 0])):
                for xb, ab in ((R[:, :, 1], True), (AL[:, :, 1], AD[:, :, 1])):
                    t1, t2 = (xa * cs, xb * sn) if hi == 0 else (xb * cs, xa * sn)
                    v = t1 + sign * t2
                    o, _ = window_ok(got[:, :, hi], v, 2 * U * (t1.abs() + t2.abs()))
                    ok |= o & aa & ab
                    if first is None:
                        first = _key(got[:, :, hi]) == _key(rne(v))
            t1, t2 = (P[:, :, 0] * cs, P[:, :, 1] * sn) if hi == 0 else (P[:, :, 1] * cs, P[:, :, 0] * sn)
            d1, d2 = (D[:, :, 0] * cs.abs(), D[:, :, 1] * sn.abs()) if hi == 0 else (D[:, :, 1] * cs.abs(), D[:, :, 0] * sn.abs())
            wide = (W[:, :, 0] | W[:, :, 1]) & ~ok & _loose(got[:, :, hi], t1 + sign * t2, (d1 + d2) * (1 + 2 * U) + 2 * U * (t1.abs() + t2.abs()))
            ok = ok | wide
            windowed(nm2, ok, ok & ~first)


def fake_outputs(case, inp, mut, rows=None, poison=0):
    """What a kernel with the fault `mut` would leave in the output views (the mutated reference)."""
    sub = _rows(case, inp, rows)
    out = reference(case, sub, mut, poison)["out"]
    if case["form"] == "glubwd":
        M = out["dgu"].shape[0]
        out["dgu_t"] = dgu_t_of(case, out["dgu"], (M + 63) // 64 * 64, mut, poison)
    return out


def window_shares(case, inp, rows=None):
    """Regime A, from the fp64 reference alone: {output: share of elements within E of a rounding boundary} (what the window could excuse at most)."""
    f = case["form"]
    sub = _rows(case, inp, rows)
    aux = reference(case, sub)["aux"]
    if f == "qgelu":
        return {"c": near_share(*quickgelu64(aux["x"]))}
    if f == "glu":
        I = case["I"]
        return {"a": near_share(*silu64(aux["gu"][:, :I].double()))}
    if f == "glubwd":
        I = case["I"]
        vg, Eg, vu, Eu = glubwd64(aux["d"], sub["gu"][:, :I], sub["gu"][:, I:])
        return {"dgu.gate": near_share(vg, Eg), "dgu.up": near_share(vu, Eu)}
    return {}


# ---------------------------------------------------------------------------------------------------------------- launch (GPU file)
def _opnd(t, dev, keep):
    buf, v = framed(t.to(BF16), fill=PLANT_BIG, dev=dev)
    keep.append(buf)
    return v


def _vec(t, dev, keep):
    """bias [N] between eight unreadable elements on each side."""
    if t is None:
        return None
    buf = torch.tensor(PLANT_BIG, dtype=F32).repeat(t.numel() // 4 + 8)[: t.numel() + 16].to(BF16)
    buf[8: 8 + t.numel()] = t.to(BF16)
    buf = buf.to(dev)
    keep.append(buf)
    return buf[8: 8 + t.numel()]


def _p(t):
    return 0 if t is None else t.data_ptr()


def launch(ops, case, inp, dev, poison=0, ws_extra=0):
    """One C-ABI call on strided operand views between unreadable values, into output views inside sentinel frames.
    -> {name: view on the CPU} after asserting that every frame kept its bits."""
    f = case["form"]
    M, N, K = dims(case)
    keep, frames = [], {}
    s = ops._s()

    def out(name, shape, dtype, init=None, cols=None, rows=1):
        init = init_of(shape, dtype, poison) if init is None else init.to(dtype)
        buf, v = framed(init, rows=rows, cols=(8 if dtype == BF16 else 4) if cols is None else cols, dev=dev)
        frames[name] = (buf, v, shape)
        return v

    a = _opnd(inp["a"], dev, keep)
    kmajor = f in ("nn", "nnacc", "glubwd") or case.get("kmajor", False)
    if kmajor:
        bt = inp["b"].t().contiguous()
        if f == "nnacc":
            for i in range(inp["kv"], K):
                bt[i] = PLANT_BIG[(i - inp["kv"]) % len(PLANT_BIG)]
        b = _opnd(bt, dev, keep)
    else:
        b = _opnd(inp["b"], dev, keep)
    bias = _vec(inp["bias"], dev, keep)
    res = _opnd(inp["res"], dev, keep) if inp["res"] is not None else None
    ldr = res.stride(0) if res is not None else 0
    call = ops.L.call
    if f == "nt":
        c = out("c", (M, N), BF16 if case["out"] == "bf16" else F32, init=inp["c0"] if case["out"] == "acc" else None)
        call("tr1_gemm_nt_bf16", _p(a), _p(b), _p(c), _p(bias), _p(res), M, N, K, a.stride(0), b.stride(0), c.stride(0), ldr, int(case["out"] != "bf16"),
             int(case["out"] == "acc"), s)
    elif f == "nn":
        c = out("c", (M, N), BF16)
        call("tr1_gemm_nn_bf16", _p(a), _p(b), _p(c), M, N, K, a.stride(0), b.stride(0), c.stride(0), s)
    elif f == "nnacc":
        c = out("c", (M, N), F32, init=inp["c0"] if case["out"] == "acc" else None)
        call("tr1_gemm_nn_acc_f32", _p(a), _p(b), _p(c), M, N, K, a.stride(0), b.stride(0), c.stride(0), int(case["out"] == "acc"), inp["kv"], s)
    elif f == "qgelu":
        c = out("c", (M, N), BF16)
        call("tr1_gemm_bias_quickgelu_bf16", _p(a), _p(b), _p(bias), _p(c), M, N, K, a.stride(0), b.stride(0), c.stride(0), s)
    elif f == "glu":
        I = case["I"]
        ao = out("a", (M, I), BF16)
        gu = out("gu", (M, 2 * I), BF16) if case["save_gu"] else None
        call("tr1_gemm_glu_bf16", _p(a), _p(b), _p(bias), _p(ao), _p(gu), M, I, K, a.stride(0), b.stride(0), ao.stride(0), gu.stride(0) if gu is not None else 0, s)
    elif f in ("rope", "vit"):
        cs, sn = inp["cos"].to(F32).contiguous().to(dev), inp["sin"].to(F32).contiguous().to(dev)
        keep += [cs, sn]
        if f == "rope":
            nh, nkv = case["nh"], case["nkv"]
            q, k, v = out("q", (M, nh * 128), BF16), out("k", (M, nkv * 128), BF16), out("v", (M, nkv * 128), BF16)
            call("tr1_gemm_qkv_rope_bf16", _p(a), _p(b), _p(bias), _p(cs), _p(sn), _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), M, nh, nkv, 128, K,
                 a.stride(0), b.stride(0), s)
        else:
            nh, half = case["nh"], case["half"]
            q, k, v = (out(n_, (M, nh * 128), BF16) for n_ in "qkv")
            call("tr1_gemm_qkv_rope_vit_bf16", _p(a), _p(b), _p(bias), _p(cs), _p(sn), _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), M, nh, half, K,
                 a.stride(0), b.stride(0), s)
    elif f == "glubwd":
        I = case["I"]
        gu = _opnd(inp["gu"], dev, keep)
        dgu = out("dgu", (M, 2 * I), BF16)
        ld_t = (M + 63) // 64 * 64
        dgt = out("dgu_t", (2 * I, ld_t), BF16, cols=0)
        call("tr1_gemm_nn_glubwd_bf16", _p(a), _p(b), _p(gu), _p(dgu), M, I, K, a.stride(0), b.stride(0), gu.stride(0), dgu.stride(0), _p(dgt), ld_t, s)
    elif f == "splitk":
        c = out("c", (M, N), BF16)
        n_ws = case["max_s"] * M * N + ws_extra
        ws = torch.full((n_ws + 64,), float("nan"), dtype=F32, device=dev)
        call("tr1_gemm_splitk_bf16", _p(a), _p(b), _p(c), _p(bias), _p(res), M, N, K, a.stride(0), b.stride(0), c.stride(0), ldr, int(kmajor), _p(ws), n_ws, s)
        keep.append(ws)
    torch.cuda.synchronize()
    if f == "splitk":
        assert bool(torch.isnan(ws[n_ws:]).all()), "%s: wrote past the workspace" % case["name"]
    got = {}
    for name, (buf, v, shape) in frames.items():
        assert frame_intact(buf, shape[0], shape[1]), "%s: the sentinel frame of %s changed" % (case["name"], name)
        got[name] = v.cpu().contiguous()
    return got
