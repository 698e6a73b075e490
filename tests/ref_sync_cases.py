"""Cases and references for the reference-policy sync (GRPOConfig.sync_ref_model; tr1_ref_mixup, csrc/optim.hip).  Shared by
tests/test_ref_sync_ref.py (CPU) and tests/test_ref_sync_gpu.py (the HIP kernel and the HIP trainer on the same cases).

The kernel, in place on ref, with a = fp32(alpha) and keep = fp32(1 - a) (exact for every alpha below: Sterbenz for 0.5 <= a <= 1, a power of two otherwise):

  ref[i] = bf16_rne(fadd(fmul(keep, ref[i]), fmul(a, policy[i])))        three separately rounded fp32 operations, one rounding to bf16
  sums   = [sum (policy - ref)^2, sum ref^2] of the values before the mix, fp32

`composite` (oracle.ref_ops.mixup_composite, which RefOps.ref_mixup applies to its arenas) is that text in torch, three separate fp32 ops: the kernel must match
it bit for bit (a NaN by position: its payload is not part of the contract).
`mix64` / `sums64` are the fp64 references.

What the composite may differ from RNE(fp64 mix) by: the three fp32 roundings move the sum by at most 2^-24 (|t1| + |t2| + |mix|) = 2^-24 (c + 1) |mix| with
t1 = keep ref, t2 = a policy and c = (|t1| + |t2|) / |mix| the cancellation of the pair.  The data keeps c <= 15 on every finite pair (data_cancellation, checked
in test_ref_sync_ref.py), so that distance stays under 2^-20 |mix| and only a value within 2^-20 relative of a bf16 tie may round the other way.  Results in the
bf16 subnormal range are built to be exact or far from a tie (see _TAME), because there fp32's own spacing (2^-149) is no longer 2^-24 relative.

Signed zeros: x + (+0) is +0 for x = -0, so alpha = 0 (alpha = 1) returns ref (policy) bit for bit except that a zero comes out as +0 where the other term
is a zero of the opposite sign.  identity_ok states exactly that.
"""
import numpy as np
import torch

import optim_cases as oc
from oracle.ref_ops import mixup_composite as composite  # noqa: F401  (the kernel's contract; RefOps.ref_mixup is built from it)

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
PAD, TOL_SUMSQ_RTOL = oc.PAD, oc.TOL_SUMSQ_RTOL
GRID_PASS = 2048 * 256 * 8          # elements one pass of ref_mixup_kernel's capped grid covers (csrc/optim.hip)
NS = (0, 1, 7, 8, 9, 1023, 65537, GRID_PASS + 3)
OFFS = (0, 64)                      # view offsets in elements (the kernel wants 16-byte alignment: the arena and its segments are aligned far beyond that)
ALPHAS = (0.0, 2.0 ** -9, 0.6, 1.0)
TIE_MARGIN = 2.0 ** -20
MAX_CANCELLATION = 15.0

_SUB = 2.0 ** -133                  # the smallest bf16 subnormal; bf16 subnormals are k * 2^-133, k = 1 .. 127
_BIG = 3e38
_NAN = float("nan")
# (ref, policy) pairs planted into the random data.  tame: finite and square-summable in fp32.  wild: the +-3e38 pairs (each product is finite and the true mix
# is finite: a formula that adds before it scales would overflow) and the NaNs (each must reach its own element only; the sums become inf / NaN).
# Subnormal pairs: equal values (the mix is the value itself, on the bf16 grid) or a zero partner (0.4 k, 0.6 k, k (1 - 2^-9), k 2^-9 with k <= 127 are all
# at least 0.1 of a bf16 subnormal step away from a tie).
_TAME = [(0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, 1.5), (-0.0, -2.5), (3.0, -0.0),
         (_SUB, _SUB), (-77 * _SUB, -77 * _SUB), (127 * _SUB, 0.0), (0.0, -93 * _SUB), (-5 * _SUB, -0.0), (2.0 ** -126, 2.0 ** -126),
         (1.0, -16.0), (-0.375, 12.0), (24.0, -0.5), (-2.0 ** -12, 2.0 ** -17)]
_WILD = [(_BIG, -_BIG), (-_BIG, _BIG), (_BIG, _BIG), (_NAN, 1.0), (-_BIG, 0.25), (1.0, _NAN)]


def f32(x):
    return float(np.float32(x))


def make_data(n, wild, seed=0):
    """-> (ref, policy) bf16 [n]: random values of mixed magnitude (2^-20 .. 2^5, either sign), half of the policy values within a few percent of the reference
    (same sign: c = 1), half independent of it, and the special pairs planted at random positions and in the last 7 elements (the scalar tail).  Small n rotate through the specials."""
    g = torch.Generator().manual_seed(1000 * seed + n + (7 if wild else 0))
    mag = torch.pow(2.0, torch.randint(-20, 6, (n,), generator=g).to(F32)) * (1.0 + torch.rand(n, generator=g))
    r = (mag * (torch.randint(0, 2, (n,), generator=g).to(F32) * 2 - 1)).to(BF16)
    p = (r.float() * (1.0 + 0.05 * torch.randn(n, generator=g))).to(BF16)
    # every other pair: a policy value drawn on its own (any magnitude, either sign).  A policy a few bf16 steps from its reference keeps the mix a small
    # multiple of alpha away from the bf16 grid - never near a tie, so a fused multiply-add in place of the separate roundings would go unseen
    # (fused_variant, test_ref_sync_ref.py); independent pairs do not have that structure.  Pairs of opposite sign that would cancel beyond
    # MAX_CANCELLATION at one of the alphas get the reference's sign instead (c = 1).
    free = torch.rand(n, generator=g) < 0.5
    q = (torch.pow(2.0, torch.randint(-20, 6, (n,), generator=g).to(F32)) * (1.0 + torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g).to(F32) * 2 - 1)).to(BF16)
    for alpha in ALPHAS:
        a = f32(alpha)
        t1, t2 = (1.0 - a) * r.double(), a * q.double()
        bad = (t1.abs() + t2.abs()) > 0.5 * MAX_CANCELLATION * (t1 + t2).abs()
        q = torch.where(bad, torch.copysign(q.float(), r.float()).to(BF16), q)
    p = torch.where(free, q, p)
    sp = _TAME + (_WILD if wild else [])
    if n == 0:
        return r, p
    copies = 1 if n < 64 else 8
    pos = torch.randperm(n, generator=g)[: min(n, copies * len(sp))].tolist()
    pos += [i for i in range(max(0, n - 7), n) if i not in pos] if n >= 64 else []
    start = (n * 5 + (3 if wild else 0)) % len(sp)
    if wild and n < len(sp):
        start = len(_TAME) + n % len(_WILD)          # the few elements of a small wild case are wild pairs
    for j, i in enumerate(pos):
        a, b = sp[(start + j) % len(sp)]
        r[i], p[i] = a, b
    return r, p


def fused_variant(r, p, alpha):
    """What a kernel computes whose compiler contracted the sum into a fused multiply-add, fma(keep, r, fmul(a, p)): one rounding fewer.  keep r (at most 32
    significant bits) is exact in fp64 and so, to far below an fp32 rounding, is its sum with the rounded product.  The cases must tell this from the composite."""
    a = torch.tensor(alpha, dtype=F32)
    keep = torch.tensor(1.0, dtype=F32) - a
    return (keep.double() * r.double() + (a * p.float()).double()).to(F32).to(r.dtype)


def mix64(r, p, alpha):
    a = f32(alpha)
    return (1.0 - a) * r.double() + a * p.double()


def sums64(r, p):
    r, p = r.double(), p.double()
    return torch.stack([((p - r) ** 2).sum(), (r ** 2).sum()])


def data_cancellation(r, p, alpha):
    """c = (|t1| + |t2|) / |mix| over the finite pairs with a non-zero mix (fp64) -> its maximum (0 for no such pair)."""
    a = f32(alpha)
    t1, t2 = (1.0 - a) * r.double(), a * p.double()
    m = t1 + t2
    ok = torch.isfinite(m) & (m != 0)
    return float(((t1.abs() + t2.abs())[ok] / m[ok].abs()).max()) if bool(ok.any()) else 0.0


def bf16_rne64(x):
    """RNE of fp64 values to bf16 without passing through fp32 (no double rounding), and the relative distance of each value to the nearest bf16 tie.
    -> (bf16 tensor, distance / |x|: inf where x is 0 or not finite, the bf16 spacing at |x| in fp64)."""
    x = x.double()
    fin = torch.isfinite(x) & (x != 0)
    ax = torch.where(fin, x.abs(), torch.ones_like(x))
    e = torch.floor(torch.log2(ax)).clamp(min=-126.0)                  # binade (the subnormal range shares the exponent -126)
    e = torch.where(ax < torch.pow(2.0, e), e - 1, e)                  # log2 rounding at a power of two
    e = torch.where(ax >= torch.pow(2.0, e + 1), e + 1, e).clamp(min=-126.0)
    ulp = torch.pow(2.0, e - 7)                                        # bf16: 8 significant bits
    q = ax / ulp                                                       # exact: a power-of-two scale
    lo = torch.floor(q)
    frac = q - lo
    up = (frac > 0.5) | ((frac == 0.5) & (lo % 2 == 1))
    mag = (lo + up.double()) * ulp
    out = torch.where(fin, torch.copysign(mag, x), x).to(F32).to(BF16)      # mag is on the bf16 grid: both casts are exact (overflow to inf as RNE does)
    dist = torch.where(fin, (frac - 0.5).abs() * ulp / ax, torch.full_like(x, float("inf")))
    return out, dist, ulp


def bits(t):
    return oc.bits16(t) if t.dtype == BF16 else oc.bits32(t)


def same_bits(got, want):
    """Bit equality, NaNs by position (any NaN encoding)."""
    got, want = got.cpu(), want.cpu()
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    return bool(torch.equal(gn, wn)) and bool(torch.equal(bits(got)[~gn], bits(want)[~wn]))


def identity_ok(out, src, other):
    """alpha = 0 (src = ref, other = policy) or alpha = 1 (src = policy, other = ref) on finite pairs: out is src bit for bit, except +0 where src is -0 and the
    other term's product is +0 (0 * other has other's sign); a pair that holds a NaN gives NaN."""
    out, src, other = out.cpu(), src.cpu(), other.cpu()
    fin = torch.isfinite(src.float()) & torch.isfinite(other.float())
    zero = fin & (src.float() == 0)
    plain = fin & ~zero
    ok = torch.equal(bits(out)[plain], bits(src)[plain]) and bool((out.float()[zero] == 0).all())
    neg_both = zero & torch.signbit(src.float()) & torch.signbit(other.float())
    return ok and bool(torch.signbit(out.float()[neg_both]).all()) and bool(torch.isnan(out.float()[~fin]).all())      # 0 * NaN is NaN: a NaN pair gives NaN


def framed(r, p, off, dev="cpu"):
    """-> (ref buffer, policy buffer, ref view, policy view): both arrays at element offset `off` inside sentinel frames (optim_cases.views)."""
    (rb, pb), (rv, pv) = oc.views([r, p], [off, off], dev)
    return rb, pb, rv, pv


def frames_intact(rb, pb, p, off):
    n = p.numel()
    return oc.sentinels_intact(rb, off, n) and oc.sentinels_intact(pb, off, n) and same_bits(pb[PAD + off: PAD + off + n], p)


def metric_keys(log):
    return {k for k in log if not k.startswith("perf/") and k not in ("samples_per_sec", "rollout_tokens_per_sec")}


def run_with_snapshots(tr, ckpt=None):
    """train() -> per optimizer step (at on_step_end, i.e. after a sync of that step): the reference and the policy weights, as CPU clones."""
    snaps = []

    class CB:
        def on_step_end(self, args, state, control, **kw):
            snaps.append(dict(step=state.global_step, ref=tr.ref_model.w16.detach().clone().cpu(), pol=tr.params.train.w16.detach().clone().cpu()))
    tr.callbacks = [CB()]
    tr.train(resume_from_checkpoint=ckpt)
    return snaps


def distance64(ref, pol):
    s = sums64(ref, pol)
    return float(s[0].sqrt() / s[1].clamp(min=float(torch.finfo(F32).tiny)).sqrt())
