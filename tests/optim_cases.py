"""Seeded cases, fp64 references and derived bounds for the optimizer side: csrc/optim.hip (fused AdamW, the grad-norm sums, the periodic
zero / sum over the small per-layer tensors) and the weight-gradient epilogue of csrc/gemm.hip that leaves sums of squares (tr1_wgrad_f32_sumsq).

Shared by tests/test_optim_side_ref.py (CPU: the fp32 oracle against these references, the host-side partition logic) and
tests/test_optim_side_gpu.py (the HIP kernels against the same references on the same cases).  Plain torch, written from the formulas:

  coef  = grad_mult * min(1, max_norm / (grad_mult * sqrt(sumsq) + 1e-6))   when sumsq is given and max_norm > 0, else grad_mult
  gg    = g * coef
  m'    = b1 m + (1 - b1) gg
  v'    = b2 v + (1 - b2) gg^2
  delta = lr / (1 - b1^step) * m' / (sqrt(v') / sqrt(1 - b2^step) + eps)
  p'    = p (1 - lr wd) - delta

A. ONE step from a given fp32 state (p, m, v, g, step, sumsq are inputs; the norm kernel's own error does not enter), recomputed in fp64.

The hyper-parameters cross the C ABI as fp32, so a case states them as fp32 values (f32(1e-6), f32(0.999), ...): kernel, oracle and reference
then work from the same numbers, and 1 - b1, 1 - b2 are exact in fp32 (Sterbenz, 0.5 <= b <= 1).  The distance between f32(0.999) and the
decimal 0.999 is a perturbation of the hyper-parameter (1.3e-8), not arithmetic, and is not measured here.

Bounds: u = 2^-24 is the largest relative error of one fp32 rounding (sqrtf and the division are correctly rounded in the default build);
contraction into fma only removes roundings.  First order in u; the second-order terms are below 1e-5 of each bound and covered by rounding
the counts up.

  coef (clipping):  sqrtf, * grad_mult, + 1e-6f (the constant itself is 1e-6 to within u), max_norm / (.), * grad_mult        5 roundings + 1 = 6u
  gg = g * coef:    1 more                                                                                                     E_GG = 7u
  m':  t1 = b1 m (1), t2 = (1 - b1) gg (1 + E_GG = 8), the sum (1, of |m'| <= |t1| + |t2|)
       |m' - ref| <= 9u (|t1| + |t2|)                                                                                          R_M = 9u
       (relative to the two terms, not to m': they can cancel)
  v':  b2 v (1); (1 - b2) gg gg = 2 roundings + 2 E_GG = 16; the sum (1); every term is >= 0, so relative to v'
       |v' - ref| <= 17u ref                                                                                                   R_V = 17u
  denom = sqrtf(v') / bc2_sqrt + eps:  sqrt halves R_V (8.5) + its own rounding (1), bc2_sqrt is an fp32 (1), the division (1), + eps (1; all
       terms >= 0)                                                                                                             12.5u
  delta = (lr / bc1) * (m' / denom):  bc1 is an fp32 (1), lr / bc1 (1), m' / denom (1), the product (1), the error of denom (12.5) - these 16.5
       scale with |m'| <= |t1| + |t2| - and the error of m' itself, 9u (|t1| + |t2|): 25.5, rounded up                          R_D = 26u
  p' = p * (1 - lr wd) - delta:  dec = fl(1 - fl(lr wd)) is off by at most 2^-24 absolute (this includes the case lr wd < 2^-25, where dec is
       exactly 1 as in torch's own fp32 AdamW: lr 1e-6 with wd 0.01), which moves p * dec by less than one ulp32(p); the product rounds
       (1/2 ulp), the subtraction rounds (1/2 ulp of the result)                                                               C_P = 2 ulp
       |p' - ref| <= C_P ulp32(max(|p|, |ref|)) + R_D (lr / bc1) (|t1| + |t2|) / denom_ref
       (max: the update can cancel p, and the intermediate p * dec has the magnitude of p)

A result below the smallest normal fp32 (2^-126) may be rounded to the denormal grid or flushed: up to three such operations feed m' and v',
so both bounds carry an absolute floor of 3 * 2^-126.  No case relies on it.

The oracle must sit at or below ORACLE_SHARE = 0.75 of every bound on every case (tests/test_optim_side_ref.py), so a GPU miss cannot be the
reference's rounding.

Out of scope: non-finite gradients (they give NaN, as clip_grad_norm_ does).  `1.f - lr * wd` equals 1 in fp32 when lr * wd < 2^-25 (lr 1e-6,
wd 0.01): torch's own fp32 behaviour, inside the ulp term above, left as it is.

B. The grad-norm pieces on data that makes fp32 summation exact in ANY order: small integers whose squares sum to less than 2^24, so every
partial sum of every reduction tree is an integer below 2^24.  The checks are bit equalities: one element missed or counted twice fails.
"""
import math
import re

import numpy as np
import torch

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

U = 2.0 ** -24
E_GG = 7 * U
R_M = 9 * U
R_V = 17 * U
R_D = 26 * U
C_P = 2.0
FLOOR = 3 * 2.0 ** -126
ORACLE_SHARE = 0.75
EXACT_LIMIT = 1 << 24
TOL_SUMSQ_RTOL = 1e-4           # the project's own tolerance for a sum of squares (tests/test_ops_gpu.py)

GRID_PASS = 4096 * 256 * 4      # elements one pass of adamw_kernel's capped grid covers (csrc/optim.hip)
SUMSQ_PASS_F32 = 2048 * 256 * 4
SUMSQ_PASS_BF16 = 2048 * 256 * 8
PAD = 8                         # sentinel elements on both sides of every view (8 fp32 = 32 B, 8 bf16 = 16 B: the view offsets below are the misalignment)


def f32(x):
    """The fp32 value of a hyper-parameter, as a Python float: what the C ABI hands the kernel."""
    return float(np.float32(x))


B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)


def worst(err, bound):
    """Largest err / bound in fp64 (0 / 0 counts as 0); a ratio <= 1 means the bound holds everywhere."""
    err, bound = err.double(), bound.double()
    assert err.shape == bound.shape, (err.shape, bound.shape)
    if err.numel() == 0:
        return 0.0
    assert torch.isfinite(err).all(), "non-finite values"
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


def ulp32(x):
    """Spacing of fp32 at |x| (fp64 tensor)."""
    a = x.abs().to(F32)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def bits32(t):
    return t.contiguous().view(torch.int32)


def bits16(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------- A. adamw_step
def ref_coef(sumsq, max_norm, grad_mult):
    if sumsq is not None and max_norm > 0:
        return grad_mult * min(1.0, max_norm / (grad_mult * math.sqrt(float(sumsq)) + 1e-6))
    return grad_mult


def ref_adamw(p, m, v, g, lr, wd, step, sumsq=None, max_norm=0.0, grad_mult=1.0, b1=B1, b2=B2, eps=EPS):
    """fp64 step from fp32 inputs (on the inputs' device) -> dict(p, m, v) and the scales the bounds need."""
    p, m, v, g = p.double(), m.double(), v.double(), g.double()
    gg = g * ref_coef(sumsq, max_norm, grad_mult)
    t1, t2 = b1 * m, (1.0 - b1) * gg
    mn = t1 + t2
    vn = b2 * v + (1.0 - b2) * gg * gg
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    den = vn.sqrt() / math.sqrt(bc2) + eps
    pn = p * (1.0 - lr * wd) - (lr / bc1) * mn / den
    terms = t1.abs() + t2.abs()
    return dict(p=pn, m=mn, v=vn, terms=terms, dscale=(lr / bc1) * terms / den, p_in=p)


def adamw_bounds(ref):
    return dict(p=C_P * ulp32(torch.maximum(ref["p_in"].abs(), ref["p"].abs())) + R_D * ref["dscale"],
                m=R_M * ref["terms"] + FLOOR,
                v=R_V * ref["v"] + FLOOR)


def adamw_ratios(got_p, got_m, got_v, ref):
    """Worst error / bound of the three fp32 outputs."""
    b = adamw_bounds(ref)
    return {k: worst((x.double() - ref[k]).abs(), b[k]) for k, x in (("p", got_p), ("m", got_m), ("v", got_v))}


def adamw_state(n, seed, state):
    """-> p, m, v, g fp32 [n].  p ~ 0.05 N(0, 1) (a weight matrix); one element in 16 of p is tiny, so the update dominates it (and can cancel it)."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * 0.05
    p[torch.arange(n) % 16 == 5] *= 1e-4
    r1, r2, r3 = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    if state == "first":            # first step: no history
        m, v, g = torch.zeros(n), torch.zeros(n), r3 * 1e-2
    elif state == "trained":        # history of the gradient's own scale; m and g of both signs, so t1 and t2 cancel in places
        m, v, g = r1 * 3e-3, (r2 * 1e-2) ** 2, r3 * 1e-2
    elif state == "tiny":           # |g| about 1e-6: v' about 1e-12, sqrt(v') about 100 eps
        m, v, g = r1 * 3e-7, (r2 * 1e-6) ** 2, r3 * 1e-6
    else:
        raise ValueError(state)
    return p, m, v, g


def _case(name, n, state="trained", lr=1e-6, wd=0.0, step=7, clip="given", max_norm=1.0, gm=0.5, offs=(0, 0, 0, 0, 0, 0), seed=None):
    """clip: None (no sumsq) | "given" (sumsq = the gradient's own, so the norm is what it is) | a float (sumsq set to it).
    offs: element offsets of the p, m, v, g, p16, g16 views into their 16-byte-aligned buffers."""
    return dict(name=name, n=n, state=state, lr=f32(lr), wd=f32(wd), step=step, clip=clip, max_norm=f32(max_norm), gm=f32(gm), offs=offs,
                seed=seed if seed is not None else (n * 31 + step) % 100003)


def adamw_cases():
    c = []
    # settings: lr x wd x step x state scale (n with a 3-element tail)
    c.append(_case("lr1e-6-wd0-step1-first", 100003, "first", 1e-6, 0.0, 1))
    c.append(_case("lr1e-6-wd0.01-step2-trained", 100003, "trained", 1e-6, 0.01, 2))
    c.append(_case("lr1e-6-wd0-step2-tiny", 100003, "tiny", 1e-6, 0.0, 2, clip=None, gm=1.0))
    c.append(_case("lr1e-6-wd0.01-step100000-trained", 100003, "trained", 1e-6, 0.01, 100000))
    c.append(_case("lr2e-5-wd0-step1000-trained", 100003, "trained", 2e-5, 0.0, 1000))
    c.append(_case("lr2e-5-wd0.01-step100000-tiny", 100003, "tiny", 2e-5, 0.01, 100000, clip=None, gm=1.0))
    c.append(_case("lr2e-5-wd0.01-step1-first", 100003, "first", 2e-5, 0.01, 1))
    c.append(_case("lr1e-3-wd0.01-step1000-trained", 100003, "trained", 1e-3, 0.01, 1000))
    c.append(_case("lr1e-3-wd0.01-step1-first", 100003, "first", 1e-3, 0.01, 1))
    # clip (grad_mult 0.5: the norm meets max_norm 1 at sumsq = 4)
    below, above = float(np.nextafter(np.float32(4.0), np.float32(0.0))), float(np.nextafter(np.float32(4.0), np.float32(8.0)))
    for nm, kw in (("none", dict(clip=None)), ("maxnorm0", dict(clip="given", max_norm=0.0)), ("sumsq0", dict(clip=0.0)),
                   ("below", dict(clip=f32(4.0 * (1 - 1e-5)))), ("just-below", dict(clip=below)), ("just-above", dict(clip=above)),
                   ("above", dict(clip=f32(4.0 * (1 + 1e-5)))), ("sumsq1e30", dict(clip=f32(1e30))),
                   ("gm0.125", dict(clip="given", gm=0.125)), ("gm0.125-none", dict(clip=None, gm=0.125))):
        c.append(_case("clip-" + nm, 10007, "trained", 1e-6, 0.01, 7, **kw))
    # length and grid
    for n in (1, 3, 4, 5, 1023, GRID_PASS + 3, 3 * GRID_PASS + 1):
        c.append(_case("n%d" % n, n, "trained", 2e-5, 0.01, 3))
    # alignment: the slices a.master[x:y], a.grad[x:y], a.w16[x:y], g16[x:y] start at any element
    for o in ((1, 1, 1, 1, 1, 1), (2, 2, 2, 2, 2, 2), (3, 3, 3, 3, 3, 3), (1, 2, 3, 0, 5, 7), (3, 0, 1, 2, 7, 3), (0, 0, 0, 0, 1, 1)):
        c.append(_case("offs" + "".join(map(str, o)), 4103, "trained", 2e-5, 0.01, 3, offs=o))
    c.append(_case("offs333333-n%d" % (GRID_PASS + 3), GRID_PASS + 3, "trained", 1e-6, 0.0, 2, offs=(3, 3, 3, 3, 3, 3)))
    return c


BIG_N = 1 << 20          # cases above this size run their reference where the data is (the GPU file: on the device)


def adamw_inputs(case):
    p, m, v, g = adamw_state(case["n"], case["seed"], case["state"])
    clip = case["clip"]
    if clip is None:
        ss = None
    elif clip == "given":
        ss = (g.double() ** 2).sum().to(F32).reshape(1)
    else:
        ss = torch.tensor([clip], dtype=F32)
    return p, m, v, g, ss


def fill_sentinel(buf):
    """Every element a distinct, recognisable bit pattern (no NaN: finite values, so a kernel that reads one poisons its result visibly)."""
    n = buf.numel()
    if buf.dtype == F32:
        buf.copy_((torch.arange(n, dtype=F64) % 977 + 1000.0).to(F32))
    else:
        buf.copy_((torch.arange(n, dtype=F32) % 97 + 300.0).to(BF16))
    return buf


def views(arrays, offs, dev="cpu"):
    """arrays: list of (tensor [n], offset).  -> (buffers, views): view i = buffer i[PAD + off : PAD + off + n], everything else sentinels."""
    bufs, vws = [], []
    for t, off in zip(arrays, offs):
        n = t.numel()
        b = fill_sentinel(torch.empty(n + 2 * PAD + off, dtype=t.dtype))
        b[PAD + off: PAD + off + n] = t
        b = b.to(dev)
        bufs.append(b)
        vws.append(b[PAD + off: PAD + off + n])
    return bufs, vws


def sentinels_intact(buf, off, n):
    want = fill_sentinel(torch.empty(buf.numel(), dtype=buf.dtype))
    fn = bits32 if buf.dtype == F32 else bits16
    lo, hi = PAD + off, PAD + off + n
    return torch.equal(fn(buf[:lo].cpu()), fn(want[:lo])) and torch.equal(fn(buf[hi:].cpu()), fn(want[hi:]))


def run_adamw(ops, case, dev="cpu", zero_grad=True, use_g16=False, inputs=None):
    """One step of `ops.adamw_step` on views at the case's offsets into sentinel-padded buffers.  -> dict(p, m, v, g, p16 views after the call, g_in, ss)
    after asserting that the sentinels on both sides of all five (six) views kept their bits."""
    p, m, v, g, ss = inputs if inputs is not None else adamw_inputs(case)
    n, o = case["n"], case["offs"]
    g16 = g.to(BF16) if use_g16 else None
    arrays = [p, m, v, g if not use_g16 else torch.full((n,), 7.0), torch.full((n,), -3.0).to(BF16)]
    offs = [o[0], o[1], o[2], o[3], o[4]]
    if use_g16:
        arrays.append(g16)
        offs.append(o[5])
    bufs, vw = views(arrays, offs, dev)
    g_before = vw[3].clone()
    ss_d = ss.to(dev) if ss is not None else None
    ops.adamw_step(vw[0], vw[1], vw[2], vw[3], vw[4], case["lr"], B1, B2, EPS, case["wd"], case["step"], sumsq=ss_d, max_norm=case["max_norm"],
                   grad_mult=case["gm"], zero_grad=zero_grad, **({"g16": vw[5]} if use_g16 else {}))
    if dev != "cpu":
        torch.cuda.synchronize()
    for b, off, what in zip(bufs, offs, ("p", "m", "v", "g", "p16", "g16")):
        assert sentinels_intact(b, off, n), "%s: %s sentinels next to the view changed" % (case["name"], what)
    if use_g16:
        assert torch.equal(bits16(vw[5]).cpu(), bits16(g16)), "%s: the bf16 gradient is read-only" % case["name"]
    if ss is not None:
        assert torch.equal(bits32(ss_d).cpu(), bits32(ss)), "%s: sumsq is read-only" % case["name"]
    return dict(p=vw[0], m=vw[1], v=vw[2], g=vw[3], p16=vw[4], g_before=g_before, g_used=(g16.float() if use_g16 else g), inputs=(p, m, v, g, ss))


def check_adamw(out, case, limit, dev="cpu"):
    """Bounds of A for one finished step + the exact properties every step has.  -> ratios."""
    p, m, v, g, ss = out["inputs"]
    where = dev if case["n"] > BIG_N else "cpu"
    to = lambda t: t.to(where)
    ref = ref_adamw(to(p), to(m), to(v), to(out["g_used"]), case["lr"], case["wd"], case["step"], ss, case["max_norm"], case["gm"])
    r = adamw_ratios(to(out["p"]), to(out["m"]), to(out["v"]), ref)
    assert torch.equal(bits16(out["p16"]), bits16(out["p"].to(BF16))), "%s: p16 != bf16(master after the step)" % case["name"]
    for k in ("p", "m", "v"):
        assert r[k] <= limit, "%s: %s error is %.3f of its bound (limit %.2f)" % (case["name"], k, r[k], limit)
    return r


# bf16 rounding (round to nearest even) of the master weights: lr = 0, wd = 0, m = v = g = 0 leave p exactly as it is (p * 1 - 0 * (0 / eps)), so the test
# controls the rounded bit pattern.  fp32 bit patterns and the bf16 pattern each must give.
BF16_PATTERNS = (
    (0x3F808000, 0x3F80),       # tie, even below: rounds down
    (0x3F818000, 0x3F82),       # tie, odd below: rounds up
    (0xBF808000, 0xBF80), (0xBF818000, 0xBF82),     # the same, negative
    (0x3F808001, 0x3F81),       # just above a tie
    (0x3F817FFF, 0x3F81),       # just below a tie
    (0x3FFF8000, 0x4000),       # tie that carries into the exponent: 1.99609375 -> 2.0
    (0x407F8000, 0x4080),
    (0x80000000, 0x8000),       # -0.0
    (0x00000000, 0x0000),
    (0x7F7F7FFF, 0x7F7F),       # largest fp32 that rounds to bf16 max
    (0x7F7F0000, 0x7F7F),
    (0x7F7F8000, 0x7F80),       # first that rounds to +inf (a tie with an odd pattern below)
    (0xFF7F7FFF, 0xFF7F), (0xFF7F8000, 0xFF80),
    (0x7F7FFFFF, 0x7F80),       # fp32 max
    (0x00000001, 0x0000),       # smallest fp32 denormal
    (0x007FFFFF, 0x0080),       # largest denormal: rounds up to the smallest normal bf16
    (0x00008000, 0x0000),       # denormal tie, even below
    (0x00018000, 0x0002),       # denormal tie, odd below
    (0x80018000, 0x8002),
    (0x00400000, 0x0040),       # a denormal bf16 represents exactly
)
BF16_N = 1024 + 3               # 22 patterns in rotation over 1027 elements: every pattern lands in every lane of the vector body and, at the three
                                # rotations below, in the 3-element scalar tail


def bf16_case(rot):
    """-> (p fp32 [BF16_N], expected bf16 bit patterns int16 [BF16_N]); element i holds pattern (i + rot) % len(BF16_PATTERNS)."""
    k = len(BF16_PATTERNS)
    idx = (torch.arange(BF16_N) + rot) % k
    src = torch.tensor([np.int32(np.uint32(a)) for a, _ in BF16_PATTERNS], dtype=torch.int32)[idx]
    dst = torch.tensor([np.int16(np.uint16(b)) for _, b in BF16_PATTERNS], dtype=torch.int16)[idx]
    return src.view(F32).clone(), dst


BF16_ROTATIONS = tuple(range(0, len(BF16_PATTERNS), 3)) + (1,)      # steps of 3: the 3-element tail sees every pattern; odd and even: every lane


# ---------------------------------------------------------------------------------------------------------------- B. exact sums
def int_data(n, seed, dtype=F32, budget=1 << 22):
    """Integers in {-2, ..., 2}, thinned so the squares sum to about `budget` at most (mean square of a kept element: 2)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (n,), generator=gen, dtype=torch.int8)
    keep = min(1.0, budget / (2.0 * max(n, 1)))
    if keep < 1.0:
        x = x * (torch.rand(n, generator=gen) < keep).to(torch.int8)
    return x.to(dtype)


def exact_sumsq(x):
    """Integer sum of squares of integer-valued data, asserted to stay below 2^24 (so fp32 summation is exact in any order)."""
    s = int((x.double() ** 2).sum().item())
    assert float(s) == float((x.double() ** 2).sum().item())
    assert s < EXACT_LIMIT, "sum of squares %d is not below 2^24" % s
    return s


SUMSQ_N = (1, 3, 4, 5, 1023, GRID_PASS + 3, 3 * GRID_PASS + 1)
OUT0 = 5.0                      # every `out` scalar starts here: the launchers accumulate


def sumsq_cases():
    """(name, dtype, n, view offset)."""
    c = []
    for n in SUMSQ_N:
        c.append(("f32-n%d" % n, F32, n, 0))
        c.append(("bf16-n%d" % n, BF16, n, 0))
    for off in (1, 2, 3):
        c.append(("f32-n4103-off%d" % off, F32, 4103, off))
    for off in range(1, 8):
        c.append(("bf16-n4111-off%d" % off, BF16, 4111, off))
    c.append(("f32-n%d-off3" % (GRID_PASS + 3), F32, GRID_PASS + 3, 3))
    c.append(("bf16-n%d-off5" % (GRID_PASS + 11), BF16, GRID_PASS + 11, 5))
    return c


def planted_positions(n, dtype):
    """Where a single 1 among zeros is planted: the last element of the vector body, each tail element, the first element of each later grid trip."""
    w, trip = (4, SUMSQ_PASS_F32) if dtype == F32 else (8, SUMSQ_PASS_BF16)
    body = (n // w) * w
    pos = set(range(body, n))
    if body:
        pos.add(body - 1)
        pos.add(0)
    t = trip
    while t < body:
        pos.add(t)
        pos.add(t - 1)
        t += trip
    return sorted(pos)


PARTIALS_N = (1, 255, 256, 257, 65535, 65536, 65537, 720000)


def partials_case(n, seed=3):
    """-> buffer fp32 [n + 256 + PAD]: n integer partials (0 .. 3, thinned), 256 scratch floats of junk, PAD sentinels; and the exact sum."""
    gen = torch.Generator().manual_seed(seed + n)
    x = torch.randint(0, 4, (n,), generator=gen).to(F32)
    if n > (1 << 21):
        x = x * (torch.rand(n, generator=gen) < 0.5)
    buf = fill_sentinel(torch.empty(n + 256 + PAD, dtype=F32))
    buf[:n] = x
    s = int(x.double().sum().item())
    assert s < EXACT_LIMIT
    return buf, s


def periodic_cases():
    """(name, base, stride, count, ranges): 1, 3 and 8 ranges; an empty range; a range longer than 64 * 256 elements (more than one trip of the 64-block
    grid); a base that is not a multiple of 4; count 1, 28 and 80."""
    return (
        ("r1-count28", 3, 20011, 28, [(5, 20005)]),
        ("r3-count80", 6, 18001, 80, [(0, 7), (100, 100), (1001, 18001)]),
        ("r8-count1", 1, 40000, 1, [(0, 1), (3, 3), (4, 260), (261, 517), (600, 601), (1000, 18000), (18001, 18256), (39999, 40000)]),
        ("r3-count1-short", 5, 777, 1, [(0, 3), (10, 266), (776, 777)]),
        ("r8-count28", 2, 3000, 28, [(0, 1), (1, 2), (5, 5), (7, 300), (301, 302), (1000, 1255), (2000, 2999), (2999, 3000)]),
    )


def periodic_mask(n, base, stride, count, ranges):
    m = torch.zeros(n, dtype=torch.bool)
    for l in range(count):
        for a, b in ranges:
            m[base + l * stride + a: base + l * stride + b] = True
    return m


def periodic_arena(case, kind, tail=9):
    """-> (arena fp32, mask, exact in-range sum).  kind "in": integers inside the ranges, zeros outside; "out": zeros inside, large values outside
    (the sum must add exactly 0); "mixed": integers inside, large values outside (which must not be read)."""
    name, base, stride, count, ranges = case
    n = base + stride * count + tail
    mask = periodic_mask(n, base, stride, count, ranges)
    ints = torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(17 + count)).to(F32)
    ints[ints == 0] = 1.0               # every in-range element counts: a single one missed changes the sum
    big = (torch.arange(n, dtype=F32) % 13 + 1.0) * 4099.0
    zero = torch.zeros(n)
    inside, outside = {"in": (ints, zero), "out": (zero, big), "mixed": (ints, big)}[kind]
    arena = torch.where(mask, inside, outside)
    return arena, mask, exact_sumsq(arena[mask])


# ---- wgrad_sumsq
def _replay(N, K, kmajor):
    """Replay of the integer cost model in tr1_wgrad_f32_sumsq (csrc/gemm.hip) for a gradient of N rows x K columns: tile height in rows.  The NT form
    starts from 224 and takes a taller tile only when strictly cheaper (the NT GEMM dispatch's own choice); the K-major form starts from 256 (nt8p_pick_rt with first = 224 / 256)."""
    t2n = (K + 255) // 256

    def cost(bm, eff):
        t = ((N + bm - 1) // bm) * t2n
        return float((t + 255) // 256) * 256.0 * float(bm * 256) / eff
    eff = (0.94, 1.0, 1.025, 1.03)
    if kmajor:
        rt, best, rng = 8, cost(256, 1.0), range(7, 11)
    else:
        rt, best, rng = 7, cost(224, eff[0]), range(8, 11)
    for r in rng:
        c = cost(r * 32, eff[r - 7])
        if c < best:
            best, rt = c, r
    return rt * 32


def wgrad_tile_rows(N, K, kmajor):
    return _replay(N, K, kmajor)


# (N rows of the gradient, K columns, Mp padded tokens, valid tokens, tile height both operand forms must pick).  K = 1032 = 4 x 256 + 8: a partial
# column tile; no N is a multiple of its tile height: a partial row tile.  If the launcher's rule changes, the CPU replay test fails: re-pick.
WGRAD_SHAPES = ((1000, 520, 128, 100, 224), (12500, 1032, 64, 50, 256), (13900, 1032, 64, 50, 288), (15000, 1032, 64, 50, 320))
WGRAD_OFFSET = 1000             # partial sums go to part[WGRAD_OFFSET : WGRAD_OFFSET + n]
PLANT_BIG = (3.0e38, float("inf"), -3.0e38, 1.0e4)       # what rows / columns the kernel must not read hold (0 * inf would show as NaN)


def _sparse_ints(shape, seed, density, hi=2):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(1, hi + 1, shape, generator=gen).float() * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
    return x * (torch.rand(shape, generator=gen) < density)


def wgrad_case(N, K, Mp, T, seed=5):
    """-> dy [Mp, N], x [Mp, K], gw0 [N, K] (fp32 tensors holding small integers; rows T.. of dy are the zero padding, rows T.. of x hold PLANT_BIG),
    gw_over = dy^T x and gw_acc = gw0 + dy^T x in fp64 (exact integers).  Density chosen so that both gradients' squares sum to about 2^22."""
    d = math.sqrt(0.25 * (1 << 22) / (N * K) / (T * 6.25))
    d = min(d, 0.5)
    dy = torch.zeros(Mp, N)
    x = torch.zeros(Mp, K)
    dy[:T] = _sparse_ints((T, N), seed, d)
    x[:T] = _sparse_ints((T, K), seed + 1, d)
    gw_over = dy[:T].double().t() @ x[:T].double()
    for i in range(T, Mp):
        x[i] = PLANT_BIG[(i - T) % len(PLANT_BIG)]
    gw0 = _sparse_ints((N, K), seed + 2, 0.25 * (1 << 22) / (N * K) / 4.7, hi=3)
    return dy, x, gw0, gw_over, gw0.double() + gw_over


def framed(t, rows=1, cols=8, fill=None, dev="cpu"):
    """t [R, C] -> (buffer [R + 2 rows, C + cols], view = buffer[rows : rows + R, :C]).  The frame holds `fill` values (default: the sentinels)."""
    R, C = t.shape
    buf = torch.empty(R + 2 * rows, C + cols, dtype=t.dtype)
    if fill is None:
        fill_sentinel(buf.view(-1))
    else:
        buf.view(-1).copy_(torch.tensor(fill, dtype=F32).repeat(buf.numel() // len(fill) + 1)[: buf.numel()])
    buf[rows: rows + R, :C] = t
    buf = buf.to(dev)
    return buf, buf[rows: rows + R, :C]


def frame_intact(buf, R, C, rows=1):
    """The sentinel frame of a `framed` buffer kept its bits."""
    want = fill_sentinel(torch.empty(buf.numel(), dtype=buf.dtype)).view(buf.shape)
    fn = bits32 if buf.dtype == F32 else bits16
    got = buf.cpu()
    keep = torch.ones(buf.shape, dtype=torch.bool)
    keep[rows: rows + R, :C] = False
    return torch.equal(fn(got[keep]), fn(want[keep]))


# ---- composition
def zero_plan_cover(n, spans, small, lz):
    """Times every index of [0, n) is covered by: the spans AdamW zeroes itself, the small ranges of every period, the keep ranges of every period."""
    cover = torch.zeros(n, dtype=torch.int32)
    for x, y, z in spans:
        if z:
            cover[x:y] += 1
    for l in range(lz["count"]):
        o = lz["base"] + l * lz["stride"]
        for a, b in list(small or []) + list(lz["keep"]):
            cover[o + a: o + b] += 1
    return cover


def random_plan(seed):
    """A random lazy-zero plan (n, dict(base, stride, count, keep)) of the form Engine.lazy_zero_plan returns: sorted, disjoint keep ranges inside one period,
    at most 7 of them (so at most 8 small ranges), possibly touching the period's ends or each other."""
    r = np.random.RandomState(seed)
    count = int(r.choice([1, 2, 5, 28]))
    nk = int(r.randint(1, 8))
    cuts = sorted(int(c) for c in r.choice(np.arange(0, 400), size=2 * nk, replace=True))
    if r.rand() < 0.3:
        cuts[0] = 0             # a matrix at the very start of the period
    keep = [(cuts[2 * i], cuts[2 * i + 1]) for i in range(nk) if cuts[2 * i + 1] > cuts[2 * i]]
    stride = (cuts[-1] if r.rand() < 0.3 else cuts[-1] + int(r.randint(0, 50)))
    stride = max(stride, 1)
    base = int(r.randint(0, 30)) if r.rand() < 0.8 else 0
    tail = int(r.randint(0, 30)) if r.rand() < 0.8 else 0
    return base + stride * count + tail, dict(base=base, stride=stride, count=count, keep=keep)


def launcher_source(name, path):
    """Whitespace-flattened body of one extern "C" launcher (to pin the constants a replay copies)."""
    src = open(path).read()
    body = src[src.index('extern "C" int %s(' % name):]
    nxt = body.find('extern "C"', 10)
    return re.sub(r"\s+", " ", body[: nxt if nxt > 0 else len(body)]), src
