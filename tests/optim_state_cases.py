"""Cases and checks for AdamW with bf16 moments and stochastic rounding (GRPOConfig.optimizer_state_dtype="bf16"; tr1_adamw_step_sr16, csrc/optim.hip).
Shared by tests/test_optim_state_ref.py (CPU) and tests/test_optim_state_gpu.py (the HIP kernel against the same emulation, bit for bit).  The emulation
itself lives in oracle/sr16.py (RefOps.adamw_step_sr16, the CPU stand-in, stores its moments) and is re-exported here.

The step, from bf16 moments m, v (widened exactly) and fp32 p, g, with EVERY fp32 operation rounded once (numpy float32, no fused multiply-add):

  coef = grad_mult * min(1, max_norm / (sqrt(sumsq) * grad_mult + 1e-6))      when sumsq is given and max_norm > 0, else grad_mult
  gg   = g * coef
  m'   = b1 * m + (1 - b1) * gg
  v'   = b2 * v + ((1 - b2) * gg) * gg
  p'   = the fp32-state step's from the same inputs (the UNROUNDED m', v'), p16 = bf16_rne(p')
  m16' = sr(m', low 16 bits of the element's random word),  v16' = sr(v', its high 16 bits)

sr(x, r) on the fp32 bits b of x: mag = b & 0x7fffffff; inf / NaN -> nearest even; else s = min(mag + r, 0x7f7fffff), result ((b & 0x80000000) | s) >> 16.
So the value goes AWAY from zero exactly when r >= 65536 - (b & 0xffff) (and the result is not clamped), a value bf16 holds keeps its bits, and the mean
over r is the value.

Random word of the GLOBAL element e = index_base + i: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter ((e >> 2) & 0xffffffff, (e >> 2) >> 32,
step & 0xffffffff, 0x53523136), output word e & 3.  oracle.sr16.philox4x32_10 is a vectorised copy of oracle.ref_ops.philox4x32_10, checked against it.

m16' and v16' are compared BIT FOR BIT with the kernel; p' against the fp64 reference optim_cases.ref_adamw applied to the bf16-valued moments, within
optim_cases.adamw_bounds (the moments' widening is exact, so the bounds of the fp32-state kernel hold unchanged).
"""
import numpy as np
import torch

import optim_cases as oc
from oracle.ref_ops import RefOps
from oracle.sr16 import (STREAM, MASK, philox4x32_10, random_words, f32_bits, bf16_rne_bits, sr_round, bf16_to_np, bits_to_bf16,  # noqa: F401
                         emu_coef, emu_moments, emu_step)

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SR16_GRID_CAP = 4096                    # blocks of adamw_sr16_kernel's capped grid (csrc/optim.hip, pinned by test_optim_state_ref.py)
SR16_PASS = SR16_GRID_CAP * 256 * 8     # elements one grid trip covers: 2^23 = 2 * oc.GRID_PASS, so oc.GRID_PASS + 3 elements are ONE partial trip and a tail
TWO_TRIPS_N = SR16_PASS + 8 * 256 * 3 + 5   # the one case beyond it: a full trip, three blocks' worth of a second one, a 5-element tail


class RneOps(RefOps):
    """The same step with the moments rounded to NEAREST EVEN: what the feature is not (a decaying v never leaves 1.0)."""

    def adamw_step_sr16(self, p32, m16, v16, g, p16, lr, beta1, beta2, eps, weight_decay, step, seed, index_base, sumsq=None, max_norm=0.0, grad_mult=1.0,
                        zero_grad=True, g16=None):
        _, _, mn, vn = emu_step(m16, v16, g16.float() if g16 is not None else g, beta1, beta2, step, seed, index_base, None if sumsq is None else float(sumsq),
                                max_norm, grad_mult)
        m16.copy_(torch.from_numpy(mn).to(BF16))
        v16.copy_(torch.from_numpy(vn).to(BF16))


# ---------------------------------------------------------------------------------------------------------------- cases
def bf16_state(case):
    """optim_cases.adamw_inputs with both moments first rounded to bf16 (nearest even; v stays >= 0)."""
    p, m, v, g, ss = oc.adamw_inputs(case)
    return p, m.to(BF16), v.to(BF16), g, ss


def kernel_cases():
    """optim_cases.adamw_cases() up to n = GRID_PASS + 3, each with an index_base: multiples of 4 and not, and two above 2^32.  The kernel's grid is capped at
    4096 blocks x 256 lanes x 8 elements, so none of those lengths enters the grid-stride loop twice (3 * GRID_PASS + 1 would not either: left out as redundant);
    TWO_TRIPS_N is added for that."""
    bases = (0, 1, 2, 3, 4, 6, (1 << 32) + 5, 64, (1 << 33) + 8, 7)
    out = []
    for i, c in enumerate(x for x in oc.adamw_cases() if x["n"] <= oc.GRID_PASS + 3):
        out.append(dict(c, index_base=bases[i % len(bases)], sr_seed=(0x9E3779B97F4A7C15 * (i + 1)) & 0xFFFFFFFFFFFFFFFF))
    for n in (7, 8, 9):
        out.append(dict(oc._case("n%d" % n, n, "trained", 2e-5, 0.01, 3), index_base=(n * 5) % 7, sr_seed=n))
    out.append(dict(oc._case("n%d-two-trips" % TWO_TRIPS_N, TWO_TRIPS_N, "trained", 2e-5, 0.01, 3), index_base=(1 << 34) - 4099, sr_seed=12345))      # the block counter e >> 2 carries into its high word inside the array
    return out


def run_sr16(ops, case, dev="cpu", zero_grad=True, use_g16=False, inputs=None, index_base=None, seed=None):
    """One ops.adamw_step_sr16 call on views at the case's offsets into sentinel-padded buffers (the m / v views take the case's p16 / g16 offsets too: odd
    bf16 offsets) -> dict of the views after the call, after asserting that the sentinels on both sides of every view kept their bits."""
    p, m16, v16, g, ss = inputs if inputs is not None else bf16_state(case)
    n, o = case["n"], case["offs"]
    g16 = g.to(BF16) if use_g16 else None
    arrays = [p, m16, v16, g if not use_g16 else torch.full((n,), 7.0), torch.full((n,), -3.0).to(BF16)]
    offs = [o[0], o[1] + o[4], o[2] + o[5], o[3], o[4]]
    if use_g16:
        arrays.append(g16)
        offs.append(o[5])
    bufs, vw = oc.views(arrays, offs, dev)
    g_before = vw[3].clone()
    ss_d = ss.to(dev) if ss is not None else None
    ib = case.get("index_base", 0) if index_base is None else index_base
    sd = case.get("sr_seed", 1) if seed is None else seed
    ops.adamw_step_sr16(vw[0], vw[1], vw[2], vw[3], vw[4], case["lr"], oc.B1, oc.B2, oc.EPS, case["wd"], case["step"], sd, ib, sumsq=ss_d,
                        max_norm=case["max_norm"], grad_mult=case["gm"], zero_grad=zero_grad, **({"g16": vw[5]} if use_g16 else {}))
    if dev != "cpu":
        torch.cuda.synchronize()
    for b, off, what in zip(bufs, offs, ("p", "m16", "v16", "g", "p16", "g16")):
        assert oc.sentinels_intact(b, off, n), "%s: %s sentinels next to the view changed" % (case["name"], what)
    if use_g16:
        assert torch.equal(oc.bits16(vw[5]).cpu(), oc.bits16(g16)), "%s: the bf16 gradient is read-only" % case["name"]
    if ss is not None:
        assert torch.equal(oc.bits32(ss_d).cpu(), oc.bits32(ss)), "%s: sumsq is read-only" % case["name"]
    return dict(p=vw[0], m16=vw[1], v16=vw[2], g=vw[3], p16=vw[4], g_before=g_before, g_used=(g16.float() if use_g16 else g), inputs=(p, m16, v16, g, ss),
                index_base=ib, seed=sd)


def check_sr16(out, case, dev="cpu", limit=1.0):
    """m16 / v16 bit-equal to the emulation on every element; p within adamw_bounds of the fp64 step from the bf16-valued moments; p16 == bf16(p).  -> p ratio."""
    p, m16, v16, g, ss = out["inputs"]
    mb, vb, _, _ = emu_step(m16, v16, out["g_used"], oc.B1, oc.B2, case["step"], out["seed"], out["index_base"], None if ss is None else float(ss),
                            case["max_norm"], case["gm"])
    got_m = out["m16"].cpu().contiguous().view(torch.int16).numpy().astype(np.uint16)
    got_v = out["v16"].cpu().contiguous().view(torch.int16).numpy().astype(np.uint16)
    bad_m, bad_v = int((got_m != mb).sum()), int((got_v != vb).sum())
    assert bad_m == 0 and bad_v == 0, "%s: %d m16 and %d v16 elements of %d differ from the emulation (first m %s, first v %s)" % (
        case["name"], bad_m, bad_v, case["n"], np.flatnonzero(got_m != mb)[:4], np.flatnonzero(got_v != vb)[:4])
    where = dev if case["n"] > oc.BIG_N else "cpu"
    to = lambda t: t.to(where)
    ref = oc.ref_adamw(to(p), to(m16.float()), to(v16.float()), to(out["g_used"]), case["lr"], case["wd"], case["step"], ss, case["max_norm"], case["gm"])
    r = oc.worst((to(out["p"]).double() - ref["p"]).abs(), oc.adamw_bounds(ref)["p"])
    assert r <= limit, "%s: p error is %.3f of its bound (limit %.2f)" % (case["name"], r, limit)
    assert torch.equal(oc.bits16(out["p16"]), oc.bits16(out["p"].to(BF16))), "%s: p16 != bf16(master after the step)" % case["name"]
    return r


# ---- rounding patterns driven through a real step made exact
def _pattern_bits():
    pats = []
    for a, _ in oc.BF16_PATTERNS:
        for b in (a, a ^ 0x80000000):
            if b not in pats:
                pats.append(b)
    return pats


PATTERN_REPEAT = 4096                   # elements per pattern: with 16 random bits each, both neighbours occur (a pattern one fp32 step from a bf16 value
#                                         moves with probability 2^-16 per element; those are checked against the rule, not for both outcomes)


def m_pattern_case(big):
    """m = v = 0, lr = 0, no clipping, grad_mult = 1.  big = False: beta1 = 0.5 and g = 2 x pattern, so m' = 0.5 * 0 + 0.5 * g = pattern exactly (every pattern
    whose double is finite).  big = True: the patterns at the top of the range, whose double overflows; there beta1 = 0 and g = pattern: m' = 0 * 0 + 1 * g.
    The zero m starts from carries the pattern's sign only for the pattern -0.0 (0.5 * (+0) + 0.5 * (-0) is +0 in IEEE arithmetic: -0.0 has to come from -0.0).
    -> (m16 bf16 tensor, g fp32 tensor, beta1, expected unrounded m' as uint32 bit patterns)."""
    pats = [b for b in _pattern_bits() if ((b & 0x7FFFFFFF) >= 0x7F000000) == big]
    want = np.repeat(np.array(pats, dtype=np.uint32), PATTERN_REPEAT)
    x = want.view(np.float32)
    g = x.copy() if big else (x * np.float32(2.0))
    assert np.isfinite(g).all()
    m16 = bits_to_bf16(np.where(want == np.uint32(0x80000000), 0x8000, 0).astype(np.uint16))
    return m16, torch.from_numpy(g), (0.0 if big else 0.5), want


def v_pattern_case():
    """beta2 = 0.5, v = 0, g with significands of at most 12 bits: v' = 0.5 * 0 + (0.5 * g) * g = 0.5 g^2 exactly (24 bits).  Covers zero, both signs of g (v' >= 0),
    values bf16 holds exactly (g a power of two), denormal results and the top of the range, where rounding up would reach inf and is clamped to 0x7F7F.
    -> (g fp32 tensor, expected unrounded v' bits)."""
    sig = np.array([2048, 2049, 2895, 3000, 4095, 2896, 2304], dtype=np.float64) / 2048.0      # 12-bit significands in [1, 2)
    exps = np.array([0, 1, -7, 20, -40, -63, -70, 64], dtype=np.float64)                         # 2^64 * 2895/2048: 0.5 g^2 = 1.998 * 2^127, below fp32 max
    vals = [0.0, -0.0]
    for e in exps:
        for s in sig:
            if e == 64 and s > 2896 / 2048.0:
                continue                                  # 0.5 g^2 would overflow
            vals += [s * 2.0 ** e, -s * 2.0 ** e]
    vals = np.array(vals, dtype=np.float32)
    with np.errstate(under="ignore"):
        exact = ((np.float32(0.5) * vals) * vals).astype(np.float64) == 0.5 * vals.astype(np.float64) ** 2
    vals = vals[exact]                                    # in the denormal range only some of the 24-bit products fit: keep those
    assert vals.size >= 100 and (np.abs(vals) < 2.0 ** -60).sum() >= 20
    g = np.repeat(vals, PATTERN_REPEAT)
    with np.errstate(under="ignore"):
        want = (np.float32(0.5) * g) * g
    assert np.isfinite(want).all() and (want.astype(np.float64) == 0.5 * g.astype(np.float64) ** 2).all(), "0.5 g^2 must be exact in fp32"
    return torch.from_numpy(g), f32_bits(want)


def away_rule(bits, r16):
    """What the rule means, written independently of sr_round: truncate towards zero, then one bf16 step away from zero exactly when r >= 65536 - low16 (low16 != 0),
    never past the largest finite bf16."""
    bits = np.asarray(bits, dtype=np.uint32)
    hi, low = (bits >> np.uint32(16)).astype(np.uint32), (bits & np.uint32(0xFFFF)).astype(np.uint32)
    up = (low != 0) & (np.asarray(r16, dtype=np.uint32) >= (np.uint32(65536) - low))
    out = hi + up.astype(np.uint32)
    clamp = (out & np.uint32(0x7FFF)) > np.uint32(0x7F7F)
    return np.where(clamp, (out & np.uint32(0x8000)) | np.uint32(0x7F7F), out).astype(np.uint16)


# ---- the two checks both files run: on the stand-in (CPU) and on the kernel
def _pattern_step(ops, m16, g, b1, b2, seed, step, dev="cpu", index_base=0):
    n = g.numel()
    p, p16, v16 = torch.zeros(n, device=dev), torch.zeros(n, dtype=BF16, device=dev), torch.zeros(n, dtype=BF16, device=dev)
    m16, gd = m16.clone().to(dev), g.clone().to(dev)
    ops.adamw_step_sr16(p, m16, v16, gd, p16, 0.0, b1, b2, oc.EPS, 0.0, step, seed, index_base, sumsq=None, max_norm=0.0, grad_mult=1.0, zero_grad=False)
    assert torch.equal(oc.bits32(gd).cpu(), oc.bits32(g)), "zero_grad off: the gradient is untouched"
    return m16.cpu(), v16.cpu()


def check_patterns(ops, dev="cpu"):
    """The rounding-pattern case (shared with the GPU file): m' and v' are made exact, so the stored bits are the rule applied to known fp32 bits."""
    seed, step = 0xC0FFEE1234, 3
    for big in (False, True):
        m0, g, b1, want = m_pattern_case(big)
        m16, _ = _pattern_step(ops, m0, g, b1, 0.5, seed, step, dev, index_base=5)
        r = random_words(g.numel(), seed, step, 5) & np.uint32(0xFFFF)
        got = m16.view(torch.int16).numpy().astype(np.uint16)
        assert (got == sr_round(want.view(np.float32), r)).all(), "m: the rule"
        assert (got == away_rule(want, r)).all(), "m: away from zero exactly when r >= 65536 - low16, clamped at the largest finite bf16"
        _check_pattern_outcomes(want, got)
    g, want = v_pattern_case()
    _, v16 = _pattern_step(ops, torch.zeros(g.numel(), dtype=BF16), g, 0.5, 0.5, seed, step, dev, index_base=6)
    r = random_words(g.numel(), seed, step, 6) >> np.uint32(16)
    got = v16.view(torch.int16).numpy().astype(np.uint16)
    assert (got == sr_round(want.view(np.float32), r)).all() and (got == away_rule(want, r)).all(), "v: the rule, from the word's HIGH half"
    assert (got < 0x8000).all(), "v stays >= 0 (and +0: no -0.0 either)"
    _check_pattern_outcomes(want, got)


def _check_pattern_outcomes(want, got):
    for b in np.unique(want):
        sel = got[want == b]
        hi, low, mag_hi = int(b) >> 16, int(b) & 0xFFFF, (int(b) >> 16) & 0x7FFF
        if low == 0:
            assert (sel == hi).all(), "a value bf16 holds (zeros and -0.0 included) keeps its bits: %08x" % b
        elif mag_hi == 0x7F7F:
            assert (sel == hi).all(), "the largest finite values clamp to 0x7F7F, never inf: %08x" % b
        else:
            assert set(sel.tolist()) <= {hi, hi + 1}, "%08x" % b
            if 8192 <= low <= 65536 - 8192:      # each neighbour has probability >= 1/8: both occur among the 4096 draws
                assert set(sel.tolist()) == {hi, hi + 1}, "both neighbours occur: %08x" % b
                share = float((sel == hi + 1).mean())
                assert abs(share - low / 65536.0) < 5 * 0.5 / np.sqrt(sel.size), "rounds away with probability low16 / 65536: %08x %.4f" % (b, share)


def _state(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * 0.05, (torch.randn(n, generator=g) * 3e-3).to(BF16), ((torch.randn(n, generator=g) * 1e-2) ** 2).to(BF16),
            torch.randn(n, generator=g) * 1e-2)


def _call(ops, st, lo, hi, seed, step, base0=0, dev="cpu"):
    p, m, v, g = (t.clone().to(dev) for t in st)
    p16 = torch.zeros(p.numel(), dtype=BF16, device=dev)
    ss = (st[3].double() ** 2).sum().to(F32).reshape(1).to(dev)
    for a, b in zip(lo, hi):
        ops.adamw_step_sr16(p[a:b], m[a:b], v[a:b], g[a:b], p16[a:b], 1e-3, oc.B1, oc.B2, oc.EPS, 0.01, step, seed, base0 + a, sumsq=ss, max_norm=1.0, grad_mult=0.5)
    return [oc.bits32(p).cpu(), oc.bits16(m).cpu(), oc.bits16(v).cpu(), oc.bits16(p16).cpu(), oc.bits32(g).cpu()]


def check_keying(ops, dev="cpu"):
    """One call over [0, n) equals three calls over [0, a), [a, b), [b, n) with index_base 0, a, b (a, b not multiples of 4); seed and step matter; same -> same."""
    n, a, b = 4103, 1021, 2050
    st = _state(n)
    for base0 in (0, (1 << 32) + 3):
        whole = _call(ops, st, [0], [n], 11, 4, base0, dev)
        parts = _call(ops, st, [0, a, b], [a, b, n], 11, 4, base0, dev)
        assert all(torch.equal(x, y) for x, y in zip(whole, parts)), "splitting a range must not change a bit (index_base %d)" % base0
    whole = _call(ops, st, [0], [n], 11, 4, 0, dev)
    again = _call(ops, st, [0], [n], 11, 4, 0, dev)
    assert all(torch.equal(x, y) for x, y in zip(whole, again))
    for kw in (dict(seed=12, step=4), dict(seed=11 + (1 << 32), step=4), dict(seed=11, step=5)):
        other = _call(ops, st, [0], [n], kw["seed"], kw["step"], 0, dev)
        assert not torch.equal(whole[1], other[1]) and not torch.equal(whole[2], other[2]), kw
    shifted = _call(ops, st, [0], [n], 11, 4, 1, dev)
    assert not torch.equal(whole[1], shifted[1]), "index_base is part of the key"
    return whole


# ---- the decay that nearest-even cannot follow
DECAY_N, DECAY_STEPS, DECAY_SEED = 65536, 100, 20240607
DECAY_BOUND = 4e-4      # five standard deviations of the mean over 65 536 elements when every step's error is at most half the bf16 spacing 2^-8 below 1
#                         (a two-point error has at most that standard deviation): 5 * sqrt(100) * 2^-9 / sqrt(65536) = 3.8e-4


def decay_want():
    x = np.float64(np.float32(0.999))
    return float(x ** DECAY_STEPS)


def run_decay(ops, dev="cpu", steps=DECAY_STEPS, seed=DECAY_SEED):
    """v = 1, g = 0, beta2 = f32(0.999), `steps` steps through ops.adamw_step_sr16 -> the bf16 v tensor (on the CPU)."""
    n = DECAY_N
    p, g, m16, v16 = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, dtype=BF16, device=dev), torch.ones(n, dtype=BF16, device=dev)
    p16 = torch.zeros(n, dtype=BF16, device=dev)
    for s in range(1, steps + 1):
        ops.adamw_step_sr16(p, m16, v16, g, p16, 0.0, oc.B1, oc.B2, oc.EPS, 0.0, s, seed, 0, sumsq=None, max_norm=0.0, grad_mult=1.0, zero_grad=False)
    return v16.cpu()


# ---- AdamWFlat on a tiny arena
def tiny_params(ops, moment_dtype=F32, seed=0):
    from time_r1_amd.config import tiny_test
    from time_r1_amd.params import ModelParams
    return ModelParams(tiny_test(), ops, seed=seed, moment_dtype=moment_dtype)


def exact_grad(numel, k, world=1):
    """Gradient k of a run: small integers / 64, so that the sum of squares is exact in fp32 in ANY order and partition (the replicated optimizer sums the
    whole arena, the sharded one its shards and then the ranks), also after the ranks' gradients - `world` equal copies - are added.  The norm is far
    above max_grad_norm = 1: the clip coefficient is active and depends on every bit of that sum."""
    assert world in (1, 2, 4, 8)          # a power of two scales every partial sum exactly: the integer sum below is what has to stay under 2^24
    g = torch.randint(-4, 5, (numel,), generator=torch.Generator().manual_seed(1000 + k)).float()
    assert float((g.double() ** 2).sum()) < oc.EXACT_LIMIT
    return g / 64.0


def flat_steps(opt, grads, dev="cpu", start=0):
    """Feed the given gradients, one optimizer step each."""
    a = opt.params.train
    for g in grads[start:]:
        a.grad.copy_(g.to(dev))
        opt.step()
    if dev != "cpu":
        torch.cuda.synchronize()


def state_bits(a):
    return dict(master=oc.bits32(a.master).cpu().clone(), m=oc.bits16(a.m).cpu().clone(), v=oc.bits16(a.v).cpu().clone(),
                w16=(oc.bits16(a.w16) if a.w16.dtype == BF16 else oc.bits32(a.w16)).cpu().clone())
