"""ORACLE - TEST INFRASTRUCTURE ONLY.  Emulation of AdamW with bf16 moments and stochastic rounding (tr1_adamw_step_sr16, csrc/optim.hip): what
RefOps.adamw_step_sr16 stores, and what tests/optim_state_cases.py compares the kernel with bit for bit.

The step, from bf16 moments m, v (widened exactly) and fp32 p, g, with EVERY fp32 operation rounded once (numpy float32, no fused multiply-add):

  coef = grad_mult * min(1, max_norm / (sqrt(sumsq) * grad_mult + 1e-6))      when sumsq is given and max_norm > 0, else grad_mult
  gg   = g * coef
  m'   = b1 * m + (1 - b1) * gg
  v'   = b2 * v + ((1 - b2) * gg) * gg
  m16' = sr(m', low 16 bits of the element's random word),  v16' = sr(v', its high 16 bits)

sr(x, r) on the fp32 bits b of x: mag = b & 0x7fffffff; inf / NaN -> nearest even; else s = min(mag + r, 0x7f7fffff), result ((b & 0x80000000) | s) >> 16.
So the value goes AWAY from zero exactly when r >= 65536 - (b & 0xffff) (and the result is not clamped), a value bf16 holds keeps its bits, and the mean
over r is the value.

Random word of the GLOBAL element e = index_base + i: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter ((e >> 2) & 0xffffffff, (e >> 2) >> 32,
step & 0xffffffff, 0x53523136), output word e & 3.  philox4x32_10 below is a vectorised copy of oracle.ref_ops.philox4x32_10, checked against it
(tests/test_optim_state_ref.py).
"""
import numpy as np
import torch

BF16 = torch.bfloat16
STREAM = 0x53523136
MASK = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------- random bits
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over the counters (uint64 arrays that hold 32-bit words); k0, k1 Python ints.  -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3))
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                     # 32 x 32 bit products: exact in uint64
        h0, l0, h1, l1 = p0 >> sh, p0 & MASK, p1 >> sh, p1 & MASK
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def random_words(n, seed, step, index_base=0):
    """-> uint32 [n]: the random word of elements index_base .. index_base + n."""
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    q0, q1 = int(index_base) >> 2, (int(index_base) + n - 1) >> 2
    q = np.arange(q0, q1 + 1, dtype=np.uint64)
    w = philox4x32_10(q & MASK, q >> np.uint64(32), np.full(q.shape, int(step) & 0xFFFFFFFF, dtype=np.uint64), np.full(q.shape, STREAM, dtype=np.uint64),
                      int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    flat = np.stack(w, axis=1).reshape(-1).astype(np.uint32)
    lo = int(index_base) - 4 * q0
    return flat[lo: lo + n]


# ---------------------------------------------------------------------------------------------------------------- the rounding rule
def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def bf16_rne_bits(x):
    """torch's nearest-even fp32 -> bf16 conversion, as uint16 bit patterns."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(BF16)
    return t.view(torch.int16).numpy().astype(np.uint16)


def sr_round(x, r16):
    """fp32 array x, 16-bit random values r16 (any unsigned dtype) -> uint16 bf16 bit patterns by the rule in the header."""
    b = f32_bits(x).astype(np.uint64)
    mag = b & np.uint64(0x7FFFFFFF)
    s = np.minimum(mag + np.asarray(r16, dtype=np.uint64), np.uint64(0x7F7FFFFF))
    out = (((b & np.uint64(0x80000000)) | s) >> np.uint64(16)).astype(np.uint16)
    special = mag >= np.uint64(0x7F800000)
    if special.any():
        out = np.where(special, bf16_rne_bits(x), out)
    return out


def bf16_to_np(t):
    """bf16 tensor -> the float32 numpy array of the same values (exact)."""
    return (t.detach().cpu().contiguous().view(torch.int16).numpy().astype(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bits_to_bf16(bits):
    """uint16 bit patterns -> bf16 tensor."""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16).copy()).view(BF16)


# ---------------------------------------------------------------------------------------------------------------- the step
def emu_coef(sumsq, max_norm, grad_mult):
    f = np.float32
    gm = f(grad_mult)
    if sumsq is None or not max_norm > 0:
        return gm
    norm = f(np.sqrt(f(sumsq)) * gm)
    den = f(norm + f(1e-6))
    return f(gm * min(f(1.0), f(f(max_norm) / den)))


def emu_moments(m, v, g, beta1, beta2, sumsq=None, max_norm=0.0, grad_mult=1.0):
    """float32 numpy arrays m, v, g -> the unrounded fp32 m', v' (every operation rounded once)."""
    f = np.float32
    b1, b2 = f(beta1), f(beta2)
    gg = g * emu_coef(sumsq, max_norm, grad_mult)
    mn = b1 * m + (f(1.0) - b1) * gg
    vn = b2 * v + ((f(1.0) - b2) * gg) * gg
    assert mn.dtype == np.float32 and vn.dtype == np.float32
    return mn, vn


def emu_step(m16, v16, g, beta1, beta2, step, seed, index_base, sumsq=None, max_norm=0.0, grad_mult=1.0):
    """bf16 tensors m16, v16 and the fp32 gradient the kernel reads (tensor) -> uint16 bit patterns of the stored m16', v16' and the unrounded fp32 m', v'."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        mn, vn = emu_moments(bf16_to_np(m16), bf16_to_np(v16), g.detach().cpu().float().contiguous().numpy(), beta1, beta2,
                             None if sumsq is None else float(sumsq), max_norm, grad_mult)
    w = random_words(mn.size, seed, step, index_base)
    return sr_round(mn, w & np.uint32(0xFFFF)), sr_round(vn, w >> np.uint32(16)), mn, vn
