"""Seeded cases and fp64 references for the vocabulary-side kernels (csrc/loss.hip, csrc/sampler.hip and the lmhead_lse tail of csrc/gemm.hip).

Shared by tests/test_vocab_side_ref.py (CPU: the fp32 oracle against these references) and tests/test_vocab_side_gpu.py (the HIP kernels against
the same references on the same cases).  Everything here is plain torch / numpy on the CPU, written from the formulas:

  logp[r] = x[r, t_r] - lse[r],  lse = log sum_v exp x,  H = -sum_v p log p,  p = softmax(x)
  d logp[r] / d x[r, v] = 1[v == t_r] - p[r, v]
  GRPO: rho = exp(logp - logp.detach()), kl = exp(ref - logp) - (ref - logp) - 1 (k3),
        use_grpo: loss = mean_g( sum_t (-(rho A - beta kl)) m / sum_t m );  clip: loss = sum (-min(rho A, clamp(rho, 1-el, 1+eh) A) + beta kl) m / sum m
  sampler: x / T, keep x >= (k-th largest x), softmax over the kept set, token = first index whose inclusive CDF reaches u (vocabulary order)

All logits are finite with |x| <= 64: a finite bf16 GEMM output is the kernels' contract; +-inf / NaN logits are out of scope (the online
(max, sum) update of the forward kernel is not defined for them).  A GRPO row with an all-zero mask divides by zero in the reference
trainer too and is left out.
"""
import math

import numpy as np
import torch

from oracle.sampler_filter import token_cdf  # noqa: F401  (the sampler's fp64 kept set and CDF; RefOps' filtered sampler draws from the same function)

BF16 = torch.bfloat16
I32 = torch.int32

# The project's own tolerances (atol, rtol), next to the quantity they already guard in tests/test_ops_gpu.py.
TOL_STATS = (1e-3, 1e-4)        # logp / entropy / lse
TOL_DLOGITS = (1e-3, 1e-2)      # bf16 gradient of the logits
TOL_GRPO = (1e-5, 1e-4)         # the four GRPO outputs
TOL_FUSED = (2e-3, 1e-4)        # lm_head with fused statistics vs the materialised HIP path
CDF_SLACK = 1e-4                # sampler: slack on the fp64 CDF interval of the drawn token
ORACLE_SHARE = 0.1              # the fp32 oracle must sit within this share of a tolerance, so a GPU miss cannot be the reference's rounding

LOGIT_LIMIT = 64.0


def worst(got, ref, tol):
    """(largest |got - ref| / (atol + rtol |ref|), largest |got - ref|) in fp64; a ratio <= 1 means `got` is within `tol` everywhere."""
    a, b = got.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0, 0.0
    assert torch.isfinite(a).all(), "non-finite values"
    err = (a - b).abs()
    return float((err / (tol[0] + tol[1] * b.abs())).max()), float(err.max())


def ceil8(n):
    return (n + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------------------------- rows (A, C)
ROW_KINDS = ("normal", "peak_hit", "peak_tail", "const", "two_level", "max_first", "max_last", "max_tail", "wide")   # 9 kinds: coprime with the 8 lanes


def stat_rows(R, V, seed, kind_offset=0, ld=None, col0=0):
    """-> (store bf16 [R, ld], view = store[:, col0:col0 + V], targets int32 [R], kinds).  Row r is of kind ROW_KINDS[(r + kind_offset) % 9]; a target
    that the kind does not pin sits in lane r % 8 of its 16-byte chunk.  Everything outside the view holds +64: a kernel that reads past V sees it."""
    ld = ceil8(V) if ld is None else ld
    assert ld % 8 == 0 and col0 % 8 == 0 and col0 + V <= ld
    g = torch.Generator().manual_seed(seed)
    store = torch.full((R, ld), LOGIT_LIMIT, dtype=torch.float32)
    x = torch.empty(R, V)
    tg = torch.empty(R, dtype=torch.int64)
    kinds = []
    tail_col = (V // 8) * 8 + (V % 8) // 2 if V % 8 else V - 3          # a column of the scalar tail where there is one
    for r in range(R):
        kind = ROW_KINDS[(r + kind_offset) % len(ROW_KINDS)]
        kinds.append(kind)
        lane = r % 8
        free = int(torch.randint(0, max(1, (V - lane + 7) // 8), (1,), generator=g)) * 8 + lane
        free = min(free, V - 1)
        row = (torch.randn(V, generator=g) * 2.5).clamp_(-12.0, 12.0)
        t = free
        if kind in ("peak_hit", "peak_tail"):
            j = int(torch.randint(0, V, (1,), generator=g))
            row[j] = 12.0 + 20.0 + 30.0 * float(torch.rand(1, generator=g))        # 20 .. 50 above everything else, <= 62
            t = j if kind == "peak_hit" else (free if free != j else (j + 1) % V)
        elif kind == "const":
            row[:] = 3.0
        elif kind == "two_level":
            row[:] = -60.0
            row[V - 1] = 60.0
            t = V - 1 if r % 2 == 0 else free % (V - 1) if V > 1 else 0
        elif kind == "max_first":
            row[0] = 30.0
            t = 0
        elif kind == "max_last":
            row[V - 1] = 30.0
            t = V - 1
        elif kind == "max_tail":
            row[tail_col] = 30.0
            t = tail_col
        elif kind == "wide":
            row = (torch.rand(V, generator=g) * 2 - 1) * 60.0
        x[r] = row
        tg[r] = t
    store[:, col0:col0 + V] = x
    store = store.to(BF16)
    return store, store[:, col0:col0 + V], tg.to(I32), kinds


STAT_V = (40, 1001, 2047, 2048, 5008, 151936, 152064)
STAT_ROWS = (1, 37, 64)


def stat_cases():
    """(id, builder kwargs) of every forward case: V x rows, plus one column slice in the middle of a wider tensor."""
    out = []
    for V in STAT_V:
        for R in STAT_ROWS:
            out.append(("V%d-R%d" % (V, R), dict(R=R, V=V, seed=1000 + V % 977 + R, kind_offset=(V + R) % 9 if R == 1 else 0)))
    out.append(("V5008-R37-ld5056-col16", dict(R=37, V=5008, seed=77, ld=5056, col0=16)))
    out.append(("V1001-R37-ld1024-col8", dict(R=37, V=1001, seed=78, ld=1024, col0=8)))
    return out


def bwd_cases():
    """Backward cases: the forward's V list without V % 8 != 0 (refused by the entry point), plus a column slice of a wider tensor (ld_out != ld)."""
    out = [c for c in stat_cases() if c[1]["V"] % 8 == 0]
    out.append(("V2048-R37-ld2112-col32", dict(R=37, V=2048, seed=79, ld=2112, col0=32)))
    return out


def bwd_dlogp(R, seed):
    """Upstream gradient of both signs; rows r % 5 == 3 are exactly 0."""
    g = torch.Generator().manual_seed(seed + 5)
    d = torch.randn(R, generator=g)
    d[torch.arange(R) % 5 == 3] = 0.0
    if R == 1:
        d[0] = -0.75
    return d


def _blocks(R, V):
    step = max(1, min(R, (1 << 24) // max(V, 1)))
    return [(a, min(R, a + step)) for a in range(0, R, step)]


def ref_stats(logits, targets):
    """fp64 (logp[target], entropy, lse) per row, in row blocks."""
    R, V = logits.shape
    outs = [torch.empty(R, dtype=torch.float64) for _ in range(3)]
    for a, b in _blocks(R, V):
        x = logits[a:b].double()
        lse = torch.logsumexp(x, -1)
        lp = x - lse[:, None]
        outs[0][a:b] = lp.gather(1, targets[a:b].long()[:, None])[:, 0]
        outs[1][a:b] = -(lp.exp() * lp).sum(-1)
        outs[2][a:b] = lse
    return tuple(outs)


def ref_dlogits(logits, targets, dlogp, lse=None):
    """fp64 dlogits = dlogp * (onehot(target) - softmax(logits)); `lse` (fp64) if already known."""
    x = logits.double()
    if lse is None:
        lse = torch.logsumexp(x, -1)
    p = torch.exp(x - lse.double()[:, None])
    p.neg_()
    p[torch.arange(x.shape[0]), targets.long()] += 1.0
    return p * dlogp.double()[:, None]


def sum_to_zero_bound(d64, dlogp):
    """Bound on |sum_v bf16(dlogits[r, v])| per row.  In exact arithmetic the sum is dlogp (1 - sum p) = 0.  Each stored element carries a
    round-to-nearest error of at most 2^-9 |d_v| (bf16 half-ulp, 8 significant bits); the V errors are independent, so their sum has a standard
    deviation of at most 2^-9 ||d_r||_2 (<= 2^-9 sqrt(2) |dlogp|, V enters through the norm); factor 6 covers the tail over every row tested.  The
    second term is the fp32 arithmetic in front of the rounding, which is common to all elements and does not average out: the LSE input
    rounded to fp32 (|lse| < 128: 2^-18 absolute), x - lse in fp32 (2^-18 for the elements that carry mass) and the fast exp (~2^-21
    relative) scale sum p by at most 1 + 2^-16; taken as |dlogp| 2^-15."""
    return 6.0 * 2.0 ** -9 * d64.norm(dim=1) + dlogp.double().abs() * 2.0 ** -15


# ---------------------------------------------------------------------------------------------------------------- lm_head (B)
def lmhead_tile_rows(M, N):
    """Replay of the integer cost model in tr1_lmhead_lse_fwd (csrc/gemm.hip): tile height in rows (224 / 256 / 288 / 320) the launcher picks."""
    def cost(bm, eff):
        t = ((M + bm - 1) // bm) * ((N + 255) // 256)
        return float((t + 255) // 256) * 256.0 * float(bm * 256) / eff
    eff = (0.94, 1.0, 1.025, 1.03)
    rt, best = 8, cost(256, 1.0)
    for r in range(7, 11):
        c = cost(r * 32, eff[r - 7])
        if c < best:
            best, rt = c, r
    return rt * 32


# (rows, V, K, tile height the launcher must pick).  If the launcher's rule changes, the replay assertion in the CPU test fails: re-pick shapes so
# that every tile height is still executed.
LMHEAD_SHAPES = ((224, 33024, 192, 224), (225, 33024, 192, 256), (256, 33024, 192, 256), (257, 33024, 192, 288), (288, 33024, 192, 288),
                 (289, 33024, 192, 320), (320, 33024, 192, 320), (321, 33024, 192, 224), (1137, 152064, 128, 288), (250, 151936, 128, 256))
LMHEAD_KINDS = ("normal", "peak_hit", "peak_tail", "const", "two_level", "normal", "peak_hit")


def lmhead_case(M, V, K, seed=11):
    """-> (hn bf16 [M, K], w bf16 [V, K], targets int32 [M], logits bf16 [M, V] = the bf16-rounded product, kinds).

    hn holds multiples of 1/16 in [-4, 4], w multiples of 1/32 in [-2, 2] (standard deviation 2.5 / sqrt(K)): every product is a multiple of 2^-9,
    every partial sum stays below 2^11, so fp32 accumulation is exact in ANY order and the bf16-rounded product is the same number on every
    correct implementation - the fp64 reference of that product is then the reference of the fused kernel, with no rounding flips in between.
    Column K-1 is reserved: w[:, K-1] = -60 (+60 for the last vocabulary row) and hn[:, K-1] = 1 only in the two-level rows.  A peaked row is
    hn[r] = 8 w[j] (logit 8 |w_j|^2 ~ 50 at j, N(0, 3.6) elsewhere), a constant row is hn[r] = 0."""
    g = torch.Generator().manual_seed(seed + M + V)
    hn = (torch.randn(M, K, generator=g) * 16).round().clamp_(-64, 64) / 16
    w = (torch.randn(V, K, generator=g) * (2.5 / math.sqrt(K - 1)) * 32).round().clamp_(-64, 64) / 32
    hn[:, K - 1] = 0.0
    w[:, K - 1] = -60.0
    w[V - 1, K - 1] = 60.0
    bm = lmhead_tile_rows(M, V)
    cols = [0, 63, 64, V - 64, V - 1, V - 100, 255, 256, V // 2 + 1]      # first / last column, slice and tile edges, the (ragged) last column tile
    tg = torch.empty(M, dtype=torch.int64)
    kinds = []
    for r in range(M):
        kind = LMHEAD_KINDS[r % len(LMHEAD_KINDS)]
        if bm < M and r in (bm - 1, bm):
            kind = "normal"                                               # last row of a tile / first row of the next: plain rows, distinct targets
        c = cols[r % len(cols)]
        t = c
        if kind in ("peak_hit", "peak_tail"):
            j = c
            hn[r] = 8.0 * w[j]
            hn[r, K - 1] = 0.0
            t = j if kind == "peak_hit" else cols[(r + 3) % len(cols)]
        elif kind == "const":
            hn[r] = 0.0
        elif kind == "two_level":
            hn[r] = 0.0
            hn[r, K - 1] = 1.0
            t = V - 1 if r % 2 == 0 else c % (V - 1)
        kinds.append(kind)
        tg[r] = t
    if bm < M:
        tg[bm - 1], tg[bm] = V - 1, 0
    hn, w = hn.to(BF16), w.to(BF16)
    logits = torch.empty(M, V, dtype=BF16)
    for a, b in _blocks(M, V):
        logits[a:b] = (hn[a:b].float() @ w.float().t()).to(BF16)          # exact in fp32 (see above), then one rounding
    return hn, w, tg.to(I32), logits, kinds


def lmhead_product_is_exact(hn, w, rows):
    """The fp32 product of the listed rows equals the fp64 product: the premise of lmhead_case."""
    a32 = hn[rows].float() @ w.float().t()
    a64 = hn[rows].double() @ w.double().t()
    return bool((a32.double() == a64).all())


# ---------------------------------------------------------------------------------------------------------------- GRPO (D)
GRPO_SHAPES = ((1, 1), (1, 7), (8, 200), (16, 1024), (64, 300), (3, 257))
GRPO_MAX_DIFF = 20.0        # |ref - logp| at live positions


def grpo_case(G, C, seed=0):
    """-> logp, ref_logp fp32 [G, C], mask int32 [G, C], adv fp32 [G].  Row 0 has length 1 (G > 1), row 1 (or the only row of a C > 1 grid) a mask
    with holes, the last row is full, the others are prefixes of random length 1 .. C; no row is empty.  Masked positions hold logp = -80,
    ref = -5: exp(75) is finite in fp32, and neither the loss nor dlogp may see it."""
    g = torch.Generator().manual_seed(seed + 131 * G + C)
    logp = -torch.rand(G, C, generator=g) * 3
    diff = (torch.rand(G, C, generator=g) * 2 - 1) * GRPO_MAX_DIFF
    mask = torch.zeros(G, C, dtype=torch.int64)
    for r in range(G):
        if G > 1 and r == 0:
            mask[r, 0] = 1
        elif (r == 1 or G == 1) and C > 1:
            m = (torch.rand(C, generator=g) < 0.6).long()
            m[int(torch.randint(0, C, (1,), generator=g))] = 1
            m[C // 2] = 0                                               # at least one hole, at least one live position
            m[0] = 1
            mask[r] = m
        elif r == G - 1:
            mask[r] = 1
        else:
            mask[r, : int(torch.randint(1, C + 1, (1,), generator=g))] = 1
    assert (mask.sum(1) >= 1).all()
    ref = logp + diff
    logp = torch.where(mask.bool(), logp, torch.full_like(logp, -80.0))
    ref = torch.where(mask.bool(), ref, torch.full_like(ref, -5.0))
    adv = torch.randn(G, generator=g)
    return logp, ref, mask.to(I32), adv


def ref_grpo(logp, ref_logp, mask, adv, beta, use_grpo, grad_scale, eps_low=0.2, eps_high=0.2):
    """fp64, the loss as the trainer writes it, differentiated by autograd: -> (dlogp = grad_scale * d loss / d logp, out3 = [loss, mean_g masked-mean
    kl, sum mask], row_len, row_kl = sum_t kl m)."""
    lp = logp.double().clone().requires_grad_(True)
    m = mask.double()
    A = adv.double()[:, None]
    kl = torch.zeros_like(lp)
    if ref_logp is not None:
        d = ref_logp.double() - lp
        kl = torch.exp(d) - d - 1
    rho = torch.exp(lp - lp.detach())
    if use_grpo:
        per_tok = rho * A
        per_tok = -(per_tok - beta * kl) if beta != 0.0 else -per_tok
        loss = ((per_tok * m).sum(1) / m.sum(1)).mean()
    else:
        per_tok = -torch.min(rho * A, torch.clamp(rho, 1 - eps_low, 1 + eps_high) * A)
        if beta != 0.0:
            per_tok = per_tok + beta * kl
        loss = (per_tok * m).sum() / m.sum()
    (grad,) = torch.autograd.grad(loss, lp)
    kl = kl.detach()
    lens = m.sum(1)
    klm = ((kl * m).sum(1) / lens).mean()
    return grad * grad_scale, torch.stack([loss.detach(), klm, m.sum()]), lens, (kl * m).sum(1)


# ---------------------------------------------------------------------------------------------------------------- sampler (E)
SAMP_FUSED_MAXV = 16 * 64 * 20 * 8      # 163840: above it the slice-sum and pick kernels run separately
V_FULL = 152064
V_UNFUSED = 163848
LOW = -60.0                             # background logit of the crafted rows: exp((-60 - 1) / T) is no mass at all next to the placed tokens


def _philox4x32_10(c, k0, k1):
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c = list(c)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def philox_u(seed, row, step):
    """The sampler's uniform: Philox4x32-10 with counter (row, step, 0, 0) and the 64-bit seed as key; the top 24 bits of the first word, centred, as the
    fp32 number the kernel forms (the 25-bit sum rounds to nearest even above 0.5)."""
    seed &= (1 << 64) - 1
    c = _philox4x32_10((row & 0xFFFFFFFF, step & 0xFFFFFFFF, 0, 0), seed & 0xFFFFFFFF, seed >> 32)
    return float(np.float32(float(c[0] >> 8) + 0.5) * np.float32(1.0 / 16777216.0))


def draw_error(keep, cdf, tok, u):
    """None if `tok` is a valid inverse-CDF answer for `u` (kept, and u inside its CDF interval with CDF_SLACK on both sides), else a description."""
    if not 0 <= tok < cdf.numel():
        return "token %d outside the vocabulary" % tok
    if not bool(keep[tok]):
        return "token %d is filtered out by top-k" % tok
    lo = float(cdf[tok - 1]) if tok > 0 else 0.0
    hi = float(cdf[tok])
    if not (lo - CDF_SLACK <= u <= hi + CDF_SLACK):
        return "u = %.9g outside the interval [%.9g, %.9g] of token %d" % (u, lo, hi, tok)
    return None


def sweep_rows(rows, V, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, V, generator=g) * 2.5).to(BF16)


SWEEP_CONFIGS = tuple((top_k, T) for top_k in (0, 50) for T in (0.7, 1.0))
SWEEP_ROWS, SWEEP_STEPS, SWEEP_SEEDS = 16, 8, tuple(4321 + 1009 * i + (i << 33) for i in range(16))      # 16 x 8 x 16 = 2048 draws per configuration


def _pair_row(V, a, b, xa, xb):
    row = torch.full((V,), LOW)
    row[a], row[b] = xa, xb
    return row


def fused_boundaries(V):
    """Token indices b such that (b - 1, b) straddle a boundary of the fused kernel's three-level search: wave segments of seg = ceil(V/8/16) chunks,
    64-chunk iterations inside a segment (the last one ragged), 8-logit chunks (lanes)."""
    nch = V // 8
    seg = (nch + 15) // 16
    nit = (seg + 63) // 64
    out = []
    for w in (1, 8, 15):
        out.append(("seg%d" % w, w * seg * 8))
    for w in (0, 7, 15):
        for j in sorted({1, nit - 2, nit - 1}):
            if j >= 1 and w * seg + j * 64 < min(nch, (w + 1) * seg):
                out.append(("seg%d-it%d" % (w, j), (w * seg + j * 64) * 8))
    for w in (0, 15):
        last_it0 = w * seg + (nit - 1) * 64
        out.append(("seg%d-lastit-lane" % w, (last_it0 + 5) * 8))                         # two lanes inside the ragged last iteration
        out.append(("seg%d-lastchunk" % w, (min(nch, (w + 1) * seg) - 1) * 8))            # the last chunk of the segment
        out.append(("seg%d-lane37" % w, (w * seg + 64 + 37) * 8))
    return out


def unfused_boundaries(V):
    """The same for the separate pick kernel: 32 slices of per = ceil(V/32) logits, 256 thread runs of tper = ceil(per/256) logits inside a slice."""
    per = (V + 31) // 32
    tper = (per + 255) // 256
    out = []
    for s in (1, 16, 31):
        out.append(("slice%d" % s, s * per))
    for s in (0, 31):
        for t in (1, 200):
            if s * per + t * tper < min(V, (s + 1) * per):
                out.append(("slice%d-run%d" % (s, t), s * per + t * tper))
    out.append(("last-run", V - 1))
    return out


def pair_case(V, bounds):
    """Rows with all mass on two tokens (b - 1, b) around each boundary, and once more inside one chunk / run (b + 3, b + 4), with the larger mass first
    and then second: the token is decided by u <= p alone (p = e / (1 + e) or 1 / (1 + e) at T = 1).  -> (logits bf16, [(name, a, b)])."""
    rows, meta = [], []
    for name, b in bounds:
        for a_, b_ in ((b - 1, b), (b + 3, b + 4)):
            if a_ < 0 or b_ >= V:
                continue
            for xa, xb in ((1.0, 0.0), (0.0, 1.0)):
                rows.append(_pair_row(V, a_, b_, xa, xb))
                meta.append(("%s@%d,%d:%g" % (name, a_, b_, xa), a_, b_))
    return torch.stack(rows).to(BF16), meta


def pair_expect(logits_row, a, b, temperature, u):
    """Token the pair row must give for u, or None when u is within CDF_SLACK of the split point."""
    za, zb = float(logits_row[a]) / temperature, float(logits_row[b]) / temperature
    p = 1.0 / (1.0 + math.exp(zb - za))
    if abs(u - p) <= CDF_SLACK:
        return None
    return a if u < p else b


def crafted_cases():
    """name -> dict(logits bf16 [rows, V], temperature, top_k, note).  Every draw is judged by draw_error(); `kept` (when present) is the exact size of
    the kept set per row, checked against token_cdf() on the CPU."""
    cases = {}
    V = V_FULL
    x = torch.full((4, V), LOW)
    x[:, 0] = 10.0
    cases["mass_at_first"] = dict(logits=x.to(BF16), temperature=1.0, top_k=0, only=0)
    x = torch.full((4, V), LOW)
    x[:, V - 1] = 10.0
    cases["mass_at_last"] = dict(logits=x.to(BF16), temperature=1.0, top_k=0, only=V - 1)
    x = torch.full((4, V), LOW)
    x[:, V - 1] = 10.0
    cases["mass_at_last_topk50"] = dict(logits=x.to(BF16), temperature=0.7, top_k=50, only=V - 1)      # everything ties at the 50th value: all kept

    # kept mass only in the last, ragged wave segment (V = 16392: 2049 chunks, segments of 129, the last one has 114)
    Vr = 16392
    g = torch.Generator().manual_seed(5)
    x = torch.full((8, Vr), LOW)
    x[:, 15 * 129 * 8:] = torch.randn(8, Vr - 15 * 129 * 8, generator=g) * 2.5
    cases["last_ragged_segment"] = dict(logits=x.to(BF16), temperature=1.0, top_k=0)
    cases["last_ragged_segment_topk"] = dict(logits=x.to(BF16), temperature=0.7, top_k=50)

    # ---- top-k
    g = torch.Generator().manual_seed(6)
    Vt = 40000
    x = (torch.randn(6, Vt, generator=g)).clamp_(-3.0, 3.0)
    pos = torch.randperm(Vt, generator=g)[:13]
    x[:, pos[:3]] = 5.0
    x[:, pos[3:]] = 4.0                                                   # 10 logits tie at the 5th largest value: 13 kept
    cases["topk_ties"] = dict(logits=x.to(BF16), temperature=1.0, top_k=5, kept=13)
    x = sweep_rows(4, 4096, seed=7).float()
    cases["topk_eq_V"] = dict(logits=x.to(BF16), temperature=0.9, top_k=4096, kept=4096)
    cases["topk_gt_V"] = dict(logits=x.to(BF16), temperature=0.9, top_k=5000, kept=4096)
    x = x.clone()
    x[:, 1234] = 20.0
    cases["topk_1"] = dict(logits=x.to(BF16), temperature=1.0, top_k=1, kept=1, only=1234)
    # the k-th value lies in a lower high-byte bin of the 16-bit key than the maximum: 40, 36, 33 have exponent 2^5, 31 .. 28 exponent 2^4
    x = sweep_rows(6, Vt, seed=8).float()
    pos = torch.randperm(Vt, generator=g)[:7]
    for p_, v in zip(pos, (40.0, 36.0, 33.0, 31.0, 30.0, 29.0, 28.0)):
        x[:, p_] = v
    cases["topk_across_bins"] = dict(logits=x.to(BF16), temperature=8.0, top_k=5, kept=5)
    # all logits negative: the order-preserving key inverts the bits of negative values
    x = -sweep_rows(6, Vt, seed=9).float().abs() - 1.0
    cases["topk_negative"] = dict(logits=x.to(BF16), temperature=1.0, top_k=50)
    # +0.0 is the k-th value, -0.0 everywhere else: a float comparison keeps both zeros (as HF's warper and the oracle do)
    x = torch.full((4, 4096), -0.0)
    x[:, [7, 900, 4095]] = 1.0
    x[:, [8, 2000]] = 0.0
    cases["topk_signed_zero"] = dict(logits=x.to(BF16), temperature=1.0, top_k=5, kept=4096)

    # ---- paths
    cases["unfused_large_V"] = dict(logits=sweep_rows(4, V_UNFUSED, seed=10), temperature=0.9, top_k=0)
    cases["unfused_large_V_topk"] = dict(logits=sweep_rows(4, V_UNFUSED, seed=10), temperature=0.9, top_k=50)
    cases["V_not_multiple_of_8"] = dict(logits=sweep_rows(6, 1001, seed=11), temperature=0.9, top_k=50)
    wide = sweep_rows(6, 4096 + 8, seed=12)      # ld % 8 == 0, base 6 bytes off a 16-byte boundary: `store` / `col0` let the GPU side rebuild the same view
    cases["unaligned_base"] = dict(logits=wide[:, 3:3 + 4096], store=wide, col0=3, temperature=0.9, top_k=50)
    return cases


CRAFTED_STEPS, CRAFTED_SEEDS = 4, (99, 5 + (7 << 40), 123456789, 2**63 + 11)      # 16 launches per case


STEP_CALLS = 20


def step_form_logits(call, rows=8, V=V_FULL, eos=3):
    """Logits of decode call `call`: fresh N(0, 2.5) rows; from call 5 on, row (call % rows) puts nearly all mass on the EOS token, so rows finish on the way."""
    x = sweep_rows(rows, V, seed=100 + call).float()
    if call >= 5:
        x[call % rows, eos] = 40.0
    return x.to(BF16)
