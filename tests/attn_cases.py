"""Attention cases shared by tests/test_attention_ref.py (CPU) and tests/test_attention_gpu.py (MI355X): seeded builders, fp64 references, derived
rounding bounds, mask mutants and an fp32 emulation of the kernels' rounding points.  Plain torch on the CPU; nothing here calls oracle/ref_ops.py.

The operation (csrc/attn_common.h): key kv is visible to query token t iff  kv < min(pre[t], n_slots)  or  lo[t] <= kv <= min(hi[t], n_slots - 1);
s = scale * q.k, lse = log sum exp s over the visible keys (-inf for a row that sees nothing), O = sum p v (0 for such a row), GQA by repetition of the kv head.

SCORES.  q and k are built so that every score family of the table below exists in every case; each tensor is rounded to bf16 ONCE and both sides get those
numbers.  16 features of a head are control features - C .. C + 15 with C = min(hd, 96) - 16, numbered from C below - and the others are free (randn, scaled
so that a free-feature score is about N(0, 1)).  The control features sit late in the head on purpose: a 60-nat term that enters an fp32 dot product first makes
every later addition round at ulp(60 / scale), and the fp32 oracle's LSE then spends 0.12 of its bound on summation order alone (measured with C = 0):
    0      ramp        k = (slot - n_slots / 2) / 64 (key tiles), q = the slope of the row in log2 units per tile
    1      bias        k = 1, q = a per-row shift of all scores
    2, 3   edge        k = 1 on the slots {pre - 1, pre} (feature 2) and {lo - 1, lo} (feature 3) of every distinct pre / lo of the case; the free features of
                       ALL these slots are EQUAL (those of slot 0), so that the two sides of an edge carry the same score for every row and a row's lift is
                       set by its own edge, not by another row's edge slot that it happens to see
    4      early       k = A on the first visible key of every early-spike row (and on the slot in front of it)
    8..15  late        one-hot codes of the last visible key j* of every late-spike row and of j* + 1: marked key number n (in slot order) has feature 8 + n % 8,
                       sign + / - for n % 16 < 8 / >= 8 and magnitude A 8^(n // 16); the row answers with the matching sign and B 8^-(n // 16) on the features of
                       j* and j* + 1.  Every visible marked key other than j* is older, so it gets -A B or at most A B / 8: j* stands 50 - 60 nats above the rest,
                       and the key just PAST the edge (j* + 1) is as hot as j*.
Families, per block of query tokens (block lengths FAMILY_BLOCKS, period 45: coprime with the 32-row waves, so waves mix families by themselves; the start of
the period is rotated per case):
    normal          randn
    ascending-slow  ramp of 3 log2 units per 64-key tile: the lazy running maximum (ATT_LAZY_MAX = 6) is kept on some tiles and replaced on others
    ascending-fast  ramp of 7 log2 units per tile: every tile rescales
    late-spike      see above
    early-spike     the first visible key 55 nats above the rest
    cold            all scores in [-64, -50]
    flat            q uses the bias feature only: K is constant as far as the row can tell, the softmax is uniform
    mixed-wave      tokens alternate between hot (free scores x 8) and cold
    edge-weighted   the edge features lift the keys at pre - 1 | pre and lo - 1 | lo to e^-1 of the row's weight (lse - 1, at most the row's maximum), and a ramp
                    of 5 log2 units per tile puts that maximum on hi | hi + 1.  (ascending, cold and hot rows get the same lift to lse - 4: without it a far
                    edge weighs e^-20 and no test of these rows could see a wrong pre / lo edge.)
V and dO are randn (dO is zero on every eleventh token); the cases marked `offset` give V mean 8 and variance 1 / 16 instead - V belongs to the keys, which every
family of rows shares, so it is a property of the case.
The builders keep |s| <= 64 nats on the visible keys (checked in test_attention_ref.py).

POISON.  Rows of K / V past n_slots (and the columns of V^T past it), up to the allocation, are NaN; in-range slots that no row sees hold +-1e4 in K and V,
except the slots next to an edge (lo - 1, hi + 1, pre of some row), which keep their scores.
"""
import functools
import math

import torch

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
U = 2.0 ** -8                  # bf16 unit roundoff (round to nearest: half an ulp of an 8-bit significand)
G128 = 2.0 ** -17              # fp32 accumulation of 128 terms: 128 * 2^-24
ATT_KV = 64
ATT_LAZY_MAX = 6.0
LOG2E = 1.4426950408889634
NCTRL = 16


def ctrl0(hd):
    """First of the 16 control features of a head: they end at feature min(hd, 96) (the live-96 launch keeps features 0..95)."""
    return min(hd, 96) - NCTRL
FAMILIES = ("normal", "ascending-slow", "ascending-fast", "late-spike", "early-spike", "cold", "flat", "mixed-wave", "edge-weighted")
FAMILY_BLOCKS = (8, 6, 6, 1, 1, 6, 6, 4, 7)        # tokens per family and period (45); the spike families are blind to some mutants by construction - kept short
DECODE_BLOCKS = (1, 1, 1, 1, 1, 1, 1, 2, 2)        # decode launches have 8 - 16 rows: period 11
MUTANTS = (("pre", -1), ("pre", 1), ("lo", -1), ("lo", 1), ("hi", -1), ("hi", 1))


# ---------------------------------------------------------------------------------------------------------------- masks
def masks_causal(T):
    t = torch.arange(T)
    return torch.zeros(T, dtype=torch.long), torch.zeros(T, dtype=torch.long), t, T


def masks_prefix_shared(P, G, C):
    """P prompt tokens, then G groups of C completion tokens; slot == token index."""
    pre = torch.cat([torch.zeros(P, dtype=torch.long), torch.full((G * C,), P)])
    lo = torch.cat([torch.zeros(P, dtype=torch.long), P + torch.arange(G).repeat_interleave(C) * C])
    return pre, lo, torch.arange(P + G * C), P + G * C


def masks_continuation(P, G, C):
    pre, lo, hi, S = masks_prefix_shared(P, G, C)
    return pre[P:], lo[P:], hi[P:], S


def masks_gap(P, G, C, stride):
    """The groups' key ranges start at P + g * stride and hold C live keys: whole tiles between the groups belong to nobody."""
    pre = torch.cat([torch.zeros(P, dtype=torch.long), torch.full((G * C,), P)])
    lo = torch.cat([torch.zeros(P, dtype=torch.long), P + torch.arange(G).repeat_interleave(C) * stride])
    hi = torch.cat([torch.arange(P), lo[P:] + torch.arange(C).repeat(G)])
    return pre, lo, hi, P + (G - 1) * stride + C


def masks_clamped(P, G, C):
    """prefix-shared with hi = n_slots + 5 on every fifth completion row and pre = n_slots + 9 on every seventh: both clamps of ATT_ROW_MASK / att_tile_range."""
    pre, lo, hi, S = masks_prefix_shared(P, G, C)
    r = torch.arange(S)
    hi = torch.where((r >= P) & (r % 5 == 0), torch.full_like(hi, S + 5), hi)
    pre = torch.where((r >= P) & (r % 7 == 3), torch.full_like(pre, S + 9), pre)
    return pre, lo, hi, S


def masks_segments(lengths):
    lo, hi, a = [], [], 0
    for n in lengths:
        lo += [a] * n
        hi += [a + n - 1] * n
        a += n
    return torch.zeros(a, dtype=torch.long), torch.tensor(lo), torch.tensor(hi), a


def masks_prefix_only(P, n, blind):
    """P causal prompt rows, n rows that see the prompt through `pre` only (every third with an EMPTY [lo, hi], the others with one key), then `blind`
    rows that see nothing at all (pre = 0, hi < lo)."""
    idx = P + torch.arange(n)
    pre = torch.cat([torch.zeros(P, dtype=torch.long), torch.full((n,), P), torch.zeros(blind, dtype=torch.long)])
    lo = torch.cat([torch.zeros(P, dtype=torch.long), idx, torch.full((blind,), 5)])
    hi = torch.cat([torch.arange(P), torch.where(torch.arange(n) % 3 == 0, idx - 1, idx), torch.full((blind,), 4)])
    return pre, lo, hi, P + n + blind


def masks_decode(P, G, cap, steps, S=None):
    """One decode step: row g sees the prompt [0, P) and its own suffix [P + g cap, P + g cap + steps[g]]; the rest of its region is not written yet."""
    g = torch.arange(G)
    lo = P + g * cap
    S = P + G * cap if S is None else S
    return torch.full((G,), P), lo, lo + torch.tensor(steps), S


def visible(pre, lo, hi, S):
    kv = torch.arange(S)[None]
    return (kv < pre.clamp(max=S)[:, None]) | ((kv >= lo[:, None]) & (kv <= hi.clamp(max=S - 1)[:, None]))


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    pass


def bf(x):
    return x.to(BF16)


def _families(T, blocks, rot):
    period = sum(blocks)
    table = torch.tensor([i for i, b in enumerate(blocks) for _ in range(b)])
    return table[(torch.arange(T) + rot) % period]


def build(name, hd, nh, nkv, masks, seed, v_kind="randn", blocks=FAMILY_BLOCKS, alloc_pad=13, rot=None):
    """-> Case with bf16 q [T, nh hd], k / v [S + alloc_pad, nkv hd] (poisoned), do [T, nh hd], int64 masks, fam [T], dead [S]."""
    pre, lo, hi, S = masks
    T = pre.numel()
    g = nh // nkv
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    scale = hd ** -0.5
    nfree = hd - NCTRL
    C = ctrl0(hd)                                               # first control feature
    fi = torch.tensor([d for d in range(hd) if not C <= d < C + NCTRL])
    amp = (hd / nfree) ** 0.25
    vis = visible(pre, lo, hi, S)
    seen = vis.any(0)
    fam = _families(T, blocks, seed % sum(blocks) if rot is None else rot)
    nonempty = hi.clamp(max=S - 1) >= lo
    has = vis.any(1)
    first = torch.where(has, vis.float().argmax(1), torch.zeros(T, dtype=torch.long))
    last = torch.where(has, S - 1 - vis.flip(1).float().argmax(1), torch.zeros(T, dtype=torch.long))

    # ---- K
    k = torch.zeros(S, nkv, hd, dtype=F64)
    k[:, :, fi] = rn(S, nkv, nfree) * amp
    slot = torch.arange(S)
    k[:, :, C] = ((slot - S // 2).double() / ATT_KV)[:, None]
    k[:, :, C + 1] = 1.0
    pre_edges = sorted({int(p) for p in pre.clamp(max=S).tolist() if 0 < p < S})
    lo_edges = sorted({int(l) for l, ne in zip(lo.tolist(), nonempty.tolist()) if ne and 0 < l < S})
    for e in sorted(set(pre_edges) | set(lo_edges)):
        k[e - 1, :, fi] = k[0, :, fi]                           # every edge slot, both sides: the SAME free features (those of slot 0) - only the ramp tells them apart
        k[e, :, fi] = k[0, :, fi]
    for e in pre_edges:
        k[e - 1:e + 1, :, C + 2] = 1.0
    for e in lo_edges:
        k[e - 1:e + 1, :, C + 3] = 1.0
    k[0, :, C + 3] = 1.0                                        # lo = 0 has no slot in front of it ...
    if bool((pre == 0).any()):
        k[0, :, C + 2] = 1.0                                    # ... and pre = 0 none behind it: slot 0 is the invisible side of that edge
    k[:, :, C + 3] = torch.where(k[:, :, C + 2] != 0, torch.zeros((), dtype=F64), k[:, :, C + 3])      # a slot on both kinds of edge: feature 2 only (one lift, not two)
    a_e = math.sqrt(55.0 / scale)
    is_early = (fam == 4) & has
    for f in sorted(set(first[is_early].tolist())):
        k[max(f - 1, 0):f + 1, :, C + 4] = a_e
    a_l = math.sqrt(60.0 / scale)
    is_late = (fam == 3) & has
    marked = sorted({j for j0 in last[is_late].tolist() for j in (j0, j0 + 1) if j < S})
    code = {}
    for n, j in enumerate(marked):
        sign = 1.0 if n % 16 < 8 else -1.0
        code[j] = (C + 8 + n % 8, sign, 8.0 ** (n // 16))
        k[j, :, C + 8 + n % 8] = sign * a_l * 8.0 ** (n // 16)
    k = bf(k.reshape(S, nkv * hd))

    # ---- Q
    q = torch.zeros(T, nh, hd, dtype=F64)
    free = rn(T, nh, nfree) * amp
    fscale = torch.tensor([1.0, 0.5, 0.5, 0.5, 0.5, 0.7, 0.0, 0.0, 0.5])[fam]
    hot = (fam == 7) & (torch.arange(T) % 2 == 0)
    fscale = torch.where(fam == 7, torch.where(hot, torch.tensor(8.0), torch.tensor(0.7)), fscale)
    q[:, :, fi] = free * fscale[:, None, None]
    q[:, :, C] = (torch.tensor([0, 3.0, 7.0, 0, 0, 0, 0, 0, 5.0])[fam] * math.log(2.0) / scale)[:, None]
    cold = (fam == 5) | ((fam == 7) & ~hot)
    q[:, :, C + 1] = torch.where(cold, torch.tensor(-57.0 / scale), torch.where(fam == 6, torch.tensor(1.0 / scale), torch.tensor(0.0))).double()[:, None]
    q[is_early, :, C + 4] = 55.0 / (scale * a_e)
    for t in torch.nonzero(is_late).flatten().tolist():
        for j in (int(last[t]), int(last[t]) + 1):
            if j in code:
                f, sign, mag = code[j]
                q[t, :, f] = sign * (60.0 / (scale * a_l)) / mag
    # edge lift: the edge keys to `below` nats under the row's maximum (never above it), one amount per edge feature and (token, head)
    below = torch.where(fam == 8, 1.0, 4.0)
    lifted = (fam == 8) | (fam == 1) | (fam == 2) | (fam == 5) | (fam == 7)
    rows = torch.arange(T)
    own = [torch.zeros(T, S, dtype=torch.bool), torch.zeros(T, S, dtype=torch.bool)]          # the invisible side of the row's own pre / lo edge
    sel = pre < S
    own[0][rows[sel], pre[sel]] = True
    sel = nonempty & (lo > 0)
    own[1][rows[sel], lo[sel] - 1] = True
    kh = k.double().view(S, nkv, hd).permute(1, 0, 2).repeat_interleave(g, 0)            # [nh, S, hd]
    score = lambda: scale * torch.einsum("thd,hsd->hts", bf(q).double(), kh)
    s0 = score().masked_fill(~vis[None], -math.inf)
    level = torch.minimum(s0.max(-1).values, torch.logsumexp(s0, -1) - below[None, :])     # [nh, T]: e^-below of the row's weight, and never above its maximum
    for f in (2, 3):
        s0 = score()                                                                       # (with the lift of feature 2 in place for feature 3)
        mk = (kh[0, :, C + f] != 0)[None, None, :] & (vis | own[f - 2])[None]
        room = (level[:, :, None] - s0).masked_fill(~mk, math.inf).min(-1).values
        room = torch.where(torch.isfinite(room), room.clamp(min=0.0), torch.zeros_like(room))
        q[:, :, C + f] = torch.where(lifted[:, None], room.t() / scale, torch.zeros_like(room.t()))
    q = bf(q.reshape(T, nh * hd))

    # ---- V, dO
    v = rn(S, nkv * hd)
    if v_kind == "offset":
        v = 8.0 + v / 4.0
    do = rn(T, nh * hd)
    do[torch.arange(T) % 11 == 5] = 0.0                       # dO == 0 rows: dQ == 0 exactly, nothing added to dK / dV
    # poison: the unseen slots, except those next to an edge (lo - 1, hi + 1, pre of some row) - these keep their scores: a key just past an edge must weigh
    guard = torch.zeros(S + 2, dtype=torch.bool)
    guard[(lo[nonempty] - 1).clamp(min=0)] = True
    guard[(hi.clamp(max=S - 1)[nonempty] + 1)] = True
    guard[pre.clamp(max=S)] = True
    poison = ~seen & ~guard[:S]
    sgn = lambda: torch.where(torch.rand(int(poison.sum()), nkv * hd, generator=gen) < 0.5, -1e4, 1e4).double()
    kk, vv = k.double(), v
    kk[poison] = sgn()
    vv[poison] = sgn()
    nan = torch.full((alloc_pad, nkv * hd), math.nan, dtype=F64)

    c = Case()
    c.name, c.hd, c.nh, c.nkv, c.group, c.T, c.S, c.scale, c.seed = name, hd, nh, nkv, g, T, S, scale, seed
    c.pre, c.lo, c.hi, c.fam, c.unseen, c.poison, c.vis = pre, lo, hi, fam, ~seen, poison, vis
    c.q, c.k, c.v, c.do = q, bf(torch.cat([kk, nan])), bf(torch.cat([vv, nan])), bf(do)
    return c


def zero_tail_features(c, keep=96):
    """The live-96 launch: features keep..hd of every head are zero in q / k / v (the control features all lie below 96: ctrl0)."""
    z = Case()
    z.__dict__.update(c.__dict__)
    m = (torch.arange(c.hd) < keep)
    cut = lambda t, n: torch.where(m[None, None, :], t.view(t.shape[0], n, c.hd), torch.zeros((), dtype=t.dtype)).reshape(t.shape[0], n * c.hd)
    z.q, z.k, z.v = cut(c.q, c.nh), cut(c.k, c.nkv), cut(c.v, c.nkv)
    z.name = c.name + "/live96"
    return z


def vt_of(c, pad=24):
    """V^T [n_kv hd, ld] as the kernels read it (ld a multiple of 8, > n_slots): NaN past n_slots."""
    ld = (c.S + 7) // 8 * 8 + pad
    vt = torch.full((c.nkv * c.hd, ld), math.nan, dtype=BF16)
    vt[:, :c.S] = c.v[:c.S].t()
    return vt


# name, head dim, n_heads, n_kv, masks, options.  Packed rows T * group: 64 / 65 / 255 / 256 / 257 are all here; groups 1, 2, 3, 6, 7.
_SPECS = [
    ("causal-1", 128, 2, 2, lambda: masks_causal(1), {}),
    ("causal-9", 32, 4, 4, lambda: masks_causal(9), {"rot": 0}),                              # (9 rows: one spike row would be 11 % of them, see MUTANTS)
    ("causal-64", 128, 2, 2, lambda: masks_causal(64), {}),                                   # 64 packed rows: QS == 1 in the backward
    ("causal-65", 80, 4, 4, lambda: masks_causal(65), {}),
    ("causal-200", 128, 4, 2, lambda: masks_causal(200), {}),
    ("rows255-g3", 64, 6, 2, lambda: masks_causal(85), {}),
    ("rows256-g2", 128, 4, 2, lambda: masks_causal(128), {}),
    ("rows257", 128, 2, 2, lambda: masks_causal(257), {}),
    ("tile-edges-63-33", 128, 12, 2, lambda: masks_prefix_shared(63, 3, 33), {}),
    ("tile-edges-64-32", 64, 6, 2, lambda: masks_prefix_shared(64, 3, 32), {}),
    ("tile-edges-65-31", 128, 7, 1, lambda: masks_prefix_shared(65, 3, 31), {}),
    ("tile-edges-128-64", 128, 14, 2, lambda: masks_prefix_shared(128, 3, 64), {}),
    ("lo-in-prefix-tile", 128, 4, 2, lambda: masks_prefix_shared(70, 3, 20), {}),
    ("gap", 128, 4, 2, lambda: masks_gap(64, 3, 20, 128), {}),
    ("gap-d64", 64, 6, 2, lambda: masks_gap(64, 3, 20, 128), {}),
    ("clamped", 128, 2, 2, lambda: masks_clamped(103, 2, 50), {}),                            # n_slots = 203: n_slots % 8 = 3
    ("clamped-d32", 32, 4, 4, lambda: masks_clamped(103, 2, 50), {}),
    ("segments", 80, 4, 4, lambda: masks_segments([1, 1, 63, 64, 65, 3, 130]), {}),
    ("segments-128", 128, 2, 2, lambda: masks_segments([1, 1, 63, 64, 65, 3, 130]), {}),
    ("prefix-only", 128, 4, 2, lambda: masks_prefix_only(90, 45, 6), {}),
    ("continuation", 128, 12, 2, lambda: masks_continuation(150, 3, 21), {}),
    ("long-causal", 128, 2, 2, lambda: masks_causal(448), {"v_kind": "offset"}),            # 7 key tiles
    ("long-prefix", 128, 4, 2, lambda: masks_prefix_shared(400, 3, 60), {}),                 # 6.25 prefix tiles + the groups: up to 9 tiles per row
    ("long-prefix-d64", 64, 6, 2, lambda: masks_prefix_shared(400, 2, 50), {"v_kind": "offset"}),
    # head dim 120 in the kernels padded to 128 (d_real < D): attn_fwd_kernel<128>, attn_bwd_dq_kernel<128>, attn_bwd_dkdv_kernel<128, 8> (128 keys per block)
    ("causal-33-d120", 120, 2, 2, lambda: masks_causal(33), {}),                              # 33 packed rows: QS == 1, the direct bf16 epilogue under d < d_real
    ("prefix-d120", 120, 4, 2, lambda: masks_prefix_shared(70, 3, 20), {}),                   # 260 packed rows, 130 slots: QS = 5, 2 keys in the second key block
]
CASE_NAMES = [s[0] for s in _SPECS]
# split-KV / decode launches: name, head dim, n_heads, n_kv, masks, options (rot: where the 11-token family period starts - every case has two edge-weighted rows)
_DECODE_SPECS = [
    ("dec-step0", 128, 28, 4, lambda: masks_decode(192, 8, 64, [0] * 8), {"rot": 5}),                                          # hi == lo on every row; 704 slots
    ("dec-p31", 128, 12, 2, lambda: masks_decode(31, 8, 32, [1, 31, 0, 5, 30, 31, 2, 17], S=320), {"rot": 9}),                # suffixes that end on a 32-key border
    ("dec-p32", 128, 12, 2, lambda: masks_decode(32, 8, 32, [31, 0, 31, 9, 1, 30, 31, 4], S=320), {"rot": 3}),
    ("dec-p33", 128, 28, 4, lambda: masks_decode(33, 8, 32, [30, 31, 0, 7, 31, 2, 29, 31], S=320), {"rot": 7}),
    ("dec-p64", 128, 12, 2, lambda: masks_decode(64, 16, 32, [(5 * i) % 32 for i in range(16)]), {"rot": 0}),
    ("dec-nopre", 128, 12, 2, lambda: masks_decode(0, 8, 64, [63, 0, 31, 32, 33, 1, 62, 40]), {"rot": 9}),                    # pre = 0
    ("dec-ragged", 128, 12, 2, lambda: masks_decode(70, 8, 40, [3, 39, 0, 17, 31, 8, 25, 12], S=397), {"rot": 3}),            # n_slots % 64 != 0: plan_mode 2 falls back
    ("dec-d64", 64, 6, 2, lambda: masks_decode(64, 8, 32, [31, 0, 31, 9, 1, 30, 31, 4]), {"rot": 9}),
    ("dec-d64-ragged", 64, 6, 2, lambda: masks_decode(33, 8, 40, [3, 39, 0, 17, 31, 8, 25, 12], S=357), {"rot": 5}),
]
DECODE_NAMES = [s[0] for s in _DECODE_SPECS]


@functools.lru_cache(maxsize=None)
def case(name):
    for i, (n, hd, nh, nkv, mk, opt) in enumerate(_SPECS):
        if n == name:
            return build(n, hd, nh, nkv, mk(), seed=100 + 7 * i, **opt)
    for i, (n, hd, nh, nkv, mk, opt) in enumerate(_DECODE_SPECS):
        if n == name:
            return build(n, hd, nh, nkv, mk(), seed=500 + 7 * i, blocks=DECODE_BLOCKS, alloc_pad=64, **opt)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- fp64 reference
def _heads(c):
    q = c.q.double().view(c.T, c.nh, c.hd).permute(1, 0, 2)                                   # [nh, T, hd]
    k = c.k[:c.S].double().view(c.S, c.nkv, c.hd).permute(1, 0, 2).repeat_interleave(c.group, 0)
    v = c.v[:c.S].double().view(c.S, c.nkv, c.hd).permute(1, 0, 2).repeat_interleave(c.group, 0)
    return q, k, v


def _flat(x):                                                                                  # [nh, T, hd] -> [T, nh hd]
    return x.permute(1, 0, 2).reshape(x.shape[1], -1)


class Fwd:
    pass


def ref_fwd(c, masks=None, bounds=True):
    """fp64 forward -> Fwd with O [T, nh hd], lse [nh, T] and the bounds tol_O / tol_lse (module docstring of test_attention_gpu.py for the derivation)."""
    pre, lo, hi = masks if masks is not None else (c.pre, c.lo, c.hi)
    vis = visible(pre, lo, hi, c.S)
    q, k, v = _heads(c)
    s = (c.scale * q @ k.transpose(1, 2)).masked_fill(~vis[None], -math.inf)
    lse = torch.logsumexp(s, -1)
    p = torch.nan_to_num(torch.exp(s - lse[..., None]), nan=0.0)
    r = Fwd()
    r.vis, r.s, r.p, r.lse = vis, s, p, lse
    r.O = _flat(p @ v)
    if bounds:
        live = ~c.poison
        r.tol_O = 1.05 * U * (_flat(p @ v.abs()) + r.O.abs()) + 2.0 ** -20 * float(c.v[:c.S][live].double().abs().max())
        a = (c.scale * q.abs() @ k.abs().transpose(1, 2)).masked_fill(~vis[None], 0.0).max(-1).values
        r.tol_lse = G128 * a + 2.0 ** -22 * torch.nan_to_num(lse.abs(), posinf=0.0) + 1e-5
    return r


@functools.lru_cache(maxsize=None)
def ref_fwd_of(name):
    return ref_fwd(case(name))


class Bwd:
    pass


def dk_from_bf16_p(c):
    """True where the dK kernel of an ordinary launch forms dS from the bf16-rounded P: attn_bwd_dkdv32_kernel, head dim exactly 128 (Q / dO within its
    32-bit DMA range; past it the launch takes attn_bwd_dkdv_kernel<128, 8>, and ref_bwd is told so)."""
    return c.hd == 128


def ref_bwd(c, o, lse, rope=None, dk_bf16_p=None):
    """fp64 flash backward OF THE INPUTS THE KERNEL IS GIVEN: bf16 q / k / v / O / dO and the fp32 lse (o: [T, nh hd], lse: [nh, T]; any dtype, used in fp64).
    -> Bwd with dQ [T, nh hd], dK / dV [S, n_kv hd] and their bounds.  rope = (cos, sin) [T, hd / 2]: dQ / dK times the transposed rotation.
    dk_bf16_p: whether dK forms dS from the bf16 P - a property of the ROUTE the launch takes (None: dk_from_bf16_p(c), an ordinary launch of the case)."""
    q, k, v = _heads(c)
    T, S, nh, nkv, g, hd = c.T, c.S, c.nh, c.nkv, c.group, c.hd
    do = c.do.double().view(T, nh, hd).permute(1, 0, 2)
    oh = o.double().view(T, nh, hd).permute(1, 0, 2)
    s = c.scale * q @ k.transpose(1, 2)
    p = torch.where(c.vis[None], torch.exp(s - lse.double()[..., None]), torch.zeros((), dtype=F64))
    p = torch.nan_to_num(p, nan=0.0, posinf=0.0)                                               # rows with lse = -inf see nothing
    delta = (do * oh).sum(-1)
    dp = do @ v.transpose(1, 2)
    ds = p * (dp - delta[..., None])
    grp = lambda x: x.view(nkv, g, S, hd).sum(1).permute(1, 0, 2).reshape(S, nkv * hd)         # [nh, S, hd] -> [S, n_kv hd]
    r = Bwd()
    r.dQ = _flat(c.scale * ds @ k)
    r.dK = grp(c.scale * ds.transpose(1, 2) @ q)
    r.dV = grp(p.transpose(1, 2) @ do)
    live = ~c.poison
    e = p * G128 * (do.abs() @ v.abs().transpose(1, 2) + (do * oh).abs().sum(-1)[..., None])
    mq, mk, mdo = float(c.q.double().abs().max()), float(c.k[:S][live].double().abs().max()), float(c.do.double().abs().max())
    r.tol_dQ = 1.05 * U * (_flat(c.scale * ds.abs() @ k.abs()) + r.dQ.abs()) + _flat(c.scale * e @ k.abs()) + 2.0 ** -20 * mk
    # head dim 128, dK only: attn_bwd_dkdv32_kernel hands P from its role-0 waves to its role-1 waves as the bf16 fragments of the dV product (the P exchange
    # buffer, make_p -> make_ds in csrc/attn_bwd.hip), so dS = bf16(bf16(P) (dP - delta)) = dS (1 + e1)(1 + e2), |e| <= u: the dS term counts twice.  The other
    # dK / dV kernels and every dQ kernel multiply the fp32 P.
    n_ds = 2.0 if (dk_from_bf16_p(c) if dk_bf16_p is None else dk_bf16_p) else 1.0
    r.tol_dK = (1.05 * U * (n_ds * grp(c.scale * ds.abs().transpose(1, 2) @ q.abs()) + r.dK.abs()) + grp(c.scale * e.transpose(1, 2) @ q.abs())
                + 2.0 ** -20 * mq)
    r.tol_dV = 1.05 * U * (grp(p.transpose(1, 2) @ do.abs()) + r.dV.abs()) + 2.0 ** -20 * mdo
    if rope is not None:
        # out = R^T g: out_a = g_a c + g_b s, out_b = g_b c - g_a s.  The error of g passes through the same linear map with absolute values, and the rotated
        # value is rounded to bf16 once more (the unfused form rounds g first: that rounding is already in g's bound; the fused form rounds only here)
        r.dQ, r.tol_dQ = _rope_bwd(r.dQ, r.tol_dQ, nh, hd, rope)
        r.dK, r.tol_dK = _rope_bwd(r.dK, r.tol_dK, nkv, hd, rope)
    return r


def _rope_bwd(x, tol, n, hd, rope):
    cos, sin = rope[0].double()[:, None, :], rope[1].double()[:, None, :]
    T, half = x.shape[0], hd // 2
    xa, xb = x.view(T, n, hd)[..., :half], x.view(T, n, hd)[..., half:]
    ta, tb = tol.view(T, n, hd)[..., :half], tol.view(T, n, hd)[..., half:]
    out = torch.cat([xa * cos + xb * sin, xb * cos - xa * sin], -1).reshape(T, n * hd)
    tout = torch.cat([ta * cos.abs() + tb * sin.abs(), tb * cos.abs() + ta * sin.abs()], -1).reshape(T, n * hd)
    return out, tout + 1.05 * U * out.abs()


def rope_tables(T, hd, seed=9):
    ang = torch.rand(T, hd // 2, generator=torch.Generator().manual_seed(seed)) * 6.28
    return bf(torch.cos(ang)).float(), bf(torch.sin(ang)).float()


def share(got, ref, tol):
    """-> (largest |got - ref| / tol, largest |got - ref|) over the finite reference entries; non-finite entries must agree exactly."""
    got, ref = got.double().cpu(), ref.double()
    fin = torch.isfinite(ref)
    assert torch.equal(got[~fin], ref[~fin]), "non-finite entries differ"
    if not bool(fin.any()):
        return 0.0, 0.0
    err = (got[fin] - ref[fin]).abs()
    assert not bool(torch.isnan(err).any()), "NaN in the result"
    return float((err / tol.double().expand_as(ref)[fin]).max()), float(err.max())


# ---------------------------------------------------------------------------------------------------------------- mutants
def mutate(c, which, d):
    m = {"pre": c.pre, "lo": c.lo, "hi": c.hi}
    m[which] = m[which] + d
    return m["pre"], m["lo"], m["hi"]


def mutant_catch(c, ref, which, d, use_lse=True, rows=None):
    """-> (rows whose visible set the mutant changes, how many of them the bounds catch): a (head, token) row is caught when its LSE (use_lse) or some
    element of its O is off by at least 2 x the bound.  rows: bool [T], restricts the count to these tokens."""
    mut = ref_fwd(c, mutate(c, which, d), bounds=False)
    changed = (mut.vis != ref.vis).any(1)
    if rows is not None:
        changed = changed & rows
    dO = ((mut.O - ref.O).abs() / ref.tol_O).view(c.T, c.nh, c.hd).max(-1).values.t()        # [nh, T]
    caught = dO >= 2.0
    if use_lse:
        dl = torch.nan_to_num((mut.lse - ref.lse).abs(), nan=0.0, posinf=math.inf) / ref.tol_lse
        caught = caught | (dl >= 2.0)
    return int(changed.sum()) * c.nh, int(caught[:, changed].sum())


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation of the rounding points
def tile_range(max_pre, min_lo, max_hi, S):
    """att_tile_range (csrc/attn_common.h): the 64-key tiles [0, pre_tiles) U [start2, end2] -> list of tile ids."""
    max_pre, max_hi = min(max_pre, S), min(max_hi, S - 1)
    pre_tiles = (max_pre + ATT_KV - 1) // ATT_KV
    s2 = max(min_lo // ATT_KV, pre_tiles)
    e2 = max_hi // ATT_KV if max_hi >= 0 else -1
    return list(range(pre_tiles)) + (list(range(s2, e2 + 1)) if (max_hi >= min_lo and e2 >= s2) else [])


def emulate_fwd(c, lazy=ATT_LAZY_MAX):
    """attn_fwd32_kernel in fp32 on the CPU: blocks of 256 packed rows (row = token * group + head of the group), waves of 32 rows, the block's 64-key tiles from
    the masks of its rows, per wave the any / full decisions and the lazy running maximum (kept while no valid row of the wave would rise by more than `lazy`
    log2 units), P = exp2(s - m) rounded to bf16 for the second product, l summed from the unrounded P, O rounded to bf16 once.
    -> O bf16 [T, nh hd], lse fp32 [nh, T], stats (counts of wave x tile visits)."""
    T, S, g, hd = c.T, c.S, c.group, c.hd
    nR = T * g
    sl2 = torch.tensor(c.scale * LOG2E, dtype=F32)
    O = torch.zeros(T, c.nh, hd, dtype=F32)
    lse = torch.full((c.nh, T), -math.inf, dtype=F32)
    st = dict(kept=0, replaced=0, any_not_full=0, full=0, not_any=0)
    pre_c, hi_c = c.pre.clamp(max=S), c.hi.clamp(max=S - 1)
    for kvh in range(c.nkv):
        kf = c.k[:S, kvh * hd:(kvh + 1) * hd].float()
        vf = torch.nan_to_num(c.v[:S, kvh * hd:(kvh + 1) * hd].float())
        for b0 in range(0, nR, 256):
            R = torch.arange(b0, min(b0 + 256, nR))
            t, hq = R // g, R % g
            ne = c.hi[t] >= c.lo[t]
            tiles = tile_range(int(c.pre[t].max()), int(c.lo[t][ne].min()) if bool(ne.any()) else 2 ** 31 - 1, int(c.hi[t][ne].max()) if bool(ne.any()) else -1, S)
            qf = c.q.view(T, c.nh, hd)[t, kvh * g + hq].float()
            for w0 in range(0, R.numel(), 32):
                w = slice(w0, min(w0 + 32, R.numel()))
                tw = t[w]
                n = tw.numel()
                padded = n < 32                        # rows past nR compare NaN <= 6 in the kernel: the wave never keeps its maximum
                m = torch.full((n,), -math.inf, dtype=F32)
                l = torch.zeros(n, dtype=F32)
                acc = torch.zeros(n, hd, dtype=F32)
                for tile in tiles:
                    kv = torch.arange(tile * ATT_KV, min((tile + 1) * ATT_KV, S))
                    vz = (kv[None] < pre_c[tw][:, None]) | ((kv[None] >= c.lo[tw][:, None]) & (kv[None] <= hi_c[tw][:, None]))
                    if not bool(vz.any()):
                        st["not_any"] += 1
                        continue
                    st["full" if (bool(vz.all()) and kv.numel() == ATT_KV) else "any_not_full"] += 1
                    s = (qf[w] @ kf[kv].t()).masked_fill(~vz, -math.inf)
                    m_cand = torch.maximum(m, s.max(-1).values * sl2)
                    rise = m_cand - m                                          # inf / NaN for rows that have seen nothing yet: not <= lazy
                    keep = (not padded) and lazy > 0 and bool((rise <= lazy).all())
                    if keep and bool((rise > 0).any()):
                        st["kept"] += 1
                    if not keep and bool(torch.isfinite(m).all()) and bool((rise > 0).any()):
                        st["replaced"] += 1
                    m_new = m if keep else m_cand
                    m_safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
                    alpha = torch.exp2(m - m_safe)
                    p = torch.exp2(s * sl2 - m_safe[:, None])
                    l = l * alpha + p.sum(-1)
                    acc = acc * alpha[:, None] + bf(p).float() @ vf[kv]
                    m = m_new
                inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
                O[tw, kvh * g + hq[w]] = acc * inv[:, None]
                lse[kvh * g + hq[w], tw] = torch.where(l > 0, (m + torch.log2(l)) * 0.6931471805599453, torch.full_like(l, -math.inf))
    return bf(O.reshape(T, c.nh * hd)), lse, st


def emulate_bwd(c, o, lse):
    """The backward kernels' rounding points in fp32 (dense; the kernels' tile order only changes the fp32 summation order): P = exp(s - lse) and
    dS = P (dP - delta) in fp32, BOTH rounded to bf16 before their MFMA (dV = P^T dO; dQ = scale dS K, dK = scale dS^T Q), outputs rounded to bf16 once;
    at head dim 128 the dS of the dK product is formed from the bf16 P (dk_from_bf16_p)."""
    T, S, nh, nkv, g, hd = c.T, c.S, c.nh, c.nkv, c.group, c.hd
    q, k, v = [x.float() for x in _heads(c)]
    k, v = torch.nan_to_num(k), torch.nan_to_num(v)
    do = c.do.float().view(T, nh, hd).permute(1, 0, 2)
    oh = o.float().view(T, nh, hd).permute(1, 0, 2)
    s = torch.tensor(c.scale, dtype=F32) * (q @ k.transpose(1, 2))
    p = torch.where(c.vis[None], torch.exp(s - lse.float()[..., None]), torch.zeros((), dtype=F32))
    p = torch.nan_to_num(p, nan=0.0, posinf=0.0)
    delta = (do * oh).sum(-1)
    dp = do @ v.transpose(1, 2)
    ds = p * (dp - delta[..., None])
    pb, dsb = bf(p).float(), bf(ds).float()
    dsk = bf(pb * (dp - delta[..., None])).float() if dk_from_bf16_p(c) else dsb           # attn_bwd_dkdv32_kernel: dS of the dK product from the bf16 P
    grp = lambda x: x.view(nkv, g, S, hd).sum(1).permute(1, 0, 2).reshape(S, nkv * hd)
    sc = torch.tensor(c.scale, dtype=F32)
    return bf(_flat(sc * (dsb @ k))), bf(grp(sc * (dsk.transpose(1, 2) @ q))), bf(grp(pb.transpose(1, 2) @ do))


# ---------------------------------------------------------------------------------------------------------------- replay of the backward launch
def replay_bwd(c):
    """dkdv_qsplit and the qmeta tile skipping of the dK / dV kernels (csrc/attn_bwd.hip) -> (QS, (query tile, key block) visits skipped, visits made)."""
    d_pad = (c.hd + 31) // 32 * 32
    kb = 192 if c.hd == 128 else 128 if d_pad in (64, 128) else 64       # by route: attn_bwd_dkdv32_kernel | the 8-wave attn_bwd_dkdv_kernel | its 4-wave form
    nR = c.T * c.group
    n_qtiles = (nR + 63) // 64
    kvblocks = ((c.S + kb - 1) // kb) * c.nkv
    qs = max(1, min(8, (1024 + kvblocks - 1) // kvblocks, n_qtiles))
    skipped = made = 0
    for qi in range(n_qtiles):
        t = torch.arange(qi * 64, min(qi * 64 + 64, nR)) // c.group
        ne = c.hi[t] >= c.lo[t]
        mp, ml = int(c.pre[t].max()), int(c.lo[t][ne].min()) if bool(ne.any()) else 2 ** 31 - 1
        mh = int(c.hi[t][ne].max()) if bool(ne.any()) else -1
        for kvb0 in range(0, c.S, kb):
            if (kvb0 < mp) or (kvb0 + kb - 1 >= ml and kvb0 <= mh):
                made += 1
            else:
                skipped += 1
    return qs, skipped, made


def unfrag(of, rows, nh, hd=128):
    """Fragment-major decode output -> [rows, nh hd]: element (m, k) at ((m // 16) * (nh * 4) + k // 32) * 512 + (m % 16) * 32 + k % 32."""
    m = torch.arange(rows)[:, None]
    k = torch.arange(nh * hd)[None, :]
    return of[((m // 16) * (nh * 4) + k // 32) * 512 + (m % 16) * 32 + k % 32]
