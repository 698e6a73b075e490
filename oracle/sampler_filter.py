"""ORACLE - TEST INFRASTRUCTURE ONLY.  The sampler's top-k / top-p / min-p kept set with its fp64 CDF, and the repetition penalty with its seen bitmap
(csrc/sampler.hip), in plain torch on the CPU and written from the rules.  RefOps.sample_tokens (at a non-default top_p / min_p), RefOps.penalize_logits and
RefOps.mark_seen are built from these; tests/vocab_cases.py and tests/sampler_filter_cases.py judge the HIP kernels by the same functions.

  order            : repetition penalty, temperature, top-k, top-p, min-p (HF generate)
  K (top-k)        : x >= k-th largest x (ties kept; every token when top-k is off)
  top-p            : masses softmax(x / T) over K; a value class v is kept iff the mass of the tokens of K with x > v is < top_p
                     (equal logits stand or fall together; the row maximum always stays)
  min-p            : keep x iff exp((x - max) / T) >= min_p
  kept set         : K, top-p and min-p intersected; the draw is the inverse CDF over it in vocabulary order
  repetition penalty: seen token: x * penalty if x < 0 else x / penalty, fp32, then one rounding to bf16
  seen bitmap      : int32 [rows, ceil(V / 32)], bit (v & 31) of word v >> 5 of row r set once token v was seen in row r
"""
import math

import torch


def token_cdf(row, temperature, top_k):
    """fp64 (keep mask, inclusive CDF over the kept set in vocabulary order) of one logits row.  Ties with the k-th largest value are kept (float
    comparison, so +0.0 and -0.0 tie)."""
    x = row.double()
    V = x.numel()
    if top_k and 0 < top_k < V:
        keep = x >= torch.topk(x, top_k).values[-1]
    else:
        keep = torch.ones(V, dtype=torch.bool)
    z = x / temperature
    p = torch.where(keep, (z - z.max()).exp(), torch.zeros_like(z))
    return keep, torch.cumsum(p, 0) / p.sum()


def ref_filter(row, temperature, top_k, top_p=1.0, min_p=0.0):
    """fp64 (keep mask, inclusive CDF over the kept set in vocabulary order, boundary margin) of one logits row.

    margin: how far the row is from a different kept set.  top-p: min over the value classes of K of |mass above the class - top_p| (masses as
    shares of K's mass); min-p: min over the tokens of |exp((x - max) / T) - min_p| / min_p.  inf for a filter that is off."""
    x = row.double()
    keep_k, _ = token_cdf(row, temperature, top_k)
    z = x / temperature
    e = torch.where(keep_k, (z - z.max()).exp(), torch.zeros_like(z))
    keep = keep_k.clone()
    margin = math.inf
    if top_p < 1.0:
        vals, inv = torch.unique(x, return_inverse=True)                  # ascending; float equality, so +0.0 and -0.0 are one class
        n = vals.numel()
        cls_mass = torch.zeros(n, dtype=torch.float64).scatter_add_(0, inv, e)
        cls_in_k = torch.zeros(n, dtype=torch.bool).scatter_(0, inv[keep_k], True)
        desc = cls_mass.flip(0)
        above = (torch.cumsum(desc, 0) - desc).flip(0) / e.sum()           # share of K's mass on strictly larger logits, per class
        keep &= (above < top_p)[inv]
        margin = min(margin, float((above[cls_in_k] - top_p).abs().min()))
    if min_p > 0.0:
        ratio = (z - z.max()).exp()
        keep &= ratio >= min_p
        margin = min(margin, float(((ratio - min_p).abs() / min_p).min()))
    assert bool(keep[int(x.argmax())]), "the row maximum is always kept"
    p = torch.where(keep, e, torch.zeros_like(e))
    return keep, torch.cumsum(p, 0) / p.sum(), margin


# ---------------------------------------------------------------------------------------------------------------- repetition penalty
def set_bit(seen, r, v):
    w = (int(seen[r, v >> 5]) & 0xFFFFFFFF) | (1 << (v & 31))
    seen[r, v >> 5] = w - (1 << 32) if w >= (1 << 31) else w


def bitmap_tokens(bm_row, V):
    """The set a bitmap row holds."""
    w = bm_row.to(torch.int64) & 0xFFFFFFFF
    bits = (w[:, None] >> torch.arange(32)[None, :]) & 1
    return set(torch.nonzero(bits.reshape(-1)[:V])[:, 0].tolist())


def ref_penalize(logits, seen_lists, penalty):
    """torch on the CPU: fp32 ops of RepetitionPenaltyLogitsProcessor on the seen tokens, then .to(bfloat16).  logits bf16 [rows, V]."""
    x = logits.float()
    out = x.clone()
    pen = torch.tensor(penalty, dtype=torch.float32)
    for r, toks in enumerate(seen_lists):
        if toks:
            idx = torch.tensor(sorted(toks), dtype=torch.long)
            s = x[r, idx]
            out[r, idx] = torch.where(s < 0, s * pen, s / pen)
    return out.to(torch.bfloat16)
