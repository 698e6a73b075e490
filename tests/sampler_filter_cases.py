"""Cases for the sampler's top-p / min-p filters and the repetition penalty (csrc/sampler.hip).  The fp64 reference (ref_filter, ref_penalize, bitmap_tokens)
lives in oracle/sampler_filter.py, where RefOps' sampler, penalty and seen bitmap use it too, and is re-exported here.

Shared by tests/test_sampler_filter_ref.py (CPU: the reference against the transformers warpers, and the host plumbing) and
tests/test_sampler_filter_gpu.py (the HIP kernels against the reference).  Plain torch on the CPU, written from the rules:

  order            : repetition penalty, temperature, top-k, top-p, min-p (HF generate)
  K (top-k)        : x >= k-th largest x (ties kept; every token when top-k is off)
  top-p            : masses softmax(x / T) over K; a value class v is kept iff the mass of the tokens of K with x > v is < top_p
                     (equal logits stand or fall together; the row maximum always stays)
  min-p            : keep x iff exp((x - max) / T) >= min_p
  kept set         : K, top-p and min-p intersected; the draw is the inverse CDF over it in vocabulary order (vc.draw_error judges it)
  repetition penalty: seen token: x * penalty if x < 0 else x / penalty, fp32, then one rounding to bf16
"""
import torch

import vocab_cases as vc
from oracle.sampler_filter import ref_filter, bitmap_tokens, ref_penalize  # noqa: F401

BF16, I32 = vc.BF16, vc.I32

# (top_k, T, top_p, min_p) of the full-vocabulary sweep
SWEEP_CONFIGS = ((0, 1.0, 0.9, 0.0), (50, 0.7, 0.9, 0.0), (0, 1.0, 1.0, 0.05), (50, 1.0, 0.95, 0.02), (0, 0.7, 0.5, 0.0))
SWEEP_ROWS, SWEEP_STEPS, SWEEP_SEEDS, SWEEP_ROW_SEED = 16, 8, (4321, 5330 + (1 << 33), 6339 + (2 << 33)), 1


def sweep_refs(cfg, rows=SWEEP_ROWS, V=vc.V_FULL, seed=SWEEP_ROW_SEED):
    """-> (logits bf16 [rows, V], [(keep, cdf)] per row, [margin] per row) of one sweep configuration."""
    top_k, T, top_p, min_p = cfg
    logits = vc.sweep_rows(rows, V, seed=seed)
    refs = [ref_filter(logits[r], T, top_k, top_p, min_p) for r in range(rows)]
    return logits, [(k, c) for k, c, _ in refs], [m for _, _, m in refs]


def tie_free_rows(rows, V, seed):
    """fp32 N(0, 2.5) rows without two equal logits (checked), for the comparison with HF's sort-based warpers."""
    x = torch.randn(rows, V, generator=torch.Generator().manual_seed(seed)) * 2.5
    assert all(torch.unique(x[r]).numel() == V for r in range(rows))
    return x


# ---------------------------------------------------------------------------------------------------------------- crafted rows
def _row(V, placed):
    row = torch.full((V,), vc.LOW)
    for i, v in placed.items():
        row[i % V] = v
    return row


def crafted_filter_cases(V):
    """name -> dict(logits bf16 [1, V], temperature, top_k, top_p, min_p, kept = exact size of the kept set).  Background vc.LOW, a few placed tokens
    (positions spread over the row: first, last, middle, odd offsets).  Masses quoted at the case's temperature."""
    a, b, c, d, e = 0, V - 1, V // 2 + 3, V // 3, (2 * V) // 3 + 1
    cases = {}

    def add(name, placed, kept, T=1.0, top_k=0, top_p=1.0, min_p=0.0):
        cases[name] = dict(logits=_row(V, placed).to(BF16)[None], temperature=T, top_k=top_k, top_p=top_p, min_p=min_p, kept=kept)

    # logits 2, 1, 1: masses .576, .212, .212.  Above the class of 1: .576 -> kept iff top_p > .576, and then BOTH ones
    add("ties_p0.7_keeps_three", {a: 2.0, b: 1.0, c: 1.0}, 3, top_p=0.7)
    add("ties_p0.5_keeps_one", {a: 2.0, b: 1.0, c: 1.0}, 1, top_p=0.5)
    # all placed logits negative (keys of negative values are the inverted bits): -1, -2, -2, -3 -> masses .534, .197, .197, .072; above -3: .928
    add("negative_boundary", {a: -1.0, b: -2.0, c: -2.0, d: -3.0}, 3, top_p=0.9)
    add("negative_boundary_minp", {a: -1.0, b: -2.0, c: -2.0, d: -3.0}, 3, min_p=0.3)      # ratios 1, .368, .368, .135
    # +0.0 and -0.0 are one class: 1, +0, -0, -0 -> masses .475, .175 x 3; above the zeros: .475 < .6 -> all four; and min-p .3 <= .368 likewise
    add("signed_zero_boundary", {a: 1.0, b: 0.0, c: -0.0, d: -0.0}, 4, top_p=0.6)
    add("signed_zero_boundary_minp", {a: 1.0, b: -0.0, c: 0.0, d: -0.0}, 4, min_p=0.3)
    add("signed_zero_dropped", {a: 1.0, b: 0.0, c: -0.0, d: -0.0}, 1, top_p=0.4)
    # boundary key with low byte 0x00: 2.0 = bf16 0x4000, 1.0 = 0x3F80 (low byte 0x80) next to 0.5 = 0x3F00 (low byte 0x00)
    add("low_byte_00", {a: 2.0, b: 0.5, c: 0.25}, 2, top_p=0.8)                          # masses .724, .162, .126: above 0.25 lies .885 > .8
    # boundary key with low byte 0xff: bf16 0x3FFF = 1.9921875 under 0x4000 = 2.0, and 0x3FFE below
    add("low_byte_ff", {a: 2.0, b: 1.9921875, c: 1.984375}, 2, top_p=0.6)                # masses ~ 1/3 each: above the third .67 > .6
    # top-k boundary (5th value 28 = exponent 2^4) in a lower high-byte bin than the top-p boundary (33, exponent 2^5); T = 8
    add("topp_bin_above_topk_bin", {a: 40.0, b: 36.0, c: 33.0, d: 31.0, e: 30.0, 7: 29.0, 9: 28.0, 11: 27.0}, 3, T=8.0, top_k=7, top_p=0.6)
    # and the reverse: top-k cuts first (k = 2), top-p = .99 would keep four
    add("topk_cuts_before_topp", {a: 3.0, b: 2.5, c: 2.0, d: 1.5}, 2, top_k=2, top_p=0.99)
    # the extremes keep exactly the ties of the maximum
    add("top_p_1e-6", {a: 5.0, b: 5.0, c: 4.96875, d: 1.0}, 2, top_p=1e-6)
    add("min_p_1", {a: 5.0, b: 5.0, c: 4.96875, d: 1.0}, 2, min_p=1.0)
    add("min_p_1_signed_zero_max", {a: 0.0, b: -0.0, c: -0.0078125}, 2, min_p=1.0)
    return cases


# ---------------------------------------------------------------------------------------------------------------- repetition penalty
def seen_bitmap(rows, V, seen_lists):
    """int32 [rows, ceil(V / 32)]: bit (v & 31) of word v >> 5 of row r set for v in seen_lists[r]."""
    W = (V + 31) // 32
    bm = torch.zeros(rows, W, dtype=torch.int64)
    for r, toks in enumerate(seen_lists):
        for v in toks:
            bm[r, v >> 5] |= 1 << (v & 31)
    return torch.where(bm >= 2 ** 31, bm - 2 ** 32, bm).to(I32)


def penalty_seen_sets(V):
    """Five rows: empty, one token, token 0, token V - 1, all of one 32-bit word (plus a partial neighbour)."""
    return [[], [V // 2 + 5], [0], [V - 1], list(range(64, 96)) + [97, V - 2]]
