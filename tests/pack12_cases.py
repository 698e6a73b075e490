"""Weights for the packed 12-bit gate/up format (time_r1_amd.torch_ops.pack_bf16_glu_ref / csrc/gemm_pk.hip), shared by the CPU and the GPU tests.

A stage is 16 gate + 16 up rows of a column-group pair x 64 k; stage_slice() addresses one in the [2I, K] weight."""
import torch

BF16 = torch.bfloat16
P = 14          # patch capacity of a stage
TINY = 2.0 ** -60


def stage_slice(I, K, pair, wave, s):
    """-> (gate rows, up rows, columns) of stage (pair, wave, s)."""
    k0 = wave * (K // 8) + s * 64
    return slice(pair * 16, pair * 16 + 16), slice(I + pair * 16, I + pair * 16 + 16), slice(k0, k0 + 64)


def bits(vals):
    return torch.tensor(vals, dtype=torch.int32).to(torch.int16).view(BF16)


def distributions(I, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(2 * I, K, generator=g) * 0.02
    u = (torch.rand(2 * I, K, generator=g) * 2 - 1) * 0.03
    t = torch.distributions.StudentT(3.0).sample((2 * I, K)) * 0.01
    den = bits(torch.randint(0, 128, (2 * I * K,), generator=g).tolist()).view(2 * I, K).clone()      # denormals (exponent 0) and +0.0
    den[::2] = -den[::2]
    return {"normal": n.to(BF16), "uniform": u.to(BF16), "student_t": t.to(BF16), "zero": torch.zeros(2 * I, K, dtype=BF16), "denormal": den}


def fill_stage(w, I, K, where, kind):
    """Overwrite stage `where` = (pair, wave, s) of w in place with an adversarial pattern; -> patches the stage needs."""
    gr, ur, cs = stage_slice(I, K, *where)
    big = torch.finfo(BF16).max
    blk = torch.full((32, 64), big, dtype=BF16)
    blk[1::2] = -big
    if kind == "max_one_tiny":                      # +-max everywhere, one tiny value: a patch
        blk[5, 7] = TINY
        n = 1
    elif kind in ("exactly_P", "P_plus_1"):         # values 16 binades under the stage maximum and below: P (P + 1) patches
        n = P if kind == "exactly_P" else P + 1
        blk = torch.full((32, 64), 1.0, dtype=BF16)
        for i in range(n):
            blk[(i * 7) % 32, (i * 11) % 64] = TINY * (i + 1)
    elif kind == "inf_nan":                         # +-Inf and NaN payloads next to ordinary weights: patches, payload kept
        blk = torch.full((32, 64), 0.01, dtype=BF16)
        sp = bits([0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F81, 0x7FFF, 0xFFFF])
        for i in range(7):
            blk[i * 4, i * 9] = sp[i]
        n = 7
    elif kind == "neg_zero":                        # -0.0 and +0.0 under ordinary weights: patches that keep the sign
        blk = torch.full((32, 64), -0.02, dtype=BF16)
        blk[3, 3] = -0.0
        blk[31, 63] = 0.0
        n = 2
    elif kind == "inf_window":                      # Inf / NaN inside the window of a +-max stage: no patch at all
        blk[0, 0] = float("inf")
        blk[31, 63] = bits([0xFFC1])[0]
        n = 0
    else:
        raise ValueError(kind)
    w[gr, cs] = blk[:16]
    w[ur, cs] = blk[16:]
    return n


ADVERSARIAL = ("max_one_tiny", "exactly_P", "inf_nan", "neg_zero", "inf_window")


def same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))
