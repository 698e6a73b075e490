"""sha256 of every output of the decode-row GEMM family (csrc/gemm_skinny.hip, csrc/gemm_w8.hip) and of the native decode step on fixed seeded inputs: run under two
builds (TR1_HIP_LIB=tools/_var_ref.so from tools/build_ref_lib.sh, then the product build) and diff the lines to show that an edit of these kernels left every
bit where it was - they are deterministic, the split-K fixup included.    python tools/hash_decode_gemm.py > out.txt"""
import hashlib, math, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import time_r1_amd  # noqa
from time_r1_amd.ops import HipOps
ops = HipOps("cuda:0")
BF16 = torch.bfloat16
h = lambda t: hashlib.sha256(t.contiguous().view({BF16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[t.dtype]).cpu().numpy().tobytes()).hexdigest()[:16]
def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF16).cuda()
lnw_of = lambda K: (1.0 + 0.1 * rnd(K, seed=2).float()).to(BF16)

# ---- gemm_nt at decode rows (launch_skinny), bias + residual, bf16 and fp32 output.  (16, 3584, 18944) is the long-K 8-wave form; (16, 512, 2048) and (7, 200, 1024)
# take the XLDS form (x through LDS: <= 16 rows, one column group, 1024 <= K <= 3840)
for M, N, K in [(8, 512, 256), (16, 4608, 3584), (16, 100032, 256), (5, 72, 320), (32, 4608, 3584), (64, 512, 3584), (16, 3584, 18944), (16, 512, 2048), (7, 200, 1024)]:
    a, b, bias, res = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1.0 / math.sqrt(K)), rnd(N, seed=3), rnd(M, N, seed=4)
    print("gemm_nt", M, N, K, "bf16", h(ops.gemm_nt(a, b, bias=bias, residual=res)), "f32", h(ops.gemm_nt(a, b, bias=bias, residual=res, out_f32=True)))

# ---- split-K + fixup: three launches on one workspace, fresh activations each
for M, N, K in [(16, 3584, 18944), (32, 3584, 18944), (8, 1536, 8960), (5, 200, 2048), (24, 1536, 1536), (64, 512, 4096), (3, 128, 18944), (1, 64, 8192), (5, 448, 8192),
                (20, 448, 8192)]:
    b, bias, res = rnd(N, K, seed=2, scale=1.0 / math.sqrt(K)), rnd(N, seed=3), rnd(M, N, seed=4)
    print("gemm_skinny_fixup", M, N, K, *[h(ops.gemm_skinny_fixup(rnd(M, K, seed=100 + rep), b, bias=bias, residual=res)) for rep in range(3)])

# ---- rmsnorm folded in: plain / SwiGLU / fragment-major SwiGLU (the cases of tests/test_ops_gpu.py::test_norm_gemm_fused + one glu = 2)
NORM_GEMM = [(8, 512, 256, False), (16, 4608, 3584, False), (16, 100032, 256, False), (32, 100096, 320, False), (5, 72, 320, False), (16, 1024, 3584, True), (13, 200, 512, True),
             (32, 4608, 3584, False), (24, 1024, 1536, True), (64, 512, 3584, False), (40, 136, 832, True),
             (5, 18944, 3584, True), (1, 48, 3584, True), (16, 8960, 1536, True), (9, 4112, 1536, True), (16, 11008, 2048, True),
             (32, 18944, 3584, True), (17, 4112, 3584, True), (20, 11008, 2048, True), (29, 48, 1536, True),
             (16, 152064, 3584, False), (7, 151936, 1536, False), (1, 65536, 2048, False), (32, 152064, 3584, False), (19, 65536, 1536, False), (16, 1024, 3584, 2)]
for M, N, K, glu in NORM_GEMM:
    x, w = rnd(M, K, seed=1, scale=2.0), rnd(2 * N if glu else N, K, seed=3, scale=1.5 / math.sqrt(K) if glu else 0.1)
    print("norm_gemm", M, N, K, "glu=%d" % int(glu), h(ops.norm_gemm(x, lnw_of(K), 1e-6, w, bias=None if glu else rnd(N, seed=4), glu=glu)))

# ---- fused rmsnorm + q/k/v + M-RoPE + cache append (the cases of test_norm_gemm_qkv_fused): q, K cache, V^T cache
# + two XLDS cases of norm_gemm_skinny_kernel (<= 16 rows, 1024 <= K <= 3840, K / 512 not in {7, 4, 3})
for R, nh, nkv, hd, K in [(16, 28, 4, 128, 3584), (8, 4, 2, 32, 128), (32, 12, 2, 128, 1536), (5, 4, 1, 64, 256), (64, 4, 2, 32, 128), (8, 4, 2, 32, 1024), (13, 4, 1, 64, 2560)]:
    N, S = (nh + 2 * nkv) * hd, 96
    x, w, b = rnd(R, K, seed=1, scale=2.0), rnd(N, K, seed=3, scale=1.0 / math.sqrt(K)), rnd(N, seed=4)
    pos = torch.randint(0, 500, (3, R), generator=torch.Generator().manual_seed(5)).int().cuda()
    cos, sin = ops.mrope_table(pos, hd, {128: (16, 24, 24), 64: (8, 12, 12), 32: (4, 6, 6)}[hd], 1e6)
    slots = torch.randperm(S, generator=torch.Generator().manual_seed(6))[:R].int().cuda()
    kc, vt = rnd(S, nkv * hd, seed=7), rnd(nkv * hd, S, seed=8)
    q = ops.norm_gemm_qkv(x, lnw_of(K), 1e-6, w, b, cos, sin, kc, vt, slots, nh, nkv, hd)
    print("norm_gemm_qkv", R, nh, nkv, hd, K, "q", h(q), "K", h(kc), "Vt", h(vt))

# ---- fp8 weights, W8A16 and W8A8 (the cases of test_gemm_w8 + the two small split-K + fixup shapes)
W8 = [(16, 4608, 3584, "norm"), (8, 512, 256, "plain"), (16, 3584, 18944, "res"), (16, 1024, 3584, "glu"), (32, 4608, 3584, "norm"), (24, 512, 1536, "glu"), (64, 512, 3584, "res"),
      (5, 72, 384, "plain"), (40, 136, 1024, "glu"), (16, 152064, 3584, "norm"), (16, 18944, 3584, "glu"), (5, 18944, 3584, "glu"), (7, 3584, 18944, "res"), (16, 8960, 1536, "glu"),
      (9, 4112, 1536, "glu"), (16, 11008, 2048, "glu"), (1, 48, 3584, "glu"), (3, 128, 8192, "res"), (5, 448, 8192, "res")]
for M, N, K, mode in W8:
    glu = mode == "glu"
    x = rnd(M, K, seed=1, scale=2.0 if mode in ("norm", "glu") else 1.0)
    q, sc = ops.quantize_fp8_rows(rnd(2 * N if glu else N, K, seed=3, scale=1.5 / math.sqrt(K) if glu else 0.1))
    lnw = lnw_of(K) if mode in ("norm", "glu") else None
    bias, res = rnd(N, seed=4) if mode in ("norm", "plain") else None, rnd(M, N, seed=5) if mode == "res" else None
    print("gemm_w8", M, N, K, mode, *["a8=%d %s" % (a8, h(ops.gemm_w8(x, q, sc, lnw=lnw, eps=1e-6, bias=bias, residual=res, glu=glu, a8=bool(a8)))) for a8 in (0, 1)])

# ---- one native rollout on the smallest configuration of tests/test_engine_gpu.py::test_native_decode_step_equals_op_by_op: the logits of every decode_step
from time_r1_amd.config import tiny_test
from time_r1_amd.params import ModelParams
from time_r1_amd.model import Engine
from time_r1_amd.grpo import GRPOCore
from time_r1_amd.synthetic import synthetic_prompt
cfg = tiny_test(n_layers=3)
cfg.text.intermediate = 256
eng = Engine(cfg, ops, ModelParams(cfg, ops, seed=1))
step = ops.decode_step
for wdtype in ("bf16", "fp8", "fp8-mfma"):
    sha, n = hashlib.sha256(), [0]
    def spy(*a, **k):
        out = step(*a, **k)
        sha.update(out.contiguous().view(torch.int16).cpu().numpy().tobytes()); n[0] += 1
        return out
    ops.decode_step = spy
    core = GRPOCore(eng, None, 8, 10, beta=0.0, seed=5, rope_index_mode="hf4")
    core.roll.native_decode = True
    if wdtype != "bf16":
        core.roll.weight_dtype = wdtype
    ids, pix, grid = synthetic_prompt(cfg, (4, 6, 8), 9, 7, seed=2, text_vocab=400)
    toks = core.rollout_many([core.prepare(ids, pix, grid)])
    ops.decode_step = step
    print("decode_step", wdtype, "steps", n[0], "logits", sha.hexdigest()[:16], "tokens", h(torch.stack([t.cpu() for t in toks]).int().float()))
