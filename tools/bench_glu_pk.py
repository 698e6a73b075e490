"""Go / no-go of the packed 12-bit gate/up decode kernel (csrc/gemm_pk.hip) against the bf16 kernel at the 7B shape: M rows x I 18944 x K 3584.
Both kernels in one process, alternating, each launch on another of NC weight copies so that nothing is served from the 256 MB Infinity Cache.
Checks first that the packer writes what the torch reference writes (a slice) and that the twin stores the bf16 kernel's bits.
   python tools/bench_glu_pk.py [M] [REPS]"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import time_r1_amd  # noqa
import time_r1_amd.torch_ops as T
from time_r1_amd.ops import HipOps
ops = HipOps("cuda:0")
M = int(sys.argv[1]) if len(sys.argv) > 1 else 16
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
K, I, NC, N = 3584, 18944, 6, 60
torch.manual_seed(0)
x = torch.randn(M, K, device="cuda").bfloat16()
lnw = (1 + 0.1 * torch.randn(K, device="cuda")).bfloat16()
ws = [(torch.randn(2 * I, K, device="cuda") * 0.02).bfloat16() for _ in range(NC)]
pk = [ops.pack_bf16_glu(w) for w in ws]
assert all(int(ops.pack_flag(p).item()) == 0 for p in pk), "not representable"
small = torch.cat([ws[0][:64], ws[0][I:I + 64]])
rec, tails, ok = T.pack_bf16_glu_ref(small)
got, n = ops.pack_bf16_glu(small.contiguous()), rec.shape[0]
print("packer == torch reference (64-column slice): records %s tails %s" % (torch.equal(got[:n * 3072].view(n, 3072), rec),
                                                                            torch.equal(got[n * 3072:-16].view(torch.int32).view(n, 16), tails)))
ref = ops.norm_gemm(x, lnw, 1e-6, ws[0], glu=True)
out = ops.norm_gemm_glu_pk(x, lnw, 1e-6, pk[0], I)
print("twin == bf16 kernel bit for bit: %s" % torch.equal(ref.view(torch.int16), out.view(torch.int16)))
i = [0]
def run_bf():
    i[0] = (i[0] + 1) % NC
    return ops.norm_gemm(x, lnw, 1e-6, ws[i[0]], glu=True)
def run_pk():
    i[0] = (i[0] + 1) % NC
    return ops.norm_gemm_glu_pk(x, lnw, 1e-6, pk[i[0]], I)
def timed(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n
for f in (run_bf, run_pk): timed(f, 20)
tb, tp = [], []
for _ in range(REPS):
    tb.append(timed(run_bf, N)); tp.append(timed(run_pk, N))
med = lambda v: sorted(v)[len(v) // 2]
print("M=%d  bf16 us: %s" % (M, " ".join("%.1f" % t for t in tb)))
print("M=%d  pk   us: %s" % (M, " ".join("%.1f" % t for t in tp)))
spread = max(tb) - min(tb)
print("median bf16 %.1f us (%.0f GB/s), median pk %.1f us (%.0f GB/s of packed bytes); gain %.1f us, bf16 spread %.2f us -> %s" % (
    med(tb), 2 * I * K * 2 / med(tb) / 1e3, med(tp), 2 * I * K * 2 * 0.766 / med(tp) / 1e3, med(tb) - med(tp), spread,
    "GO" if med(tb) - med(tp) > 3 * spread else "NO-GO"))
print("packer: %.0f us per [2 x %d, %d] matrix" % (timed(lambda: ops.pack_bf16_glu(ws[0], pk[0]), 10), I, K))
