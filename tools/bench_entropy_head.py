"""tr1_logp_entropy_bwd beside tr1_logp_bwd, and tr1_entropy_quantile_weight: microseconds per launch on the MI355X.

    python tools/bench_entropy_head.py                 # one JSON line + the table of BASELINE.md section 4h
    python tools/bench_entropy_head.py --launches 200 --warmup 10

Vocabulary-side backward at the head of config 3 (R = 1600 = 8 x 200 rows, V = 152064) and at one chunk of config 4 (R = 4096): both kernels read and write the
same R x V bf16, in place as the engine runs them, so tr1_logp_bwd IN THE SAME RUN is the yardstick of the new kernel and the spread tr1_logp_bwd shows over its own
launches is the margin.  The two alternate launch by launch; before every launch the logits are restored from a pristine copy (outside the timed pair of device
events), so each launch sees real logits and the same cache state.  Reported per kernel: median, min, p05, p95, max over `--launches` launches, achieved GB/s over
the 2 x R x V x 2 bytes the pass must move, and the ratio of the medians.

The selection kernel at (G, C) = (8, 200) and (16, 1024): uniform entropies, ragged prefix masks, rho = 0.2; one device-event pair per launch.  No gate hangs on it."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
I32 = torch.int32


def _stats(us):
    s = sorted(us)
    n = len(s)
    q = lambda f: s[min(n - 1, int(f * (n - 1) + 0.5))]
    return {"us_median": round(q(0.5), 2), "us_min": round(s[0], 2), "us_p05": round(q(0.05), 2), "us_p95": round(q(0.95), 2), "us_max": round(s[-1], 2)}


def _one(fn, before=None):
    if before is not None:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0


def bench_head(ops, R, V, launches, warmup, dev):
    g = torch.Generator().manual_seed(R)
    gd = torch.Generator(device=dev).manual_seed(R)
    pristine = torch.empty(R, V, dtype=torch.bfloat16, device=dev)
    for a in range(0, R, 256):      # N(0, 2.5) logits, drawn on the device in slices
        pristine[a:a + 256] = (torch.randn(min(256, R - a), V, generator=gd, device=dev) * 2.5).to(torch.bfloat16)
    work = torch.empty_like(pristine)
    tg = torch.randint(0, V, (R,), generator=g).to(I32).to(dev)
    _, ent, lse = ops.logp_entropy_fwd(pristine, tg)
    dlogp = torch.randn(R, generator=g).to(dev)
    dent = (torch.randn(R, generator=g) * 0.01).to(dev)
    restore = lambda: work.copy_(pristine)
    plain = lambda: ops.logp_bwd(work, tg, lse, dlogp, inplace=True)
    with_ent = lambda: ops.logp_entropy_bwd(work, tg, lse, ent, dlogp, dent, inplace=True)
    for _ in range(warmup):
        _one(plain, restore)
        _one(with_ent, restore)
    t_plain, t_ent = [], []
    for _ in range(launches):
        t_plain.append(_one(plain, restore))
        t_ent.append(_one(with_ent, restore))
    gb = 2.0 * R * V * 2 / 1e9
    out = {"R": R, "V": V, "logp_bwd": _stats(t_plain), "logp_entropy_bwd": _stats(t_ent)}
    for k in ("logp_bwd", "logp_entropy_bwd"):
        out[k]["GBps_at_median"] = round(gb / (out[k]["us_median"] * 1e-6), 1)
    out["ratio_of_medians"] = round(out["logp_entropy_bwd"]["us_median"] / out["logp_bwd"]["us_median"], 4)
    out["logp_bwd_spread_p05_p95"] = round((out["logp_bwd"]["us_p95"] - out["logp_bwd"]["us_p05"]) / out["logp_bwd"]["us_median"], 4)
    return out


def bench_select(ops, G, C, launches, warmup, dev, rho=0.2):
    g = torch.Generator().manual_seed(G * C)
    ent = (torch.rand(G, C, generator=g) * 5).to(dev)
    lens = torch.randint(1, C + 1, (G,), generator=g)
    lens[-1] = C
    mask = (torch.arange(C)[None, :] < lens[:, None]).to(I32).to(dev)
    fn = lambda: ops.entropy_quantile_weight(ent, mask, rho)
    for _ in range(warmup):
        _one(fn)
    out = {"G": G, "C": C, "rho": rho, "live": int(mask.sum())}
    out.update(_stats([_one(fn) for _ in range(launches)]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--rows", type=int, nargs="+", default=[1600, 4096])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_entropy_head: no HIP device (a timing needs the GPU)")
    import time_r1_amd  # noqa: F401
    from time_r1_amd.ops import HipOps
    dev = "cuda:0"
    ops = HipOps(dev)
    res = {"launches": a.launches, "head": [bench_head(ops, R, a.vocab, a.launches, a.warmup, dev) for R in a.rows],
           "select": [bench_select(ops, G, C, a.launches, a.warmup, dev) for G, C in ((8, 200), (16, 1024))]}
    print(json.dumps(res))
    print("| shape | kernel | median us | min | p05 | p95 | max | GB/s at median |")
    print("|---|---|---|---|---|---|---|---|")
    for h in res["head"]:
        for k in ("logp_bwd", "logp_entropy_bwd"):
            s = h[k]
            print("| R = %d, V = %d | tr1_%s | %.2f | %.2f | %.2f | %.2f | %.2f | %.1f |" % (h["R"], h["V"], k, s["us_median"], s["us_min"], s["us_p05"], s["us_p95"],
                                                                                         s["us_max"], s["GBps_at_median"]))
        print("| | ratio of medians %.4f; tr1_logp_bwd's own p05..p95 spread %.4f of its median | | | | | | |" % (h["ratio_of_medians"], h["logp_bwd_spread_p05_p95"]))
    for s in res["select"]:
        print("| G = %d, C = %d (%d live), rho = %g | tr1_entropy_quantile_weight | %.2f | %.2f | %.2f | %.2f | %.2f | |"
              % (s["G"], s["C"], s["live"], s["rho"], s["us_median"], s["us_min"], s["us_p05"], s["us_p95"], s["us_max"]))


if __name__ == "__main__":
    main()
