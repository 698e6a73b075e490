"""Milliseconds per reference-policy sync (tr1_ref_mixup, GRPOConfig.sync_ref_model) over the 7B trainable arena, against tr1_add_bf16 on the same element count.

    python tools/bench_ref_sync.py                     # Qwen2.5-VL-7B arena (fix_vit=True), alpha = 0.6
    python tools/bench_ref_sync.py --numel 100000000   # any other size (rounded down to a multiple of 8: tr1_add_bf16 takes no tail)

tr1_add_bf16 is the yardstick: it moves the same bytes (two bf16 reads, one bf16 write per element) and is not code under test.  Both run in this one process,
alternating, on the same two random bf16 arrays (normal, the policy a few percent off the reference); each figure is device events around `--calls`
back-to-back calls, repeated `--repeats` times; median and [min, max] of the repeats and the ratio of the medians are printed as one JSON line.
The arrays are far larger than the 256 MiB memory-side cache: every call streams from HBM."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _CountOps:
    """Arena only asks its backend for zero-filled storage: meta tensors give the element count without the memory."""
    act_dtype = torch.bfloat16

    def zeros(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or self.act_dtype, device="meta")


def arena_numel(preset):
    import time_r1_amd  # noqa: F401
    from time_r1_amd import config
    from time_r1_amd.params import Arena, arena_specs
    trs, _ = arena_specs(getattr(config, preset)(), train_vit=False)
    return Arena(_CountOps(), trs, with_optimizer_state=False, with_grad=False).numel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="qwen2_5_vl_7b")
    ap.add_argument("--numel", type=int, default=0, help="elements; 0 = the preset's trainable arena")
    ap.add_argument("--alpha", type=float, default=0.6)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ref_sync: no HIP device (a timing needs the GPU)")
    from time_r1_amd.ops import HipOps, _p
    ops = HipOps("cuda:0")
    n = (a.numel or arena_numel(a.preset)) // 8 * 8
    ref = torch.empty(n, dtype=torch.bfloat16, device=ops.device).normal_(0.0, 0.02)
    pol = torch.empty(n, dtype=torch.bfloat16, device=ops.device)
    step = 1 << 28
    for i in range(0, n, step):        # policy = reference * (1 + 3 % noise), built in pieces: no fp32 copy of the whole arena
        pol[i:i + step] = (ref[i:i + step].float() * (1.0 + 0.03 * torch.randn(min(step, n - i), device=ops.device))).to(torch.bfloat16)
    out = torch.empty(n, dtype=torch.bfloat16, device=ops.device)

    def mix():
        ops.ref_mixup(ref, pol, a.alpha)

    def add():
        ops.L.call("tr1_add_bf16", _p(ref), _p(pol), _p(out), n, ops._s())

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    for _ in range(a.warmup):
        mix()
        add()
    torch.cuda.synchronize()
    t = {"ref_mixup": [], "add_bf16": []}
    for _ in range(a.repeats):         # alternating: clock and temperature drift hit both alike
        t["ref_mixup"].append(once(mix))
        t["add_bf16"].append(once(add))

    def stats(v):
        v = sorted(v)
        return {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                "tb_per_s_median": round(6.0 * n / (v[len(v) // 2] * 1e-3) / 1e12, 3)}
    res = {"numel": n, "bytes_moved": 6 * n, "alpha": a.alpha, "calls": a.calls, "repeats": a.repeats, "ref_mixup": stats(t["ref_mixup"]), "add_bf16": stats(t["add_bf16"])}
    res["ratio_of_medians"] = round(res["ref_mixup"]["ms_median"] / res["add_bf16"]["ms_median"], 4)
    res["add_bf16_spread"] = round((res["add_bf16"]["ms_max"] - res["add_bf16"]["ms_min"]) / res["add_bf16"]["ms_median"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
