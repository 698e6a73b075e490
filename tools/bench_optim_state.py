"""Milliseconds per fused AdamW launch over the 7B trainable arena with fp32 moments (tr1_adamw_step) and with bf16 moments rounded stochastically
(tr1_adamw_step_sr16, GRPOConfig.optimizer_state_dtype="bf16"), and the device memory of the two optimizer states.

    python tools/bench_optim_state.py                     # Qwen2.5-VL-7B arena (fix_vit=True)
    python tools/bench_optim_state.py --numel 100000000   # any other size

Both kernels run in this one process on the same build, alternating, on the same master / gradient / working-copy arrays (the moments are each kernel's own);
tr1_adamw_step is untouched by the bf16 path, so its figure is the yardstick.  zero_grad is off: 30 B per parameter move with fp32 moments, 22 B with bf16 ones
(the in-place zeroing adds 4 B to both).  Each figure is device events around `--calls` back-to-back launches, repeated `--repeats` times; median and
[min, max] of the repeats, GB/s from those algorithmic bytes and the ratio of the medians are printed as one JSON line.  "sr16_odd_base" is the same launch
with an index_base that is no multiple of 4 (three Philox blocks per lane and trip instead of two): the distance between the two sr16 figures is arithmetic,
not traffic.  lr = 0 keeps the weights where they are however many launches run; the gradient is small random data; the clip coefficient is active.
The arrays are far larger than the 256 MiB memory-side cache: every launch streams from HBM."""
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
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_state: no HIP device (a timing needs the GPU)")
    from time_r1_amd.ops import HipOps
    ops = HipOps("cuda:0")
    dev, F32, BF16 = ops.device, torch.float32, torch.bfloat16
    n = a.numel or arena_numel(a.preset)
    torch.cuda.synchronize()
    p = torch.empty(n, dtype=F32, device=dev).normal_(0.0, 0.02)
    g = torch.empty(n, dtype=F32, device=dev).normal_(0.0, 1e-3)
    p16 = torch.empty(n, dtype=BF16, device=dev)
    base = torch.cuda.memory_allocated()
    m32, v32 = torch.zeros(n, dtype=F32, device=dev), torch.zeros(n, dtype=F32, device=dev)
    mem32 = torch.cuda.memory_allocated() - base
    m16, v16 = torch.zeros(n, dtype=BF16, device=dev), torch.zeros(n, dtype=BF16, device=dev)
    mem16 = torch.cuda.memory_allocated() - base - mem32
    ss = torch.zeros(1, dtype=F32, device=dev)
    ops.sumsq_accum(g, ss)
    step = [0]
    hyp = (0.0, 0.9, 0.999, 1e-8, 0.0)      # lr, betas, eps, weight decay

    def fp32():
        step[0] += 1
        ops.adamw_step(p, m32, v32, g, p16, *hyp, step[0], sumsq=ss, max_norm=1.0, grad_mult=1.0, zero_grad=False)

    def sr16(index_base=0):
        step[0] += 1
        ops.adamw_step_sr16(p, m16, v16, g, p16, *hyp, step[0], 42, index_base, sumsq=ss, max_norm=1.0, grad_mult=1.0, zero_grad=False)

    runs = {"adamw_step": fp32, "adamw_step_sr16": sr16, "sr16_odd_base": lambda: sr16(1)}

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(a.repeats):         # alternating: clock and temperature drift hit all alike
        for k, fn in runs.items():
            t[k].append(once(fn))

    def stats(v, bytes_per):
        v = sorted(v)
        return {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                "gb_per_s_median": round(bytes_per * n / (v[len(v) // 2] * 1e-3) / 1e9, 1)}
    res = {"numel": n, "calls": a.calls, "repeats": a.repeats, "bytes_per_param": {"adamw_step": 30, "adamw_step_sr16": 22},
           "adamw_step": stats(t["adamw_step"], 30), "adamw_step_sr16": stats(t["adamw_step_sr16"], 22), "sr16_odd_base": stats(t["sr16_odd_base"], 22),
           "moments_bytes_allocated": {"fp32": mem32, "bf16": mem16}}
    res["ratio_of_medians"] = round(res["adamw_step_sr16"]["ms_median"] / res["adamw_step"]["ms_median"], 4)
    res["ratio_expected_from_bytes"] = round(22 / 30, 4)
    res["adamw_step_spread"] = round((res["adamw_step"]["ms_max"] - res["adamw_step"]["ms_min"]) / res["adamw_step"]["ms_median"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
