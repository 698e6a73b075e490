"""Cost of training the vision tower (GRPOConfig.fix_vit=False) against the frozen tower, on bench.py's workload: the same TimeR1_Trainer,
synthetic clips and `optimizer_window` loop, one setting per process (the two arena layouts do not fit one card together at 7B).

    python tools/bench_vit_train.py --model qwen2-vl-7b --fix-vit false      # config 3 shapes (32 frames of 360x640, G 8, C 200)
    python tools/bench_vit_train.py --model qwen2.5-vl-7b --fix-vit false --frames 64 --G 16 --C 1024 --beta 0 --clip-loss   # config 4

Prints one JSON line: ms per micro-step (device-synchronised wall clock over the timed windows), the tower's backward and its recompute
(device events around Engine.vit_bwd / vit_features(save=True), summed per micro-step), and peak HBM (torch.cuda.max_memory_allocated)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from time_r1_amd import trainer as T  # noqa: E402
from time_r1_amd.params import ModelParams  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen2-vl-7b")
    ap.add_argument("--fix-vit", default="false", choices=["true", "false"])
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--C", type=int, default=200)
    ap.add_argument("--beta", type=float, default=0.04)
    ap.add_argument("--ga", type=int, default=2)
    ap.add_argument("--clip-loss", action="store_true", help="PPO-clip branch (bench.py --clip-loss; config 4 as specified)")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args(argv)
    fix_vit = a.fix_vit == "true"
    bargs = bench.parse_args(["--model", a.model, "--frames", str(a.frames), "--G", str(a.G), "--C", str(a.C), "--beta", str(a.beta), "--ga", str(a.ga)]
                             + (["--clip-loss"] if a.clip_loss else []))
    from time_r1_amd.ops import HipOps
    ops = HipOps("cuda:0")
    ops.use_priority_stream()
    # the workload builds its ModelParams and GRPOConfig itself: give both the fix_vit setting (no relayout copy of a 7B arena)
    bench.ModelParams = lambda *x, **k: ModelParams(*x, **k, train_vit=not fix_vit)
    base_cfg = T.GRPOConfig
    T.GRPOConfig = lambda **k: base_cfg(**k, fix_vit=fix_vit)
    wl = bench.Workload(bargs, ops, torch.device("cuda:0"), 0)
    eng = wl.eng
    ev = {"vit_bwd": [], "recompute": []}

    def timed(name, fn, pred=lambda *x, **k: True):
        def f(*x, **k):
            if not pred(*x, **k):
                return fn(*x, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*x, **k)
            e1.record()
            ev[name].append((e0, e1))
            return r
        return f
    eng.vit_bwd = timed("vit_bwd", eng.vit_bwd)
    eng.vit_features = timed("recompute", eng.vit_features, lambda *x, **k: k.get("save", False))
    for _ in range(a.warmup):
        wl.window()
    torch.cuda.synchronize()
    for k in ev:
        ev[k] = []
    torch.cuda.reset_peak_memory_stats()
    n = max(1, a.steps // a.ga)
    t0 = time.perf_counter()
    for _ in range(n):
        wl.window()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    micro = n * a.ga
    out = dict(model=a.model, fix_vit=fix_vit, frames=a.frames, G=a.G, C=a.C, beta=a.beta, ga=a.ga, micro_steps=micro,
               ms_per_micro_step=round(1e3 * dt / micro, 2),
               ms_vit_bwd_per_micro_step=round(sum(e0.elapsed_time(e1) for e0, e1 in ev["vit_bwd"]) / micro, 2),
               ms_vit_recompute_per_micro_step=round(sum(e0.elapsed_time(e1) for e0, e1 in ev["recompute"]) / micro, 2),
               peak_hbm_gb=round(torch.cuda.max_memory_allocated() / 1e9, 2))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
