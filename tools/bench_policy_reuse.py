"""What several policy updates per rollout (GRPOConfig.num_iterations = mu) buy, and what the ratio-loss kernel costs.

    python tools/bench_policy_reuse.py --kernels                         # tr1_grpo_loss_ratio and tr1_grpo_policy_loss against tr1_grpo_loss, us per launch
    python tools/bench_policy_reuse.py --model qwen2-vl-7b               # bench.py's config 3 workload (32 frames, G 8, C 200, beta 0.04, GA 2), mu = 1, 2, 4
    python tools/bench_policy_reuse.py --model qwen2-vl-2b --frames 16   # config 2

The end-to-end part builds bench.py's Workload (same presets, synthetic clips, seeds, TimeR1_Trainer.optimizer_window loop) with the PPO-clip loss
(`bench.py --clip-loss`: num_iterations > 1 needs the clipped branch; mu = 1 is timed on the same branch) and, for each mu in one process, warms up
`--warmup` loader windows and times `--windows` more.  Times are the trainer's HIP-event phase times (the marks `log()` reads: preprocess, vision, rollout,
logps, backward, optimizer) summed over the timed windows; the host wall clock over the same windows is printed beside them.  One JSON line per mode.
The kernel part: device events around each single launch, median of `--launches` (>= 50) launches after a warm-up, at (G, C) = (8, 200) and (16, 1024).  An event
pair around one launch includes the launch itself; for kernel time alone run the same command under `rocprofv3 --kernel-trace --stats`, one `--shapes GxC` per run."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def kernel_times(ops, launches, warmup, shapes):
    res = {}
    g = torch.Generator().manual_seed(0)
    for G, C in shapes:
        logp = (-torch.rand(G, C, generator=g) * 3).to(ops.device)
        old = (logp.cpu() - (torch.rand(G, C, generator=g) * 2 - 1) * 0.6).to(ops.device)
        ref = (logp.cpu() + torch.randn(G, C, generator=g) * 0.3).to(ops.device)
        tokw = (torch.rand(G, C, generator=g) * 2).to(ops.device)
        mask = torch.ones(G, C, dtype=torch.int32)
        for r in range(G):
            mask[r, int(torch.randint(C // 2, C + 1, (1,), generator=g)):] = 0
        mask = mask.to(ops.device)
        adv = torch.randn(G, generator=g).to(ops.device)
        fns = {
            "grpo_loss (one update per rollout)": lambda: ops.grpo_loss(logp, ref, mask, adv, 0.04, False, 0.5),
            "grpo_loss_ratio": lambda: ops.grpo_loss_ratio(logp, old, ref, mask, adv, 0.04, False, 0.2, 0.2, 0.5),
            "grpo_loss_ratio + tok_weight": lambda: ops.grpo_loss_ratio(logp, old, ref, mask, adv, 0.04, False, 0.2, 0.2, 0.5, tok_weight=tokw),
            "grpo_loss_ratio, use_grpo": lambda: ops.grpo_loss_ratio(logp, old, ref, mask, adv, 0.04, True, 0.2, 0.2, 0.5),
            "grpo_policy_loss, token level (bnpo)": lambda: ops.grpo_policy_loss(logp, old, ref, mask, adv, 0.04, "token", "token", 0.2, 0.2, None, 0.5),
            "grpo_policy_loss, token level, row mean + delta": lambda: ops.grpo_policy_loss(logp, old, ref, mask, adv, 0.04, "row", "token", 0.2, 0.2, 1.5, 0.5),
            "grpo_policy_loss, sequence level": lambda: ops.grpo_policy_loss(logp, old, ref, mask, adv, 0.04, "token", "sequence", 0.2, 0.2, None, 0.5),
            "grpo_policy_loss, sequence level + delta + tok_weight": lambda: ops.grpo_policy_loss(logp, old, ref, mask, adv, 0.04, "fixed", "sequence", 0.2, 0.2, 1.5, 0.5,
                                                                                                  tok_weight=tokw),
        }
        row = {}
        for name, fn in fns.items():
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            us = []
            for _ in range(launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            us.sort()
            row[name] = {"us_median": round(us[len(us) // 2], 2), "us_min": round(us[0], 2), "us_max": round(us[-1], 2)}
        res["G=%d,C=%d" % (G, C)] = row
    return res


def end_to_end(a, ops):
    import bench
    bargs = bench.parse_args(["--model", a.model, "--frames", str(a.frames), "--G", str(a.G), "--C", str(a.C), "--beta", str(a.beta), "--ga", str(a.ga), "--clip-loss"])
    wl = bench.Workload(bargs, ops, torch.device("cuda:0"), 0)
    tr = wl.trainer
    out = dict(model=a.model, frames=a.frames, G=a.G, C=a.C, beta=a.beta, ga=a.ga, loss="clip", windows=a.windows, warmup=a.warmup, by_mu={})
    for mu in a.mu:
        tr.num_iterations = mu
        for _ in range(a.warmup):
            wl.window()
        torch.cuda.synchronize()
        tr.phase_ms_total.clear()
        step0 = tr.state.global_step
        t0 = time.perf_counter()
        for _ in range(a.windows):
            wl.window()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        tr._throughput_keys()                     # folds any phase marks log() has not read yet into phase_ms_total
        steps = tr.state.global_step - step0
        assert steps == a.windows * mu, (steps, a.windows, mu)
        ph = {k: round(v / steps, 2) for k, v in sorted(tr.phase_ms_total.items())}
        ms = sum(tr.phase_ms_total.values()) / steps
        out["by_mu"][str(mu)] = dict(optimizer_steps=steps, rollouts=a.windows, ms_per_optimizer_step=round(ms, 1), optimizer_steps_per_sec=round(1e3 / ms, 3),
                                     wall_ms_per_optimizer_step=round(1e3 * wall / steps, 1), phase_ms_per_optimizer_step=ph,
                                     policy_kl_old=[round(x["policy_kl_old"], 6) for x in tr.state.log_history[-mu:] if "policy_kl_old" in x],
                                     clip_region=[round(x["clip_ratio/region_mean"], 6) for x in tr.state.log_history[-mu:] if "clip_ratio/region_mean" in x])
    out["peak_hbm_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="time the loss kernels only")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--shapes", nargs="+", default=["8x200", "16x1024"], help="GxC grids of the kernel part (one per process under a profiler: its table is per kernel name)")
    ap.add_argument("--model", default="qwen2-vl-7b")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--C", type=int, default=200)
    ap.add_argument("--beta", type=float, default=0.04)
    ap.add_argument("--ga", type=int, default=2)
    ap.add_argument("--mu", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--windows", type=int, default=4, help="timed loader windows (rollouts) per mu")
    ap.add_argument("--warmup", type=int, default=2, help="warm-up loader windows per mu")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_policy_reuse: no HIP device (a timing needs the GPU)")
    import time_r1_amd  # noqa: F401
    from time_r1_amd.ops import HipOps
    ops = HipOps("cuda:0")
    if a.kernels:
        assert a.launches >= 50
        print(json.dumps({"kernel_us": kernel_times(ops, a.launches, 20, [tuple(int(x) for x in sh.split("x")) for sh in a.shapes]), "launches": a.launches}), flush=True)
        return
    ops.use_priority_stream()
    print(json.dumps(end_to_end(a, ops)), flush=True)


if __name__ == "__main__":
    main()
