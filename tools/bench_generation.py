"""What one rollout for several accumulation windows (GRPOConfig.steps_per_generation = k x GA) buys: TimeR1_Trainer.generation_cycle timed for a list of k.

    python tools/bench_generation.py                                       # bench.py's flagship: 7B, 32 frames, G 8, C 200, GA 2, beta 0.04; k = 1, 2, 4
    python tools/bench_generation.py --model qwen2-vl-2b --frames 16 --k 1 2

The workload is bench.py's (its Workload class: presets, synthetic clips, seeds, sampler and prefetch thread) on the PPO-clip loss - k > 1 needs the clipped
branch, and k = 1, the yardstick, is timed on the same branch in the same process (k = 1 is `optimizer_window`, what bench.py times).  After `--warmup` cycles
of every k, `--reps` repetitions alternate over the k values; each repetition times ONE cycle of each k: host wall clock around the cycle between device
synchronisations, divided by the cycle's k x GA micro-steps.  Phases are the trainer's HIP-event marks (rollout, score, logps, backward, optimizer, ...), in ms
per micro-step; rollout tokens/s = generated tokens over the rollout phase; peak memory is torch's max_memory_allocated over that k's timed cycles (reset
before each).  Prints ONE JSON line: per k the median and min - max of ms per micro-step over the repetitions, and the medians of the rest."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def one_cycle(wl, k):
    """One generation cycle of k windows through the trainer -> dict(ms per micro-step, phases per micro-step, tokens, peak bytes)."""
    tr, ga = wl.trainer, wl.args.ga
    tr.args.steps_per_generation = None if k == 1 else k * ga
    windows = [[next(wl._feed) for _ in range(ga)] for _ in range(k)]
    tr._flush_metrics()
    tr._throughput_keys()                         # fold earlier marks away: the cycle's phases are what follows
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ph0, tok0, step0 = dict(tr.phase_ms_total), tr.generated_tokens, tr.state.global_step
    t0 = time.perf_counter()
    tr.generation_cycle(windows)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    tr._flush_metrics()
    tr._throughput_keys()
    assert tr.state.global_step - step0 == k * tr.num_iterations
    n = k * ga
    ph = {p: (v - ph0.get(p, 0.0)) / n for p, v in tr.phase_ms_total.items() if v - ph0.get(p, 0.0) > 0}
    toks = tr.generated_tokens - tok0
    return dict(ms=1e3 * wall / n, phases=ph, tokens_per_sec=toks / (ph["rollout"] * n * 1e-3) if ph.get("rollout") else None,
                peak=torch.cuda.max_memory_allocated())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen2-vl-7b")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--C", type=int, default=200)
    ap.add_argument("--ga", type=int, default=2)
    ap.add_argument("--beta", type=float, default=0.04)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 2, 4], help="windows per generation cycle (steps_per_generation = k x GA)")
    ap.add_argument("--reps", type=int, default=3, help="timed cycles per k, alternating over the k values")
    ap.add_argument("--warmup", type=int, default=1, help="untimed cycles per k before the first repetition")
    ap.add_argument("--group-rows", type=int, default=None, help="TimeR1_Trainer.rollout_group_rows (default: the class attribute, 32)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_generation: no HIP device (a timing needs the GPU)")
    import time_r1_amd  # noqa: F401
    from time_r1_amd.ops import HipOps
    import bench
    ops = HipOps("cuda:0")
    ops.use_priority_stream()
    bargs = bench.parse_args(["--model", a.model, "--frames", str(a.frames), "--G", str(a.G), "--C", str(a.C), "--beta", str(a.beta), "--ga", str(a.ga),
                              "--clip-loss", "--n-prompts", str(max(2, max(a.k) * a.ga))])
    wl = bench.Workload(bargs, ops, torch.device("cuda:0"), 0)
    if a.group_rows is not None:
        wl.trainer.rollout_group_rows = a.group_rows
    for _ in range(a.warmup):
        for k in a.k:
            one_cycle(wl, k)
    runs = {k: [] for k in a.k}
    for _ in range(a.reps):
        for k in a.k:
            runs[k].append(one_cycle(wl, k))
    med = statistics.median
    by_k = {}
    for k, rs in runs.items():
        names = sorted({p for r in rs for p in r["phases"]})
        by_k[str(k)] = dict(steps_per_generation=k * a.ga, decode_rows=min(k * a.ga * a.G, max(a.G, wl.trainer.rollout_group_rows // a.G * a.G)),
                            ms_per_micro_step=dict(median=round(med(r["ms"] for r in rs), 2), min=round(min(r["ms"] for r in rs), 2), max=round(max(r["ms"] for r in rs), 2)),
                            phases_ms_per_micro_step={p: round(med(r["phases"].get(p, 0.0) for r in rs), 2) for p in names},
                            rollout_tokens_per_sec=round(med(r["tokens_per_sec"] or 0.0 for r in rs), 1),
                            max_memory_allocated_gb=round(max(r["peak"] for r in rs) / 1e9, 2))
    print(json.dumps(dict(tool="bench_generation", model=a.model, frames=a.frames, G=a.G, C=a.C, ga=a.ga, beta=a.beta, loss="clip", reps=a.reps, warmup=a.warmup,
                          rollout_group_rows=wl.trainer.rollout_group_rows, P=int(wl.trainer.core.last_P), by_k=by_k)), flush=True)


if __name__ == "__main__":
    main()
