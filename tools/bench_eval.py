"""Batched greedy decoding for evaluation / sample filtering (evaluate.evaluate_grounding(batch_size=...)): what a batch size buys.

    python tools/bench_eval.py --model qwen2-vl-7b --frames 32 --steps 128 --batches 1,4,16,32,64 --reps 3 --parent-like

Seeded synthetic prompts (synthetic.synthetic_prompt; the vision tower runs once per prompt BEFORE the timed region), EOS disabled (an eos id outside the
vocabulary), so every run decodes exactly --steps tokens per row.  Per batch size: prefill of all prompts + the decode loop of `GRPOCore(greedy=True)
.rollout_many` (greedy kernel, early-stop polling armed but never firing).  --parent-like adds the one-row path of `batch_size=None` (top_k = 1 sampler, no
polling): what the evaluation launched per row before batching existed.  The settings alternate inside every repetition; repetition 0 is the warm-up
and is dropped.  One JSON line per setting and repetition, then one summary line per setting (median, min, max):

    ms_per_decode_step   HIP events around the decode loop / steps
    prefill_ms_per_prompt  (HIP events around the whole call - decode loop) / batch: prefill, first-token head, step tables
    samples_per_s        batch / (whole call), decode phase alone in decode_samples_per_s
    hbm_share            algorithmic bytes of the decode loop (weights once per step + the K/V of every row, GRPOCore._count_decode) / time / 8 TB/s

The last lines time the greedy kernel against the three-launch top_k = 1 sampler on the same [64, 152064] bf16 logits (HIP events, alternating)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import time_r1_amd  # noqa: F401,E402
from time_r1_amd.config import PRESETS  # noqa: E402
from time_r1_amd.grpo import GRPOCore  # noqa: E402
from time_r1_amd.model import Engine  # noqa: E402
from time_r1_amd.params import ModelParams  # noqa: E402
from time_r1_amd.synthetic import synthetic_prompt  # noqa: E402

I32 = torch.int32


def time_selection(ops, rows, V, iters, reps):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(rows, V, generator=g).to(torch.bfloat16).to(ops.device)
    step = torch.zeros(1, dtype=I32, device=ops.device)
    tokens = torch.zeros(rows, 4, dtype=I32, device=ops.device)
    fin = torch.zeros(rows, dtype=I32, device=ops.device)
    ids = torch.zeros(rows, dtype=I32, device=ops.device)
    cnt = torch.zeros(1, dtype=I32, device=ops.device)
    forms = {"greedy_kernel": lambda: ops.greedy_tokens(logits, step, tokens, fin, -1, 0, next_ids=ids, done_count=cnt),
             "sampler_top_k_1": lambda: ops.sample_tokens(logits, 1.0, 1, 0, step, tokens, fin, -1, 0, True, group_rows=1, seed_stride=7919, next_ids=ids)}
    out = {k: [] for k in forms}
    for rep in range(reps + 1):
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            if rep:
                out[name].append(1e3 * e0.elapsed_time(e1) / iters)
    for name, v in out.items():
        print(json.dumps(dict(what="token selection [%d, %d] bf16" % (rows, V), form=name, us_per_call_median=round(statistics.median(v), 2),
                              us_min=round(min(v), 2), us_max=round(max(v), 2), iters=iters, reps=reps)), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen2-vl-7b", choices=list(PRESETS))
    ap.add_argument("--frames", type=int, default=32, choices=list(bench.GRIDS))
    ap.add_argument("--steps", type=int, default=128, help="decode steps per run")
    ap.add_argument("--batches", default="1,4,16,32,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-like", action="store_true", help="also time the one-row top_k=1 sampler path without early-stop polling (batch_size=None)")
    ap.add_argument("--layers", type=int, default=0, help="decoder layers (0 = the preset's; smaller values are for trying the tool out)")
    ap.add_argument("--selection-only", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval needs the GPU: there is no CPU path to time")
    from time_r1_amd.ops import HipOps
    ops = HipOps("cuda:0")
    cfg = PRESETS[a.model]()
    if a.layers:
        cfg.text.n_layers = a.layers
    if not a.selection_only:
        batches = [int(x) for x in a.batches.split(",")]
        assert all(1 <= b <= 64 for b in batches)
        grid = bench.GRIDS[a.frames] if a.model not in ("tiny", "tiny25") else (2, 4, 6)
        params = ModelParams(cfg, ops, init="none")
        params.init_random_device(0)
        eng = Engine(cfg, ops, params)
        cfg.eos_token_id = -1          # outside the vocabulary: no row ever finishes
        C = a.steps + 1
        settings = [("batch_%d" % b, b, True) for b in batches]
        if a.parent_like:
            settings.insert(0, ("parent_like_batch_1", 1, False))
        cores = {name: GRPOCore(eng, None, 1, C, beta=0.0, temperature=1.0, top_k=1, seed=0, rope_index_mode="hf4", stop_at_eos=True, reuse_prefill=False, greedy=gr)
                 for name, _, gr in settings}
        prep = cores[settings[0][0]]
        states = [prep.prepare(*synthetic_prompt(cfg, grid, 64, 64, seed=i)) for i in range(max(batches))]
        torch.cuda.synchronize()
        runs = {name: [] for name, _, _ in settings}
        for rep in range(a.reps + 1):
            for name, B, gr in settings:
                core = cores[name]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if gr:
                    core.rollout_many(states[:B])
                else:
                    core.rollout(states[0])
                e1.record()
                e1.synchronize()
                w = core.drain_work()
                total, dec = e0.elapsed_time(e1), w["decode_ms_events"]
                r = dict(setting=name, rep=rep, batch=B, P=states[0].P, steps=a.steps, ms_per_decode_step=round(dec / a.steps, 4),
                         prefill_ms_per_prompt=round((total - dec) / B, 2), samples_per_s=round(B / (total * 1e-3), 3),
                         decode_samples_per_s=round(B / (dec * 1e-3), 3), hbm_share=round(w["decode_bytes"] / (dec * 1e-3) / 8.0e12, 4),
                         steps_run=core.roll.last_steps_run if gr else a.steps)
                print(json.dumps(r), flush=True)
                if rep:
                    runs[name].append(r)
        for name, B, gr in settings:
            rs = runs[name]
            s = dict(setting=name, summary=True, model=cfg.name, layers=cfg.text.n_layers, batch=B, P=states[0].P, steps=a.steps, reps=len(rs))
            for k in ("ms_per_decode_step", "prefill_ms_per_prompt", "samples_per_s", "decode_samples_per_s", "hbm_share"):
                v = [r[k] for r in rs]
                s[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
            s["peak_hbm_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
            print(json.dumps(s), flush=True)
    time_selection(ops, 64, 152064, 200, a.reps)


if __name__ == "__main__":
    main()
