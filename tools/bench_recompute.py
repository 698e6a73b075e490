"""One GRPO micro-step with activation_recompute="none" and "mlp" (DESIGN.md section 7p): milliseconds per phase and peak memory, one JSON line per mode.

    python tools/bench_recompute.py                                       # configuration 4: Qwen2.5-VL-7B, 64 frames, G = 16, C = 1024, beta = 0, both modes
    python tools/bench_recompute.py --modes mlp --C 2048                  # a shape whose "none" activations do not fit beside the optimizer state
    python tools/bench_recompute.py --preset tiny --frames 4 --G 4 --C 24 # plumbing check

Synthetic weights (normal, 0.02) with the optimizer state a training run holds, synthetic uint8 frames through the fused preprocess kernel, sampled completions.
A micro-step is prepare -> rollout -> forward_logps -> loss_backward on one prompt; there is no optimizer step, so every repeat of both modes runs on the same
weights.  The "none" record is the yardstick: it is the code path of a run that does not name the option, in the same process on the same card.  Per phase:
a device-event pair around the phase, `--warmup` untimed micro-steps, then the median (and min / max) of `--repeats` timed ones.  Memory: the caching allocator's
peak allocated / reserved bytes and retry count over the mode's micro-steps, the cache emptied and the peaks reset before each mode.  A mode that runs out of
memory prints the phase it failed in and the peaks it reached."""
import argparse
import gc
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("prepare", "rollout", "forward_logps", "loss_backward")
SRC_HW = (360, 640)
VIDEO_ELE = {"total_pixels": 3584 * 28 * 28, "min_pixels": 16 * 28 * 28}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="qwen2.5-vl-7b")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--G", type=int, default=16)
    ap.add_argument("--C", type=int, default=1024)
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--fix-vit", default="true", choices=["true", "false"])
    ap.add_argument("--modes", default="none,mlp")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_recompute: no HIP device (a timing needs the GPU)")
    import time_r1_amd  # noqa: F401
    from time_r1_amd import vision_process as VP
    from time_r1_amd.config import PRESETS
    from time_r1_amd.grpo import GRPOCore
    from time_r1_amd.model import Engine, check_activation_recompute
    from time_r1_amd.ops import HipOps
    from time_r1_amd.params import ModelParams
    from time_r1_amd.synthetic import SyntheticProcessor
    modes = [check_activation_recompute(m) for m in a.modes.split(",") if m]
    ops = HipOps("cuda:0")
    cfg = PRESETS[a.preset]()
    v, tiny = cfg.vision, a.preset.startswith("tiny")
    params = ModelParams(cfg, ops, init="none", optimizer_state=True, train_vit=a.fix_vit == "false")
    params.init_random_device(seed=0)
    ref = params.train.clone_weights_only() if a.beta != 0.0 else None
    src_hw = (72, 96) if tiny else SRC_HW
    target = (56, 84) if tiny else VP.video_target_size(VIDEO_ELE, a.frames, *src_hw)
    frames = torch.randint(0, 256, (a.frames, 3) + src_hw, generator=torch.Generator().manual_seed(7), dtype=torch.uint8).to(ops.device)
    proc = SyntheticProcessor(cfg)
    adv = ops.tensor(torch.randn(a.G, generator=torch.Generator().manual_seed(1)).numpy(), torch.float32)
    mask = torch.ones(a.G, a.C, dtype=torch.int32, device=ops.device)
    eng = Engine(cfg, ops, params)

    def micro_step(core, times):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(PHASES) + 1)]
        phase = PHASES[0]
        try:
            ev[0].record()
            pix, grid = ops.video_preprocess(frames, target, v.patch_dim_padded, v.patch_size, v.temporal_patch_size, v.spatial_merge_size)
            ids = np.asarray(proc.prompt_ids("synthetic query", grid[0] * grid[1] * grid[2] // v.merge_unit)).reshape(-1)
            st = core.prepare(ids, pix, np.asarray([grid]))
            ev[1].record()
            phase = PHASES[1]
            core.rollout(st)
            ev[2].record()
            phase = PHASES[2]
            core.forward_logps(st)
            ev[3].record()
            phase = PHASES[3]
            core.loss_backward(st, mask, adv, 1.0)
            ev[4].record()
            ev[4].synchronize()
        except torch.OutOfMemoryError:
            return phase, None
        if times is not None:
            for i, p in enumerate(PHASES):
                times[p].append(ev[i].elapsed_time(ev[i + 1]))
        return None, st.layout.M

    for mode in modes:
        core = GRPOCore(eng, ref, a.G, a.C, beta=a.beta, use_grpo=False, seed=1234, rope_index_mode="hf4", activation_recompute=mode)
        params.train.grad.zero_()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        retries0 = torch.cuda.memory_stats().get("num_alloc_retries", 0)
        times = {p: [] for p in PHASES}
        failed, rows = None, None
        for i in range(a.warmup + a.repeats):
            failed, rows = micro_step(core, times if i >= a.warmup else None)
            if failed:
                break
        torch.cuda.synchronize()
        rec = {"mode": mode, "preset": a.preset, "frames": a.frames, "G": a.G, "C": a.C, "beta": a.beta, "fix_vit": a.fix_vit == "true", "rows": rows,
               "prompt_rows": getattr(core, "last_P", None), "warmup": a.warmup, "repeats": len(times[PHASES[0]])}
        if failed:
            rec["failed_in"] = failed
            rec["failed_at_micro_step"] = i
        if times[PHASES[-1]]:
            med = {p: sorted(t)[len(t) // 2] for p, t in times.items()}
            rec["ms"] = {p: round(med[p], 3) for p in PHASES}
            rec["ms_min_max"] = {p: [round(min(t), 3), round(max(t), 3)] for p, t in times.items()}
            rec["ms_update"] = round(med["forward_logps"] + med["loss_backward"], 3)
            rec["ms_step"] = round(sum(med.values()), 3)
        rec["max_memory_allocated"] = torch.cuda.max_memory_allocated()
        rec["max_memory_reserved"] = torch.cuda.max_memory_reserved()
        rec["alloc_retries"] = torch.cuda.memory_stats().get("num_alloc_retries", 0) - retries0
        if rows:
            rec["ctx_bytes"] = eng.ctx_bytes(rows)
            rec["recompute_set_bytes"] = eng.recompute_set_bytes(rows) if mode == "mlp" else 0
        print(json.dumps(rec), flush=True)
        del core
        eng.__dict__.pop("_ctx_pool", None)
        eng.__dict__.pop("_rc_set", None)


if __name__ == "__main__":
    main()
