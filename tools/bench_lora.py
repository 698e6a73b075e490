"""LoRA measurements (peft_config, DESIGN.md section 7r / BASELINE.md section 4m).  One JSON line per mode.

    python tools/bench_lora.py kernels                 # tr1_lora_merge over the 7B decoder, tr1_lora_wgrad against the composition at config 3's operand shapes
    python tools/bench_lora.py step --lora             # config 3 (Qwen2-VL-7B, 32 frames, G = 8, C = 200, GA = 2): ms per micro-step, phases, peak memory, r = 16 all-linear
    python tools/bench_lora.py step                    # the same script, full-parameter training (the comparison run)

kernels: device events around `--calls` back-to-back calls, `--repeats` times, kernel and composition alternating; median [min, max].  The merge is timed over all
28 layers' seven projections (W and W0 of 13 GB each: far beyond the 256 MiB memory-side cache), its bytes bound is 4 B per merged parameter over 8 TB/s.
step: `--warmup` windows, then `--windows` timed optimizer windows through TimeR1_Trainer.optimizer_window, as bench.py does; the phase times are the trainer's own
perf/ms_* keys (HIP events), memory is torch.cuda.max_memory_allocated over the timed windows."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def _events(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def _stats(v):
    v = sorted(v)
    return {"ms_median": round(v[len(v) // 2], 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4)}


def kernels(a):
    import time_r1_amd  # noqa: F401
    from time_r1_amd.config import PRESETS
    from time_r1_amd.ops import HipOps
    ops = HipOps("cuda:0")
    dev = ops.device
    t = PRESETS[a.model]().text
    M = a.rows
    res = {"mode": "kernels", "model": a.model, "rows": M, "calls": a.calls, "repeats": a.repeats}
    # ---- merge: every targeted projection of every layer, as LoraAdapters.merge issues them
    mats = [("qkv", t.qkv_dim, t.hidden, ((0, t.q_dim), (t.q_dim, t.kv_dim), (t.q_dim + t.kv_dim, t.kv_dim))), ("o", t.hidden, t.q_dim, ((0, t.hidden),)),
            ("gu", 2 * t.intermediate, t.hidden, ((0, t.intermediate), (t.intermediate, t.intermediate))), ("down", t.hidden, t.intermediate, ((0, t.hidden),))]
    per_layer = sum(o * i for _, o, i, _ in mats)
    W = torch.empty(t.n_layers * per_layer, dtype=torch.bfloat16, device=dev)
    W0 = torch.empty(t.n_layers * per_layer, dtype=torch.bfloat16, device=dev).normal_(0.0, 0.02)
    res["merge"] = {"parameters": t.n_layers * per_layer}
    for r in (16, 64):
        ad = {}
        for _, _, in_, parts in mats:
            for _, rows in parts:
                ad.setdefault((rows, in_), (torch.empty(r, in_, device=dev).uniform_(-in_ ** -0.5, in_ ** -0.5), torch.empty(r, rows, device=dev).normal_(0.0, 0.02)))

        def merge_all():
            off = 0
            for _ in range(t.n_layers):
                for _, o, i, parts in mats:
                    w, w0 = W[off: off + o * i].view(o, i), W0[off: off + o * i].view(o, i)
                    for r0, rows in parts:
                        A, Bt = ad[(rows, i)]
                        ops.lora_merge(w[r0:r0 + rows], w0[r0:r0 + rows], A, Bt, 2.0)
                    off += o * i
        merge_all()
        torch.cuda.synchronize()
        ts = [_events(merge_all, 1) for _ in range(a.repeats)]
        s = _stats(ts)
        bound_ms = 4.0 * t.n_layers * per_layer / HBM_PEAK * 1e3
        s.update(bytes_bound_ms=round(bound_ms, 4), frac_of_bytes_bound=round(bound_ms / s["ms_median"], 4), launches=t.n_layers * 7)
        res["merge"]["r%d" % r] = s
    del W, W0
    # ---- rank-r weight gradient: the operand shapes of one decoder layer's backward at config 3 (wide = dY for dBt, wide = x for dA)
    shapes = [("dY q (slice of dqkv)", t.q_dim, t.qkv_dim, 1), ("dY k / v (slices of dqkv)", t.kv_dim, t.qkv_dim, 2), ("dY o", t.hidden, t.hidden, 1),
              ("dY gate / up (halves of dgu)", t.intermediate, 2 * t.intermediate, 2), ("dY down", t.hidden, t.hidden, 1),
              ("x = xn / xn2 (q, k, v, gate, up)", t.hidden, t.hidden, 5), ("x = attention output (o)", t.q_dim, t.q_dim, 1), ("x = SwiGLU output (down)", t.intermediate, t.intermediate, 1)]
    res["wgrad"] = []
    for r in (16, 64):
        layer_k = layer_c = 0.0
        for name, Wd, ld, uses in shapes:
            buf = torch.empty(M, ld, dtype=torch.bfloat16, device=dev).normal_()
            wide = buf[:, ld - Wd:] if ld > Wd else buf
            thin = torch.empty(M, r, dtype=torch.bfloat16, device=dev).normal_()
            g = torch.zeros(r, Wd, dtype=torch.float32, device=dev)
            assert ops.lora_wgrad_covers(g, thin, wide)
            k = lambda: ops.lora_wgrad(g, thin, wide, 2.0, accumulate=True)
            c = lambda: ops.lora_wgrad_composed(g, thin, wide, 2.0, accumulate=True)
            for _ in range(2):
                k(); c()
            torch.cuda.synchronize()
            tk, tc = [], []
            for _ in range(a.repeats):
                tk.append(_events(k, a.calls))
                tc.append(_events(c, a.calls))
            sk, scmp = _stats(tk), _stats(tc)
            bound_ms = (2.0 * M * Wd + 2.0 * M * r + 4.0 * r * Wd) / HBM_PEAK * 1e3
            res["wgrad"].append({"operand": name, "r": r, "Wd": Wd, "ldw": ld, "uses_per_layer": uses, "splits": ops.lora_wgrad_splits(M, Wd)[0], "kernel": sk,
                                 "composition": scmp, "ratio_of_medians": round(sk["ms_median"] / scmp["ms_median"], 4),
                                 "kernel_frac_of_bytes_bound": round(bound_ms / sk["ms_median"], 4)})
            layer_k += uses * sk["ms_median"]
            layer_c += uses * scmp["ms_median"]
            del buf, wide, thin, g
        res["wgrad_layer_ms_r%d" % r] = {"kernel": round(layer_k, 4), "composition": round(layer_c, 4)}
    print(json.dumps(res))


def step(a):
    import bench
    import time_r1_amd  # noqa: F401
    from time_r1_amd import rewards as R
    from time_r1_amd import vision_process as VP
    from time_r1_amd.config import PRESETS
    from time_r1_amd.ops import HipOps
    from time_r1_amd.params import ModelParams
    from time_r1_amd.synthetic import SyntheticClips, SyntheticProcessor
    from time_r1_amd.trainer import GRPOConfig, TimeR1_Trainer
    ops = HipOps("cuda:0")
    ops.use_priority_stream()
    dev = ops.device
    cfg = PRESETS[a.model]()
    kw = dict(optimizer_state=False, with_grad=False) if a.lora else {}
    params = ModelParams(cfg, ops, init="none", **kw)
    params.init_random_device(seed=0)
    grid, v = bench.GRIDS[a.frames], cfg.vision
    n_frames = grid[0] * v.temporal_patch_size
    assert tuple(x // v.patch_size for x in VP.video_target_size(bench.VIDEO_ELE, n_frames, *bench.SRC_HW)) == tuple(grid[1:])
    data = SyntheticClips(a.n_prompts, n_frames, bench.SRC_HW, device=dev, pin=False)
    targs = GRPOConfig(output_dir="/tmp/tr1_bench_lora", num_generations=a.G, max_completion_length=a.C, beta=0.04, use_grpo=True, temperature=1.0, top_k=50, seed=1234,
                       rope_index_mode="hf4", gradient_accumulation_steps=a.ga, learning_rate=1e-6, lr_scheduler_type="constant", logging_steps=1, save_strategy="no",
                       disable_log_print=True, activation_recompute=a.activation_recompute, optimizer_state_dtype=a.optimizer_state_dtype)
    peft = dict(r=a.r, lora_alpha=2 * a.r, target_modules="all-linear") if a.lora else None
    tr = TimeR1_Trainer(params, [R.iou_timestamp_reward_v2, R.format_reward], [], args=targs, train_dataset=data, processing_class=SyntheticProcessor(cfg), ops=ops,
                        peft_config=peft)

    def feed():
        while True:
            for b in tr._prefetching(tr.get_train_dataloader()):
                yield b
    it = feed()
    for _ in range(a.warmup):
        tr.optimizer_window([next(it) for _ in range(a.ga)])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    n0 = len(tr.state.log_history)
    t0 = time.perf_counter()
    for _ in range(a.windows):
        tr.optimizer_window([next(it) for _ in range(a.ga)])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    logs = tr.state.log_history[n0:]
    phases = {}
    for k in ("rollout", "logps", "backward", "optimizer"):
        vals = sorted(l["perf/ms_" + k] for l in logs if "perf/ms_" + k in l)
        if vals:
            phases[k] = {"ms_median": round(vals[len(vals) // 2], 3), "ms_min": round(vals[0], 3), "ms_max": round(vals[-1], 3)}
    res = {"mode": "step", "lora": bool(a.lora), "model": a.model, "frames": a.frames, "G": a.G, "C": a.C, "ga": a.ga, "windows": a.windows, "warmup": a.warmup,
           "P": int(tr.core.last_P), "rows": int(tr.core.last_P) + a.G * a.C, "ms_per_micro_step": round(wall * 1e3 / (a.windows * a.ga), 3),
           "phase_ms_per_micro_step": phases, "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated() / 1e9, 3),
           "memory_allocated_gb": round(torch.cuda.memory_allocated() / 1e9, 3), "activation_recompute": a.activation_recompute,
           "optimizer_state_dtype": a.optimizer_state_dtype}
    if a.lora:
        base = params.train.numel
        res.update(r=a.r, adapter_parameters=tr.lora.numel(), base_parameters=int(base), derived_weights_and_adapter_state_gb=round((4 * base + 18 * tr.lora.train.numel) / 1e9, 3))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "step"])
    ap.add_argument("--model", default="qwen2-vl-7b")
    ap.add_argument("--rows", type=int, default=5074, help="kernels: M of the rank-r weight gradients (config 3: 3474 prompt rows + 8 x 200)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--lora", action="store_true")
    ap.add_argument("--r", type=int, default=16)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--C", type=int, default=200)
    ap.add_argument("--ga", type=int, default=2)
    ap.add_argument("--n-prompts", type=int, default=2)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--activation-recompute", default="none")
    ap.add_argument("--optimizer-state-dtype", default="fp32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lora: no HIP device (a timing needs the GPU)")
    kernels(a) if a.mode == "kernels" else step(a)


if __name__ == "__main__":
    main()
