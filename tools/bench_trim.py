"""What GRPOConfig.trim_completions buys in the update when completions end early: the `logps` and `backward` phases with the option off, off again and on.

    python tools/bench_trim.py                       # bench.py's config 3 workload (qwen2-vl-7b, 32 frames, G 8, C 200, beta 0.04, GA 2)
    python tools/bench_trim.py --C 1024              # the completion length of the reference's downstream scripts
    python tools/bench_trim.py --model qwen2-vl-2b --frames 16

Builds bench.py's Workload (same presets, synthetic clips, seeds, TimeR1_Trainer.optimizer_window loop) once and runs five modes in one process:
"eos / off", "eos / off again" (their spread is the noise), "eos / on", "no eos / off", "no eos / on" (the option must change nothing there beyond that noise).
"eos": after every rollout an EOS is written into each row at a uniform position in [C/8, C/4) (seeded; every mode sees the same positions), the way
`bench.py --ragged-eos` does it - the random-init model never draws the id itself, so the decode loop runs all C - 1 steps in every mode and the rollout
phase is not what this tool measures; its early stop is exercised by the tests.  Per mode: `--warmup` loader windows, then `--windows` timed ones.  Times are
the trainer's HIP-event phase times (the marks `log()` reads) per micro-step; rows = packed rows of the update's forward (P + G*Ct), steps = decode steps
enqueued.  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MODES = (("eos / off", True, False), ("eos / off again", True, False), ("eos / on", True, True), ("no eos / off", False, False), ("no eos / on", False, True))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="qwen2-vl-7b")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--C", type=int, default=200)
    ap.add_argument("--beta", type=float, default=0.04)
    ap.add_argument("--ga", type=int, default=2)
    ap.add_argument("--windows", type=int, default=3, help="timed loader windows per mode")
    ap.add_argument("--warmup", type=int, default=1, help="warm-up loader windows per mode")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_trim: no HIP device (a timing needs the GPU)")
    import time_r1_amd  # noqa: F401
    from time_r1_amd.ops import HipOps
    import bench
    ops = HipOps("cuda:0")
    ops.use_priority_stream()
    bargs = bench.parse_args(["--model", a.model, "--frames", str(a.frames), "--G", str(a.G), "--C", str(a.C), "--beta", str(a.beta), "--ga", str(a.ga)])
    wl = bench.Workload(bargs, ops, torch.device("cuda:0"), 0)
    tr, core, eos = wl.trainer, wl.trainer.core, wl.cfg.eos_token_id
    state = dict(inject=False, rng=None, rows=[], steps=[])
    orig_many, orig_one, orig_logps = core.rollout_many, core.rollout, core.forward_logps

    def inject(states):
        state["steps"].append(core.roll.last_steps_run)
        if not state["inject"]:
            return
        for st in states:
            toks = st.completion_ids.cpu().numpy().copy()
            toks[np.arange(a.G), state["rng"].integers(a.C // 8, max(a.C // 8 + 1, a.C // 4), size=a.G)] = eos
            st.completion_ids = ops.tensor(toks.astype(np.int32), torch.int32)

    def rollout_many(states):
        out = orig_many(states)
        inject(states)
        return out

    def rollout(st):
        out = orig_one(st)
        inject([st])
        return out

    def forward_logps(st, *args, **kw):
        state["rows"].append(int(st.layout.M))
        return orig_logps(st, *args, **kw)
    core.rollout_many, core.rollout, core.forward_logps = rollout_many, rollout, forward_logps
    out = dict(model=a.model, frames=a.frames, G=a.G, C=a.C, beta=a.beta, ga=a.ga, windows=a.windows, warmup=a.warmup, eos="uniform[C/8, C/4) per row, seed 1", modes={})
    for name, with_eos, on in MODES:
        # the option as GRPOConfig(trim_completions=on) sets it up (GRPOCore.__init__)
        core.trim_completions = core.roll.stop_at_eos = core.roll.early_stop = on
        tr.args.trim_completions = tr.args.stop_at_eos = on
        state.update(inject=with_eos, rng=np.random.default_rng(1))
        for _ in range(a.warmup):
            wl.window()
        torch.cuda.synchronize()
        tr._throughput_keys()
        tr.phase_ms_total.clear()
        state["rows"], state["steps"] = [], []
        micro0 = wl.micro
        for _ in range(a.windows):
            wl.window()
        torch.cuda.synchronize()
        tr._throughput_keys()                     # folds any phase marks log() has not read yet into phase_ms_total
        n = wl.micro - micro0
        ph = {k: round(v / n, 2) for k, v in sorted(tr.phase_ms_total.items())}
        out["modes"][name] = dict(micro_steps=n, P=wl.P, rows_per_micro_step=round(float(np.mean(state["rows"])), 1), rows_untrimmed=wl.P + a.G * a.C,
                                  decode_steps=state["steps"], logps_ms=ph.get("logps"), backward_ms=ph.get("backward"), phase_ms_per_micro_step=ph)
    m = out["modes"]
    for k in ("logps_ms", "backward_ms"):
        out[k + "_noise"] = round(abs(m["eos / off"][k] - m["eos / off again"][k]), 2)
    out["peak_hbm_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
