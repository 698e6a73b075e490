"""Microseconds per sampler call at the rollout's decode shape (16 rows x 152 064 bf16 logits, step form, top_k = 50, T = 0.9).

    python tools/bench_sampler.py                      # defaults, top_p = 0.9, min_p = 0.05, repetition_penalty = 1.05 (penalise + sample + mark)
    python tools/bench_sampler.py --lib OTHER.so       # only tr1_sample_tokens_step at the defaults, from another build of the library (an A/B base:
                                                       # it needs just that symbol and tr1_sample_workspace_words, so an older library works)

Each figure: device events around `--calls` back-to-back calls (after `--warmup`), repeated `--repeats` times; median and [min, max] of the
repeats are printed as one JSON line.  The logits stay in place between the calls (an L2 / MALL read, as behind the lm_head launch)."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
I32 = torch.int32


def timed(fn, calls, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / calls)
    out.sort()
    return {"us_median": round(out[len(out) // 2], 2), "us_min": round(out[0], 2), "us_max": round(out[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--vocab", type=int, default=152064)
    ap.add_argument("--top_k", type=int, default=50)
    ap.add_argument("--temperature", type=float, default=0.9)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--lib", default=None, help="another build of libtimer1_hip.so: time its tr1_sample_tokens_step at the defaults only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler: no HIP device (a timing needs the GPU)")
    dev = "cuda:0"
    rows, V = a.rows, a.vocab
    logits = (torch.randn(rows, V, generator=torch.Generator().manual_seed(1)) * 2.5).to(torch.bfloat16).to(dev)
    tokens = torch.zeros(rows, 8, dtype=I32, device=dev)
    step = torch.tensor([1], dtype=I32, device=dev)
    nid = torch.zeros(rows, dtype=I32, device=dev)
    res = {"rows": rows, "vocab": V, "top_k": a.top_k, "temperature": a.temperature, "calls": a.calls, "repeats": a.repeats}
    if a.lib:
        L = ctypes.CDLL(a.lib)
        L.tr1_sample_workspace_words.restype, L.tr1_sample_workspace_words.argtypes = ctypes.c_int64, [ctypes.c_int64]
        c = ctypes
        L.tr1_sample_tokens_step.restype = c.c_int
        L.tr1_sample_tokens_step.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_float, c.c_int64, c.c_uint64, c.c_int64, c.c_uint64, c.c_void_p, c.c_void_p,
                                             c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_int, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p, c.c_int, c.c_void_p, c.c_void_p]      # (the last: done_count, NULL - a build from before that argument ignores it)
        nws = int(L.tr1_sample_workspace_words(rows))
        ws = torch.zeros(nws, dtype=I32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def base():
            rc = L.tr1_sample_tokens_step(logits.data_ptr(), V, rows, V, a.temperature, a.top_k, 1234, 0, 0, step.data_ptr(), tokens.data_ptr(), tokens.stride(0),
                                          None, -1, 0, 0, None, ws.data_ptr(), nws, nid.data_ptr(), 1, stream, None)
            assert rc == 0
        res["lib"] = a.lib
        res["defaults"] = timed(base, a.calls, a.warmup, a.repeats)
        print(json.dumps(res))
        return
    import time_r1_amd  # noqa: F401
    from time_r1_amd.ops import HipOps
    ops = HipOps(dev)
    seen = torch.zeros(rows, ops.seen_words(V), dtype=I32, device=dev)
    ops.mark_seen(seen, V, ids=torch.randint(0, V, (3400,), generator=torch.Generator().manual_seed(2)).to(I32).to(dev))      # a prompt's worth of seen tokens
    pen = torch.empty(rows, V, dtype=torch.bfloat16, device=dev)

    def sample(x=logits, **kw):
        ops.sample_tokens(x, a.temperature, a.top_k, 1234, step, tokens, None, -1, 0, False, next_ids=nid, **kw)

    def penalised():
        sample(ops.penalize_logits(logits, seen, 1.05, out=pen))
        ops.mark_seen(seen, V, tokens=nid)

    for name, fn in (("defaults", sample), ("top_p_0.9", lambda: sample(top_p=0.9)), ("min_p_0.05", lambda: sample(min_p=0.05)),
                     ("repetition_penalty_1.05", penalised), ("all_three", lambda: (sample(ops.penalize_logits(logits, seen, 1.05, out=pen), top_p=0.9, min_p=0.05),
                                                                                   ops.mark_seen(seen, V, tokens=nid)))):
        res[name] = timed(fn, a.calls, a.warmup, a.repeats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
