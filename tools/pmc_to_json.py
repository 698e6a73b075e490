#!/usr/bin/env python
"""rocprofv3 `--kernel-trace --pmc FETCH_SIZE` database -> profiles/<name>.json: per kernel family the average HBM read bytes per launch
(FETCH_SIZE KiB x 1024 x 2: gfx950 tallies 128-byte requests at 64 B, MI355X_MICROARCH.md HBM section).
Usage: pmc_to_json.py results.db out.json "<note>" """
import json
import re
import sqlite3
import sys
from collections import defaultdict


def family(name):
    n = re.sub(r"^void\s+", "", re.sub(r"\(.*", "", name))
    n = re.sub(r"<.*", "", n)
    return n.strip()


def main():
    db = sqlite3.connect(sys.argv[1])
    rows = db.execute("select name, counter_name, counter_value from pmc_events").fetchall()
    acc = defaultdict(lambda: [0, 0.0])
    for n, c, v in rows:
        if c != "FETCH_SIZE":
            continue
        a = acc[family(n)]
        a[0] += 1
        a[1] += v
    out = {k: {"launches": c, "fetch_bytes_per_launch_corrected": 2.0 * 1024.0 * t / c} for k, (c, t) in sorted(acc.items()) if c and t / c > 1024}
    out["_note"] = sys.argv[3] if len(sys.argv) > 3 else ""
    # fingerprint of the kernel sources this pass measured: bench.py attaches these numbers as `roofline.traffic` only while the sources are
    # unchanged (a kernel edit that alters traffic must not keep quoting the old counters)
    import hashlib, os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "time-r1_amd", "csrc")
    out["_source_sha16"] = {f: hashlib.sha256(open(os.path.join(csrc, f), "rb").read()).hexdigest()[:16] for f in (("gemm.hip", "gemm_skinny.hip", "gemm_pk.hip", "skinny_common.h", "decode.hip", "oproj.hip") + (("gemm_w8.hip",) if any(("_w8" in k or "_f8" in k) for k in out) else ()))}      # (the fp8 twins only when the pass ran them)
    json.dump(out, open(sys.argv[2], "w"), indent=1)
    for k, v in out.items():
        if not k.startswith("_"):
            print("%-40s %7d launches  %10.2f MB/launch" % (k, v["launches"], v["fetch_bytes_per_launch_corrected"] / 1e6))


if __name__ == "__main__":
    main()
