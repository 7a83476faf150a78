#!/usr/bin/env python3
"""K4 (AVG by group) step time per group count 1 .. 8 and per table size, for ONE build of the library (EXON_HIP_LIB picks it:
tools/build_variant.sh) -- run it once per build, alternating, and compare the lines.  Columns from the device generator
(exon_hip_gen_c4, seed 4), group ids a 2^24-row block of uniform ids repeated over the table, predicate x > 0.01, OVERWRITE
launches through exon_hip_plan_launch, times from exon_hip_timer_* (one event pair around `batch` launches).

    python tools/time_k4_groups.py [rows ...]        (default: 1e9 125e6 1e7 1e6; every size is a prefix of the largest)

Per size and group count: 3 warm-up batches, then 7 timed ones.  One JSON line each."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import exon_amd  # noqa: E402

BLOCK = 1 << 24
REPS, WARMUP = 7, 3


def main():
    sizes = [int(float(a)) for a in sys.argv[1:]] or [10**9, 125 * 10**6, 10**7, 10**6]
    ctx = exon_amd.Context(0)
    rows = (max(sizes) + BLOCK - 1) // BLOCK * BLOCK
    af, av, q, qv, _ = ctx.gen_c4(4, 0, rows)
    gid = ctx.empty(np.int32, rows)
    for G in range(1, 9):
        block = np.random.default_rng(G).integers(0, G, BLOCK, dtype=np.int32)
        for lo in range(0, rows, BLOCK):
            ctx._check(ctx.lib.exon_hip_memcpy_h2d(ctx.h, gid.ptr + 4 * lo, block.ctypes.data, block.nbytes, None))
        ctx.sync()
        plan, st = ctx.plan_cmp_avg_by_group(">", 0.01, G), ctx.zeros(np.int64, 3 * G)
        for n in sizes:
            go = plan.prepared([(af, av, None), (q, qv, None), (gid, None, None)], n, st, overwrite=True)
            batch = max(1, min(50, int(2e8 // n)))
            t = []
            for i in range(WARMUP + REPS):
                ctx.timer_start()
                for _ in range(batch):
                    go()
                ms = ctx.timer_stop_ms() / batch
                if i >= WARMUP:
                    t.append(ms)
            m = statistics.median(t)
            print(json.dumps({"lib": os.path.basename(exon_amd.LIB_PATH), "groups": G, "rows": n, "batch": batch, "median_ms": round(m, 5),
                              "min_ms": round(min(t), 5), "max_ms": round(max(t), 5), "GBps": round(12.25 * n / m / 1e6, 1)}), flush=True)
        plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
