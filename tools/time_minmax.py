#!/usr/bin/env python3
"""K4 (AVG by group) and K8 (MIN / MAX by group) on the SAME resident columns, one box, one run: both stream 12.25 B/row, so
K8's step time should sit inside K4's own spread.  Columns come from the device generator (exon_hip_gen_c4), times from the
library's event timer (exon_hip_timer_*): nothing but the library is needed on the GPU machine.

    python tools/time_minmax.py [rows]        (default: the largest 2^24-multiple whose columns take half the HBM, at most 2^32)

Per shape (5, 64 and 4096 groups over the same rows): 3 warm-up launches, then 7 timed launches of each kernel, alternating.
Prints one JSON line per shape and a markdown table.  The group-id column of the 64 / 4096-group shapes is a 2^24-row block of
uniform ids repeated over the table (the 5-group shape keeps the generator's FILTER ids)."""
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
    ctx = exon_amd.Context(0)
    info = ctx.info()
    if len(sys.argv) > 1:
        rows = int(float(sys.argv[1])) // BLOCK * BLOCK
    else:
        rows = min(int(info["hbm_bytes"] * 0.5 / 12.25), 1 << 32) // BLOCK * BLOCK
    rows = max(rows, BLOCK)
    af, av, q, qv, fid = ctx.gen_c4(4, 0, rows)
    ctx.sync()
    gid = ctx.empty(np.int32, rows)
    lib, out = ctx.lib, []

    def step_ms(go):
        ctx.timer_start()
        go()
        return ctx.timer_stop_ms()

    for G in (5, 64, 4096):
        if G == 5:
            ids = fid
        else:
            block = np.random.default_rng(G).integers(0, G, BLOCK, dtype=np.int32)
            for lo in range(0, rows, BLOCK):
                ctx._check(lib.exon_hip_memcpy_h2d(ctx.h, gid.ptr + 4 * lo, block.ctypes.data, block.nbytes, None))
            ctx.sync()
            ids = gid
        cols = [(af, av, None), (q, qv, None), (ids, None, None)]
        k4, k8 = ctx.plan_cmp_avg_by_group(">", 0.01, G), ctx.plan_cmp_minmax_by_group(">", 0.01, G)
        s4, s8 = ctx.zeros(np.int64, 3 * G), ctx.zeros(np.int64, 4 * G)
        go4, go8 = k4.prepared(cols, rows, s4, overwrite=True), k8.prepared(cols, rows, s8, overwrite=True)
        for _ in range(WARMUP):
            go4()
            go8()
        ctx.sync()
        t4, t8 = [], []
        for _ in range(REPS):
            t4.append(step_ms(go4))
            t8.append(step_ms(go8))
        ctx.sync()
        c4, c8 = s4.to_host(), s8.to_host()
        assert np.array_equal(c4[:2 * G], c8[:2 * G]), "K4 and K8 disagree on COUNT(y) / COUNT(*)"
        m4, m8 = statistics.median(t4), statistics.median(t8)
        r = {"groups": G, "rows": rows, "k4_ms": [round(t, 4) for t in t4], "k8_ms": [round(t, 4) for t in t8],
             "k4_median_ms": round(m4, 4), "k8_median_ms": round(m8, 4), "k8_over_k4": round(m8 / m4, 4),
             "k4_GBps": round(12.25 * rows / m4 / 1e6, 1), "k8_GBps": round(12.25 * rows / m8 / 1e6, 1),
             "k8_median_within_k4_spread": bool(min(t4) <= m8 <= max(t4))}
        out.append(r)
        print(json.dumps(r), flush=True)
        k4.close()
        k8.close()
    print(f"\n{info['name']} ({info['compute_units']} CUs), {rows} rows, {REPS} timed launches each after {WARMUP} warm-ups\n")
    print("| groups | K4 median ms (min - max) | K8 median ms (min - max) | K8 / K4 | K4 GB/s | K8 GB/s | K8 median within K4's spread |")
    print("|---|---|---|---|---|---|---|")
    for r in out:
        print(f"| {r['groups']} | {r['k4_median_ms']} ({min(r['k4_ms'])} - {max(r['k4_ms'])}) | {r['k8_median_ms']} ({min(r['k8_ms'])} - {max(r['k8_ms'])}) "
              f"| {r['k8_over_k4']} | {r['k4_GBps']} | {r['k8_GBps']} | {'yes' if r['k8_median_within_k4_spread'] else 'no'} |")
    ctx.close()


if __name__ == "__main__":
    main()
