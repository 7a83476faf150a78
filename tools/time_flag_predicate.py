#!/usr/bin/env python3
"""A BAM scan's batches from the GPU pipeline (exon_hip_scan_bind_ctx) with and without a pushed-down flag / mapping-quality
predicate (exon_hip_scan_set_flag_predicate): what masking and taking the kept rows on the device buys over "scan everything, filter
above".  project = name, cigar, sequence, quality_score.  Cases: no predicate -- the parent commit's way of answering the query, its
caller-side filter NOT included, so a lower bound of that baseline -- then three predicates over gen_text's mix (12 flags equally
likely, three of them unmapped; mapping_quality 2 % NULL, 8 % 0, 12 % 1..29, 20 % 30..59, 58 % 60):
    90   flag & 2048 = 0                                  about 92 % of the rows
    50   flag & 1284 = 0 AND mapping_quality >= 30        about 45 %
    5    flag & 65535 = 16 AND mapping_quality >= 60      about 5 %
One untimed pass, then PASSES warm passes per case, cases interleaved; min / median / max seconds, rows out, quality items out,
bytes copied device -> host (exon_hip_scan_export_stats) and bytes per kept row.  Batches are taken and released without a pyarrow
import.  The box's streaming-read ceiling (exon_hip_read_probe) is printed for the span-copy kernel's share, whose time comes from a
kernel trace of a run of its own.  EXON_HIP_PIPE_TRACE=1 makes the library print, per scan, the take-rows step's share of the export.

    tools/bin/gen_text bam 20000000 t.u && tools/bin/bgzip t.u t.bam 6      # untimed
    tools/time_flag_predicate.py t.bam [passes=5] [cases=none,90,50,5]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exon_amd  # noqa: E402

CASES = {"none": ("no predicate", None), "90": ("flag & 2048 = 0", (2048, 0, -1)), "50": ("flag & 1284 = 0 AND mapq >= 30", (1284, 0, 30)),
         "5": ("flag & 65535 = 16 AND mapq >= 60", (65535, 16, 60))}
path = sys.argv[1]
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cases = [CASES[k] for k in (sys.argv[3] if len(sys.argv) > 3 else "none,90,50,5").split(",")]
REL = C.CFUNCTYPE(None, C.c_void_p)
QUALITY = 8  # the batch's child: five fixed-width columns, name, cigar, sequence, quality_score
ctx = exon_amd.Context(0)


def one(where_flags):
    t0 = time.perf_counter()
    s = exon_amd.Scan(path, "bam", gpu_parse=True, project=("name", "cigar", "sequence", "quality_score"), where_flags=where_flags).bind_ctx(ctx)
    rows = items = 0
    while True:
        arr = s.next_raw()
        if arr is None:
            break
        rows += arr.length
        q = arr.children[QUALITY].contents
        off = C.cast(q.buffers[1], C.POINTER(C.c_int32))
        items += off[q.offset + q.length] - off[q.offset]
        REL(arr.release)(C.addressof(arr))
    dt = time.perf_counter() - t0
    st, on = s.export_stats(), s.decoded_on_gpu()[0]
    s.close()
    assert on, "the host reader took over: not the path this tool times"
    return dt, rows, items, st


d = ctx.zeros(np.uint8, 1 << 30)
gbps, _ = ctx.read_probe([d.ptr], 1 << 30)
del d
for _, where in cases:  # untimed: buffers, code objects, page cache
    one(where)
times = {name: [] for name, _ in cases}
last = {}
for _ in range(passes):
    for name, where in cases:
        dt, rows, items, st = one(where)
        times[name].append(dt)
        last[name] = (rows, items, st)
total = last["no predicate"][0] if "no predicate" in last else 0
print(f"{path}: {total} rows, {passes} warm passes per case, interleaved; exon_hip_read_probe ceiling {gbps:.0f} GB/s")
print("| case | rows out | kept | quality items out | min s | median s | max s | slabs (compacted) | d2h bytes | bytes / kept row |")
print("|---|---|---|---|---|---|---|---|---|---|")
for name, _ in cases:
    rows, items, st = last[name]
    t = times[name]
    kept = f"{rows / total:.4%}" if total else "-"
    print(f"| {name} | {rows} | {kept} | {items} | {min(t):.4f} | {statistics.median(t):.4f} | {max(t):.4f} | {st['slabs']} ({st['compacted_slabs']}) | "
          f"{st['d2h_bytes']} | {st['d2h_bytes'] / max(rows, 1):.1f} |")
