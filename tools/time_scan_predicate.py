#!/usr/bin/env python3
"""A VCF scan's batches from the GPU pipeline (exon_hip_scan_bind_ctx) with and without a pushed-down value predicate: what the device
take-rows step buys over "scan everything, filter above".  project = id, ref, alt, info; cases: no predicate, then `qual >= t` for the
thresholds given (gen_text's QUAL is uniform in [0, 1000): 500 keeps about half, 950 about 5 %, 999 about 0.1 %).  One untimed
pass, then PASSES warm passes per case, cases interleaved; min / median / max seconds, rows out, bytes copied device -> host
(exon_hip_scan_export_stats) and bytes per kept row.  Batches are taken and released without a pyarrow import.
EXON_HIP_PIPE_TRACE=1 makes the library print, per pass, the text kernels' and the take-rows step's share of the export.

    tools/bin/gen_text vcf 30000000 t.vcf && tools/bin/bgzip t.vcf t.vcf.gz 6      # untimed
    tools/time_scan_predicate.py t.vcf.gz [passes=5] [thresholds=500,950,999]"""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exon_amd  # noqa: E402

path = sys.argv[1]
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 5
thresholds = [float(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "500,950,999").split(",")]
REL = C.CFUNCTYPE(None, C.c_void_p)
ctx = exon_amd.Context(0)
cases = [("no predicate", None)] + [(f"qual >= {t:g}", (2, ">=", t)) for t in thresholds]


def one(where):
    t0 = time.perf_counter()
    s = exon_amd.Scan(path, "vcf", info_field="AF", gpu_parse=True, project=("id", "ref", "alt", "info"), where=where).bind_ctx(ctx)
    rows = 0
    while True:
        arr = s.next_raw()
        if arr is None:
            break
        rows += arr.length
        REL(arr.release)(C.addressof(arr))
    dt = time.perf_counter() - t0
    st, on = s.export_stats(), s.decoded_on_gpu()[0]
    s.close()
    assert on, "the host reader took over: not the path this tool times"
    return dt, rows, st


for _, where in cases:  # untimed: buffers, code objects, page cache
    one(where)
times = {name: [] for name, _ in cases}
last = {}
for _ in range(passes):
    for name, where in cases:
        dt, rows, st = one(where)
        times[name].append(dt)
        last[name] = (rows, st)
total = last["no predicate"][0]
print(f"{path}: {total} rows, {passes} warm passes per case, interleaved")
print("| case | rows out | kept | min s | median s | max s | slabs (compacted) | d2h bytes | bytes / kept row |")
print("|---|---|---|---|---|---|---|---|---|")
for name, _ in cases:
    rows, st = last[name]
    t = times[name]
    print(f"| {name} | {rows} | {rows / max(total, 1):.4%} | {min(t):.4f} | {statistics.median(t):.4f} | {max(t):.4f} | {st['slabs']} ({st['compacted_slabs']}) | "
          f"{st['d2h_bytes']} | {st['d2h_bytes'] / max(rows, 1):.1f} |")
