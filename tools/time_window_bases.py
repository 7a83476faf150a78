#!/usr/bin/env python3
"""K13 (bases per fixed-width window, plan kind 13) on resident columns, with K12 over the same windows as a region set and K6 beside it.

  time_window_bases.py [rows=1e8] [out.md | -] [k13]

`rows` reads of 150 bases on a 25-contig genome of GRCh37's lengths (3.1 Gb): the reference and a raw position from the interval
generator (gen_c6), the start folded into [1, L - 149] of the read's contig, end = start + 149, 2 % unmapped; 20.375 B/row.  Once
shuffled (generator order) and once sorted by (reference, start), as a coordinate-sorted BAM has them.  Cases:

  W = 1 000 000   3.1 k windows: K13 in its LDS tier; K12 over the same windows fits its LDS tier too
  W = 1 000       3.1 M windows: K13 in its global tier, all rows.  K12 takes at most 1 048 576 regions: the first that many windows,
                  and the rows that start on them, for BOTH kinds (K13 keeps its whole plan)

Per case one K13, one K12 and one K6 launch ALTERNATE, 7 rounds after a warm-up round, timed with device events; medians, min and
max, the ratios, and the fraction of the box's read probe (exon_hip_read_probe over the three value buffers, this run):
(20.375 B/row * rows / time) / probe rate.  `k13` as a third argument times K13 alone (to compare two builds of the library)."""
import os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exon_amd
rows = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
out = open(sys.argv[2], "w") if len(sys.argv) > 2 and sys.argv[2] != "-" else None
only_k13 = len(sys.argv) > 3 and sys.argv[3] == "k13"
ctx = exon_amd.Context(0)
BPR = 20.375
ROUNDS = 7
READ = 150
MAX_REGIONS = 1 << 20
# GRCh37: chr1 .. chr22, X, Y, MT
LENGTHS = [249250621, 243199373, 198022430, 191154276, 180915260, 171115067, 159138663, 146364022, 141213431, 135534747, 135006516, 133851895,
           115169878, 107349540, 102531392, 90354753, 81195210, 78077248, 59128983, 63025520, 48129895, 51304566, 155270560, 59373566, 16569]
CONTIGS = list(enumerate(LENGTHS))


def say(line=""):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed(fs):
    """the launches of `fs` alternate; -> (median, min, max) of each"""
    for f in fs:
        f()
    ctx.sync()
    t = [[] for _ in fs]
    for _ in range(ROUNDS):
        for k, f in enumerate(fs):
            ctx.timer_start(); f(); t[k].append(ctx.timer_stop_ms())
    ctx.sync()
    return [(statistics.median(x), min(x), max(x)) for x in t]


def windows(W, limit):
    out = []
    for c, ln in CONTIGS:
        for j in range((ln - 1) // W + 1):
            if len(out) == limit:
                return out
            out.append((c, j * W + 1, min((j + 1) * W, ln)))
    return out


say(f"# bases per window: {rows} reads of {READ} bases, {ctx.info()['name']} ({ctx.info()['compute_units']} CUs), WINDOW_BASES_LDS_MAX "
    f"{exon_amd.WINDOW_BASES_LDS_MAX}, REGION_BASES_LDS_MAX {exon_amd.REGION_BASES_LDS_MAX}, {ROUNDS} alternating rounds a case, library {exon_amd.LIB_PATH}")
ref, rv, start, end, pv = ctx.gen_c6(6, 0, rows)
ctx.sync()
h_ref, h_raw = ref.to_host(), start.to_host()
h_rv = np.unpackbits(rv.to_host()[: (rows + 7) // 8], bitorder="little")[:rows].astype(bool)
del ref, rv, start, end, pv
lens = np.array(LENGTHS, np.int64)[np.clip(h_ref, 0, 24)]
h_start = 1 + h_raw % np.maximum(lens - (READ - 1), 1)
h_end = np.minimum(h_start + (READ - 1), lens)
del h_raw, lens


def resident(sel):
    r, s, e, v = h_ref[sel], h_start[sel], h_end[sel], h_rv[sel]
    bits = ctx.to_device(np.concatenate([np.packbits(v, bitorder="little"), np.zeros(64, np.uint8)]))
    return ctx.to_device(r), bits, ctx.to_device(s), ctx.to_device(e), len(r)


key = np.where(h_rv, h_ref.astype(np.int64), -1) * (1 << 32) + np.where(h_rv, h_start, 0)
order = np.argsort(key, kind="stable")
del key
# the rows that start on the first MAX_REGIONS windows of W = 1000 (K12's cap): whole contigs, then a prefix of one
first = windows(1000, MAX_REGIONS)
last_c, _, last_e = first[-1]
on_first = h_rv & ((h_ref < last_c) | ((h_ref == last_c) & (h_start <= last_e)))
orders = {"shuffled (generator order)": np.arange(rows), "sorted by (reference, start)": order}

for label, perm in orders.items():
    for W, sub in [(1_000_000, False), (1000, False), (1000, True)]:
        if sub and only_k13:
            continue
        sel = perm[on_first[perm]] if sub else perm
        c_ref, c_rv, c_start, c_end, n = resident(sel)
        cols = [(c_ref, c_rv, None), (c_start, None, None), (c_end, None, None)]
        gbps, _ = ctx.read_probe([c_ref.ptr, c_start.ptr, c_end.ptr], n * 4)
        floor_ms = BPR * n / (gbps * 1e9) * 1e3
        k13 = ctx.plan_window_bases(CONTIGS, W, columns=(0, 1, 2))
        B = (k13.n_i64 - 4) // 2
        d13 = ctx.zeros(np.int64, k13.n_i64)
        fs = [k13.prepared(cols, n, d13, overwrite=True)]
        regions = None if only_k13 or (B > MAX_REGIONS and not sub) else windows(W, MAX_REGIONS)
        if regions is not None:
            k12 = ctx.plan_region_set_bases(regions, columns=(0, 1, 2))
            d12 = ctx.zeros(np.int64, k12.n_i64)
            fs.append(k12.prepared(cols, n, d12, overwrite=True))
        if not only_k13:
            k6 = ctx.plan_overlap_count(0, 1_000_000, 2_000_000, columns=(0, 1, 2))
            d6 = ctx.zeros(np.int64, 1)
            fs.append(k6.prepared(cols, n, d6, overwrite=True))
        t = timed(fs)
        s13 = d13.to_host()
        b13 = k13.decode(s13)
        assert s13[:4].sum() == n
        line = (f"| {label} | {W} | {B} ({'LDS' if B <= exon_amd.WINDOW_BASES_LDS_MAX else 'global'}) | {n} | {gbps:.0f} | {floor_ms:.3f} | "
                f"{t[0][0]:.3f} | {t[0][1]:.3f} | {t[0][2]:.3f} | {floor_ms / t[0][0]:.2f} | ")
        if regions is not None:
            s12 = d12.to_host()
            assert s12[:4].tolist()[0] <= s13[0] and np.array_equal(k12.decode(s12), b13[:len(regions)])  # the same sums, window for window
            u = (k12.n_i64 - 4) // 4
            line += f"{t[1][0]:.3f} | {t[1][1]:.3f} | {t[1][2]:.3f} | {'LDS' if u <= exon_amd.REGION_BASES_LDS_MAX else 'global'} | {t[0][0] / t[1][0]:.2f} | "
            k12.close()
        else:
            line += "- | - | - | - | - | "
        if not only_k13:
            line += f"{t[-1][0]:.3f} | {t[0][0] / t[-1][0]:.2f} | "
            k6.close()
        else:
            line += "- | - | "
        line += f"{int(s13[0])} rows, {int(b13.sum())} bases |"
        if label == list(orders)[0] and W == 1_000_000:
            say()
            say("| rows | W | windows (K13 tier) | n | probe GB/s | probe ms | K13 ms (median) | min | max | of the probe | K12 ms (median) | min | max | K12 tier | "
                "K13 / K12 | K6 ms | K13 / K6 | counted |")
            say("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        say(line)
        k13.close()
        del c_ref, c_rv, c_start, c_end, d13
