#!/usr/bin/env python3
"""K14 (per-base depth over a region set, plan kind 14) on resident columns, with K12 on the same rows and regions beside it, and the
device reduce beside the copy of the state to the host plus the host decode.

  time_region_depth.py [rows=1e8] [out.md | -]

`rows` rows of the interval generator (gen_c6: 25 references ~ GRCh37 lengths, start uniform in [1, 249e6], end = start + up to 20000,
2 % unmapped; 20.375 B/row), once in generator order and once sorted by (reference, start) as a coordinate-sorted BAM has them.  The
region sets are uniform over the 25 references and their coordinates: 8 targets of 100 bases and 40 of 200 (both in kind 14's LDS
tier: 800 + C and about 8000 + C bins), and an exome-like 200000 targets of 200 bases (about 4e7 bins: the global tier).  Per case one
kind-14 launch and one kind-12 launch ALTERNATE, 7 rounds after a warm-up round, timed with device events; medians, min and max, the
ratio K14 / K12, and the fraction of the box's read probe (exon_hip_read_probe over the three value buffers, this run).  Then, per
case, the reduce (device events, median of 7) against to_host() + decode() of the same state (wall clock, once)."""
import os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exon_amd
rows = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
out = open(sys.argv[2], "w") if len(sys.argv) > 2 and sys.argv[2] != "-" else None
ctx = exon_amd.Context(0)
BPR = 20.375
BOUND = exon_amd.REGION_DEPTH_LDS_MAX
ROUNDS = 7
THR = [1, 10, 20, 30]


def say(line=""):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed_pair(fa, fb):
    """fa and fb alternate; -> ((median, min, max) of fa, of fb)"""
    fa(); fb(); ctx.sync()
    a, b = [], []
    for _ in range(ROUNDS):
        ctx.timer_start(); fa(); a.append(ctx.timer_stop_ms())
        ctx.timer_start(); fb(); b.append(ctx.timer_stop_ms())
    ctx.sync()
    return (statistics.median(a), min(a), max(a)), (statistics.median(b), min(b), max(b))


def region_set(m, width, seed=1):
    rng = np.random.default_rng(seed)
    contig = rng.integers(0, 25, m)
    start = rng.integers(1, 249_000_000, m)
    return [(int(c), int(s), int(s) + width - 1) for c, s in zip(contig, start)]


sets = [(8, 100), (40, 200), (200_000, 200)]

say(f"# per-base depth over a region set: {rows} rows, {ctx.info()['name']} ({ctx.info()['compute_units']} CUs), REGION_DEPTH_LDS_MAX {BOUND}, "
    f"REGION_BASES_LDS_MAX {exon_amd.REGION_BASES_LDS_MAX}, thresholds {THR}, {ROUNDS} alternating rounds a case")
ref, rv, start, end, pv = ctx.gen_c6(6, 0, rows)
ctx.sync()
orders = {"generator order": (ref, rv, start, end, pv)}
# the same rows sorted by (reference, start); NULL references (-1) first
h_ref, h_start, h_end = ref.to_host(), start.to_host(), end.to_host()
h_rv = np.unpackbits(rv.to_host()[: (rows + 7) // 8], bitorder="little")[:rows].astype(bool)
key = np.where(h_rv, h_ref.astype(np.int64), -1) * (1 << 32) + np.where(h_rv, h_start, 0)
order = np.argsort(key, kind="stable")
vbits = np.concatenate([np.packbits(h_rv[order], bitorder="little"), np.zeros(64, np.uint8)])
s_rv = ctx.to_device(vbits)
orders["sorted by (reference, start)"] = (ctx.to_device(h_ref[order]), s_rv, ctx.to_device(h_start[order]), ctx.to_device(h_end[order]), s_rv)
del h_ref, h_start, h_end, key, order

for label, (c_ref, c_rv, c_start, c_end, c_pv) in orders.items():
    cols = [(c_ref, c_rv, None), (c_start, c_pv, None), (c_end, c_pv, None)]
    gbps, probe_ms = ctx.read_probe([c_ref.ptr, c_start.ptr, c_end.ptr], rows * 4)
    floor_ms = BPR * rows / (gbps * 1e9) * 1e3
    say()
    say(f"## {label}: read probe {gbps:.0f} GB/s -> {floor_ms:.3f} ms for {BPR} B/row")
    say()
    say("| M | T + C | intervals | K14 tier | K14 ms (median) | min | max | of the probe | K12 tier | K12 ms (median) | min | max | K14 / K12 | "
        "reduce ms (median) | to_host + decode ms | counted |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for m, width in sets:
        regions = region_set(m, width)
        k14 = ctx.plan_region_set_depth(regions, THR, columns=(0, 1, 2))
        k12 = ctx.plan_region_set_bases(regions, columns=(0, 1, 2))
        nb, n_iv = k14.n_i64 - 4, len(k14.intervals()[0])
        t14 = "global" if nb > BOUND else "LDS" if nb * 8 + n_iv * 16 <= BOUND * 16 else "LDS bins"
        t12 = "LDS" if (k12.n_i64 - 4) // 4 <= exon_amd.REGION_BASES_LDS_MAX else "global"
        d14, d12 = ctx.zeros(np.int64, k14.n_i64), ctx.zeros(np.int64, k12.n_i64)
        a, b = timed_pair(k14.prepared(cols, rows, d14, overwrite=True), k12.prepared(cols, rows, d12, overwrite=True))
        red = []
        k14.reduce(d14); ctx.sync()
        for _ in range(ROUNDS):
            ctx.timer_start(); table = k14.reduce(d14); red.append(ctx.timer_stop_ms())
        ctx.sync()
        t0 = time.perf_counter()
        s14 = d14.to_host()
        bases, ge = k14.decode(s14)
        host_ms = (time.perf_counter() - t0) * 1e3
        s12 = d12.to_host()
        got = table.to_host().reshape(m, 1 + len(THR))
        assert s14[:4].sum() == rows and s14[:4].tolist() == s12[:4].tolist()
        assert np.array_equal(got[:, 0], bases) and np.array_equal(got[:, 1:], ge) and np.array_equal(bases, k12.decode(s12))
        say(f"| {m} | {nb} | {n_iv} | {t14} | {a[0]:.3f} | {a[1]:.3f} | {a[2]:.3f} | {floor_ms / a[0]:.2f} | {t12} | {b[0]:.3f} | {b[1]:.3f} | {b[2]:.3f} | "
            f"{a[0] / b[0]:.2f} | {statistics.median(red):.3f} | {host_ms:.1f} | {int(s14[0])} rows, {int(bases.sum())} bases, ge {ge.sum(axis=0).tolist()} |")
        k14.close(); k12.close()
