#!/usr/bin/env python3
"""K12 (covered bases per region of a set, plan kind 12) on resident columns, with K11 on the same rows beside it.

  time_region_bases.py [rows=1e8] [out.md | -]

`rows` rows of the interval generator (gen_c6: 25 references ~ GRCh37 lengths, start uniform in [1, 249e6], end = start + up to 20000,
2 % unmapped; 20.375 B/row), once in generator order and once sorted by (reference, start) as a coordinate-sorted BAM has them.  The
region sets are time_region_set.py's (uniform over the 25 references and their coordinates, 10 kb wide): M = 1, 64, the largest M whose
P + C still fits REGION_BASES_LDS_MAX (P = the set's distinct boundaries, about 2 M), 8 regions more (kind 12 in its global tier, kind 11
still in LDS), and 100000 (both in their global tiers).  Per case one kind-12 launch and one kind-11 launch ALTERNATE, 7 rounds after a
warm-up round, timed with device events; medians, min and max, the ratio K12 / K11, and the fraction of the box's read probe
(exon_hip_read_probe over the three value buffers, this run): (20.375 B/row * rows / time) / probe rate."""
import os, statistics, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exon_amd
rows = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
out = open(sys.argv[2], "w") if len(sys.argv) > 2 and sys.argv[2] != "-" else None
ctx = exon_amd.Context(0)
BPR = 20.375
BOUND = exon_amd.REGION_BASES_LDS_MAX
ROUNDS = 7


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


def region_set(m, seed=1):
    rng = np.random.default_rng(seed)
    contig = rng.integers(0, 25, m)
    start = rng.integers(1, 249_000_000, m)
    return [(int(c), int(s), int(s) + 10_000) for c, s in zip(contig, start)]


def units(regions):  # P + C
    pts = {(c, s - 1) for c, s, _ in regions} | {(c, e) for c, _, e in regions}
    return len(pts) + len({c for c, _, _ in regions})


m_edge = BOUND // 2
while units(region_set(m_edge)) > BOUND:
    m_edge -= 1
sizes = [1, 64, m_edge, m_edge + 8, 100_000]

say(f"# covered bases per region: {rows} rows, {ctx.info()['name']} ({ctx.info()['compute_units']} CUs), REGION_BASES_LDS_MAX {BOUND}, "
    f"REGION_SET_LDS_MAX {exon_amd.REGION_SET_LDS_MAX}, {ROUNDS} alternating rounds a case")
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
    say("| M | P + C | K12 tier | K12 ms (median) | min | max | of the probe | K11 tier | K11 ms (median) | min | max | K12 / K11 | counted |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for m in sizes:
        regions = region_set(m)
        k12 = ctx.plan_region_set_bases(regions, columns=(0, 1, 2))
        k11 = ctx.plan_region_set_overlap(regions, columns=(0, 1, 2))
        u = (k12.n_i64 - 4) // 4
        n_contigs = len({r[0] for r in regions})
        t12 = "LDS" if u <= BOUND else "global"
        t11 = "LDS" if m + n_contigs <= exon_amd.REGION_SET_LDS_MAX else "global"
        d12, d11 = ctx.zeros(np.int64, k12.n_i64), ctx.zeros(np.int64, k11.n_i64)
        a, b = timed_pair(k12.prepared(cols, rows, d12, overwrite=True), k11.prepared(cols, rows, d11, overwrite=True))
        s12, s11 = d12.to_host(), d11.to_host()
        assert s12[:4].sum() == rows and s12[:4].tolist() == s11[:4].tolist()
        say(f"| {m} | {u} | {t12} | {a[0]:.3f} | {a[1]:.3f} | {a[2]:.3f} | {floor_ms / a[0]:.2f} | {t11} | {b[0]:.3f} | {b[1]:.3f} | {b[2]:.3f} | "
            f"{a[0] / b[0]:.2f} | {int(s12[0])} rows, {int(k12.decode(s12).sum())} bases |")
        k12.close(); k11.close()
