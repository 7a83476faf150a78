#!/usr/bin/env python3
"""K11 (region-set overlap counts, plan kind 11) on resident columns and end to end.

  time_region_set.py [rows=1e8] [e2e_reads=20e6] [out.md | -]

Resident: `rows` rows of the interval generator (gen_c6: 25 references ~ GRCh37 lengths, start uniform in [1, 249e6], end = start +
up to 20000, 2 % unmapped; 20.375 B/row = K6's traffic), once in generator order and once sorted by (reference, start) as a
coordinate-sorted BAM has them.  For M = 1, 64, 4096, 1e5 and 1e6 regions (uniform over the 25 references and their coordinates, 10 kb
wide) one kind-11 launch is timed with device events (median of 7 after a warm-up); beside it K6 (one region) on the same columns and
the box's read probe (exon_hip_read_probe over the three value buffers), all in this run.  The "fraction of the probe" of a launch is
(20.375 B/row * rows / time) / probe rate.  M + C <= REGION_SET_LDS_MAX takes the LDS tier, the rest the global one; M = 6000 and 7000
are timed too: the two sides of the tier bound at nearly the same M.
End to end: a synthetic BAM of `e2e_reads` reads (gen_text, BGZF level 1) through exon_hip_stream_consume_scan -- kind 11 with 4096
named regions against ONE K6 stream over the same file (one region); M K6 passes are that time M-fold, which is an extrapolation."""
import os, statistics, subprocess, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exon_amd
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
rows = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
e2e_reads = int(float(sys.argv[2])) if len(sys.argv) > 2 else 20_000_000
out = open(sys.argv[3], "w") if len(sys.argv) > 3 and sys.argv[3] != "-" else None
ctx = exon_amd.Context(0)
BPR = 20.375


def say(line=""):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed(fn, reps=7):
    fn(); ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.timer_start(); fn(); ms.append(ctx.timer_stop_ms()); ctx.sync()
    return statistics.median(ms), min(ms), max(ms)


def region_set(m, seed=1):
    rng = np.random.default_rng(seed)
    contig = rng.integers(0, 25, m)
    start = rng.integers(1, 249_000_000, m)
    return [(int(c), int(s), int(s) + 10_000) for c, s in zip(contig, start)]


say(f"# region-set overlap counts: {rows} rows, {ctx.info()['name']} ({ctx.info()['compute_units']} CUs), REGION_SET_LDS_MAX {exon_amd.REGION_SET_LDS_MAX}")
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
    k6 = ctx.plan_overlap_count(6, 50_000_000, 100_000_000, columns=(0, 1, 2))
    d1 = ctx.zeros(np.int64, 1)
    k6_ms = timed(k6.prepared(cols, rows, d1, overwrite=True))
    say(f"K6, one region: {k6_ms[0]:.3f} ms (min {k6_ms[1]:.3f}, max {k6_ms[2]:.3f}) = {floor_ms / k6_ms[0]:.2f} of the probe")
    say()
    say("| M | tier | ms (median) | min | max | of the probe | x K6 | M x K6 ms | counted |")
    say("|---|---|---|---|---|---|---|---|---|")
    for m in (1, 8, 64, 4096, 6000, 7000, 100_000, 1_000_000):
        regions = region_set(m)
        plan = ctx.plan_region_set_overlap(regions, columns=(0, 1, 2))
        n_contigs = len({r[0] for r in regions})
        tier = "LDS" if m + n_contigs <= exon_amd.REGION_SET_LDS_MAX else "global"
        d = ctx.zeros(np.int64, plan.n_i64)
        ms = timed(plan.prepared(cols, rows, d, overwrite=True))
        st = d.to_host()
        assert st[:4].sum() == rows
        say(f"| {m} | {tier} | {ms[0]:.3f} | {ms[1]:.3f} | {ms[2]:.3f} | {floor_ms / ms[0]:.2f} | {ms[0] / k6_ms[0]:.2f} | {m * k6_ms[0]:.1f} | {int(plan.decode(st).sum())} hits |")
        plan.close()
    k6.close()

if e2e_reads > 0:
    say()
    say(f"## end to end: a BAM of {e2e_reads} reads, 4096 regions")
    with tempfile.TemporaryDirectory() as tmp:
        ub, bam = os.path.join(tmp, "e2e.ubam"), os.path.join(tmp, "e2e.bam")
        subprocess.check_call([os.path.join(BIN, "gen_text"), "bam", str(e2e_reads), ub, "100"])
        subprocess.check_call([os.path.join(BIN, "bgzip"), ub, bam, "1"])
        os.unlink(ub)
        say(f"{os.path.getsize(bam) / 1e9:.2f} GB of BGZF")
        names = exon_amd.Scan(bam, "bam").dictionary(2)
        rng = np.random.default_rng(2)
        regions = [(names[int(c)], int(s), int(s) + 10_000) for c, s in zip(rng.integers(0, len(names), 4096), rng.integers(1, 200_000_000, 4096))]

        def run(make_plan, prepare=None):
            plan = make_plan()
            st = plan.open()
            if prepare:
                prepare(st)
            scan = exon_amd.Scan(bam, "bam", gpu_parse=True)
            t = time.perf_counter()
            n = st.consume(scan)
            state, _ = st.finish()
            dt = time.perf_counter() - t
            on = scan.decoded_on_gpu()
            st.close(); scan.close()
            return dt, n, state, on, plan
        for rep in range(3):  # alternating, the first pair is the warm-up
            a = run(lambda: ctx.plan_region_set_overlap(regions, columns=(2, 3, 4)))
            b = run(lambda: ctx.plan_overlap_count(0, regions[0][1], regions[0][2]), lambda st: st.set_region_contig(regions[0][0]))
            hits = a[4].decode(a[2])
            assert hits[0] == b[2][0] and a[1] == b[1] == e2e_reads
            say(f"pass {rep}: kind 11, 4096 regions {a[0]:.3f} s (decoded on the GPU {a[3]}); K6, one region {b[0]:.3f} s -> 4096 K6 passes = {4096 * b[0]:.0f} s (extrapolated); "
                f"{int(hits.sum())} hits")
            a[4].close(); b[4].close()
