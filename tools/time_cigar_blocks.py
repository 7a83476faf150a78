#!/usr/bin/env python3
"""exon_hip_cigar_blocks (alignment rows -> aligned block rows, list form) on resident columns, and K12 / K13 / K14 beside it on the
block rows it made.

  time_cigar_blocks.py [rows=1e7] [out.md | -]
  time_cigar_blocks.py slab [rows a slab=1e7] [out.md | -]   the BAM-slab form: what a blocks-mode scan runs per slab (see below)
  time_cigar_blocks.py e2e <file.bam> [pairs=5]      a BAM scan end to end, blocks mode against span mode (see below)
  time_cigar_blocks.py cli <file.bam> <this cli> <another cli> [pairs=5]   span mode, two builds in separate processes (see below)

Two inputs of `rows` rows, 25 references, start uniform in [1, 5e7]:
  DNA-like   one op a row, 150M: one block a row;
  RNA-like   two thirds of the rows 150M, a sixth 75M1000N75M (2 blocks), a sixth 50M500N50M800N50M (3 blocks).
Per input: the whole call (count pass, offsets scan, the copy of the total, fill pass; it is synchronous) between two device events,
median, min and max of 7 after a warm-up; the bytes it must move at the least -- every input read once, every output written once --
and what the two passes move in all (the fill pass reads the inputs again, the counts are written and read); the least as a
fraction of this run's exon_hip_read_probe ceiling.  Then one launch each of kinds 12, 13 and 14 over the block rows, the same way."""
import os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exon_amd

if len(sys.argv) > 1 and sys.argv[1] == "e2e":
    # time_cigar_blocks.py e2e <file.bam> [pairs=5]: a kind-12 plan of 4096 regions over the whole file through
    # exon_hip_stream_consume_scan, blocks mode (ALIGNED) and span mode alternating in this process; the first pair is the warm-up
    #     tools/bin/gen_text bam 20000000 t.u 100 && tools/bin/bgzip t.u t.bam 1      # untimed
    bam, pairs = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5
    ctx = exon_amd.Context(0)
    names = exon_amd.Scan(bam, "bam").dictionary(2)
    rng = np.random.default_rng(2)
    regions = [(names[int(c)], int(s), int(s) + 10_000) for c, s in zip(rng.integers(0, len(names), 4096), rng.integers(1, 200_000_000, 4096))]

    def run(cover):
        plan = ctx.plan_region_set_bases(regions, columns=(2, 3, 4))
        st = plan.open()
        scan = exon_amd.Scan(bam, "bam", gpu_parse=True, cover_ops=cover)
        t = time.perf_counter()
        n = st.consume(scan)
        state, _ = st.finish()
        dt = time.perf_counter() - t
        assert scan.decoded_on_gpu()[0], "the host reader took over: not the path this tool times"
        bases = int(plan.decode(state).sum())
        st.close(); scan.close(); plan.close()
        return dt, n, bases, int(state[:4].sum())
    tb, ts = [], []
    for rep in range(pairs + 1):
        b, s = run("aligned"), run(None)
        assert b[1] == s[1]
        if rep:
            tb.append(b[0]); ts.append(s[0])
        print(f"pass {rep}: blocks {b[0]:.4f} s ({b[3]} block rows, {b[2]} bases), span {s[0]:.4f} s ({s[3]} rows, {s[2]} bases); {b[1]} records", flush=True)
    print(f"blocks: median {statistics.median(tb):.4f} s, min {min(tb):.4f}, max {max(tb):.4f}; span: median {statistics.median(ts):.4f} s, min {min(ts):.4f}, max {max(ts):.4f}; "
          f"blocks - span {1e3 * (statistics.median(tb) - statistics.median(ts)):.1f} ms at the medians, span's own spread {1e3 * (max(ts) - min(ts)):.1f} ms")
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "cli":
    # time_cigar_blocks.py cli <file.bam> <this exon-hip-cli> <another exon-hip-cli> [pairs=5]: span mode, two builds (this tree's and, for
    # instance, the parent commit's CLI beside its own library) in SEPARATE processes, alternating: covered_bases over 4096 regions; wall
    # time of each process (context creation included) and the md5 of the table it prints
    import hashlib, subprocess, tempfile
    bam, clis, pairs = sys.argv[2], sys.argv[3:5], int(sys.argv[5]) if len(sys.argv) > 5 else 5
    names = exon_amd.Scan(bam, "bam").dictionary(2)
    rng = np.random.default_rng(2)
    with tempfile.NamedTemporaryFile("w", suffix=".bed") as bed:
        for c, s in zip(rng.integers(0, len(names), 4096), rng.integers(1, 200_000_000, 4096)):
            bed.write("%s\t%d\t%d\n" % (names[int(c)], int(s) - 1, int(s) + 10_000))
        bed.flush()
        t = {c: [] for c in clis}
        for rep in range(pairs):
            for who, cli in zip(("this", "other"), clis):
                t0 = time.perf_counter()
                r = subprocess.run([cli, "-q", "-c", f"SELECT * FROM covered_bases('{bam}', '{bed.name}')"], capture_output=True, timeout=600, check=True)
                t[cli].append(time.perf_counter() - t0)
                print(f"cli pass {rep} {who} {1e3 * t[cli][-1]:.0f} ms {hashlib.md5(r.stdout).hexdigest()}", flush=True)
    for who, cli in zip(("this", "other"), clis):
        print(f"{who}: median {1e3 * statistics.median(t[cli]):.0f} ms, min {1e3 * min(t[cli]):.0f}, max {1e3 * max(t[cli]):.0f}")
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "slab":
    # time_cigar_blocks.py slab [rows a slab=1e7] [out.md | -]: the BAM-slab form, what a blocks-mode scan runs per slab
    # (exon_hip_bam_parser_cigar_blocks: k_blocks_count<BamSrc>, the offsets scan, k_blocks_fill<BamSrc>, two synchronisations) over a
    # resident slab of records as gen_text writes them (l_seq 100, an 8-byte name: 198 bytes and up, so every other record's ops are
    # unaligned), split by the BAM parser first.  A slab stays below 4 GiB, so 1e8 rows are ten calls back to back over the slab.
    import struct
    per = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10_000_000
    out = open(sys.argv[3], "w") if len(sys.argv) > 3 and sys.argv[3] != "-" else None
    ctx = exon_amd.Context(0)

    def say(line=""):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def rec(ops):
        name = b"read000\0"
        body = struct.pack("<iiBBHHHiiii", 0, 0, len(name), 60, 4680, len(ops), 0, 100, -1, -1, 0) + name + b"".join(struct.pack("<I", v) for v in ops) + bytes(50) + bytes([30] * 100)
        return struct.pack("<i", len(body)) + body

    M, N = 0, 3
    one, two, three = [150 << 4 | M], [75 << 4 | M, 1000 << 4 | N, 75 << 4 | M], [50 << 4 | M, 500 << 4 | N, 50 << 4 | M, 800 << 4 | N, 50 << 4 | M]
    say(f"# aligned blocks, BAM-slab form: slabs of {per} rows, {ctx.info()['name']} ({ctx.info()['compute_units']} CUs), cover_ops ALIGNED (0x181), 7 rounds a case")
    for kind, group in (("DNA-like", [one]), ("RNA-like", [one, one, two, one, one, three])):
        recs = [rec(o) for o in group]
        n = per // len(group) * len(group)
        pat = np.frombuffer(b"".join(recs), np.uint8)
        slab = np.tile(pat, n // len(group)).reshape(n // len(group), len(pat))
        rng = np.random.default_rng(7)
        at = 0
        for r in recs:  # every record its own reference id and position
            slab[:, at + 4:at + 8] = rng.integers(0, 25, len(slab)).astype("<i4").view(np.uint8).reshape(-1, 4)
            slab[:, at + 8:at + 12] = rng.integers(0, 50_000_000, len(slab)).astype("<i4").view(np.uint8).reshape(-1, 4)
            at += len(r)
        n_bytes = slab.size
        d = ctx.to_device(np.concatenate([slab.reshape(-1), np.zeros(64, np.uint8)]))
        del slab
        parser = exon_amd.BAMParser(ctx, 25, n_bytes + 64)
        cols = parser.parse(d, n_bytes)
        assert cols.n_rows == n and cols.n_undecided == 0
        ops = sum(len(o) for o in group) * (n // len(group))
        total = sum((len(o) + 1) // 2 for o in group) * (n // len(group))
        gbps, _ = ctx.read_probe([d.ptr], n_bytes // 4)
        least = n * (4 + 4 + 8 + 24) + 4 * ops + total * 20.125  # rec_of_row, ref_id, start, the header's first 24 bytes, the ops; the block rows
        got = []

        def call():
            got.append(parser.cigar_blocks(d, n_bytes, cols, exon_amd.COVER_ALIGNED)[:2])
        call(); ctx.sync()
        t1, t10, wall = [], [], []
        for _ in range(7):
            w0 = time.perf_counter(); ctx.timer_start(); call(); t1.append(ctx.timer_stop_ms()); wall.append(1e3 * (time.perf_counter() - w0))
        for _ in range(7):
            ctx.timer_start()
            for _ in range(10):
                call()
            t10.append(ctx.timer_stop_ms())
        assert set(got) == {(total, 0)}
        m1, m10 = statistics.median(t1), statistics.median(t10)
        say()
        say(f"## {kind}: {n} records in {n_bytes / 1e6:.0f} MB ({n_bytes / n:.0f} B a record), {ops} ops, {total} block rows; read probe {gbps:.0f} GB/s")
        say()
        say("| step | ms (median) | min | max | host wall ms (median) | bytes at the least | least / time, GB/s | of the probe | slab bytes / time, GB/s |")
        say("|---|---|---|---|---|---|---|---|---|")
        say(f"| one slab, {n} rows | {m1:.3f} | {min(t1):.3f} | {max(t1):.3f} | {statistics.median(wall):.3f} | {least / 1e6:.1f} MB | {least / m1 / 1e6:.0f} | {least / m1 / 1e6 / gbps:.2f} | {n_bytes / m1 / 1e6:.0f} |")
        say(f"| ten slabs back to back, {10 * n} rows | {m10:.3f} | {min(t10):.3f} | {max(t10):.3f} | | {10 * least / 1e6:.1f} MB | {10 * least / m10 / 1e6:.0f} | {10 * least / m10 / 1e6 / gbps:.2f} | {10 * n_bytes / m10 / 1e6:.0f} |")
        parser.close()
        del d
    sys.exit(0)

rows = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
out = open(sys.argv[2], "w") if len(sys.argv) > 2 and sys.argv[2] != "-" else None
ctx = exon_amd.Context(0)
ROUNDS = 7
M, N = 0, 3


def say(line=""):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed(f):
    f(); ctx.sync()
    t = []
    for _ in range(ROUNDS):
        ctx.timer_start(); f(); t.append(ctx.timer_stop_ms())
    ctx.sync()
    return statistics.median(t), min(t), max(t)


def op(n, code):
    return (n << 4) | code


SHAPES = {1: [op(150, M)], 2: [op(75, M), op(1000, N), op(75, M)], 3: [op(50, M), op(500, N), op(50, M), op(800, N), op(50, M)]}


def make(kind, rng):
    """(ref, start, offsets, ops, blocks per row) on the host"""
    ref = rng.integers(0, 25, rows).astype(np.int32)
    start = rng.integers(1, 50_000_000, rows)
    k = np.ones(rows, np.int64) if kind == "DNA-like" else rng.choice([1, 1, 1, 1, 2, 3], rows)
    n_ops = 2 * k - 1
    offsets = np.concatenate([[0], np.cumsum(n_ops)]).astype(np.int32)
    ops = np.empty(int(offsets[-1]), np.uint32)
    for b, shape in SHAPES.items():
        at = offsets[:-1][k == b].astype(np.int64)
        for j, v in enumerate(shape):
            ops[at + j] = v
    return ref, start, offsets, ops, k


say(f"# aligned blocks, list form: {rows} rows, {ctx.info()['name']} ({ctx.info()['compute_units']} CUs), cover_ops ALIGNED (0x181), {ROUNDS} rounds a case")
regions = [(int(c), int(s), int(s) + 199) for c, s in zip(np.random.default_rng(1).integers(0, 25, 40), np.random.default_rng(2).integers(1, 49_000_000, 40))]
contigs = [(c, 60_000_000) for c in range(25)]
for kind in ("DNA-like", "RNA-like"):
    ref, start, offsets, ops, k = make(kind, np.random.default_rng(7))
    total = int(k.sum())
    d_ref, d_start, d_off, d_ops = ctx.to_device(ref), ctx.to_device(start), ctx.to_device(offsets), ctx.to_device(ops)
    o_ref, o_start, o_end, o_valid = ctx.empty(np.int32, total), ctx.empty(np.int64, total), ctx.empty(np.int64, total), ctx.empty(np.uint8, (total + 31) // 32 * 4)
    gbps, _ = ctx.read_probe([d_ref.ptr, d_start.ptr, d_off.ptr], rows * 4)
    least = rows * (4 + 8 + 4) + 4 * len(ops) + total * 20 + total / 8
    moved = rows * (8 + 4 + 4) + 4 * len(ops) + rows * (4 + 8 + 4 + 4) + 4 * len(ops) + total * 20 + 2 * total / 8
    got = []
    t = timed(lambda: got.append(ctx.cigar_blocks(d_ref, None, d_start, None, d_off, d_ops, rows, exon_amd.COVER_ALIGNED, o_ref, o_start, o_end, o_valid, total)))
    assert set(got) == {total}
    h_s, h_e = o_start.to_host(), o_end.to_host()
    assert int((h_e - h_s + 1).sum()) == 150 * rows and np.array_equal(h_s[np.concatenate([[0], np.cumsum(k)[:-1]])], start)
    say()
    say(f"## {kind}: {len(ops)} ops, {total} block rows; read probe {gbps:.0f} GB/s")
    say()
    say("| step | ms (median) | min | max | bytes at the least | bytes the passes move | least / time, GB/s | of the probe |")
    say("|---|---|---|---|---|---|---|---|")
    say(f"| exon_hip_cigar_blocks | {t[0]:.3f} | {t[1]:.3f} | {t[2]:.3f} | {least / 1e6:.1f} MB | {moved / 1e6:.1f} MB | {least / t[0] / 1e6:.0f} | {least / t[0] / 1e6 / gbps:.2f} |")
    cols = [(o_ref, o_valid, None), (o_start, o_valid, None), (o_end, o_valid, None)]
    for name, plan in (("K12, 40 regions", ctx.plan_region_set_bases(regions, columns=(0, 1, 2))), ("K13, W = 1000", ctx.plan_window_bases(contigs, 1000, columns=(0, 1, 2))),
                       ("K14, 40 regions", ctx.plan_region_set_depth(regions, [1, 10], columns=(0, 1, 2)))):
        d = ctx.zeros(np.int64, plan.n_i64)
        t = timed(plan.prepared(cols, total, d, overwrite=True))
        b = total * 20.125
        assert int(d.to_host()[:4].sum()) == total  # every block row is in one of the four classes
        say(f"| {name} on the block rows | {t[0]:.3f} | {t[1]:.3f} | {t[2]:.3f} | {b / 1e6:.1f} MB | | {b / t[0] / 1e6:.0f} | {b / t[0] / 1e6 / gbps:.2f} |")
        plan.close()
    del d_ref, d_start, d_off, d_ops, o_ref, o_start, o_end, o_valid
