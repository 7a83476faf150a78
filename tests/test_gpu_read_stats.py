"""GPU: the per-read FASTQ statistics plan (EXON_HIP_PLAN_READ_STATS_HIST, kind 9: read length, GC percent, mean quality, four
totals) against tests/read_stats_expect.py, word for word (==): the bare operators over Arrow columns and over views, every launch
form, streams fed from the host and the device, and FASTQ files through exon_hip_stream_consume_scan.

The kernel gives a read to 16 lanes of 16 bytes each, so one step covers W x B = 256 bytes of a line; its length bins live in LDS
up to lmax = 8191 and in global memory beyond.  No load of it reaches outside a line (a partial chunk is fetched as the 16 bytes
that END at the line's end), so it relies on no slack behind a slab or an Arrow buffer: the views tests end the text buffer on the
last line's last byte and surround every line with bytes that would count if they were read."""
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import read_stats_expect as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "fastq")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
WB = 256          # bytes of a line per step of a lane group
LDS_LMAX = 8191   # the largest lmax whose length bins are all in LDS


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def utf8(lines):
    off = np.zeros(len(lines) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lines])
    return off, np.frombuffer(b"".join(lines), np.uint8)


def arrow_dev(ctx, reads):
    so, sd = utf8([s for s, _ in reads])
    qo, qd = utf8([q for _, q in reads])
    return tuple(ctx.to_device(a) for a in (so, sd, qo, qd))


def run_arrow(ctx, reads, lmax):
    so, sd, qo, qd = arrow_dev(ctx, reads)
    d = ctx.zeros(np.int64, E.layout(lmax)[4])
    ctx.read_stats_hist(so, sd, qo, qd, len(reads), lmax, d)
    ctx.sync()
    return d.to_host()


def views_text(reads, base=0, seed=0):
    """Raw text with both lines of every read at a random place: 0 .. 15 filler bytes ('G', 0xFF: they would change every sum)
    in front of each line, `base` of them in front of all; the last quality line ends on the last byte."""
    rng = np.random.default_rng(seed)
    parts, pos, v = [b"G" * base], base, [[], [], [], []]
    for i, (s, q) in enumerate(reads):
        for k, line in ((0, s), (2, q)):
            fill = (b"G\xff" * 8)[:int(rng.integers(0, 16))] if (i or k) else b""
            parts += [fill, line]
            pos += len(fill)
            v[k].append(pos)
            pos += len(line)
            v[k + 1].append(pos)
    return b"".join(parts), [np.array(x, np.int32) for x in v]


def run_views(ctx, reads, lmax, base=0, seed=0):
    text, v = views_text(reads, base, seed)
    assert not reads or v[3][-1] == len(text)
    d_text = ctx.to_device(np.frombuffer(text, np.uint8)) if text else ctx.zeros(np.uint8, 16)
    dv = [ctx.to_device(x) for x in v]
    d = ctx.zeros(np.int64, E.layout(lmax)[4])
    ctx.read_stats_hist_views(d_text, *dv, len(reads), lmax, d)
    ctx.sync()
    return d.to_host()


def both(ctx, reads, lmax):
    want = E.expect(reads, lmax)
    assert np.array_equal(run_arrow(ctx, reads, lmax), want)
    assert np.array_equal(run_views(ctx, reads, lmax, base=len(reads) % 16, seed=len(reads)), want)


def rnd_line(rng, n, alphabet=None):
    if alphabet is None:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def ragged(seed, n, lo=0, hi=180):
    """n reads, sequence and quality lengths drawn independently"""
    rng = np.random.default_rng(seed)
    ls, lq = rng.integers(lo, hi, n), rng.integers(lo, hi, n)
    sb, qb = rnd_line(rng, int(ls.sum()), b"ACGTNacgt"), rng.integers(33, 75, int(lq.sum()), dtype=np.uint8).tobytes()
    so, qo = np.concatenate([[0], np.cumsum(ls)]), np.concatenate([[0], np.cumsum(lq)])
    return [(sb[so[i]:so[i + 1]], qb[qo[i]:qo[i + 1]]) for i in range(n)]


LENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, WB - 1, WB, WB + 1, 2 * WB + 1]


# ---- 1. lengths -------------------------------------------------------------------------------------------------------------------
def test_every_length_alone_and_mixed(ctx):
    rng = np.random.default_rng(1)
    reads = [(rnd_line(rng, n, b"ACGT"), rnd_line(rng, n)) for n in LENS]
    for r in reads:
        both(ctx, [r], 600)
    both(ctx, reads, 600)


def test_sequence_and_quality_lengths_are_independent(ctx):
    rng = np.random.default_rng(2)
    pick = [0, 1, 15, 16, 17, 255, 256, 257, 513]
    reads = [(rnd_line(rng, a, b"GCAT"), rnd_line(rng, b)) for a in pick for b in pick]
    both(ctx, reads, 600)
    both(ctx, [(b"", b"IIII")], 10)
    both(ctx, [(b"GGCA", b"")], 10)
    both(ctx, [(b"", b"")], 1)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 4095, 4097])
def test_read_counts(ctx, n):
    reads = ragged(n, n, 0, 60)
    want = E.expect_fast([s for s, _ in reads], [q for _, q in reads], 64)
    assert np.array_equal(run_arrow(ctx, reads, 64), want)
    assert np.array_equal(run_views(ctx, reads, 64, base=n % 16, seed=n), want)


# ---- 2. alignment -----------------------------------------------------------------------------------------------------------------
def test_views_at_every_alignment(ctx):
    """the text base at each of the 16 alignments; the fillers put every line start at every alignment too (checked)"""
    reads = ragged(5, 400, 0, 300)
    want = E.expect(reads, 300)
    seen = set()
    for base in range(16):
        text, v = views_text(reads, base, seed=base)
        seen |= {int(x) % 16 for x in v[0]} | {int(x) % 16 for x in v[2]}
        assert v[3][-1] == len(text)
        assert np.array_equal(run_views(ctx, reads, 300, base=base, seed=base), want), base
    assert seen == set(range(16))


# ---- 3. byte classes --------------------------------------------------------------------------------------------------------------
def test_all_byte_values_and_near_misses(ctx):
    rng = np.random.default_rng(7)
    every = bytes(range(256))
    reads = [(every, every), (every[::-1] * 2, every * 2), (rng.permutation(np.frombuffer(every * 3, np.uint8)).tobytes(), every)]
    near = [0x42, 0x44, 0x46, 0x48, 0x63, 0x67, 0xC3, 0xC7, 0x00, 0xFF]
    for b in near:
        for gc in (b"G", b"C"):
            for m in range(4):  # a G / C at every position mod 4 inside runs of the near miss
                for n in (5, 16, 19, 64, 67):
                    s = bytearray([b]) * n
                    for i in range(m, n, 4):
                        s[i] = gc[0]
                    reads.append((bytes(s), bytes([b]) * n))
                reads.append((bytes([b]) * 23, b"I" * 23))
    both(ctx, reads, 1024)
    want = E.expect(reads, 1024)
    assert want[2] == sum(E.gc_count(s) for s, _ in reads) > 0


def test_largest_quality_sum(ctx):
    reads = [(b"G", b"\xff" * 65536), (b"C" * 16, b"\xff" * 65535 + b"\xfe"), (b"", b"\xff" * 65536)]
    st = run_arrow(ctx, reads, 100)
    assert np.array_equal(st, E.expect(reads, 100))
    at = E.layout(100)
    assert st[3] == 3 * 65536 * 255 - 1 and st[at[3] + 255] == 2 and st[at[3] + 254] == 1
    assert np.array_equal(run_views(ctx, reads, 100, base=3, seed=3), E.expect(reads, 100))


def test_mean_quality_floor_boundaries(ctx):
    reads = []
    for n in (1, 3, 7, 16, 100, 257, 513):
        for k in (1, 33, 74, 128, 255):
            q = bytearray([k]) * n
            reads.append((b"A" * n, bytes(q)))        # sum = k n      -> bin k
            q[n // 2] = k - 1
            reads.append((b"A" * n, bytes(q)))        # sum = k n - 1  -> bin k - 1
    st = run_arrow(ctx, reads, 600)
    assert np.array_equal(st, E.expect(reads, 600))
    at = E.layout(600)
    for k in (1, 33, 74, 128, 255):
        assert st[at[3] + k] >= 7 and st[at[3] + k - 1] >= 7
    assert np.array_equal(run_views(ctx, reads, 600, base=9, seed=4), st)


def test_gc_percent_floor_boundaries(ctx):
    def seq(gc, n):
        return (b"GC" * n)[:gc] + b"A" * (n - gc)
    cases = [(1, 3, 33), (57, 200, 28), (1, 101, 0), (100, 101, 99), (200, 200, 100), (1, 1, 100), (0, 7, 0), (2, 3, 66), (29, 100, 29)]
    reads = [(seq(gc, n), b"I" * n) for gc, n, _ in cases]
    at = E.layout(256)
    for (gc, n, b), r in zip(cases, reads):
        st = run_arrow(ctx, [r], 256)
        assert st[at[2] + b] == 1 and st[2] == gc, (gc, n)
    both(ctx, reads, 256)


# ---- 4. lmax ----------------------------------------------------------------------------------------------------------------------
GUARD = 64


def guarded_state(ctx, lmax, fill=0):
    n = E.layout(lmax)[4]
    h = np.full(n + 2 * GUARD, 0x5A5A5A5A5A5A5A5A, np.int64)
    h[GUARD:GUARD + n] = fill
    return ctx.to_device(h), n


@pytest.mark.parametrize("lmax", [1, 100, 256, LDS_LMAX, LDS_LMAX + 1])
def test_a_read_of_lmax_bytes_is_counted_and_one_more_is_refused(ctx, lmax):
    rng = np.random.default_rng(lmax)
    ok = [(rnd_line(rng, lmax, b"ACGT"), rnd_line(rng, lmax)), (rnd_line(rng, lmax - 1, b"ACGT"), b"I"), (b"", b"")]
    so, sd, qo, qd = arrow_dev(ctx, ok)
    buf, n = guarded_state(ctx, lmax)
    ctx.read_stats_hist(so, sd, qo, qd, len(ok), lmax, buf.ptr + 8 * GUARD)
    ctx.sync()
    h = buf.to_host()
    want = E.expect(ok, lmax)
    assert np.array_equal(h[GUARD:GUARD + n], want) and want[E.layout(lmax)[1] + lmax] == 1
    assert (h[:GUARD] == 0x5A5A5A5A5A5A5A5A).all() and (h[GUARD + n:] == 0x5A5A5A5A5A5A5A5A).all()
    # lmax + 1 bytes: the status word is raised (reported by the next sync), nothing outside the state is written
    bad = ok + [(rnd_line(rng, lmax + 1, b"ACGT"), b"II")]
    so, sd, qo, qd = arrow_dev(ctx, bad)
    buf, n = guarded_state(ctx, lmax)
    ctx.read_stats_hist(so, sd, qo, qd, len(bad), lmax, buf.ptr + 8 * GUARD)
    with pytest.raises(exon_amd.ExonHipError, match="longer than lmax"):
        ctx.sync()
    ctx.sync()  # reported once
    h = buf.to_host()
    assert (h[:GUARD] == 0x5A5A5A5A5A5A5A5A).all() and (h[GUARD + n:] == 0x5A5A5A5A5A5A5A5A).all()
    assert (h[GUARD:GUARD + n] >= 0).all() and h[GUARD] <= len(bad)


def test_stream_finish_reports_a_read_longer_than_lmax(ctx):
    import pyarrow as pa
    plan = ctx.plan_read_stats_hist(50)
    st = plan.open()
    st.push(pa.record_batch({"s": pa.array([b"ACGT", b"A" * 51], pa.binary()), "q": pa.array([b"IIII", b"I"], pa.binary())}))
    with pytest.raises(exon_amd.ExonHipError, match="longer than lmax"):
        st.finish()
    st.close()
    plan.close()


def test_a_quality_line_beyond_65536_bytes_is_refused(ctx):
    so, sd, qo, qd = arrow_dev(ctx, [(b"ACGT", b"I" * 65537)])
    d = ctx.zeros(np.int64, E.layout(10)[4])
    ctx.read_stats_hist(so, sd, qo, qd, 1, 10, d)
    with pytest.raises(exon_amd.ExonHipError, match="longer than lmax"):
        ctx.sync()


def test_lmax_65536(ctx):
    rng = np.random.default_rng(65536)
    reads = [(rnd_line(rng, n, b"ACGTN"), rnd_line(rng, m)) for n, m in [(65536, 65536), (65535, 1), (8191, 100), (8192, 0), (0, 9), (40000, 8193)]]
    both(ctx, reads, 65536)


def test_argument_checks(ctx):
    so, sd, qo, qd = arrow_dev(ctx, [(b"ACGT", b"IIII")])
    d = ctx.zeros(np.int64, E.layout(10)[4])
    for lmax in (0, 65537):
        with pytest.raises(exon_amd.ExonHipError):
            ctx.read_stats_hist(so, sd, qo, qd, 1, lmax, d)
    with pytest.raises(exon_amd.ExonHipError):
        ctx.read_stats_hist(so, sd, qo, qd, 1, 10, d.ptr + 4)  # misaligned state
    with pytest.raises(exon_amd.ExonHipError):
        ctx.read_stats_hist(so, sd, qo, qd, 1, 10, None)
    with pytest.raises(exon_amd.ExonHipError):
        ctx.read_stats_hist_views(None, so, so, qo, qo, 1, 10, d)
    ctx.read_stats_hist(None, None, None, None, 0, 10, d)  # no reads: nothing happens
    ctx.read_stats_hist_views(None, None, None, None, None, 0, 10, d)
    ctx.sync()
    assert not d.to_host().any()
    with pytest.raises(exon_amd.ExonHipError):
        ctx.plan_read_stats_hist(0)
    with pytest.raises(exon_amd.ExonHipError):
        ctx.plan_read_stats_hist(65537)
    p = ctx.plan_read_stats_hist(151)
    assert (p.n_i64, p.n_f64) == (E.layout(151)[4], 0)
    p.close()


# ---- 5. launch forms --------------------------------------------------------------------------------------------------------------
def cols_of(dev):
    so, sd, qo, qd = dev
    return [(sd, None, so), (qd, None, qo)]


def test_overwrite_accumulate_and_chunks(ctx):
    a, b = ragged(11, 3000, 0, 200), ragged(12, 2500, 0, 200)
    lmax = 200
    ea, eb = E.expect(a, lmax), E.expect(b, lmax)
    da, db, dab = arrow_dev(ctx, a), arrow_dev(ctx, b), arrow_dev(ctx, a + b)
    plan = ctx.plan_read_stats_hist(lmax)
    st = ctx.to_device(np.full(plan.n_i64, 0x7B7B7B7B7B7B7B7B, np.int64))
    plan.launch(cols_of(da), len(a), st, overwrite=True)  # over a dirty state
    ctx.sync()
    assert np.array_equal(st.to_host(), ea)
    plan.launch(cols_of(db), len(b), st)                  # two launches that accumulate = one over the concatenation
    ctx.sync()
    one = ctx.zeros(np.int64, plan.n_i64)
    plan.launch(cols_of(dab), len(a) + len(b), one)
    ctx.sync()
    assert np.array_equal(st.to_host(), ea + eb) and np.array_equal(one.to_host(), ea + eb)
    plan.launch(cols_of(da), 0, st, overwrite=True)       # an overwrite by nothing is the empty state
    ctx.sync()
    assert not st.to_host().any()
    st = ctx.to_device(np.full(plan.n_i64, -3, np.int64))
    plan.launch_chunks([(cols_of(da), len(a)), (cols_of(db), 0), (cols_of(db), len(b))], st, overwrite=True)  # an empty chunk in the middle
    ctx.sync()
    assert np.array_equal(st.to_host(), ea + eb)
    plan.launch_chunks([(cols_of(da), len(a))], st)
    ctx.sync()
    assert np.array_equal(st.to_host(), 2 * ea + eb)
    plan.close()


def test_one_hot_bin(ctx):
    n = 100_000
    s, q = b"GATTACAGATTACAGGC" * 6, b"IIIIHHHHGGGG#" * 8  # 102 / 104 bytes
    so = np.arange(n + 1, dtype=np.int32) * len(s)
    qo = np.arange(n + 1, dtype=np.int32) * len(q)
    dev = tuple(ctx.to_device(x) for x in (so, np.frombuffer(s * n, np.uint8), qo, np.frombuffer(q * n, np.uint8)))
    d = ctx.zeros(np.int64, E.layout(151)[4])
    ctx.read_stats_hist(*dev, n, 151, d)
    ctx.sync()
    want = n * E.expect([(s, q)], 151)
    assert np.array_equal(d.to_host(), want) and np.count_nonzero(want) == 7


def test_fold_states_adds_every_word(ctx):
    lmax = 300
    parts = [E.expect(ragged(20 + i, 500, 0, 300), lmax) for i in range(3)]
    plan = ctx.plan_read_stats_hist(lmax)
    out = ctx.zeros(np.int64, plan.n_i64)
    plan.fold_states(ctx.to_device(np.concatenate(parts)), 3, out)
    ctx.sync()
    assert np.array_equal(out.to_host(), parts[0] + parts[1] + parts[2])
    plan.close()


# ---- 6. streams -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """100 000 reads whose two payloads differ in size by 10 x (short sequences, long quality lines), and their state"""
    rng = np.random.default_rng(31)
    n = 100_000
    ls, lq = rng.integers(0, 12, n), rng.integers(60, 120, n)
    sb, qb = rnd_line(rng, int(ls.sum()), b"ACGT"), rng.integers(33, 75, int(lq.sum()), dtype=np.uint8).tobytes()
    so, qo = np.concatenate([[0], np.cumsum(ls)]), np.concatenate([[0], np.cumsum(lq)])
    seqs, quals = [sb[so[i]:so[i + 1]] for i in range(n)], [qb[qo[i]:qo[i + 1]] for i in range(n)]
    assert 8 * len(sb) < len(qb)
    return seqs, quals, E.expect_fast(seqs, quals, 151)


@pytest.mark.parametrize("rows,coalesce", [(1, None), (8192, None), (100_000, None), (8192, "20000")])
def test_stream_push_host_batches(ctx, big, rows, coalesce, monkeypatch):
    import pyarrow as pa
    if coalesce:
        monkeypatch.setenv("EXON_HIP_COALESCE_ROWS", coalesce)  # several slot flushes: each Utf8 column keeps its own byte count
    seqs, quals, want = big
    n = 300 if rows == 1 else len(seqs)
    if rows == 1:
        want = E.expect_fast(seqs[:n], quals[:n], 151)
    tbl = pa.record_batch({"name": pa.array(np.zeros(n, np.int32)), "sequence": pa.array(seqs[:n], pa.binary()),
                           "quality_scores": pa.array(quals[:n], pa.binary())})
    plan = ctx.plan_read_stats_hist(151, columns=(1, 2))
    st = plan.open()
    for i in range(0, n, rows):
        st.push(tbl.slice(i, rows))  # slices: offset != 0 into both offsets buffers
    counts, sums = st.finish()
    assert np.array_equal(counts, want) and len(sums) == 0
    st.close()
    plan.close()


def test_stream_push_device_and_finish_arrow(ctx):
    reads = ragged(41, 5000, 0, 150)
    want = E.expect(reads, 151)
    so, sd, qo, qd = arrow_dev(ctx, reads)
    plan = ctx.plan_read_stats_hist(151)
    st = plan.open()
    st.push_device([(sd, None, so), (qd, None, qo)], len(reads))
    st.push_device([(sd, None, so), (qd, None, qo)], len(reads))
    arr = st.finish_arrow()
    assert [f.name for f in arr.type] == ["stat", "bin", "count"]
    rows = [(r["stat"], r["bin"], r["count"]) for r in arr.to_pylist()]
    at = E.layout(151)
    exp = [(0, i, int(2 * want[i])) for i in range(4)]
    exp += [(s, w - at[s], int(2 * want[w])) for s in (1, 2, 3) for w in range(at[s], at[s + 1]) if want[w]]
    assert rows == exp and rows == sorted(rows)
    st.close()
    # an empty stream: the four totals rows, all zero, and nothing else
    st = plan.open()
    assert [(r["stat"], r["bin"], r["count"]) for r in st.finish_arrow().to_pylist()] == [(0, i, 0) for i in range(4)]
    st.close()
    plan.close()


# ---- 7. files ---------------------------------------------------------------------------------------------------------------------
def through_scan(ctx, path, gpu_parse, lmax, columns=(2, 3), on_gpu=None):
    scan = exon_amd.Scan(str(path), "fastq", gpu_parse=gpu_parse)
    plan = ctx.plan_read_stats_hist(lmax, columns=columns)
    st = plan.open()
    try:
        rows = st.consume(scan)
        counts, _ = st.finish()
        assert scan.decoded_on_gpu()[0] == (gpu_parse if on_gpu is None else on_gpu)
    finally:
        st.close()
        plan.close()
        scan.close()
    return rows, counts


@pytest.mark.parametrize("name", ["test.fastq", "test.fastq.gz", "test_bgzip.fastq.gz"])
def test_reference_fixtures(ctx, name):
    at = E.layout(512)
    for gpu_parse in (True, False):
        rows, st = through_scan(ctx, os.path.join(FX, name), gpu_parse, 512)
        assert rows == 2 and st[:4].tolist() == [2, 128, 34, 5768]
        assert st[at[1] + 64] == 2 and st[at[2] + 26] == 2 and st[at[3] + 48] == 2 and st.sum() == 2 + 128 + 34 + 5768 + 6
    assert np.array_equal(st, E.expect(E.read_fastq(os.path.join(FX, name)), 512))


def test_views_plan_needs_the_sequence_and_quality_columns(ctx):
    with pytest.raises(exon_amd.ExonHipError, match=r"\(2, 3\)"):
        through_scan(ctx, os.path.join(FX, "test.fastq"), True, 512, columns=(3, 2))


def test_synthetic_file_over_several_slabs(ctx, tmp_path, monkeypatch):
    """300 000 ragged reads, with and without a description, CRLF on some, as plain text and as BGZF over 8 MiB slabs: decoded on
    the device, = the host reader's batches through the staging slots = the expectation."""
    rng = np.random.default_rng(17)
    n = 300_000
    lens = rng.integers(1, 180, n)
    o = np.concatenate([[0], np.cumsum(lens)])
    sb = rnd_line(rng, int(o[-1]), b"ACGTN")
    qb = rng.integers(33, 74, int(o[-1]), dtype=np.uint8).tobytes()
    seqs, quals = [sb[o[i]:o[i + 1]] for i in range(n)], [qb[o[i]:o[i + 1]] for i in range(n)]
    heads = [b"@r%d" % i + (b"", b" lane:%d x y" % (i % 7), b" ")[i % 3] for i in range(n)]
    eols = [b"\r\n" if i % 1000 == 7 else b"\n" for i in range(n)]
    p = tmp_path / "syn.fastq"
    p.write_bytes(b"".join(h + e + s + e + b"+" + e + q + e for h, e, s, q in zip(heads, eols, seqs, quals)))
    gz = str(p) + ".gz"
    subprocess.check_call([BGZIP, str(p), gz, "1"])
    want = E.expect_fast(seqs, quals, 256)
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "8")
    for path in (str(p), gz):
        rows, st = through_scan(ctx, path, True, 256)
        assert rows == n and np.array_equal(st, want), path
    for path in (str(p), gz):  # gpu_parse off is what EXON_HIP_GPU_PARSE=0 makes the CLI open (tests/test_cli_read_stats.py runs that)
        rows, st = through_scan(ctx, path, False, 256)
        assert rows == n and np.array_equal(st, want), path


def test_hand_over_to_the_host_reader_mid_file(ctx, tmp_path, monkeypatch):
    """A .fastq.gz whose first member holds 60 000 reads and whose tail is 3000 one-read members: the device takes the first slabs,
    refuses the run of tiny members, the state is rolled back and the host reader's batches go through exon_hip_stream_push --
    every read once."""
    import gzip
    n1, n2 = 60_000, 3000
    reads = ragged(23, n1 + n2, 20, 60)

    def rec(i):
        return b"@n%d d%d\n" % (i, i) + reads[i][0] + b"\n+\n" + reads[i][1] + b"\n"
    p = tmp_path / "members.fastq.gz"
    with open(p, "wb") as f:
        f.write(gzip.compress(b"".join(rec(i) for i in range(n1)), 6))
        for i in range(n1, n1 + n2):
            f.write(gzip.compress(rec(i), 6))
    monkeypatch.setenv("EXON_HIP_GZ_SLAB_MB", "1")
    rows, st = through_scan(ctx, p, True, 64, on_gpu=False)
    assert rows == n1 + n2
    assert np.array_equal(st, E.expect_fast([s for s, _ in reads], [q for _, q in reads], 64))
