"""GPU: the per-record sequence statistics plan (EXON_HIP_PLAN_SEQ_STATS_HIST, kind 10: totals, byte composition, length, log2 length
and GC percent) against tests/seq_stats_expect.py, word for word (==), in both input forms: Arrow (uploaded Utf8 columns) and views
(text -> exon_hip_fasta_parser_parse -> exon_hip_seq_stats_hist_views); every launch form, streams fed from the host and the device,
and FASTA files through exon_hip_stream_consume_scan.

The kernel divides its work by source bytes in tiles of a power of two, so the tests put records and lines around every power of two
from 16 to 65536 without knowing the tile.  It must load no byte outside the payload / the consumed text: both are surrounded by 'G's,
which would change the totals, the composition and the GC bins if they were read."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import fasta_expect
import seq_stats_expect as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "ref_fixtures")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
EINVAL, EUNSUPPORTED = -1, -4
POWERS = [1 << k for k in range(4, 17)]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parser(ctx):
    p = exon_amd.FASTAParser(ctx, max_slab_bytes=24 << 20)
    yield p
    p.close()


def rnd(rng, n, alphabet=b"ACGTNacgtn"):
    if alphabet is None:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def run_arrow(ctx, seqs, lmax, first=0, odd=0, d_state=None):
    """the Arrow form: values = ['G' x (16 + odd)] ['G' x first] payload ['G' x 64], handed over `16 + odd` bytes in: the first offset is
    `first`, the values pointer sits at `odd` mod 16, and every byte around the payload would count"""
    data = b"".join(seqs)
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    off += first
    d_val = ctx.to_device(np.frombuffer(b"G" * (16 + odd + first) + data + b"G" * 64, np.uint8))
    d_off = ctx.to_device(off)
    d = ctx.zeros(np.int64, E.layout(lmax)[5]) if d_state is None else d_state
    ctx.seq_stats_hist(d_off, d_val.ptr + 16 + odd, len(seqs), lmax, d)
    ctx.sync()
    return d.to_host() if d_state is None else None


def run_views(ctx, parser, text, lmax, final=True, misalign=0, d_state=None):
    """the views form: ['G' x (16 + misalign)] text ['G' x 64] in HBM, parsed as one slab, K10 over the views.  Returns (state, views)"""
    buf = b"G" * (16 + misalign) + text + b"G" * 64
    d_text = ctx.to_device(np.frombuffer(buf, np.uint8))
    v = parser.parse_device(d_text.ptr + 16 + misalign, len(text), final)
    assert v.n_undecided == 0
    d = ctx.zeros(np.int64, E.layout(lmax)[5]) if d_state is None else d_state
    ctx.seq_stats_hist_views(v, lmax, d)
    ctx.sync()
    return (d.to_host() if d_state is None else None), v


def fasta(seqs, width=None, eol=b"\n"):
    """one record per sequence, on one line (width None; an empty sequence has no line) or wrapped at `width`"""
    out = []
    for i, s in enumerate(seqs):
        out.append(b">r%d d" % i + eol)
        if width is None:
            if s:
                out.append(s + eol)
        else:
            out.extend(s[k:k + width] + eol for k in range(0, len(s), width))
    return b"".join(out)


def both(ctx, parser, seqs, lmax, width=None, misalign=0, first=0, odd=0):
    """seqs without '\\n', '\\r' at a line's end or '>' at a line's start go through both forms"""
    want = E.expect_fast(seqs, lmax)
    assert E.identities(want, lmax)
    got = run_arrow(ctx, seqs, lmax, first, odd)
    assert np.array_equal(got, want), ("arrow", np.nonzero(got != want)[0][:8], got[:3], want[:3])
    text = fasta(seqs, width)
    assert E.sequences(text) == list(seqs)
    got, _ = run_views(ctx, parser, text, lmax, True, misalign)
    assert np.array_equal(got, want), ("views", np.nonzero(got != want)[0][:8], got[:3], want[:3])
    return want


# ---- 1. lengths -------------------------------------------------------------------------------------------------------------------
def test_every_length_alone_and_mixed(ctx, parser):
    rng = np.random.default_rng(1)
    seqs = [rnd(rng, n) for n in range(131)]
    for s in seqs:  # every length 0 .. 130 alone, in both forms
        both(ctx, parser, [s], 140)
    both(ctx, parser, seqs, 140)
    both(ctx, parser, seqs, 140, width=7)
    assert np.array_equal(E.expect(seqs, 140), E.expect_fast(seqs, 140))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_record_counts(ctx, parser, n):
    rng = np.random.default_rng(n)
    lens = rng.integers(0, 90, n)
    seqs = [rnd(rng, int(k)) for k in lens]
    both(ctx, parser, seqs, 64, misalign=n % 16, odd=n % 16)


@pytest.mark.parametrize("lmax", [1, 100, 65536])
def test_a_record_of_lmax_bytes_and_one_more(ctx, parser, lmax):
    """lmax + 1 bytes land in the overflow bin: no error"""
    rng = np.random.default_rng(lmax)
    seqs = [rnd(rng, lmax), rnd(rng, lmax + 1), b"", rnd(rng, lmax - 1), rnd(rng, lmax + 1)]
    want = both(ctx, parser, seqs, lmax)
    at = E.layout(lmax)
    assert want[at[2] + lmax] == 1 and want[at[2] + lmax + 1] == 2


# ---- 2. tile edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", POWERS)
def test_records_and_lines_around_a_power_of_two(ctx, parser, P):
    rng = np.random.default_rng(P)
    seqs = [rnd(rng, P - 1), rnd(rng, P), rnd(rng, P + 1), b"", rnd(rng, P), rnd(rng, 3)]
    both(ctx, parser, seqs, 65536 if P > 4096 else 5000)                       # single lines
    both(ctx, parser, seqs, 300, width=60, misalign=P % 13, odd=3, first=P - 1)  # wrapped; the payload starts 1 byte before a multiple of P
    # Arrow: a record that starts 1 byte before a multiple of P, and one that ends 1 byte after (first offset 0, values 16-aligned)
    seqs = [rnd(rng, P - 1), rnd(rng, 2 * P + 2), rnd(rng, 5), rnd(rng, P - 6 + 1), rnd(rng, 40)]
    want = E.expect_fast(seqs, 1000)
    assert np.array_equal(run_arrow(ctx, seqs, 1000), want)
    # views: the same for the text.  A definition line of d bytes in all puts the sequence line at d
    text = b">" + b"x" * (P - 3) + b"\n" + rnd(rng, 2 * P + 1) + b"\n" + b">" + b"y" * (P - 5) + b"\n" + rnd(rng, P + 2) + b"\n>z\nGC\n"
    assert text.index(b"\n") + 1 == P - 1
    got, _ = run_views(ctx, parser, text, 1000)
    assert np.array_equal(got, E.from_text(text, 1000))


def test_a_200000_byte_record_as_one_line_and_wrapped(ctx, parser):
    rng = np.random.default_rng(200000)
    seqs = [rnd(rng, 17), rnd(rng, 200000), rnd(rng, 9)]
    want = both(ctx, parser, seqs, 65536)
    assert want[E.layout(65536)[3] + 18] == 1  # 2^17 <= 200000 < 2^18
    both(ctx, parser, seqs, 65536, width=60, misalign=5, odd=11)


def test_many_records_share_a_tile(ctx, parser):
    rng = np.random.default_rng(5000)
    seqs = [rnd(rng, int(k)) for k in rng.integers(1, 4, 5000)]
    both(ctx, parser, seqs, 10)
    both(ctx, parser, [b""] * 3000 + [b"G"] + [b""] * 3000, 10)  # thousands of empty records at one place


def test_an_empty_record_between_two_spanning_ones(ctx, parser):
    rng = np.random.default_rng(77)
    for n in (1000, 16384, 70000, 150000):
        seqs = [rnd(rng, n), b"", rnd(rng, n + 1)]
        both(ctx, parser, seqs, 100)
        both(ctx, parser, seqs, 100, width=61)


# ---- 3. alignment and guards ------------------------------------------------------------------------------------------------------
def test_views_at_every_alignment(ctx, parser):
    rng = np.random.default_rng(16)
    seqs = [rnd(rng, int(k)) for k in rng.integers(0, 400, 300)]
    text = fasta(seqs, 70)
    want = E.expect_fast(seqs, 512)
    for m in range(16):
        got, v = run_views(ctx, parser, text, 512, misalign=m)
        assert v.first_line_start == m
        assert np.array_equal(got, want), m


def test_arrow_first_offset_and_odd_addresses(ctx):
    rng = np.random.default_rng(17)
    seqs = [rnd(rng, int(k)) for k in rng.integers(0, 400, 300)]
    want = E.expect_fast(seqs, 512)
    for first, odd in [(0, 0), (1, 0), (0, 1), (7, 9), (15, 15), (16, 3), (40000, 5), (33, 8)]:
        assert np.array_equal(run_arrow(ctx, seqs, 512, first, odd), want), (first, odd)


def test_guard_bytes_are_never_counted(ctx, parser):
    """payloads without a single G or C: whatever is loaded from the guards shows up in the totals, the composition and the GC bins"""
    seqs = [b"AT" * 9, b"", b"T" * 31, b"A" * 16, b"N"]
    for first, odd in [(0, 0), (3, 5), (0, 15), (16, 1)]:
        got = run_arrow(ctx, seqs, 64, first, odd)
        assert got[2] == 0 and got[E.layout(64)[1] + ord("G")] == 0 and np.array_equal(got, E.expect(seqs, 64))
    for m in (0, 1, 15):
        got, _ = run_views(ctx, parser, fasta(seqs, 10), 64, misalign=m)
        assert got[2] == 0 and got[E.layout(64)[1] + ord("G")] == 0 and np.array_equal(got, E.expect(seqs, 64))


# ---- 4. bytes ---------------------------------------------------------------------------------------------------------------------
def test_all_byte_values(ctx, parser):
    rng = np.random.default_rng(256)
    every = bytes(range(256))
    seqs = [every, every[::-1] * 2, rng.permutation(np.frombuffer(every * 3, np.uint8)).tobytes()]
    want = E.expect(seqs, 1024)
    assert np.array_equal(run_arrow(ctx, seqs, 1024, 5, 7), want) and (want[3:259] == 6).all()
    # views: every value but '\n'; '>' and '\r' sit in the middle of their lines, where they are sequence bytes
    no_nl = bytes(b for b in range(256) if b != 10)
    lines = [b"A" + no_nl, no_nl[::-1] + b"T", b"AC>G\rT>>\r\rA"]
    text = b">all\n" + b"\n".join(lines) + b"\n>next\n" + lines[0] + b"\n"
    got, _ = run_views(ctx, parser, text, 1024, misalign=9)
    want = E.expect([b"".join(lines), lines[0]], 1024)
    assert np.array_equal(got, want) and want[3 + ord(">")] == 6 and want[3 + 13] == 6
    assert E.sequences(text) == [b"".join(lines), lines[0]]


def test_near_misses_of_g_and_c(ctx, parser):
    seqs = []
    for b in (0x42, 0x44, 0x45, 0x46, 0x48, 0xC3, 0xC7, 0x63, 0x67):
        for gc in b"GC":
            for m in range(4):  # a G / C at every position mod 4 inside runs of the near miss
                for n in (5, 16, 19, 67):
                    s = bytearray([b]) * n
                    for i in range(m, n, 4):
                        s[i] = gc
                    seqs.append(bytes(s))
        seqs.append(bytes([b]) * 23)
    want = both(ctx, parser, seqs, 100)
    assert want[2] == sum(E.gc_count(s) for s in seqs) > 0
    assert np.array_equal(E.expect(seqs, 100), want)


def test_8_mib_of_g(ctx, parser):
    """one hot composition word, gc bin 100"""
    n = 8 << 20
    want = both(ctx, parser, [b"G" * n], 65536, misalign=3, odd=5)
    at = E.layout(65536)
    assert want[:3].tolist() == [1, n, n] and want[at[1] + ord("G")] == n and want[at[4] + 100] == 1 and want[at[3] + 24] == 1
    assert np.count_nonzero(want) == 7


def test_gc_percent_floor_boundaries(ctx, parser):
    def seq(gc, n):
        return (b"GC" * n)[:gc] + b"A" * (n - gc)
    cases = [(1, 3, 33), (57, 200, 28), (1, 101, 0), (100, 101, 99), (200, 200, 100), (1, 1, 100), (0, 7, 0), (2, 3, 66), (29, 100, 29)]
    seqs = [seq(gc, n) for gc, n, _ in cases]
    at = E.layout(256)
    for (gc, n, b), s in zip(cases, seqs):
        st = run_arrow(ctx, [s], 256)
        assert st[at[4] + b] == 1 and st[2] == gc, (gc, n)
        st, _ = run_views(ctx, parser, fasta([s], 13), 256)
        assert st[at[4] + b] == 1 and st[2] == gc, (gc, n)
    both(ctx, parser, seqs, 256)


# ---- 5. the FASTA rules, views form -----------------------------------------------------------------------------------------------
RULES = (b">a one\r\nACGT\r\nGG\nCC\r\n"          # CRLF on some lines
         b">b\nAC\rGT\n"                          # a lone CR mid-line counts
         b">c\nAC\n\n\r\nGT\n\n"                  # empty lines (one of them "\r\n") inside a record
         b">d only empty lines\n\n\n\r\n"
         b">e\n>f\n>g no sequence\r\n"            # definition-only records in the middle
         b">h\nGC>G\n"                            # '>' that is not at a line start
         b">i\nA C\tG T\n>j\n")                   # inner blanks are sequence bytes; a definition-only record at the end


def test_fasta_rules_final_slab(ctx, parser):
    assert E.sequences(RULES) == [b"ACGTGGCC", b"AC\rGT", b"ACGT", b"", b"", b"", b"", b"GC>G", b"A C\tG T", b""]
    for text in (RULES, b">first has nothing\n" + RULES, RULES * 700):
        for m in (0, 7):
            got, v = run_views(ctx, parser, text, 16, True, m)
            assert v.n_records == len(E.sequences(text)) and v.consumed_bytes == len(text)
            assert np.array_equal(got, E.from_text(text, 16)), (len(text), m)


def test_fasta_rules_slab_that_is_not_the_last(ctx, parser):
    """final_slab = 0: the last record and its lines add nothing, consumed_bytes is honoured (what follows is full of G)"""
    for text in (RULES + b">last\nGGGGGGGG\nGGGG\n", RULES * 700 + b">last\n" + b"G" * 40000 + b"\n", RULES + b">last\nGGGG\nGG"):
        want = fasta_expect.slab(text, False)
        got, v = run_views(ctx, parser, text, 16, False, 3)
        assert v.n_records == want["n_records"] and v.consumed_bytes == want["consumed"]
        assert np.array_equal(got, E.from_text(text[:want["consumed"]], 16))
        assert got[0] == want["n_records"] and got[1] == sum(want["seq_len"])
    got, v = run_views(ctx, parser, b">only one\nGGGG\n", 16, False)  # nothing is consumed: nothing is counted
    assert v.n_records == 0 and not got.any()


# ---- 6. the state -----------------------------------------------------------------------------------------------------------------
def ragged(seed, n, hi=300):
    rng = np.random.default_rng(seed)
    return [rnd(rng, int(k)) for k in rng.integers(0, hi, n)]


def cols_of(ctx, seqs):
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return [(ctx.to_device(np.frombuffer(b"".join(seqs) or b"\0", np.uint8)), None, ctx.to_device(off))]


def test_overwrite_accumulate_and_chunks(ctx, parser):
    a, b = ragged(11, 3000), ragged(12, 2500)
    lmax = 200
    ea, eb = E.expect_fast(a, lmax), E.expect_fast(b, lmax)
    da, db, dab = cols_of(ctx, a), cols_of(ctx, b), cols_of(ctx, a + b)
    plan = ctx.plan_seq_stats_hist(lmax)
    assert (plan.n_i64, plan.n_f64) == (E.layout(lmax)[5], 0)
    st = ctx.to_device(np.full(plan.n_i64, 0x7B7B7B7B7B7B7B7B, np.int64))
    plan.launch(da, len(a), st, overwrite=True)  # over a dirty state
    ctx.sync()
    assert np.array_equal(st.to_host(), ea)
    plan.launch(db, len(b), st)                  # two launches that accumulate = one over the concatenation
    ctx.sync()
    one = ctx.zeros(np.int64, plan.n_i64)
    plan.launch(dab, len(a) + len(b), one)
    ctx.sync()
    assert np.array_equal(st.to_host(), ea + eb) and np.array_equal(one.to_host(), ea + eb)
    plan.launch(da, 0, st, overwrite=True)       # an overwrite by nothing is the empty state
    ctx.sync()
    assert not st.to_host().any()
    st = ctx.to_device(np.full(plan.n_i64, -3, np.int64))
    plan.launch_chunks([(da, len(a)), (db, 0), (db, len(b))], st, overwrite=True)  # an empty chunk in the middle
    ctx.sync()
    assert np.array_equal(st.to_host(), ea + eb)
    plan.launch_chunks([(da, len(a))], st)
    ctx.sync()
    assert np.array_equal(st.to_host(), 2 * ea + eb)
    # the views form accumulates on top
    run_views(ctx, parser, fasta(b, 60), lmax, d_state=st)
    assert np.array_equal(st.to_host(), 2 * ea + 2 * eb)
    plan.close()


def test_one_hot_bin(ctx):
    n = 100_000
    s = b"GATTACAGATTACAGGC" * 6
    off = np.arange(n + 1, dtype=np.int32) * len(s)
    d = ctx.zeros(np.int64, E.layout(151)[5])
    ctx.seq_stats_hist(ctx.to_device(off), ctx.to_device(np.frombuffer(s * n, np.uint8)), n, 151, d)
    ctx.sync()
    want = n * E.expect([s], 151)
    assert np.array_equal(d.to_host(), want) and np.count_nonzero(want) == 3 + 4 + 3


def test_fold_states_adds_every_word(ctx):
    lmax = 300
    parts = [E.expect_fast(ragged(20 + i, 500), lmax) for i in range(3)]
    plan = ctx.plan_seq_stats_hist(lmax)
    out = ctx.zeros(np.int64, plan.n_i64)
    plan.fold_states(ctx.to_device(np.concatenate(parts)), 3, out)
    ctx.sync()
    assert np.array_equal(out.to_host(), parts[0] + parts[1] + parts[2])
    plan.close()


@pytest.mark.parametrize("lmax", [1, 2046, 2047, 65536])
def test_nothing_is_written_outside_the_state(ctx, parser, lmax):
    """(2046 / 2047: around the length bins the kernel keeps in LDS)"""
    GUARD, MARK = 64, 0x5A5A5A5A5A5A5A5A
    n = E.layout(lmax)[5]
    rng = np.random.default_rng(lmax)
    seqs = [rnd(rng, k) for k in (0, 1, lmax - 1, lmax, lmax + 1, 2 * lmax + 40000, 2047, 2048, 2049, 70000)]
    want = E.expect_fast(seqs, lmax)
    for form in ("arrow", "views"):
        h = np.full(n + 2 * GUARD, MARK, np.int64)
        h[GUARD:GUARD + n] = 0
        buf = ctx.to_device(h)
        if form == "arrow":
            run_arrow(ctx, seqs, lmax, d_state=buf.ptr + 8 * GUARD)
        else:
            run_views(ctx, parser, fasta(seqs, 80), lmax, d_state=buf.ptr + 8 * GUARD)
        h = buf.to_host()
        assert np.array_equal(h[GUARD:GUARD + n], want), form
        assert (h[:GUARD] == MARK).all() and (h[GUARD + n:] == MARK).all(), form


def test_argument_checks(ctx, parser):
    d = ctx.zeros(np.int64, E.layout(10)[5])
    (val, _, off), = cols_of(ctx, [b"ACGT"])
    for lmax in (0, 65537):
        with pytest.raises(exon_amd.ExonHipError):
            ctx.seq_stats_hist(off, val, 1, lmax, d)
        with pytest.raises(exon_amd.ExonHipError):
            ctx.plan_seq_stats_hist(lmax)
    with pytest.raises(exon_amd.ExonHipError):
        ctx.seq_stats_hist(off, val, 1, 10, d.ptr + 4)  # misaligned state
    with pytest.raises(exon_amd.ExonHipError):
        ctx.seq_stats_hist(off, val, 1, 10, None)
    with pytest.raises(exon_amd.ExonHipError):
        ctx.seq_stats_hist(None, val, 1, 10, d)
    ctx.seq_stats_hist(None, None, 0, 10, d)  # no records: nothing happens
    ctx.seq_stats_hist_views(exon_amd._lib.FASTAViews(), 10, d)
    ctx.sync()
    assert not d.to_host().any()
    assert exon_amd.seq_stats_layout(10) == E.layout(10)


# ---- 7. streams -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(31)
    n = 100_000
    lens = rng.integers(0, 120, n)
    sb = rnd(rng, int(lens.sum()))
    o = np.concatenate([[0], np.cumsum(lens)])
    seqs = [sb[o[i]:o[i + 1]] for i in range(n)]
    return seqs, E.expect_fast(seqs, 151)


@pytest.mark.parametrize("rows,coalesce", [(1, None), (8192, None), (100_000, None), (8192, "20000")])
def test_stream_push_host_batches(ctx, big, rows, coalesce, monkeypatch):
    import pyarrow as pa
    if coalesce:
        monkeypatch.setenv("EXON_HIP_COALESCE_ROWS", coalesce)
    seqs, want = big
    n = 300 if rows == 1 else len(seqs)
    if rows == 1:
        want = E.expect_fast(seqs[:n], 151)
    tbl = pa.record_batch({"id": pa.array(np.zeros(n, np.int32)), "description": pa.array([None] * n, pa.binary()),
                           "sequence": pa.array(seqs[:n], pa.binary())})
    plan = ctx.plan_seq_stats_hist(151, columns=(2,))
    st = plan.open()
    for i in range(0, n, rows):
        st.push(tbl.slice(i, rows))  # slices: offset != 0 into the offsets buffer
    counts, sums = st.finish()
    assert np.array_equal(counts, want) and len(sums) == 0
    st.close()
    plan.close()


def test_stream_push_device_and_finish_arrow(ctx):
    seqs = ragged(41, 5000, 150)
    want = E.expect_fast(seqs, 151)
    cols = cols_of(ctx, seqs)
    plan = ctx.plan_seq_stats_hist(151)
    st = plan.open()
    st.push_device(cols, len(seqs))
    st.push_device(cols, len(seqs))
    arr = st.finish_arrow()
    assert [f.name for f in arr.type] == ["stat", "bin", "count"]
    assert [str(f.type) for f in arr.type] == ["int32", "int32", "int64"]
    rows = [(r["stat"], r["bin"], r["count"]) for r in arr.to_pylist()]
    at = E.layout(151)
    exp = [(0, i, int(2 * want[i])) for i in range(3)]
    exp += [(s, w - at[s], int(2 * want[w])) for s in (1, 2, 3, 4) for w in range(at[s], at[s + 1]) if want[w]]
    assert rows == exp and rows == sorted(rows)
    st.close()
    st = plan.open()  # an empty stream: the three totals rows, all zero, and nothing else
    assert [(r["stat"], r["bin"], r["count"]) for r in st.finish_arrow().to_pylist()] == [(0, i, 0) for i in range(3)]
    st.close()
    plan.close()


# ---- 8. files ---------------------------------------------------------------------------------------------------------------------
def through_scan(ctx, path, gpu_parse, lmax, fmt="fasta", columns=(2,), on_gpu=None):
    scan = exon_amd.Scan(str(path), fmt, gpu_parse=gpu_parse)
    plan = ctx.plan_seq_stats_hist(lmax, columns=columns)
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


@pytest.mark.parametrize("name", ["test.fasta", "test.fasta.gz"])
def test_reference_fixtures(ctx, name):
    at = E.layout(512)
    want = E.from_text(open(os.path.join(FX, "fasta", "test.fasta"), "rb").read(), 512)
    for gpu_parse in (True, False):
        rows, st = through_scan(ctx, os.path.join(FX, "fasta", name), gpu_parse, 512)
        assert rows == 2 and st[:3].tolist() == [2, 8, 4]
        assert all(st[at[1] + b] == 2 for b in b"ACGT") and st[at[2] + 4] == 2 and st[at[3] + 3] == 2 and st[at[4] + 50] == 2
        assert np.array_equal(st, want)


@pytest.fixture(scope="module")
def synthetic():
    """200 000 ragged records: some unwrapped, some at 60 columns, CRLF on some, empty records"""
    rng = np.random.default_rng(2024)
    n = 200_000
    lens = rng.integers(0, 260, n)
    lens[rng.integers(0, n, 2000)] = 0
    sb = rnd(rng, int(lens.sum()), b"ACGTNacgtRYKM")
    o = np.concatenate([[0], np.cumsum(lens)])
    seqs, out = [], []
    for i in range(n):
        s = sb[o[i]:o[i + 1]]
        seqs.append(s)
        eol = b"\r\n" if i % 11 == 5 else b"\n"
        out.append(b">s%d some text" % i + eol)
        if i % 3 == 0:
            if s:
                out.append(s + eol)
        else:
            out.extend(s[k:k + 60] + eol for k in range(0, len(s), 60))
    text = b"".join(out)
    assert len(text) > (20 << 20)
    return text, seqs, E.expect_fast(seqs, 256)


@pytest.mark.parametrize("kind", ["plain", "bgzf", "gzip"])
def test_synthetic_file_over_many_slabs(ctx, tmp_path, monkeypatch, synthetic, kind):
    text, seqs, want = synthetic
    p = tmp_path / "syn.fasta"
    if kind == "gzip":
        p = tmp_path / "syn.fasta.gz"
        p.write_bytes(gzip.compress(text, 1))
    else:
        p.write_bytes(text)
        if kind == "bgzf":
            q = tmp_path / "syn.bgzf.fasta.gz"
            subprocess.check_call([BGZIP, str(p), str(q), "1"], stdout=subprocess.DEVNULL)
            p = q
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    monkeypatch.setenv("EXON_HIP_GZ_SLAB_MB", "1")
    rows, st = through_scan(ctx, p, True, 256)
    assert rows == len(seqs) and np.array_equal(st, want)
    rows, host = through_scan(ctx, p, False, 256)
    assert rows == len(seqs) and np.array_equal(host, st)


def test_no_final_newline(ctx, tmp_path):
    for text in (RULES * 50 + b">last one\nACGT\nAC", RULES * 50 + b">last one"):
        p = tmp_path / "nonl.fasta"
        p.write_bytes(text)
        rows, st = through_scan(ctx, p, True, 16)
        assert rows == len(E.sequences(text)) and np.array_equal(st, E.from_text(text, 16))


def test_a_record_beyond_the_carry_limit_goes_to_the_host_reader(ctx, tmp_path, monkeypatch):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    rng = np.random.default_rng(3)
    seqs = ragged(5, 6000, 400) + [rnd(rng, 3 << 20)] + ragged(6, 6000, 400)
    p = tmp_path / "big.fasta"
    p.write_bytes(fasta(seqs, 70))
    rows, st = through_scan(ctx, p, True, 1000, on_gpu=False)
    assert rows == len(seqs) and np.array_equal(st, E.expect_fast(seqs, 1000))  # every record once


def test_text_in_front_of_the_first_record_goes_to_the_host_reader(ctx, tmp_path):
    p = tmp_path / "front.fasta"
    p.write_bytes(b"GGGG stray text\n" + RULES)
    rows, st = through_scan(ctx, p, True, 16, on_gpu=False)
    assert rows == 10 and np.array_equal(st, E.from_text(RULES, 16))


def test_an_empty_file_gives_the_zero_state(ctx, tmp_path):
    p = tmp_path / "empty.fasta"
    p.write_bytes(b"")
    rows, st = through_scan(ctx, p, True, 16, on_gpu=False)
    assert rows == 0 and not st.any()


def test_the_plan_needs_the_sequence_column(ctx):
    with pytest.raises(exon_amd.ExonHipError, match="column 2") as e:
        through_scan(ctx, os.path.join(FX, "fasta", "test.fasta"), True, 16, columns=(1,))
    assert e.value.code == EINVAL


def test_gpu_parsed_fastq_is_refused_and_host_fastq_works(ctx):
    fq = os.path.join(FX, "fastq", "test.fastq")
    scan = exon_amd.Scan(fq, "fastq", gpu_parse=True)
    plan = ctx.plan_seq_stats_hist(512, columns=(2,))
    st = plan.open()
    with pytest.raises(exon_amd.ExonHipError, match=r"kind 9.*gpu_parse=False") as e:
        st.consume(scan)
    assert e.value.code == EUNSUPPORTED
    counts, _ = st.finish()  # the stream is unchanged
    assert not counts.any()
    st.close()
    plan.close()
    scan.close()
    rows, st = through_scan(ctx, fq, False, 512, fmt="fastq", columns=(2,))
    assert rows == 2 and st[:3].tolist() == [2, 128, 34] and E.identities(st, 512)


def test_other_plans_over_a_gpu_parse_fasta_scan_use_the_host_reader(ctx):
    """as before this plan existed: a FASTA scan opened with gpu_parse under another kind is the host reader's"""
    scan = exon_amd.Scan(os.path.join(FX, "fasta", "test.fasta"), "fasta", gpu_parse=True)
    plan = ctx.plan_qual_pos_hist(16, columns=(2,))
    st = plan.open()
    assert st.consume(scan) == 2 and not scan.decoded_on_gpu()[0]
    counts, _ = st.finish()
    assert counts.sum() == 8
    st.close()
    plan.close()
    scan.close()
