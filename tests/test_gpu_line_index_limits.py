"""GPU: the line index every text parser shares (gpu_parse.hip: LineIndex -- k_index_lines, k_index_verdict, k_last_newline) and the
framing kernels on top of it, at their limits, through the *Parser.parse_host helpers and against tests/line_index_expect.py and
tests/fasta_expect.py.  Every comparison is exact.  FASTAParser is the direct probe: its line_end IS the index' nl_pos.

What is pinned, by the geometry of k_index_lines (16 bytes a load group, 64 a thread, 4096 a wave, 65536 a tile, 64 tiles a look-back
round):
  * newlines directly in front of, on and behind every such edge, in the first load group and as the slab's last byte; the slab at
    misalign 0, 1, 15 (parse_host pads the front with newlines, which must count for nothing);
  * tiles that publish a count of 0 (one line across three tiles; an unterminated tail of more than a tile) and a tile, every wave
    and every thread of which is full of newlines;
  * CR as the last byte of a thread, a wave and a tile with its LF the first of the next;
  * slabs of 66 and 130 tiles: a second look-back round, also over tiles that contribute 0;
  * one parser over a long slab, a short one, the long one again and a middle one: words of older generations, the tile counter;
  * slabs without any newline, and the slab that is one newline;
  * the line capacities, as observed (read from the code, run on the device):
      FASTQ  max/4 + 8 lines: at the capacity decided, one more line: n_undecided 1, no reads
      FASTA  max/8 + 8 lines: at the capacity decided, one more line: n_undecided 1, no records
      VCF    rows bounded by n_bytes/16 + 1 (n_bytes with the misalignment) and max/16 + 1.  Rows of 16 bytes, the shortest there
             are, stay one below that bound whatever their number, so no well-formed slab reaches it: 256 rows fill a parser of 4096
             bytes and are decided.  A slab reaches the bound only with lines that are no rows -- pinned with blank lines, which are
             undecided by themselves: at the bound the parse returns (n_undecided = the blank lines), one more line fails with EINVAL.
      SAM    n_bytes/12 + 1 and max/12 + 1: as VCF with rows of 12 bytes, but a slab beyond the bound is no error: n_undecided goes
             up by one
      GFF    n_bytes/16 + 1 and max/16 + 1, '#' lines counting: at the bound decided, beyond it n_undecided 1
      BED    n_bytes/8 + 1 and max/8 + 1, '#' lines counting; rows of 6 bytes are well-formed and shorter than the bound assumes:
             five of them are beyond it and handed over (n_undecided 1), never mis-decoded
    and after every refusal the same parser returns a fresh parser's result for a good slab -- with one thing that stays, by design:
    a dictionary (BED reference names here) grows with every slab the parser sees and never takes an id back, so names the
    refused slab's rows brought keep their ids; the good slab's rows have the fresh parser's NAMES, not its ids.
Where the code is right and the first description of these cases was not: a well-formed VCF or SAM slab cannot reach its row bound
(above), so "exactly at the capacity, decided" exists for them only one row below it; adjacent newlines around an edge are empty
lines, which only FASTA takes -- FASTQ gets them with the splitter's verdict checked, VCF one newline an edge in three slabs.
One thing the results cannot show: k_index_lines writes nl_pos[k] only for k < cap; the word behind the buffer belongs to another
allocation of the pool, so a store to nl_pos[cap] changes nothing a caller reads.  The capacity cases pin what can be seen: that a
slab of cap + 1 lines is refused and leaves nothing behind."""
import numpy as np
import pytest

import exon_amd
import fasta_expect
import line_index_expect as E

pytestmark = pytest.mark.gpu
TILE, WAVE, THREAD = E.TILE, E.WAVE, E.THREAD
EINVAL = -1
EDGE_BYTES = 3 * TILE + 1000


# ---- parsers shared by the module (a parser's buffers are sized at its creation) -------------------------------------------------
@pytest.fixture(scope="module")
def fasta(ctx):
    p = exon_amd.FASTAParser(ctx, 9 << 20)  # 130 tiles and a few bytes; 9 MiB / 8 + 8 lines
    yield p
    p.close()


@pytest.fixture(scope="module")
def fastq(ctx):
    p = exon_amd.FASTQParser(ctx, 1 << 20)
    yield p
    p.close()


@pytest.fixture(scope="module")
def vcf(ctx):
    p = exon_amd.VCFParser(ctx, ["1"], max_slab_bytes=1 << 20)
    yield p
    p.close()


# ---- the comparisons ------------------------------------------------------------------------------------------------------------------
def check_fasta(parser, text, final=True, misalign=0):
    got = parser.parse_host(text, final=final, misalign=misalign)
    begin, end, end_nocr = E.lines(text)
    a = np.frombuffer(text, np.uint8)
    is_def = a[begin] == ord(">")
    assert got["n_undecided"] == 0
    assert got["n_lines"] == len(end)
    assert np.array_equal(got["line_end"], end.astype(np.uint32))
    lens = np.where(is_def, 0, end_nocr - begin)
    assert np.array_equal(got["line_dst"], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32))
    want = fasta_expect.slab(text, final)
    assert got["n_records"] == want["n_records"] and got["consumed"] == want["consumed"]
    if final:
        assert got["consumed"] == E.consumed(text)
    assert got["definitions"] == want["definitions"] and got["seq_len"] == want["seq_len"]
    assert got["seq_bytes"] == sum(want["seq_len"])
    return got


VIEWS = ("head_start", "head_end", "seq_start", "seq_end", "qual_start", "qual_end")


def check_fastq(parser, text, final=True, misalign=0, undecided=None):
    got = parser.parse_host(text, final=final, misalign=misalign)
    want = E.fastq_views(text, final)
    assert got["n_reads"] == want["n_reads"] and got["consumed_bytes"] == want["consumed"]
    assert got["n_undecided"] == want["n_undecided"]
    if undecided is not None:
        assert got["n_undecided"] == undecided
    for k in VIEWS:
        assert np.array_equal(got[k], want[k].astype(np.int32)), k
    return got


def check_vcf(parser, text, misalign=0):
    got = parser.parse_host(text, misalign=misalign)
    n = len(E.newlines(text))
    assert got["n_rows"] == n and got["n_undecided"] == 0 and got["consumed_bytes"] == E.consumed(text)
    assert np.array_equal(got["pos"], np.arange(1, n + 1))
    assert np.array_equal(np.unpackbits(got["pos_valid"], bitorder="little")[:n], np.ones(n, np.uint8))
    assert not got["chrom_id"].any()
    return got


def same(a, b):
    """two parse_host results, everything but the device handles"""
    assert a.keys() == b.keys()
    for k in a:
        if k in ("views", "keepalive", "d_text"):
            continue
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


# ---- newlines on every edge ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misalign", [0, 1, 15])
def test_fasta_newlines_on_every_edge(fasta, misalign):
    pos = E.edge_positions(EDGE_BYTES)
    assert len(pos) == 17 and pos[0] < 16 and pos[-1] == EDGE_BYTES - 1
    text = E.with_newlines_at(EDGE_BYTES, pos, "fasta")
    got = check_fasta(fasta, text, True, misalign)
    assert got["line_end"].tolist() == pos and got["n_records"] == 2
    check_fasta(fasta, text, False, misalign)


def test_fastq_newlines_on_every_edge(fastq):
    """The same positions: adjacent newlines are empty lines, which a FASTQ record allows as its sequence and quality line alone --
    the splitter counts the records with an empty header or '+' line as undecided and still writes their views, exactly as
    fastq_views says.  The three slabs below it have one newline an edge and well-formed records only."""
    pos = E.edge_positions(EDGE_BYTES)
    text = E.with_newlines_at(EDGE_BYTES, pos, "fastq", strict=False)
    got = check_fastq(fastq, text, True)
    assert got["n_reads"] == 4 and got["n_undecided"] > 1
    check_fastq(fastq, text, False)
    for d in (-1, 0, 1):
        pos = E.edge_positions(EDGE_BYTES, deltas=(d,), first=5)
        assert len(pos) == 7
        pos += [pos[-1] + 10]  # ... and the second record's quality line, so that every line counts
        text = E.with_newlines_at(pos[-1] + 1, pos, "fastq")
        for misalign in (0, 15):
            got = check_fastq(fastq, text, True, misalign, undecided=0)
            assert got["n_reads"] == 2 and got["consumed_bytes"] == len(text)


def test_vcf_newlines_on_every_edge(vcf):
    """A row is 16 bytes at the least, so the three newlines around an edge are three slabs' (adjacent newlines are blank lines, no
    rows); the first row ends in the first load group's last byte or right behind it."""
    for d in (-1, 0, 1):
        pos = E.edge_positions(EDGE_BYTES, deltas=(d,), first=16 + d)
        assert len(pos) == 6 and (d >= 0 or pos[0] == 15)
        text = E.with_newlines_at(EDGE_BYTES, pos, "vcf")
        for misalign in (0, 1, 15):
            assert check_vcf(vcf, text, misalign)["n_rows"] == 6


# ---- tiles without a newline, and a tile full of them --------------------------------------------------------------------------------------
def test_three_tiles_in_a_row_without_a_newline(fasta):
    pos = [9, 70, 100, 100 + 200_001, 200_200, 200_260, 200_261]
    assert (pos[3] >> 16) - (pos[2] >> 16) == 3  # tiles 1 and 2 hold no newline at all, tile 0 and 3 hold the line's ends
    text = E.with_newlines_at(pos[-1] + 1, pos, "fasta", defs={0, 4})
    assert pos[3] - pos[2] - 1 == 200_000
    got = check_fasta(fasta, text, True)
    assert got["seq_len"][0] == 60 + 29 + 200_000
    check_fasta(fasta, text, False, misalign=15)


def test_an_unterminated_tail_of_more_than_a_tile(fasta):
    pos = [9, 70, 100, 5000]
    text = E.with_newlines_at(pos[-1] + 1 + 70_000, pos, "fasta", defs={0, 2})
    assert (len(text) - 1) >> 16 == 1 and pos[-1] < TILE  # the last tile holds no newline
    got = check_fasta(fasta, text, True)
    assert got["consumed"] == 5001 and got["n_lines"] == 4
    got = check_fasta(fasta, text, False)
    assert got["consumed"] == 71


def test_a_tile_full_of_newlines(fasta):
    run = TILE + WAVE + THREAD + 1
    text = E.dense(TILE, run)
    assert len(text) * 8 <= 9 << 20  # the capacity is not the limit
    got = check_fasta(fasta, text, True)
    n = run + 1
    assert got["n_lines"] == n
    rng = np.random.default_rng(5)
    for k in [0, 1, n - 1] + rng.integers(0, n, 1000).tolist():
        assert got["line_end"][k] == TILE - 1 + k
    assert np.array_equal(got["line_end"], np.arange(TILE - 1, TILE + run, dtype=np.uint32))
    assert got["n_records"] == 1 and got["seq_len"] == [0]
    check_fasta(fasta, text, True, misalign=1)


# ---- CR across an edge ------------------------------------------------------------------------------------------------------------------------
CR_EDGES = [THREAD, 2 * THREAD, 3 * THREAD, 4 * THREAD, WAVE, 2 * WAVE, 3 * WAVE, 4 * WAVE, TILE, 2 * TILE, 3 * TILE, 4 * TILE]


def test_fasta_cr_last_byte_of_a_thread_wave_and_tile(fasta):
    """lines 0, 2, 4, ... are definition lines: both kinds end in a CR that is a thread's, a wave's and a tile's last byte"""
    text = E.with_newlines_at(CR_EDGES[-1] + 1, CR_EDGES, "fasta", crlf=range(12), defs=set(range(0, 12, 2)))
    a = np.frombuffer(text, np.uint8)
    assert all(a[e - 1] == 13 and a[e] == 10 for e in CR_EDGES)
    got = check_fasta(fasta, text, True)
    assert got["n_records"] == 6 and all(not d.endswith(b"\r") for d in got["definitions"])
    assert got["seq_len"] == [CR_EDGES[i] - CR_EDGES[i - 1] - 2 for i in range(1, 12, 2)]
    check_fasta(fasta, text, False, misalign=15)


def test_fastq_cr_last_byte_of_a_thread_wave_and_tile(fastq):
    """lines 0 .. 3, 4 .. 7 and 8 .. 11 end on thread, wave and tile edges: each of the four line kinds on each kind of edge"""
    text = E.with_newlines_at(CR_EDGES[-1] + 1, CR_EDGES, "fastq", crlf=range(12))
    got = check_fastq(fastq, text, True, undecided=0)
    assert got["n_reads"] == 3
    a = np.frombuffer(text, np.uint8)
    for k in ("head_end", "seq_end", "qual_end"):
        assert all(a[e] == 13 and a[e + 1] == 10 for e in got[k])
    check_fastq(fastq, text, False, misalign=15, undecided=0)


# ---- more than 64 tiles: a second look-back round ------------------------------------------------------------------------------------------
def test_66_tiles(fasta):
    n = 66 * TILE
    pos = sorted({t * TILE + (t * 9973 + 11) % TILE for t in range(66)} | {n - 1})
    text = E.with_newlines_at(n, pos, "fasta")
    got = check_fasta(fasta, text, True)
    assert got["n_lines"] == 67 or got["n_lines"] == 66
    check_fasta(fasta, text, False, misalign=1)


def test_130_tiles_with_newlines_in_the_first_and_the_last_alone(fasta):
    n = 130 * TILE
    pos = [5, 90, 300, 129 * TILE + 7, 129 * TILE + 100, n - 1]
    text = E.with_newlines_at(n, pos, "fasta", defs={0, 4})
    got = check_fasta(fasta, text, True)
    assert got["line_end"].tolist() == pos and got["n_records"] == 2
    check_fasta(fasta, text, True, misalign=15)


def test_130_tiles_of_random_line_lengths(fasta):
    rng = np.random.default_rng(130)
    n = 130 * TILE
    pos = np.cumsum(rng.integers(2, 3002, n // 1400)).astype(np.int64)
    pos = pos[pos < n - 1].tolist() + [n - 1]
    assert pos[-2] > 128 * TILE and len(pos) > 5000
    text = E.with_newlines_at(n, pos, "fasta")
    got = check_fasta(fasta, text, True)
    assert got["n_lines"] == len(pos)
    check_fasta(fasta, text, False)


# ---- one parser, slabs of different lengths one after the other ----------------------------------------------------------------------------
def slab_of_tiles(seed, tiles, fmt):
    rng = np.random.default_rng(seed)
    n = tiles * TILE - 100 * seed
    least = 40 if fmt == "vcf" else 2
    pos = np.cumsum(rng.integers(least, 700, n // 300)).astype(np.int64)
    pos = pos[pos < n - 50].tolist() + [n - 1]
    return E.with_newlines_at(n, pos, fmt)


def test_fasta_parser_reuse_long_short_long_middle(ctx):
    slabs = {"A": slab_of_tiles(1, 5, "fasta"), "B": slab_of_tiles(2, 1, "fasta"), "C": slab_of_tiles(3, 3, "fasta")}
    fresh = {}
    for name, text in slabs.items():
        p = exon_amd.FASTAParser(ctx, 1 << 20)
        fresh[name] = check_fasta(p, text, True)
        p.close()
    p = exon_amd.FASTAParser(ctx, 1 << 20)
    try:
        for name in "ABAC":
            same(check_fasta(p, slabs[name], True), fresh[name])
    finally:
        p.close()


def test_fasta_parser_reuse_many_tiles_of_other_content(ctx):
    """40 and 24 tiles in turn, other newlines in every tile: a look-back word an earlier slab left (an inclusive count, flag 2) would
    be taken by the tile behind it whenever that tile looks before its new neighbour has published -- a coin a tile, 100 tiles"""
    slabs = {"A": slab_of_tiles(4, 40, "fasta"), "B": slab_of_tiles(5, 1, "fasta"), "C": slab_of_tiles(6, 24, "fasta")}
    p = exon_amd.FASTAParser(ctx, 40 * TILE)
    try:
        for name in "ABACA":
            check_fasta(p, slabs[name], True)
    finally:
        p.close()


def test_vcf_parser_reuse_long_short_long_middle(ctx):
    slabs = {"A": slab_of_tiles(1, 5, "vcf"), "B": slab_of_tiles(2, 1, "vcf"), "C": slab_of_tiles(3, 3, "vcf")}
    fresh = {}
    for name, text in slabs.items():
        p = exon_amd.VCFParser(ctx, ["1"], max_slab_bytes=1 << 20)
        fresh[name] = check_vcf(p, text)
        p.close()
    p = exon_amd.VCFParser(ctx, ["1"], max_slab_bytes=1 << 20)
    try:
        for name in "ABAC":
            same(check_vcf(p, slabs[name]), fresh[name])
    finally:
        p.close()


# ---- no newline at all, and the shortest slabs -----------------------------------------------------------------------------------------------
def tabular_parsers(ctx, max_bytes):
    return {"vcf": exon_amd.VCFParser(ctx, ["1"], max_slab_bytes=max_bytes), "sam": exon_amd.SAMParser(ctx, [], max_slab_bytes=max_bytes),
            "gff": exon_amd.GFFParser(ctx, max_slab_bytes=max_bytes), "bed": exon_amd.BEDParser(ctx, max_slab_bytes=max_bytes)}


@pytest.fixture(scope="module")
def roomy(ctx):
    """every parser at 128 KiB"""
    ps = tabular_parsers(ctx, 1 << 17)
    ps["fasta"] = exon_amd.FASTAParser(ctx, 1 << 17)
    ps["fastq"] = exon_amd.FASTQParser(ctx, 1 << 17)
    yield ps
    for p in ps.values():
        p.close()


@pytest.mark.parametrize("n", [1, 15, 16, 17, 65537])
def test_slabs_without_a_newline(roomy, n):
    """nothing is a line yet: no line, no read, no row, nothing consumed and nothing undecided, in the last slab as in any other (the
    statement: fastq_views counts an unfinished record of a final slab by its LINES, and there is none)"""
    for fmt in E.FORMATS:
        text = E.with_newlines_at(n, [], fmt)
        assert b"\n" not in text and len(text) == n
        for misalign in (0, 15):
            if fmt == "fasta":
                for final in (True, False):
                    got = roomy[fmt].parse_host(text, final=final, misalign=misalign)
                    assert (got["n_lines"], got["n_records"], got["consumed"], got["n_undecided"]) == (0, 0, 0, 0), (fmt, final)
            elif fmt == "fastq":
                for final in (True, False):
                    got = check_fastq(roomy[fmt], text, final, misalign, undecided=0)
                    assert (got["n_reads"], got["consumed_bytes"]) == (0, 0), (fmt, final)
            else:
                got = roomy[fmt].parse_host(text, misalign=misalign)
                assert (got["n_rows"], got["consumed_bytes"], got["n_undecided"]) == (0, 0, 0), fmt
                assert E.consumed(text) == 0


def test_the_slab_that_is_one_newline(roomy):
    """one empty line.  FASTA: a first line without '>' is undecided, nothing comes back.  FASTQ: no record; the last slab counts the
    line that is left over (fastq_views).  The tabular parsers: one row, undecided (a blank line is no record), one byte consumed."""
    for misalign in (0, 15):
        for final in (True, False):
            got = roomy["fasta"].parse_host(b"\n", final=final, misalign=misalign)
            assert (got["n_lines"], got["n_records"], got["consumed"], got["n_undecided"]) == (0, 0, 0, 1)
            got = check_fastq(roomy["fastq"], b"\n", final, misalign, undecided=1 if final else 0)
            assert (got["n_reads"], got["consumed_bytes"]) == (0, 0)
        for fmt in ("vcf", "sam", "gff", "bed"):
            got = roomy[fmt].parse_host(b"\n", misalign=misalign)
            assert (got["n_rows"], got["consumed_bytes"], got["n_undecided"]) == (1, 1, 1), fmt


# ---- the line capacities --------------------------------------------------------------------------------------------------------------------
SMALL = 4096


def test_fastq_line_capacity(ctx):
    cap = SMALL // 4 + 8
    assert cap % 4 == 0
    whole = b"@\n\n+\n\n" * (cap // 4)  # the shortest record there is: four lines in six bytes
    good = b"@a b\nACGT\n+\nIIII\n" * 5
    fresh = exon_amd.FASTQParser(ctx, SMALL)
    want_good = check_fastq(fresh, good, True, undecided=0)
    fresh.close()
    p = exon_amd.FASTQParser(ctx, SMALL)
    try:
        for misalign in (0, 15):
            got = check_fastq(p, whole, True, misalign, undecided=0)
            assert got["n_reads"] == cap // 4 and got["consumed_bytes"] == len(whole)
            for final in (False, True):
                got = p.parse_host(whole + b"@\n", final=final, misalign=misalign)  # cap + 1 lines
                assert (got["n_reads"], got["n_undecided"], got["consumed_bytes"]) == (0, 1, 0)
                same(check_fastq(p, good, True, undecided=0), want_good)
    finally:
        p.close()


def test_fasta_line_capacity(ctx):
    cap = SMALL // 8 + 8
    good = b">a b\nACGT\nAC\n>c\n\nA\n"
    fresh = exon_amd.FASTAParser(ctx, SMALL)
    want_good = check_fasta(fresh, good, True)
    fresh.close()
    p = exon_amd.FASTAParser(ctx, SMALL)
    try:
        for misalign in (0, 15):
            text = E.dense(3, cap - 1)
            got = check_fasta(p, text, True, misalign)
            assert got["n_lines"] == cap and got["line_end"][-1] == len(text) - 1
            check_fasta(p, text, False, misalign)
            for final in (False, True):
                got = p.parse_host(text + b"\n", final=final, misalign=misalign)  # cap + 1 lines
                assert (got["n_lines"], got["n_records"], got["n_undecided"], got["consumed"]) == (0, 0, 1, 0)
                same(check_fasta(p, good, True), want_good)
    finally:
        p.close()


def vcf_rows(k):
    """k rows of 16 bytes, POS 1 .. 9 in turn"""
    return b"".join(b"1\t%d\t.\tA\tC\t.\t.\t.\n" % (i % 9 + 1) for i in range(k))


def test_vcf_row_bound(ctx):
    """n_bytes / 16 + 1 rows, n_bytes with the misalignment; beyond it exon_hip_vcf_parser_parse fails with EINVAL"""
    good = E.with_newlines_at(400, [40, 99, 170, 399], "vcf")
    fresh = exon_amd.VCFParser(ctx, ["1"], max_slab_bytes=SMALL)
    want_good = check_vcf(fresh, good)
    fresh.close()
    p = exon_amd.VCFParser(ctx, ["1"], max_slab_bytes=SMALL)
    try:
        def decided(k, misalign):
            got = p.parse_host(vcf_rows(k), misalign=misalign)
            assert (got["n_rows"], got["n_undecided"], got["consumed_bytes"]) == (k, 0, 16 * k)
            assert np.array_equal(got["pos"], np.arange(k) % 9 + 1)

        def blank(k, n_blank, misalign):
            got = p.parse_host(vcf_rows(k) + b"\n" * n_blank, misalign=misalign)
            assert (got["n_rows"], got["n_undecided"], got["consumed_bytes"]) == (k + n_blank, n_blank, 16 * k + n_blank)
            assert np.array_equal(got["pos"][:k], np.arange(k) % 9 + 1)

        def refused(k, n_blank, misalign):
            with pytest.raises(exon_amd.ExonHipError) as e:
                p.parse_host(vcf_rows(k) + b"\n" * n_blank, misalign=misalign)
            assert e.value.code == EINVAL and "more than its byte size allows" in str(e.value)
            same(check_vcf(p, good), want_good)

        decided(256, 0)   # the parser's 4096 bytes, one row below max / 16 + 1 = 257: the most well-formed text reaches
        decided(255, 15)
        for k in (1, 7, 100):
            decided(k, 0)
            blank(k, 1, 0)     # k + 1 lines in 16 k + 1 bytes: the bound
            refused(k, 2, 0)   # ... and one beyond it
            blank(k, 2, 15)    # 15 bytes of misalignment move the bound by one line
            refused(k, 3, 15)
        refused(254, 18, 0)    # 272 lines, more than the index holds (257) and than 4082 bytes allow (256)
        with pytest.raises(exon_amd.ExonHipError) as e:  # (4096 + 15 bytes: the slab itself is beyond the parser, another refusal)
            p.parse_host(vcf_rows(256), misalign=15)
        assert e.value.code == EINVAL and "exceeds the parser's" in str(e.value)
        same(check_vcf(p, good), want_good)
    finally:
        p.close()


def sam_rows(k):
    """k rows of 12 bytes: the six fields the device layout reads, POS 1 .. 9 in turn"""
    return b"".join(b"r\t0\t*\t%d\t0\t*\n" % (i % 9 + 1) for i in range(k))


def test_sam_row_bound(ctx):
    """n_bytes / 12 + 1 rows, n_bytes with the misalignment; beyond it n_undecided goes up by one.  parse_host brings back the
    rows the buffers hold even where n_rows says more."""
    good = E.with_newlines_at(400, [40, 99, 170, 399], "sam")
    fresh = exon_amd.SAMParser(ctx, [], max_slab_bytes=SMALL)
    want_good = fresh.parse_host(good)
    assert (want_good["n_rows"], want_good["n_undecided"], want_good["consumed_bytes"]) == (4, 0, 400)
    assert want_good["start"].tolist() == [1, 2, 3, 4]
    fresh.close()
    p = exon_amd.SAMParser(ctx, [], max_slab_bytes=SMALL)
    max_rows = SMALL // 12 + 1
    try:
        def run(k, n_blank, misalign, undecided):
            got = p.parse_host(sam_rows(k) + b"\n" * n_blank, misalign=misalign)
            assert (got["n_rows"], got["n_undecided"]) == (k + n_blank, undecided), (k, n_blank, misalign)
            assert len(got["start"]) == min(k + n_blank, max_rows)
            assert np.array_equal(got["start"][:k], np.arange(k) % 9 + 1)
            if k + n_blank <= max_rows:
                assert got["consumed_bytes"] == 12 * k + n_blank
            else:
                assert got["consumed_bytes"] == 0  # (the index was cut short: its last entry is not the last newline)
            if undecided:
                same(p.parse_host(good), want_good)

        run(341, 0, 0, 0)      # 4092 bytes, one row below max / 12 + 1 = 342
        run(340, 0, 15, 0)
        for k in (1, 7, 100):
            run(k, 0, 0, 0)
            run(k, 1, 0, 1)    # k + 1 lines in 12 k + 1 bytes: the bound; the blank line is undecided by itself
            run(k, 2, 0, 2)    # one line beyond the bound: the line is not looked at, the slab counts one more
            run(k, 2, 15, 2)   # 12 k + 17 bytes: the bound is k + 2, both blank lines are looked at
            run(k, 3, 15, 3)   # ... and here the third is not
        run(341, 1, 0, 1)      # 342 lines: what the index and the row buffers hold
        run(341, 2, 0, 2)      # 343 lines: beyond both
    finally:
        p.close()


def comment_slab(rows, n_lines, n_bytes):
    """`rows` and '#' lines behind them: n_lines lines in n_bytes bytes (the last '#' line takes the slack)"""
    c = n_lines - rows.count(b"\n")
    slack = n_bytes - len(rows) - 2 * c
    assert c >= 1 and slack >= 0
    text = rows + b"#\n" * (c - 1) + b"#" + b"c" * slack + b"\n"
    assert len(text) == n_bytes and text.count(b"\n") == n_lines
    return text


def test_gff_row_bound(ctx):
    """n_bytes / 16 + 1 lines, '#' lines counting, n_bytes with the misalignment; beyond it n_undecided is 1 and nothing is read"""
    row = E.with_newlines_at(32, [31], "gff")
    good = E.with_newlines_at(400, [40, 99, 170, 399], "gff")
    fresh = exon_amd.GFFParser(ctx, max_slab_bytes=SMALL)
    want_good = fresh.parse_host(good)
    assert (want_good["n_rows"], want_good["n_undecided"], want_good["consumed_bytes"]) == (4, 0, 400)
    assert want_good["start"].tolist() == [1, 2, 3, 4]
    fresh.close()
    p = exon_amd.GFFParser(ctx, max_slab_bytes=SMALL)
    try:
        def run(n_lines, n_bytes, misalign, decided):
            got = p.parse_host(comment_slab(row, n_lines, n_bytes), misalign=misalign)
            if decided:
                assert (got["n_rows"], got["n_undecided"], got["consumed_bytes"]) == (1, 0, n_bytes), (n_lines, n_bytes, misalign)
                assert got["start"].tolist() == [1] and got["end"].tolist() == [10]
            else:
                assert got["n_undecided"] == 1, (n_lines, n_bytes, misalign)
                same(p.parse_host(good), want_good)

        run(3, 36, 0, True)      # 36 / 16 + 1 = 3 lines: the bound
        run(4, 38, 0, False)     # 38 / 16 + 1 = 3 < 4
        run(4, 38, 15, True)     # (38 + 15) / 16 + 1 = 4
        run(5, 40, 15, False)
        run(4, 48, 0, True)
        run(5, 48, 0, False)
        run(257, 4096, 0, True)  # max / 16 + 1 lines: what the index holds
        run(258, 4096, 0, False)
        run(256, 4081, 15, True)
        run(257, 4081, 15, True)
        run(258, 4081, 15, False)
    finally:
        p.close()


def bed_rows(k, width=8):
    """k rows of 8 bytes (end = 100 + row) or of 6 (`1 5 9`)"""
    return b"".join(b"1\t5\t%d\n" % (100 + i) for i in range(k)) if width == 8 else b"1\t5\t9\n" * k


def test_bed_row_bound(ctx):
    """n_bytes / 8 + 1 lines, '#' lines counting, n_bytes with the misalignment; beyond it n_undecided is 1.  Rows of 6 bytes are
    well-formed BED and shorter than the bound assumes: from five of them on the slab is handed over, it is never mis-decoded."""
    good = E.with_newlines_at(400, [40, 99, 170, 399], "bed")
    fresh = exon_amd.BEDParser(ctx, max_slab_bytes=SMALL)
    want_good = fresh.parse_host(good)
    assert (want_good["n_rows"], want_good["n_undecided"], want_good["consumed_bytes"]) == (4, 0, 400)
    assert want_good["start"].tolist() == [1, 2, 3, 4]
    fresh.close()
    p = exon_amd.BEDParser(ctx, max_slab_bytes=SMALL)
    try:
        def run(text, misalign, rows):
            got = p.parse_host(text, misalign=misalign)
            if rows is not None:
                assert (got["n_rows"], got["n_undecided"], got["consumed_bytes"]) == (rows, 0, len(text)), (len(text), misalign)
                assert got["start"].tolist() == [5] * rows
                assert got["end"].tolist() == ([9] * rows if text.startswith(b"1\t5\t9\n") else list(range(100, 100 + rows)))
            else:
                assert got["n_undecided"] == 1, (len(text), misalign)
                # the index and the columns keep nothing of the refused slab.  The dictionary does: it grows with every slab the
                # parser sees and never takes an id back, so the name the refused rows brought ("1") keeps its id and the good
                # slab's name comes behind it -- the NAMES of the rows are the fresh parser's
                after = p.parse_host(good)
                names = p.names()
                assert names[0] == "1" and [names[i] for i in after["chrom_id"]] == ["c"] * 4
                same({k: v for k, v in after.items() if k != "chrom_id"}, {k: v for k, v in want_good.items() if k != "chrom_id"})

        for k in (1, 7, 100):
            run(bed_rows(k), 0, k)
            run(comment_slab(bed_rows(k), k + 1, 8 * k + 2), 0, k)      # (8 k + 2) / 8 + 1 = k + 1 lines: the bound
            run(comment_slab(bed_rows(k), k + 2, 8 * k + 4), 0, None)   # k + 2 lines, the bound is k + 1
            run(comment_slab(bed_rows(k), k + 2, 8 * k + 4), 15, k)     # (8 k + 19) / 8 + 1 = k + 3
            run(comment_slab(bed_rows(k), k + 4, 8 * k + 8), 15, None)  # (8 k + 23) / 8 + 1 = k + 3 < k + 4
        for k in (1, 4):
            run(bed_rows(k, 6), 0, k)        # 6 k / 8 + 1 >= k up to four rows
        for k in (5, 6, 100, 600):
            run(bed_rows(k, 6), 0, None)     # ... and not from five on: the host reader's
        run(bed_rows(5, 6), 15, 5)           # (30 + 15) / 8 + 1 = 6
        run(bed_rows(11, 6), 15, 11)         # (66 + 15) / 8 + 1 = 11: the bound
        run(bed_rows(12, 6), 15, None)       # (72 + 15) / 8 + 1 = 11 < 12
        run(comment_slab(bed_rows(511), 513, 4096), 0, 511)   # max / 8 + 1 lines: what the index holds
        run(comment_slab(bed_rows(510), 514, 4096), 0, None)
    finally:
        p.close()
