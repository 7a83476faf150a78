"""GPU: the FASTA device parser alone (exon_hip_fasta_parser_*, through exon_amd.FASTAParser.parse_host) against
tests/fasta_expect.py: record counts around the wave and workgroup sizes, records of 0 .. 20 000 lines (one record's lines across
the workgroups of the offsets scans), every line length around the fill's 8-byte groups, every alignment of the slab, non-final
slabs cut in the three places that matter, and what the parser calls undecided.  Beside what parse_host returns per record, every
line's place in the compacted sequence column (line_dst) is checked: that is what the line-parallel fill copies by."""
import numpy as np
import pytest

import exon_amd
import fasta_expect

pytestmark = pytest.mark.gpu
BASES = b"ACGTNacgtn"


def seq_line(i, n):
    return bytes(BASES[(i + 3 * j) % 10] for j in range(n))


def make(n_records, lines_of_record, len_of_line, crlf_every=0):
    """rows for fasta_expect.write_text: record r has lines_of_record(r) lines, its line j len_of_line(r, j) bytes; every
    crlf_every-th line (definitions included) ends in CRLF"""
    rows, k = [], 0
    for r in range(n_records):
        d = b"r%d" % r + (b"" if r % 3 == 0 else b" d%d x" % r if r % 3 == 1 else b"\t")
        lines = [seq_line(r + j, len_of_line(r, j)) for j in range(lines_of_record(r))]
        if crlf_every:
            if k % crlf_every == 0:
                d += b"\r"
            lines = [ln + b"\r" if (k + 1 + j) % crlf_every == 0 else ln for j, ln in enumerate(lines)]
        k += 1 + len(lines)
        rows.append((d, lines))
    return rows


@pytest.fixture(scope="module")
def parser(ctx):
    p = exon_amd.FASTAParser(ctx, 8 << 20)  # 1 Mi lines
    yield p
    p.close()


def check(parser, text, final, misalign=0):
    got = parser.parse_host(text, final=final, misalign=misalign)
    want = fasta_expect.slab(text, final)
    assert got["n_undecided"] == 0
    assert got["n_records"] == want["n_records"] and got["consumed"] == want["consumed"]
    assert got["definitions"] == want["definitions"]
    assert got["seq_len"] == want["seq_len"]
    # every line's destination: the exclusive prefix of the sequence lines' lengths (CR dropped, definition lines 0)
    raw = text.split(b"\n")[:-1]
    lens = [0 if ln[:1] == b">" else len(ln) - ln.endswith(b"\r") for ln in raw]
    assert got["n_lines"] == len(raw)
    assert np.array_equal(got["line_dst"], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32))
    assert np.array_equal(got["line_end"], np.cumsum([len(ln) + 1 for ln in raw]).astype(np.uint32) - 1)
    assert got["seq_bytes"] == sum(want["seq_len"])
    if want["n_records"]:
        assert got["seq_offsets"][0] == 0 and got["seq_offsets"][-1] == got["seq_bytes"]
    return got


@pytest.mark.parametrize("n_records", [1, 63, 64, 65, 255, 256, 257])
def test_record_counts(parser, n_records):
    rows = make(n_records, lambda r: (0, 1, 2, 1)[r % 4], lambda r, j: 1 + (7 * r + j) % 70, crlf_every=5)
    text = fasta_expect.write_text(rows)
    check(parser, text, True)
    check(parser, text, False)


@pytest.mark.parametrize("n_lines", [0, 1, 2, 300])
def test_lines_per_record(parser, n_lines):
    rows = make(5, lambda r: n_lines, lambda r, j: 60 if j + 1 < n_lines else 17)
    text = fasta_expect.write_text(rows)
    check(parser, text, True)
    check(parser, text, False, misalign=5)


def test_one_record_of_20000_lines_between_short_ones(parser):
    rows = make(41, lambda r: 20000 if r == 20 else 2, lambda r, j: 61 if (r + j) % 9 else 0)
    text = fasta_expect.write_text(rows)
    got = check(parser, text, True)
    assert max(got["seq_len"]) == sum(61 if (20 + j) % 9 else 0 for j in range(20000))
    check(parser, text, False, misalign=9)


@pytest.mark.parametrize("width", [0, 1, 7, 8, 9, 15, 16, 17, 60, 61, 255, 256, 257])
def test_line_lengths(parser, width):
    rows = make(70, lambda r: 1 + r % 3, lambda r, j: width, crlf_every=4)
    check(parser, fasta_expect.write_text(rows), True)


@pytest.mark.parametrize("misalign", range(16))
def test_every_alignment_of_the_slab(parser, misalign):
    rows = make(130, lambda r: r % 4, lambda r, j: (r + 5 * j) % 23, crlf_every=7)
    text = fasta_expect.write_text(rows)
    check(parser, text, True, misalign=misalign)
    check(parser, text, False, misalign=misalign)


def test_non_final_slabs_cut_in_three_places(parser):
    rows = make(300, lambda r: 2, lambda r, j: 60)
    text = fasta_expect.write_text(rows)
    last_def = text.rindex(b"\n>") + 1
    line_start = text.rindex(b"\n", 0, last_def - 1) + 1  # the sequence line in front of the last definition
    cuts = {"inside a sequence line": line_start + 30, "directly behind a newline": line_start, "directly in front of a '>'": last_def}
    for what, cut in cuts.items():
        slab = text[:cut]
        assert slab[-1:] == (b"\n" if what != "inside a sequence line" else slab[-1:])
        got = check(parser, slab, False)
        # the last record never comes out of a slab that is not the input's last, wherever the cut falls
        assert got["n_records"] == 298 and got["consumed"] == text.rindex(b"\n>", 0, cut) + 1, what


def test_non_final_slab_with_one_definition_line_consumes_nothing(parser):
    text = fasta_expect.write_text(make(1, lambda r: 500, lambda r, j: 60))
    got = check(parser, text, False)
    assert got["n_records"] == 0 and got["consumed"] == 0
    got = check(parser, text, True)
    assert got["n_records"] == 1 and got["consumed"] == len(text)


def test_first_line_without_a_definition_is_undecided(parser):
    for text in (b"ACGT\n>a\nAC\n", b"\n>a\nAC\n", b" >a\nAC\n"):
        for final in (True, False):
            got = parser.parse_host(text, final=final)
            assert got["n_undecided"] > 0 and got["n_records"] == 0


def test_more_lines_than_the_parser_was_sized_for_is_undecided(ctx):
    small = exon_amd.FASTAParser(ctx, 4096)  # 4096 / 8 + 8 = 520 lines
    try:
        rows = make(1, lambda r: 518, lambda r, j: 2)
        text = fasta_expect.write_text(rows)  # 519 lines: fits
        got = small.parse_host(text, final=True)
        assert got["n_undecided"] == 0 and got["n_records"] == 1 and got["seq_len"] == [2 * 518]
        text = fasta_expect.write_text(make(1, lambda r: 520, lambda r, j: 2))  # 521 lines
        assert len(text) + 15 <= 4096
        got = small.parse_host(text, final=True)
        assert got["n_undecided"] > 0 and got["n_records"] == 0
    finally:
        small.close()
