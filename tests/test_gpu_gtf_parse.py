"""GPU: GTF at the parser level (exon_hip_gff_parser_set_dialect + k_parse_gff_lines<ATTR, true>; text_columns.hip:
k_gtf_attr_measure -> three offset scans -> k_gtf_attr_fill) against tests/gtf_expect.py: the eight columns and the five buffers
of Map<Utf8, Utf8>, byte for byte -- row counts around the wave and block sizes, ranked rows and row = line, every misalignment,
a row per attribute rule, stale offsets, a slab cut inside a ninth field, and the rows the device hands over.

The capacity table above scratch_for (text_columns.hip) derives that every GTF buffer "fits": no buffer is "checked", so there is
no slab that exceeds one by a row and the list of such cases is empty.  What the derivation rests on is tested instead: the
densest field there is ("k v;k v;...": an entry every four bytes) builds, and its totals are the bound's."""
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import gtf_expect
from test_gpu_gff_parse import device_columns
from test_gtf_scan import ASCII_GOOD, PREFIX

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
BUFFERS = ("map_offsets", "key_offsets", "key_values", "value_offsets", "value_values")
TOTALS = ("n_entries", "n_key_bytes", "n_value_bytes")
ESTATE = -5


def check(ctx, text, misalign=0, parser=None, want=None):
    """the eight columns, the five buffers and the three totals of `text`'s whole lines"""
    own = parser is None
    parser = parser or exon_amd.GFFParser(ctx, dialect="gtf")
    res = parser.parse_host(text, misalign=misalign, attributes=True)
    assert res["n_undecided"] == 0 and res["attributes"]["n_undecided"] == 0
    last = text.rfind(b"\n") + 1
    assert res["consumed_bytes"] == last
    want = want or gtf_expect.expect(text[:last], attrs=True)
    got = device_columns(res, parser)
    assert got["n_rows"] == want["n_rows"]
    for name in ("seqname", "source", "type"):
        assert list(got[name]) == list(want[name]), (name, misalign)
    for name in ("start", "end", "strand_id", "phase_id", "score_valid", "strand_valid", "phase_valid"):
        assert np.array_equal(got[name], want[name]), (name, misalign)
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), misalign
    bufs = want.get("buffers") or gtf_expect.buffers(want["maps"])
    at = res["attributes"]
    assert len(bufs["map_offsets"]) == res["n_rows"] + 1
    for k in TOTALS:
        assert at[k] == bufs[k], (k, misalign)
    for k in BUFFERS:
        assert np.array_equal(at[k], bufs[k]), (k, misalign)
    if own:
        parser.close()
    return res


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    """gen_text gtf 3000 attrs: its lines (two "#!" lines in front, a '#' comment every 1000 rows)"""
    p = tmp_path_factory.mktemp("gtfgpu") / "a.gtf"
    subprocess.check_call([GEN, "gtf", "3000", str(p), "attrs"])
    return open(p, "rb").read().split(b"\n")


def test_row_counts_around_the_wave_and_block_sizes(ctx, rich):
    plain = [ln for ln in rich[2:400] if not ln.startswith(b"#")]
    parser = exon_amd.GFFParser(ctx, dialect="gtf")
    for n in (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 130, 257):
        body = b"\n".join(plain[:n]) + b"\n"
        check(ctx, body, parser=parser)                              # row = line
        check(ctx, b"#!head\n" + body, misalign=3, parser=parser)    # rows are ranks
    parser.close()


def test_every_misalignment_plain_and_ranked(ctx, rich):
    plain = b"\n".join(ln for ln in rich[2:300] if not ln.startswith(b"#")) + b"\n"
    ranked = b"\n".join(rich[380:700]) + b"\n"
    assert b"\n#" not in plain and ranked.count(b"\n#") >= 1
    for slab in (plain, ranked):
        want = gtf_expect.expect(slab, attrs=True)
        want["buffers"] = gtf_expect.buffers(want["maps"])
        parser = exon_amd.GFFParser(ctx, dialect="gtf")
        for misalign in range(16):
            check(ctx, slab, misalign=misalign, parser=parser, want=want)
        parser.close()


def test_a_row_per_rule(ctx):
    assert len(ASCII_GOOD) >= 18
    text = b"".join(PREFIX + f + (b"\r\n" if i % 3 == 0 else b"\n") for i, (f, _m) in enumerate(ASCII_GOOD))
    assert gtf_expect.expect(text, attrs=True)["maps"] == [m for _f, m in ASCII_GOOD]
    check(ctx, text)
    check(ctx, b"#!genome-build x\r\n" + text, misalign=11)


def test_no_stale_offsets_between_slabs(ctx, rich):
    full = b"\n".join(ln for ln in rich[2:300] if not ln.startswith(b"#")) + b"\n"
    empty = b"".join(PREFIX + (b"   \n" if i % 2 else b"\n") for i in range(300))
    parser = exon_amd.GFFParser(ctx, dialect="gtf")
    for slab in (full, empty, full, empty, empty, full):
        res = check(ctx, slab, parser=parser)
        if slab is empty:
            at = res["attributes"]
            assert [at[k] for k in TOTALS] == [0, 0, 0] and not at["map_offsets"].any()
            assert list(at["key_offsets"]) == [0] and list(at["value_offsets"]) == [0]
    parser.close()


def test_a_slab_cut_inside_a_ninth_field(ctx, rich):
    head = b"\n".join(rich[2:200])
    last = head.rfind(b"\n")
    assert b'"' in head[last:]
    for cut in (len(head), last + 1, last + 60, last, len(head) - 1):
        res = check(ctx, head[:cut])
        want_consumed = head.rfind(b"\n", 0, cut) + 1
        assert res["consumed_bytes"] == want_consumed and head[want_consumed - 1:want_consumed] == b"\n"


def test_the_dialects_part_at_the_question_mark_and_keep_their_builders(ctx):
    line = b"chr1\ts\texon\t1\t2\t.\t?\t.\t"
    gtf = exon_amd.GFFParser(ctx, dialect="gtf")
    for attributes in (False, True):
        res = gtf.parse_host(line + b'k "v";\n', attributes=attributes)
        assert res["n_undecided"] == 1
    gff = exon_amd.GFFParser(ctx)
    res = gff.parse_host(line + b"ID=1\n")
    assert res["n_undecided"] == 0 and res["n_rows"] == 1 and not res["strand_valid"][0] & 1
    # each dialect's attributes builder refuses the other's parser
    gff.parse_host(PREFIX + b"ID=1\n", attributes=True)
    a = exon_amd._lib.GTFAttributes()
    import ctypes as C
    assert ctx.lib.exon_hip_gff_parser_gtf_attributes(gff.h, None, C.byref(a)) == ESTATE
    gtf.parse_host(PREFIX + b'k "v";\n', attributes=True)
    b = exon_amd._lib.GFFAttributes()
    assert ctx.lib.exon_hip_gff_parser_attributes(gtf.h, None, C.byref(b)) == ESTATE
    assert ctx.lib.exon_hip_gff_parser_set_dialect(gtf.h, 3) < 0
    gff.close()
    gtf.close()


GOOD_LINE = PREFIX + b'gene_id "G1"; n 1;\n'
UNDECIDED = [("a byte >= 0x80 in a value", b'k "caf\xc3\xa9"'), ("a byte >= 0x80 in a key", b'caf\xc3\xa9 1'), ("an invalid byte", b'k "\xff"'),
             ("an unterminated quote", b'gene_id "G1'), ("an unterminated quote before more entries", b'gene_id "G1; x "y";'),
             ("a key without a value", b"gene_id"), ("a key and spaces", b"gene_id  "), ("a key and ';'", b'a "b"; gene_id;'),
             ("';;'", b'a "b";;'), ("';;' behind a bare value", b"a b;;c d"), ("a leading ';'", b';a "b"'), ("';' alone", b";"),
             ("bytes behind a closing quote", b'a "b"x;')]


@pytest.mark.parametrize("what,field", UNDECIDED, ids=[u[0] for u in UNDECIDED])
def test_rows_the_device_hands_over(ctx, what, field):
    if max(field) < 0x80:  # (a field with a byte >= 0x80 may be valid UTF-8: the host reader's to say, not an error)
        with pytest.raises(gtf_expect.GtfError):
            gtf_expect.attributes(field)
    parser = exon_amd.GFFParser(ctx, dialect="gtf")
    for text in (GOOD_LINE * 70 + PREFIX + field + b"\n" + GOOD_LINE * 70, PREFIX + field + b"\n", b"# c\n" + GOOD_LINE * 3 + PREFIX + field + b"\n"):
        res = parser.parse_host(text, misalign=2, attributes=True)
        assert res["n_undecided"] == 0 and res["attributes"]["n_undecided"] == 1, what
        assert "map_offsets" not in res["attributes"]  # nothing built
    check(ctx, GOOD_LINE * 3, parser=parser)
    parser.close()


def test_the_densest_field_builds_and_meets_the_bound(ctx):
    """an entry every four bytes ("k v;"): a ninth field of k bytes holds (k + 1) / 4 entries, the most the rules allow -- the
    figure the capacity table sizes key_offsets / value_offsets by"""
    rows = [b"a 1;" * 4000 + b"b 2", b"", b"k v", b"a 1;" * 257]
    text = b"".join(b"c\ts\tt\t%d\t%d\t.\t-\t0\t" % (i + 1, i + 2) + f + b"\n" for i, f in enumerate(rows))
    res = check(ctx, text)
    at = res["attributes"]
    assert at["n_entries"] == sum((len(f) + 1) // 4 for f in rows) == 4001 + 0 + 1 + 257
    assert at["n_key_bytes"] == at["n_entries"] == at["n_value_bytes"]
    field_bytes = sum(len(f) for f in rows)
    assert at["n_entries"] <= (field_bytes + len(rows)) // 4 <= len(text) // 4
