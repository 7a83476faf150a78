"""The numbers the device parsers produce, at their limits: QUAL / Float INFO / Float list items of VCF and the GFF score through
`dec::parse_f32`; POS, Integer INFO values and list items, GFF start / end; FLAG, POS, MAPQ and the CIGAR span of SAM; the typed
integers and floats of BCF.  Two halves of one contract: what the device decides is bit-identical to the correctly rounded,
correctly ranged value, and what it cannot decide is counted as undecided -- never served as a value.

Float expectations come from tests/decimal_exact.py (exact rational arithmetic; tests/test_decimal_exact.py proves it equal to
glibc's strtof and to the host reader on the same case list); integer and BCF expectations from the python rows the slabs are
written from.  The host readers are a second opinion (CPU tests below, no marker)."""
import ctypes as C
import gzip
import os
import struct

import numpy as np
import pytest

import bam_sam_writer as bsw
import decimal_exact as dx
import exon_amd
import vcf_bcf_writer as W
from exon_amd import _lib as L

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")

CASES = dx.float_cases()
WANT = np.array([dx.f32_bits(t) for t in CASES], np.uint32)  # computed once, shared, never changed
SITES = ["qual", "info_f", "list_F", "gff_score"]
# a line the slab does not finish: with it the last complete line is NOT within the slab's final 16 bytes, without it it is
UNFINISHED = {"qual": b"1\t5\t.", "info_f": b"1\t5\t.", "list_F": b"1\t5\t.", "gff_score": b"chr1\tsrc", "vcf": b"1\t5\t.", "gff": b"chr1\tsrc"}
SLAB = 1 << 20  # every slab here is far below it


def bits(bm, n):
    return np.unpackbits(np.asarray(bm).view(np.uint8), bitorder="little")[:n].astype(bool)


@pytest.fixture(scope="module")
def parsers(ctx):
    """one parser per site, shared by the tests of this file (their dictionaries grow; nothing here reads them)"""
    made = {"qual": exon_amd.VCFParser(ctx, ["1"], info_field="AF", max_slab_bytes=SLAB),
            "info_f": exon_amd.VCFParser(ctx, ["1"], info_field="AF,DP:i,DB:b", max_slab_bytes=SLAB),
            "list_F": exon_amd.VCFParser(ctx, ["1"], info_field="DP:i,MQS:F", max_slab_bytes=SLAB),
            "gff_score": exon_amd.GFFParser(ctx, max_slab_bytes=SLAB),
            "ints": exon_amd.VCFParser(ctx, ["1"], info_field="DP:i,AC:I", max_slab_bytes=SLAB),
            "sam": exon_amd.SAMParser(ctx, [n for n, _ in bsw.REFS], max_slab_bytes=SLAB)}
    yield made
    for p in made.values():
        p.close()


# ---- floats: one text per case at each of the four call sites of dec::parse_f32 -------------------------------------------------
LIST_SHAPES = ["C", "C,.,C", ".,C,,C,C", "C,C,C,C", ",C", "C,", "C,.", ".,.,C", "C,C"]  # C = the next case; '.' and '' are NULL items


def list_rows(texts):
    """-> (the MQS value of every row, per row the list of case indexes (None = a NULL item))"""
    values, layout, k, r = [], [], 0, 0
    while k < len(texts):
        items, idx = [], []
        for it in LIST_SHAPES[r % len(LIST_SHAPES)].split(","):
            if it == "C" and k < len(texts):
                items.append(texts[k])
                idx.append(k)
                k += 1
            elif it != "C":
                items.append(it)
                idx.append(None)
        if all(i is None for i in idx):
            continue  # (the cases ran out inside a shape)
        values.append(",".join(items))
        layout.append(idx)
        r += 1
    return values, layout


def site_slab(site, texts):
    if site == "qual":
        return "".join(f"1\t{i + 1}\t.\tA\tC\t{t}\tPASS\tAF=0.5\n" for i, t in enumerate(texts)).encode()
    if site == "info_f":  # the value ends at the line's end, at a ';', behind other keys
        shapes = ["AF={}", "DP=3;AF={}", "AF={};DB", "DB;AF={};DP=7"]
        return "".join(f"1\t{i + 1}\t.\tA\tC\t1\tPASS\t{shapes[i % 4].format(t)}\n" for i, t in enumerate(texts)).encode()
    if site == "list_F":
        shapes = ["MQS={}", "DP=3;MQS={}", "MQS={};DP=1"]
        return "".join(f"1\t{i + 1}\t.\tA\tC\t1\tPASS\t{shapes[i % 3].format(v)}\n" for i, v in enumerate(list_rows(texts)[0])).encode()
    return "".join(f"chr1\tsrc\tgene\t{i + 1}\t{i + 10}\t{t}\t+\t.\tID=g\n" for i, t in enumerate(texts)).encode()


def parse_site(parsers, site, texts, misalign=0, tail=b""):
    """-> (n_undecided, per case: valid, per case: the value's bits)"""
    slab = site_slab(site, texts) + tail
    n = len(texts)
    if site == "gff_score":
        res = parsers[site].parse_host(slab, misalign=misalign, all_rows=True)
        assert res["n_rows"] == n
        return res["n_undecided"], bits(res["score_valid"], n), res["score"].view(np.uint32)
    res = parsers[site].parse_host(slab, misalign=misalign)
    if site == "qual":
        assert res["n_rows"] == n
        return res["n_undecided"], bits(res["qual_valid"], n), res["qual"].view(np.uint32)
    if site == "info_f":
        assert res["n_rows"] == n
        return res["n_undecided"], bits(res["info_valid"], n), res["info"].view(np.uint32)
    # the list column: its shape (list validity, offsets, item validity) is checked here, the items are handed back per case
    values, layout = list_rows(texts)
    k = res["infos"][1]
    rows = len(values)
    assert res["n_rows"] == rows and k["kind"] == "F"
    want_off = np.concatenate([[0], np.cumsum([len(x) for x in layout])]).astype(np.int32)
    assert np.array_equal(k["offsets"], want_off) and bits(k["valid"], rows).all()
    item_valid, item_bits = bits(k["item_valid"], int(want_off[-1])), k["values"].view(np.uint32)
    valid, got = np.zeros(n, bool), np.zeros(n, np.uint32)
    for r, idx in enumerate(layout):
        for j, case in enumerate(idx):
            i = int(want_off[r]) + j
            if case is None:
                assert not item_valid[i], (site, r, j, "a '.' or empty item must be a NULL item")
            else:
                valid[case], got[case] = item_valid[i], item_bits[i]
    return res["n_undecided"], valid, got


def assert_exact(site, und, valid, got, texts=CASES, want=WANT, what=""):
    assert und == 0, (site, what, "rows left undecided", und)
    assert valid.all(), (site, what, "NULL:", [texts[i] for i in np.flatnonzero(~valid)[:10]])
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (site, what, [(texts[i], hex(want[i]), hex(got[i])) for i in diff[:10]])


@gpu
@pytest.mark.parametrize("site", SITES)
def test_every_decimal_the_device_decides_is_the_nearest_binary32(ctx, parsers, site):
    """tie-adjacent values with 17-19 digits across the exponent range, 1-19 significant digits with leading and trailing zeros,
    both sides of the 2^24 division fast path, exponent forms and the borders of the power-of-ten table, FLT_MAX / inf, FLT_MIN,
    the subnormals, underflow, signs and short forms: no row undecided, no value NULL, every bit that of the exact reference"""
    und, valid, got = parse_site(parsers, site, CASES, tail=UNFINISHED[site])
    assert_exact(site, und, valid, got)


@gpu
@pytest.mark.parametrize("site", SITES)
def test_decimals_at_every_slab_misalignment_and_in_the_slab_tail(ctx, parsers, site):
    """the slab 0-15 bytes past a 16-byte boundary, and ending right behind the last line (its last fields inside the final 16 bytes:
    the byte-wise tail of the 16-byte group loads) or inside an unfinished line"""
    for misalign in range(16):
        for tail in (UNFINISHED[site], b""):
            und, valid, got = parse_site(parsers, site, CASES, misalign=misalign, tail=tail)
            assert_exact(site, und, valid, got, what=(misalign, tail))


NEIGHBOURS = ["1.5", "16777217", "1.000000059604644776", "3.4028235677973366e38", "7.006492321624085355e-46", "-0", ".5", "1e-5"]
NEIGHBOUR_BITS = np.array([dx.f32_bits(t) for t in NEIGHBOURS], np.uint32)
NULL_SPELLINGS = {"qual": ["."], "info_f": [".", ""], "list_F": [".", ""], "gff_score": ["."]}


@gpu
@pytest.mark.parametrize("site", SITES)
def test_what_the_device_must_not_decide_is_counted_not_served(ctx, parsers, site):
    """each text in a slab of its own between decidable rows: exactly one row undecided, no value served for it, the neighbours keep
    theirs.  The NULL spellings of the site ('.', and an empty INFO value or list item) are NULL and decided."""
    texts = [t for t, _ in dx.FLOAT_UNDECIDABLE]
    if site != "list_F":
        texts += [t for t, _ in dx.FLOAT_UNDECIDABLE_SCALAR_ONLY]
    texts += [t for t in ("", ".") if t not in NULL_SPELLINGS[site]]
    keep = np.ones(len(NEIGHBOURS) + 1, bool)
    keep[4] = False
    for t in texts:
        und, valid, got = parse_site(parsers, site, NEIGHBOURS[:4] + [t] + NEIGHBOURS[4:])
        assert und == 1, (site, t, und)
        assert not valid[4], (site, t, "served as", hex(got[4]))
        assert valid[keep].all() and np.array_equal(got[keep], NEIGHBOUR_BITS), (site, t)
    for t in NULL_SPELLINGS[site]:
        if site == "list_F":  # as an item of a longer list (alone it is the NULL list: below)
            res = parsers[site].parse_host(b"1\t1\t.\tA\tC\t1\tPASS\tMQS=1.5," + t.encode() + b",2.5\n")
            k = res["infos"][1]
            assert res["n_undecided"] == 0 and k["offsets"].tolist() == [0, 3] and bits(k["item_valid"], 3).tolist() == [True, False, True]
            res = parsers[site].parse_host(b"1\t1\t.\tA\tC\t1\tPASS\tMQS=" + t.encode() + b"\n")
            assert res["n_undecided"] == 0 and res["infos"][1]["offsets"].tolist() == [0, 0] and not bits(res["infos"][1]["valid"], 1)[0]
            continue
        und, valid, got = parse_site(parsers, site, NEIGHBOURS[:4] + [t] + NEIGHBOURS[4:])
        assert und == 0 and not valid[4] and valid[keep].all() and np.array_equal(got[keep], NEIGHBOUR_BITS), (site, t)


VCF_HEAD = ('##fileformat=VCFv4.3\n##contig=<ID=1>\n##INFO=<ID=AF,Number=1,Type=Float,Description="x">\n'
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def scan_columns(ctx, path, gpu_parse):
    s = exon_amd.Scan(str(path), "vcf", info_field="AF", gpu_parse=gpu_parse)
    if gpu_parse:
        s.bind_ctx(ctx)
    try:
        qual, info = [], []
        for b in s:
            qual += b.field(2).to_pylist()
            info += b.field(4).to_pylist()
        return np.array(qual, np.float32).view(np.uint32), np.array(info, np.float32).view(np.uint32)
    finally:
        s.close()


@gpu
def test_a_file_with_an_undecidable_float_gets_the_host_readers_answer(ctx, tmp_path, monkeypatch):
    """through the GPU pipeline (Scan, gpu_parse=True) the same file gives what the host reader gives: a value for inf / infinity /
    nan in any letter case and for more than 19 digits, the host's error for the rest (test_float_fields_follow_rusts_grammar)"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")  # (small device buffers: one pipeline is set up per text)
    rows = CASES[:300]
    for t, ok in dx.FLOAT_UNDECIDABLE + dx.FLOAT_UNDECIDABLE_SCALAR_ONLY:
        p = tmp_path / "t.vcf"
        body = [f"1\t{i + 1}\t.\tA\tC\t{c}\tPASS\tAF={rows[-1 - i]}\n" for i, c in enumerate(rows)]
        body.insert(200, f"1\t201\t.\tA\tC\t{t}\tPASS\tAF={t}\n")
        p.write_bytes((VCF_HEAD + "".join(body)).encode())
        if not ok:
            with pytest.raises(exon_amd.ExonHipError, match="float"):
                scan_columns(ctx, p, True)
            continue
        want_q, want_i = scan_columns(ctx, p, False)
        got_q, got_i = scan_columns(ctx, p, True)
        assert len(got_q) == 301, t
        nan = np.isnan(want_q.view(np.float32))  # (a NaN is NaN on both paths: its payload is strtof's)
        assert np.array_equal(nan, np.isnan(got_q.view(np.float32))) and np.array_equal(got_q[~nan], want_q[~nan]), t
        assert np.array_equal(nan, np.isnan(got_i.view(np.float32))) and np.array_equal(got_i[~nan], want_i[~nan]), t
        exact = dx.f32_bits(t)
        assert nan[200] or (got_q[200] == exact and got_i[200] == exact), t


# ---- integers -------------------------------------------------------------------------------------------------------------------
def pos_slab(texts):
    return "".join(f"1\t{t}\t.\tA\tC\t.\t.\t.\n" for t in texts).encode()


POS_TEXTS = [t for t, _ in dx.POS_CASES] + dx.POS_ZERO
POS_WANT = [v for _, v in dx.POS_CASES] + [None] * len(dx.POS_ZERO)


def check_pos(res, want, what=""):
    n = len(want)
    assert res["n_rows"] == n and res["n_undecided"] == 0, (what, res["n_undecided"])
    valid = bits(res["pos_valid"], n)
    assert [int(p) if v else None for p, v in zip(res["pos"], valid)] == want, what


@gpu
def test_vcf_pos_up_to_18_digits_at_every_alignment(ctx, parsers):
    """1-18 digits (both sides of the 16-digit load), one '+', leading zeros up to 18 characters, 0 and +0 -> NULL; every slab
    misalignment, the slab ending behind the last line or inside the next"""
    p = parsers["ints"]
    for misalign in range(16):
        for tail in (UNFINISHED["vcf"], b""):
            check_pos(p.parse_host(pos_slab(POS_TEXTS) + tail, misalign=misalign), POS_WANT, (misalign, tail))


@gpu
def test_vcf_pos_in_the_last_line_of_the_slab(ctx, parsers):
    """every POS text as the slab's last line, the shortest the format allows: the field lies inside the final 16 bytes (a one-digit
    POS starts less than 16 bytes from the end: the 16-byte digit load must not be taken there)"""
    p = parsers["ints"]
    for t, v in zip(POS_TEXTS, POS_WANT):
        for misalign in (0, 9):
            check_pos(p.parse_host(pos_slab(["77", t]), misalign=misalign), [77, v], (t, misalign))


@gpu
def test_vcf_pos_the_device_hands_over(ctx, parsers):
    """19 and 20 digits, signs other than one leading '+', blanks, an empty field: one undecided row each, the neighbours keep theirs"""
    p = parsers["ints"]
    for t in dx.POS_UNDECIDABLE:
        for tail in (UNFINISHED["vcf"], b""):
            res = p.parse_host(pos_slab(["12345678901234567", t, "+5"]) + tail)
            assert res["n_rows"] == 3 and res["n_undecided"] == 1, (t, res["n_undecided"])
            valid = bits(res["pos_valid"], 3)
            assert not valid[1] and valid[0] and valid[2] and res["pos"][0] == 12345678901234567 and res["pos"][2] == 5, t
        res = p.parse_host(pos_slab(["5", t]))  # ... and as the slab's last line
        assert res["n_undecided"] == 1 and not bits(res["pos_valid"], 2)[1] and res["pos"][0] == 5, t


def int_slab(texts):
    """case i as the scalar DP of row i and, with case n - 1 - i and a NULL item, in its AC list"""
    n = len(texts)
    shapes = ["DP={0};AC={1},.,{0}", "AC={0},{1};DP={0}", "DP={0};AC={0},,{1};X"]
    return "".join(f"1\t{i + 1}\t.\tA\tC\t.\t.\t{shapes[i % 3].format(t, texts[n - 1 - i])}\n" for i, t in enumerate(texts)).encode()


def int_expected(values):
    n = len(values)
    lists = [[[values[n - 1 - i], None, v], [v, values[n - 1 - i]], [v, None, values[n - 1 - i]]][i % 3] for i, v in enumerate(values)]
    return list(values), lists


def int_columns(res):
    n = res["n_rows"]
    dp, ac = res["infos"]
    assert dp["kind"] == "i" and ac["kind"] == "I"
    v = bits(dp["valid"], n)
    scalars = [int(x) if ok else None for x, ok in zip(dp["values"].view(np.int32), v)]
    off, lv = ac["offsets"], bits(ac["valid"], n)
    iv, items = bits(ac["item_valid"], int(off[-1]) if n else 0), ac["values"].view(np.int32)
    lists = [None if not lv[r] else [int(items[i]) if iv[i] else None for i in range(off[r], off[r + 1])] for r in range(n)]
    return scalars, lists


@gpu
def test_vcf_integer_info_values_and_list_items_cover_int32(ctx, parsers):
    """INT32_MIN, INT32_MAX, -0, +7, ten digits with leading zeros: scalar 'i' and list items 'I', at every slab alignment"""
    texts, values = [t for t, _ in dx.INT_CASES], [v for _, v in dx.INT_CASES]
    want = int_expected(values)
    for misalign in range(16):
        for tail in (UNFINISHED["vcf"], b""):
            res = parsers["ints"].parse_host(int_slab(texts) + tail, misalign=misalign)
            assert res["n_rows"] == len(texts) and res["n_undecided"] == 0, (misalign, tail, res["n_undecided"])
            assert int_columns(res) == want, (misalign, tail)


@gpu
def test_vcf_integer_info_values_the_device_hands_over(ctx, parsers):
    """one past either end of int32, eleven characters, lone or doubled signs, a fraction: as the scalar and as a list item, one
    undecided row each; the neighbours keep their values"""
    for t in dx.INT_UNDECIDABLE:
        for bad_row in (f"DP={t};AC=1,2", f"DP=4;AC=1,{t},3", f"AC={t}"):
            slab = f"1\t1\t.\tA\tC\t.\t.\tDP=-2147483648;AC=2147483647,.\n1\t2\t.\tA\tC\t.\t.\t{bad_row}\n1\t3\t.\tA\tC\t.\t.\tAC=-7;DP=+7\n".encode()
            res = parsers["ints"].parse_host(slab)
            assert res["n_rows"] == 3 and res["n_undecided"] == 1, (t, bad_row, res["n_undecided"])
            scalars, lists = int_columns(res)
            assert (scalars[0], scalars[2], lists[0], lists[2]) == (-2**31, 7, [2**31 - 1, None], [-7]), (t, bad_row)
            if bad_row.startswith(f"DP={t}"):
                assert not bits(res["infos"][0]["valid"], 3)[1], (t, "served as a scalar")
            else:
                off = res["infos"][1]["offsets"]
                k = 1 if "," in bad_row else 0
                assert not bits(res["infos"][1]["item_valid"], int(off[-1]))[off[1] + k], (t, "served as a list item")


def gff_slab(pairs):
    return "".join(f"chr1\tsrc\tgene\t{a}\t{b}\t.\t+\t.\tx\n" for a, b in pairs).encode()


@gpu
def test_gff_start_and_end_up_to_18_digits_at_every_alignment(ctx, parsers):
    """the POS list in both columns (end < start is accepted as it is), every misalignment, the slab tail, and every text in the last
    line of a slab (nine bytes behind `end`: up to six digits of it are read byte by byte there)"""
    texts, values = [t for t, _ in dx.POS_CASES], [v for _, v in dx.POS_CASES]
    n = len(texts)
    pairs = [(t, texts[n - 1 - i]) for i, t in enumerate(texts)]
    p = parsers["gff_score"]
    for misalign in range(16):
        for tail in (UNFINISHED["gff"], b""):
            res = p.parse_host(gff_slab(pairs) + tail, misalign=misalign)
            assert res["n_rows"] == n and res["n_undecided"] == 0, (misalign, tail, res["n_undecided"])
            assert res["start"].tolist() == values and res["end"].tolist() == values[::-1], (misalign, tail)
    for t, v in zip(texts, values):
        res = p.parse_host(gff_slab([("7", "8"), ("3", t)]), misalign=5)
        assert res["n_undecided"] == 0 and res["start"].tolist() == [7, 3] and res["end"].tolist() == [8, v], t


@gpu
def test_gff_start_and_end_the_device_hands_over(ctx, parsers):
    """what POS hands over, and 0 in every spelling: the host rejects a start or end below 1"""
    p = parsers["gff_score"]
    for t in dx.POS_UNDECIDABLE + dx.POS_ZERO:
        for pair in ((t, "9"), ("9", t)):
            res = p.parse_host(gff_slab([("123456789012345678", "2"), pair, ("+4", "5")]), all_rows=True)
            assert res["n_rows"] == 3 and res["n_undecided"] == 1, (pair, res["n_undecided"])
            assert res["start"][[0, 2]].tolist() == [123456789012345678, 4] and res["end"][[0, 2]].tolist() == [2, 5], pair
            res = p.parse_host(gff_slab([("1", "2"), pair]))  # ... in the slab's last line
            assert res["n_undecided"] == 1, pair


# ---- SAM ------------------------------------------------------------------------------------------------------------------------
REF_NAMES = [n for n, _ in bsw.REFS]
SAM_ROWS = [  # (flag, rname, pos, mapq, cigar)
    ("0", "r1", "1", "0", "5M"), ("65535", "r2", "2147483647", "254", "1M"), ("4095", "*", "0", "255", "*"), ("1", "zz", "7", "255", "10M"),
    ("16", "r1", "100", "60", "12M34I56D78N90S12H34P56=78X"), ("0000", "r1", "0000000100", "000", "007M"), ("99", "r2", "2147483647", "1", "2147483647M2147483647D"),
    ("147", "r2", "2147483647", "37", "268435455M268435455D268435455N268435455=268435455X"), ("65535", "r1", "5", "254", "100S"), ("4", "r1", "9", "3", "*"),
    ("256", "r2", "0", "0", "50M"), ("2048", "r1", "1000000", "42", "1M2I3M"), ("0", "r1", "2", "7", "0M"), ("1024", "r1", "123456789", "200", "10M1000000N10M")]


def sam_slab(rows):
    return "".join(f"q{i}\t{f}\t{r}\t{p}\t{m}\t{c}\t*\t0\t0\t*\t*\n" for i, (f, r, p, m, c) in enumerate(rows)).encode()


def sam_expected(rows):
    """gpu_parse.hip's SAM rules, stated plainly: FLAG as it is; RNAME through the header's @SQ order, '*' or unknown -> NULL; POS 0 ->
    NULL start and end; MAPQ 255 -> NULL; end = POS + (sum of the M / D / N / = / X lengths) - 1"""
    import re
    out = dict(flag=[], mapq=[], ref=[], start=[], end=[])
    for f, r, p, m, c in rows:
        span = 0 if c == "*" else sum(int(n) for n, op in re.findall(r"([0-9]+)([A-Z=])", c) if op in "MDN=X")
        out["flag"].append(int(f))
        out["mapq"].append(None if int(m) == 255 else int(m))
        out["ref"].append(REF_NAMES.index(r) if r in REF_NAMES else None)
        out["start"].append(int(p) if int(p) >= 1 else None)
        out["end"].append(int(p) + span - 1 if int(p) >= 1 else None)
    return out


def sam_columns(res, rows=None):
    n = res["n_rows"]
    mv, rv, pv = bits(res["mapq_valid"], n), bits(res["ref_valid"], n), bits(res["pos_valid"], n)
    pick = range(n) if rows is None else rows
    return dict(flag=[int(res["flag"][i]) for i in pick], mapq=[int(res["mapq"][i]) if mv[i] else None for i in pick],
                ref=[int(res["ref_id"][i]) if rv[i] else None for i in pick], start=[int(res["start"][i]) if pv[i] else None for i in pick],
                end=[int(res["end"][i]) if pv[i] else None for i in pick])


def test_sam_statement_agrees_with_the_host_reader(tmp_path):
    """CPU: the plain statement above against the host SAM reader on the decidable rows (a reference the header lacks left out:
    whether the host takes it is not this test's matter)"""
    rows = [r for r in SAM_ROWS if r[1] != "zz"]
    p = tmp_path / "t.sam"
    p.write_bytes(("@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in bsw.REFS)).encode() + sam_slab(rows))
    s = exon_amd.Scan(str(p), "sam")
    got = {k: [] for k in ("flag", "mapping_quality", "reference", "start", "end")}
    for b in s:
        for i in range(b.type.num_fields):
            if b.type.field(i).name in got:
                got[b.type.field(i).name] += b.field(i).to_pylist()
    s.close()
    want = sam_expected(rows)
    assert got["flag"] == want["flag"] and got["mapping_quality"] == want["mapq"] and got["start"] == want["start"] and got["end"] == want["end"]
    assert got["reference"] == [None if r is None else REF_NAMES[r] for r in want["ref"]]


@gpu
def test_sam_flag_pos_mapq_and_cigar_span_at_their_limits(ctx, parsers):
    """FLAG 0 and 65535, MAPQ 0 / 254 / 255 (NULL), POS 0 (NULL) and 2^31 - 1, CIGAR '*', every operator with multi-digit lengths,
    end = pos + span - 1 at the top of the range (beyond 2^32: the columns are 64-bit); every misalignment and the slab tail"""
    want = sam_expected(SAM_ROWS)
    assert want["end"][6] == 3 * (2**31 - 1) - 1 > 2**32
    for misalign in range(16):
        for tail in (b"q\t0\tr1", b""):
            res = parsers["sam"].parse_host(sam_slab(SAM_ROWS) + tail, misalign=misalign)
            assert res["n_rows"] == len(SAM_ROWS) and res["n_undecided"] == 0, (misalign, tail, res["n_undecided"])
            assert sam_columns(res) == want, (misalign, tail)


@gpu
def test_sam_numbers_the_device_hands_over(ctx, parsers):
    """FLAG 65536, MAPQ 256, POS 2^31, any sign, a blank, an empty field, 19 digits: one undecided row each, the neighbours decided"""
    good = ("65535", "r2", "2147483647", "254", "3M")
    bad = [("65536", "r1", "1", "0", "1M"), ("0", "r1", "1", "256", "1M"), ("0", "r1", "2147483648", "0", "1M"), ("0", "r1", "4294967297", "0", "1M"),
           ("4294967296", "r1", "1", "0", "1M"), ("0", "r1", "1", "4294967296", "1M"), ("0", "r1", "1" + "0" * 18, "0", "1M")]
    for t in ("+1", "-1", "", " 1", "1 ", "1.0", "0x1"):
        bad += [(t, "r1", "1", "0", "1M"), ("0", "r1", t, "0", "1M"), ("0", "r1", "1", t, "1M")]
    want = sam_expected([good, good])
    for row in bad:
        res = parsers["sam"].parse_host(sam_slab([good, row, good]))
        assert res["n_rows"] == 3 and res["n_undecided"] == 1, (row, res["n_undecided"])
        assert sam_columns(res, rows=(0, 2)) == want, row


# ---- BCF typed values -----------------------------------------------------------------------------------------------------------
F1 = 0x3F800000  # 1.0f
FLOAT_BITS = [0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800003, 0xFFC00001, 0x7F7FFFFF, 0x3F800001]
INT_EDGES = {1: [-120, -119, -1, 0, 1, 126, 127], 2: [-32760, -121, -120, 127, 128, 32767], 3: [-2147483640, -32761, -32760, 32767, 32768, 2147483647, 16777217]}


def bcf_rows():
    """rows for tests/vcf_bcf_writer.py's opt-in knobs: AF (Float, Number=1), DP (Integer, Number=1), AC (Integer list), MQS (Float list)"""
    infos = []
    for w, edges in INT_EDGES.items():
        for v in edges:  # every edge value of the width: as a scalar, in a list, and read through a Float key
            infos.append({"DP": W.Ints([v], width=w), "AC": W.Ints([v, 0, v], width=w), "AF": W.Ints([v], width=w), "MQS": W.Ints([0, v], width=w)})
        # the width's missing value: a NULL scalar, a NULL item, a NULL one-item list
        infos.append({"DP": W.Ints([None], width=w), "AC": W.Ints([5, None, 7], width=w), "AF": W.Ints([None], width=w), "MQS": W.Ints([None, 3], width=w)})
        infos.append({"AC": W.Ints([None], width=w), "MQS": W.Ints([None], width=w)})
        # end of vector after 0, 1 and k items
        infos.append({"AC": W.Ints([], width=w, pad=2), "MQS": W.Ints([], width=w, pad=1), "DP": W.Ints([], width=w, pad=1), "AF": W.Ints([], width=w, pad=3)})
        infos.append({"AC": W.Ints([5], width=w, pad=1), "MQS": W.Ints([6], width=w, pad=2), "DP": W.Ints([9], width=w, pad=2), "AF": W.Ints([4], width=w, pad=1)})
        infos.append({"AC": W.Ints([5, None, 7], width=w, pad=2), "MQS": W.Ints([1, 2, None, 4], width=w, pad=1)})
        infos.append({"AC": W.Ints([None], width=w, pad=2), "MQS": W.Ints([None], width=w, pad=1)})  # `.` and padding: still the one missing item
        # the vector's length written as an extended count in this width
        infos.append({"AC": W.Ints([1, 2, 3], count_width=w), "MQS": W.Floats([F1, None, F1 + 1], count_width=w), "DP": W.Ints([11], count_width=w)})
    infos.append({"MQS": W.Floats([], pad=2), "AF": W.Floats([], pad=1)})
    infos.append({"MQS": W.Floats([F1], pad=1), "AF": W.Floats([F1], pad=2)})
    infos.append({"MQS": W.Floats([F1, None, F1 + 2], pad=3), "AF": W.Floats([None], pad=1)})
    infos.append({"MQS": W.Floats([None]), "AF": W.Floats([None])})
    infos.append({"MQS": W.Floats([None], pad=2)})
    for n in (14, 15, 16, 300):  # on both sides of the inline count's limit; 300 needs an int16 count
        infos.append({"AC": W.Ints([(-1) ** i * (i * 7919 % 100000) for i in range(n)]), "MQS": W.Floats([F1 + 3 * i for i in range(n)])})
        infos.append({"AC": W.Ints([None if i % 5 == 2 else i for i in range(n)], pad=2), "MQS": W.Floats([None if i % 7 == 1 else F1 + i for i in range(n)], pad=1)})
    infos.append({"AC": W.Ints(range(300), width=3, count_width=3), "MQS": W.Ints(range(-150, 150), width=2)})
    for b in FLOAT_BITS:  # bit patterns kept as they are: only 0x7F800001 (missing) and 0x7F800002 (end of vector) mean something else
        infos.append({"AF": W.Floats([b]), "MQS": W.Floats([b, F1, b])})
    infos.append({"AF": W.Ints([16777217], width=3), "MQS": W.Ints([2147483647, None, -2147483640, 16777219], width=3, pad=1)})  # integers under Float keys round
    rows = [dict(chrom="1", pos=i + 1, qual=None, filter=[], info=info) for i, info in enumerate(infos)]
    for kw in (1, 2, 3):  # the INFO key index as int8, int16 and int32
        rows.append(dict(chrom="1", pos=len(rows) + 1, qual=None, filter=[], key_width=kw, info={"DP": 100 + kw, "AF": W.Floats([F1 + kw]), "AC": W.Ints([kw, kw])}))
    for b in FLOAT_BITS:  # QUAL: the same patterns
        rows.append(dict(chrom="1", pos=len(rows) + 1, qual=None, qual_bits=b, filter=[], info=None))
    rows.append(dict(chrom="1", pos=None, pos0=-1, qual=1.5, filter=[], info=None))  # POS 0: NULL
    rows.append(dict(chrom="2", pos=2**31 - 1, pos0=2**31 - 2, qual=None, filter=[], info=None))
    return rows


def f32_of_int(v):
    return dx.f32_bits(str(v))


def bcf_expected(rows):
    """The python statement of the BCF rules (VCF specification 6.3.3 decides where the readers and this statement differ; none
    of the cases left standing differ): a vector's items are those in front of its first end-of-vector value; the width's missing
    value is a NULL item; a Number=1 key takes the first item (NULL when there is none or it is missing); a list is NULL when it has
    no item or its ONE item is missing (`key=.`); an integer under a Float key converts to the nearest binary32; float bits are kept.
    -> columns pos, qual (bits), AF (bits), DP, AC, MQS (lists of bits)"""
    out = {k: [] for k in ("pos", "qual", "AF", "DP", "AC", "MQS")}

    def items(v, as_float):
        if isinstance(v, W.Ints):
            return [None if x is None else (f32_of_int(x) if as_float else x) for x in v.vals]
        if isinstance(v, W.Floats):
            return list(v.bits)
        return [f32_of_int(v) if as_float else v]
    for r in rows:
        pos0 = r["pos0"] if "pos0" in r else r["pos"] - 1
        out["pos"].append(pos0 + 1 if pos0 >= 0 else None)
        q = r.get("qual_bits", None if r["qual"] is None else dx.f32_bits(repr(r["qual"])))
        out["qual"].append(None if q == W.FLOAT_MISSING else q)
        info = r["info"] or {}
        for key, as_float, scalar in (("AF", True, True), ("DP", False, True), ("AC", False, False), ("MQS", True, False)):
            if key not in info:
                out[key].append(None)
                continue
            it = items(info[key], as_float)
            if scalar:
                out[key].append(it[0] if it else None)
            else:
                out[key].append(None if not it or it == [None] else it)
    return out


def arrow_column(batches, k, as_bits):
    """column k of the batches as python values; a float column (or a float list's items) as bit patterns, read from the buffers"""
    import pyarrow as pa
    out = []
    for b in batches:
        col = b.field(k)

        def flat(a):
            if not as_bits:
                return a.to_pylist()
            raw = np.frombuffer(a.buffers()[1], np.uint32)[a.offset:a.offset + len(a)]
            return [int(x) if ok else None for x, ok in zip(raw, a.is_valid().to_pylist())]
        if pa.types.is_list(col.type):
            child, off = flat(col.values), col.offsets.to_pylist()
            out += [child[off[i]:off[i + 1]] if ok else None for i, ok in enumerate(col.is_valid().to_pylist())]
        else:
            out += flat(col)
    return out


def scan_bcf(path, ctx=None, keys=("AF", "DP", "AC", "MQS")):
    s = exon_amd.Scan(str(path), "bcf", info_field=",".join(keys), gpu_parse=ctx is not None)
    if ctx is not None:
        s.bind_ctx(ctx)
    batches = list(s)
    got = {"pos": arrow_column(batches, 1, False), "qual": arrow_column(batches, 2, True)}
    for k, key in enumerate(keys):
        got[key] = arrow_column(batches, 4 + k, key in ("AF", "MQS"))
    on_gpu = s.decoded_on_gpu()[0] if ctx is not None else False
    s.close()
    return got, on_gpu


@pytest.fixture(scope="module")
def bcf_file(tmp_path_factory):
    rows = bcf_rows()
    path = tmp_path_factory.mktemp("numeric_limits") / "typed.bcf"
    W.write_bcf(path, rows, BGZIP, filters=[])
    return path, rows, bcf_expected(rows)


def test_bcf_typed_values_host_reader(bcf_file):
    """CPU: the host BCF reader against the python statement"""
    path, rows, want = bcf_file
    got, _ = scan_bcf(path)
    for k in want:
        bad = [(i, want[k][i], got[k][i]) for i in range(len(rows)) if want[k][i] != got[k][i]]
        assert not bad, (k, bad[:5])


@gpu
def test_bcf_typed_values_device_parser(ctx, bcf_file):
    """k_bcf_extract / k_bcf_list_fill against the python statement: every width's edge, missing and end-of-vector values, vectors of
    14 / 15 / 16 / 300 items, key indexes and extended counts in every integer width, integers under Float keys, float bits kept"""
    path, rows, want = bcf_file
    raw = gzip.decompress(open(path, "rb").read())
    l_text, = struct.unpack_from("<I", raw, 5)
    body = raw[9 + l_text:]
    sidx = W.string_index([])
    h = C.c_void_p()
    ctx._check(ctx.lib.exon_hip_bcf_parser_create(ctx.h, 2, len(sidx), 0, -1, len(body) + 4096, C.byref(h)))
    keys = (C.c_int32 * 4)(sidx["AF"], sidx["DP"], sidx["AC"], sidx["MQS"])
    ctx._check(ctx.lib.exon_hip_bcf_parser_set_info_keys(h, keys, b"fiIF", 4))
    d = ctx.to_device(np.frombuffer(body + bytes(64), np.uint8))
    cols = L.VCFColumns()
    ctx._check(ctx.lib.exon_hip_bcf_parser_parse(h, None, d.ptr, len(body), C.byref(cols)))
    n = cols.n_rows
    assert n == len(rows) and cols.n_undecided == 0 and cols.info_kinds[:4] == b"fiIF"

    def dev(ptr, dtype, count):
        out = np.empty(count, dtype)
        if count:
            ctx._check(ctx.lib.exon_hip_memcpy_d2h(ctx.h, out.ctypes.data, ptr, out.nbytes, None))
        return out

    def scalar(ptr, vptr, dtype):
        v = bits(dev(vptr, np.uint8, (n + 7) // 8), n)
        return [int(x) if ok else None for x, ok in zip(dev(ptr, dtype, n), v)]

    def lists(q, dtype):
        v, off = bits(dev(cols.infos_valid[q], np.uint8, (n + 7) // 8), n), dev(cols.list_offsets[q], np.int32, n + 1)
        total = int(off[-1])
        items, iv = dev(cols.infos[q], dtype, total), bits(dev(cols.list_item_valid[q], np.uint8, (total + 7) // 8), total)
        assert off[0] == 0 and np.all(np.diff(off) >= 0)
        return [None if not v[r] else [int(items[i]) if iv[i] else None for i in range(off[r], off[r + 1])] for r in range(n)]
    got = {"pos": scalar(cols.pos, cols.pos_valid, np.int64), "qual": scalar(cols.qual, cols.qual_valid, np.uint32),
           "AF": scalar(cols.infos[0], cols.infos_valid[0], np.uint32), "DP": scalar(cols.infos[1], cols.infos_valid[1], np.int32),
           "AC": lists(2, np.int32), "MQS": lists(3, np.uint32)}
    ctx._check(ctx.lib.exon_hip_bcf_parser_destroy(h))
    for k in want:
        bad = [(i, want[k][i], got[k][i]) for i in range(n) if want[k][i] != got[k][i]]
        assert not bad, (k, bad[:5])


@gpu
def test_bcf_typed_values_through_the_gpu_pipeline(ctx, bcf_file):
    """the same file as Arrow batches out of the GPU decode pipeline: decoded on the device, equal to the python statement.  POS, QUAL
    and the Number=1 keys: the batches of a scan that names a list-valued key are the host reader's (exon_hip_scan_bind_ctx refuses
    it), the device-built lists are the parser test's above."""
    path, rows, want = bcf_file
    got, on_gpu = scan_bcf(path, ctx, keys=("AF", "DP"))
    assert on_gpu, "silent host fallback"
    for k in got:
        bad = [(i, want[k][i], got[k][i]) for i in range(len(rows)) if want[k][i] != got[k][i]]
        assert not bad, (k, bad[:5])


def bcf_body(path):
    raw = gzip.decompress(open(path, "rb").read())
    l_text, = struct.unpack_from("<I", raw, 5)
    return raw[9 + l_text:]


class RawBCFParser:
    """exon_hip_bcf_parser_* through ctypes (no compute here): AC as List<Int32>, MQS as List<Float32>"""

    def __init__(self, ctx, max_bytes, n_strings=None):
        self.ctx, self.h = ctx, C.c_void_p()
        sidx = W.string_index([])
        ctx._check(ctx.lib.exon_hip_bcf_parser_create(ctx.h, 2, len(sidx) if n_strings is None else n_strings, 0, -1, max_bytes, C.byref(self.h)))
        ctx._check(ctx.lib.exon_hip_bcf_parser_set_info_keys(self.h, (C.c_int32 * 2)(sidx["AC"], sidx["MQS"]), b"IF", 2))

    def parse(self, d, n_bytes):
        cols = L.VCFColumns()
        self.ctx._check(self.ctx.lib.exon_hip_bcf_parser_parse(self.h, None, d.ptr, n_bytes, C.byref(cols)))
        return cols

    def dev(self, ptr, dtype, count, first=0):
        out = np.empty(count, dtype)
        if count:
            self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, out.ctypes.data, ptr + first * out.itemsize, out.nbytes, None))
        return out

    def lists(self, cols, q, dtype, row0, row1):
        """rows [row0, row1) of list key q (every list valid and without NULL items here)"""
        off = self.dev(cols.list_offsets[q], np.int32, row1 - row0 + 1, row0)
        items = self.dev(cols.infos[q], dtype, int(off[-1] - off[0]), int(off[0]))
        return [items[off[r] - off[0]:off[r + 1] - off[0]] for r in range(row1 - row0)]

    def close(self):
        self.ctx._check(self.ctx.lib.exon_hip_bcf_parser_destroy(self.h))


@gpu
def test_bcf_list_values_beyond_512_mib_into_the_slab(ctx, tmp_path):
    """A list value's location used to travel as `offset | type << 29`: from 2^29 bytes into a slab on, the offset lost its top
    bits and the type gained one.  One record with an int16 and a float vector, tiled to a little over 512 MiB with POS and both
    vectors' first items numbered per row: the rows on either side of the border decode to their own values."""
    n_items = 300
    row = dict(chrom="1", pos=1, qual=None, filter=[], info={"AC": W.Ints([0] + [1000 + i for i in range(1, n_items)], width=2),
                                                              "MQS": W.Floats([0] + [F1 + i for i in range(1, n_items)])})
    path = tmp_path / "one.bcf"
    W.write_bcf(path, [row], BGZIP, filters=[])
    rec = np.frombuffer(bcf_body(path), np.uint8)
    period = len(rec)
    ac0 = bytes(rec).index(struct.pack("<hh", 0, 1001))      # the first AC item (int16), the first MQS item (float bits)
    mq0 = bytes(rec).index(struct.pack("<II", 0, F1 + 1))
    rows = ((1 << 29) + (1 << 20)) // period + 1
    slab = np.tile(rec, rows).reshape(rows, period)
    number = np.arange(rows, dtype=np.int32)
    slab[:, 12:16] = number.view(np.uint8).reshape(rows, 4)                                    # pos0 = row
    slab[:, ac0:ac0 + 2] = (number % 30000).astype(np.int16).view(np.uint8).reshape(rows, 2)   # AC[0] = row % 30000
    slab[:, mq0:mq0 + 4] = number.view(np.uint8).reshape(rows, 4)                              # MQS[0] = the row number as float bits
    n_bytes = rows * period
    border = (1 << 29) // period
    assert n_bytes > (1 << 29) + (1 << 19) and border + 300 < rows
    p = RawBCFParser(ctx, n_bytes + 4096)
    d = ctx.to_device(np.concatenate([slab.reshape(-1), np.zeros(64, np.uint8)]))
    del slab
    cols = p.parse(d, n_bytes)
    assert cols.n_rows == rows and cols.n_undecided == 0
    for row0, row1 in ((border - 200, border + 200), (rows - 200, rows), (0, 100)):
        pos = p.dev(cols.pos, np.int64, row1 - row0, row0)
        assert pos.tolist() == list(range(row0 + 1, row1 + 1))
        for r, (ac, mq) in enumerate(zip(p.lists(cols, 0, np.int32, row0, row1), p.lists(cols, 1, np.uint32, row0, row1)), start=row0):
            assert ac.tolist() == [r % 30000] + [1000 + i for i in range(1, n_items)], r
            assert mq.tolist() == [r] + [F1 + i for i in range(1, n_items)], r
    p.close()


@gpu
def test_bcf_slab_with_an_undecided_record_reads_no_list_items(ctx, tmp_path):
    """An undecided record keeps the list count and offset its row had in the slab before: the slab is counted undecided, its list
    items are not read (they may point anywhere), and the parser decodes the next slab as if nothing had happened.  The undecided
    record: a FILTER index beyond the header's strings, in a slab of the same size as the one before it."""
    rows = [dict(chrom="1", pos=i + 1, qual=None, filter=["PASS"], info={"AC": W.Ints([i, i + 1, i + 2], width=3), "MQS": W.Floats([F1 + i] * 40)}) for i in range(600)]
    path = tmp_path / "u.bcf"
    W.write_bcf(path, rows, BGZIP, filters=[])
    good = bcf_body(path)
    bad = bytearray(good)
    k = good.index(b"\x11\x00", 32)  # the first record's FILTER vector: one int8, PASS
    bad[k + 1] = 100
    p = RawBCFParser(ctx, len(good) + 4096)
    want = [[i, i + 1, i + 2] for i in range(600)]
    for body, und in ((good, 0), (bytes(bad), 1), (good, 0)):
        d = ctx.to_device(np.frombuffer(body + bytes(64), np.uint8))
        cols = p.parse(d, len(body))
        assert cols.n_rows == 600 and cols.n_undecided == und
        if not und:
            assert [x.tolist() for x in p.lists(cols, 0, np.int32, 0, 600)] == want
    p.close()
