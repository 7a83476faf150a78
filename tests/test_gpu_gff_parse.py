"""GPU-side GFF3 parsing (exon_hip_gff_parser_*, k_parse_gff_lines) and the GFF file pipeline: text in HBM -> the GFF device
layout -> K2 / K6 / K7, against tests/gff_expect.py (the plain-Python restatement of the line rules), the host reader, and the
one-shot operators on hand-pushed columns."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import gff_expect
from test_gff_scan import FIX, SHAPES, assert_same, scan_columns

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
ESTATE = -5


def bits(bitmap, n):
    return np.unpackbits(bitmap, bitorder="little")[:n].astype(bool)


def device_columns(res, parser):
    """parse_host's result in gff_expect.columns' form: ids through the parser's names"""
    n = res["n_rows"]
    out = {"n_rows": n}
    for k, name in enumerate(("seqname", "source", "type")):
        names = np.array(parser.names(k) + [None], object)
        assert (res[name + "_id"] >= 0).all() and (res[name + "_id"] < len(names) - 1).all()
        out[name] = names[res[name + "_id"]]
    for name in ("start", "end", "score"):
        out[name] = res[name]
    for name in ("score", "strand", "phase"):
        out[name + "_valid"] = bits(res[name + "_valid"], n)
    # NULL slots hold defined values: 0
    out["score"] = np.where(out["score_valid"], out["score"], np.float32(0)).astype(np.float32)
    assert (res["score"][~out["score_valid"]] == 0).all()
    for name in ("strand", "phase"):
        assert (res[name + "_id"][~out[name + "_valid"]] == 0).all()
        out[name + "_id"] = res[name + "_id"]
    return out


def check(ctx, text, misalign=0, parser=None, want=None):
    own = parser is None
    parser = parser or exon_amd.GFFParser(ctx)
    res = parser.parse_host(text, misalign=misalign)
    assert res["n_undecided"] == 0
    last = text.rfind(b"\n") + 1
    assert res["consumed_bytes"] == last
    assert_same(device_columns(res, parser), want or gff_expect.expect(text[:last]), f"misalign {misalign}")
    if own:
        parser.close()
    return res


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    p = tmp_path_factory.mktemp("gffgpu") / "s.gff"
    subprocess.check_call([GEN, "gff", "200000", str(p)])
    text = open(p, "rb").read()
    return p, text, gff_expect.expect(text)


def test_parser_on_the_reference_fixtures(ctx):
    for text in (gzip.open(os.path.join(FIX, "test.gff.gz")).read(), open(os.path.join(FIX, "ecoli.gff"), "rb").read(),
                 open(os.path.join(FIX, "bad-directive.gff"), "rb").read()):
        check(ctx, text)
    res = check(ctx, open(os.path.join(FIX, "ecoli.gff"), "rb").read())
    assert np.array_equal(res["score"].view(np.uint32), np.array([27.0, 128.0, 152.4, 203.4, 161.6, 179.9, 111.3], np.float32).view(np.uint32))


def test_parser_field_shapes(ctx):
    """CRLF, '+' positions, .5 / 1e-5 scores, tabs inside the ninth field, end < start, an empty ninth field; the row with an `inf`
    score is the host reader's (Eisel-Lemire leaves the word open)"""
    lines = SHAPES.split(b"\n")
    decided = b"\n".join(ln for ln in lines if b"\tinf\t" not in ln) + b"\n"
    check(ctx, decided)
    p = exon_amd.GFFParser(ctx)
    assert p.parse_host(SHAPES + b"\n")["n_undecided"] == 1
    p.close()


def test_parser_200k_rows_ranked_rows_and_both_alignments(ctx, synthetic):
    _p, text, want = synthetic
    assert text.count(b"\n#") > 200  # '#' lines all over the slab: rows are ranks, not line numbers
    for misalign in (0, 5):
        check(ctx, text, misalign=misalign, want=want)


def test_parser_every_misalignment_identity_and_ranked(ctx, synthetic):
    _p, text, _want = synthetic
    lines = text.split(b"\n")
    plain = b"\n".join(ln for ln in lines[1:700] if not ln.startswith(b"#")) + b"\n"  # no '#' line: row = line, validity by ballot
    ranked = b"\n".join(lines[990:2100]) + b"\n"                                       # '###' and a comment in the middle
    assert b"\n#" not in plain and not plain.startswith(b"#") and ranked.count(b"\n#") >= 2
    for slab in (plain, ranked):
        want = gff_expect.expect(slab)
        parser = exon_amd.GFFParser(ctx)
        for misalign in range(16):
            check(ctx, slab, misalign=misalign, parser=parser, want=want)
        parser.close()
    # 1 .. 130 rows: the last wave's bitmap bytes, a slab of one line
    for n in (1, 7, 8, 9, 63, 64, 65, 130):
        check(ctx, b"\n".join(plain.split(b"\n")[:n]) + b"\n")
        check(ctx, b"# head\n" + b"\n".join(plain.split(b"\n")[:n]) + b"\n", misalign=3)


def test_parser_slab_cut_inside_a_line(ctx, synthetic):
    _p, text, _want = synthetic
    head = text[:300_000]
    for cut in (len(head), len(head) - 1, head.rfind(b"\n") + 1, head.rfind(b"\n") + 2, head.rfind(b"\n")):
        res = check(ctx, head[:cut])
        assert 0 < res["consumed_bytes"] <= cut and head[res["consumed_bytes"] - 1:res["consumed_bytes"]] == b"\n"
    p = exon_amd.GFFParser(ctx)
    res = p.parse_host(b"chr1\ts\tgene\t1\t2")  # not one whole line
    assert (res["n_rows"], res["n_undecided"], res["consumed_bytes"]) == (0, 0, 0)
    p.close()


def test_parser_dictionaries_grow_across_slabs_and_seeds_keep_their_ids(ctx, synthetic):
    _p, text, _want = synthetic
    cut = text.rfind(b"\n", 0, len(text) // 3) + 1
    a, b = text[:cut], text[cut:]
    parser = exon_amd.GFFParser(ctx, seed_seqnames=["chrY", "chrM", "chr3"])
    check(ctx, a, parser=parser)
    n_a = [list(parser.names(k)) for k in range(3)]
    assert n_a[0][:3] == ["chrY", "chrM", "chr3"] and 3 < len(n_a[0]) < 24
    res = check(ctx, b, misalign=9, parser=parser)
    n_b = [list(parser.names(k)) for k in range(3)]
    for k in range(3):
        assert n_b[k][:len(n_a[k])] == n_a[k]  # ids handed out stay
    assert sorted(n_b[0]) == sorted(set(gff_expect.expect(text)["seqname_names"]) | {"chrM"}) and len(n_b[2]) == 10 and len(n_b[1]) == 3
    got = device_columns(res, parser)
    assert (res["seqname_id"][got["seqname"] == "chrY"] == 0).all() and (got["seqname"] == "chrY").sum() > 1000
    assert (res["seqname_id"][got["seqname"] == "chr3"] == 2).all() and 1 not in res["seqname_id"]
    parser.close()


GOOD = b"chr1\ts\tgene\t1\t2\t.\t+\t.\tID=1\n"


@pytest.mark.parametrize("what,bad", [
    ("20-digit start", b"chr1\ts\tgene\t10000000000000000000\t2\t.\t+\t.\tx\n"), ("19-digit end", b"chr1\ts\tgene\t1\t1000000000000000000\t.\t+\t.\tx\n"),
    ("bad strand", b"chr1\ts\tgene\t1\t2\t.\tx\t.\tx\n"), ("short line", b"chr1\ts\tgene\t1\t2\t.\t+\t.\n"), ("one field", b"chr1\n"),
    ("empty line", b"\n"), ("##FASTA", b"##FASTA\n"), ("start 0", b"chr1\ts\tgene\t0\t2\t.\t+\t.\tx\n"), ("phase 3", b"chr1\ts\tgene\t1\t2\t.\t+\t3\tx\n"),
    ("score word", b"chr1\ts\tgene\t1\t2\tabc\t+\t.\tx\n"), ("20-digit score", b"chr1\ts\tgene\t1\t2\t0.12345678901234567890\t+\t.\tx\n"),
    ("inf score", b"chr1\ts\tgene\t1\t2\tinf\t+\t.\tx\n"),
])
def test_rows_the_device_cannot_decide_are_counted(ctx, what, bad):
    parser = exon_amd.GFFParser(ctx)
    for text in (GOOD * 70 + bad + GOOD * 70, bad + GOOD, GOOD + bad, b"# c\n" + GOOD * 3 + bad):
        res = parser.parse_host(text, misalign=2)
        assert res["n_undecided"] >= 1, what
        assert res["consumed_bytes"] == len(text)
    parser.close()
    check(ctx, GOOD * 70 + b"##FASTQ is no section\n" + GOOD)


def test_the_4097th_seqname_hands_the_slab_over(ctx):
    def slab(n):
        return b"".join(b"contig_%d\tsrc\tgene\t%d\t%d\t.\t+\t.\tID=%d\n" % (i, i + 1, i + 9, i) for i in range(n))
    parser = exon_amd.GFFParser(ctx)
    res = check(ctx, slab(4096), parser=parser)
    assert len(parser.names(0)) == 4096 and sorted(res["seqname_id"]) == list(range(4096))
    parser.close()
    parser = exon_amd.GFFParser(ctx)
    assert parser.parse_host(slab(4097))["n_undecided"] >= 1
    parser.close()
    # the same for source and type, and for the text pool (1 MiB)
    parser = exon_amd.GFFParser(ctx)
    text = b"".join(b"c\tsrc%d\tgene\t1\t2\t.\t+\t.\tx\n" % i for i in range(4097))
    assert parser.parse_host(text)["n_undecided"] >= 1
    parser.close()
    parser = exon_amd.GFFParser(ctx)
    text = b"".join(b"c\ts\t%s%d\t1\t2\t.\t+\t.\tx\n" % (b"t" * 600, i) for i in range(2000))
    assert parser.parse_host(text)["n_undecided"] >= 1
    parser.close()


# ---- the file pipeline ---------------------------------------------------------------------------------------------------

REGIONS = [("chr1", 1, None), ("chr7", 1_000_000, 2_000_000), ("chr12", 3_000_000, 3_000_500), ("chrY", 1, 77), ("chrM", 1, None), ("chr3", 4_100_000, None)]


@pytest.fixture(scope="module")
def million(tmp_path_factory):
    """a 1 M-row gen_text gff file as plain text, BGZF and plain gzip, and its (seqname, start, end) columns"""
    d = tmp_path_factory.mktemp("gffpipe")
    p, bgz, gz = d / "m.gff", d / "m.gff.bgz.gz", d / "m.gff.gz"
    subprocess.check_call([GEN, "gff", "1000000", str(p)])
    subprocess.check_call([BGZIP, str(p), str(bgz), "6"])
    text = open(p, "rb").read()
    with gzip.open(gz, "wb", compresslevel=1) as fh:
        fh.write(text)
    return {"plain": p, "bgzf": bgz, "gzip": gz}, gff_expect.interval_columns(text)


def run_plan(ctx, path, kind, region, gpu_parse, want_inflated=None):
    name, a, b = region
    scan = exon_amd.Scan(str(path), "gff", gpu_parse=gpu_parse)
    plan = {"k2": lambda: ctx.plan_region_count(0, a, b, columns=(0, 3)), "k6": lambda: ctx.plan_overlap_count(0, a, b, columns=(0, 3, 4)),
            "k7": lambda: ctx.plan_within_count(0, a, b, columns=(0, 3, 4))}[kind]()
    st = plan.open()
    st.set_region_contig(name)
    rows = st.consume(scan)
    counts, _ = st.finish()
    decoded, inflated = scan.decoded_on_gpu()
    assert decoded == bool(gpu_parse), "silent host fallback"
    if gpu_parse and want_inflated is not None:
        assert inflated == want_inflated
    st.close(); plan.close(); scan.close()
    return rows, int(counts[0])


def test_pipeline_agrees_four_ways(ctx, million, monkeypatch):
    paths, (names, ids, start, end) = million
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "16")  # several slabs per file: lines carried across them
    n = len(ids)
    d_ids, d_start, d_end = ctx.to_device(ids), ctx.to_device(start), ctx.to_device(end)
    big = 2**63 - 1
    for region in REGIONS:
        name, a, b = region
        rid = names.index(name) if name in names else -1
        hi = big if b is None else b
        sel = ids == rid
        want = {"k2": int((sel & (start >= a) & (start <= hi)).sum()), "k6": int((sel & (start <= hi) & (end >= a)).sum()),
                "k7": int((sel & (start > a) & (end < hi)).sum())}
        for kind in ("k2", "k6", "k7"):
            d_count = ctx.zeros(np.int64, 1)
            op = {"k2": lambda: ctx.region_count(d_ids, d_start, n, rid, a, b, d_count),
                  "k6": lambda: ctx.overlap_count(d_ids, None, d_start, None, d_end, None, n, rid, a, b, d_count),
                  "k7": lambda: ctx.within_count(d_ids, None, d_start, None, d_end, None, n, rid, a, b, d_count)}[kind]
            op()
            ctx.sync()
            by_hand = int(d_count.to_host()[0])
            host = run_plan(ctx, paths["plain"], kind, region, False)
            assert host == (n, want[kind]) and by_hand == want[kind], (region, kind)
            for twin in (("plain", "bgzf", "gzip") if kind == "k6" or region is REGIONS[1] else ("plain",)):
                got = run_plan(ctx, paths[twin], kind, region, True, want_inflated=twin != "plain")
                assert got == (n, want[kind]), (region, kind, twin)
    assert want["k2"] > 0


def test_pushed_down_region_and_indexed_scan_on_the_device(ctx, million, tmp_path):
    paths, (names, ids, start, end) = million
    assert gff_expect.write_gff_tabix(paths["bgzf"]) == len(ids)
    for region, (name, a, b) in [("chr7:1000000-2000000", ("chr7", 1_000_000, 2_000_000)), ("chr2", ("chr2", 1, 2**62)), ("chrM", ("chrM", 1, 2**62))]:
        rid = names.index(name) if name in names else -1
        kept = (ids == rid) & (start >= a) & (start <= b)
        want_k6 = int((kept & (end >= 1_500_000)).sum())
        for use_index in (False, True):
            for gpu_parse in (True, False):
                scan = exon_amd.Scan(str(paths["bgzf"]), "gff", region=region, use_index=use_index, gpu_parse=gpu_parse)
                plan = ctx.plan_overlap_count(0, 1_500_000, None, columns=(0, 3, 4))
                st = plan.open()
                st.set_region_contig(name)
                rows = st.consume(scan)
                counts, _ = st.finish()
                assert scan.decoded_on_gpu() == (gpu_parse, gpu_parse)
                st.close(); plan.close(); scan.close()
                assert (rows, int(counts[0])) == (int(kept.sum()), want_k6), (region, use_index, gpu_parse)


def test_batches_from_the_gpu_pipeline_equal_the_host_readers(ctx, synthetic, tmp_path, monkeypatch):
    p, _text, want = synthetic
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "4")
    bgz = tmp_path / "s.gff.gz"
    subprocess.check_call([BGZIP, str(p), str(bgz), "6"])

    for path in (p, bgz):
        got = scan_columns(path, bind=ctx)
        assert got["decoded_on_gpu"] and got["n_rows"] == 200_000
        assert_same(got, want, str(path))
    host = scan_columns(p, region="chr7:100000-300000")
    got = scan_columns(p, bind=ctx, region="chr7:100000-300000")
    assert got["decoded_on_gpu"] and host["n_rows"] > 1000
    assert_same(got, host, "pushed-down region")
    # an undecidable row in a later slab: the host reader takes over behind the rows emitted; nothing is lost or doubled
    text = open(p, "rb").read()
    broken = tmp_path / "inf.gff"
    cut = text.rfind(b"\n", 0, 9_000_000) + 1
    broken.write_bytes(text[:cut] + b"chr20\ts\tgene\t1\t2\tinf\t+\t.\tx\n" + text[cut:])
    got = scan_columns(broken, bind=ctx)
    assert not got["decoded_on_gpu"]
    s = exon_amd.Scan(str(broken), "gff", gpu_parse=True).bind_ctx(ctx)
    assert sum(len(b) for b in s) == 200_001 and sorted(s.dictionary(0)) == sorted(want["seqname_names"]) and len(s.dictionary(2)) == 10
    s.close()
    s = exon_amd.Scan(str(p), "gff", gpu_parse=True).bind_ctx(ctx)
    assert sum(len(b) for b in s) == 200_000 and sorted(s.dictionary(0)) == sorted(want["seqname_names"]) and len(s.dictionary(1)) == 3
    s.close()
    assert_same(got, scan_columns(broken), "hand-over")
    assert got["n_rows"] == 200_001


def test_5000_seqnames_finish_through_the_hand_over(ctx, tmp_path, monkeypatch):
    p = tmp_path / "many.gff"
    p.write_bytes(b"##gff-version 3\n" + b"".join(b"contig_%d\tsrc\tgene\t%d\t%d\t0.5\t-\t1\tID=%d\n" % (i % 5000, i + 1, i + 50, i) for i in range(20_000)))

    def k6(gpu_parse):
        scan = exon_amd.Scan(str(p), "gff", gpu_parse=gpu_parse)
        plan = ctx.plan_overlap_count(0, 100, 12_000, columns=(0, 3, 4))
        st = plan.open()
        st.set_region_contig("contig_77")
        try:
            rows = st.consume(scan)
            counts, _ = st.finish()
            return rows, int(counts[0]), scan.decoded_on_gpu()[0]
        finally:
            st.close(); plan.close(); scan.close()

    want = sum(1 for i in range(20_000) if i % 5000 == 77 and i + 1 <= 12_000 and i + 50 >= 100)
    assert k6(False) == (20_000, want, False) and want == 3
    assert k6(True) == (20_000, want, False)  # the device hands the file over: the host path's answer, never a wrong id
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_STRICT", "1")
    with pytest.raises(exon_amd.ExonHipError) as e:
        k6(True)
    assert e.value.code == ESTATE and "EXON_HIP_GPU_PARSE_STRICT" in str(e.value)
