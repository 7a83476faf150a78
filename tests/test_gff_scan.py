"""CPU: GFF3 scans through the host reader (exon_amd/csrc/host/gff.h) against tests/gff_expect.py, the plain-Python restatement
of the line rules: the reference's slt pins (gff-scan-tests.slt) on its own fixtures, every field shape and every error shape,
the pushed-down region filter with and without a tabix index, and the reference's block-range quirk of indexed scans."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import gff_expect
from bgzf_index_writer import bgzf_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "gff")
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
REF_INDEXED = "/root/reference/exon/exon-core/test-data/datasources/gff-index/gencode.v38.polyAs.gff.gz"
EUNSUPPORTED = -4


def scan_columns(path, bind=None, **kw):
    """Every batch of a GFF scan as the columns gff_expect.columns returns (dictionary columns decoded through their values).
    bind: a Context -- the batches come out of the GPU pipeline (gpu_parse + bind_ctx); out["decoded_on_gpu"] tells how it ended."""
    s = exon_amd.Scan(str(path), "gff", gpu_parse=bind is not None, **kw)
    try:
        if bind is not None:
            s.bind_ctx(bind)
        batches = list(s)
        decoded = s.decoded_on_gpu()[0] if bind is not None else False
    finally:
        s.close()
    out = {"n_rows": sum(len(b) for b in batches), "decoded_on_gpu": decoded}

    def col(k):
        return [b.field(k) for b in batches]

    for k, name in enumerate(("seqname", "source", "type")):
        out[name] = np.array([v for a in col(k) for v in a.to_pylist()], object)
    for k, name in ((3, "start"), (4, "end")):
        assert all(a.null_count == 0 for a in col(k))
        out[name] = np.concatenate([a.to_numpy(zero_copy_only=False) for a in col(k)] or [np.zeros(0, np.int64)]).astype(np.int64)
    vals = [v for a in col(5) for v in a.to_pylist()]
    out["score_valid"] = np.array([v is not None for v in vals], bool)
    out["score"] = np.array([0.0 if v is None else v for v in vals], np.float32)
    for k, name, names in ((6, "strand", gff_expect.STRANDS), (7, "phase", gff_expect.PHASES)):
        vals = [v for a in col(k) for v in a.to_pylist()]
        out[name + "_valid"] = np.array([v is not None for v in vals], bool)
        out[name + "_id"] = np.array([0 if v is None else names.index(v) for v in vals], np.int32)
    return out


def assert_same(got, want, what=""):
    assert got["n_rows"] == want["n_rows"], what
    for name in ("seqname", "source", "type"):
        assert list(got[name]) == list(want[name]), (what, name)
    for name in ("start", "end", "strand_id", "phase_id", "score_valid", "strand_valid", "phase_valid"):
        assert np.array_equal(got[name], want[name]), (what, name)
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), (what, "score bits")


@pytest.fixture(scope="module")
def plain_fixture(tmp_path_factory):
    """the reference's test.gff (280 KB): its .gz twin inflated"""
    p = tmp_path_factory.mktemp("gff") / "test.gff"
    p.write_bytes(gzip.open(os.path.join(FIX, "test.gff.gz")).read())
    return p


def test_format_constant_and_schema(plain_fixture):
    assert exon_amd._lib.FORMATS["gff"] == 8
    assert "#define EXON_HIP_FORMAT_GFF 8" in open(os.path.join(ROOT, "include", "exon_hip.h")).read()
    s = exon_amd.Scan(str(plain_fixture), "gff")
    names = [f.name for f in s.schema()]
    s.close()
    assert names == ["seqname", "source", "type", "start", "end", "score", "strand", "phase"]


@pytest.mark.parametrize("name", ["test.gff", "test.gff.gz", "test.gff3.gz"])
def test_slt_first_row_and_count(name, plain_fixture):
    path = plain_fixture if name == "test.gff" else os.path.join(FIX, name)
    got = scan_columns(path)
    assert got["n_rows"] == 5000
    # gff-scan-tests.slt: `sq0 caat 8 13 NULL + NULL`
    assert (got["seqname"][0], got["source"][0], got["start"][0], got["end"][0]) == ("sq0", "caat", 8, 13)
    assert not got["score_valid"][0] and got["strand_valid"][0] and got["strand_id"][0] == 0 and not got["phase_valid"][0]
    assert_same(got, gff_expect.expect(open(plain_fixture, "rb").read()), name)


def test_slt_ecoli_scores_are_bit_equal():
    got = scan_columns(os.path.join(FIX, "ecoli.gff"))
    assert got["n_rows"] == 7 and got["score_valid"].all()
    want = np.array([27.0, 128.0, 152.4, 203.4, 161.6, 179.9, 111.3], np.float32)
    assert np.array_equal(got["score"].view(np.uint32), want.view(np.uint32))
    assert_same(got, gff_expect.expect(open(os.path.join(FIX, "ecoli.gff"), "rb").read()))


def test_malformed_directive_is_ignored():
    got = scan_columns(os.path.join(FIX, "bad-directive.gff"))
    assert got["n_rows"] == 7
    assert_same(got, gff_expect.expect(open(os.path.join(FIX, "bad-directive.gff"), "rb").read()))


def test_zstd_is_refused_by_name():
    with pytest.raises(exon_amd.ExonHipError) as e:
        exon_amd.Scan(os.path.join(FIX, "test.gff.zst"), "gff")
    assert e.value.code == EUNSUPPORTED and "zstd" in str(e.value)


def test_attributes_projection_is_unsupported(plain_fixture):
    lib = exon_amd.load()
    import ctypes as C
    opt = exon_amd._lib.ScanOptions(8, 0, 0, None, None, 0, 0, 1)
    h = C.c_void_p()
    assert lib.exon_hip_scan_open(str(plain_fixture).encode(), C.byref(opt), C.byref(h)) == EUNSUPPORTED
    assert b"attributes" in lib.exon_hip_last_error(None)


SHAPES = (b"##gff-version 3\n"
          b"# a comment\r\n"
          b"chr1\tsrc a\tgene\t+12\t40\t1e-5\t+\t0\tID=1\r\n"
          b"chr1\tsrc%20b\texon\t7\t+9\tinf\t-\t1\tID=2;Parent=1\n"
          b"###\n"
          b"chr2\tsrc a\tCDS\t5\t3\t.5\t.\t2\t\n"
          b"##sequence-region chr2 1\n"
          b"chr2\t.\tgene\t000123\t999999999999999999\t.\t?\t.\tID=4\twith\ttabs\n"
          b"chr10\tsrc a\tgene\t1\t1\t-3.25E2\t+\t.\tNote=no newline at the end")


def test_every_field_shape(tmp_path):
    p = tmp_path / "shapes.gff"
    p.write_bytes(SHAPES)
    want = gff_expect.expect(SHAPES)
    assert want["n_rows"] == 5 and list(want["start"]) == [12, 7, 5, 123, 1] and want["score"][1] == np.inf
    assert_same(scan_columns(p), want)
    s = exon_amd.Scan(str(p), "gff")
    list(s)
    assert s.dictionary(0) == ["chr1", "chr2", "chr10"] and s.dictionary(1) == ["src a", "src%20b", "."]
    assert s.dictionary(6) == ["+", "-"] and s.dictionary(7) == ["0", "1", "2"]
    s.close()
    gz = tmp_path / "shapes.gff.gz"
    gz.write_bytes(gzip.compress(SHAPES))
    assert_same(scan_columns(gz), want, "plain gzip")
    assert_same(scan_columns(gz, compression="gzip"), want, "compression gzip")


GOOD = b"chr1\ts\tgene\t1\t2\t.\t+\t.\tID=1\n"


@pytest.mark.parametrize("what,bad", [
    ("empty line", b"\n"), ("empty CRLF line", b"\r\n"), ("eight fields", b"chr1\ts\tgene\t1\t2\t.\t+\t.\n"),
    ("one field", b"chr1\n"), ("start 0", b"chr1\ts\tgene\t0\t2\t.\t+\t.\tx\n"), ("end 0", b"chr1\ts\tgene\t1\t0\t.\t+\t.\tx\n"),
    ("negative start", b"chr1\ts\tgene\t-1\t2\t.\t+\t.\tx\n"), ("start with a blank", b"chr1\ts\tgene\t 1\t2\t.\t+\t.\tx\n"),
    ("empty end", b"chr1\ts\tgene\t1\t\t.\t+\t.\tx\n"), ("'.' start", b"chr1\ts\tgene\t.\t2\t.\t+\t.\tx\n"),
    ("19-digit start", b"chr1\ts\tgene\t1000000000000000000\t2\t.\t+\t.\tx\n"), ("score word", b"chr1\ts\tgene\t1\t2\tabc\t+\t.\tx\n"),
    ("empty score", b"chr1\ts\tgene\t1\t2\t\t+\t.\tx\n"), ("hex score", b"chr1\ts\tgene\t1\t2\t0x10\t+\t.\tx\n"),
    ("strand word", b"chr1\ts\tgene\t1\t2\t.\tplus\t.\tx\n"), ("empty strand", b"chr1\ts\tgene\t1\t2\t.\t\t.\tx\n"),
    ("phase 3", b"chr1\ts\tgene\t1\t2\t.\t+\t3\tx\n"), ("phase 00", b"chr1\ts\tgene\t1\t2\t.\t+\t00\tx\n"),
])
def test_every_error_shape_fails_the_scan(tmp_path, what, bad):
    text = GOOD + bad + GOOD
    with pytest.raises(gff_expect.GffError):
        gff_expect.expect(text)
    p = tmp_path / "bad.gff"
    p.write_bytes(text)
    with pytest.raises(exon_amd.ExonHipError) as e:
        scan_columns(p)
    assert e.value.code < 0 and e.value.code != EUNSUPPORTED, what
    if bad.strip():
        assert bad.strip().decode()[:20] in str(e.value), "the message names the line"


def test_fasta_section_is_unsupported(tmp_path):
    text = GOOD + b"##FASTA\n>chr1\nACGT\n"
    with pytest.raises(gff_expect.GffUnsupported):
        gff_expect.expect(text)
    p = tmp_path / "fa.gff"
    p.write_bytes(text)
    with pytest.raises(exon_amd.ExonHipError) as e:
        scan_columns(p)
    assert e.value.code == EUNSUPPORTED and "##FASTA" in str(e.value)


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """gen_text gff: 200 000 rows (15 MB: the host reader decodes it slab-parallel), its text, and the expected columns"""
    p = tmp_path_factory.mktemp("gffsyn") / "s.gff"
    subprocess.check_call([GEN, "gff", "200000", str(p)])
    text = open(p, "rb").read()
    return p, text, gff_expect.records(text)


def test_gen_text_gff_covers_the_shapes(synthetic):
    _p, text, recs = synthetic
    c = gff_expect.columns(recs)
    assert text.startswith(b"##gff-version 3\n") and text.count(b"\n###\n") == 199 and text.count(b"\n# ") >= 20
    assert c["n_rows"] == 200_000 and len(c["seqname_names"]) == 24 and len(c["type_names"]) == 10 and len(c["source_names"]) == 3
    assert 0.1 < c["score_valid"].mean() < 0.9 and 0.3 < c["strand_valid"].mean() < 0.7 and 0.6 < c["phase_valid"].mean() < 0.9
    assert set(c["strand_id"][c["strand_valid"]]) == {0, 1} and set(c["phase_id"][c["phase_valid"]]) == {0, 1, 2}
    for ch in (b"\t.\tID", b"\t?\t", b"\t.\t.\tID"):
        assert ch in text
    # sorted by (seqname, start): every seqname is one run, starts ascend inside it
    ids = c["seqname_id"]
    assert (np.diff(ids) >= 0).all() and all((np.diff(c["start"][ids == k]) > 0).all() for k in range(24))


def test_parallel_reader_equals_expect_and_the_sequential_reader(synthetic, monkeypatch):
    p, _text, recs = synthetic
    want = gff_expect.columns(recs)
    got = scan_columns(p)
    assert_same(got, want, "slab-parallel")
    s = exon_amd.Scan(str(p), "gff")
    n = [len(b) for b in s]
    assert s.dictionary(0) == want["seqname_names"] and s.dictionary(1) == want["source_names"] and s.dictionary(2) == want["type_names"]
    s.close()
    assert max(n) <= 8192 and sum(n) == 200_000
    monkeypatch.setenv("EXON_HIP_DECODE_THREADS", "1")
    assert_same(scan_columns(p), want, "sequential")
    s = exon_amd.Scan(str(p), "gff")
    assert [len(b) for b in s][:3] == [8192, 8192, 8192]
    s.close()


REGIONS = ["chr1", "chr7:100000-300000", "chr7:250000", "chrY:1-50", "chr3:99999999-100000000", "chrM", "chr2:1-1"]


def test_region_without_index_is_the_readers_filter(synthetic):
    p, _text, recs = synthetic
    for region in REGIONS:
        rg = gff_expect.parse_region(region)
        want = gff_expect.columns([r for r in recs if gff_expect.hit(r, rg)])
        assert_same(scan_columns(p, region=region), want, region)
    assert scan_columns(p, region="chrM")["n_rows"] == 0 and scan_columns(p, region="chr7:100000-300000")["n_rows"] > 1000


@pytest.fixture(scope="module")
def indexed(tmp_path_factory):
    """a bgzipped gen_text gff file of 60 000 rows (more than 50 BGZF blocks) with a tabix index from gff_expect's writer"""
    d = tmp_path_factory.mktemp("gffidx")
    p, gz = d / "s.gff", d / "s.gff.gz"
    subprocess.check_call([GEN, "gff", "60000", str(p)])
    subprocess.check_call([BGZIP, str(p), str(gz), "6"])
    assert gff_expect.write_gff_tabix(gz) == 60_000 and len(bgzf_blocks(open(gz, "rb").read())) > 50
    return gz, gff_expect.records(open(p, "rb").read())


INDEXED_REGIONS = ["chr1", "chr2", "chr7:100000-200000", "chr12:1-5000", "chrY", "chrY:249000-250100", "chr5:240000", "chrM", "chr3:260000-270000"]


def test_indexed_scan_equals_brute_force(indexed):
    gz, recs = indexed
    hdr, names, _ = gff_expect.read_tabix(str(gz) + ".tbi")
    assert (hdr["col_seq"], hdr["col_beg"], hdr["col_end"]) == (1, 4, 5) and len(names) == 24
    for region in INDEXED_REGIONS:
        rg = gff_expect.parse_region(region)
        want = [r for r in recs if gff_expect.hit(r, rg)]
        assert gff_expect.indexed_records(gz, rg) == want, region  # (the restated planner loses nothing either)
        s = exon_amd.Scan(str(gz), "gff", region=region, use_index=True)
        n = sum(len(b) for b in s)
        chunks = s.index_chunks()
        s.close()
        assert n == len(want) and (chunks >= 1 or not want), region
        assert_same(scan_columns(gz, region=region, use_index=True), gff_expect.columns(want), region)
    assert scan_columns(gz, region="chrM", use_index=True)["n_rows"] == 0


def test_reference_quirk_reads_whole_blocks_only(indexed, monkeypatch):
    gz, recs = indexed
    monkeypatch.setenv("EXON_HIP_REFERENCE_QUIRKS", "1")
    differs = 0
    for region in ("chr1", "chr7:100000-200000", "chrY:249000-250100", "chrM"):
        rg = gff_expect.parse_region(region)
        want = gff_expect.indexed_records(gz, rg, reference_quirk=True)
        full = [r for r in recs if gff_expect.hit(r, rg)]
        assert_same(scan_columns(gz, region=region, use_index=True), gff_expect.columns(want), region)
        # (fewer rows where a chunk's last block is cut off; MORE where a chunk lies inside one block: that range runs to the end of
        # the file, over records other chunks return as well)
        differs += len(want) != len(full)
        # without use_index the switch changes nothing
        assert scan_columns(gz, region=region)["n_rows"] == len(full)
    assert differs >= 1


def test_index_with_another_preset_is_refused(indexed, tmp_path):
    import shutil
    import struct
    gz, _ = indexed
    mine = tmp_path / "s.gff.gz"
    shutil.copy(gz, mine)
    raw = bytearray(gzip.open(str(gz) + ".tbi").read())
    struct.pack_into("<3i", raw, 12, 1, 2, 0)  # the VCF preset's columns
    with gzip.open(str(mine) + ".tbi", "wb") as fh:
        fh.write(bytes(raw))
    with pytest.raises(exon_amd.ExonHipError) as e:
        exon_amd.Scan(str(mine), "gff", region="chr1", use_index=True)
    assert "preset" in str(e.value)


@pytest.mark.skipif(not os.path.exists(REF_INDEXED), reason=f"the reference's indexed GFF fixture is not at {REF_INDEXED}")
def test_restated_block_range_rule_on_the_references_fixture():
    """gff-scan-tests.slt expects 8786 (chr1) and 7091 (chr2) from gff_indexed_scan over a file that holds 8813 and 7223: the
    restated rule (whole blocks in front of the chunk end's block, the cut line dropped) gives exactly those."""
    text = gzip.open(REF_INDEXED).read()
    recs = gff_expect.records(text)
    for name, every, quirk in (("chr1", 8813, 8786), ("chr2", 7223, 7091)):
        rg = gff_expect.parse_region(name)
        assert sum(gff_expect.hit(r, rg) for r in recs) == every
        assert len(gff_expect.indexed_records(REF_INDEXED, rg)) == every
        assert len(gff_expect.indexed_records(REF_INDEXED, rg, reference_quirk=True)) == quirk
