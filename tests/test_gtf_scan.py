"""CPU: GTF scans through the host reader (exon_amd/csrc/host/gtf.h) against tests/gtf_expect.py, the plain-Python restatement of
the rules: the reference's slt pins (gtf-scan-tests.slt) on its two fixtures, a ninth field per attribute rule and per error, the
line rules (where GTF parts from GFF3 included), threads, batch sizes, the region filter, and what stays refused."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import exon_amd
import gtf_expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "gtf")
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
EUNSUPPORTED = -4
PREFIX = b"chr1\thavana\texon\t11869\t12227\t.\t+\t.\t"


def scan_gtf(path, bind=None, attributes=True, fmt="gtf", **kw):
    """Every batch of a scan as the columns gtf_expect.columns returns (dictionary columns decoded through their values), the rows'
    maps as to_pylist() gives them (out["maps"]) and the batches' row counts (out["sizes"]); every batch is validated in full.
    bind: a Context -- the batches come out of the GPU pipeline (gpu_parse + bind_ctx); out["decoded_on_gpu"] tells how it ended."""
    s = exon_amd.Scan(str(path), fmt, gpu_parse=bind is not None, project=("attributes",) if attributes else (), **kw)
    try:
        if bind is not None:
            s.bind_ctx(bind)
        batches = list(s)
        decoded = s.decoded_on_gpu()[0] if bind is not None else False
    finally:
        s.close()
    out = {"n_rows": sum(len(b) for b in batches), "decoded_on_gpu": decoded, "sizes": [len(b) for b in batches]}
    for b in batches:
        b.validate(full=True)
        assert b.type.num_fields == (9 if attributes else 8)

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
    for k, name, names in ((6, "strand", gtf_expect.STRANDS), (7, "frame", gtf_expect.FRAMES)):
        vals = [v for a in col(k) for v in a.to_pylist()]
        out[name + "_valid"] = np.array([v is not None for v in vals], bool)
        out[name + "_id"] = np.array([0 if v is None else names.index(v) for v in vals], np.int32)
    if attributes:
        assert all(a.null_count == 0 for a in col(8))
        out["maps"] = [m for a in col(8) for m in a.to_pylist()]
    return out


def assert_same(got, want, what=""):
    assert got["n_rows"] == want["n_rows"], what
    for name in ("seqname", "source", "type"):
        assert list(got[name]) == list(want[name]), (what, name)
    for name in ("start", "end", "strand_id", "frame_id", "score_valid", "strand_valid", "frame_valid"):
        assert np.array_equal(got[name], want[name]), (what, name)
    assert np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32)), (what, "score bits")
    if "maps" in want:
        assert got["maps"] == want["maps"], (what, "attributes")


def fixture_text(name):
    p = os.path.join(FIX, name)
    return gzip.open(p).read() if name.endswith(".gz") else open(p, "rb").read()


def test_format_constant_and_schema():
    hdr = open(os.path.join(ROOT, "include", "exon_hip.h")).read()
    assert exon_amd._lib.FORMATS["gtf"] == 9 and "#define EXON_HIP_FORMAT_GTF 9" in hdr
    assert "#define EXON_HIP_PROJECT_GTF_ATTRIBUTES 256ull" in hdr
    s = exon_amd.Scan(os.path.join(FIX, "test.gtf"), "gtf")
    assert [f.name for f in s.schema()] == ["seqname", "source", "type", "start", "end", "score", "strand", "frame"]
    s.close()
    s = exon_amd.Scan(os.path.join(FIX, "test.gtf"), "gtf", project=("attributes",))
    t = s.schema()
    f = t.field(8)
    assert f.name == "attributes" and not f.nullable and f.type == pa.map_(pa.string(), pa.string()) and not f.type.keys_sorted
    assert not f.type.key_field.nullable and f.type.item_field.nullable
    # (pyarrow's importer renames a map's fields: the reference's names and the format are read off the C schema)
    sch = exon_amd._lib.ArrowSchema()
    s._check(s.lib.exon_hip_scan_schema(s.h, C.byref(sch)))
    m = sch.children[8].contents
    entries = m.children[0].contents
    keys, values = entries.children[0].contents, entries.children[1].contents
    NULLABLE, KEYS_SORTED = 2, 4
    assert (m.format, m.name, m.flags & (NULLABLE | KEYS_SORTED), m.n_children) == (b"+m", b"attributes", 0, 1)
    assert (entries.format, entries.name, entries.flags & NULLABLE, entries.n_children) == (b"+s", b"entries", 0, 2)
    assert (keys.format, keys.name, keys.flags & NULLABLE) == (b"u", b"keys", 0)
    assert (values.format, values.name, values.flags & NULLABLE) == (b"u", b"values", NULLABLE)
    pa.DataType._import_from_c(C.addressof(sch))  # (releases it)
    s.close()


@pytest.mark.parametrize("name", ["test.gtf", "test.gtf.gz"])
def test_slt_pins_and_every_column(name):
    got = scan_gtf(os.path.join(FIX, name))
    assert got["n_rows"] == 77 and got["sizes"] == [77]
    # gtf-scan-tests.slt: `chr1 processed_transcript exon 11869 12227 NULL + NULL`
    assert (got["seqname"][0], got["source"][0], got["type"][0], got["start"][0], got["end"][0]) == ("chr1", "processed_transcript", "exon", 11869, 12227)
    assert not got["score_valid"][0] and got["strand_valid"][0] and got["strand_id"][0] == 0 and not got["frame_valid"][0]
    assert got["strand_valid"].all() and int((got["strand_id"] == 0).sum()) == 22 and int((got["strand_id"] == 1).sum()) == 55
    assert not got["score_valid"].any() and not got["frame_valid"].any()
    assert got["maps"][0] == [("gene_id", "ENSG00000223972"), ("transcript_id", "ENST00000456328"), ("exon_number", "1"), ("gene_name", "DDX11L1"),
                              ("gene_biotype", "pseudogene"), ("transcript_name", "DDX11L1-002"), ("exon_id", "ENSE00002234944")]
    assert_same(got, gtf_expect.expect(fixture_text(name), attrs=True), name)
    # without the column the eight others are the same
    assert_same(scan_gtf(os.path.join(FIX, name), attributes=False), gtf_expect.expect(fixture_text(name)), name)


def test_the_gz_fixture_is_a_plain_gzip_member_with_a_name():
    raw = open(os.path.join(FIX, "test.gtf.gz"), "rb").read()
    assert raw[:3] == b"\x1f\x8b\x08" and raw[3] & 8 and not raw[3] & 4  # FNAME, no FEXTRA: not BGZF
    assert gzip.decompress(raw) == open(os.path.join(FIX, "test.gtf"), "rb").read()


# one ninth field per rule of host/gtf.h's ATTRIBUTE RULES: (field 9, the map it gives | None for an error)
RULES = [
    (b"", []),                                                                        # "" is a map of 0 entries
    (b'gene_id "G1";', [("gene_id", "G1")]),
    (b'gene_id "G1"', [("gene_id", "G1")]),                                           # the last ';' may be missing
    (b'gene_id "G1"; transcript_id "T1";', [("gene_id", "G1"), ("transcript_id", "T1")]),
    (b'note "a;b; c";x "y"', [("note", "a;b; c"), ("x", "y")]),                       # ';' and spaces inside quotes are the value's
    (b'note "";', [("note", "")]),                                                    # "" as a value
    (b'exon_number 3;', [("exon_number", "3")]),                                      # a bare value
    (b'exon_number 3', [("exon_number", "3")]),
    (b'level 2  ; k v w  ;', [("level", "2"), ("k", "v w")]),                         # a bare value runs to the ';', trailing spaces dropped
    (b'k a"b;j "c', None),                                                            # (a bare value keeps a '"'; j's quote never closes)
    (b'k a"b;', [("k", 'a"b')]),
    (b'gene_id "G1"; ', [("gene_id", "G1")]),                                         # a trailing "; "
    (b'gene_id "G1";   ', [("gene_id", "G1")]),
    (b'gene_id    "G1"  ;   x   1', [("gene_id", "G1"), ("x", "1")]),                 # one or more spaces; optional ones in front of ';' and behind it
    (b'  k "v"', [("k", "v")]),                                                       # spaces in front of the first key
    (b'   ', []),                                                                     # spaces alone
    (b'tag "basic"; tag "CCDS"; tag "basic";', [("tag", "basic"), ("tag", "CCDS"), ("tag", "basic")]),  # repeated keys stay, in file order
    (b'k "a%3Bb"; j %41', [("k", "a%3Bb"), ("j", "%41")]),                            # nothing is percent-decoded
    (b'k "v\tw"', [("k", "v\tw")]),                                                   # a TAB behind the eighth is a byte like any other
    (b'"q" "v"', [('"q"', "v")]),                                                     # only a value is unquoted
    (b'k "caf\xc3\xa9"; caf\xc3\xa9 1', [("k", "café"), ("café", "1")]),    # UTF-8
    (b'gene_id "G1', None),                                                           # a missing closing quote
    (b'gene_id "G1; x "y";', None),                                                   # (the quote closes at x's: `y";` follows it)
    (b'gene_id', None),                                                               # a key with no value
    (b'gene_id ', None),
    (b'gene_id;', None),
    (b'gene_id ;', None),
    (b'a "b"; gene_id', None),
    (b'k\tv', None),                                                                  # (a TAB is no space: a key alone)
    (b';', None),                                                                     # an empty piece: a leading ';'
    (b'a "b";;', None),                                                               # ";;"
    (b'a b;;c d', None),
    (b'a "b"; ;', None),
    (b'a "b"x;', None),                                                               # bytes behind a closing quote
    (b'a "b" c "d";', None),
    (b'k "\xff"', None),                                                              # no UTF-8 in a value
    (b'\xc3 "v"', None),                                                              # ... in a key
    (b'k \xed\xa0\x80', None),                                                        # (a surrogate)
]
GOOD = [(f, m) for f, m in RULES if m is not None]
ASCII_GOOD = [(f, m) for f, m in GOOD if max(f, default=0) < 0x80]
RULE_TEXT = b"#!genome-build x\n" + b"".join(PREFIX + f + (b"\r\n" if i % 3 == 0 else b"\n") for i, (f, m) in enumerate(GOOD))


def test_the_rule_table_in_the_restatement():
    for f, m in RULES:
        if m is None:
            with pytest.raises(gtf_expect.GtfError):
                gtf_expect.attributes(f)
        else:
            assert gtf_expect.attributes(f) == m, f
    assert gtf_expect.expect(RULE_TEXT, attrs=True)["maps"] == [m for _, m in GOOD]


def test_a_row_per_rule(tmp_path):
    p = tmp_path / "rules.gtf"
    p.write_bytes(RULE_TEXT)
    got = scan_gtf(p)
    assert got["maps"] == [m for _, m in GOOD]
    assert_same(got, gtf_expect.expect(RULE_TEXT, attrs=True))
    for bs in (1, 7):
        assert scan_gtf(p, batch_size=bs)["maps"] == got["maps"]


@pytest.mark.parametrize("k", [i for i, (f, m) in enumerate(RULES) if m is None])
def test_a_file_per_error(k, tmp_path):
    field = RULES[k][0]
    line = PREFIX + field
    p = tmp_path / "bad.gtf"
    p.write_bytes(PREFIX + b'gene_id "ok";\n' + line + b"\n")
    with pytest.raises(exon_amd.ExonHipError) as e:
        scan_gtf(p)
    assert "GTF line" in str(e.value) and line[:60].decode(errors="replace") in str(e.value)
    # the field is not looked at without the column ...
    assert scan_gtf(p, attributes=False)["n_rows"] == 2
    # ... and with it every record is validated, kept by a filter or not
    with pytest.raises(exon_amd.ExonHipError):
        scan_gtf(p, region="chrNone")


def write(tmp_path, text, name="t.gtf"):
    p = tmp_path / name
    p.write_bytes(text)
    return p


def test_question_mark_strand_is_an_error_for_gtf_only(tmp_path):
    line = b"chr1\ts\texon\t1\t2\t.\t?\t.\t"
    p = write(tmp_path, line + b'k "v";\n')
    with pytest.raises(exon_amd.ExonHipError) as e:
        scan_gtf(p)
    assert "invalid strand '?'" in str(e.value) and "GTF line 'chr1\ts\texon" in str(e.value)
    with pytest.raises(gtf_expect.GtfError):
        gtf_expect.expect(line + b'k "v";\n')
    g = write(tmp_path, line + b"ID=1\n", "t.gff")
    got = scan_gtf(g, attributes=False, fmt="gff")  # the GFF3 reader still reads it, as NULL
    assert got["n_rows"] == 1 and not got["strand_valid"][0]
    # '.' is NULL in both; the frame column takes '.', 0, 1, 2 and nothing else
    got = scan_gtf(write(tmp_path, b"".join(b"c\ts\tt\t1\t2\t0.5\t.\t%c\tk 1\n" % c for c in b".012"), "f.gtf"))
    assert not got["strand_valid"].any() and list(got["frame_valid"]) == [False, True, True, True] and list(got["frame_id"]) == [0, 0, 1, 2]
    for bad in (b"3", b"", b"00"):
        with pytest.raises(exon_amd.ExonHipError) as e:
            scan_gtf(write(tmp_path, b"c\ts\tt\t1\t2\t.\t+\t" + bad + b"\tk 1\n", "b.gtf"))
        assert "invalid frame" in str(e.value)


def test_line_rules(tmp_path):
    rec = PREFIX + b'gene_id "G1"; n 1'
    # CRLF: one CR in front of the LF is dropped; '#' lines are no rows ("##FASTA" too: there is no sequence section in GTF)
    text = b"#!a\r\n" + rec + b"\r\n##FASTA\n" + rec + b";\n# c\n"
    got = scan_gtf(write(tmp_path, text))
    assert got["n_rows"] == 2 and got["maps"] == [[("gene_id", "G1"), ("n", "1")]] * 2
    assert_same(got, gtf_expect.expect(text, attrs=True))
    # a last line without LF is read whole (the reference's reader would drop its last byte)
    text = rec + b"\n" + rec + b"23"
    got = scan_gtf(write(tmp_path, text))
    assert got["maps"][1] == [("gene_id", "G1"), ("n", "123")]
    assert_same(got, gtf_expect.expect(text, attrs=True))
    # end < start is accepted as it stands; a leading '+' on a position
    got = scan_gtf(write(tmp_path, b"c\ts\tt\t+9\t3\t1e-3\t-\t2\t\n"))
    assert (got["start"][0], got["end"][0], got["maps"][0]) == (9, 3, [])
    for bad, what in ((rec + b"\n\n" + rec + b"\n", "empty line"), (b"\n", "empty line"),
                      (b"chr1\thavana\texon\t11869\t12227\t.\t+\t.\n", "fewer than nine"),     # seven TABs
                      (b"c\ts\tt\t0\t3\t.\t+\t.\tk 1\n", "invalid start"), (b"c\ts\tt\t1\tx\t.\t+\t.\tk 1\n", "invalid end"),
                      (b"c\ts\tt\t1\t3\tabc\t+\t.\tk 1\n", "invalid score")):
        with pytest.raises(exon_amd.ExonHipError) as e:
            scan_gtf(write(tmp_path, bad))
        assert what in str(e.value), bad
        with pytest.raises((gtf_expect.GtfError, gtf_expect.gff_expect.GffError)):
            gtf_expect.expect(bad, attrs=True)


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """a generated file large enough for the slab-parallel reader (>= 8 MiB), with rich ninth fields"""
    p = tmp_path_factory.mktemp("gtf") / "gen.gtf"
    subprocess.check_call([GEN, "gtf", "60000", str(p), "attrs"])
    assert os.path.getsize(p) >= 8 << 20
    text = open(p, "rb").read()
    return p, text, gtf_expect.expect(text, attrs=True)


def test_threads_and_batch_sizes_agree(generated):
    p, text, want = generated
    seq = scan_gtf(p, batch_size=8192)
    assert_same(seq, want, "threads=0")
    assert seq["n_rows"] == 60000 and max(len(m) for m in seq["maps"]) == 12 and any(k == "tag" for m in seq["maps"] for k, _ in m)
    os.environ["EXON_HIP_DECODE_THREADS"] = "1"
    try:
        one = scan_gtf(p, batch_size=8192)
    finally:
        del os.environ["EXON_HIP_DECODE_THREADS"]
    assert_same(one, want, "threads=1")
    for bs in (1, 7):
        small = scan_gtf(os.path.join(FIX, "test.gtf"), batch_size=bs)
        assert small["sizes"] == [bs] * (77 // bs) + ([77 % bs] if 77 % bs else [])
        assert_same(small, gtf_expect.expect(fixture_text("test.gtf"), attrs=True), bs)


def test_region_filter(generated):
    p, text, _ = generated
    for region in ("chr7:100000-200000", "chrY:200000", "nope"):
        want = gtf_expect.expect(text, region, attrs=True)
        assert_same(scan_gtf(p, region=region), want, region)
    assert gtf_expect.expect(text, "chr7:100000-200000")["n_rows"] > 100
    want = gtf_expect.expect(fixture_text("test.gtf"), "chr1:12000-13000", attrs=True)
    assert 0 < want["n_rows"] < 77
    assert_same(scan_gtf(os.path.join(FIX, "test.gtf.gz"), region="chr1:12000-13000"), want)


def test_what_stays_refused():
    with pytest.raises(exon_amd.ExonHipError) as e:
        exon_amd.Scan(os.path.join(FIX, "test.gtf"), "gtf", region="chr1:1-100", use_index=True)
    assert e.value.code == EUNSUPPORTED and "indexed GTF" in str(e.value)
    lib = exon_amd.load()
    for bits in (1, 2, 256 | 1, 512):
        opt = exon_amd._lib.ScanOptions(9, 0, 0, None, None, 0, 0, bits)
        h = C.c_void_p()
        assert lib.exon_hip_scan_open(os.path.join(FIX, "test.gtf").encode(), C.byref(opt), C.byref(h)) == EUNSUPPORTED
        assert b"EXON_HIP_PROJECT_GTF_ATTRIBUTES" in lib.exon_hip_last_error(None)


def test_dictionaries_answer_as_for_gff():
    s = exon_amd.Scan(os.path.join(FIX, "test.gtf"), "gtf")
    list(s)
    assert s.dictionary(0) == ["chr1"] and s.dictionary(2) == ["exon"] and s.dictionary(1)[0] == "processed_transcript"
    assert s.dictionary(6) == ["+", "-"] and s.dictionary(7) == ["0", "1", "2"]
    assert s.intern(6, "-") == 1 and s.intern(7, "2") == 2 and s.intern(6, "?") == -1
    assert s.intern(0, "chr2") == 1
    s.close()
