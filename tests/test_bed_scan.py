"""CPU: BED scans through the host reader (exon_amd/csrc/host/bed.h) against tests/bed_expect.py, the plain-Python restatement of
the rules: the reference's slt pins (bed-select-tests.slt) on its fixtures, a case per rule and per error, every projection mask
of n_fields 3 .. 12, batch sizes, threads, and what stays refused."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import exon_amd
import bed_expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "bed")
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
EUNSUPPORTED = -4
ALL = bed_expect.COLUMNS[3:]


def scan_bed(path, project=ALL, bind=None, **kw):
    """Every batch of a scan as the columns bed_expect.expect returns (the dictionary columns decoded through their values), the
    batches' row counts (out["sizes"]) and, for the projected columns 6 .. 11, out["nulls"][name] = are all rows NULL; every batch
    is validated in full.
    bind: a Context -- the batches come out of the GPU pipeline (gpu_parse + bind_ctx); out["decoded_on_gpu"] tells how it ended."""
    s = exon_amd.Scan(str(path), "bed", project=project, gpu_parse=bind is not None, **kw)
    try:
        if bind is not None:
            s.bind_ctx(bind)
        batches = list(s)
        fields = [f.name for f in s.schema()]
        decoded = s.decoded_on_gpu()[0] if bind is not None else False
    finally:
        s.close()
    assert fields == bed_expect.COLUMNS[:3] + [c for c in ALL if c in project]
    out = {"n_rows": sum(len(b) for b in batches), "sizes": [len(b) for b in batches], "fields": fields, "nulls": {}, "decoded_on_gpu": decoded}
    for b in batches:
        b.validate(full=True)
        assert b.type.num_fields == len(fields)

    def values(name):
        k = fields.index(name)
        return [v for b in batches for v in b.field(k).to_pylist()]

    out["chrom"] = [v.encode() for v in values("reference_sequence_name")]
    for name in ("start", "end"):
        v = values(name)
        assert None not in v
        out[name] = np.array(v, np.int64).reshape(len(v))
    if "name" in fields:
        out["names"] = [None if v is None else v.encode() for v in values("name")]
    if "score" in fields:
        v = values("score")
        out["score_valid"] = np.array([x is not None for x in v], bool).reshape(len(v))
        out["score"] = np.array([x or 0 for x in v], np.int64).reshape(len(v))
    if "strand" in fields:
        v = values("strand")
        out["strand_valid"] = np.array([x is not None for x in v], bool).reshape(len(v))
        out["strand_id"] = np.array([0 if x is None else bed_expect.STRANDS.index(x) for x in v], np.int32).reshape(len(v))
    for name in bed_expect.COLUMNS[6:]:
        if name in fields:
            out["nulls"][name] = all(v is None for v in values(name))
    return out


def assert_same(got, want, what=""):
    assert got["n_rows"] == want["n_rows"], what
    assert got["chrom"] == want["chrom"], (what, "reference_sequence_name")
    for name in ("start", "end"):
        assert np.array_equal(got[name], want[name]), (what, name)
    if "names" in got:
        assert got["names"] == want["names"], (what, "name")
    for name in ("score", "strand"):
        if name + "_valid" in got:
            assert np.array_equal(got[name + "_valid"], want[name + "_valid"]), (what, name + " validity")
            key = name if name == "score" else "strand_id"
            assert np.array_equal(got[key], want[key]), (what, name)
    assert all(got["nulls"].values()), (what, "columns 6 .. 11 are NULL on every row")


def fixture_text(name):
    p = os.path.join(FIX, name)
    return gzip.open(p).read() if name.endswith(".gz") else open(p, "rb").read()


def write(tmp_path, text, name="t.bed"):
    p = tmp_path / name
    p.write_bytes(text)
    return p


def test_header_and_lib_constants_agree():
    hdr = open(os.path.join(ROOT, "include", "exon_hip.h")).read()
    assert exon_amd._lib.FORMATS["bed"] == 10 and "#define EXON_HIP_FORMAT_BED 10" in hdr
    assert "#define EXON_HIP_FORMAT_GFF 8" in hdr and "BED is not read" not in hdr
    for k, name in enumerate(ALL, 3):
        assert exon_amd._lib.PROJECT_BED[name] == 1 << k
        assert f"#define EXON_HIP_PROJECT_BED_{name.upper()} (1ull << {k})" in hdr
    assert "int exon_hip_abi_version" in hdr and exon_amd.load().exon_hip_abi_version() == 5


def test_schema_is_the_references():
    s = exon_amd.Scan(os.path.join(FIX, "test.bed"), "bed", project=ALL)
    t = s.schema()
    s.close()
    assert [f.name for f in t] == bed_expect.COLUMNS
    for f in t:
        want = pa.dictionary(pa.int32(), pa.string()) if f.name in ("reference_sequence_name", "strand") else pa.string() if f.name in bed_expect.UTF8_COLUMNS else pa.int64()
        assert f.type == want, f.name
        assert f.nullable == (f.name not in ("reference_sequence_name", "start", "end")), f.name
    s = exon_amd.Scan(os.path.join(FIX, "test.bed"), "bed")
    assert [f.name for f in s.schema()] == bed_expect.COLUMNS[:3]  # the default columns: the interval kernels' operands
    s.close()


def test_slt_pins_test_bed():
    got = scan_bed(os.path.join(FIX, "test.bed"))
    assert got["n_rows"] == 10 and got["sizes"] == [10]  # the `#comment` line is no row
    # bed-select-tests.slt: `chr1 11873 12227 NR_046018_exon_0_0_chr1_11874_f 0 + NULL NULL NULL NULL NULL NULL`
    assert (got["chrom"][0], got["start"][0], got["end"][0], got["names"][0]) == (b"chr1", 11873, 12227, b"NR_046018_exon_0_0_chr1_11874_f")
    assert got["score_valid"][0] and got["score"][0] == 0 and got["strand_valid"][0] and got["strand_id"][0] == 0
    assert len(got["nulls"]) == 6 and all(got["nulls"].values())
    assert_same(got, bed_expect.expect(fixture_text("test.bed")))


def test_slt_pins_gz_and_three_fields_and_long_name():
    got = scan_bed(os.path.join(FIX, "test.bed.gz"))  # one 12-field line
    assert got["n_rows"] == 1 and got["names"] == [b"."] and got["score_valid"][0] and got["score"][0] == 0 and not got["strand_valid"][0]
    assert (got["chrom"][0], got["start"][0], got["end"][0]) == (b"sq0", 7, 13) and all(got["nulls"].values())
    assert_same(got, bed_expect.expect(fixture_text("test.bed.gz")))
    assert_same(scan_bed(os.path.join(FIX, "test.bed.gz"), compression="gzip"), bed_expect.expect(fixture_text("test.bed.gz")))
    got = scan_bed(os.path.join(FIX, "test3.bed"))
    assert got["n_rows"] == 10 and got["names"] == [None] * 10 and not got["score_valid"].any() and not got["strand_valid"].any()
    assert_same(got, bed_expect.expect(fixture_text("test3.bed")))
    text = fixture_text("name_256bytes.one.bed")
    got = scan_bed(os.path.join(FIX, "name_256bytes.one.bed"), project=("name",))
    want = text.split(b"\n")[0].split(b"\t")[3]
    assert len(want) == 256 and want.startswith(b"PURK_peak_11,INH_SST_peak_18b,") and got["names"] == [want]


def test_zstd_is_refused_with_the_codec_named():
    with pytest.raises(exon_amd.ExonHipError) as e:
        exon_amd.Scan(os.path.join(FIX, "test.bed.zst"), "bed")
    assert e.value.code == EUNSUPPORTED and "zstd" in str(e.value)


# one line per rule of host/bed.h: (line, (chrom, start, end, name, score, strand id) | None for an error)
RULES = [
    (b"chr1\t5\t9", (b"chr1", 5, 9, None, None, None)),                                  # 3 fields
    (b"chr1\t5\t9\tn", (b"chr1", 5, 9, None, None, None)),                               # 4 fields: the name is read and dropped
    (b"chr1\t5\t9\tn\t7", (b"chr1", 5, 9, b"n", 7, None)),                               # 5 fields
    (b"chr1\t5\t9\tn\t7\t-", (b"chr1", 5, 9, b"n", 7, 1)),                               # 6 fields
    (b"chr1\t5\t9\tn\t7\t+", (b"chr1", 5, 9, b"n", 7, 0)),
    (b"chr1\t5\t9\tn\t7\t.", (b"chr1", 5, 9, b"n", 7, None)),                            # '.' strand -> NULL
    (b"chr1\t5\t9\tn\t7\t+\t5\t9\t0,0,0\t1\t4\t0", (b"chr1", 5, 9, b"n", 7, 0)),         # 12 fields: 7 .. 12 dropped unread
    (b"chr1\t5\t9\tn\t7\t+\tx\t\t\t\t\t", (b"chr1", 5, 9, b"n", 7, 0)),                  # ... whatever they hold
    (b"chr1\t0\t0", (b"chr1", 0, 0, None, None, None)),                                  # 0 is a value like any other
    (b"chr1\t+5\t+0", (b"chr1", 5, 0, None, None, None)),                                # one leading '+'; end < start as it stands
    (b"chr1\t007\t9", (b"chr1", 7, 9, None, None, None)),
    (b"chr1\t9223372036854775807\t9", (b"chr1", 2**63 - 1, 9, None, None, None)),        # i64::MAX is the last value
    (b"chr1\t000000000000000000000012\t9", (b"chr1", 12, 9, None, None, None)),          # (digits, however many)
    (b"chr1\t5\t9\t.\t0", (b"chr1", 5, 9, b".", 0, None)),                               # "." stays "."
    (b"chr1\t5\t9\t\t0", (b"chr1", 5, 9, b"", 0, None)),                                 # an empty name stays ""
    (b"chr1\t5\t9\tn\t65535", (b"chr1", 5, 9, b"n", 65535, None)),
    (b"chr1\t5\t9\tn\t+7", (b"chr1", 5, 9, b"n", 7, None)),
    (b"chr1\t5\t9\tn\t0000042", (b"chr1", 5, 9, b"n", 42, None)),
    (b"\t5\t9", (b"", 5, 9, None, None, None)),                                          # the sequence's name as it stands
    (b"caf\xc3\xa9\t5\t9\tn\xc3\xa9\t1", ("café".encode(), 5, 9, "né".encode(), 1, None)),  # UTF-8
    (b"chr1\t5\t9\ta b;c\t1", (b"chr1", 5, 9, b"a b;c", 1, None)),                       # only TAB separates
    (b"", None),                                                                         # an empty line
    (b"chr1", None), (b"chr1\t5", None),                                                 # 1, 2 fields
    (b"track name=x", None), (b"browser position chr1:1-2", None),
    (b"track\tname=x\ty", None),                                                         # (three fields, and no positions)
    (b"chr1\t5\t9\tn\t7\t+\t5", None),                                                   # 7 fields
    (b"chr1\t5\t9\tn\t7\t+\t5\t9", None), (b"chr1\t5\t9\tn\t7\t+\t5\t9\t0", None),       # 8, 9
    (b"chr1\t5\t9\tn\t7\t+\t5\t9\t0\t1", None), (b"chr1\t5\t9\tn\t7\t+\t5\t9\t0\t1\t4", None),  # 10, 11
    (b"chr1\t5\t9\tn\t7\t+\t5\t9\t0\t1\t4\t0\tx", None),                                 # 13
    (b"chr1\t5\t9\tn\t7\t+\t5\t9\t0\t1\t4\t0\tx\ty\tz", None),                           # 15
    (b"chr1\t5\t9\t", (b"chr1", 5, 9, None, None, None)),                                # (a trailing TAB: four fields, the fourth read and dropped ...)
    (b"chr1\t5\t9\tn\t7\t", None),                                                       # ... an empty strand is not
    (b"chr1\t\t9", None), (b"chr1\t5\t", None), (b"chr1\t-1\t9", None), (b"chr1\t5\t9x", None), (b"chr1\t5 \t9", None),
    (b"chr1\t++5\t9", None), (b"chr1\t+\t9", None), (b"chr1\t1e3\t9", None),
    (b"chr1\t9223372036854775808\t9", None), (b"chr1\t5\t99999999999999999999", None),   # above i64::MAX
    (b"chr1\t5\t9\tn\t65536", None), (b"chr1\t5\t9\tn\t.", None), (b"chr1\t5\t9\tn\t", None), (b"chr1\t5\t9\tn\t-1", None),
    (b"chr1\t5\t9\tn\t1.0", None), (b"chr1\t5\t9\tn\t+", None),
    (b"chr1\t5\t9\tn\t7\t?", None), (b"chr1\t5\t9\tn\t7\t++", None), (b"chr1\t5\t9\tn\t7\t*", None),
    (b"chr\xff\t5\t9", None), (b"chr1\t5\t9\tn\xc3\t1", None),                           # no UTF-8
    (b"chr1\t5\t9\tn", (b"chr1", 5, 9, None, None, None)),
    (b"chr1\t5\t9\t\xff", None),                                                         # ... in a field that is dropped
    (b"chr1\t5\t9\tn\t7\t+\t5\t9\t0\t1\t4\t\xed\xa0\x80", None),                         # ... in an ignored one (a surrogate)
]
GOOD = [(l, r) for l, r in RULES if r is not None]
BAD = [l for l, r in RULES if r is None]
RULE_TEXT = b"#a comment\n" + b"".join(l + (b"\r\n" if i % 3 == 0 else b"\n") for i, (l, r) in enumerate(GOOD))


def test_the_rule_table_in_the_restatement():
    for line, want in RULES:
        if want is None:
            with pytest.raises(bed_expect.BedError):
                bed_expect.parse_record(line)
        else:
            assert bed_expect.parse_record(line) == want, line


def test_a_row_per_rule(tmp_path):
    p = write(tmp_path, RULE_TEXT)
    got = scan_bed(p)
    want = bed_expect.expect(RULE_TEXT)
    assert want["n_rows"] == len(GOOD) and want["names"] == [r[3] for _, r in GOOD]
    assert_same(got, want)
    for bs in (1, 7):
        assert_same(scan_bed(p, batch_size=bs), want, bs)


@pytest.mark.parametrize("k", range(len(BAD)))
def test_a_file_per_error(k, tmp_path):
    line = BAD[k]
    text = b"chr1\t1\t2\n" + line + b"\nchr1\t3\t4\n"
    with pytest.raises(bed_expect.BedError):
        bed_expect.expect(text)
    # every line is validated in full whatever is projected
    for project in (ALL, ()):
        with pytest.raises(exon_amd.ExonHipError) as e:
            scan_bed(write(tmp_path, text), project=project)
        ascii_prefix = line[:40].split(b"\xc3")[0].split(b"\xff")[0].split(b"\xed")[0].decode()
        assert "BED line '" + ascii_prefix in str(e.value), str(e.value)


def test_line_rules(tmp_path):
    # CRLF: one CR in front of the LF is dropped; '#' lines are no rows wherever they stand
    text = b"#h\r\nchr1\t1\t2\tn\t3\t+\r\n# c\r\nchr2\t0\t5\r\n#\n"
    got = scan_bed(write(tmp_path, text))
    assert got["n_rows"] == 2 and got["names"] == [b"n", None] and got["chrom"] == [b"chr1", b"chr2"]
    assert_same(got, bed_expect.expect(text))
    # ... one CR: a second one belongs to the last field
    with pytest.raises(exon_amd.ExonHipError):
        scan_bed(write(tmp_path, b"chr1\t1\t2\r\r\n"))
    # a last line without LF is read whole (the reference's reader would drop its last byte)
    text = b"chr1\t1\t2\nchr1\t3\t45"
    got = scan_bed(write(tmp_path, text))
    assert list(got["end"]) == [2, 45]
    assert_same(got, bed_expect.expect(text))
    text = b"chr1\t1\t2\tn\t7\t-"
    got = scan_bed(write(tmp_path, text))
    assert got["strand_id"][0] == 1 and got["strand_valid"][0]
    # an empty file and a file of comments have no rows
    assert scan_bed(write(tmp_path, b""))["n_rows"] == 0 and scan_bed(write(tmp_path, b"#a\n#b\n"))["n_rows"] == 0
    with pytest.raises(exon_amd.ExonHipError) as e:
        scan_bed(write(tmp_path, b"chr1\t1\t2\n\nchr1\t3\t4\n"))
    assert "empty line" in str(e.value)


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    """20 000 generated rows of mixed field counts"""
    p = tmp_path_factory.mktemp("bed") / "gen.bed"
    subprocess.check_call([GEN, "bed", "20000", str(p), "mix"])
    text = open(p, "rb").read()
    return p, text, bed_expect.expect(text)


@pytest.mark.parametrize("n_fields", range(3, 13))
def test_every_projection_mask_of_n_fields(n_fields, generated):
    p, text, want = generated
    project = bed_expect.COLUMNS[3:n_fields]
    assert sum(exon_amd._lib.PROJECT_BED[c] for c in project) == bed_expect.mask_of(n_fields)
    got = scan_bed(p, project=project)
    assert got["fields"] == bed_expect.COLUMNS[:n_fields] and len(got["nulls"]) == max(0, n_fields - 6)
    assert_same(got, want, n_fields)
    assert_same(scan_bed(os.path.join(FIX, "test.bed"), project=project), bed_expect.expect(fixture_text("test.bed")), n_fields)


def test_scattered_projection_bits(generated):
    p, text, want = generated
    for project in (("strand",), ("score", "color"), ("name", "block_starts"), ("thick_end",)):
        assert_same(scan_bed(p, project=project), want, project)


@pytest.mark.parametrize("bs", [1, 7, 8192])
def test_batch_sizes(bs, generated):
    p, text, want = generated
    assert want["n_rows"] == 20000 and {len(l.split(b"\t")) for l in text.split(b"\n") if l and l[:1] != b"#"} == {3, 4, 5, 6, 12}
    got = scan_bed(p, batch_size=bs, project=("name", "score", "strand") if bs > 1 else ())
    assert got["sizes"] == [bs] * (20000 // bs) + ([20000 % bs] if 20000 % bs else [])
    assert_same(got, want, bs)


def test_threads_agree(tmp_path):
    p = tmp_path / "big.bed"  # large enough for the slab-parallel reader (>= 8 MiB)
    subprocess.check_call([GEN, "bed", "200000", str(p), "mix"])
    assert os.path.getsize(p) >= 8 << 20
    text = open(p, "rb").read()
    want = bed_expect.expect(text)
    par = scan_bed(p, project=("name", "score", "strand", "color"), batch_size=8192)
    assert_same(par, want, "threads=0")
    assert par["n_rows"] == 200000 and len(set(par["chrom"])) == 24
    os.environ["EXON_HIP_DECODE_THREADS"] = "1"
    try:
        one = scan_bed(p, project=("name", "score", "strand", "color"), batch_size=8192)
    finally:
        del os.environ["EXON_HIP_DECODE_THREADS"]
    assert_same(one, want, "threads=1")
    assert one["sizes"] == [8192] * (200000 // 8192) + [200000 % 8192]
    # an error in a later slab surfaces from the parallel reader too, the line quoted
    bad = tmp_path / "bad.bed"
    bad.write_bytes(text + b"chrY\t1\t2\tn\t65536\n")
    with pytest.raises(exon_amd.ExonHipError) as e:
        scan_bed(bad, project=())
    assert "invalid score '65536'" in str(e.value)


def test_batches_carry_their_own_row_count():
    # the struct's length is explicit (RecordBatchOptions::with_row_count): a consumer that takes no column still counts rows
    s = exon_amd.Scan(os.path.join(FIX, "test.bed"), "bed", batch_size=4)
    sizes = []
    while True:
        arr = s.next_raw()
        if arr is None:
            break
        assert arr.n_children == 3 and arr.null_count == 0
        sizes.append(arr.length)
        C.cast(arr.release, C.CFUNCTYPE(None, C.POINTER(exon_amd._lib.ArrowArray)))(C.byref(arr))
    s.close()
    assert sizes == [4, 4, 2]


def test_what_stays_refused():
    path = os.path.join(FIX, "test.bed")
    for kw, word in ((dict(region="chr1:1-100"), "region"), (dict(region="chr1:1-100", use_index=True), "region")):
        with pytest.raises(exon_amd.ExonHipError) as e:
            exon_amd.Scan(path, "bed", **kw)
        assert e.value.code == EUNSUPPORTED and word in str(e.value) and "reference has neither" in str(e.value)
    lib = exon_amd.load()
    opt = exon_amd._lib.ScanOptions(10, 0, 0, None, None, 1, 0, 0)  # use_index alone
    h = C.c_void_p()
    assert lib.exon_hip_scan_open(path.encode(), C.byref(opt), C.byref(h)) == EUNSUPPORTED and b"use_index" in lib.exon_hip_last_error(None)
    for bits in (1, 2, 4, 1 << 12, (1 << 3) | 1):
        opt = exon_amd._lib.ScanOptions(10, 0, 0, None, None, 0, 0, bits)
        assert lib.exon_hip_scan_open(path.encode(), C.byref(opt), C.byref(h)) == EUNSUPPORTED
        assert b"EXON_HIP_PROJECT_BED_NAME" in lib.exon_hip_last_error(None)
    opt = exon_amd._lib.ScanOptions(10, 0, 0, b"AF", None, 0, 0, 0)
    assert lib.exon_hip_scan_open(path.encode(), C.byref(opt), C.byref(h)) < 0 and b"info_field" in lib.exon_hip_last_error(None)


def test_dictionaries():
    s = exon_amd.Scan(os.path.join(FIX, "test.bed"), "bed", project=("score", "strand"))
    list(s)
    assert s.dictionary(0) == ["chr1"] and s.dictionary(4) == ["+", "-"]  # strand is scan column 4 under this projection
    assert s.intern(4, "-") == 1 and s.intern(4, "?") == -1 and s.intern(0, "chr2") == 1
    with pytest.raises(exon_amd.ExonHipError):
        s.dictionary(3)
    s.close()
    s = exon_amd.Scan(os.path.join(FIX, "test.bed"), "bed", project=ALL)
    assert s.dictionary(5) == ["+", "-"]
    s.close()
