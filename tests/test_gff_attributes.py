"""CPU: the GFF `attributes` column (EXON_HIP_PROJECT_GFF_ATTRIBUTES, Map<Utf8, List<Utf8>>) through the host reader
(exon_amd/csrc/host/gff.h) against tests/gff_attr_expect.py, the plain-Python restatement of the attribute rules: the schema,
literals pinned on the reference's fixtures, a row per rule and a file per error, the sequential and the slab-parallel reader on
the generator's rich fields, region and indexed-region scans, batch sizes, and the projection bits that stay refused."""
import ctypes as C
import gzip
import os
import subprocess

import pyarrow as pa
import pytest

import exon_amd
import gff_attr_expect
import gff_expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "gff")
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
EUNSUPPORTED = -4
PREFIX = b"chr1\ts\tgene\t1\t2\t.\t+\t.\t"


def scan_attributes(path, bind=None, **kw):
    """(the attributes of every row as to_pylist() gives them, the batches' row counts, the scan's decoded_on_gpu); every batch is
    validated in full.  bind: a Context -- the batches come out of the GPU pipeline."""
    s = exon_amd.Scan(str(path), "gff", gpu_parse=bind is not None, project=("attributes",), **kw)
    try:
        if bind is not None:
            s.bind_ctx(bind)
        batches = list(s)
        decoded = s.decoded_on_gpu()[0] if bind is not None else False
    finally:
        s.close()
    out = []
    for b in batches:
        b.validate(full=True)
        assert b.type.num_fields == 9 and b.field(8).null_count == 0
        out += b.field(8).to_pylist()
    return out, [len(b) for b in batches], decoded


def test_schema_is_the_references_map():
    s = exon_amd.Scan(os.path.join(FIX, "ecoli.gff"), "gff", project=("attributes",))
    t = s.schema()
    s.close()
    assert [f.name for f in t] == ["seqname", "source", "type", "start", "end", "score", "strand", "phase", "attributes"]
    f = t.field(8)
    assert not f.nullable and pa.types.is_map(f.type) and not f.type.keys_sorted
    assert f.type == pa.map_(pa.string(), pa.list_(pa.string()))
    assert not f.type.key_field.nullable and f.type.item_field.nullable and f.type.item_field.type.value_field.nullable
    # (pyarrow's importer renames a map's fields to its own "key" / "value": the reference's names are read off the C schema)
    sch = exon_amd._lib.ArrowSchema()
    s = exon_amd.Scan(os.path.join(FIX, "ecoli.gff"), "gff", project=("attributes",))
    s._check(s.lib.exon_hip_scan_schema(s.h, C.byref(sch)))
    m = sch.children[8].contents
    entries = m.children[0].contents
    keys, values = entries.children[0].contents, entries.children[1].contents
    item = values.children[0].contents
    NULLABLE, KEYS_SORTED = 2, 4
    assert (m.format, m.name, m.flags & (NULLABLE | KEYS_SORTED), m.n_children) == (b"+m", b"attributes", 0, 1)
    assert (entries.format, entries.name, entries.flags & NULLABLE, entries.n_children) == (b"+s", b"entries", 0, 2)
    assert (keys.format, keys.name, keys.flags & NULLABLE) == (b"u", b"keys", 0)
    assert (values.format, values.name, values.flags & NULLABLE) == (b"+l", b"values", NULLABLE)
    assert (item.format, item.name, item.flags & NULLABLE) == (b"u", b"item", NULLABLE)
    pa.DataType._import_from_c(C.addressof(sch))  # (releases it)
    s.close()
    assert "#define EXON_HIP_PROJECT_GFF_ATTRIBUTES 256ull" in open(os.path.join(ROOT, "include", "exon_hip.h")).read()
    # the struct array itself names the entries field as the reference does
    b = next(iter(exon_amd.Scan(os.path.join(FIX, "ecoli.gff"), "gff", project=("attributes",))))
    assert b.field(8).type == f.type and b.type.field(8).name == "attributes"


def test_ecoli_rows_end_in_a_semicolon_and_have_no_empty_entry():
    got, _, _ = scan_attributes(os.path.join(FIX, "ecoli.gff"))
    assert len(got) == 7
    assert got[0] == [("ID", ["1_1"]), ("partial", ["00"]), ("start_type", ["ATG"]), ("rbs_motif", ["AGGA"]), ("rbs_spacer", ["5-10bp"]),
                      ("gc_cont", ["0.382"]), ("conf", ["99.80"]), ("score", ["26.99"]), ("cscore", ["8.27"]), ("sscore", ["18.72"]),
                      ("rscore", ["10.52"]), ("uscore", ["4.30"]), ("tscore", ["3.91"])]
    assert all(len(r) == 13 for r in got)
    assert got == gff_attr_expect.rows(open(os.path.join(FIX, "ecoli.gff"), "rb").read())


@pytest.mark.parametrize("name", ["test.gff.gz", "test.gff3.gz"])
def test_reference_test_gff(name):
    got, sizes, _ = scan_attributes(os.path.join(FIX, name))
    assert len(got) == 5000 and sizes == [5000]
    assert got[0] == [("gene_id", ["caat1"]), ("gene_name", ["gene0"])]
    assert all(len(r) == 2 for r in got)
    assert got == gff_attr_expect.rows(gzip.open(os.path.join(FIX, name)).read())


def test_bad_directive_fixture():
    got, _, _ = scan_attributes(os.path.join(FIX, "bad-directive.gff"))
    assert len(got) == 7
    assert [r for r in got if ("partial", ["5'"]) in r][0][0] == ("ID", ["Ga0604745_000001_2_2116"])
    assert got == gff_attr_expect.rows(open(os.path.join(FIX, "bad-directive.gff"), "rb").read())


# one row per rule: (field 9, the map it gives)
RULES = [
    (b"", []),
    (b".", []),
    (b"ID=1", [("ID", ["1"])]),
    (b"ID=1;", [("ID", ["1"])]),                                   # one trailing ';' is ignored
    (b"ID=1;Parent=g1;Name=x", [("ID", ["1"]), ("Parent", ["g1"]), ("Name", ["x"])]),
    (b"a=b\twith\ttabs", [("a", ["b\twith\ttabs"])]),                # TABs behind the eighth are kept
    (b"=v", [("", ["v"])]),                                        # an empty key
    (b"k=", [("k", [""])]),                                        # an empty value: one empty item
    (b"k=a=b", [("k", ["a=b"])]),                                  # split at the FIRST '='
    (b"k=a,b,c", [("k", ["a", "b", "c"])]),
    (b"k=,a,,b,", [("k", ["", "a", "", "b", ""])]),                # empty pieces are empty items
    (b"k=,", [("k", ["", ""])]),
    (b"k%3D1=v%3Bw%2cx%25y", [("k=1", ["v;w,x%y"])]),              # decoded AFTER the splitting, either case
    (b"k=caf%C3%A9", [("k", ["café"])]),
    (b"k=caf\xc3\xa9", [("k", ["café"])]),                    # raw UTF-8
    (b"k=100%;j=%zz;i=%4", [("k", ["100%"]), ("j", ["%zz"]), ("i", ["%4"])]),  # a '%' without two hex digits stays
    (b"k=%2", [("k", ["%2"])]),
    (b"k=%41%42,%43", [("k", ["AB", "C"])]),
    (b"k= v ;j=\"q\"", [("k", [" v "]), ("j", ["\"q\""])]),       # nothing trimmed or unquoted
    (b"k=1;k=2;k=1", [("k", ["1"]), ("k", ["2"]), ("k", ["1"])]),  # duplicate keys stay, in file order
    (b".;a=b", None),                                              # ('.' is only special as the whole field: a piece without '=')
]
RULE_TEXT = b"##gff-version 3\n" + b"".join(PREFIX + f + (b"\r\n" if i % 3 == 0 else b"\n") for i, (f, m) in enumerate(RULES) if m is not None)
RULE_MAPS = [m for _, m in RULES if m is not None]


def test_a_row_per_rule(tmp_path):
    assert gff_attr_expect.rows(RULE_TEXT) == RULE_MAPS
    p = tmp_path / "rules.gff"
    p.write_bytes(RULE_TEXT)
    got, _, _ = scan_attributes(p)
    assert got == RULE_MAPS
    gz = tmp_path / "rules.gff.gz"
    gz.write_bytes(gzip.compress(RULE_TEXT))
    assert scan_attributes(gz)[0] == RULE_MAPS


ERRORS = [("no '='", b"ID=1;flag;x=y"), ("';;'", b"a=b;;c=d"), ("a leading ';'", b";a=b"), ("'a=b;;'", b"a=b;;"), ("';' alone", b";"),
          ("%FF", b"a=x%FFy"), ("%C3 cut short", b"k%C3=v"), ("a raw invalid byte", b"a=x\xffy"), ("a raw overlong form", b"a=\xc0\xaf"),
          ("a raw surrogate", b"a=\xed\xa0\x80"), ("'.' as a piece", b".;a=b")]


@pytest.mark.parametrize("what,field", ERRORS, ids=[e[0] for e in ERRORS])
def test_every_error_quotes_the_line(tmp_path, what, field):
    line = b"chrE\ts\tgene\t11\t22\t.\t+\t.\t" + field
    with pytest.raises(gff_expect.GffError):
        gff_attr_expect.rows(line + b"\n")
    p = tmp_path / "bad.gff"
    p.write_bytes(line + b"\n")
    with pytest.raises(exon_amd.ExonHipError) as e:
        scan_attributes(p)
    assert e.value.code < 0 and e.value.code != EUNSUPPORTED, what
    assert "chrE\ts\tgene\t11\t22" in str(e.value), "the message quotes the line"
    # without the column the same file is read: the ninth field is nobody's business then
    s = exon_amd.Scan(str(p), "gff")
    assert sum(len(b) for b in s) == 1
    s.close()


def test_a_filtered_out_record_is_validated_too(tmp_path):
    text = PREFIX + b"ID=1\n" + b"chr2\ts\tgene\t1\t2\t.\t+\t.\tnoequals\n"
    p = tmp_path / "f.gff"
    p.write_bytes(text)
    with pytest.raises(exon_amd.ExonHipError) as e:
        scan_attributes(p, region="chr1")
    assert "noequals" in str(e.value)


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    """gen_text gff 20000 attrs: more than 8 MiB, so the host reader decodes it slab-parallel; its text and the expected maps"""
    p = tmp_path_factory.mktemp("gffattr") / "a.gff"
    subprocess.check_call([GEN, "gff", "20000", str(p), "attrs"])
    text = open(p, "rb").read()
    assert len(text) >= 8 << 20
    return p, text, gff_attr_expect.rows(text)


def test_gen_text_attrs_covers_the_shapes_and_leaves_the_default_alone(rich, tmp_path):
    _p, text, maps = rich
    fields = [gff_attr_expect.field9(ln) for ln in gff_expect.lines_of(text) if ln[:1] != b"#"]
    assert len(maps) == 20000 and b"." in fields and b"" in fields
    assert {len(m) for m in maps} == set(range(13))
    assert sum(f.endswith(b";") for f in fields) > 5000 and sum(not f.endswith(b";") for f in fields) > 5000
    lens = {len(v) for m in maps for _, vs in m if len(vs) == 1 for v in vs}
    assert {0, 1, 7, 8, 9, 300} <= lens
    assert any("" in vs and len(vs) > 2 for m in maps for _, vs in m)
    for esc in (b"%3B", b"%2c", b"%25", b"=100%;", b"%zz"):
        assert esc in text
    assert any(len({k for k, _ in m}) < len(m) for m in maps), "duplicate keys"
    assert any(k == "" for m in maps for k, _ in m) and any(k == "tag x" for m in maps for k, _ in m)
    assert max(text) < 0x80
    # the default output is what it was: the same eight columns row by row, and the old ninth field
    d = tmp_path / "d.gff"
    subprocess.check_call([GEN, "gff", "3000", str(d)])
    a = tmp_path / "a.gff"
    subprocess.check_call([GEN, "gff", "3000", str(a), "attrs"])
    dl, al = open(d, "rb").read().split(b"\n"), open(a, "rb").read().split(b"\n")
    assert len(dl) == len(al) and all(x.split(b"\t")[:8] == y.split(b"\t")[:8] for x, y in zip(dl, al))
    assert dl[1].endswith(b"\tID=f0;Name=n%d" % int(dl[1].rsplit(b"=n", 1)[1]))


def test_sequential_reader_parallel_reader_and_expectation_agree(rich, monkeypatch):
    p, _text, maps = rich
    got, sizes, _ = scan_attributes(p)
    assert got == maps and max(sizes) <= 8192 and sum(sizes) == 20000
    monkeypatch.setenv("EXON_HIP_DECODE_THREADS", "1")
    got, sizes, _ = scan_attributes(p)
    assert got == maps and sizes[:2] == [8192, 8192]


@pytest.mark.parametrize("batch_size", [1, 16, 1 << 20])
def test_batch_sizes(tmp_path, batch_size):
    p = tmp_path / "rules.gff"
    p.write_bytes(RULE_TEXT)
    got, sizes, _ = scan_attributes(p, batch_size=batch_size)
    assert got == RULE_MAPS
    assert sizes == [min(batch_size, len(RULE_MAPS) - k) for k in range(0, len(RULE_MAPS), batch_size)]


REGIONS = ["chr1", "chr7:10000-30000", "chrY:1-50", "chrM", "chr2:1-1"]


def test_region_scans(rich, monkeypatch):
    p, text, _maps = rich
    want = {region: gff_attr_expect.rows(text, region) for region in REGIONS}
    for region in REGIONS:  # the slab-parallel reader
        assert scan_attributes(p, region=region)[0] == want[region], region
    monkeypatch.setenv("EXON_HIP_DECODE_THREADS", "1")
    for region in REGIONS[:2]:
        assert scan_attributes(p, region=region)[0] == want[region], (region, "sequential")
    assert len(gff_attr_expect.rows(text, "chr7:10000-30000")) > 100 and gff_attr_expect.rows(text, "chrM") == []


def test_indexed_region_scans(rich, tmp_path):
    p, text, _maps = rich
    gz = tmp_path / "a.gff.gz"
    subprocess.check_call([BGZIP, str(p), str(gz), "6"])
    assert gff_expect.write_gff_tabix(gz) == 20000
    for region in ["chr1", "chr7:10000-20000", "chrY", "chrM", "chr12:1-5000"]:
        s = exon_amd.Scan(str(gz), "gff", region=region, use_index=True, project=("attributes",))
        chunks = s.index_chunks()
        s.close()
        want = gff_attr_expect.rows(text, region)
        assert chunks >= 1 or not want
        assert scan_attributes(gz, region=region, use_index=True)[0] == want, region


@pytest.mark.parametrize("projection", [1, 257, 2, 512, 1 << 40])
def test_other_projection_bits_stay_refused(projection):
    lib = exon_amd.load()
    opt = exon_amd._lib.ScanOptions(8, 0, 0, None, None, 0, 0, projection)
    h = C.c_void_p()
    assert lib.exon_hip_scan_open(os.path.join(FIX, "ecoli.gff").encode(), C.byref(opt), C.byref(h)) == EUNSUPPORTED
    msg = lib.exon_hip_last_error(None)
    assert b"attributes" in msg and b"EXON_HIP_PROJECT_GFF_ATTRIBUTES" in msg
