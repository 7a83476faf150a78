"""GPU: the GFF `attributes` column built on the device (text_columns.hip: k_gff_attr_measure -> four offset scans ->
k_gff_attr_fill) against tests/gff_attr_expect.py and the host reader: the six buffers at the parser level (row counts around
the wave and block sizes, ranked rows and row = line, every misalignment, stale offsets, a slab cut inside a ninth field), the
rows the device hands over, the item-offsets buffer at its capacity, and the file pipeline (slabs, compression, batch sizes,
region runs and the gather, an indexed scan) -- and a fused plan over a scan that has the bit set, which builds none of it."""
import gzip
import os
import subprocess
import zlib

import numpy as np
import pyarrow as pa
import pytest

import exon_amd
import gff_attr_expect
import gff_expect
from test_gff_attributes import PREFIX, RULES, scan_attributes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
BUFFERS = ("map_offsets", "key_offsets", "key_values", "list_offsets", "item_offsets", "item_values")
TOTALS = ("n_entries", "n_items", "n_key_bytes", "n_item_bytes")


def check(ctx, text, misalign=0, parser=None, want=None):
    """the six buffers and four totals of `text`'s whole lines, byte for byte"""
    own = parser is None
    parser = parser or exon_amd.GFFParser(ctx)
    res = parser.parse_host(text, misalign=misalign, attributes=True)
    assert res["n_undecided"] == 0 and res["attributes"]["n_undecided"] == 0
    last = text.rfind(b"\n") + 1
    assert res["consumed_bytes"] == last
    want = want or gff_attr_expect.buffers(gff_attr_expect.rows(text[:last]))
    got = res["attributes"]
    assert len(want["map_offsets"]) == res["n_rows"] + 1
    for k in TOTALS:
        assert got[k] == want[k], (k, misalign)
    for k in BUFFERS:
        assert np.array_equal(got[k], want[k]), (k, misalign)
    assert got["map_offsets"][0] == 0 and got["key_offsets"][0] == 0 and got["list_offsets"][0] == 0 and got["item_offsets"][0] == 0
    if own:
        parser.close()
    return res


@pytest.fixture(scope="module")
def rich(tmp_path_factory):
    """gen_text gff 15000 attrs (about 7 MB: two BGZF slabs at EXON_HIP_GPU_PARSE_SLAB_MB=1, whose first is 64 blocks): the file, its
    text, its lines"""
    p = tmp_path_factory.mktemp("gffattrgpu") / "a.gff"
    subprocess.check_call([GEN, "gff", "15000", str(p), "attrs"])
    text = open(p, "rb").read()
    assert 5 << 20 < len(text) < 8 << 20
    return p, text, text.split(b"\n")


def test_row_counts_around_the_wave_and_block_sizes(ctx, rich):
    _p, _text, lines = rich
    plain = [ln for ln in lines[1:400] if not ln.startswith(b"#")]
    parser = exon_amd.GFFParser(ctx)
    for n in (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 130, 257):
        body = b"\n".join(plain[:n]) + b"\n"
        check(ctx, body, parser=parser)                          # row = line
        check(ctx, b"# head\n" + body, misalign=3, parser=parser)  # rows are ranks
    parser.close()


def test_every_misalignment_plain_and_ranked(ctx, rich):
    _p, _text, lines = rich
    plain = b"\n".join(ln for ln in lines[1:700] if not ln.startswith(b"#")) + b"\n"
    ranked = b"\n".join(lines[990:2100]) + b"\n"
    assert b"\n#" not in plain and ranked.count(b"\n#") >= 2
    for slab in (plain, ranked):
        want = gff_attr_expect.buffers(gff_attr_expect.rows(slab))
        parser = exon_amd.GFFParser(ctx)
        for misalign in range(16):
            check(ctx, slab, misalign=misalign, parser=parser, want=want)
        parser.close()


def test_a_row_per_rule(ctx):
    ascii_rules = [(f, m) for f, m in RULES if m is not None and max(f, default=0) < 0x80 and b"%C3" not in f]
    assert len(ascii_rules) >= 17
    text = b"".join(PREFIX + f + (b"\r\n" if i % 3 == 0 else b"\n") for i, (f, _m) in enumerate(ascii_rules))
    assert gff_attr_expect.rows(text) == [m for _f, m in ascii_rules]
    check(ctx, text)
    check(ctx, b"##gff-version 3\n" + text, misalign=11)


def test_no_stale_offsets_between_slabs(ctx, rich):
    _p, _text, lines = rich
    full = b"\n".join(ln for ln in lines[1:300] if not ln.startswith(b"#")) + b"\n"
    dots = b"".join(PREFIX + (b".\n" if i % 2 else b"\n") for i in range(300))
    parser = exon_amd.GFFParser(ctx)
    for slab in (full, dots, full, dots, dots, full):
        res = check(ctx, slab, parser=parser)
        if slab is dots:
            at = res["attributes"]
            assert [at[k] for k in TOTALS] == [0, 0, 0, 0] and not at["map_offsets"].any()
            assert list(at["key_offsets"]) == [0] and list(at["list_offsets"]) == [0] and list(at["item_offsets"]) == [0]
    parser.close()


def test_a_slab_cut_inside_a_ninth_field(ctx, rich):
    _p, text, _lines = rich
    head = text[:200_000]
    last = head.rfind(b"\n")
    long_field = max(range(0, 150_000, 997), key=lambda u: head.find(b"\n", u) - u)
    end = head.find(b"\n", long_field)
    for cut in (len(head), last + 1, last + 30, last, end - 5, end - 1):
        res = check(ctx, head[:cut])
        assert 0 < res["consumed_bytes"] <= cut


GOOD = PREFIX + b"ID=1;Name=a,b\n"
UNDECIDED = [("a raw byte >= 0x80", b"k=caf\xc3\xa9"), ("an escape that gives a byte >= 0x80", b"k=caf%C3%A9"), ("%FF", b"a=x%FFy"),
             ("a raw invalid byte", b"a=x\xffy"), ("a piece without '='", b"ID=1;flag;x=y"), ("a last piece without '='", b"ID=1;flag"),
             ("';;'", b"a=b;;c=d"), ("a leading ';'", b";a=b"), ("'a=b;;'", b"a=b;;"), ("';' alone", b";")]


@pytest.mark.parametrize("what,field", UNDECIDED, ids=[u[0] for u in UNDECIDED])
def test_rows_the_device_cannot_decide_are_counted(ctx, what, field):
    parser = exon_amd.GFFParser(ctx)
    for text in (GOOD * 70 + PREFIX + field + b"\n" + GOOD * 70, PREFIX + field + b"\n", b"# c\n" + GOOD * 3 + PREFIX + field + b"\n"):
        res = parser.parse_host(text, misalign=2, attributes=True)
        assert res["n_undecided"] == 0 and res["attributes"]["n_undecided"] == 1, what
        assert "map_offsets" not in res["attributes"]
    check(ctx, GOOD * 3, parser=parser)
    parser.close()


def host_result(path, **kw):
    try:
        return scan_attributes(path, **kw)[0], None
    except exon_amd.ExonHipError as e:
        return None, (e.code, str(e))


@pytest.mark.parametrize("what,field", UNDECIDED, ids=[u[0] for u in UNDECIDED])
def test_hand_over_inside_an_otherwise_good_file(ctx, rich, tmp_path, monkeypatch, what, field):
    """the undecidable row sits in the file's third slab: the batches (or the error) are the host reader's, and the scan says that
    the host took over"""
    _p, text, _lines = rich
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    cut = text.rfind(b"\n", 0, 2_500_000) + 1
    p = tmp_path / "h.gff"
    p.write_bytes(text[:cut] + b"chrH\ts\tgene\t5\t6\t.\t+\t.\t" + field + b"\n" + text[cut:])
    want, err = host_result(p)
    assert (want is None) != (err is None)
    s = exon_amd.Scan(str(p), "gff", gpu_parse=True, project=("attributes",)).bind_ctx(ctx)
    got = []
    try:
        for b in s:
            b.validate(full=True)
            got += b.field(8).to_pylist()
        assert err is None, "the host reader refuses this file"
        assert got == want and len(got) == 15001
        assert not s.decoded_on_gpu()[0]
    except exon_amd.ExonHipError as e:
        assert err is not None and (e.code, str(e)) == err, what
        assert "chrH\ts\tgene\t5\t6" in str(e)
    finally:
        s.close()


REGION_FIELDS = [("a piece without '='", b"noequals"), ("'a=b;;'", b"a=b;;"), ("%FF", b"a=x%FFy"), ("a raw byte >= 0x80", b"k=caf\xc3\xa9")]


@pytest.mark.parametrize("region", ["chr20", "chrM"])
@pytest.mark.parametrize("where", ["a slab that keeps nothing", "a slab that keeps rows"])
@pytest.mark.parametrize("what,field", REGION_FIELDS, ids=[u[0] for u in REGION_FIELDS])
def test_field_nine_is_validated_under_a_region_kept_or_not(ctx, rich, tmp_path, monkeypatch, what, field, where, region):
    """with the column projected every record's ninth field is validated, whether the pushed-down filter keeps the record or its
    slab keeps any row at all: the undecidable row (its own seqname is chr1, so no region here keeps it) makes the device hand the
    file over, and the batches or the error are the host reader's"""
    _p, text, _lines = rich
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    run = text.index(b"\nchr20\t") + 1
    assert run > 4_000_000
    at = text.rfind(b"\n", 0, 1_500_000) + 1 if where == "a slab that keeps nothing" else text.index(b"\n", run + 100_000) + 1
    assert where == "a slab that keeps nothing" or text[at:at + 6] == b"chr20\t"
    p = tmp_path / "r.gff"
    p.write_bytes(text[:at] + b"chr1\ts\tgene\t5\t6\t.\t+\t.\t" + field + b"\n" + text[at:])
    want, err = host_result(p, region=region)
    assert (err is None) == (what == "a raw byte >= 0x80")
    try:
        got, _sizes, decoded = scan_attributes(p, bind=ctx, region=region)
        assert err is None, "the host reader refuses this file, the device pipeline answered"
        assert got == want and not decoded
        assert len(got) == (0 if region == "chrM" else len(gff_attr_expect.rows(text, region)))
    except exon_amd.ExonHipError as e:
        assert err is not None and (e.code, str(e)) == err, what
        assert "chr1\ts\tgene\t5\t6" in str(e)


# ---- the one buffer the table above scratch_for marks "checked": the items' byte offsets --------------------------------------------
# a slab under 1 MiB gets item-offset buffers of (1 << 20) / 2 + (1 << 16) + 64 + 2 entries; the items and the closing entry take them
ITEM_CAP = (1 << 19) + (1 << 16) + 64 + 2


@pytest.mark.parametrize("at", [0, 1, 2])
def test_item_offsets_around_the_scratch_capacity(ctx, tmp_path, monkeypatch, at):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    items = ITEM_CAP + at - 1
    per_row = [items // 7] * 6
    per_row.append(items - sum(per_row))
    text = b"".join(b"chr1\ts\tgene\t%d\t%d\t.\t+\t.\tk=" % (i + 1, i + 2) + b"," * (n - 1) + b"\n" for i, n in enumerate(per_row))
    assert len(text) + 16 <= 1 << 20 and text.count(b",") + 7 + 1 == ITEM_CAP + at
    p = tmp_path / "cap.gff"
    p.write_bytes(text)
    want = [[("k", [""] * n)] for n in per_row]
    assert scan_attributes(p)[0] == want
    got, _sizes, decoded = scan_attributes(p, bind=ctx)
    assert got == want
    assert decoded == (at == 0), "at the capacity the device builds the slab; past it the host reader answers"
    if at == 0:  # the parser-level entry shows the closing entry in the buffer's last slot
        res = check(ctx, text)
        assert res["attributes"]["n_items"] + 1 == ITEM_CAP and res["attributes"]["item_offsets"][-1] == 0
    else:
        parser = exon_amd.GFFParser(ctx)
        res = parser.parse_host(text, attributes=True)
        assert res["attributes"]["n_undecided"] == 7
        parser.close()


# ---- the file pipeline ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twins(rich, tmp_path_factory):
    p, text, _lines = rich
    d = tmp_path_factory.mktemp("gffattrpipe")
    bgz, gz = d / "a.gff.bgz.gz", d / "a.gff.gz"
    subprocess.check_call([BGZIP, str(p), str(bgz), "6"])
    # plain gzip in DEFLATE blocks of at most 1024 symbols (memLevel 4): the long repetitive values compress so well that zlib's
    # default 16 K-symbol blocks inflate to more than a 1 MiB slab, which is the host reader's by design
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 4)
    gz.write_bytes(co.compress(text) + co.flush())
    assert gzip.decompress(gz.read_bytes()) == text
    return {"plain": p, "bgzf": bgz, "gzip": gz}, gff_attr_expect.rows(text)


@pytest.mark.parametrize("twin", ["plain", "bgzf", "gzip"])
def test_slabs_of_an_irregular_file(ctx, twins, monkeypatch, twin):
    paths, maps = twins
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    monkeypatch.setenv("EXON_HIP_GZ_SLAB_MB", "1")  # (plain-gzip slabs are cut by output bytes, by a switch of their own)
    got, sizes, decoded = scan_attributes(paths[twin], bind=ctx, batch_size=1 << 20)
    assert decoded and len(sizes) >= 2, sizes  # (batches end with their slab)
    assert got == maps
    assert got == scan_attributes(paths[twin])[0]


@pytest.mark.parametrize("batch_size", [1, 16, 8192])
def test_batch_sizes(ctx, twins, monkeypatch, batch_size):
    paths, maps = twins
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    s = exon_amd.Scan(str(paths["plain"]), "gff", gpu_parse=True, project=("attributes",), batch_size=batch_size).bind_ctx(ctx)
    batches = list(s)
    assert s.decoded_on_gpu()[0]
    s.close()
    assert max(len(b) for b in batches) <= batch_size and sum(len(b) for b in batches) == len(maps)
    for b in batches[:: max(1, len(batches) // 200)]:
        b.validate(full=True)
    got = pa.chunked_array([b.field(8) for b in batches])
    assert got.to_pylist() == maps
    # the other eight columns ride along unchanged: the host reader's, value by value
    host = list(exon_amd.Scan(str(paths["plain"]), "gff", project=("attributes",)))
    for k in range(8):
        assert pa.chunked_array([b.field(k) for b in batches]).to_pylist() == pa.chunked_array([b.field(k) for b in host]).to_pylist(), k


@pytest.mark.parametrize("gather", ["0", "1"])
def test_region_runs_and_the_gather(ctx, twins, rich, monkeypatch, gather):
    paths, _maps = twins
    _p, text, _lines = rich
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    monkeypatch.setenv("EXON_HIP_EXPORT_GATHER", gather)
    for region in ("chr7:1000-20000", "chr1", "chrM", "chr24", "chrY:1-50"):
        want = gff_attr_expect.rows(text, region)
        for batch_size in (16, 8192):
            got, _sizes, decoded = scan_attributes(paths["plain"], bind=ctx, region=region, batch_size=batch_size)
            assert decoded and got == want, (region, batch_size)
    assert len(gff_attr_expect.rows(text, "chr7:1000-20000")) > 100


def test_more_than_256_kept_runs_go_through_the_gather(ctx, rich, tmp_path, monkeypatch):
    _p, _text, lines = rich
    monkeypatch.delenv("EXON_HIP_EXPORT_GATHER", raising=False)
    rows = [ln for ln in lines[1:1300] if ln and not ln.startswith(b"#")]
    alt = b"".join((b"chrA" if i % 2 else b"chrB") + ln[ln.index(b"\t"):] + b"\n" for i, ln in enumerate(rows))
    p = tmp_path / "alt.gff"
    p.write_bytes(alt)
    want = gff_attr_expect.rows(alt, "chrA")
    assert len(want) > 300
    got, _sizes, decoded = scan_attributes(p, bind=ctx, region="chrA", batch_size=100)
    assert decoded and got == want and got == scan_attributes(p, region="chrA")[0]


def test_indexed_region_scan(ctx, twins, rich):
    paths, _maps = twins
    _p, text, _lines = rich
    assert gff_expect.write_gff_tabix(paths["bgzf"]) == 15000
    for region in ("chr7:1000-20000", "chr2", "chrM"):
        want = gff_attr_expect.rows(text, region)
        got, _sizes, decoded = scan_attributes(paths["bgzf"], bind=ctx, region=region, use_index=True)
        assert decoded and got == want, region
        assert scan_attributes(paths["bgzf"], region=region, use_index=True)[0] == want


def test_200k_rows_device_host_and_expectation(ctx, tmp_path):
    p = tmp_path / "big.gff"
    subprocess.check_call([GEN, "gff", "200000", str(p), "attrs"])

    def column(bind):
        s = exon_amd.Scan(str(p), "gff", gpu_parse=bind, project=("attributes",))
        if bind:
            s.bind_ctx(ctx)
        chunks = [b.field(8) for b in s]
        decoded = s.decoded_on_gpu()[0] if bind else False
        s.close()
        return pa.chunked_array(chunks), decoded

    dev, decoded = column(True)
    host, _ = column(False)
    assert decoded and len(dev) == 200_000
    dev.validate(full=True)
    assert dev.equals(host)
    want = gff_attr_expect.buffers(gff_attr_expect.rows(open(p, "rb").read(), well_formed=True))
    flat = pa.concat_arrays(dev.chunks)

    def utf8_buffers(arr):
        _valid, off, data = arr.buffers()
        off = np.frombuffer(off, np.int32)[arr.offset:arr.offset + len(arr) + 1]
        return off - off[0], np.frombuffer(data, np.uint8)[off[0]:off[-1]]

    assert np.array_equal(flat.offsets.to_numpy(), want["map_offsets"])
    assert np.array_equal(flat.items.offsets.to_numpy(), want["list_offsets"])
    for arr, off, val in ((flat.keys, "key_offsets", "key_values"), (flat.items.values, "item_offsets", "item_values")):
        got_off, got_val = utf8_buffers(arr)
        assert np.array_equal(got_off, want[off]) and np.array_equal(got_val, want[val])


def test_a_fused_plan_over_a_scan_with_the_bit_set(ctx, twins):
    paths, _maps = twins

    def k6(project):
        scan = exon_amd.Scan(str(paths["bgzf"]), "gff", gpu_parse=True, project=project)
        plan = ctx.plan_overlap_count(0, 1000, 30000, columns=(0, 3, 4))
        st = plan.open()
        st.set_region_contig("chr7")
        rows = st.consume(scan)
        counts, _ = st.finish()
        decoded = scan.decoded_on_gpu()
        st.close(); plan.close(); scan.close()
        return rows, int(counts[0]), decoded

    without = k6(())
    assert without[0] == 15000 and without[1] > 100 and without[2] == (True, True)
    assert k6(("attributes",)) == without
