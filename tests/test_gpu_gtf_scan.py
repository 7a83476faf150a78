"""GPU: the GTF file pipeline -- text, BGZF or plain gzip in HBM -> the device parser under the GTF dialect -> K2 / K6 / K7, or
(bound to a context) batches with the attributes map built on the device -- against tests/gtf_expect.py and the host reader: the
reference's two fixtures, a generated file of two slabs in three compressions, batch sizes, a region that keeps one run and one
with scattered survivors, the hand-over at a non-ASCII value, and a fused plan over a scan that has the bit set."""
import gzip
import os
import subprocess
import zlib

import pytest

import exon_amd
import gtf_expect
from test_gtf_scan import FIX, assert_same, fixture_text, scan_gtf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
BIG = 2**63 - 1


def run_plan(ctx, path, kind, region, gpu_parse=True, project=()):
    name, a, b = region
    scan = exon_amd.Scan(str(path), "gtf", gpu_parse=gpu_parse, project=project)
    plan = {"k2": lambda: ctx.plan_region_count(0, a, b, columns=(0, 3)), "k6": lambda: ctx.plan_overlap_count(0, a, b, columns=(0, 3, 4)),
            "k7": lambda: ctx.plan_within_count(0, a, b, columns=(0, 3, 4))}[kind]()
    st = plan.open()
    st.set_region_contig(name)
    rows = st.consume(scan)
    counts, _ = st.finish()
    decoded = scan.decoded_on_gpu()
    st.close(); plan.close(); scan.close()
    return rows, int(counts[0]), decoded


def numpy_counts(want, region):
    name, a, b = region
    hi = BIG if b is None else b
    sel = want["seqname"] == name
    start, end = want["start"], want["end"]
    return {"k2": int((sel & (start >= a) & (start <= hi)).sum()), "k6": int((sel & (start <= hi) & (end >= a)).sum()),
            "k7": int((sel & (start > a) & (end < hi)).sum())}


@pytest.mark.parametrize("name", ["test.gtf", "test.gtf.gz"])
def test_fixtures_through_k2_k6_k7(ctx, name):
    want = gtf_expect.expect(fixture_text(name))
    assert want["n_rows"] == 77
    for region in (("chr1", 12000, 13500), ("chr1", 1, None), ("chr1", 14000, 14500), ("chr2", 1, None)):
        counts = numpy_counts(want, region)
        for kind in ("k2", "k6", "k7"):
            rows, count, decoded = run_plan(ctx, os.path.join(FIX, name), kind, region)
            assert (rows, count) == (77, counts[kind]), (region, kind)
            # decoded on the device; the .gz fixture (one plain-gzip member with a file name) is inflated there too
            assert decoded == (True, name.endswith(".gz")), (region, kind)
            assert run_plan(ctx, os.path.join(FIX, name), kind, region, gpu_parse=False)[:2] == (77, counts[kind])
    assert numpy_counts(want, ("chr1", 12000, 13500))["k2"] > 0
    assert numpy_counts(want, ("chr1", 12000, 13500))["k6"] > numpy_counts(want, ("chr1", 12000, 13500))["k7"] > 0


@pytest.mark.parametrize("name", ["test.gtf", "test.gtf.gz"])
def test_fixture_batches_from_the_device(ctx, name):
    got = scan_gtf(os.path.join(FIX, name), bind=ctx)
    assert got["decoded_on_gpu"] and got["n_rows"] == 77
    assert_same(got, gtf_expect.expect(fixture_text(name), attrs=True), name)
    got = scan_gtf(os.path.join(FIX, name), bind=ctx, attributes=False, batch_size=7)
    assert got["decoded_on_gpu"] and got["sizes"] == [7] * 11
    assert_same(got, gtf_expect.expect(fixture_text(name)), name)


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    """gen_text gtf 30000 attrs (about 6 MB: two slabs at EXON_HIP_GPU_PARSE_SLAB_MB=1 in every compression) as plain text, BGZF and
    plain gzip; its text and what a scan of it returns"""
    d = tmp_path_factory.mktemp("gtfpipe")
    p, bgz, gz = d / "a.gtf", d / "a.gtf.bgz.gz", d / "a.gtf.gz"
    subprocess.check_call([GEN, "gtf", "30000", str(p), "attrs"])
    subprocess.check_call([BGZIP, str(p), str(bgz), "6"])
    text = open(p, "rb").read()
    assert 5 << 20 < len(text) < 8 << 20
    # plain gzip in DEFLATE blocks of at most 1024 symbols (memLevel 4), so that a block never inflates to more than a 1 MiB slab
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 4)
    gz.write_bytes(co.compress(text) + co.flush())
    assert gzip.decompress(gz.read_bytes()) == text
    return {"plain": p, "bgzf": bgz, "gzip": gz}, text, gtf_expect.expect(text, attrs=True)


@pytest.mark.parametrize("batch_size", [1000, 8192])
@pytest.mark.parametrize("twin", ["plain", "bgzf", "gzip"])
def test_two_slabs_in_three_compressions(ctx, twins, monkeypatch, twin, batch_size):
    paths, _text, want = twins
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    monkeypatch.setenv("EXON_HIP_GZ_SLAB_MB", "1")  # (plain-gzip slabs are cut by output bytes, by a switch of their own)
    got = scan_gtf(paths[twin], bind=ctx, batch_size=batch_size)
    assert got["decoded_on_gpu"] and max(got["sizes"]) <= batch_size
    if batch_size == 8192:  # batches end with their slab: one slab would give four
        assert len(got["sizes"]) >= 5, got["sizes"]
    assert_same(got, want, twin)
    if batch_size == 8192:
        assert_same(scan_gtf(paths[twin], batch_size=batch_size), want, twin + " host")


@pytest.mark.parametrize("gather", ["0", "1"])
def test_a_region_that_keeps_one_run(ctx, twins, monkeypatch, gather):
    paths, text, _want = twins
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    monkeypatch.setenv("EXON_HIP_EXPORT_GATHER", gather)  # 1: the same rows through the row-by-row gather
    for region in ("chr7:1000-60000", "chr1", "chrM", "chrY:1-50"):
        want = gtf_expect.expect(text, region, attrs=True)
        for batch_size in (16, 8192):
            got = scan_gtf(paths["plain"], bind=ctx, region=region, batch_size=batch_size)
            assert got["decoded_on_gpu"], (region, batch_size)
            assert_same(got, want, (region, batch_size))
    assert gtf_expect.expect(text, "chr7:1000-60000")["n_rows"] > 100


def test_a_region_with_scattered_survivors(ctx, twins, tmp_path, monkeypatch):
    """every other row on another seqname: more kept runs than the views take, so the two-level map gather builds the batches"""
    _paths, text, _want = twins
    monkeypatch.delenv("EXON_HIP_EXPORT_GATHER", raising=False)
    rows = [ln for ln in text.split(b"\n")[2:1400] if ln and not ln.startswith(b"#")]
    alt = b"".join((b"chrA" if i % 2 else b"chrB") + ln[ln.index(b"\t"):] + b"\n" for i, ln in enumerate(rows))
    p = tmp_path / "alt.gtf"
    p.write_bytes(alt)
    want = gtf_expect.expect(alt, "chrA", attrs=True)
    assert want["n_rows"] > 300
    got = scan_gtf(p, bind=ctx, region="chrA", batch_size=100)
    assert got["decoded_on_gpu"]
    assert_same(got, want)
    assert_same(scan_gtf(p, region="chrA"), want)


def test_a_non_ascii_value_in_the_second_slab_hands_over(ctx, twins, tmp_path, monkeypatch):
    _paths, text, _want = twins
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    cut = text.rfind(b"\n", 0, 2_500_000) + 1
    planted = text[:cut] + b'chrH\thavana\tgene\t5\t6\t.\t+\t.\tgene_name "caf\xc3\xa9"; n 1;\n' + text[cut:]
    p = tmp_path / "h.gtf"
    p.write_bytes(planted)
    want = gtf_expect.expect(planted, attrs=True)
    got = scan_gtf(p, bind=ctx, batch_size=8192)
    assert not got["decoded_on_gpu"], "the device cannot say whether the bytes are UTF-8"
    assert got["n_rows"] == 30001 and [("gene_name", "café"), ("n", "1")] in got["maps"]
    assert_same(got, want)
    # an attribute error in the same place: the error is the host reader's, and it quotes the line
    p.write_bytes(text[:cut] + b'chrH\thavana\tgene\t5\t6\t.\t+\t.\tgene_name "open\n' + text[cut:])
    with pytest.raises(exon_amd.ExonHipError) as e:
        scan_gtf(p, bind=ctx)
    assert "GTF line 'chrH\thavana\tgene\t5\t6" in str(e.value) and "closing quote" in str(e.value)


def test_a_fused_plan_over_a_scan_with_the_bit_set(ctx, twins):
    paths, text, want = twins
    region = ("chr7", 1000, 60000)
    counts = numpy_counts(want, region)
    without = run_plan(ctx, paths["bgzf"], "k6", region)
    assert without == (30000, counts["k6"], (True, True)) and counts["k6"] > 100
    assert run_plan(ctx, paths["bgzf"], "k6", region, project=("attributes",)) == without
    # nothing of the column is validated by a fused plan either: a ninth field the rules refuse does not stop it
    p = paths["plain"].parent / "broken.gtf"
    p.write_bytes(b'chr1\thavana\tgene\t5\t6\t.\t+\t.\tgene_id "open\n' + text)
    assert run_plan(ctx, p, "k6", region, project=("attributes",)) == (30001, counts["k6"], (True, False))
