"""The BED file pipeline on the GPU through the C ABI: file -> slabs in HBM (plain text, gzip and BGZF inflated on the device) ->
k_parse_bed_lines -> K2 / K6 / K7 over columns (0, 1, 2), and the batches of exon_hip_scan_bind_ctx, against the host reader and
tests/bed_expect.py."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import bed_expect
from test_bed_scan import ALL, assert_same, scan_bed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
BIG = 2**63 - 1


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """20 000 generated rows of mixed field counts as plain text, BGZF and plain gzip; bed_expect's columns of them, computed once"""
    d = tmp_path_factory.mktemp("bedgpu")
    p, bgz, gz = d / "m.bed", d / "m.bed.bgz", d / "m.bed.gz"
    subprocess.check_call([GEN, "bed", "20000", str(p), "mix"])
    subprocess.check_call([BGZIP, str(p), str(bgz), "6"])
    text = open(p, "rb").read()
    with gzip.open(gz, "wb", compresslevel=1) as fh:
        fh.write(text)
    return {"plain": p, "bgzf": bgz, "gzip": gz}, text, bed_expect.expect(text)


def run_plan(ctx, path, kind, region, gpu_parse):
    """-> (rows consumed, the plan's count, decoded on the device, inflated on the device)"""
    name, a, b = region
    scan = exon_amd.Scan(str(path), "bed", gpu_parse=gpu_parse)
    plan = {"k2": lambda: ctx.plan_region_count(0, a, b, columns=(0, 1)), "k6": lambda: ctx.plan_overlap_count(0, a, b, columns=(0, 1, 2)),
            "k7": lambda: ctx.plan_within_count(0, a, b, columns=(0, 1, 2))}[kind]()
    st = plan.open()
    st.set_region_contig(name)
    try:
        rows = st.consume(scan)
        counts, _ = st.finish()
        decoded, inflated = scan.decoded_on_gpu()
    finally:
        st.close(); plan.close(); scan.close()
    return rows, int(counts[0]), decoded, inflated


REGIONS = [("chr7", 10_000, 60_000), ("chr1", 1, None), ("chrY", 40_000, 41_000), ("chrM", 1, 100)]


def test_k2_k6_k7_over_the_device_parsed_columns(ctx, mixed, monkeypatch):
    paths, _text, want = mixed
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")  # several slabs a file: lines carried across them
    chrom, start, end = np.array(want["chrom"], object), want["start"], want["end"]
    n = want["n_rows"]
    for region in REGIONS:
        name, a, b = region
        hi = BIG if b is None else b
        sel = chrom == name.encode()
        counts = {"k2": int((sel & (start >= a) & (start <= hi)).sum()), "k6": int((sel & (start <= hi) & (end >= a)).sum()),
                  "k7": int((sel & (start > a) & (end < hi)).sum())}  # (K7 is the strict form: start > a AND end < b)
        for kind in ("k2", "k6", "k7"):
            assert run_plan(ctx, paths["plain"], kind, region, False) == (n, counts[kind], False, False), (region, kind, "host")
            for twin in (("plain", "bgzf", "gzip") if region is REGIONS[0] else ("plain",)):
                got = run_plan(ctx, paths[twin], kind, region, True)
                assert got == (n, counts[kind], True, twin != "plain"), (region, kind, twin)  # decoded_on_gpu == 1: no silent hand-over
        if region is REGIONS[0]:
            assert 0 < counts["k7"] < counts["k6"] and counts["k2"] > 0


def test_a_bad_line_in_the_last_slab_gives_the_hosts_error_on_both_paths(ctx, mixed, tmp_path, monkeypatch):
    _paths, text, want = mixed
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    text = text * 3  # three slabs of 1 MiB
    assert len(text) > (2 << 20)
    bad = tmp_path / "bad.bed"
    bad.write_bytes(text + b"chrY\t5\t9\tlast\t65536\t+\n")
    errors = []
    for gpu_parse in (False, True):
        with pytest.raises(exon_amd.ExonHipError) as e:
            run_plan(ctx, bad, "k7", REGIONS[0], gpu_parse)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "invalid score '65536'" in errors[0] and "BED line 'chrY\t5\t9\tlast" in errors[0]
    # a row only the host decides (six score digits) finishes through the hand-over with the host's answer
    odd = tmp_path / "odd.bed"
    odd.write_bytes(text + b"chr7\t10001\t10002\tlast\t000001\t+\n")
    host = run_plan(ctx, odd, "k7", REGIONS[0], False)
    got = run_plan(ctx, odd, "k7", REGIONS[0], True)
    assert got[:2] == host[:2] and host[0] == 3 * want["n_rows"] + 1 and not got[2]
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_STRICT", "1")
    with pytest.raises(exon_amd.ExonHipError):
        run_plan(ctx, odd, "k7", REGIONS[0], True)


def test_many_names_finish_through_the_hand_over(ctx, tmp_path):
    p = tmp_path / "many.bed"
    p.write_bytes(b"".join(b"contig_%d\t%d\t%d\n" % (i % 5000, i, i + 50) for i in range(20_000)))
    want = sum(1 for i in range(20_000) if i % 5000 == 77 and i <= 12_000 and i + 50 >= 100)
    assert run_plan(ctx, p, "k6", ("contig_77", 100, 12_000), False) == (20_000, want, False, False) and want == 3
    assert run_plan(ctx, p, "k6", ("contig_77", 100, 12_000), True) == (20_000, want, False, False)


MASKS = [(), ("name",), tuple(ALL)]


@pytest.mark.parametrize("twin", ["plain", "gzip", "bgzf"])
def test_batches_from_the_gpu_pipeline_equal_the_host_readers(ctx, mixed, twin, monkeypatch):
    paths, _text, want = mixed
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    for project in MASKS:
        got = scan_bed(paths[twin], project=project, bind=ctx)
        assert got["decoded_on_gpu"] and got["n_rows"] == 20000, (twin, project)  # decoded_on_gpu == 1: no silent hand-over
        assert max(got["sizes"]) <= 8192  # (batches are cut slab by slab)
        assert_same(got, want, (twin, project))
        host = scan_bed(paths[twin], project=project)
        assert_same(host, want, (twin, project, "host"))
        for key in got:
            if key not in ("decoded_on_gpu", "sizes"):
                assert np.array_equal(got[key], host[key]) if isinstance(got[key], np.ndarray) else got[key] == host[key], (twin, project, key)
    if twin == "plain":
        for project in (("score", "block_count"), ("strand",), ("name", "strand", "block_starts")):  # scattered bits
            assert_same(scan_bed(paths[twin], project=project, bind=ctx, batch_size=777), want, project)


def test_batches_hand_over_and_dictionaries(ctx, mixed, tmp_path, monkeypatch):
    paths, text, want = mixed
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    s = exon_amd.Scan(str(paths["plain"]), "bed", gpu_parse=True, project=("score", "strand")).bind_ctx(ctx)
    assert sum(len(b) for b in s) == 20000 and sorted(s.dictionary(0)) == sorted({c.decode() for c in want["chrom"]}) and s.dictionary(4) == ["+", "-"]
    s.close()
    # a row only the host reads (UTF-8 beyond ASCII) in a later slab: the host reader takes over behind the rows emitted
    big = text * 3
    cut = big.rfind(b"\n", 0, 2_500_000) + 1
    odd = tmp_path / "odd.bed"
    odd.write_bytes(big[:cut] + "chr20\t1\t2\tcaf\u00e9\t5\t+\n".encode() + big[cut:])
    got = scan_bed(odd, bind=ctx)
    assert not got["decoded_on_gpu"] and got["n_rows"] == 60001
    assert_same(got, scan_bed(odd), "hand-over")
    assert "café".encode() in got["names"]
    # ... and a bad line raises the host's error from the GPU pipeline too
    bad = tmp_path / "bad.bed"
    bad.write_bytes(big + b"chrY\t5\t9\tlast\t65536\t+\n")
    errors = []
    for bind in (None, ctx):
        with pytest.raises(exon_amd.ExonHipError) as e:
            scan_bed(bad, bind=bind)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "invalid score '65536'" in errors[0]
