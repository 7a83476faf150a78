"""exon-hip-cli over GFF: STORED AS GFF / INDEXED_GFF, gff_scan, gff_indexed_scan and gff_region_filter.  CPU part: the counts of
the reference's slt (gff-scan-tests.slt) through the host reader.  GPU part: the filtered count is K2 over (seqname, start) with
the text parsed on the device, and equals the host reader's."""
import gzip
import os
import subprocess

import pytest

import gff_expect
from test_cli import CLI, last_count, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "gff")
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")


def test_count_star_over_gff_sources(tmp_path):
    assert last_count(run(f"SELECT COUNT(*) FROM gff_scan('{FIX}/ecoli.gff')").stdout) == 7           # gff-scan-tests.slt
    assert last_count(run(f"SELECT COUNT(*) FROM gff_scan('{FIX}/test.gff.gz', 'gzip')").stdout) == 5000
    t = f"CREATE EXTERNAL TABLE g STORED AS GFF OPTIONS (compression gzip) LOCATION '{FIX}/test.gff3.gz';"
    assert last_count(run(t + "SELECT COUNT(*) FROM g; DROP TABLE g;").stdout) == 5000
    # a directory: .gff and .gff3 files (and their .gz twins) are the table's
    (tmp_path / "a.gff").write_bytes(open(os.path.join(FIX, "ecoli.gff"), "rb").read())
    (tmp_path / "b.gff3").write_bytes(open(os.path.join(FIX, "bad-directive.gff"), "rb").read())
    (tmp_path / "c.txt").write_bytes(b"not a table file\n")
    t = f"CREATE EXTERNAL TABLE g STORED AS GFF LOCATION '{tmp_path}';"
    assert last_count(run(t + "SELECT COUNT(*) FROM g").stdout) == 14
    r = run(f"SELECT COUNT(*) FROM gff_scan('{FIX}/test.gff.zst')", ok=False)
    assert r.returncode != 0 and "zstd" in r.stderr


def _host(*cmds):
    r = subprocess.run([CLI, "-q", "-c", *cmds], capture_output=True, text=True, env=dict(os.environ, EXON_HIP_GPU_PARSE="0"), timeout=600)
    assert r.returncode == 0, r.stderr
    return last_count(r.stdout)


def test_region_filter_and_indexed_table_on_the_host(tmp_path):
    text = gzip.open(os.path.join(FIX, "test.gff.gz")).read()
    for region, args in (("sq0", "seqname"), ("sq0:1-9", "seqname, start"), ("sq1:8", "seqname, start"), ("nope", "seqname")):
        want = gff_expect.expect(text, region)["n_rows"]
        assert _host(f"SELECT COUNT(*) FROM gff_scan('{FIX}/test.gff.gz', 'gzip') WHERE gff_region_filter('{region}', {args}) = true") == want
    assert gff_expect.expect(text, "sq0")["n_rows"] > 0
    p, gz = tmp_path / "s.gff", tmp_path / "s.gff.gz"
    subprocess.check_call([GEN, "gff", "30000", str(p)])
    subprocess.check_call([BGZIP, str(p), str(gz), "6"])
    gff_expect.write_gff_tabix(gz)
    want = gff_expect.expect(open(p, "rb").read(), "chr5:20000-90000")["n_rows"]
    t = f"CREATE EXTERNAL TABLE g STORED AS INDEXED_GFF OPTIONS (compression gzip) LOCATION '{gz}';"
    assert _host(t + "SELECT COUNT(*) AS cnt FROM g WHERE gff_region_filter('chr5:20000-90000', seqname, start) = true") == want > 100
    assert _host(f"SELECT COUNT(*) FROM gff_indexed_scan('{gz}', 'chr5:20000-90000')") == want
    r = run(t + "SELECT COUNT(*) FROM g", ok=False)
    assert r.returncode != 0 and "region" in r.stderr


@pytest.mark.gpu
def test_region_filter_runs_k2_on_the_device(tmp_path):
    p = tmp_path / "s.gff"
    subprocess.check_call([GEN, "gff", "300000", str(p)])
    text = open(p, "rb").read()
    gz = tmp_path / "s.gff.gz"
    subprocess.check_call([BGZIP, str(p), str(gz), "6"])
    for region in ("chr7", "chr7:100000-900000", "chrM", "chrY:1200000"):
        want = gff_expect.expect(text, region)["n_rows"]
        for src in (f"gff_scan('{p}')", f"gff_scan('{gz}', 'gzip')"):
            sql = f"SELECT COUNT(*) FROM {src} WHERE gff_region_filter('{region}', seqname, start)"
            env = dict(os.environ, EXON_HIP_GPU_PARSE_STRICT="1")  # the device decides every record, or the query fails
            r = subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, env=env, timeout=600)
            assert r.returncode == 0, r.stderr
            assert last_count(r.stdout) == want == _host(sql), (region, src)
