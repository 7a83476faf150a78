"""exon-hip-cli over GTF: STORED AS GTF, gtf_scan, the extension .gtf and OPTIONS (compression gzip).  CPU part: the pins of the
reference's slt (gtf-scan-tests.slt: 77 rows, the first row) through the host reader, and the region filter.  GPU part: the
filtered count is K2 over (seqname, start) with the text parsed on the device, and equals the host reader's."""
import os
import subprocess

import pytest

import gtf_expect
from test_cli import CLI, last_count, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "gtf")
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")


def test_count_star_over_gtf_sources(tmp_path):
    assert last_count(run(f"SELECT COUNT(*) FROM gtf_scan('{FIX}/test.gtf')").stdout) == 77           # gtf-scan-tests.slt
    assert last_count(run(f"SELECT COUNT(*) FROM gtf_scan('{FIX}/test.gtf.gz', 'gzip')").stdout) == 77
    t = f"CREATE EXTERNAL TABLE g STORED AS GTF LOCATION '{FIX}/test.gtf';"
    assert last_count(run(t + "SELECT COUNT(*) FROM g; DROP TABLE g;").stdout) == 77
    t = f"CREATE EXTERNAL TABLE g STORED AS GTF OPTIONS (compression gzip) LOCATION '{FIX}/test.gtf.gz';"
    assert last_count(run(t + "SELECT COUNT(*) FROM g").stdout) == 77
    # a directory: its .gtf files are the table's
    (tmp_path / "a.gtf").write_bytes(open(os.path.join(FIX, "test.gtf"), "rb").read())
    (tmp_path / "b.gtf").write_bytes(open(os.path.join(FIX, "test.gtf"), "rb").read())
    (tmp_path / "c.gff").write_bytes(b"not a table file\n")
    t = f"CREATE EXTERNAL TABLE g STORED AS GTF LOCATION '{tmp_path}';"
    assert last_count(run(t + "SELECT COUNT(*) FROM g").stdout) == 154
    r = run(f"CREATE EXTERNAL TABLE g STORED AS INDEXED_GTF LOCATION '{FIX}/test.gtf'", ok=False)
    assert r.returncode != 0 and "GTF" in r.stderr


def cells(line):
    return [c.strip() for c in line.strip().strip("|").split("|")]


@pytest.mark.parametrize("src", [f"gtf_scan('{FIX}/test.gtf')", f"gtf_scan('{FIX}/test.gtf.gz', 'gzip')"])
def test_first_row_select(src):
    # gtf-scan-tests.slt: SELECT seqname, source, type, start, end, score, strand, frame FROM gtf_table LIMIT 1
    out = run(f"SELECT seqname, source, type, start, end, score, strand, frame FROM {src} LIMIT 1").stdout
    rows = [cells(ln) for ln in out.splitlines() if ln.startswith("|")]
    assert rows == [["seqname", "source", "type", "start", "end", "score", "strand", "frame"],
                    ["chr1", "processed_transcript", "exon", "11869", "12227", "NULL", "+", "NULL"]]
    out = run(f"SELECT * FROM {src} LIMIT 3").stdout  # (the map is not printed)
    rows = [cells(ln) for ln in out.splitlines() if ln.startswith("|")]
    assert len(rows) == 4 and rows[0][-1] == "frame" and rows[3][3] == "13221"
    out = run(f"SELECT start, strand FROM {src}").stdout
    assert len([ln for ln in out.splitlines() if ln.startswith("|")]) == 78


def _host(*cmds):
    r = subprocess.run([CLI, "-q", "-c", *cmds], capture_output=True, text=True, env=dict(os.environ, EXON_HIP_GPU_PARSE="0"), timeout=600)
    assert r.returncode == 0, r.stderr
    return last_count(r.stdout)


def test_region_filter_on_the_host():
    text = open(os.path.join(FIX, "test.gtf"), "rb").read()
    for region, args in (("chr1", "seqname"), ("chr1:12000-13000", "seqname, start"), ("chr1:14000", "seqname, start"), ("nope", "seqname")):
        want = gtf_expect.expect(text, region)["n_rows"]
        assert _host(f"SELECT COUNT(*) FROM gtf_scan('{FIX}/test.gtf.gz', 'gzip') WHERE gff_region_filter('{region}', {args}) = true") == want
    assert 0 < gtf_expect.expect(text, "chr1:12000-13000")["n_rows"] < 77


@pytest.mark.gpu
def test_region_filter_runs_k2_on_the_device(tmp_path):
    p = tmp_path / "s.gtf"
    subprocess.check_call([GEN, "gtf", "100000", str(p)])
    names, seq, start, _ = gtf_expect.gff_expect.interval_columns(open(p, "rb").read())
    gz = tmp_path / "s.gtf.gz"
    subprocess.check_call([BGZIP, str(p), str(gz), "6"])
    for region in ("chr7", "chr7:100000-300000", "chrM", "chrY:200000"):
        name, a, b = gtf_expect.parse_region(region)
        want = int(((seq == (names.index(name) if name in names else -1)) & (start >= a) & (start <= b)).sum())
        for src in (f"gtf_scan('{p}')", f"gtf_scan('{gz}', 'gzip')"):
            sql = f"SELECT COUNT(*) FROM {src} WHERE gff_region_filter('{region}', seqname, start)"
            env = dict(os.environ, EXON_HIP_GPU_PARSE_STRICT="1")  # the device decides every record, or the query fails
            r = subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, env=env, timeout=600)
            assert r.returncode == 0, r.stderr
            assert last_count(r.stdout) == want, (region, src)
    assert want > 0
