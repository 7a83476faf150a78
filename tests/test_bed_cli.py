"""exon-hip-cli over BED: STORED AS BED, bed_scan, the extension .bed, OPTIONS (compression gzip, n_fields N).  CPU part: the pins of
the reference's slt (bed-select-tests.slt: 10 rows, the first row with its six NULLs, 1 row of the gzip fixture, the 256-byte name)
through the host reader.  GPU part: the filtered count is K2 over (reference_sequence_name, start) with the text parsed on the
device, and equals what the host reader gives."""
import os
import subprocess

import numpy as np
import pytest

import bed_expect
from test_cli import CLI, last_count, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "bed")
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")


def cells(line):
    return [c.strip() for c in line.strip().strip("|").split("|")]


def table(out):
    return [cells(ln) for ln in out.splitlines() if ln.startswith("|")]


def test_count_star_over_bed_sources(tmp_path):
    assert last_count(run(f"SELECT COUNT(*) FROM bed_scan('{FIX}/test.bed')").stdout) == 10             # bed-select-tests.slt
    assert last_count(run(f"SELECT COUNT(*) FROM bed_scan('{FIX}/test.bed.gz', 'gzip')").stdout) == 1
    t = f"CREATE EXTERNAL TABLE bed STORED AS BED LOCATION '{FIX}/test.bed';"
    assert last_count(run(t + "SELECT COUNT(*) as cnt FROM bed; DROP TABLE bed;").stdout) == 10
    t = f"CREATE EXTERNAL TABLE bed STORED AS BED OPTIONS (compression gzip) LOCATION '{FIX}/test.bed.gz';"
    assert last_count(run(t + "SELECT COUNT(*) FROM bed").stdout) == 1
    # a directory: its .bed files are the table's
    for name in ("a.bed", "b.bed"):
        (tmp_path / name).write_bytes(open(os.path.join(FIX, "test.bed"), "rb").read())
    (tmp_path / "c.gff").write_bytes(b"not a table file\n")
    assert last_count(run(f"SELECT COUNT(*) FROM bed_scan('{tmp_path}')").stdout) == 20
    r = run(f"CREATE EXTERNAL TABLE bed STORED AS INDEXED_BED LOCATION '{FIX}/test.bed'", ok=False)
    assert r.returncode != 0 and "BED" in r.stderr
    r = run(f"SELECT COUNT(*) FROM bed_scan('{FIX}/test.bed.zst')", ok=False)
    assert r.returncode != 0 and "zstd" in r.stderr


def test_first_row_with_its_nulls():
    # bed-select-tests.slt: SELECT * FROM bed LIMIT 1
    t = f"CREATE EXTERNAL TABLE bed STORED AS BED LOCATION '{FIX}/test.bed';"
    rows = table(run(t + "SELECT * FROM bed LIMIT 1").stdout)
    assert rows == [bed_expect.COLUMNS, ["chr1", "11873", "12227", "NR_046018_exon_0_0_chr1_11874_f", "0", "+"] + ["NULL"] * 6]
    rows = table(run(f"SELECT * FROM bed_scan('{FIX}/test.bed.gz', 'gzip')").stdout)
    assert rows[1] == ["sq0", "7", "13", ".", "0"] + ["NULL"] * 7  # a '.' name stays ".", a '.' strand is NULL
    rows = table(run(f"SELECT * FROM bed_scan('{FIX}/test3.bed') LIMIT 2").stdout)
    assert rows[1:] == [["chr1", "11873", "12227"] + ["NULL"] * 9, ["chr1", "12612", "12721"] + ["NULL"] * 9]
    rows = table(run(f"SELECT start, strand, name FROM bed_scan('{FIX}/test.bed')").stdout)
    assert len(rows) == 11 and rows[0] == ["start", "strand", "name"] and rows[4] == ["14361", "-", "NR_024540_exon_0_0_chr1_14362_r"]


def test_the_256_byte_name():
    t = f"CREATE EXTERNAL TABLE bed STORED AS BED LOCATION '{FIX}/name_256bytes.one.bed';"
    rows = table(run(t + "SELECT name FROM bed LIMIT 1").stdout)
    want = open(os.path.join(FIX, "name_256bytes.one.bed"), "rb").read().split(b"\n")[0].split(b"\t")[3].decode()
    assert len(want) == 256 and rows == [["name"], [want]]


def test_n_fields_option():
    for n in (3, 4, 6, 9, 12):
        t = f"CREATE EXTERNAL TABLE bed STORED AS BED OPTIONS (n_fields {n}) LOCATION '{FIX}/test.bed';"
        rows = table(run(t + "SELECT * FROM bed LIMIT 1").stdout)
        assert rows[0] == bed_expect.COLUMNS[:n]
        assert rows[1] == (["chr1", "11873", "12227", "NR_046018_exon_0_0_chr1_11874_f", "0", "+"] + ["NULL"] * 6)[:n]
    t = f"CREATE EXTERNAL TABLE bed STORED AS BED OPTIONS (n_fields 4) LOCATION '{FIX}/test.bed';"
    r = run(t + "SELECT score FROM bed", ok=False)
    assert r.returncode != 0 and "score" in r.stderr
    for n in (2, 13):
        r = run(f"CREATE EXTERNAL TABLE bed STORED AS BED OPTIONS (n_fields {n}) LOCATION '{FIX}/test.bed'", ok=False)
        assert r.returncode != 0 and "n_fields" in r.stderr


def test_a_bad_line_is_reported_with_the_line(tmp_path):
    p = tmp_path / "bad.bed"
    p.write_bytes(b"chr1\t1\t2\nchr1\t3\t4\tn\t70000\n")
    for sql in (f"SELECT COUNT(*) FROM bed_scan('{p}')", f"SELECT start FROM bed_scan('{p}')"):
        r = run(sql, ok=False)
        assert r.returncode != 0 and "invalid score '70000'" in r.stderr and "BED line 'chr1\t3\t4" in r.stderr


@pytest.mark.gpu
def test_region_predicate_runs_k2_on_the_device(tmp_path):
    p = tmp_path / "s.bed"
    subprocess.check_call([GEN, "bed", "100000", str(p), "mix"])
    want_cols = bed_expect.expect(open(p, "rb").read())
    chrom, start = np.array(want_cols["chrom"], object), want_cols["start"]
    gz = tmp_path / "s.bed.gz"
    subprocess.check_call([BGZIP, str(p), str(gz), "6"])
    for region, (name, a, b) in (("chr7", (b"chr7", 1, 2**62)), ("chr7:100000-300000", (b"chr7", 100000, 300000)), ("chrM", (b"chrM", 1, 2**62)),
                                 ("chrY:200000", (b"chrY", 200000, 2**62))):
        want = int(((chrom == name) & (start >= a) & (start <= b)).sum())
        for src in (f"bed_scan('{p}')", f"bed_scan('{gz}', 'gzip')"):
            sql = f"SELECT COUNT(*) FROM {src} WHERE gff_region_filter('{region}', reference_sequence_name, start)"
            env = dict(os.environ, EXON_HIP_GPU_PARSE_STRICT="1")  # the device decides every record, or the query fails
            r = subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, env=env, timeout=600)
            assert r.returncode == 0, r.stderr
            assert last_count(r.stdout) == want, (region, src)
            env = dict(os.environ, EXON_HIP_GPU_PARSE="0")  # ... and the host reader's rows give the same count
            r = subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, env=env, timeout=600)
            assert r.returncode == 0 and last_count(r.stdout) == want, (region, src, r.stderr)
    assert want > 0
