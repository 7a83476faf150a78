"""exon-hip-cli: `SELECT * FROM overlap_counts('<file>', '<regions.bed>')` runs the region-set overlap plan (kind 11) -- one row per BED
line, in file order; a BED (chrom, s, e) is the 1-based closed interval [s + 1, e].  The GPU case runs over the reference's BAM
fixture, decoded on the device and, with EXON_HIP_GPU_PARSE=0, by the host reader; the refusals need no device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "exon_amd", "bin", "exon-hip-cli")
BAM = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "bam", "test.bam")

# chr1:1-12209145 holds 7 of the fixture's reads (slt/bam-indexed-select-tests.slt:16-19)
BED = "# targets\nchr1\t0\t12209145\tfirst\nchr1\t12209145\t250000000\nnot-in-the-file\t0\t100\nchr1\t0\t250000000\r\nchr1\t0\t12209145\n"


def table(out):
    return [[c.strip() for c in line.strip("|").split("|")] for line in out.splitlines() if line.startswith("|")]


def run(sql, **env):
    e = dict(os.environ)
    e.pop("EXON_HIP_GPU_PARSE", None)
    e.update(env)
    return subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, timeout=600, env=e)


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [None, "0"])
def test_cli_overlap_counts_over_the_bam_fixture(tmp_path, gpu_parse):
    bed = tmp_path / "targets.bed"
    bed.write_text(BED)
    r = run(f"SELECT * FROM overlap_counts('{BAM}', '{bed}')", **({} if gpu_parse is None else {"EXON_HIP_GPU_PARSE": gpu_parse}))
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    assert t[0] == ["contig", "start", "end", "count"]
    assert [row[:3] for row in t[1:]] == [["chr1", "1", "12209145"], ["chr1", "12209146", "250000000"], ["not-in-the-file", "1", "100"],
                                          ["chr1", "1", "250000000"], ["chr1", "1", "12209145"]]
    counts = [int(row[3]) for row in t[1:]]
    assert counts == [7, 61, 0, 61, 7]  # (the seven reads that start in front of 12209146 end behind it: all 61 overlap the second region)
    # the same question, one region at a time, through K6
    k6 = run(f"SELECT COUNT(*) FROM bam_scan('{BAM}') WHERE bam_region_filter('chr1:12209146-250000000', reference, start, end)")
    assert k6.returncode == 0 and int(table(k6.stdout)[-1][0]) == counts[1]


def test_a_zero_length_region_is_an_error_that_names_the_line(tmp_path):
    bed = tmp_path / "bad.bed"
    bed.write_text("chr1\t0\t10\n\nchr1\t55\t55\n")
    r = run(f"SELECT * FROM overlap_counts('{BAM}', '{bed}')")
    assert r.returncode != 0
    assert "line 3" in r.stderr and "zero-length region" in r.stderr and "chr1:55-55" in r.stderr


def test_other_refusals(tmp_path):
    bed = tmp_path / "t.bed"
    bed.write_text("chr1\t0\t10\n")
    r = run(f"SELECT * FROM overlap_counts('{bed}', '{bed}')")  # a BED source is out of scope
    assert r.returncode != 0 and "BED source" in r.stderr
    r = run(f"SELECT * FROM overlap_counts('{BAM}', '{tmp_path / 'missing.bed'}')")
    assert r.returncode != 0 and "no such file" in r.stderr
    bed.write_text("chr1\t10\t5\n")
    r = run(f"SELECT * FROM overlap_counts('{BAM}', '{bed}')")
    assert r.returncode != 0 and "line 1" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "overlap_counts('<bam|sam|cram|gff|gtf file>', '<regions.bed>'" in r.stdout + r.stderr
