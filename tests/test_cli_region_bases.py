"""exon-hip-cli: `SELECT * FROM covered_bases('<file>', '<regions.bed>')` runs the covered-bases plan (kind 12) -- one row per BED
line, in file order; a BED (chrom, s, e) is the 1-based closed interval [s + 1, e].  The GPU case runs over the reference's BAM
fixture, decoded on the device and, with EXON_HIP_GPU_PARSE=0, by the host reader; the refusals need no device."""
import os
import subprocess

import pytest

import exon_amd
import flag_predicate_expect as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "exon_amd", "bin", "exon-hip-cli")
BAM = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "bam", "test.bam")

BED = "# targets\nchr1\t0\t12209145\tfirst\nchr1\t12209145\t250000000\nnot-in-the-file\t0\t100\nchr1\t0\t250000000\r\nchr1\t12209144\t12209145\n"
REGIONS = [("chr1", 1, 12209145), ("chr1", 12209146, 250000000), ("not-in-the-file", 1, 100), ("chr1", 1, 250000000), ("chr1", 12209145, 12209145)]


def table(out):
    return [[c.strip() for c in line.strip("|").split("|")] for line in out.splitlines() if line.startswith("|")]


def run(sql, **env):
    e = dict(os.environ)
    e.pop("EXON_HIP_GPU_PARSE", None)
    e.update(env)
    return subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, timeout=600, env=e)


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [None, "0"])
def test_cli_covered_bases_over_the_bam_fixture(tmp_path, gpu_parse):
    bed = tmp_path / "targets.bed"
    bed.write_text(BED)
    r = run(f"SELECT * FROM covered_bases('{BAM}', '{bed}')", **({} if gpu_parse is None else {"EXON_HIP_GPU_PARSE": gpu_parse}))
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    assert t[0] == ["contig", "start", "end", "bases"]
    assert [row[:3] for row in t[1:]] == [[c, str(a), str(b)] for c, a, b in REGIONS]
    bases = [int(row[3]) for row in t[1:]]
    # the host reader's rows, clipped here
    cols, _ = FE.table(exon_amd.Scan(BAM, "bam", gpu_parse=False))
    want = [sum(max(0, min(e, b) - max(s, a) + 1) for n, s, e in zip(cols["reference"], cols["start"], cols["end"])
                if n == c and s is not None and e is not None and e >= s) for c, a, b in REGIONS]
    assert bases == want
    assert bases[0] + bases[1] == bases[3] > 0 and bases[2] == 0
    # a region of one base holds as many bases as reads overlap it: K11 over the same line
    k11 = run(f"SELECT * FROM overlap_counts('{BAM}', '{bed}')")
    assert k11.returncode == 0 and int(table(k11.stdout)[-1][3]) == bases[4] > 0


def test_a_zero_length_region_is_an_error_that_names_the_line(tmp_path):
    bed = tmp_path / "bad.bed"
    bed.write_text("chr1\t0\t10\n\nchr1\t55\t55\n")
    r = run(f"SELECT * FROM covered_bases('{BAM}', '{bed}')")
    assert r.returncode != 0
    assert "line 3" in r.stderr and "zero-length region" in r.stderr and "chr1:55-55" in r.stderr


def test_other_refusals(tmp_path):
    bed = tmp_path / "t.bed"
    bed.write_text("chr1\t0\t10\n")
    r = run(f"SELECT * FROM covered_bases('{bed}', '{bed}')")  # a BED source is out of scope, for overlap_counts' reason
    k11 = run(f"SELECT * FROM overlap_counts('{bed}', '{bed}')")
    assert r.returncode != 0 and "BED source" in r.stderr and "covered_bases" in r.stderr
    assert r.stderr.replace("covered_bases", "overlap_counts") == k11.stderr
    r = run(f"SELECT * FROM covered_bases('{BAM}', '{tmp_path / 'missing.bed'}')")
    assert r.returncode != 0 and "no such file" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "covered_bases('<bam|sam|cram|gff|gtf file>', '<regions.bed>'" in r.stdout + r.stderr
