"""exon-hip-cli: `SELECT * FROM depth_thresholds('<file>', '<regions.bed>', '<T1,T2,...>')` runs the region-set depth plan (kind 14) --
one row per BED line, in file order: its bases and how many of them are covered at least T times; a BED (chrom, s, e) is the 1-based
closed interval [s + 1, e].  The GPU case runs over the reference's SAM fixture, decoded on the device and, with EXON_HIP_GPU_PARSE=0,
by the host reader, against the host reader's rows piled up per base; the refusals need no device."""
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import flag_predicate_expect as FE
import region_depth_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "exon_amd", "bin", "exon-hip-cli")
SAM = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "sam", "test.sam")


def table(out):
    return [[c.strip() for c in line.strip("|").split("|")] for line in out.splitlines() if line.startswith("|")]


def run(sql, **env):
    e = dict(os.environ)
    e.pop("EXON_HIP_GPU_PARSE", None)
    e.update(env)
    return subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, timeout=600, env=e)


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [None, "0"])
def test_cli_depth_thresholds_over_the_sam_fixture(tmp_path, gpu_parse):
    cols, _ = FE.table(exon_amd.Scan(SAM, "sam", gpu_parse=False))
    ref, s, e = cols["reference"][0], cols["start"][0], cols["end"][0]
    regions = [(ref, s, e), (ref, max(1, s - 5), s + 2), ("not-in-the-file", 1, 100), (ref, e, e + 40), (ref, s, e)]
    bed = tmp_path / "targets.bed"
    bed.write_text("# targets\n" + "".join("%s\t%d\t%d\tname\r\n" % (c, a - 1, b) for c, a, b in regions))
    r = run(f"SELECT * FROM depth_thresholds('{SAM}', '{bed}', '1, 2,30')", **({} if gpu_parse is None else {"EXON_HIP_GPU_PARSE": gpu_parse}))
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    assert t[0] == ["contig", "start", "end", "bases", "ge_1", "ge_2", "ge_30"]
    assert [row[:3] for row in t[1:]] == [[c, str(a), str(b)] for c, a, b in regions]
    # the host reader's rows, piled up per base
    ids = {ref: 0, "not-in-the-file": 1}
    names = cols["reference"]
    rows = (np.array([ids.get(c, 9) for c in names], np.int32), np.array(cols["start"], np.int64), np.array(cols["end"], np.int64))
    _, _, bases, ge = E.expect([(ids[c], a, b) for c, a, b in regions], [1, 2, 30], *rows)
    assert [[int(x) for x in row[3:]] for row in t[1:]] == [[int(b)] + g.tolist() for b, g in zip(bases, ge)]
    assert bases[0] == e - s + 1 == ge[0][0] and bases[2] == 0 and bases[3] == 1


def test_refusals(tmp_path):
    bed = tmp_path / "t.bed"
    bed.write_text("chr1\t0\t10\n")
    for bad in ("10,1", "5,5", "0", "1,,2", "", "1,2,3,4,5,6,7,8,9", "1,x", "2,"):  # not increasing, below 1, empty, nine of them, no number
        r = run(f"SELECT * FROM depth_thresholds('{SAM}', '{bed}', '{bad}')")
        assert r.returncode != 0 and "depth_thresholds" in r.stderr and "strictly increasing" in r.stderr, bad
    r = run(f"SELECT * FROM depth_thresholds('{bed}', '{bed}', '1')")  # a BED source is out of scope, for overlap_counts' reason
    k11 = run(f"SELECT * FROM overlap_counts('{bed}', '{bed}')")
    assert r.returncode != 0 and "BED source" in r.stderr and "depth_thresholds" in r.stderr
    assert r.stderr.replace("depth_thresholds", "overlap_counts") == k11.stderr
    r = run(f"SELECT * FROM depth_thresholds('{SAM}', '{tmp_path / 'missing.bed'}', '1')")
    assert r.returncode != 0 and "no such file" in r.stderr
    r = run(f"SELECT * FROM depth_thresholds('{SAM}', '{bed}')")  # the thresholds are not optional
    assert r.returncode != 0
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "depth_thresholds('<bam|sam|cram|gff|gtf file>', '<regions.bed>', '<T1,T2,...>'" in r.stdout + r.stderr
