"""GPU: exon-hip-cli runs `SELECT * FROM fastq_read_stats('<path>')` through the per-read statistics plan (kind 9) on the
reference's fixture -- decoded on the device and, with EXON_HIP_GPU_PARSE=0, by the host reader -- against the pinned numbers."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "exon_amd", "bin", "exon-hip-cli")
FX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "fastq")

WANT = [["total", "reads", "2"], ["total", "bases", "128"], ["total", "gc", "34"], ["total", "quality_sum", "5768"],
        ["length", "64", "2"], ["gc_percent", "26", "2"], ["mean_quality", "48", "2"]]


def table(out):
    return [[c.strip() for c in line.strip("|").split("|")] for line in out.splitlines() if line.startswith("|")]


@pytest.mark.parametrize("gpu_parse", ["1", "0"])
@pytest.mark.parametrize("name,arg", [("test.fastq", ""), ("test.fastq.gz", ", 'gzip'"), ("test_bgzip.fastq.gz", ", 'gzip'")])
def test_cli_read_stats_on_the_reference_fixture(name, arg, gpu_parse):
    sql = f"SELECT * FROM fastq_read_stats('{os.path.join(FX, name)}'{arg})"
    r = subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, timeout=600, env=dict(os.environ, EXON_HIP_GPU_PARSE=gpu_parse))
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    assert t[0] == ["stat", "bin", "count"] and t[1:] == WANT
