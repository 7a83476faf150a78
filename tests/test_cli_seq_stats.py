"""GPU: exon-hip-cli runs `SELECT * FROM fasta_seq_stats('<path>')` through the per-record sequence statistics plan (kind 10) on the
reference's fixtures -- decoded on the device and, with EXON_HIP_GPU_PARSE=0, by the host reader -- against the pinned rows."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "exon_amd", "bin", "exon-hip-cli")
FX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "fasta")

# (a composition row shows its byte as a number: 65 A, 67 C, 71 G, 84 T)
WANT = [["total", "records", "2"], ["total", "bases", "8"], ["total", "gc", "4"],
        ["composition", "65", "2"], ["composition", "67", "2"], ["composition", "71", "2"], ["composition", "84", "2"],
        ["length", "4", "2"], ["length_log2", "3", "2"], ["gc_percent", "50", "2"]]


def table(out):
    return [[c.strip() for c in line.strip("|").split("|")] for line in out.splitlines() if line.startswith("|")]


@pytest.mark.parametrize("gpu_parse", [None, "0"])
@pytest.mark.parametrize("name,arg", [("test.fasta", ""), ("test.fasta.gz", ", 'gzip'")])
def test_cli_seq_stats_on_the_reference_fixtures(name, arg, gpu_parse):
    sql = f"SELECT * FROM fasta_seq_stats('{os.path.join(FX, name)}'{arg})"
    env = dict(os.environ)
    env.pop("EXON_HIP_GPU_PARSE", None)
    if gpu_parse is not None:
        env["EXON_HIP_GPU_PARSE"] = gpu_parse
    r = subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    assert t[0] == ["stat", "bin", "count"] and t[1:] == WANT


def test_usage_names_the_function():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "fasta_seq_stats('<path>'" in r.stdout + r.stderr
