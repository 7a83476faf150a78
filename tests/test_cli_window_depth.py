"""exon-hip-cli: `SELECT * FROM window_depth('<file>', <W>[, '<genome file>'])` runs the window plan (kind 13) -- one row per window
of width W along every contig, from the file's own header or from a bedtools genome file.  The GPU cases run over a written BAM,
decoded on the device and, with EXON_HIP_GPU_PARSE=0, by the host reader, against the Python rows; the refusals need no device."""
import os
import subprocess

import numpy as np
import pytest

import bam_sam_writer as bsw
import exon_amd
import window_bases_expect as E
from test_flag_predicate import BGZIP, mixed
from test_gpu_window_bases_scan import by_slot, host_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "exon_amd", "bin", "exon-hip-cli")
REFS = [("r1", 9000), ("empty", 2500), ("r2", 20001)]  # the rows behind r1's end are clipped or outside; no row is on `empty`


def table(out):
    return [[c.strip() for c in line.strip("|").split("|")] for line in out.splitlines() if line.startswith("|")]


def run(sql, **env):
    e = dict(os.environ)
    e.pop("EXON_HIP_GPU_PARSE", None)
    e.update(env)
    return subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, timeout=600, env=e)


def written_bam(tmp_path):
    recs = mixed(3000, seed=41)
    for r in recs:
        if r["ref"] == 1:
            r["ref"] = 2
    path = str(tmp_path / "w.bam")
    bsw.write_bam(path, recs, BGZIP, refs=REFS)
    return path


def want_rows(path, contigs, W):
    totals, bases = E.expect(by_slot(contigs), W, *host_rows(path, "bam", contigs))
    assert totals[0] > 0 and bases.sum() > 0
    return [[c, str(s), str(e), str(b)] for (c, s, e), b in zip(E.windows(contigs, W), bases.tolist())]


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_parse", [None, "0"])
def test_cli_window_depth_from_the_header_and_from_a_genome_file(tmp_path, gpu_parse):
    path = written_bam(tmp_path)
    env = {} if gpu_parse is None else {"EXON_HIP_GPU_PARSE": gpu_parse}
    r = run(f"SELECT * FROM window_depth('{path}', 1000)", **env)
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    assert t[0] == ["contig", "start", "end", "bases"]
    assert t[1:] == want_rows(path, REFS, 1000)
    assert t[9] == ["r1", "8001", "9000", t[9][3]] and t[10][:3] == ["empty", "1", "1000"] and t[-1][:3] == ["r2", "20001", "20001"]
    # the genome file decides the contigs, their order and their lengths; a name the file lacks has windows and no bases
    genome = tmp_path / "genome.txt"
    genome.write_text("# name\tlength\nr2\t12000\tignored\nchrNone\t700\r\n\nr1\t20000\n")
    contigs = [("r2", 12000), ("chrNone", 700), ("r1", 20000)]
    r = run(f"SELECT * FROM window_depth('{path}', 512, '{genome}')", **env)
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    assert t[1:] == want_rows(path, contigs, 512)
    assert sum(int(row[3]) for row in t[1:] if row[0] == "chrNone") == 0


def test_refusals(tmp_path):
    bam = tmp_path / "x.bam"
    bam.write_bytes(b"")
    r = run(f"SELECT * FROM window_depth('{bam}', 0)")
    assert r.returncode != 0 and "window width must be at least 1" in r.stderr
    r = run(f"SELECT * FROM window_depth('{bam}', 1.5)")
    assert r.returncode != 0 and "whole number" in r.stderr
    genome = tmp_path / "bad.txt"
    genome.write_text("r1\t9000\nr2\tlong\n")
    r = run(f"SELECT * FROM window_depth('{bam}', 100, '{genome}')")
    assert r.returncode != 0 and "line 2" in r.stderr and "expected <name> <length>" in r.stderr
    genome.write_text("r1\t0\n")
    r = run(f"SELECT * FROM window_depth('{bam}', 100, '{genome}')")
    assert r.returncode != 0 and "line 1" in r.stderr
    genome.write_text("# nothing\n")
    r = run(f"SELECT * FROM window_depth('{bam}', 100, '{genome}')")
    assert r.returncode != 0 and "no contigs" in r.stderr
    r = run(f"SELECT * FROM window_depth('{bam}', 100, '{tmp_path / 'missing.txt'}')")
    assert r.returncode != 0 and "no such file" in r.stderr
    bed = tmp_path / "t.bed"
    bed.write_text("chr1\t0\t10\n")
    r = run(f"SELECT * FROM window_depth('{bed}', 100)")
    assert r.returncode != 0 and "BED source" in r.stderr and "window_depth" in r.stderr
    gff = tmp_path / "t.gff"
    gff.write_text("##gff-version 3\n")
    r = run(f"SELECT * FROM window_depth('{gff}', 100)")
    assert r.returncode != 0 and "genome file" in r.stderr
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "window_depth('<bam|sam|cram file>', <W>)" in r.stdout + r.stderr and "'<genome file>')" in r.stdout + r.stderr


def test_the_header_of_a_written_bam_gives_the_contigs(tmp_path):
    path = written_bam(tmp_path)
    scan = exon_amd.Scan(path, "bam", gpu_parse=False)
    assert list(zip(scan.dictionary(2), scan.reference_lengths())) == REFS
    scan.close()
    assert np.array_equal(E.offsets(REFS, 1000), [0, 9, 12, 33])
