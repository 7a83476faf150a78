"""exon-hip-cli: the last optional argument 'cover=span' | 'cover=aligned' | 'cover=aligned+del' of covered_bases, depth_thresholds and
window_depth puts the BAM / SAM scan into blocks mode (exon_hip_scan_set_cover_ops).  Each function with each value over a written
SAM and BAM of spliced, deleted and clipped reads, decoded on the device and, with EXON_HIP_GPU_PARSE=0, by the host reader, against
the records' aligned blocks (cigar_blocks_expect.py) through each plan's own expectation.  overlap_counts refuses the argument; the
refusals need no device."""
import os
import subprocess

import numpy as np
import pytest

import bam_sam_writer as bsw
import cigar_blocks_expect as E
import region_bases_expect as E12
import region_depth_expect as E14
import window_bases_expect as E13

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "exon_amd", "bin", "exon-hip-cli")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
REFS = [("r1", 5000), ("r2", 3000)]
REGIONS = [("r1", 100, 900), ("r2", 1, 3000), ("r1", 850, 2400), ("absent", 1, 10), ("r1", 100, 900)]
SHAPES = ["30M", "10M200N15M", "5S20M3D20M2I10M", "8=1X8=", "12M300N12M40N6M", "25N", "", "7M2D"]
COVER = {"span": None, "aligned": E.ALIGNED, "aligned+del": E.ALIGNED_DEL}
W, THR = 500, [1, 2, 4]


def records(n=400):
    rng = np.random.default_rng(3)
    shape = rng.integers(0, len(SHAPES), n)
    pos = rng.integers(1, 2400, n)
    return [dict(name="n%d" % i, flag=0, ref=None if i % 23 == 5 else i % 2, pos=0 if i % 29 == 7 else int(pos[i]), mapq=60, cigar=E.cigar(SHAPES[shape[i]]), seq="ACGT",
                 qual=[30] * 4) for i in range(n)]


def rows_of(recs, mask, ids):
    """the block rows (mask None: the spans) as ids-form columns + validity"""
    rv = np.array([r["ref"] is not None for r in recs], bool)
    sv = np.array([r["pos"] >= 1 for r in recs], bool)
    ref = np.array([ids.get(REFS[r["ref"]][0], 99) if r["ref"] is not None else -1 for r in recs], np.int32)
    start = np.array([r["pos"] for r in recs], np.int64)
    cig = [r["cigar"] for r in recs]
    if mask is None:
        end = start + np.array([sum(ln for ln, c in ops if c in E.REF_CODES) for ops in cig], np.int64) - 1
        return ref, start, end, rv, sv, sv
    r, s, e, v = E.expand(ref, start, cig, mask, rv, sv)
    return r, s, e, v, v, v


def table(out):
    return [[c.strip() for c in line.strip("|").split("|")] for line in out.splitlines() if line.startswith("|")]


def run(sql, **env):
    e = dict(os.environ)
    e.pop("EXON_HIP_GPU_PARSE", None)
    e.update(env)
    return subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, timeout=600, env=e)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cover")
    recs = records()
    sam, bam = str(tmp / "reads.sam"), str(tmp / "reads.bam")
    bsw.write_sam(sam, recs, refs=REFS)
    bsw.write_bam(bam, recs, BGZIP, refs=REFS)
    bed = tmp / "targets.bed"
    bed.write_text("".join("%s\t%d\t%d\n" % (c, a - 1, b) for c, a, b in REGIONS))
    return recs, {"sam": sam, "bam": bam}, str(bed)


@pytest.mark.gpu
@pytest.mark.parametrize("cover", ["span", "aligned", "aligned+del", None])
@pytest.mark.parametrize("fmt,gpu_parse", [("sam", None), ("bam", None), ("sam", "0")])
def test_the_three_table_functions_with_each_cover_value(inputs, fmt, gpu_parse, cover):
    recs, paths, bed = inputs
    env = {} if gpu_parse is None else {"EXON_HIP_GPU_PARSE": gpu_parse}
    arg = "" if cover is None else f", 'cover={cover}'"  # (no argument at all: the span)
    mask = COVER[cover or "span"]
    ids = {}
    for c, _, _ in REGIONS:
        ids.setdefault(c, len(ids))
    regions = [(ids[c], a, b) for c, a, b in REGIONS]

    r = run(f"SELECT * FROM covered_bases('{paths[fmt]}', '{bed}'{arg})", **env)
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    _, bases = E12.expect(regions, *rows_of(recs, mask, ids))
    assert t[0] == ["contig", "start", "end", "bases"] and [row[:3] for row in t[1:]] == [[c, str(a), str(b)] for c, a, b in REGIONS]
    assert [int(row[3]) for row in t[1:]] == bases.tolist() and bases[0] == bases[4] > 0 and bases[3] == 0

    r = run(f"SELECT * FROM depth_thresholds('{paths[fmt]}', '{bed}', '1,2,4'{arg})", **env)
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    _, _, b14, ge = E14.expect(regions, THR, *rows_of(recs, mask, ids))
    assert [[int(x) for x in row[3:]] for row in t[1:]] == [[int(b)] + g.tolist() for b, g in zip(b14, ge)] and b14.tolist() == bases.tolist()

    r = run(f"SELECT * FROM window_depth('{paths[fmt]}', {W}{arg})", **env)
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    wid = {n: i for i, (n, _) in enumerate(REFS)}
    _, wb = E13.expect([(wid[n], ln) for n, ln in REFS], W, *rows_of(recs, mask, wid))
    assert [row[0] for row in t[1:]] == ["r1"] * 10 + ["r2"] * 6 and [int(row[3]) for row in t[1:]] == np.asarray(wb).tolist()
    if cover in ("aligned", "aligned+del"):  # the introns and (without +del) the deletions are gone
        span = E13.expect([(wid[n], ln) for n, ln in REFS], W, *rows_of(recs, None, wid))[1]
        assert 0 < np.asarray(wb).sum() < np.asarray(span).sum()


def test_overlap_counts_and_unknown_values_refuse(inputs):
    recs, paths, bed = inputs
    r = run(f"SELECT * FROM overlap_counts('{paths['sam']}', '{bed}', 'cover=aligned')")
    assert r.returncode != 0 and "overlap_counts" in r.stderr and "once per aligned block" in r.stderr
    r = run(f"SELECT * FROM overlap_counts('{paths['sam']}', '{bed}', 'gzip', 'cover=span')")
    assert r.returncode != 0 and "once per aligned block" in r.stderr
    for fn, args in (("covered_bases", f"'{bed}'"), ("depth_thresholds", f"'{bed}', '1'"), ("window_depth", "100")):
        r = run(f"SELECT * FROM {fn}('{paths['sam']}', {args}, 'cover=exons')")
        assert r.returncode != 0 and fn in r.stderr and "span, aligned or aligned+del" in r.stderr
    r = run(f"SELECT * FROM covered_bases('{paths['sam']}', '{bed}', 'cover=aligned', 'gzip')")  # cover= is the LAST argument
    assert r.returncode != 0
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "'cover=aligned'" in r.stdout + r.stderr and "'cover=aligned+del'" in r.stdout + r.stderr


@pytest.mark.gpu
def test_a_source_without_a_cigar_refuses(inputs):
    recs, paths, bed = inputs
    gff = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "gff", "test.gff.gz")
    r = run(f"SELECT * FROM covered_bases('{gff}', '{bed}', 'cover=aligned')")  # the scan's own refusal
    assert r.returncode != 0 and "no CIGAR" in r.stderr
    r = run(f"SELECT * FROM covered_bases('{gff}', '{bed}', 'cover=span')")  # the default, spelled out, is no mode at all
    assert r.returncode == 0, r.stderr
