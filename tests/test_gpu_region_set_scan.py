"""GPU: a names-form region-set plan (kind 11) fed by files.  Every consumed scan resolves the set's contig names in its own
dictionary; the counts must equal one K6 stream per region (set_region_contig), the host-decoded run of the same file, and what the
records themselves say."""
import gzip
import os

import numpy as np
import pytest

import bam_sam_writer as bsw
import exon_amd
import flag_predicate_expect as FE
from oracle_expect import k6_expected
from test_flag_predicate import FX, mixed, write

pytestmark = pytest.mark.gpu
OPEN = 2**63 - 1  # EXON_HIP_REGION_OPEN_END
COLS = {"bam": (2, 3, 4), "sam": (2, 3, 4), "gff": (0, 3, 4)}


def through_set(ctx, paths, fmt, regions, gpu_parse, where_flags=None):
    """-> (rows of every file, totals, counts per region, decoded on the GPU? of every file) with ONE stream over all `paths`"""
    plan = ctx.plan_region_set_overlap(regions, columns=COLS[fmt])
    st = plan.open()
    rows, on = [], []
    for p in paths:
        kw = {} if where_flags is None else {"where_flags": where_flags}
        scan = exon_amd.Scan(str(p), fmt, gpu_parse=gpu_parse, **kw)
        rows.append(st.consume(scan))
        on.append(scan.decoded_on_gpu()[0])
        scan.close()
    state, _ = st.finish()
    counts = plan.decode(state)
    st.close(); plan.close()
    return rows, state[:4].tolist(), counts.tolist(), on


def through_k6(ctx, path, fmt, region, gpu_parse, where_flags=None):
    name, a, b = region
    kw = {} if where_flags is None else {"where_flags": where_flags}
    scan = exon_amd.Scan(str(path), fmt, gpu_parse=gpu_parse, **kw)
    plan = ctx.plan_overlap_count(0, a, b, columns=COLS[fmt])
    st = plan.open()
    st.set_region_contig(name)
    st.consume(scan)
    counts, _ = st.finish()
    st.close(); plan.close(); scan.close()
    return int(counts[0])


def check_file(ctx, path, fmt, regions, n_rows):
    g = through_set(ctx, [path], fmt, regions, True)
    h = through_set(ctx, [path], fmt, regions, False)
    assert g[3] == [True] and h[3] == [False], "silent host fallback"  # decoded_on_gpu == 1, and == 0 with the device parser off
    assert g[0] == h[0] == [n_rows] and g[1] == h[1] and g[2] == h[2]
    assert sum(g[1]) == n_rows
    assert g[2] == [through_k6(ctx, path, fmt, r, True) for r in regions]
    return g


def test_bam_reference_fixture(ctx):
    """bam_region_filter('chr1:1-12209145', ...) on the reference's fixture is 7 (slt/bam-indexed-select-tests.slt:16-19)"""
    path = os.path.join(FX, "bam", "test.bam")
    regions = [("chr1", 1, 12209145), ("chr1", 1, None), ("chr1", 12209146, None), ("chr1", 1, 12209145), ("not-in-the-file", 1, None),
               ("chr1", 1, 1)]
    g = check_file(ctx, path, "bam", regions, 61)
    # (seven reads start in front of 12209146 and all of them end behind it; the oracle counts each region on its own)
    assert g[2] == [7, 61, 61, 7, 0, 0]
    assert g[2] == [k6_expected(path, "bam", name, a, b)[1] if name == "chr1" else 0 for name, a, b in regions]


def test_sam_reference_fixture(ctx):
    path = os.path.join(FX, "sam", "test.sam")
    refs = exon_amd.Scan(path, "sam").dictionary(2)
    regions = [(refs[0], 1, None), (refs[0], 1, 5), (refs[0], 40, 50), ("absent", 1, None)]
    g = check_file(ctx, path, "sam", regions, 1)
    assert g[2][0] == 1 and g[2][3] == 0


def test_gff_reference_fixture(ctx):
    path = os.path.join(FX, "gff", "test.gff.gz")
    rows = [ln.split("\t") for ln in gzip.open(path, "rt") if ln.strip() and not ln.startswith("#")]
    name = np.array([r[0] for r in rows])
    start, end = np.array([int(r[3]) for r in rows]), np.array([int(r[4]) for r in rows])
    lo, hi = int(start.min()), int(end.max())
    regions = [("sq0", 1, None), ("sq1", lo, lo), ("sq1", hi, None), ("sq0", lo + 1, hi - 1), ("sq7", 1, None), ("sq1", 1, None), ("sq0", 1, None)]
    g = check_file(ctx, path, "gff", regions, len(rows))
    want = [int(((name == c) & (start <= (2**63 - 1 if b is None else b)) & (end >= a)).sum()) for c, a, b in regions]
    assert g[2] == want and want[4] == 0 and want[0] + want[5] == len(rows)
    assert g[1] == [len(rows), 0, 0, 0]  # "sq7" was interned: no row is elsewhere, nothing is NULL


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_synthetic_records_and_the_flag_predicate(ctx, tmp_path, fmt):
    recs = mixed(5000, seed=21)
    path = write(tmp_path, "rs", recs, fmt)
    regions = [("r2", 3000, 9000), ("r1", 1, OPEN), ("r2", 1, 99), ("r1", 7000, 7000), ("r3", 1, OPEN), ("r2", 3000, 9000)]
    want = [len(FE.keep(recs, 0, 0, region=r)) for r in regions]
    g = check_file(ctx, path, fmt, regions, len(recs))
    assert g[2] == want and want[0] > 0 and want[4] == 0
    # under a pushed-down flag / mapping-quality predicate only the kept rows are counted, by K6's route
    where = (1284, 0, 30)
    kept = FE.keep(recs, *where)
    for gpu_parse in (True, False):
        rows, totals, counts, on = through_set(ctx, [path], fmt, regions, gpu_parse, where_flags=where)
        assert on == [gpu_parse] and rows == [len(kept)]
        assert counts == [len(FE.keep(recs, *where, region=r)) for r in regions]
        assert counts == [through_k6(ctx, path, fmt, r, gpu_parse, where_flags=where) for r in regions]
        assert 0 < counts[0] < want[0]


def test_two_files_with_different_sq_orders_in_one_stream(ctx, tmp_path):
    a, b = mixed(3000, seed=31), mixed(2000, seed=32)
    flipped = [bsw.REFS[1], bsw.REFS[0]]  # in the second file id 0 is "r2"
    pa, pb = str(tmp_path / "a.sam"), str(tmp_path / "b.sam")
    bsw.write_sam(pa, a)
    bsw.write_sam(pb, b, refs=flipped)
    regions = [("r2", 3000, 9000), ("r1", 1, 5000), ("r1", 1, OPEN), ("r2", 1, OPEN)]
    want = [len(FE.keep(a, 0, 0, region=r)) + sum(1 for x in b if FE.hits(x, r, refs=flipped)) for r in regions]
    for gpu_parse in (True, False):
        rows, totals, counts, on = through_set(ctx, [pa, pb], "sam", regions, gpu_parse)
        assert on == [gpu_parse, gpu_parse] and rows == [3000, 2000] and sum(totals) == 5000
        assert counts == want
    one = [through_set(ctx, [p], "sam", regions, True)[2] for p in (pa, pb)]
    assert [x + y for x, y in zip(*one)] == want and one[1][0] > 0 and one[1][1] > 0
