"""GPU: a names-form region-set depth plan (kind 14) fed by files.  Every consumed scan resolves the set's contig names in its own
dictionary.  The expected depths come from the HOST reader's batches of the same file (gpu_parse off), piled up per base in numpy
(region_depth_expect.py); the device-decoded run and the host-decoded run must both give them, through decode and through the
reduce behind finish_arrow."""
import os

import numpy as np
import pytest

import bam_sam_writer as bsw
import exon_amd
import flag_predicate_expect as FE
import region_depth_expect as E
from test_flag_predicate import FX, mixed, write

pytestmark = pytest.mark.gpu
COLS = {"bam": (2, 3, 4), "sam": (2, 3, 4)}
THR = [1, 2, 5, 20]


def through_set(ctx, paths, fmt, regions, gpu_parse, where_flags=None, arrow=False):
    """-> (rows of every file, totals, bases[M], ge[M, k], decoded on the GPU? of every file) with ONE stream over all `paths`;
    arrow: the table finish_arrow makes on the device instead of the host decode (no totals then)"""
    plan = ctx.plan_region_set_depth(regions, THR, columns=COLS[fmt])
    st = plan.open()
    rows, on = [], []
    for p in paths:
        kw = {} if where_flags is None else {"where_flags": where_flags}
        scan = exon_amd.Scan(str(p), fmt, gpu_parse=gpu_parse, **kw)
        rows.append(st.consume(scan))
        on.append(scan.decoded_on_gpu()[0])
        scan.close()
    if arrow:
        t = st.finish_arrow()
        assert [f.name for f in t.type] == ["contig", "start", "end", "bases"] + ["ge_%d" % x for x in THR] and str(t.type[0].type) == "string"
        assert t.field("contig").to_pylist() == [r[0] for r in regions] and t.field("start").to_pylist() == [r[1] for r in regions]
        totals, bases = None, np.array(t.field("bases").to_pylist(), np.int64)
        ge = np.array([t.field("ge_%d" % x).to_pylist() for x in THR], np.int64).T
    else:
        state, _ = st.finish()
        totals = state[:4].tolist()
        bases, ge = plan.decode(state)
    st.close(); plan.close()
    return rows, totals, bases.tolist(), ge.tolist(), on


def piled(path, fmt, regions, where_flags=None):
    """-> (rows, totals, bases, ge) from the host reader's batches, piled up per base in numpy; `path` may be a list of files, whose
    rows are piled up together (by contig NAME)"""
    kw = {} if where_flags is None else {"where_flags": where_flags}
    names, starts, ends = [], [], []
    for p in path if isinstance(path, list) else [path]:
        scan = exon_amd.Scan(str(p), fmt, gpu_parse=False, **kw)
        cols, _ = FE.table(scan)
        scan.close()
        names += cols["reference"]
        starts += cols["start"]
        ends += cols["end"]
    ids = {}
    for c, _, _ in regions:
        ids.setdefault(c, len(ids))
    ref = np.array([-1 if c is None else ids.get(c, 99) for c in names], np.int32)
    start = np.array([0 if s is None else s for s in starts], np.int64)
    end = np.array([0 if e is None else e for e in ends], np.int64)
    valid = [np.array([x is not None for x in col]) for col in (names, starts, ends)]
    totals, _, bases, ge = E.expect([(ids[c], s, e) for c, s, e in regions], THR, ref, start, end, *valid)
    return len(names), totals.tolist(), bases.tolist(), ge.tolist()


def check_file(ctx, path, fmt, regions, n_rows):
    g = through_set(ctx, [path], fmt, regions, True)
    h = through_set(ctx, [path], fmt, regions, False)
    assert g[4] == [True] and h[4] == [False], "silent host fallback"  # decoded_on_gpu == 1, and == 0 with the device parser off
    assert g[0] == h[0] == [n_rows] and g[1:4] == h[1:4]
    assert sum(g[1]) == n_rows
    want = piled(path, fmt, regions)
    assert want[0] == n_rows and g[1] == want[1] and g[2] == want[2] and g[3] == want[3]
    a = through_set(ctx, [path], fmt, regions, True, arrow=True)  # the reduce on the device
    assert a[4] == [True] and a[2] == want[2] and a[3] == want[3]
    return g


def test_bam_reference_fixture(ctx):
    path = os.path.join(FX, "bam", "test.bam")
    cols, _ = FE.table(exon_amd.Scan(path, "bam", gpu_parse=False))
    starts = sorted(s for c, s in zip(cols["reference"], cols["start"]) if c == "chr1" and s is not None)
    s0, med = starts[0], starts[len(starts) // 2]
    regions = [("chr1", s0, s0 + 999), ("chr1", s0 + 500, s0 + 2000), ("chr1", max(1, s0 - 100), s0 + 10), ("not-in-the-file", 1, 100),
               ("chr1", med, med + 5000), ("chr1", s0, s0 + 999), ("chr1", s0, s0)]
    g = check_file(ctx, path, "bam", regions, 61)
    b, ge = g[2], g[3]
    assert b[0] == b[5] > 0 and b[3] == 0 and ge[3] == [0] * len(THR) and b[6] >= ge[6][0] == 1


def test_sam_reference_fixture(ctx):
    path = os.path.join(FX, "sam", "test.sam")
    cols, _ = FE.table(exon_amd.Scan(path, "sam", gpu_parse=False))
    ref, s, e = cols["reference"][0], cols["start"][0], cols["end"][0]
    regions = [(ref, s, e), (ref, max(1, s - 5), s + 2), (ref, e, e + 40), ("absent", 1, 1000), (ref, s + 1, e - 1)]
    g = check_file(ctx, path, "sam", regions, 1)
    assert g[2][0] == e - s + 1 == g[3][0][0] and g[2][3] == 0 and g[2][2] == 1 and g[3][0][1] == 0


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_synthetic_records_and_the_flag_predicate(ctx, tmp_path, fmt):
    recs = mixed(5000, seed=21)
    path = write(tmp_path, "rd", recs, fmt)
    regions = [("r2", 3000, 9000), ("r1", 1, 4000), ("r2", 1, 99), ("r1", 7000, 7000), ("r3", 1, 500), ("r2", 3000, 9000), ("r2", 9001, 9500)]
    g = check_file(ctx, path, fmt, regions, len(recs))
    assert g[2][0] == g[2][5] > 0 and g[2][4] == 0 and g[3][0][0] > g[3][0][3] >= 0
    # under a pushed-down flag / mapping-quality predicate only the kept rows are piled up
    where = (1284, 0, 30)
    kept = FE.keep(recs, *where)
    for gpu_parse in (True, False):
        rows, totals, bases, ge, on = through_set(ctx, [path], fmt, regions, gpu_parse, where_flags=where)
        assert on == [gpu_parse] and rows == [len(kept)]
        # (the device path masks the rows the predicate drops, which the plan then sees as NULL rows; the host reader never emits
        # them: `counted`, the sums and the threshold counts agree, null_rows need not)
        w = piled(path, fmt, regions, where_flags=where)
        assert (rows[0], totals[0], bases, ge) == (w[0], w[1][0], w[2], w[3]) and totals[2:] == w[1][2:]
        assert 0 < bases[0] < g[2][0]


def test_two_files_with_different_sq_orders_in_one_stream(ctx, tmp_path):
    a, b = mixed(3000, seed=31), mixed(2000, seed=32)
    flipped = [bsw.REFS[1], bsw.REFS[0]]  # in the second file id 0 is "r2"
    pa, pb = str(tmp_path / "a.sam"), str(tmp_path / "b.sam")
    bsw.write_sam(pa, a)
    bsw.write_sam(pb, b, refs=flipped)
    regions = [("r2", 3000, 9000), ("r1", 1, 5000), ("r1", 4000, 6000), ("r2", 1, 2000)]
    one = [piled(p, "sam", regions) for p in (pa, pb)]
    want = piled([pa, pb], "sam", regions)  # the threshold counts do not add over files: both files' rows are piled up together
    assert want[2] == [x + y for x, y in zip(one[0][2], one[1][2])] and want[3] != (np.array(one[0][3]) + np.array(one[1][3])).tolist()
    for gpu_parse in (True, False):
        rows, totals, bases, ge, on = through_set(ctx, [pa, pb], "sam", regions, gpu_parse)
        assert on == [gpu_parse, gpu_parse] and rows == [3000, 2000] and sum(totals) == 5000
        assert bases == want[2] and ge == want[3]
        assert totals == [x + y for x, y in zip(one[0][1], one[1][1])]
    assert one[1][2][0] > 0 and one[1][2][1] > 0
    # resolved by ids instead, the second file's rows would land on the other contig: the two files alone differ from each other
    assert through_set(ctx, [pb], "sam", regions, True)[2] == one[1][2] != one[0][2]
