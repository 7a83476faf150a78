"""GPU: a names-form covered-bases plan (kind 12) fed by files.  Every consumed scan resolves the set's contig names in its own
dictionary.  The expected sums come from the HOST reader's batches of the same file (gpu_parse off), clipped against every region in
numpy; the device-decoded run and the host-decoded run must both give them."""
import os

import numpy as np
import pytest

import bam_sam_writer as bsw
import exon_amd
import flag_predicate_expect as FE
from test_flag_predicate import FX, mixed, write

pytestmark = pytest.mark.gpu
OPEN = 2**63 - 1  # EXON_HIP_REGION_OPEN_END
COLS = {"bam": (2, 3, 4), "sam": (2, 3, 4), "gff": (0, 3, 4)}
CONTIG = {"bam": "reference", "sam": "reference", "gff": "seqname"}


def through_set(ctx, paths, fmt, regions, gpu_parse, where_flags=None):
    """-> (rows of every file, totals, bases per region, decoded on the GPU? of every file) with ONE stream over all `paths`"""
    plan = ctx.plan_region_set_bases(regions, columns=COLS[fmt])
    st = plan.open()
    rows, on = [], []
    for p in paths:
        kw = {} if where_flags is None else {"where_flags": where_flags}
        scan = exon_amd.Scan(str(p), fmt, gpu_parse=gpu_parse, **kw)
        rows.append(st.consume(scan))
        on.append(scan.decoded_on_gpu()[0])
        scan.close()
    state, _ = st.finish()
    bases = plan.decode(state)
    at = plan.layout()
    assert state[at[1]:at[2]].sum() == state[0] == state[at[3]:at[4]].sum()
    st.close(); plan.close()
    return rows, state[:4].tolist(), bases.tolist(), on


def clipped(path, fmt, regions, where_flags=None):
    """-> (rows, totals, bases per region) from the host reader's batches, every row clipped against every region"""
    kw = {} if where_flags is None else {"where_flags": where_flags}
    scan = exon_amd.Scan(str(path), fmt, gpu_parse=False, **kw)
    cols, _ = FE.table(scan)
    scan.close()
    names, starts, ends = cols[CONTIG[fmt]], cols["start"], cols["end"]
    in_set = {r[0] for r in regions}
    totals, bases = [0, 0, 0, 0], [0] * len(regions)
    for c, s, e in zip(names, starts, ends):
        if c is None or s is None or e is None:
            totals[1] += 1
        elif c not in in_set:
            totals[2] += 1
        elif e < s:
            totals[3] += 1
        else:
            totals[0] += 1
            for i, (rc, rs, re) in enumerate(regions):
                if rc == c:
                    bases[i] += max(0, min(e, OPEN if re is None else re) - max(s, rs) + 1)
    return len(names), totals, bases


def check_file(ctx, path, fmt, regions, n_rows):
    g = through_set(ctx, [path], fmt, regions, True)
    h = through_set(ctx, [path], fmt, regions, False)
    assert g[3] == [True] and h[3] == [False], "silent host fallback"  # decoded_on_gpu == 1, and == 0 with the device parser off
    assert g[0] == h[0] == [n_rows] and g[1] == h[1] and g[2] == h[2]
    assert sum(g[1]) == n_rows
    want = clipped(path, fmt, regions)
    assert want[0] == n_rows and g[1] == want[1] and g[2] == want[2]
    return g


def test_bam_reference_fixture(ctx):
    path = os.path.join(FX, "bam", "test.bam")
    regions = [("chr1", 1, 12209145), ("chr1", 1, None), ("chr1", 12209146, None), ("chr1", 1, 12209145), ("not-in-the-file", 1, None),
               ("chr1", 1, 1)]
    g = check_file(ctx, path, "bam", regions, 61)
    b = g[2]
    assert b[0] == b[3] > 0 and b[1] == b[0] + b[2] and b[2] > 0 and b[4] == 0 and b[5] == 0  # the first and the third tile the second


def test_sam_reference_fixture(ctx):
    path = os.path.join(FX, "sam", "test.sam")
    refs = exon_amd.Scan(path, "sam").dictionary(2)
    regions = [(refs[0], 1, None), (refs[0], 1, 5), (refs[0], 40, 50), ("absent", 1, None)]
    g = check_file(ctx, path, "sam", regions, 1)
    assert g[2][0] > 0 and g[2][3] == 0


def test_gff_reference_fixture(ctx):
    path = os.path.join(FX, "gff", "test.gff.gz")
    cols, _ = FE.table(exon_amd.Scan(path, "gff", gpu_parse=False))
    n, lo, hi = len(cols["start"]), min(cols["start"]), max(cols["end"])
    regions = [("sq0", 1, None), ("sq1", lo, lo), ("sq1", hi, None), ("sq0", lo + 1, hi - 1), ("sq7", 1, None), ("sq1", 1, None), ("sq0", 1, None)]
    g = check_file(ctx, path, "gff", regions, n)
    span = sum(e - s + 1 for s, e in zip(cols["start"], cols["end"]))
    assert g[2][4] == 0 and g[2][0] + g[2][5] == span and g[2][0] == g[2][6] > 0  # the open regions hold every base of their contig
    assert g[1] == [n, 0, 0, 0]  # "sq7" was interned: no row is elsewhere, nothing is NULL


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_synthetic_records_and_the_flag_predicate(ctx, tmp_path, fmt):
    recs = mixed(5000, seed=21)
    path = write(tmp_path, "rb", recs, fmt)
    regions = [("r2", 3000, 9000), ("r1", 1, None), ("r2", 1, 99), ("r1", 7000, 7000), ("r3", 1, None), ("r2", 3000, 9000)]

    def from_records(kept):  # what the records' own dicts say: [pos, pos + reference-consuming cigar length - 1]
        out = []
        for name, a, b in regions:
            t = 0
            for i in kept:
                r = recs[i]
                if r["ref"] is None or r["pos"] < 1 or bsw.REFS[r["ref"]][0] != name:
                    continue
                end = r["pos"] + sum(n for n, op in r["cigar"] if op in bsw.REF_CONSUMING) - 1
                t += max(0, min(end, OPEN if b is None else b) - max(r["pos"], a) + 1)
            out.append(t)
        return out
    g = check_file(ctx, path, fmt, regions, len(recs))
    want = from_records(range(len(recs)))
    assert g[2] == want and want[0] > 0 and want[4] == 0 and want[0] == want[5]
    # under a pushed-down flag / mapping-quality predicate only the kept rows are summed
    where = (1284, 0, 30)
    kept = FE.keep(recs, *where)
    for gpu_parse in (True, False):
        rows, totals, bases, on = through_set(ctx, [path], fmt, regions, gpu_parse, where_flags=where)
        assert on == [gpu_parse] and rows == [len(kept)]
        # (the device path masks the rows the predicate drops, which kind 11 and kind 12 then see as NULL rows; the host reader never
        # emits them: `counted` and the sums agree, null_rows need not)
        w = clipped(path, fmt, regions, where_flags=where)
        assert (rows[0], totals[0], bases) == (w[0], w[1][0], w[2]) and totals[2:] == w[1][2:]
        assert bases == from_records(kept)
        assert 0 < bases[0] < want[0]


def test_two_files_with_different_sq_orders_in_one_stream(ctx, tmp_path):
    a, b = mixed(3000, seed=31), mixed(2000, seed=32)
    flipped = [bsw.REFS[1], bsw.REFS[0]]  # in the second file id 0 is "r2"
    pa, pb = str(tmp_path / "a.sam"), str(tmp_path / "b.sam")
    bsw.write_sam(pa, a)
    bsw.write_sam(pb, b, refs=flipped)
    regions = [("r2", 3000, 9000), ("r1", 1, 5000), ("r1", 1, None), ("r2", 1, None)]
    one = [clipped(p, "sam", regions) for p in (pa, pb)]
    want = [x + y for x, y in zip(one[0][2], one[1][2])]
    for gpu_parse in (True, False):
        rows, totals, bases, on = through_set(ctx, [pa, pb], "sam", regions, gpu_parse)
        assert on == [gpu_parse, gpu_parse] and rows == [3000, 2000] and sum(totals) == 5000
        assert bases == want
        assert totals == [x + y for x, y in zip(one[0][1], one[1][1])]
    assert one[1][2][0] > 0 and one[1][2][1] > 0
    # resolved by ids instead, the second file's rows would land on the other contig: the two files alone differ from each other
    assert through_set(ctx, [pb], "sam", regions, True)[2] == one[1][2] != one[0][2]
