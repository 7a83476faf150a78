"""GPU: the region-set overlap plan (kind 11) against plain numpy (region_set_expect.py), on all four totals and on every region:
the bare operator, plan launches in both modes, chunks, folds and streams, in both tiers and both launch shapes."""
import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L

import region_set_expect as E
import region_set_rows
from region_set_rows import full, launch, random_regions, random_rows

pytestmark = pytest.mark.gpu

LDS_MAX = exon_amd.REGION_SET_LDS_MAX
TILE_S, TILE_B = L.REGION_SET_TILE_SMALL, L.REGION_SET_TILE_BIG
ESTATE = -5


class Cols(region_set_rows.Cols):
    E = E


def check(plan, state, want):
    totals, counts = want
    assert state[:4].tolist() == totals.tolist()
    assert plan.decode(state).tolist() == counts.tolist()
    at = plan.layout()
    assert state[at[1]:at[2]].sum() == totals[0] == state[at[2]:at[3]].sum()  # every counted row adds once to A and once to B


SEVEN = [(0, 100, 400), (0, 100, 400), (2, 1, None), (2, 500, 500), (1, 300, 1900), (4, 1500, 1600), (0, 350, 360)]


def test_seven_regions_equal_seven_k6_plans(ctx):
    rng = np.random.default_rng(1)
    cols = Cols(ctx, *random_rows(rng, 5000))
    plan = ctx.plan_region_set_overlap(SEVEN, columns=(0, 1, 2))
    got = plan.decode(launch(ctx, plan, cols).to_host())
    for i, (c, s, e) in enumerate(SEVEN):
        k6 = ctx.plan_overlap_count(c, s, e, columns=(0, 1, 2))
        d = ctx.zeros(np.int64, 1)
        k6.launch(cols.columns(), cols.n, d, overwrite=True)
        ctx.sync()
        # K6 also counts inverted rows for a region that strictly contains the gap; K11 does not (the header's DECISION): take them out
        ref, start, end = cols.host
        ok = cols.valid[0] & cols.valid[1] & cols.valid[2] & (ref == c) & (end < start)
        gap = int((ok & (start <= (E.OPEN_END if e is None else e)) & (end >= s)).sum())
        assert got[i] == d.to_host()[0] - gap, i
        k6.close()
    check(plan, launch(ctx, plan, cols).to_host(), cols.expect(SEVEN))
    # M = 1 on rows that are never inverted: exactly K6
    ref, start, end, rv, sv, ev = random_rows(rng, 3000, inverted=0)
    cols = Cols(ctx, ref, start, end, rv, sv, ev)
    one = ctx.plan_region_set_overlap([(3, 700, 900)], columns=(0, 1, 2))
    k6 = ctx.plan_overlap_count(3, 700, 900, columns=(0, 1, 2))
    d = ctx.zeros(np.int64, 1)
    k6.launch(cols.columns(), cols.n, d, overwrite=True)
    ctx.sync()
    assert one.decode(launch(ctx, one, cols).to_host()).tolist() == [d.to_host()[0]] == cols.expect([(3, 700, 900)])[1].tolist()


@pytest.mark.parametrize("row,want", [((0, 20, 25), [1, 0, 1]), ((0, 21, 25), [0, 0, 1]), ((0, 3, 10), [1, 0, 0]), ((0, 3, 9), [0, 0, 0]),
                                      ((0, 5000, 5000), [0, 0, 1]), ((0, 15, 15), [1, 1, 0]), ((0, 2**62, 2**63 - 1), [0, 0, 1])])
def test_boundaries_one_row(ctx, row, want):
    """s == re, s == re + 1, e == rs, e == rs - 1, the open end, start == end"""
    regions = [(0, 10, 20), (0, 15, 15), (0, 21, None)]
    plan = ctx.plan_region_set_overlap(regions, columns=(0, 1, 2))
    cols = Cols(ctx, [row[0]], [row[1]], [row[2]])
    st = launch(ctx, plan, cols).to_host()
    assert plan.decode(st).tolist() == want
    check(plan, st, cols.expect(regions))


def test_region_shapes_and_row_classes(ctx):
    rng = np.random.default_rng(2)
    regions = [(1, 50, 90)] * 3                                          # identical x 3
    regions += [(1, 10, 1000), (1, 20, 900), (1, 30, 800), (1, 40, 41)]  # nested
    regions += [(2, 10, 500), (2, 100, 500), (2, 499, 500)]              # equal ends
    regions += [(2, 700, 710), (2, 700, 800), (2, 700, None)]            # equal starts
    regions += [(40, 1, 100), (40, 1, None)]                             # a contig no row has
    ref, start, end, rv, sv, ev = random_rows(rng, 4000, n_refs=4, span=1100)
    ref[:50] = -1
    ref[50:100] = 41           # beyond the map (its last id is 40)
    ref[100:150] = 2**31 - 1
    ref[150:200] = -2**31
    ref[200:260] = 3           # inside the map, not in the set
    cols = Cols(ctx, ref, start, end, rv, sv, ev)
    plan = ctx.plan_region_set_overlap(regions, columns=(0, 1, 2))
    st = launch(ctx, plan, cols).to_host()
    want = cols.expect(regions)
    check(plan, st, want)
    assert want[0].min() > 0 and want[0].sum() == cols.n  # all four classes occur
    assert np.array_equal(st, E.expect_state(full(regions), *cols.host, *cols.valid))  # word by word
    got = plan.decode(st)
    assert got[0] == got[1] == got[2] and got[-1] == got[-2] == 0


@pytest.mark.parametrize("which", [0, 1, 2])
def test_each_column_null_alone(ctx, which):
    rng = np.random.default_rng(3 + which)
    ref, start, end, _, _, _ = random_rows(rng, 3000, inverted=0)
    v = [None, None, None]
    v[which] = rng.random(3000) < 0.5
    cols = Cols(ctx, ref, start, end, *v)
    plan = ctx.plan_region_set_overlap(SEVEN, columns=(0, 1, 2))
    st = launch(ctx, plan, cols).to_host()
    check(plan, st, cols.expect(SEVEN))
    assert st[1] == (~v[which]).sum() > 0


def test_inverted_rows_count_for_no_region(ctx):
    regions = [(0, 1, 1000), (0, 40, 60)]
    cols = Cols(ctx, [0, 0, 0, 0], [70, 50, 61, 30], [30, 50, 39, 70])  # [70, 30] and [61, 39] span region 1's interval backwards
    plan = ctx.plan_region_set_overlap(regions, columns=(0, 1, 2))
    st = launch(ctx, plan, cols).to_host()
    assert st[:4].tolist() == [2, 0, 0, 2] and plan.decode(st).tolist() == [2, 2]
    check(plan, st, cols.expect(regions))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE_S - 1, TILE_S, TILE_S + 1, 3 * TILE_S + 517])
def test_row_counts_small_shape(ctx, n):
    rng = np.random.default_rng(100 + n)
    cols = Cols(ctx, *random_rows(rng, n))
    plan = ctx.plan_region_set_overlap(SEVEN, columns=(0, 1, 2))
    d = ctx.to_device(np.full(plan.n_i64, -7, np.int64))  # overwrite: garbage in front, n = 0 included
    check(plan, launch(ctx, plan, cols, d_state=d).to_host(), cols.expect(SEVEN))


@pytest.mark.parametrize("extra", [TILE_B - 1, TILE_B + 1])
@pytest.mark.parametrize("tier", ["lds", "global"])
def test_row_counts_big_shape(ctx, extra, tier):
    """the 1024-thread shape takes over once every CU gets a tile: that many rows and one tile -/+ 1 more"""
    n = ctx.info()["compute_units"] * TILE_B + extra
    rng = np.random.default_rng(extra)
    cols = Cols(ctx, *random_rows(rng, n, null=0.01))
    regions = SEVEN if tier == "lds" else SEVEN + [(5, 1 + i, 1 + i) for i in range(LDS_MAX)]
    plan = ctx.plan_region_set_overlap(regions, columns=(0, 1, 2))
    check(plan, launch(ctx, plan, cols).to_host(), cols.expect(regions, fast=True))


@pytest.mark.parametrize("shift", [(1, 1, 1), (3, 1, 1), (2, 1, 0), (1, 0, 0), (0, 1, 0)])
def test_unaligned_column_bases(ctx, shift):
    """(1, 1, 1) and (3, 1, 1) line up behind a head of 3 / 1 rows; the others never do and are read row by row"""
    rng = np.random.default_rng(sum(shift))
    cols = Cols(ctx, *random_rows(rng, 2 * TILE_S + 77), shift=shift)
    plan = ctx.plan_region_set_overlap(SEVEN, columns=(0, 1, 2))
    check(plan, launch(ctx, plan, cols).to_host(), cols.expect(SEVEN))
    d = ctx.zeros(np.int64, plan.n_i64)
    c = cols.columns()
    ctx.region_set_overlap(c[0][0], c[0][1], c[1][0], c[1][1], c[2][0], c[2][1], cols.n, plan, d)  # the bare operator takes them too
    ctx.sync()
    check(plan, d.to_host(), cols.expect(SEVEN))


def edge_sets(total, many):
    """region sets with M + C == total: one contig, or every region on a contig of its own (then one region more on contig 0)"""
    rng = np.random.default_rng(total)
    if not many:
        return random_regions(rng, total - 1, [0], span=50_000, width=400)
    c = total // 2
    regions = [(i, int(rng.integers(1, 1000)), int(rng.integers(1000, 2000))) for i in range(c)]
    return regions + [(0, 500, 1500)] * (total - 2 * c)


@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("total", [LDS_MAX, LDS_MAX + 1])
def test_tier_edge(ctx, total, many):
    regions = edge_sets(total, many)
    plan = ctx.plan_region_set_overlap(regions, columns=(0, 1, 2))
    assert plan.n_i64 == 4 + 2 * total
    rng = np.random.default_rng(7)
    n = 30_000
    ref = rng.integers(0, total // 2 if many else 2, n).astype(np.int32)
    start = rng.integers(1, 2200 if many else 51_000, n)
    end = start + rng.integers(0, 300, n)
    cols = Cols(ctx, ref, start, end, rng.random(n) < 0.97)
    st = launch(ctx, plan, cols).to_host()
    check(plan, st, cols.expect(regions, fast=True))
    sub = slice(0, 400)  # and by brute force on a few rows, in the same plan
    few = Cols(ctx, ref[sub], start[sub], end[sub])
    check(plan, launch(ctx, plan, few).to_host(), few.expect(regions))


def test_large_tier_100000_regions(ctx):
    rng = np.random.default_rng(11)
    regions = random_regions(rng, 100_000, [0, 5, 9], span=3_000_000, width=5000)
    n = 200_000
    ref = rng.choice([0, 5, 9, 2], n).astype(np.int32)
    start = rng.integers(1, 3_000_000, n)
    end = start + rng.integers(0, 400, n)
    cols = Cols(ctx, ref, start, end, None, rng.random(n) < 0.99, None)
    plan = ctx.plan_region_set_overlap(regions, columns=(0, 1, 2))
    check(plan, launch(ctx, plan, cols).to_host(), cols.expect(regions, fast=True))


@pytest.mark.parametrize("tier", ["lds", "global"])
def test_hot_bin_sorted_rows(ctx, tier):
    """a coordinate-sorted file: a million rows inside ONE region of the set, ascending -- whole waves on one bin"""
    m = 4096 if tier == "lds" else LDS_MAX + 1
    regions = [(0, 1 + 1000 * i, 1000 * (i + 1)) for i in range(m)]
    n = 1_000_000
    rng = np.random.default_rng(5)
    start = np.sort(rng.integers(2_000_100, 2_000_800, n))  # region 2000 = [2000001, 2001000]
    end = start + rng.integers(0, 100, n)
    cols = Cols(ctx, np.zeros(n, np.int32), start, end)
    plan = ctx.plan_region_set_overlap(regions, columns=(0, 1, 2))
    st = launch(ctx, plan, cols).to_host()
    got = plan.decode(st)
    assert got[2000] == n and got.sum() == n
    check(plan, st, cols.expect(regions, fast=True))


def test_launch_modes_and_chunks(ctx):
    rng = np.random.default_rng(13)
    cols = Cols(ctx, *random_rows(rng, 3 * 4096))
    plan = ctx.plan_region_set_overlap(SEVEN, columns=(0, 1, 2))
    whole = launch(ctx, plan, cols).to_host()
    check(plan, whole, cols.expect(SEVEN))
    d = ctx.zeros(np.int64, plan.n_i64)
    for k in range(3):  # accumulate over three launches = one launch of the concatenation
        launch(ctx, plan, cols, overwrite=False, d_state=d, lo=4096 * k, hi=4096 * (k + 1))
    assert np.array_equal(d.to_host(), whole)
    d = ctx.to_device(rng.integers(-2**40, 2**40, plan.n_i64))  # overwrite on a state full of garbage
    assert np.array_equal(launch(ctx, plan, cols, d_state=d).to_host(), whole)
    d = ctx.to_device(rng.integers(-2**40, 2**40, plan.n_i64))
    plan.launch_chunks([(cols.columns(0), 4096), (cols.columns(4096), 0), (cols.columns(4096), 8192)], d, overwrite=True)
    ctx.sync()
    assert np.array_equal(d.to_host(), whole)
    plan.launch_chunks([], d, overwrite=True)  # an overwrite of nothing is the empty state
    ctx.sync()
    assert not d.to_host().any()


def test_fold_states_of_two_ranks(ctx):
    rng = np.random.default_rng(17)
    cols = Cols(ctx, *random_rows(rng, 6000))
    plan = ctx.plan_region_set_overlap(SEVEN, columns=(0, 1, 2))
    a = launch(ctx, plan, cols, lo=0, hi=2400).to_host()
    b = launch(ctx, plan, cols, lo=2400).to_host()
    out = ctx.zeros(np.int64, plan.n_i64)
    plan.fold_states(ctx.to_device(np.concatenate([a, b])), 2, out)
    ctx.sync()
    whole = launch(ctx, plan, cols).to_host()
    assert np.array_equal(out.to_host(), whole)
    assert np.array_equal(plan.decode(a) + plan.decode(b), plan.decode(whole))


def test_streams(ctx):
    import pyarrow as pa
    rng = np.random.default_rng(19)
    plan = ctx.plan_region_set_overlap(SEVEN, columns=(1, 2, 3))
    st = plan.open()
    ref, start, end, rv, sv, ev = random_rows(rng, 9000)

    def batch(lo, hi, pad):
        # `pad` rows in front, sliced away: the validity bitmaps start at a bit offset that is not zero
        sl = slice(max(lo - pad, 0), hi)
        arrs = [pa.array(ref[sl], mask=~rv[sl]), pa.array(start[sl], mask=~sv[sl]), pa.array(end[sl], mask=~ev[sl])]
        b = pa.RecordBatch.from_arrays([pa.array(np.zeros(hi - sl.start, np.int8))] + arrs, names=["x", "ref", "start", "end"])
        return b.slice(lo - sl.start)
    for lo, hi, pad in [(0, 100, 0), (100, 4099, 3), (4099, 4100, 5), (4100, 9000, 13)]:
        st.push(batch(lo, hi, pad))
    want = E.expect(full(SEVEN), ref, start, end, rv, sv, ev)
    counts, sums = st.finish()
    assert sums.size == 0
    check(plan, counts, want)
    # a new query on the same stream: reset, device batches, the Arrow result
    st.reset()
    cols = Cols(ctx, ref[:5000], start[:5000], end[:5000], rv[:5000], sv[:5000], ev[:5000])
    dummy = ctx.zeros(np.int8, 5000)
    st.push_device([(dummy, None, None)] + [(b, v, None) for b, v in zip(cols.bufs, cols.vbufs)], 5000)
    table = st.finish_arrow()
    want = cols.expect(SEVEN)
    assert [f.name for f in table.type] == ["contig", "start", "end", "count"]
    assert [str(f.type) for f in table.type] == ["int32", "int64", "int64", "int64"]
    assert table.field("contig").to_pylist() == [r[0] for r in SEVEN]
    assert table.field("start").to_pylist() == [r[1] for r in SEVEN]
    assert table.field("end").to_pylist() == [r[2] for r in full(SEVEN)]
    assert table.field("count").to_pylist() == want[1].tolist()
    # reset with nothing behind it: the empty state
    st.reset()
    assert not st.finish()[0].any()
    st.close()


def test_names_form_refuses_rows_without_a_file(ctx):
    import pyarrow as pa
    plan = ctx.plan_region_set_overlap([("chr1", 1, 100), ("chr2", 5, None)], columns=(0, 1, 2))
    assert plan.by_name and plan.layout() == (0, 4, 8, 12)
    st = plan.open()
    b = pa.RecordBatch.from_arrays([pa.array(np.zeros(4, np.int32)), pa.array(np.ones(4, np.int64)), pa.array(np.ones(4, np.int64))], names=["r", "s", "e"])
    with pytest.raises(exon_amd.ExonHipError) as e:
        st.push(b)
    assert e.value.code == ESTATE and "NAMES" in str(e.value)
    cols = Cols(ctx, np.zeros(4, np.int32), np.ones(4, np.int64), np.ones(4, np.int64))
    with pytest.raises(exon_amd.ExonHipError) as e:
        st.push_device([(x, None, None) for x in cols.bufs], 4)
    assert e.value.code == ESTATE
    d = ctx.zeros(np.int64, plan.n_i64)
    with pytest.raises(exon_amd.ExonHipError) as e:
        plan.launch(cols.columns(), 4, d)
    assert e.value.code == ESTATE
    with pytest.raises(exon_amd.ExonHipError) as e:
        c = cols.columns()
        ctx.region_set_overlap(c[0][0], None, c[1][0], None, c[2][0], None, 4, plan, d)
    assert e.value.code == ESTATE
    table = st.finish_arrow()  # nothing was counted; the names come back
    assert str(table.type[0].type) == "string" and table.field("contig").to_pylist() == ["chr1", "chr2"]
    assert table.field("count").to_pylist() == [0, 0]
    st.close()
