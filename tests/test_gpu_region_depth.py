"""GPU: the region-set depth plan (kind 14) against plain numpy (region_depth_expect.py): every state word for word against
expect_state, and per_base, decode and the device reduce against the per-base pileup (or its sorted form where a pileup would take
minutes): the bare operator, plan launches in both modes, chunks, folds and streams, in every tier and both launch shapes, at every
target seam and at every seam of the reduce's tiles.  The reduce must leave the state as it found it."""
import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L

import region_depth_expect as E
import region_set_rows
from region_set_rows import launch

pytestmark = pytest.mark.gpu

LDS_MAX = exon_amd.REGION_DEPTH_LDS_MAX
RT = exon_amd.REGION_DEPTH_REDUCE_TILE
TILE_S, TILE_B = L.REGION_SET_TILE_SMALL, L.REGION_SET_TILE_BIG
ESTATE = -5

# ids 3 and 6 are inside the map and not in the set; abutting, nested, duplicate and overlapping regions, gaps of one base and more
REGIONS = [(0, 100, 180), (0, 181, 260), (0, 262, 300), (2, 1, 50), (0, 120, 130), (1, 500, 1999), (1, 700, 2100), (4, 7, 7), (5, 1, 1),
           (0, 900, 1400), (2, 1, 50), (0, 1402, 1402), (2, 60, 61), (1, 1, 3)]
THR = [1, 2, 10, 20]


class Cols(region_set_rows.Cols):
    def want(self, regions, thr, fast=False):
        return E.expect(regions, thr, *self.host, *self.valid, fast=fast)

    def state(self, regions):
        return E.expect_state(regions, *self.host, *self.valid)


def check(ctx, plan, cols, d_state, regions, thr, fast=False):
    """the state word for word; per_base, decode and reduce against the pileup; the reduce leaves the state alone"""
    state = d_state.to_host()
    totals, depth, bases, ge = cols.want(regions, thr, fast)
    assert state[:4].tolist() == totals.tolist()
    assert np.array_equal(state, cols.state(regions))
    assert np.array_equal(plan.per_base(state), depth)
    b, g = plan.decode(state)
    assert np.array_equal(b, bases) and np.array_equal(g, ge)
    d_table = plan.reduce(d_state)
    ctx.sync()
    table = d_table.to_host().reshape(len(regions), 1 + len(thr))
    assert np.array_equal(table[:, 0], bases) and np.array_equal(table[:, 1:], ge)
    assert np.array_equal(d_state.to_host(), state)  # byte for byte
    if len(thr):  # ge falls along the thresholds and stays within the region (thresholds[0] >= 1)
        assert (np.diff(ge, axis=1) <= 0).all() and (ge[:, 0] <= [e - s + 1 for _, s, e in regions]).all()
    return totals, depth, bases, ge


def random_rows(rng, n, n_refs=6, span=2300, null=0.05, inverted=0.02, length=150):
    ref = rng.integers(-1, n_refs + 1, n).astype(np.int32)
    start = rng.integers(-40, span, n)  # below 1 and beyond every target
    end = start + rng.integers(0, length, n)
    inv = rng.random(n) < inverted
    end[inv] = start[inv] - rng.integers(1, 5, int(inv.sum()))
    return ref, start, end, rng.random(n) >= null, rng.random(n) >= null, rng.random(n) >= null


SEAMS = [9, 10, 11, 12, 19, 20, 21, 22, 29, 30, 31, 32, 39, 40, 41, 42]


def test_one_row_at_every_seam(ctx):
    regions, thr = [(0, 11, 20), (0, 31, 40)], [1, 2]
    plan = ctx.plan_region_set_depth(regions, thr, columns=(0, 1, 2))
    assert plan.n_i64 == 4 + 21
    rows = [(s, e) for s in SEAMS for e in SEAMS if s <= e]
    assert (21, 29) in rows and (20, 31) in rows and (9, 42) in rows  # inside the gap, across it, over everything
    rows += [(-2**63, 2**63 - 1), (-2**63, 15), (35, 2**63 - 1), (1, 12), (1, 2**63 - 1), (-5, 0), (0, 0), (-2**63, 0), (1, 1), (-2**63, -2**63)]
    for s, e in rows:
        cols = Cols(ctx, [0], [s], [e])
        d = launch(ctx, plan, cols)
        totals, depth, bases, ge = check(ctx, plan, cols, d, regions, thr)
        assert totals.tolist() == [1, 0, 0, 0]
        covered = [x for x in list(range(11, 21)) + list(range(31, 41)) if s <= x <= e]
        assert depth.sum() == len(covered) == bases.sum() == ge[:, 0].sum() and not ge[:, 1].any()
        st = d.to_host()
        assert np.count_nonzero(st[4:]) == (2 if covered else 0)  # a row inside the gap makes no add, one across it one pair


def test_row_classes(ctx):
    rng = np.random.default_rng(2)
    ref, start, end, rv, sv, ev = random_rows(rng, 4000)
    ref[:50] = -1
    ref[50:100] = 6            # beyond the map (its last id is 5)
    ref[100:150] = 2**31 - 1
    ref[150:200] = -2**31
    ref[200:260] = 3           # inside the map, not in the set
    cols = Cols(ctx, ref, start, end, rv, sv, ev)
    plan = ctx.plan_region_set_depth(REGIONS, THR, columns=(0, 1, 2))
    totals, depth, bases, ge = check(ctx, plan, cols, launch(ctx, plan, cols), REGIONS, THR)
    assert totals.min() > 0 and totals.sum() == cols.n  # all four classes occur
    assert totals[2] >= 260 and depth.max() >= 20 and ge[:, 3].sum() > 0
    fast = cols.want(REGIONS, THR, fast=True)
    assert np.array_equal(fast[1], depth) and np.array_equal(fast[3], ge)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_each_column_null_alone(ctx, which):
    rng = np.random.default_rng(3 + which)
    ref, start, end, _, _, _ = random_rows(rng, 3000, inverted=0)
    v = [None, None, None]
    v[which] = rng.random(3000) < 0.5
    cols = Cols(ctx, ref, start, end, *v)
    plan = ctx.plan_region_set_depth(REGIONS, THR, columns=(0, 1, 2))
    d = launch(ctx, plan, cols)
    check(ctx, plan, cols, d, REGIONS, THR)
    assert d.to_host()[1] == (~v[which]).sum() > 0


def test_inverted_rows_add_to_no_bin(ctx):
    regions = [(0, 1, 100)]
    cols = Cols(ctx, [0, 0, 0, 0], [70, 50, 61, 30], [30, 50, 39, 70])
    plan = ctx.plan_region_set_depth(regions, [1, 2], columns=(0, 1, 2))
    d = launch(ctx, plan, cols)
    st = d.to_host()
    assert st[:4].tolist() == [2, 0, 0, 2]
    assert plan.decode(st)[0].tolist() == [42] and plan.decode(st)[1].tolist() == [[41, 1]]  # [50, 50] and [30, 70] only
    check(ctx, plan, cols, d, regions, [1, 2])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE_S - 1, TILE_S, TILE_S + 1])
def test_row_counts_small_shape(ctx, n):
    rng = np.random.default_rng(100 + n)
    cols = Cols(ctx, *random_rows(rng, n))
    plan = ctx.plan_region_set_depth(REGIONS, THR, columns=(0, 1, 2))
    d = ctx.to_device(np.full(plan.n_i64, -7, np.int64))  # overwrite: garbage in front, n = 0 included
    check(ctx, plan, cols, launch(ctx, plan, cols, d_state=d), REGIONS, THR)


GLOBAL_REGIONS = [(c, 1 + 250 * j, 200 + 250 * j) for c in (0, 2) for j in range(25)] + [(1, 10, 1500)]


@pytest.mark.parametrize("extra", [TILE_B - 1, TILE_B + 1])
@pytest.mark.parametrize("tier", ["lds", "global"])
def test_row_counts_big_shape(ctx, extra, tier):
    """the 1024-thread shape takes over once every CU gets a tile: that many rows and one tile -/+ 1 more"""
    n = ctx.info()["compute_units"] * TILE_B + extra
    rng = np.random.default_rng(extra)
    regions = REGIONS if tier == "lds" else GLOBAL_REGIONS
    cols = Cols(ctx, *random_rows(rng, n, null=0.01, span=6400 if tier == "global" else 2300))
    plan = ctx.plan_region_set_depth(regions, THR, columns=(0, 1, 2))
    assert plan.n_i64 - 4 <= LDS_MAX // 2 if tier == "lds" else plan.n_i64 - 4 > LDS_MAX
    check(ctx, plan, cols, launch(ctx, plan, cols), regions, THR, fast=True)


@pytest.mark.parametrize("shift", [(1, 1, 1), (3, 1, 1), (2, 1, 0), (1, 0, 0), (0, 1, 0)])
def test_unaligned_column_bases(ctx, shift):
    """(1, 1, 1) and (3, 1, 1) line up behind a head of 3 / 1 rows; the others never do and are read row by row"""
    rng = np.random.default_rng(sum(shift))
    cols = Cols(ctx, *random_rows(rng, 2 * TILE_S + 77), shift=shift)
    plan = ctx.plan_region_set_depth(REGIONS, THR, columns=(0, 1, 2))
    check(ctx, plan, cols, launch(ctx, plan, cols), REGIONS, THR)
    d = ctx.zeros(np.int64, plan.n_i64)
    c = cols.columns()
    ctx.region_set_depth(c[0][0], c[0][1], c[1][0], c[1][1], c[2][0], c[2][1], cols.n, plan, d)  # the bare operator takes them too
    ctx.sync()
    check(ctx, plan, cols, d, REGIONS, THR)


def edge_set(total, many):
    """T + C == total.  One long region; or regions of one to three bases, several on each of many contigs"""
    if not many:
        return [(0, 5, 5 + total - 2)]
    rng = np.random.default_rng(total)
    regions, left, c = [], total, 0
    while left:
        if left == 1:  # a terminator alone is no contig: the last region grows by a base
            c0, s, e = regions[-1]
            regions[-1] = (c0, s, e + 1)
            break
        left -= 1
        pos = 1
        for _ in range(int(rng.integers(5, 40))):
            if not left:
                break
            ln = min(int(rng.integers(1, 4)), left)
            pos += int(rng.integers(2, 6))  # a gap of one base or more in front
            regions.append((c, pos, pos + ln - 1))
            pos += ln
            left -= ln
        c += 1
    return regions


@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("total", [LDS_MAX, LDS_MAX + 1])
def test_tier_edge(ctx, total, many):
    regions = edge_set(total, many)
    plan = ctx.plan_region_set_depth(regions, THR, columns=(0, 1, 2))
    assert plan.n_i64 == 4 + total
    n_contigs = regions[-1][0] + 1
    if many:  # the most intervals a set of this size has here: the largest table the LDS tier copies
        assert n_contigs > 100 and 3000 < len(plan.intervals()[0]) == len(regions) <= 4096
    rng = np.random.default_rng(7)
    n = 30_000
    ref = rng.integers(0, n_contigs + 2, n).astype(np.int32)
    start = rng.integers(-20, 260 if many else total + 50, n)
    end = start + rng.integers(0, 60 if many else 300, n)
    cols = Cols(ctx, ref, start, end, rng.random(n) < 0.97)
    check(ctx, plan, cols, launch(ctx, plan, cols), regions, THR, fast=True)
    sub = slice(0, 400)  # and by pileup on a few rows, in the same plan
    few = Cols(ctx, ref[sub], start[sub], end[sub])
    check(ctx, plan, few, launch(ctx, plan, few), regions, THR)


def test_one_base_targets_search_through_l2(ctx):
    """nearly an interval a bin: the bins stay in LDS, the table (16 bytes an interval) no longer fits beside them"""
    regions = [(0, 3 * i + 1, 3 * i + 1) for i in range(5600)]
    plan = ctx.plan_region_set_depth(regions, [1, 5], columns=(0, 1, 2))
    assert plan.n_i64 - 4 == 5601 <= LDS_MAX and 5601 * 8 + 5600 * 16 > 128 * 1024
    rng = np.random.default_rng(23)
    n = 40_000
    start = rng.integers(-20, 16_900, n)
    cols = Cols(ctx, np.zeros(n, np.int32), start, start + rng.integers(0, 200, n))
    check(ctx, plan, cols, launch(ctx, plan, cols), regions, [1, 5], fast=True)


def test_global_tier(ctx):
    rng = np.random.default_rng(11)
    regions = [(c, 1 + 300 * j, 200 + 300 * j) for c in (0, 1) for j in range(250)]
    n = 200_000
    ref = rng.integers(0, 2, n).astype(np.int32)
    start = rng.integers(-100, 75_300, n)
    end = start + rng.integers(0, 400, n)
    cols = Cols(ctx, ref, start, end, None, rng.random(n) < 0.99, None)
    plan = ctx.plan_region_set_depth(regions, THR, columns=(0, 1, 2))
    assert plan.n_i64 - 4 == 100_002 > LDS_MAX
    d = launch(ctx, plan, cols)
    check(ctx, plan, cols, d, regions, THR, fast=True)
    assert np.count_nonzero(d.to_host()[4:]) > 50_000  # D is used throughout


@pytest.mark.parametrize("tier", ["lds", "global"])
def test_hot_bin(ctx, tier):
    """amplicon data: a million rows on one start -- whole waves on one bin, combined before they add"""
    regions = [(0, 1000, 1000 + (LDS_MAX // 2 if tier == "lds" else 2 * LDS_MAX))]
    n = 1_000_000
    rng = np.random.default_rng(5)
    start = np.full(n, 1500, np.int64)
    end = start + rng.integers(0, 100, n)
    cols = Cols(ctx, np.zeros(n, np.int32), start, end)
    plan = ctx.plan_region_set_depth(regions, [1, 1_000_000, 1_000_001], columns=(0, 1, 2))
    d = launch(ctx, plan, cols)
    st = d.to_host()
    assert st[4 + 500] == n and plan.per_base(st)[500] == n
    totals, depth, bases, ge = check(ctx, plan, cols, d, regions, [1, 1_000_000, 1_000_001], fast=True)
    assert bases[0] == int((end - start + 1).sum()) and ge[0].tolist() == [100, 1, 0]


def reduce_case(ctx, regions, thr, seed, span, n=6000):
    rng = np.random.default_rng(seed)
    start = rng.integers(-30, span, n)
    cols = Cols(ctx, rng.integers(0, 2, n).astype(np.int32), start, start + rng.integers(0, 2 * RT, n))
    plan = ctx.plan_region_set_depth(regions, thr, columns=(0, 1, 2))
    return check(ctx, plan, cols, launch(ctx, plan, cols), regions, thr, fast=True)


@pytest.mark.parametrize("T", [RT - 2, RT - 1, RT, RT + 1, 5 * RT + 17])
def test_reduce_sections_around_the_tile(ctx, T):
    """T + C at the tile size - 1, at it, + 1, + 2, and several tiles"""
    totals, depth, bases, ge = reduce_case(ctx, [(0, 10, 9 + T), (0, 10, 10), (0, 9 + T, 9 + T)], THR, T, T + 40)
    assert bases[0] == depth.sum() > 0 and ge[0, 0] >= ge[0, 3] > 0


def test_reduce_region_borders_at_the_tile_seams(ctx):
    """one interval from position 1 on contig 0, so bin = position - 1: borders on, one before and one after a seam; a region over
    many tiles nested in another; a second contig behind, whose bins start inside a tile"""
    xs = [RT - 1, RT, RT + 1, RT + 2, 2 * RT, 2 * RT + 1, 3 * RT - 1, 3 * RT]
    regions = [(0, 1, 6 * RT + 5), (0, 3, 6 * RT - 5)] + [(0, a, b) for a in xs for b in xs if a <= b] + [(0, 1, x) for x in xs] + [(1, 5, 5 + 2 * RT)]
    totals, depth, bases, ge = reduce_case(ctx, regions, THR, 31, 6 * RT + 40)
    assert bases[0] == depth[:6 * RT + 5].sum() and bases[-1] == depth[6 * RT + 5:].sum() > 0
    assert (bases[2:] > 0).all()


@pytest.mark.parametrize("k", [0, 8])
def test_reduce_a_thousand_one_base_regions(ctx, k):
    thr = [1, 2, 3, 5, 8, 13, 21, 10**9][:k]
    regions = [(i % 2, 2 * (i // 2) + 1, 2 * (i // 2) + 1) for i in range(1000)]
    totals, depth, bases, ge = reduce_case(ctx, regions, thr, 37 + k, 1040)
    assert np.array_equal(bases[0::2], depth[:500]) and np.array_equal(bases[1::2], depth[500:])  # contig 0's bins, then contig 1's
    assert bases.sum() == depth.sum() > 0 and ge.shape == (1000, k)
    if k:
        assert np.array_equal(ge[:, 0], (bases >= 1).astype(np.int64)) and not ge[:, 7].any()  # a threshold above every depth


def test_against_kind_12(ctx):
    rng = np.random.default_rng(29)
    cols = Cols(ctx, *random_rows(rng, 20_000))
    k14 = ctx.plan_region_set_depth(REGIONS, THR, columns=(0, 1, 2))
    k12 = ctx.plan_region_set_bases(REGIONS, columns=(0, 1, 2))
    da = launch(ctx, k14, cols)
    a, b = da.to_host(), launch(ctx, k12, cols).to_host()
    assert a[:4].tolist() == b[:4].tolist()
    assert k14.decode(a)[0].tolist() == k12.decode(b).tolist() and k12.decode(b).sum() > 0
    check(ctx, k14, cols, da, REGIONS, THR)


def test_launch_modes_and_chunks(ctx):
    rng = np.random.default_rng(13)
    cols = Cols(ctx, *random_rows(rng, 3 * 4096))
    plan = ctx.plan_region_set_depth(REGIONS, THR, columns=(0, 1, 2))
    dw = launch(ctx, plan, cols)
    whole = dw.to_host()
    check(ctx, plan, cols, dw, REGIONS, THR)
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
    plan = ctx.plan_region_set_depth(REGIONS, THR, columns=(0, 1, 2))
    a = launch(ctx, plan, cols, lo=0, hi=2400).to_host()
    b = launch(ctx, plan, cols, lo=2400).to_host()
    out = ctx.zeros(np.int64, plan.n_i64)
    plan.fold_states(ctx.to_device(np.concatenate([a, b])), 2, out)
    ctx.sync()
    assert np.array_equal(out.to_host(), launch(ctx, plan, cols).to_host())
    totals, depth, bases, ge = check(ctx, plan, cols, out, REGIONS, THR)  # decode and reduce AFTER the fold
    assert (plan.decode(a)[0] + plan.decode(b)[0]).tolist() == bases.tolist()
    assert (plan.decode(a)[1] + plan.decode(b)[1]).tolist() != ge.tolist()  # the threshold counts of the parts do not add


def test_streams(ctx):
    import pyarrow as pa
    rng = np.random.default_rng(19)
    plan = ctx.plan_region_set_depth(REGIONS, THR, columns=(1, 2, 3))
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
    counts, sums = st.finish()
    assert sums.size == 0
    assert np.array_equal(counts, E.expect_state(REGIONS, ref, start, end, rv, sv, ev))
    want = E.expect(REGIONS, THR, ref, start, end, rv, sv, ev)
    assert plan.decode(counts)[0].tolist() == want[2].tolist() and plan.decode(counts)[1].tolist() == want[3].tolist()
    # a new query on the same stream: reset, device batches, the Arrow result
    st.reset()
    cols = Cols(ctx, ref[:5000], start[:5000], end[:5000], rv[:5000], sv[:5000], ev[:5000])
    dummy = ctx.zeros(np.int8, 5000)
    st.push_device([(dummy, None, None)] + [(b, v, None) for b, v in zip(cols.bufs, cols.vbufs)], 5000)
    table = st.finish_arrow()
    totals, depth, bases, ge = cols.want(REGIONS, THR)
    assert [f.name for f in table.type] == ["contig", "start", "end", "bases", "ge_1", "ge_2", "ge_10", "ge_20"]
    assert [str(f.type) for f in table.type] == ["int32"] + ["int64"] * 7
    assert len(table) == len(REGIONS)
    assert table.field("contig").to_pylist() == [r[0] for r in REGIONS]
    assert table.field("start").to_pylist() == [r[1] for r in REGIONS]
    assert table.field("end").to_pylist() == [r[2] for r in REGIONS]
    assert table.field("bases").to_pylist() == bases.tolist() and bases.sum() > 0
    for t, name in enumerate(["ge_1", "ge_2", "ge_10", "ge_20"]):
        assert table.field(name).to_pylist() == ge[:, t].tolist()
    # reset with nothing behind it: the empty state
    st.reset()
    assert not st.finish()[0].any()
    st.close()


def test_names_form_refuses_rows_without_a_file(ctx):
    import pyarrow as pa
    plan = ctx.plan_region_set_depth([("chr1", 1, 25), ("chr2", 5, 10), ("chr1", 20, 30)], [3], columns=(0, 1, 2))
    assert plan.by_name and plan.layout() == (0, 4, 4 + 30 + 6 + 2)
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
        ctx.region_set_depth(c[0][0], None, c[1][0], None, c[2][0], None, 4, plan, d)
    assert e.value.code == ESTATE
    table = st.finish_arrow()  # nothing was summed; the names come back
    assert [f.name for f in table.type] == ["contig", "start", "end", "bases", "ge_3"]
    assert str(table.type[0].type) == "string" and table.field("contig").to_pylist() == ["chr1", "chr2", "chr1"]
    assert table.field("start").to_pylist() == [1, 5, 20] and table.field("end").to_pylist() == [25, 10, 30]
    assert table.field("bases").to_pylist() == [0, 0, 0] and table.field("ge_3").to_pylist() == [0, 0, 0]
    st.close()
