"""GPU: the window plan (kind 13) against plain numpy (window_bases_expect.py): every state word for word against expect_state, every
decode against the per-base pileup (or its sorted form where a pileup would take minutes): the bare operator, plan launches in both
modes, chunks, folds and streams, in both tiers and both launch shapes, at every window seam and for every division the kernel does."""
import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L

import window_bases_expect as E
import region_set_rows
from region_set_rows import launch

pytestmark = pytest.mark.gpu

LDS_MAX = exon_amd.WINDOW_BASES_LDS_MAX
TILE_S, TILE_B = L.REGION_SET_TILE_SMALL, L.REGION_SET_TILE_BIG
ESTATE = -5

CONTIGS = [(0, 1999), (2, 700), (1, 2500), (4, 64), (5, 1)]  # ids 3 and 6 are inside the map and not in the plan
W0 = 64


class Cols(region_set_rows.Cols):
    def want(self, contigs, W, fast=False):
        return (E.expect_fast if fast else E.expect)(contigs, W, *self.host, *self.valid)

    def state(self, contigs, W):
        return E.expect_state(contigs, W, *self.host, *self.valid)


def check(plan, cols, state, contigs, W, fast=False):
    totals, bases = cols.want(contigs, W, fast)
    assert state[:4].tolist() == totals.tolist()
    assert np.array_equal(state, cols.state(contigs, W))  # word for word
    assert plan.decode(state).tolist() == bases.tolist()
    return totals, bases


def random_rows(rng, n, n_refs=6, span=2600, null=0.05, inverted=0.02, length=150):
    ref = rng.integers(-1, n_refs + 1, n).astype(np.int32)
    start = rng.integers(-40, span, n)  # below 1 and beyond every contig's end
    end = start + rng.integers(0, length, n)
    inv = rng.random(n) < inverted
    end[inv] = start[inv] - rng.integers(1, 5, int(inv.sum()))
    return ref, start, end, rng.random(n) >= null, rng.random(n) >= null, rng.random(n) >= null


SEAMS = [10, 11, 20, 21, 30, 31, 35, 36]


@pytest.mark.parametrize("row,want", [
    ((3, 7), [5, 0, 0, 0]), ((12, 15), [0, 4, 0, 0]),                        # inside one window
    ((10, 11), [1, 1, 0, 0]), ((5, 25), [6, 10, 5, 0]), ((1, 35), [10, 10, 10, 5]),  # two, three, all four
    ((11, 20), [0, 10, 0, 0]), ((31, 35), [0, 0, 0, 5]),                     # equal to a window, and to the short last one
    ((0, 3), [3, 0, 0, 0]), ((-5, 12), [10, 2, 0, 0]), ((33, 135), [0, 0, 0, 3]), ((-5, 135), [10, 10, 10, 5]),  # clipped
    ((36, 40), [0, 0, 0, 0]), ((-3, 0), [0, 0, 0, 0]),                       # s = L + 1, e = 0: counted, in no window
] + [((s, e), None) for s in SEAMS for e in SEAMS if s <= e])
def test_one_row_at_every_seam(ctx, row, want):
    contigs = [(0, 35)]
    plan = ctx.plan_window_bases(contigs, 10, columns=(0, 1, 2))
    cols = Cols(ctx, [0], [row[0]], [row[1]])
    st = launch(ctx, plan, cols).to_host()
    totals, bases = check(plan, cols, st, contigs, 10)
    assert totals.tolist() == [1, 0, 0, 0]
    if want is not None:
        assert bases.tolist() == want
    assert bases.sum() == max(0, min(row[1], 35) - max(row[0], 1) + 1)


def seam_rows(W, ln):
    """every pair of coordinates taken from k * W - 1 .. k * W + 2 at k = 0, the middle and K"""
    K = (ln - 1) // W + 1
    xs = sorted({k * W + d for k in (0, K // 2, K) for d in (-1, 0, 1, 2)} | {ln - 1, ln, ln + 1})
    s, e = np.meshgrid(np.array(xs, np.int64), np.array(xs, np.int64), indexing="ij")
    return s.ravel(), e.ravel()


@pytest.mark.parametrize("W,ln", [(1, 8192), (2, 16383), (3, 3 * 8192 - 2), (7, 7 * 8192), (1000, 8192 * 1000 - 3), (1023, 8192 * 1023),
                                  (1024, 8192 * 1024), (1025, 8191 * 1025 + 1), (2**20 + 1, 2**31 - 1), (2**31 - 1, 2**31 - 1)])
def test_exact_division_at_the_seams(ctx, W, ln):
    contigs = [(0, ln)]
    plan = ctx.plan_window_bases(contigs, W, columns=(0, 1, 2))
    assert (plan.n_i64 - 4) // 2 <= LDS_MAX
    s, e = seam_rows(W, ln)
    cols = Cols(ctx, np.zeros(len(s), np.int32), s, e)
    st = launch(ctx, plan, cols).to_host()
    totals, bases = check(plan, cols, st, contigs, W, fast=True)
    k = int(round(len(s) ** 0.5))  # every pair of k coordinates: s <= e in k (k + 1) / 2 of them, the others are inverted
    assert k >= 8 and totals.tolist() == [k * (k + 1) // 2, 0, 0, k * (k - 1) // 2] and bases.sum() > 0
    short = (e - s >= 0) & (e - s <= 5000)  # by pileup where that is a matter of seconds; every row next to a seam is among them
    few = Cols(ctx, np.zeros(int(short.sum()), np.int32), s[short], e[short])
    assert short.sum() >= 20  # (four neighbouring coordinates give ten pairs, and there are two such groups or more)
    check(plan, few, launch(ctx, plan, few).to_host(), contigs, W)


def test_row_classes(ctx):
    rng = np.random.default_rng(2)
    ref, start, end, rv, sv, ev = random_rows(rng, 4000)
    ref[:50] = -1
    ref[50:100] = 6            # beyond the map (its last id is 5)
    ref[100:150] = 2**31 - 1
    ref[150:200] = -2**31
    ref[200:260] = 3           # inside the map, not in the plan
    cols = Cols(ctx, ref, start, end, rv, sv, ev)
    plan = ctx.plan_window_bases(CONTIGS, W0, columns=(0, 1, 2))
    st = launch(ctx, plan, cols).to_host()
    totals, bases = check(plan, cols, st, CONTIGS, W0)
    assert totals.min() > 0 and totals.sum() == cols.n  # all four classes occur
    assert totals[2] >= 260
    assert cols.want(CONTIGS, W0, fast=True)[1].tolist() == bases.tolist()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_each_column_null_alone(ctx, which):
    rng = np.random.default_rng(3 + which)
    ref, start, end, _, _, _ = random_rows(rng, 3000, inverted=0)
    v = [None, None, None]
    v[which] = rng.random(3000) < 0.5
    cols = Cols(ctx, ref, start, end, *v)
    plan = ctx.plan_window_bases(CONTIGS, W0, columns=(0, 1, 2))
    st = launch(ctx, plan, cols).to_host()
    check(plan, cols, st, CONTIGS, W0)
    assert st[1] == (~v[which]).sum() > 0


def test_inverted_rows_add_to_no_window(ctx):
    contigs = [(0, 100)]
    cols = Cols(ctx, [0, 0, 0, 0], [70, 50, 61, 30], [30, 50, 39, 70])
    plan = ctx.plan_window_bases(contigs, 10, columns=(0, 1, 2))
    st = launch(ctx, plan, cols).to_host()
    assert st[:4].tolist() == [2, 0, 0, 2]
    assert plan.decode(st).tolist() == [0, 0, 1, 10, 11, 10, 10, 0, 0, 0]  # [50, 50] and [30, 70] only
    check(plan, cols, st, contigs, 10)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE_S - 1, TILE_S, TILE_S + 1, 3 * TILE_S + 517])
def test_row_counts_small_shape(ctx, n):
    rng = np.random.default_rng(100 + n)
    cols = Cols(ctx, *random_rows(rng, n))
    plan = ctx.plan_window_bases(CONTIGS, W0, columns=(0, 1, 2))
    d = ctx.to_device(np.full(plan.n_i64, -7, np.int64))  # overwrite: garbage in front, n = 0 included
    check(plan, cols, launch(ctx, plan, cols, d_state=d).to_host(), CONTIGS, W0)


@pytest.mark.parametrize("extra", [TILE_B - 1, TILE_B + 1])
@pytest.mark.parametrize("tier", ["lds", "global"])
def test_row_counts_big_shape(ctx, extra, tier):
    """the 1024-thread shape takes over once every CU gets a tile: that many rows and one tile -/+ 1 more"""
    n = ctx.info()["compute_units"] * TILE_B + extra
    rng = np.random.default_rng(extra)
    contigs, W = (CONTIGS, W0) if tier == "lds" else ([(0, 5000), (2, 3000), (1, 2500), (4, 64), (5, 1)], 1)
    cols = Cols(ctx, *random_rows(rng, n, null=0.01))
    plan = ctx.plan_window_bases(contigs, W, columns=(0, 1, 2))
    B = (plan.n_i64 - 4) // 2
    assert B <= LDS_MAX // 4 if tier == "lds" else B > LDS_MAX
    check(plan, cols, launch(ctx, plan, cols).to_host(), contigs, W, fast=True)


@pytest.mark.parametrize("shift", [(1, 1, 1), (3, 1, 1), (2, 1, 0), (1, 0, 0), (0, 1, 0)])
def test_unaligned_column_bases(ctx, shift):
    """(1, 1, 1) and (3, 1, 1) line up behind a head of 3 / 1 rows; the others never do and are read row by row"""
    rng = np.random.default_rng(sum(shift))
    cols = Cols(ctx, *random_rows(rng, 2 * TILE_S + 77), shift=shift)
    plan = ctx.plan_window_bases(CONTIGS, W0, columns=(0, 1, 2))
    check(plan, cols, launch(ctx, plan, cols).to_host(), CONTIGS, W0)
    d = ctx.zeros(np.int64, plan.n_i64)
    c = cols.columns()
    ctx.window_bases(c[0][0], c[0][1], c[1][0], c[1][1], c[2][0], c[2][1], cols.n, plan, d)  # the bare operator takes them too
    ctx.sync()
    check(plan, cols, d.to_host(), CONTIGS, W0)


def edge_contigs(total, many):
    """B == total.  One contig of `total` windows of width 7, the last one short; or contigs of one to three windows of width 50"""
    if not many:
        return [(0, 7 * total - 4)], 7
    rng = np.random.default_rng(total)
    contigs, left = [], total
    while left:
        k = min(int(rng.integers(1, 4)), left)
        contigs.append((len(contigs), 50 * (k - 1) + int(rng.integers(1, 51))))
        left -= k
    return contigs, 50


@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("total", [LDS_MAX, LDS_MAX + 1])
def test_tier_edge(ctx, total, many):
    contigs, W = edge_contigs(total, many)
    plan = ctx.plan_window_bases(contigs, W, columns=(0, 1, 2))
    assert plan.n_i64 == 4 + 2 * total and plan.offsets()[-1] == total
    rng = np.random.default_rng(7)
    n = 30_000
    ref = rng.integers(0, len(contigs) + 2, n).astype(np.int32)
    start = rng.integers(-20, 180 if many else 7 * total + 50, n)
    end = start + rng.integers(0, 120 if many else 300, n)
    cols = Cols(ctx, ref, start, end, rng.random(n) < 0.97)
    check(plan, cols, launch(ctx, plan, cols).to_host(), contigs, W, fast=True)
    sub = slice(0, 400)  # and by pileup on a few rows, in the same plan
    few = Cols(ctx, ref[sub], start[sub], end[sub])
    check(plan, few, launch(ctx, plan, few).to_host(), contigs, W)


def test_global_tier(ctx):
    rng = np.random.default_rng(11)
    contigs, W = [(0, 100_000)], 7
    n = 200_000
    start = rng.integers(-100, 100_300, n)
    end = start + rng.integers(0, 400, n)
    cols = Cols(ctx, np.zeros(n, np.int32), start, end, None, rng.random(n) < 0.99, None)
    plan = ctx.plan_window_bases(contigs, W, columns=(0, 1, 2))
    assert (plan.n_i64 - 4) // 2 == 14_286 > LDS_MAX
    st = launch(ctx, plan, cols).to_host()
    check(plan, cols, st, contigs, W, fast=True)
    at = plan.layout()
    assert np.count_nonzero(st[at[2]:at[3]]) > 5000  # D is used throughout


@pytest.mark.parametrize("tier", ["lds", "global"])
def test_hot_bin_sorted_rows(ctx, tier):
    """a coordinate-sorted file: a million rows inside ONE window, ascending -- whole waves on one bin, whose values the wave sums
    before it adds"""
    k = LDS_MAX // 2 if tier == "lds" else 2 * LDS_MAX
    contigs, W = [(0, 1000 * k)], 1000
    n = 1_000_000
    rng = np.random.default_rng(5)
    start = np.sort(rng.integers(1_000_001, 1_000_800, n))  # window 1000 = [1000001, 1001000]
    end = start + rng.integers(0, 100, n)
    cols = Cols(ctx, np.zeros(n, np.int32), start, end)
    plan = ctx.plan_window_bases(contigs, W, columns=(0, 1, 2))
    assert plan.n_i64 == 4 + 2 * k
    st = launch(ctx, plan, cols).to_host()
    got = plan.decode(st)
    assert got[1000] == int((end - start + 1).sum()) == got.sum()
    check(plan, cols, st, contigs, W, fast=True)


def test_against_kind_12_over_the_same_windows(ctx):
    rng = np.random.default_rng(29)
    W = 3
    cols = Cols(ctx, *random_rows(rng, 20_000))
    regions = E.windows(CONTIGS, W)
    assert len(regions) <= 4000
    k13 = ctx.plan_window_bases(CONTIGS, W, columns=(0, 1, 2))
    k12 = ctx.plan_region_set_bases(regions, columns=(0, 1, 2))
    a, b = launch(ctx, k13, cols).to_host(), launch(ctx, k12, cols).to_host()
    assert a[:4].tolist() == b[:4].tolist()
    assert k13.decode(a).tolist() == k12.decode(b).tolist()
    assert k13.decode(a).sum() > 0
    check(k13, cols, a, CONTIGS, W, fast=True)


def test_launch_modes_and_chunks(ctx):
    rng = np.random.default_rng(13)
    cols = Cols(ctx, *random_rows(rng, 3 * 4096))
    plan = ctx.plan_window_bases(CONTIGS, W0, columns=(0, 1, 2))
    whole = launch(ctx, plan, cols).to_host()
    check(plan, cols, whole, CONTIGS, W0)
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
    plan = ctx.plan_window_bases(CONTIGS, 5, columns=(0, 1, 2))
    a = launch(ctx, plan, cols, lo=0, hi=2400).to_host()
    b = launch(ctx, plan, cols, lo=2400).to_host()
    out = ctx.zeros(np.int64, plan.n_i64)
    plan.fold_states(ctx.to_device(np.concatenate([a, b])), 2, out)
    ctx.sync()
    whole = launch(ctx, plan, cols).to_host()
    assert np.array_equal(out.to_host(), whole)
    assert np.array_equal(plan.decode(a) + plan.decode(b), plan.decode(whole))
    check(plan, cols, whole, CONTIGS, 5)


def test_streams(ctx):
    import pyarrow as pa
    rng = np.random.default_rng(19)
    plan = ctx.plan_window_bases(CONTIGS, W0, columns=(1, 2, 3))
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
    assert np.array_equal(counts, E.expect_state(CONTIGS, W0, ref, start, end, rv, sv, ev))
    assert plan.decode(counts).tolist() == E.expect(CONTIGS, W0, ref, start, end, rv, sv, ev)[1].tolist()
    # a new query on the same stream: reset, device batches, the Arrow result
    st.reset()
    cols = Cols(ctx, ref[:5000], start[:5000], end[:5000], rv[:5000], sv[:5000], ev[:5000])
    dummy = ctx.zeros(np.int8, 5000)
    st.push_device([(dummy, None, None)] + [(b, v, None) for b, v in zip(cols.bufs, cols.vbufs)], 5000)
    table = st.finish_arrow()
    wins = E.windows(CONTIGS, W0)
    assert [f.name for f in table.type] == ["contig", "start", "end", "bases"]
    assert [str(f.type) for f in table.type] == ["int32", "int64", "int64", "int64"]
    assert table.field("contig").to_pylist() == [w[0] for w in wins]
    assert table.field("start").to_pylist() == [w[1] for w in wins]
    assert table.field("end").to_pylist() == [w[2] for w in wins]
    assert table.field("bases").to_pylist() == cols.want(CONTIGS, W0)[1].tolist()
    # reset with nothing behind it: the empty state
    st.reset()
    assert not st.finish()[0].any()
    st.close()


def test_names_form_refuses_rows_without_a_file(ctx):
    import pyarrow as pa
    plan = ctx.plan_window_bases([("chr1", 25), ("chr2", 10)], 10, columns=(0, 1, 2))
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
        ctx.window_bases(c[0][0], None, c[1][0], None, c[2][0], None, 4, plan, d)
    assert e.value.code == ESTATE
    table = st.finish_arrow()  # nothing was summed; the names come back
    assert str(table.type[0].type) == "string" and table.field("contig").to_pylist() == ["chr1"] * 3 + ["chr2"]
    assert table.field("start").to_pylist() == [1, 11, 21, 1] and table.field("end").to_pylist() == [10, 20, 25, 10]
    assert table.field("bases").to_pylist() == [0, 0, 0, 0]
    st.close()
