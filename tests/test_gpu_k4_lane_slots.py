"""K4 with G <= 8 groups keeps its per-lane sums in lane-private LDS slots (one ds_add_f64 per row into the slot of the row's own
group, a dummy row per wave for rows that do not contribute).  Differential tests against numpy in f64: y is a multiple of 1/8
with |y| <= 4096, so every sum is exact in f64 whatever the order and equality is exact.

Shapes: N_BIG takes the 1024-thread shape, deals the workgroups unequal tile counts and leaves a remainder behind the last whole
tile; 700 001 rows take the 256-thread shape; 5 and 0 rows are the degenerate ends."""
import numpy as np
import pytest

import exon_amd

pytestmark = pytest.mark.gpu

N_BIG = 2 * 256 * 16384 + 3 * 16384 + 777
SHAPES = [N_BIG, 700_001, 5, 0]
GROUPS = [1, 5, 8]
THR = 0.25
OPS = {">": np.greater, "!=": np.not_equal}


def _bits(ok):
    return np.packbits(np.asarray(ok, np.uint8), bitorder="little")


class Table:
    """One set of columns per row count, uploaded once and never changed; references are computed per case from the host copies."""

    def __init__(self, ctx, n):
        rng = np.random.default_rng(1000 + n % 9973)
        self.ctx, self.n = ctx, n
        self.x = rng.choice(np.array([0.0, 0.01, 0.25, 0.5, 1.0, -1.0], np.float32), n)
        self.yf = (rng.integers(-32768, 32769, n) / 8.0).astype(np.float32)  # eighths, |y| <= 4096
        self.yi = rng.integers(-4096, 4097, n).astype(np.int32)
        self.base = rng.integers(0, 8, n).astype(np.int32)
        self.xok = rng.random(n) < 0.8
        self.yok = rng.random(n) < 0.6
        self.d = {}
        self.up("x", self.x)
        self.up("yf", self.yf)
        self.up("yi", self.yi)
        self.up("xok", _bits(self.xok))
        self.up("yok", _bits(self.yok))

    def up(self, name, host):
        """upload (with 64 spare elements behind, so that a zero-row table still has an address)"""
        self.d[name] = self.ctx.to_device(np.concatenate([host, np.zeros(64, host.dtype)]))
        return self.d[name]

    def gid(self, G):
        return self.base % G

    def d_gid(self, G):
        return self.d[("gid", G)] if ("gid", G) in self.d else self.up(("gid", G), self.gid(G))

    def keep(self, op, valid):
        k = OPS[op](self.x.astype(np.float64), THR)  # a Float32 column against a Float64 literal: the COLUMN is widened
        return k & self.xok if valid else k

    def expect(self, gid, G, keep, y, yok):
        yv = keep if yok is None else keep & yok
        crow = np.bincount(gid[keep], minlength=G)
        cnn = np.bincount(gid[yv], minlength=G)
        sums = np.bincount(gid[yv], weights=y[yv].astype(np.float64), minlength=G)
        return cnn, crow, sums


_TABLES = {}


@pytest.fixture(scope="module")
def tables(ctx):
    def get(n):
        if n not in _TABLES:
            _TABLES[n] = Table(ctx, n)
        return _TABLES[n]
    yield get
    _TABLES.clear()


def _launch(ctx, G, op, x, xv, y, yv, gid, n, y_type="f32", state=None, overwrite=True):
    plan = ctx.plan_cmp_avg_by_group(op, THR, G, y_type=y_type)
    st = ctx.zeros(np.int64, 3 * G) if state is None else state
    plan.launch([(x, xv, None), (y, yv, None), (gid, None, None)], n, st, overwrite=overwrite)
    ctx.sync()
    plan.close()
    return st


def _split(st, G):
    w = st.to_host()
    return w[:G], w[G:2 * G], w[2 * G:].view(np.float64)


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("n", SHAPES)
def test_sums_and_counts(ctx, tables, n, G):
    t = tables(n)
    gid, dg = t.gid(G), t.d_gid(G)
    for y_type, y, dy in (("f32", t.yf, t.d["yf"]), ("i32", t.yi, t.d["yi"])):
        for valid in (True, False):
            for op in OPS:
                st = _launch(ctx, G, op, t.d["x"], t.d["xok"] if valid else None, dy, t.d["yok"] if valid else None, dg, n, y_type)
                cnn, crow, sums = t.expect(gid, G, t.keep(op, valid), y, t.yok if valid else None)
                got = _split(st, G)
                what = (n, G, y_type, valid, op)
                assert np.array_equal(got[0], cnn), what
                assert np.array_equal(got[1], crow), what
                assert np.array_equal(got[2], sums), what


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("n", [N_BIG, 700_001])
def test_dummy_row_isolation(ctx, tables, n, G):
    """NaN, +Inf, -Inf and -0.0 on every row that fails the predicate or whose y is NULL: no real slot may see them.  Then ONE
    passing, valid NaN: it lands in its own group and nowhere else."""
    t = tables(n)
    gid, dg = t.gid(G), t.d_gid(G)
    keep = t.keep(">", True)
    live = keep & t.yok
    if "poison" not in t.d:
        y = t.yf.copy()
        dead = np.flatnonzero(~live)
        y[dead] = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)[np.arange(dead.size) % 4]
        t.poison = y
        t.up("poison", y)
    st = _launch(ctx, G, ">", t.d["x"], t.d["xok"], t.d["poison"], t.d["yok"], dg, n)
    cnn, crow, sums = t.expect(gid, G, keep, t.yf, t.yok)
    got = _split(st, G)
    assert np.array_equal(got[0], cnn) and np.array_equal(got[1], crow)
    assert np.all(np.isfinite(got[2])) and np.array_equal(got[2], sums)

    y = t.poison.copy()
    at = int(np.flatnonzero(live)[-1])  # a row of the remainder behind the last whole tile, if the shape has one
    y[at] = np.nan
    dy = ctx.to_device(y)
    st = _launch(ctx, G, ">", t.d["x"], t.d["xok"], dy, t.d["yok"], dg, n)
    yh = t.yf.copy()
    yh[at] = np.nan
    cnn, crow, sums = t.expect(gid, G, keep, yh, t.yok)
    got = _split(st, G)
    assert np.array_equal(got[0], cnn) and np.array_equal(got[1], crow)
    assert np.isnan(got[2][gid[at]]) and np.isnan(got[2]).sum() == 1
    assert np.array_equal(got[2], sums, equal_nan=True)


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("n", [N_BIG, 700_001])
def test_one_group_and_all_null(ctx, tables, n, G):
    t = tables(n)
    only = G - 1
    gid = np.full(n, only, np.int32)
    dg = ctx.to_device(gid)
    keep = t.keep(">", True)
    st = _launch(ctx, G, ">", t.d["x"], t.d["xok"], t.d["yf"], t.d["yok"], dg, n)
    cnn, crow, sums = t.expect(gid, G, keep, t.yf, t.yok)
    got = _split(st, G)
    assert np.array_equal(got[0], cnn) and np.array_equal(got[1], crow) and np.array_equal(got[2], sums)
    assert np.array_equal(got[2].view(np.int64)[:only], np.zeros(only, np.int64))  # +0.0 where nothing contributed
    # every y NULL: COUNT(*) as before, COUNT(y) = 0, every sum +0.0
    nulls = ctx.zeros(np.uint8, n // 8 + 64)
    st = _launch(ctx, G, ">", t.d["x"], t.d["xok"], t.d["yf"], nulls, t.d_gid(G), n)
    got = _split(st, G)
    assert np.array_equal(got[0], np.zeros(G, np.int64))
    assert np.array_equal(got[1], np.bincount(t.gid(G)[keep], minlength=G))
    assert np.array_equal(got[2].view(np.int64), np.zeros(G, np.int64))


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("n", [N_BIG, 700_001])
def test_ids_out_of_range(ctx, tables, n, G):
    """An id >= G or < 0 on a passing row is reported at the next sync, and it wrote nothing outside its wave's block of slots:
    the next launch on the same context is right."""
    t = tables(n)
    keep = t.keep(">", True)
    rows = np.flatnonzero(keep & t.yok)
    for bad in (G, G + 100000, -1):
        gid = t.gid(G).copy()
        gid[rows[[0, rows.size // 2, -1]]] = bad  # the first tile, the middle, the remainder
        dg = ctx.to_device(gid)
        plan = ctx.plan_cmp_avg_by_group(">", THR, G)
        st = ctx.zeros(np.int64, 3 * G)
        plan.launch([(t.d["x"], t.d["xok"], None), (t.d["yf"], t.d["yok"], None), (dg, None, None)], n, st, overwrite=True)
        with pytest.raises(exon_amd.ExonHipError, match="group id out of range"):
            ctx.sync()
        plan.close()
        st = _launch(ctx, G, ">", t.d["x"], t.d["xok"], t.d["yf"], t.d["yok"], t.d_gid(G), n)
        cnn, crow, sums = t.expect(t.gid(G), G, keep, t.yf, t.yok)
        got = _split(st, G)
        assert np.array_equal(got[0], cnn) and np.array_equal(got[1], crow) and np.array_equal(got[2], sums), bad


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("n", [N_BIG, 700_001])
def test_accumulate_two_halves(ctx, tables, n, G):
    t = tables(n)
    dg = t.d_gid(G)
    h = n // 2 // 64 * 64  # a split on a bitmap byte and a 16-byte boundary
    whole = _split(_launch(ctx, G, ">", t.d["x"], t.d["xok"], t.d["yf"], t.d["yok"], dg, n), G)
    st = ctx.zeros(np.int64, 3 * G)
    for lo, m in ((0, h), (h, n - h)):
        _launch(ctx, G, ">", t.d["x"].ptr + 4 * lo, t.d["xok"].ptr + lo // 8, t.d["yf"].ptr + 4 * lo, t.d["yok"].ptr + lo // 8,
                dg.ptr + 4 * lo, m, state=st, overwrite=False)
    got = _split(st, G)
    for a, b in zip(got, whole):
        assert np.array_equal(a, b)
    cnn, crow, sums = t.expect(t.gid(G), G, t.keep(">", True), t.yf, t.yok)
    assert np.array_equal(got[0], cnn) and np.array_equal(got[1], crow) and np.array_equal(got[2], sums)


@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("n", [N_BIG, 700_001])
def test_deterministic(ctx, tables, n, G):
    """f32 y that is no multiple of 1/8: the sums round, and three launches still give the same bytes."""
    t = tables(n)
    if "frac" not in t.d:
        t.up("frac", np.random.default_rng(7).normal(30.0, 1000.0, n).astype(np.float32))
    states = [_launch(ctx, G, ">", t.d["x"], t.d["xok"], t.d["frac"], t.d["yok"], t.d_gid(G), n).to_host().tobytes() for _ in range(3)]
    assert states[0] == states[1] == states[2]
    assert np.any(np.frombuffer(states[0], np.int64)[:G] > 0)
