"""cmp_avg_by_group (K4) with more than 8 groups: the LDS tier (ids 4 .. 4099) and every form of tier 3 (ids from 4100 on) --
global atomics, the scatter pass (per-workgroup regions, k4_tail_wg_scan / offsets / scatter / aggregate), the direct partition
with one stream per id range and with the four streams of a single range (chunk rollover included) -- on both launch shapes,
with Float32 and Int32 x and y.  Every case is compared with tests/k4_expect.py (numpy, int64 / float64) on all 3 * G state words;
y is a multiple of 1/8 with |y| <= 4096 (or an Int32 with |y| <= 4096), so every float64 sum is exact in any order and equality is
on the bits, +0.0 included.

Which device code a case runs is the host's choice (exon_amd/csrc/host/k4_route.h) and depends on what the stream's tier-3 scratch
has grown to.  The module therefore runs on a Context of its own, follows the scratch through tests/k4_route.py (held against the
C++ by tests/test_k4_route.py) and ASSERTS the route of every launch before it is made: a case that would silently take another
route fails.  Direct cases stay below the range count at which a scratch sized by the launch itself stops fitting the chunk pool,
scatter cases have more than 128 ranges, so both hold whatever ran before on the context; the capacity border itself is walked
on a fresh Context.

Out of scope: tables longer than 2^28 rows (the loop that cuts them into launches).  A test of seconds cannot hold such a table;
tests/test_gpu_fullsize.py keeps covering it by properties."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exon_amd
import k4_expect as E
import k4_route as kr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIT = {"f32": 0.25, "i32": 1}  # the literal each x type is compared with
NL = kr.LDS_GROUPS
JUNK = 0x7F7F7F7F7F7F7F7F
# (x type, y type, bitmaps, op): the two pairs every tier-3 case runs, and the mixed ones
COMBOS = [("f32", "f32", True, ">"), ("i32", "i32", False, "!=")]
MIXED = [("f32", "i32", False, "!="), ("i32", "f32", True, ">")]


class Table:
    """One set of columns per row count, uploaded once and never changed (64 spare elements behind, so that a table of no rows
    still has an address); the references are computed per case from the host copies."""

    def __init__(self, ctx, n):
        rng = np.random.default_rng(4100 + n % 9973)
        self.ctx, self.n = ctx, n
        self.h = {
            ("x", "f32"): rng.choice(np.array([0.0, 0.01, 0.25, 0.5, 1.0, -1.0], np.float32), n),
            ("x", "i32"): rng.choice(np.array([0, 1, 1, 2, 5, -7, 2**31 - 1, -2**31], np.int32), n),
            ("y", "f32"): (rng.integers(-32768, 32769, n) / 8.0).astype(np.float32),  # eighths, |y| <= 4096
            ("y", "i32"): rng.integers(-4096, 4097, n).astype(np.int32),
            "all": np.ones(n, np.float32),  # an x every row of which passes `> 0.25`
        }
        self.xok = rng.random(n) < 0.8
        self.yok = rng.random(n) < 0.6
        self.d = {k: self.up(v) for k, v in self.h.items()}
        self.d["xok"] = self.up(E.bits(self.xok))
        self.d["yok"] = self.up(E.bits(self.yok))
        self._keep = {}

    def up(self, host):
        return self.ctx.to_device(np.concatenate([host, np.zeros(64, host.dtype)]))

    def keep(self, x, op, valid):
        k = (x, op, valid)
        if k not in self._keep:
            self._keep[k] = np.ones(self.n, bool) if x == "all" else E.keep(self.h[("x", x)], op, LIT[x], self.xok if valid else None)
        return self._keep[k]


class Bench:
    """the module's Context, its tables, the mirror of its tier-3 scratch and the list of routes taken"""

    def __init__(self, ctx, log):
        self.ctx, self.log = ctx, log
        self.cus = ctx.info()["compute_units"]
        b = os.environ.get("EXON_HIP_BLOCKS_PER_CU", "")
        self.bpc = int(b) if b.isdigit() and 1 <= int(b) <= 32 else 8
        self.scratch = kr.Scratch(self.cus, self.bpc)
        self.tables = {}
        self.N_BIG = self.cus * 16384 + 3 * 8192 + 777
        self.N_MID = self.cus * 4608 + 5  # the 256-thread shape with 2.25 tiles per CU: where two workgroups fit a CU, some get two tiles

    def table(self, n):
        if n not in self.tables:
            self.tables[n] = Table(self.ctx, n)
        return self.tables[n]

    def n_of(self, kind):
        return {"big": self.N_BIG, "small": 700_001, "small3": 300_001, "mid": self.N_MID}[kind]

    def last_direct(self, n):
        """the most id ranges that go direct on a scratch sized by a launch of n rows itself (so on any larger one too)"""
        r = 1
        while kr.route(self.cus, self.bpc, n, kr.groups_of(r + 1), n + kr.TAIL_SLACK).form == "direct":
            r += 1
        return r

    def route(self, group, n, G, want, big=None):
        """the route of the next launch, asserted: `want` is what the rows of the tile loop meet"""
        r = self.scratch.launch(n, G)
        got = kr.tile_loop_form(r, n)
        assert got == want, (group, n, G, want, r)
        if big is not None:
            assert r.big == big, (group, n, G, r)
        self.log.add((group, n, G, got + ("/%d" % r.n_ranges if r.has_tail else ""), "1024" if r.big else "256"))
        return r

    def launch(self, group, t, G, dg, want, combo=COMBOS[0], n=None, lo=0, state=None, overwrite=True, y=None, yv=None, big=None, sync=True):
        """one launch over rows [lo, lo + n) of table t with the group ids dg (a device buffer); returns the state buffer"""
        x, yt, valid, op = combo
        n = t.n if n is None else n
        if n > 0:
            self.route(group, n, G, want, big)
        plan = self.ctx.plan_cmp_avg_by_group(op, LIT["f32" if x == "all" else x], G, x_type="i32" if x == "i32" else "f32", y_type=yt)
        st = self.ctx.zeros(np.int64, 3 * G) if state is None else state
        dx = t.d["all"] if x == "all" else t.d[("x", x)]
        dy = t.d[("y", yt)] if y is None else y
        dyv = (t.d["yok"] if valid else None) if yv is None else yv
        cols = [(dx.ptr + 4 * lo, t.d["xok"].ptr + lo // 8 if valid and x != "all" else None, None), (dy.ptr + 4 * lo, dyv.ptr + lo // 8 if dyv is not None else None, None),
                (dg.ptr + 4 * lo, None, None)]
        try:
            plan.launch(cols, n, st, overwrite=overwrite)
            if sync:
                self.ctx.sync()
        finally:
            plan.close()
        return st

    def check(self, group, t, G, gid, want, combos=COMBOS, dg=None, big=None):
        """launch every combo over the whole table and compare all 3 * G words with the reference"""
        dg = t.up(gid) if dg is None else dg
        for combo in combos:
            x, yt, valid, op = combo
            got = self.launch(group, t, G, dg, want, combo, big=big).to_host()
            same(got, G, gid, t.keep(x, op, valid), t.h[("y", yt)], t.yok if valid else None, (group, t.n, G, combo))
        return dg


def same(got, G, gid, kept, y, yok, what):
    cnn, crow, sums = E.expect(gid, G, kept, y, yok)
    assert got.size == 3 * G
    assert np.array_equal(got[G:2 * G], crow), what
    assert np.array_equal(got[:G], cnn), what
    assert np.array_equal(got[2 * G:], sums.view(np.int64)), what  # the bits: a group nothing was added to holds +0.0


@pytest.fixture(scope="module")
def K():
    ctx = exon_amd.Context(0)
    log = set()
    yield Bench(ctx, log)
    path = os.environ.get("EXON_K4_TIERS_ROUTES")
    if path:  # the (case group, rows, groups, form / ranges, threads) the module ran, for the record
        with open(path, "w") as f:
            f.write("".join("%s n=%d G=%d %s %s\n" % r for r in sorted(log)))
    ctx.close()


# ---- id patterns ------------------------------------------------------------------------------------------------------------
def ids_uniform(rng, n, G):
    return rng.integers(0, G, n).astype(np.int32)


def ids_zipf(rng, n, G):
    """log-uniform: P(id < k) = ln(k + 1) / ln(G + 1), frequent keys early (bench.py --group-dist zipf)"""
    return np.minimum(np.exp(rng.random(n) * np.log(G + 1.0)) - 1.0, G - 1).astype(np.int32)


def ids_runs(n, G, run):
    """a key that changes exactly every `run` rows"""
    return ((np.arange(n, dtype=np.int64) // run * 37) % G).astype(np.int32)


def only_ranges(gid, allowed):
    """the tier-3 rows outside the id ranges `allowed` moved into tiers 1 and 2"""
    g = gid.copy()
    move = (g >= NL) & ~np.isin((g - NL) // kr.TAIL_RANGE, allowed)
    g[move] %= NL
    return g


def only_rows(gid, lo, hi):
    """tier-3 ids kept in rows [lo, hi) alone"""
    g = gid.copy()
    move = g >= NL
    move[lo:hi] = False
    g[move] %= NL
    return g


def range_patterns(rng, n, G, tile_rows):
    """uniform; all tier-3 records in the first range, in the last, in every other one (empty ranges leading, trailing and in
    between); none at all; all of them inside one workgroup-sized block of rows"""
    R = kr.n_ranges_of(G)
    u = ids_uniform(rng, n, G)
    if R > 4:  # with many ranges a uniform draw leaves the first ones nearly empty of rows: half the rows go to tier 3 evenly
        u = np.where(rng.random(n) < 0.5, rng.integers(NL, G, n), u).astype(np.int32)
    mid = (n // tile_rows // 2) * tile_rows
    return {"uniform": u, "first": only_ranges(u, [0]), "last": only_ranges(u, [R - 1]), "alternating": only_ranges(u, np.arange(1, R, 2)),
            "none": only_ranges(u, []), "one block": only_rows(u, mid, mid + tile_rows)}


# ---- 1. tier 2 --------------------------------------------------------------------------------------------------------------
TIER2 = {
    "uniform": lambda rng, n, G: ids_uniform(rng, n, G),
    "sorted": lambda rng, n, G: np.sort(ids_uniform(rng, n, G)),  # long single-key runs: rows4_uniform and its 15-group skip
    "one key >= 4": lambda rng, n, G: np.full(n, G - 1, np.int32),
    "one key < 4": lambda rng, n, G: np.full(n, 2, np.int32),
    "runs of 256": lambda rng, n, G: ids_runs(n, G, 256),
    "runs of 255": lambda rng, n, G: ids_runs(n, G, 255),
}


@pytest.mark.parametrize("pattern", list(TIER2))
@pytest.mark.parametrize("kind", ["big", "small"])
@pytest.mark.parametrize("G", [9, 64, 4099, 4100])
def test_tier2_lds_table(K, G, kind, pattern):
    t = K.table(K.n_of(kind))
    gid = TIER2[pattern](np.random.default_rng(G), t.n, G)
    combos = [(x, y, valid, op) for x in ("f32", "i32") for y in ("f32", "i32") for valid in (True, False) for op in (">", "!=")]
    K.check("1 tier 2", t, G, gid, "none", combos, big=kind == "big")


# ---- 2. direct, one range (four streams) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["big", "small"])
@pytest.mark.parametrize("G", [4101, 12292])
def test_direct_one_range(K, G, kind):
    t = K.table(K.n_of(kind))
    rng = np.random.default_rng(G + 1)
    n, tile = t.n, 8192 if kind == "big" else 2048
    whole = n // tile * tile
    u = ids_uniform(rng, n, G)
    if G == 4101:  # one id of 4101 is tier 3: a uniform draw would leave it a thousand rows
        u[rng.random(n) < 0.3] = 4100
    pats = {"uniform": u, "zipf": ids_zipf(rng, n, G), "all tier 3": rng.integers(NL, G, n).astype(np.int32), "one tier-3 key": np.full(n, G - 1, np.int32),
            "last tile": only_rows(u, whole - tile, whole), "remainder": only_rows(u, whole, n)}
    assert np.any(pats["zipf"] >= NL) and np.any(pats["remainder"][whole:] >= NL) and not np.any(pats["remainder"][:whole] >= NL)
    for name, gid in pats.items():
        K.check("2 direct, one range: " + name, t, G, gid, "direct", COMBOS + MIXED, big=kind == "big")


# ---- 3. chunk rollover ------------------------------------------------------------------------------------------------------
def _craft(rng, n, G, tile, at, k, one_range):
    """exactly k rows of one stream in tile `at` (k None: every row of the table), none of that stream's anywhere else.  Every
    row passes (x = "all"), so rows are records.  Several ranges: the stream is range 1.  One range: the stream is
    (row // 4) % 4 == 1, which a tile has a quarter of its rows of."""
    rows = np.arange(n, dtype=np.int64)
    if one_range:
        mine = (rows // 4) % 4 == 1
        g = ids_uniform(rng, n, G)
        g[mine & (g >= NL)] %= NL
        pick = np.flatnonzero(mine) if k is None else rng.choice(np.flatnonzero(mine[at * tile:(at + 1) * tile]) + at * tile, k, replace=False)
        g[pick] = rng.integers(NL, G, pick.size)
    else:
        lo, hi = NL + kr.TAIL_RANGE, NL + 2 * kr.TAIL_RANGE
        g = ids_uniform(rng, n, G - kr.TAIL_RANGE)
        g[g >= lo] += kr.TAIL_RANGE  # no id of range 1
        pick = rows if k is None else rng.choice(tile, k, replace=False) + at * tile
        g[pick] = rng.integers(lo, hi, pick.size)
    return g


@pytest.mark.parametrize("kind,R", [("big", 3), ("big", 1), ("small", 2), ("small", 1), ("mid", 2)])
def test_chunk_rollover(K, kind, R):
    """K4_CHUNK = 2048 records: a stream that ends at 2047, exactly fills its chunk, opens a second one with one record, fills
    two, opens a third; a tile that is one stream; a table that is one stream (every workgroup rolls over; on the 256-thread
    shape those that get a second tile: N_MID.  With one range a stream has a quarter of a tile's rows, and the 256-thread shape
    never gives a workgroup the five tiles a rollover would take)"""
    t = K.table(K.n_of(kind))
    n, tile = t.n, 8192 if kind == "big" else 2048
    G = kr.groups_of(R) if R > 1 else 12292
    rng = np.random.default_rng(R)
    per_tile = tile if R > 1 else tile // 4  # rows of the stream a tile can hold
    ks = [k for k in (2047, 2048, 2049, 4096, 4097, 8192) if k <= per_tile] or [per_tile - 1, per_tile]
    tiles = n // tile
    combo = ("all", "f32", True, ">")
    for at in (0, tiles // 2, tiles - 1):
        for k in ks:
            gid = _craft(rng, n, G, tile, at, k, R == 1)
            K.check("3 rollover", t, G, gid, "direct", [combo], big=kind == "big")
    gid = _craft(rng, n, G, tile, 0, None, R == 1)
    K.check("3 rollover", t, G, gid, "direct", [combo, ("all", "i32", False, ">")], big=kind == "big")


# ---- 4. direct, several ranges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["big", "small", "small3"])
@pytest.mark.parametrize("which", ["2", "3", "border"])
def test_direct_several_ranges(K, kind, which):
    """R full ranges, one id more (a last range of one id) and one less (of 8191); R = 2, 3, and the most that still goes direct
    with the one-id range added"""
    t = K.table(K.n_of(kind))
    R = K.last_direct(t.n) - 1 if which == "border" else int(which)
    assert R >= 3 or which != "border"
    for G in (kr.groups_of(R), kr.groups_of(R) + 1, kr.groups_of(R) - 1):
        assert kr.n_ranges_of(G) == R + (G == kr.groups_of(R) + 1)
        pats = range_patterns(np.random.default_rng(G), t.n, G, 8192 if kind == "big" else 2048)
        for name in ("uniform", "first", "last", "alternating", "none"):
            K.check("4 direct, several ranges: " + name, t, G, pats[name], "direct", COMBOS if name != "uniform" else COMBOS + MIXED, big=kind == "big")


# ---- 5. the capacity border -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["small", "small3", "big"])
def test_capacity_border(kind):
    """On a fresh Context the first range count past the bound goes scatter and the one below direct; after one launch that
    grew the scratch the same (n, G) goes direct.  All equal the reference."""
    ctx = exon_amd.Context(0)
    try:
        log = set()
        B = Bench(ctx, log)
        n = B.n_of(kind)
        t = Table(ctx, n)
        Rd = B.last_direct(n)
        assert Rd + 1 <= kr.DIRECT_MAX_RANGES
        Gs, Gd = kr.groups_of(Rd + 1, 1), kr.groups_of(Rd)
        pats = range_patterns(np.random.default_rng(n), n, Gs, 2048)
        dg = B.check("5 border", t, Gs, pats["uniform"], "scatter", big=kind == "big")
        B.check("5 border", t, Gd, only_ranges(pats["uniform"], np.arange(Rd)), "direct", big=kind == "big")
        B.check("5 border", t, Gs, pats["uniform"], "scatter", COMBOS[:1], dg=dg)  # the smaller launch did not change the scratch
        # one launch of more rows grows the scratch: four times the rows of this table, its columns repeated
        big_n = 4 * (n // 64 * 64)
        reps = [np.tile(t.h[k][:n // 64 * 64], 4) for k in (("x", "f32"), ("y", "f32"))]
        g4 = np.tile(pats["uniform"][:n // 64 * 64], 4)
        B.route("5 border: the growing launch", big_n, Gs, B.scratch.peek(big_n, Gs).form)
        plan = ctx.plan_cmp_avg_by_group(">", LIT["f32"], Gs)
        st = ctx.zeros(np.int64, 3 * Gs)
        plan.launch([(ctx.to_device(reps[0]), None, None), (ctx.to_device(reps[1]), None, None), (ctx.to_device(g4), None, None)], big_n, st, overwrite=True)
        ctx.sync()
        plan.close()
        same(st.to_host(), Gs, g4, E.keep(reps[0], ">", LIT["f32"]), reps[1], None, ("growing launch", big_n, Gs))
        B.check("5 border", t, Gs, pats["uniform"], "direct", dg=dg, big=kind == "big")
        assert {r[3].split("/")[0] for r in log} >= {"scatter", "direct"}
    finally:
        ctx.close()


# ---- 6. scatter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranges", [129, 192, 193, 384, 385, 768, 769, 1536, 1537, 2047, 2048, "CUs - 1", "CUs", "CUs + 1"])
def test_scatter_small(K, ranges):
    """every border of k4_hist_copies_log2, 129 ranges (the fewest that are never direct), ranges around the CU count (`target`
    of k4_tail_offsets reaches 1) and the most ranges there are (2^24 groups)"""
    R = ranges if isinstance(ranges, int) else max(129, min(2048, K.cus + {"CUs - 1": -1, "CUs": 0, "CUs + 1": 1}[ranges]))
    G = min(kr.groups_of(R), 1 << 24)
    assert kr.n_ranges_of(G) == R
    t = K.table(K.n_of("small"))
    pats = range_patterns(np.random.default_rng(R), t.n, G, 2048)
    for name, gid in pats.items():
        K.check("6 scatter: " + name, t, G, gid, "scatter", COMBOS if G < (1 << 22) else COMBOS[:1] if name != "uniform" else COMBOS, big=False)


@pytest.mark.parametrize("R", [129, 769, 1537])
def test_scatter_big(K, R):
    t = K.table(K.N_BIG)
    G = kr.groups_of(R) - 1
    pats = range_patterns(np.random.default_rng(R), t.n, G, 8192)
    for name, gid in pats.items():
        K.check("6 scatter: " + name, t, G, gid, "scatter", COMBOS, big=True)


# ---- 7. atomic --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [4101, 200_000])
def test_atomic_no_whole_tile(K, G):
    rng = np.random.default_rng(G)
    for n in (2047, 1, 0):
        t = K.table(n)
        gid = np.where(rng.random(n) < 0.5, rng.integers(NL, G, n), ids_uniform(rng, n, G)).astype(np.int32)
        K.check("7 atomic: no whole tile", t, G, gid, "atomic", COMBOS + MIXED)
    t = K.table(1)  # the one row passes and sits in tier 3
    st = K.launch("7 atomic: no whole tile", t, G, t.up(np.array([G - 1], np.int32)), "atomic", ("all", "f32", False, ">")).to_host()
    assert st[G - 1] == 1 and st[2 * G - 1] == 1 and st[3 * G - 1] == np.float64(t.h[("y", "f32")][0]).view(np.int64) and np.count_nonzero(st) <= 3


@pytest.mark.parametrize("kind", ["big", "small"])
def test_atomic_remainder_rows(K, kind):
    """the rows behind the last whole tile carry tier-3 ids that occur nowhere else: only global atomics ever touch those groups"""
    t = K.table(K.n_of(kind))
    tile = 8192 if kind == "big" else 2048
    whole = t.n // tile * tile
    rng = np.random.default_rng(whole)
    for G, want in ((12292, "direct"), (kr.groups_of(129), "scatter")):
        gid = ids_uniform(rng, t.n, G - 64)
        gid[whole:] = rng.integers(G - 64, G, t.n - whole)
        K.check("7 atomic: remainder rows", t, G, gid, want, big=kind == "big")


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import exon_amd
d = np.load(sys.argv[2])
ctx = exon_amd.Context(0)
out = {"cus": np.array([ctx.info()["compute_units"]])}
cols = [(ctx.to_device(d["x"]), ctx.to_device(d["xok"]), None), (ctx.to_device(d["y"]), ctx.to_device(d["yok"]), None)]
for G in (5000, 200000):
    plan = ctx.plan_cmp_avg_by_group(">", 0.25, G)
    st = ctx.zeros(np.int64, 3 * G)
    plan.launch(cols + [(ctx.to_device(d["g%d" % G]), None, None)], int(d["n"]), st, overwrite=True)
    ctx.sync()
    plan.close()
    out["s%d" % G] = st.to_host()
np.savez(sys.argv[3], **out)
ctx.close()
"""


def test_atomic_grid_beyond_histogram_rows(K, tmp_path):
    """9 workgroups per CU: more workgroups than the partition has histogram rows for (2048), every tier-3 row takes global
    atomics.  The setting is read when a Context is made, so a child process makes one."""
    if K.cus * 9 <= kr.TAIL_MAX_GRID:
        pytest.fail("this device has %d CUs: 9 workgroups per CU do not exceed %d" % (K.cus, kr.TAIL_MAX_GRID))
    t = K.table(K.n_of("small"))
    rng = np.random.default_rng(9)
    gids = {G: np.where(rng.random(t.n) < 0.5, rng.integers(NL, G, t.n), ids_uniform(rng, t.n, G)).astype(np.int32) for G in (5000, 200_000)}
    pad = lambda a: np.concatenate([a, np.zeros(64, a.dtype)])  # noqa: E731
    np.savez(tmp_path / "in.npz", n=t.n, x=pad(t.h[("x", "f32")]), y=pad(t.h[("y", "f32")]), xok=pad(E.bits(t.xok)), yok=pad(E.bits(t.yok)),
             g5000=pad(gids[5000]), g200000=pad(gids[200_000]))
    child = kr.Scratch(K.cus, 9)
    for G in gids:
        assert child.launch(t.n, G).form == "atomic"
        K.log.add(("7 atomic: 9 workgroups per CU", t.n, G, "atomic/%d" % kr.n_ranges_of(G), "256"))
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=dict(os.environ, EXON_HIP_BLOCKS_PER_CU="9"),
                       timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    out = np.load(tmp_path / "out.npz")
    assert int(out["cus"][0]) == K.cus
    for G, gid in gids.items():
        same(out["s%d" % G], G, gid, t.keep("f32", ">", True), t.h[("y", "f32")], t.yok, ("child", G))


# ---- 8 - 10: state handling, poison, ids out of range: on the direct and on the scatter route --------------------------------
ROUTES = [("direct", "big"), ("direct", "small"), ("scatter", "big"), ("scatter", "small")]


def _route_case(K, want, kind):
    t = K.table(K.n_of(kind))
    G = kr.groups_of(3) - 5 if want == "direct" else kr.groups_of(129) + 1
    key = ("gid", G)
    if key not in t.h:
        rng = np.random.default_rng(G)
        t.h[key] = np.where(rng.random(t.n) < 0.5, rng.integers(NL, G, t.n), ids_uniform(rng, t.n, G)).astype(np.int32)
        t.d[key] = t.up(t.h[key])
    return t, G, t.h[key], t.d[key]


@pytest.mark.parametrize("want,kind", ROUTES)
def test_state_with_a_tail(K, want, kind):
    t, G, gid, dg = _route_case(K, want, kind)
    cnn, crow, sums = E.expect(gid, G, t.keep("f32", ">", True), t.h[("y", "f32")], t.yok)
    ref = E.state_words(cnn, crow, sums)
    # overwrite into junk: tier 3 adds to the state, so the launch has to clear it first
    st = K.ctx.to_device(np.full(3 * G, JUNK, np.int64))
    assert np.array_equal(K.launch("8 state", t, G, dg, want, state=st).to_host(), ref)
    # accumulate twice into zeros: twice the reference (2 * sum is exact)
    st = K.ctx.zeros(np.int64, 3 * G)
    for _ in range(2):
        K.launch("8 state", t, G, dg, want, state=st, overwrite=False)
    assert np.array_equal(st.to_host(), E.state_words(2 * cnn, 2 * crow, 2 * sums))
    # two halves, split on a bitmap byte and a 16-byte boundary, accumulate to the whole
    h = t.n // 2 // 64 * 64
    st = K.ctx.zeros(np.int64, 3 * G)
    for lo, m in ((0, h), (h, t.n - h)):
        K.launch("8 state: halves", t, G, dg, want, n=m, lo=lo, state=st, overwrite=False)
    assert np.array_equal(st.to_host(), ref)


@pytest.mark.parametrize("want,kind", ROUTES)
def test_poison_and_nulls_with_a_tail(K, want, kind):
    t, G, gid, dg = _route_case(K, want, kind)
    kept = t.keep("f32", ">", True)
    live = kept & t.yok
    yf = t.h[("y", "f32")]
    if "poison" not in t.h:
        y = yf.copy()
        dead = np.flatnonzero(~live)
        y[dead] = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)[np.arange(dead.size) % 4]
        t.h["poison"], t.d["poison"] = y, t.up(y)
    got = K.launch("9 poison", t, G, dg, want, y=t.d["poison"]).to_host()
    assert np.all(np.isfinite(got[2 * G:].view(np.float64)))
    same(got, G, gid, kept, yf, t.yok, ("poison", want, kind))
    # one passing NaN in a tier-3 group: exactly that sum is NaN
    at = int(np.flatnonzero(live & (gid >= NL))[3])
    y = t.h["poison"].copy()
    y[at] = np.nan
    got = K.launch("9 poison", t, G, dg, want, y=t.up(y)).to_host()
    cnn, crow, sums = E.expect(gid, G, kept, np.where(np.arange(t.n) == at, np.float32(np.nan), yf), t.yok)
    s = got[2 * G:].view(np.float64)
    assert np.array_equal(got[:G], cnn) and np.array_equal(got[G:2 * G], crow)
    assert np.isnan(s[gid[at]]) and np.isnan(s).sum() == 1 and np.array_equal(s, sums, equal_nan=True)
    keep_rest = np.arange(G) != gid[at]
    assert np.array_equal(got[2 * G:][keep_rest], sums.view(np.int64)[keep_rest])
    # every y NULL
    nulls = K.ctx.zeros(np.uint8, t.n // 8 + 64)
    got = K.launch("9 nulls", t, G, dg, want, yv=nulls).to_host()
    assert not got[:G].any() and not got[2 * G:].any()
    assert np.array_equal(got[G:2 * G], np.bincount(gid[kept], minlength=G))


@pytest.mark.parametrize("want,kind", ROUTES)
def test_ids_out_of_range_with_a_tail(K, want, kind):
    """a reported input error the kernel contains: the sync after it raises, the next launch on the same context is exact"""
    t, G, gid, dg = _route_case(K, want, kind)
    kept = t.keep("f32", ">", True)
    rows = np.flatnonzero(kept & t.yok)
    for bad in (G, G + 100_000, -1):
        g = gid.copy()
        g[rows[[0, rows.size // 2, -1]]] = bad  # the first tile, a middle one, the remainder
        db = t.up(g)
        with pytest.raises(exon_amd.ExonHipError, match="group id out of range"):
            K.launch("10 ids out of range", t, G, db, want)
        got = K.launch("10 ids out of range", t, G, dg, want).to_host()
        same(got, G, gid, kept, t.h[("y", "f32")], t.yok, ("after", bad, want, kind))
