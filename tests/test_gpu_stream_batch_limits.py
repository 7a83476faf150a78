"""GPU: Arrow batch ingestion of the stream layer (exon_hip_stream_push / _push_device) at its limits, word for word (==) against
tests/stream_batches_expect.py.

A parent table of N rows is cut into batches by a CUT LIST of (parent offset, rows, bitmap mode per column); the batches are pushed,
finish() is compared with the statement over the concatenated rows.  Batches are zero-copy pyarrow arrays over the parent's buffers
(pa.Array.from_buffers with an offset: a slice), or hand-built ArrowArray structs (ctypes) with a release callback that counts its
calls where pyarrow cannot express the case: null_count == -1, an all-ones bitmap beside null_count == 0 (pyarrow exports the
count it computed, and no validity buffer when that is 0), a struct-level offset, children without buffers, malformed batches.

  1  host batches: bit residues, one-row batches, a bitmap that comes and goes, slot boundaries, the hold limit, a struct-level
     offset, Utf8 slices, reset() with staged rows
  2  the slot's tail on the device: rows and validity bits past n that would pass, by direct launches and through a recycled slot
  3  refusals and ownership: the error code, the state of the rows accepted before, every release callback exactly once
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L

import stream_batches_expect as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, ESTATE = -1, -4, -5
HOLD_MAX_ROWS = 131072

# bitmap modes of one column of one batch
NONE, NULLS, ONES, UNKNOWN = "none", "nulls", "ones", "unknown"  # no buffer / NULLs, exact null_count / all ones, null_count 0 / NULLs, null_count -1
LENGTHS = [1, 2, 3, 5, 7, 9, 61, 63, 64, 65, 127, 129, 8191, 8193]


# ---- the plan kinds ---------------------------------------------------------------------------------------------------------------
class U8:
    """a Utf8 column: int32 offsets [n + 1] and the bytes"""

    def __init__(self, lens, data):
        self.off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        self.data = np.ascontiguousarray(data, np.uint8)
        assert self.off[-1] == len(self.data)

    def __len__(self):
        return len(self.off) - 1

    def rows(self, idx):
        raw, o = self.data.tobytes(), self.off
        return [raw[o[i]:o[i + 1]] for i in idx]

    @staticmethod
    def random(rng, n, lo, hi, alphabet=None):
        lens = rng.integers(lo, hi + 1, n)
        if n:
            lens[rng.integers(0, n, max(1, n // 16))] = 0  # empty strings everywhere
        tot = int(lens.sum())
        data = rng.integers(33, 75, tot, dtype=np.uint8) if alphabet is None else np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), tot)]
        return U8(lens, data)


def _gen_k2(rng, n):
    return [rng.integers(0, 4, n).astype(np.int32), rng.integers(1, 1000, n).astype(np.int64)]


def _gen_k6(rng, n):
    start = rng.integers(1, 5000, n).astype(np.int64)
    return [rng.integers(0, 3, n).astype(np.int32), start, start + rng.integers(0, 300, n)]


def _gen_k3(rng, n):
    return [rng.choice(np.array([0, 4, 16, 99, 147, 256, 1024, 1028, 1284, 2048], np.int32), n), rng.integers(0, 61, n).astype(np.uint8),
            rng.integers(0, 25, n).astype(np.int32)]


def _gen_k4f(rng, n):  # y from eighths: the f64 sums are exact in any order
    return [rng.choice(np.array([0.0, 0.01, 0.25, 0.5, 1.0, -1.0], np.float32), n), (rng.integers(0, 8000, n) / 8.0).astype(np.float32),
            rng.integers(0, 5, n).astype(np.int32)]


def _gen_k4i(rng, n):
    return [rng.integers(-3, 4, n).astype(np.int32), rng.integers(0, 100_000, n).astype(np.int32), rng.integers(0, 9, n).astype(np.int32)]


def _gen_k8(rng, n):
    return [rng.choice(np.array([0.0, 0.01, 0.25, 0.5, 1.0, -1.0], np.float32), n), (rng.integers(-8000, 8000, n) / 8.0).astype(np.float32),
            rng.integers(0, 7, n).astype(np.int32)]


def _gen_k5(rng, n):
    return [U8.random(rng, n, 0, 24)]


def _gen_k9(rng, n):  # the two payloads differ in size
    return [U8.random(rng, n, 0, 40, b"ACGTNacgt"), U8.random(rng, n, 0, 17)]


def _const(dtype, v):
    return lambda m: np.full(m, v, dtype)


class Spec:
    def __init__(self, kind, params, plan, gen, types, nullable, passing):
        self.kind, self.params, self.plan, self.gen, self.types, self.nullable, self.passing = kind, params, plan, gen, types, nullable, passing
        self.n_cols = len(types)


# `passing`: per column, m rows that pass the predicate (group ids valid) -- what sits BEHIND a column in the tail tests
SPECS = {
    "k2": Spec("k2", (2, 100, 600), lambda ctx: ctx.plan_region_count(2, 100, 600, columns=(0, 1)), _gen_k2, ["i32", "i64"], [True, True],
               [_const(np.int32, 2), _const(np.int64, 100)]),
    "k6": Spec("k6", (1, 1000, 3000), lambda ctx: ctx.plan_overlap_count(1, 1000, 3000, columns=(0, 1, 2)), _gen_k6, ["i32", "i64", "i64"], [True] * 3,
               [_const(np.int32, 1), _const(np.int64, 1000), _const(np.int64, 1000)]),
    "k7": Spec("k7", (1, 1000, 3000), lambda ctx: ctx.plan_within_count(1, 1000, 3000, columns=(0, 1, 2)), _gen_k6, ["i32", "i64", "i64"], [True] * 3,
               [_const(np.int32, 1), _const(np.int64, 1001), _const(np.int64, 2999)]),
    "k3": Spec("k3", (1284, 0, 30, 25), lambda ctx: ctx.plan_flag_mapq_group_count(1284, 0, 30, 25), _gen_k3, ["i32", "u8", "i32"], [True] * 3,
               [_const(np.int32, 0), _const(np.uint8, 60), _const(np.int32, 3)]),
    "k4f": Spec("k4", (">", 0.01, 5, False, False), lambda ctx: ctx.plan_cmp_avg_by_group(">", 0.01, 5), _gen_k4f, ["f32", "f32", "i32"], [True, True, False],
                [_const(np.float32, 1.0), _const(np.float32, 2.5), _const(np.int32, 4)]),
    "k4i": Spec("k4", (">=", 1.0, 9, True, True), lambda ctx: ctx.plan_cmp_avg_by_group(">=", 1.0, 9, x_type="i32", y_type="i32"), _gen_k4i,
                ["i32", "i32", "i32"], [True, True, False], [_const(np.int32, 1), _const(np.int32, 7), _const(np.int32, 8)]),
    "k8": Spec("k8", ("<=", 0.25, 7, False, False), lambda ctx: ctx.plan_cmp_minmax_by_group("<=", 0.25, 7), _gen_k8, ["f32", "f32", "i32"], [True, True, False],
               [_const(np.float32, 0.0), _const(np.float32, 4096.0), _const(np.int32, 6)]),
    "k5": Spec("k5", (24,), lambda ctx: ctx.plan_qual_pos_hist(24), _gen_k5, ["utf8"], [False], [lambda m: U8(np.full(m, 3), np.full(3 * m, 70, np.uint8))]),
    "k9": Spec("k9", (40,), lambda ctx: ctx.plan_read_stats_hist(40), _gen_k9, ["utf8", "utf8"], [False, False],
               [lambda m: U8(np.full(m, 3), np.full(3 * m, 71, np.uint8)), lambda m: U8(np.full(m, 2), np.full(2 * m, 72, np.uint8))]),
}
KINDS = list(SPECS)
FIXED_KINDS = [k for k in KINDS if "utf8" not in SPECS[k].types]
UTF8_KINDS = ["k5", "k9"]


def fit(kind, modes):
    """a cut's modes for this kind: one per column, and no NULLs where the plan takes none (group keys, FASTQ lines) -- such a
    column carries the all-ones bitmap instead"""
    spec = SPECS[kind]
    modes = [modes] * spec.n_cols if isinstance(modes, str) else list(modes)[:spec.n_cols] + [modes[-1]] * (spec.n_cols - len(modes))
    return tuple(m if spec.nullable[c] or m in (NONE, ONES) else ONES for c, m in enumerate(modes))


class Table:
    """the parent: values and boolean validity per column; rows covered by a cut whose mode has no NULLs are valid"""

    def __init__(self, kind, n, cuts=(), seed=1, p_valid=0.5):
        self.kind, self.spec, self.n = kind, SPECS[kind], n
        rng = np.random.default_rng([seed, n, KINDS.index(kind)])
        self.values = self.spec.gen(rng, n)
        self.valid = [(rng.random(n) < p_valid) if nb else np.ones(n, bool) for nb in self.spec.nullable]
        for lo, rows, modes in cuts:
            assert 0 <= lo and lo + rows <= n
            for c, m in enumerate(fit(kind, modes)):
                if m in (NONE, ONES):
                    self.valid[c][lo:lo + rows] = True
        self.seal()

    def seal(self):
        pad = np.zeros(8, np.uint8)
        self.bitmaps = [np.concatenate([np.packbits(v, bitorder="little"), pad]) for v in self.valid]
        self.ones = np.full(self.n // 8 + 16, 0xFF, np.uint8)
        self._rows = {}

    def statement_cols(self, idx):
        out = []
        for c, (v, ok) in enumerate(zip(self.values, self.valid)):
            if isinstance(v, U8):
                if c not in self._rows:
                    self._rows[c] = v.rows(range(self.n))
                out.append(([self._rows[c][i] for i in idx], ok[idx]))
            else:
                out.append((v[idx], ok[idx]))
        return out

    def want(self, cuts):
        idx = np.concatenate([np.arange(lo, lo + rows) for lo, rows, _ in cuts] + [np.zeros(0, np.int64)]).astype(np.int64)
        return S.expect(self.spec.kind, self.spec.params, self.statement_cols(idx))

    def batch(self, lo, rows, modes):
        """rows [lo, lo + rows) as a pyarrow RecordBatch over the parent's own buffers: every child has offset lo.  (pyarrow counts
        the NULLs when it exports an array and drops the validity buffer of one that has none: null_count == -1 and the all-ones
        bitmap are hand() 's)"""
        import pyarrow as pa
        arrays = []
        for c, m in enumerate(fit(self.kind, modes)):
            assert m in (NONE, NULLS)
            vbuf, nc = None, 0
            if m == NULLS:
                vbuf, nc = pa.py_buffer(self.bitmaps[c]), int(rows - self.valid[c][lo:lo + rows].sum())
            v = self.values[c]
            if isinstance(v, U8):
                arrays.append(pa.Array.from_buffers(pa.binary(), rows, [vbuf, pa.py_buffer(v.off), pa.py_buffer(v.data)], nc, lo))
            else:
                arrays.append(pa.Array.from_buffers(pa.from_numpy_dtype(v.dtype), rows, [vbuf, pa.py_buffer(v)], nc, lo))
        return pa.RecordBatch.from_arrays(arrays, [f"c{c}" for c in range(len(arrays))])

    def hand(self, lo, rows, modes):
        """the same slice as a hand-built struct: children of offset lo over the parent's buffers, null_count -1 where the mode says so"""
        children = []
        for c, m in enumerate(fit(self.kind, modes)):
            bitmap = {NONE: None, ONES: self.ones}.get(m, self.bitmaps[c])
            nc = {NONE: 0, ONES: 0, UNKNOWN: -1, NULLS: int(rows - self.valid[c][lo:lo + rows].sum())}[m]
            v = self.values[c]
            children.append({"length": rows, "offset": lo, "null_count": nc, "buffers": [bitmap, v.off, v.data] if isinstance(v, U8) else [bitmap, v]})
        return Hand(rows, children)

    def push(self, st, cut, hands):
        """a cut into the stream: a pyarrow slice where pyarrow can express it, a hand-built struct (kept in `hands`) otherwise"""
        if set(fit(self.kind, cut[2])) & {UNKNOWN, ONES}:
            hands.append(self.hand(*cut))
            assert hands[-1].push(st) == 0 and not hands[-1].arr.release
        else:
            st.push(self.batch(*cut))

    def carries_bitmap(self, c, lo, rows, modes):
        """what the library sees: a validity buffer AND a null_count that is not 0"""
        m = fit(self.kind, modes)[c]
        return rows > 0 and (m == UNKNOWN or (m == NULLS and not self.valid[c][lo:lo + rows].all()))


def same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:8]
    assert np.array_equal(got[1], want[1])


def released_once(hands):
    return all(h.released == 1 and h.child_released == 0 and not h.arr.release for h in hands)


def run_cuts(ctx, table, cuts):
    plan = table.spec.plan(ctx)
    st = plan.open()
    hands = []
    try:
        for cut in cuts:
            table.push(st, cut, hands)
        got = st.finish()
    finally:
        st.close()
        plan.close()
    assert released_once(hands)
    return got


def chain(lengths, modes, start=0, residues=None):
    """a cut list of consecutive batches; residues[i] (optional): the parent offset of batch i mod 8 (a gap of up to 7 rows)"""
    cuts, lo = [], start
    for i, rows in enumerate(lengths):
        if residues is not None and residues[i] is not None:
            lo += (residues[i] - lo) % 8
        cuts.append((lo, rows, modes[i] if isinstance(modes, list) else modes))
        lo += rows
    return cuts


def end_of(cuts):
    return max(lo + rows for lo, rows, _ in cuts)


# ---- hand-built ArrowArray structs ------------------------------------------------------------------------------------------------
RELEASE_T = C.CFUNCTYPE(None, C.POINTER(L.ArrowArray))


class Hand:
    """A struct ArrowArray built field by field.  children: dicts of length / offset / null_count / buffers (numpy arrays or None) /
    n_buffers / n_children.  .released counts the parent's release callback; a child's callback must never run (the consumer
    releases the parent only).  The object keeps every buffer alive: keep IT alive until .released == 1."""

    def __init__(self, length, children, offset=0, n_children=None):
        self.released, self.child_released = 0, 0
        self._keep = []

        def rel(p):
            self.released += 1
            p.contents.release = None

        def crel(p):
            self.child_released += 1

        self._cb, self._ccb = RELEASE_T(rel), RELEASE_T(crel)
        self.kids = (C.POINTER(L.ArrowArray) * max(1, len(children)))()
        for i, ch in enumerate(children):
            a = L.ArrowArray()
            bufs = ch.get("buffers", [])
            tb = (C.c_void_p * max(1, len(bufs)))(*[None if b is None else (b if isinstance(b, int) else b.ctypes.data) for b in bufs])
            a.length, a.null_count, a.offset = ch["length"], ch.get("null_count", 0), ch.get("offset", 0)
            a.n_buffers, a.n_children = ch.get("n_buffers", len(bufs)), ch.get("n_children", 0)
            a.buffers = C.cast(tb, C.POINTER(C.c_void_p))
            a.release = C.cast(self._ccb, C.c_void_p).value
            self._keep += [a, tb, bufs]
            self.kids[i] = C.pointer(a)
        self.arr = L.ArrowArray()
        self._tb = (C.c_void_p * 1)(None)
        self.arr.length, self.arr.null_count, self.arr.offset = length, 0, offset
        self.arr.n_buffers, self.arr.buffers = 1, C.cast(self._tb, C.POINTER(C.c_void_p))
        self.arr.n_children = len(children) if n_children is None else n_children
        self.arr.children = C.cast(self.kids, C.POINTER(C.POINTER(L.ArrowArray)))
        self.arr.release = C.cast(self._cb, C.c_void_p).value

    def push(self, st):
        """the raw return code of exon_hip_stream_push"""
        return st.ctx.lib.exon_hip_stream_push(st.h, C.byref(self.arr))


def hand_children(table, lo, rows, modes, batch_offset=0, child_offsets=None, junk_seed=7):
    """children for rows [lo, lo + rows) of the table under a struct of offset `batch_offset`: child c has its own offset
    child_offsets[c] and the length that just suffices (batch_offset + rows); the rows in front of the batch's (child offset +
    batch offset of them) are junk that would pass the predicate, with NULLs at random"""
    spec = table.spec
    child_offsets = child_offsets or [0] * spec.n_cols
    rng = np.random.default_rng(junk_seed)
    out = []
    for c, m in enumerate(fit(table.kind, modes)):
        lead = child_offsets[c] + batch_offset
        ok = np.concatenate([rng.random(lead) < 0.5, table.valid[c][lo:lo + rows]])
        if m == ONES:
            ok[:] = True
        bitmap = None if m == NONE else np.packbits(ok, bitorder="little")
        nc = {NONE: 0, ONES: 0, UNKNOWN: -1, NULLS: int((~ok[lead:]).sum())}[m]
        v = table.values[c]
        junk = spec.passing[c](lead)
        if isinstance(v, U8):
            o, o2 = v.off, junk.off
            data = np.concatenate([junk.data, v.data[o[lo]:o[lo + rows]], np.zeros(1, np.uint8)])
            off = np.concatenate([o2, o2[-1] + (o[lo + 1:lo + rows + 1] - o[lo])]).astype(np.int32)
            bufs = [bitmap, off, data]
        else:
            bufs = [bitmap, np.concatenate([junk, v[lo:lo + rows]])]
        out.append({"length": batch_offset + rows, "offset": child_offsets[c], "null_count": nc, "buffers": bufs})
    return out


def empty_hand(n_cols, types):
    """a zero-row batch whose children have NO buffers at all (NULL pointers)"""
    return Hand(0, [{"length": 0, "buffers": [None] * (3 if t == "utf8" else 2)} for t in types[:n_cols]])


# ---- 1. host batches --------------------------------------------------------------------------------------------------------------
def residue_cuts(kind):
    """LENGTHS in cycles until, among the batches that carry a bitmap, every (source bit offset mod 8, destination row mod 8) pair
    has occurred; a batch's source residue is chosen to be the first one its destination residue still lacks"""
    rng = np.random.default_rng(11)
    need = {(s, d) for s in range(8) for d in range(8)}
    cuts, lo, pushed, i = [], 0, 0, 0
    while need or i < 3 * len(LENGTHS):
        rows = LENGTHS[(i + i // len(LENGTHS)) % len(LENGTHS)]  # (a cycle is 16920 = 0 (mod 8) rows: each one starts a length later, or the destination residues would repeat)
        if i % 7 == 3:
            mode = NONE
        elif i % 7 == 5:
            mode = ONES
        else:
            mode = UNKNOWN if (rows < 61 or i % 2) else NULLS
        d = pushed % 8
        s = next((s for s in range(8) if (s, d) in need), int(rng.integers(0, 8)))
        lo += (s - lo) % 8
        if mode in (NULLS, UNKNOWN):
            need.discard((s, d))
        if i % 10 == 4:
            cuts.append((lo, 0, mode))  # a zero-row batch in between (buffers present)
        cuts.append((lo, rows, mode))
        lo, pushed, i = lo + rows, pushed + rows, i + 1
        assert lo <= 400_000
    return cuts


def pairs_of(table, cuts, c):
    pairs, pushed = set(), 0
    for lo, rows, modes in cuts:
        if table.carries_bitmap(c, lo, rows, modes):
            pairs.add((lo % 8, pushed % 8))
        pushed += rows
    return pairs


@pytest.mark.parametrize("kind", KINDS)
def test_bit_residues(ctx, kind):
    cuts = residue_cuts(kind)
    table = Table(kind, end_of(cuts), cuts)
    spec = table.spec
    for c in range(spec.n_cols):  # a condition on the INPUT: every residue pair is there, in every column that can hold NULLs
        if spec.nullable[c]:
            assert len(pairs_of(table, cuts, c)) == 64
    assert {rows for _, rows, _ in cuts} == set(LENGTHS) | {0}
    want = table.want(cuts)
    plan = spec.plan(ctx)
    st = plan.open()
    hands = []
    empties = 0
    for cut in cuts:
        table.push(st, cut, hands)
        if cut[1] == 0:  # ... and a zero-row batch without buffers
            hands.append(empty_hand(spec.n_cols, spec.types))
            assert hands[-1].push(st) == 0
            empties += 1
    got = st.finish()
    st.close()
    plan.close()
    same(got, want)
    assert empties and released_once(hands)


@pytest.mark.parametrize("kind", KINDS)
def test_300_batches_of_one_row(ctx, kind):
    cuts = chain([1] * 300, [UNKNOWN if i % 3 else NULLS for i in range(300)], start=5)
    table = Table(kind, end_of(cuts), cuts)
    same(run_cuts(ctx, table, cuts), table.want(cuts))


@pytest.mark.parametrize("kind", KINDS)
def test_bitmap_comes_and_goes(ctx, kind):
    """no validity buffer for 99 rows, then NULLs from destination row 99 = 3 (mod 8), then 101 rows without a buffer from row
    182 = 6 (mod 8): two head bits, twelve whole bytes, three tail bits; and once more.  One column at a time carries the bitmap."""
    spec = SPECS[kind]
    lengths = [8, 64, 27, 13, 70, 101, 5, 9, 1000, 3, 8]
    with_nulls = [False, False, False, True, True, False, False, True, False, True, False]
    for k in range(spec.n_cols):
        on = UNKNOWN if k % 2 else NULLS
        modes = [tuple((on if w else NONE) if c == k else NONE for c in range(spec.n_cols)) for w in with_nulls]
        cuts = chain(lengths, modes, start=2 + k, residues=[None, None, None, 5, None, None, 1, 2, None, 7, None])
        table = Table(kind, end_of(cuts), cuts, seed=20 + k)
        if spec.nullable[k]:
            for (lo, rows, _), w in zip(cuts, with_nulls):
                if w:
                    table.valid[k][lo + rows // 2] = False  # (at least one NULL: a batch of 3 rows has none once in eight)
            table.seal()
        assert sum(r for _, r, _ in cuts[:3]) % 8 == 3 and sum(r for _, r, _ in cuts[:5]) % 8 == 6
        if spec.nullable[k]:
            assert [table.carries_bitmap(k, *cut) for cut in cuts] == with_nulls
        same(run_cuts(ctx, table, cuts), table.want(cuts))


def boundary_cuts():
    """against slots of 1000 rows: 333 + 334 + 333 fill one exactly; 7 + 500 + 493 the next, then one row more; 998 make 999, then 2;
    2 rows are staged when one batch of 1001 re-allocates the slots, 3 when one of 5000 does; small batches afterwards.  Every
    batch has NULLs (where its column may), the parent offsets run from 3 with gaps, so no boundary is a multiple of 8 there."""
    lengths = [333, 334, 333, 7, 500, 493, 1, 998, 2, 1001, 3, 5000] + [LENGTHS[i % 12] for i in range(60)] + [4990, 11, 5000, 1]
    modes = [UNKNOWN if i % 2 else NULLS for i in range(len(lengths))]
    return chain(lengths, modes, start=3, residues=[3, None, None, 1, None, None, 7, None, 5, 2, None, 6] + [None] * (len(lengths) - 12))


@pytest.mark.parametrize("kind", KINDS)
def test_slot_boundaries(ctx, kind, monkeypatch):
    monkeypatch.setenv("EXON_HIP_COALESCE_ROWS", "1000")  # read when the slots are allocated: run_cuts opens a fresh stream
    cuts = boundary_cuts()
    table = Table(kind, end_of(cuts), cuts, seed=3)
    ends = np.cumsum([r for _, r, _ in cuts])
    assert ends[2] == 1000 and ends[5] == 2000 and ends[6] == 2001 and ends[7] == 2999
    assert all(cuts[i][0] % 8 for i in (0, 3, 6, 8, 9, 11))  # the first batch behind every boundary starts inside a byte of its parent bitmap
    same(run_cuts(ctx, table, cuts), table.want(cuts))


def hold_cuts(first_bitmap_in):
    """3 rows, 131072 (the largest batch that is held), 131073 (copied at once), 5; the bitmap is first seen in batch 1 or 2"""
    lengths = [3, HOLD_MAX_ROWS, HOLD_MAX_ROWS + 1, 5]
    modes = [NONE if i < first_bitmap_in else (NULLS if i % 2 else UNKNOWN) for i in range(4)]
    return chain(lengths, modes, start=1, residues=[None, 5, 2, None])


@functools.lru_cache(maxsize=None)
def hold_case(kind, first_bitmap_in):
    """(table, cuts, expected state): computed once, shared by the run with holding and the one without"""
    cuts = hold_cuts(first_bitmap_in)
    table = Table(kind, end_of(cuts), cuts, seed=4)
    return table, cuts, table.want(cuts)


@pytest.mark.parametrize("first_bitmap_in", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_hold_limit(ctx, kind, first_bitmap_in):
    table, cuts, want = hold_case(kind, first_bitmap_in)
    same(run_cuts(ctx, table, cuts), want)


CHILD = """
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import exon_amd
import test_gpu_stream_batch_limits as T
ctx = exon_amd.Context(0)
out = {{}}
for kind in T.FIXED_KINDS:
    for first in (1, 2):
        table, cuts, _ = T.hold_case(kind, first)
        counts, sums = T.run_cuts(ctx, table, cuts)
        out[kind + str(first)] = [counts.tolist(), [x.hex() for x in sums.tolist()]]
ctx.close()
print("STATES " + json.dumps(out))
"""


def test_hold_limit_with_holding_switched_off(tmp_path):
    """EXON_HIP_HOLD_SMALL_BATCHES is read once per process: the same cut lists in one fresh child process, which prints its states
    (the fixed-width kinds: a batch with a Utf8 column is never held)"""
    script = tmp_path / "hold_off_child.py"
    script.write_text(CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    env = dict(os.environ, EXON_HIP_HOLD_SMALL_BATCHES="0")
    r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    line = [ln for ln in r.stdout.decode().split("\n") if ln.startswith("STATES ")]
    assert len(line) == 1
    states = json.loads(line[0][7:])
    assert sorted(states) == sorted(k + str(f) for k in FIXED_KINDS for f in (1, 2))
    for kind in FIXED_KINDS:
        for first in (1, 2):
            want = hold_case(kind, first)[2]
            counts, sums = states[kind + str(first)]
            same((np.array(counts, np.int64), np.array([float.fromhex(x) for x in sums], np.float64)), want)


@pytest.mark.parametrize("kind", KINDS)
def test_struct_offset(ctx, kind):
    """batch->offset = 5 over children with their own offsets 0, 3 and 8, each of the length that just suffices: the same state as
    the same rows pushed as a plain slice"""
    spec = SPECS[kind]
    cuts = chain([40, 777, 9], [NULLS, UNKNOWN, NONE], start=3)
    table = Table(kind, end_of(cuts), cuts, seed=5)
    want = table.want(cuts)
    same(run_cuts(ctx, table, cuts), want)
    plan = spec.plan(ctx)
    st = plan.open()
    hands = [Hand(rows, hand_children(table, lo, rows, modes, batch_offset=5, child_offsets=[0, 3, 8][:spec.n_cols]), offset=5) for lo, rows, modes in cuts]
    for h in hands:
        assert h.arr.offset == 5 and [k.contents.offset for k in h.kids[:spec.n_cols]] == [0, 3, 8][:spec.n_cols]
        assert all(k.contents.length == 5 + h.arr.length for k in h.kids[:spec.n_cols])
        assert h.push(st) == 0 and not h.arr.release
    got = st.finish()
    st.close()
    plan.close()
    same(got, want)
    assert released_once(hands)


@pytest.mark.parametrize("kind", UTF8_KINDS)
def test_utf8_batches(ctx, kind, monkeypatch):
    """slices whose first offset is not 0, empty strings at either end of a batch, batches of empty strings only, and slot boundaries"""
    monkeypatch.setenv("EXON_HIP_COALESCE_ROWS", "1000")
    cuts = chain([10, 1, 64, 333, 592, 1, 999, 2, 1001, 17, 3000], NONE, start=7) + [(0, 7, ONES)]
    table = Table(kind, end_of(cuts), seed=6)
    for v in table.values:  # empty strings: first and last row of some batches, batches 1, 5 and 9 as a whole
        lens = np.diff(v.off)
        for b, (lo, rows, _) in enumerate(cuts):
            if b in (1, 5, 9):
                lens[lo:lo + rows] = 0
            elif b % 2 == 0:
                lens[lo] = lens[lo + rows - 1] = 0
        keep = np.repeat(np.arange(table.n), lens)  # (the bytes of the rows' shortened lengths, taken from the front of each)
        data = v.data[(v.off[:-1][keep] + (np.arange(len(keep)) - np.repeat(np.cumsum(lens) - lens, lens)))] if len(keep) else v.data[:0]
        v.off, v.data = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.ascontiguousarray(data)
    table.seal()
    assert all(v.off[cuts[0][0]] > 0 for v in table.values)
    if kind == "k9":
        assert table.values[0].off[-1] != table.values[1].off[-1]
    same(run_cuts(ctx, table, cuts), table.want(cuts))


@pytest.mark.parametrize("kind", KINDS)
def test_reset_with_staged_rows(ctx, kind):
    """batches with NULLs up to an odd row, reset(), a batch WITHOUT any bitmap, then one with: the second query's state must not see
    the first one's bits"""
    first = chain([8193, 77, 5], [NULLS, UNKNOWN, NULLS], start=1)
    second = chain([9000, 123], [NONE, UNKNOWN], start=end_of(first) + 4)
    table = Table(kind, end_of(second), first + second, seed=8, p_valid=0.3)
    assert sum(r for _, r, _ in first) % 2 == 1
    plan = table.spec.plan(ctx)
    st = plan.open()
    hands = []
    for cut in first:
        table.push(st, cut, hands)
    st.reset()
    assert released_once(hands)  # held for the abandoned query: released uncopied
    for cut in second:
        table.push(st, cut, hands)
    got = st.finish()
    st.close()
    plan.close()
    same(got, table.want(second))
    assert released_once(hands)


# ---- 2. the slot's tail on the device ---------------------------------------------------------------------------------------------
TAIL = 512
TAIL_N = [1, 7, 8, 9, 63, 64, 65, 255, 257, 2047, 2049, 8193, 100_003]


def device_columns(ctx, table, n, with_bitmaps):
    """[(values, validity | None, offsets | None)] of the first n rows, with TAIL rows behind that pass the predicate and every
    validity bit from n to the end of its allocation set; Utf8 offsets past n keep ascending into bytes that are there"""
    spec, cols = table.spec, []
    for c in range(spec.n_cols):
        v, tail = table.values[c], spec.passing[c](TAIL)
        bm = None
        if with_bitmaps and spec.nullable[c]:
            bits = np.ones((n + TAIL + 7) // 8 * 8 + 64 * 8, bool)
            bits[:n] = table.valid[c][:n]
            bm = ctx.to_device(np.packbits(bits, bitorder="little"))
        if isinstance(v, U8):
            nb = int(v.off[n])
            off = ctx.to_device(np.concatenate([v.off[:n + 1], nb + tail.off[1:]]).astype(np.int32))
            data = ctx.to_device(np.concatenate([v.data[:nb], tail.data, np.full(64, 73, np.uint8)]))
            cols.append((data, bm, off))
        else:
            cols.append((ctx.to_device(np.concatenate([v[:n], tail])), bm, None))
    return cols


def direct_launch(ctx, kind, cols, n):
    """the operator's own Python entry point where the fuzz test uses one, plan.launch otherwise -> (counts, sums)"""
    spec = SPECS[kind]
    p = spec.params
    none = np.zeros(0, np.float64)
    if kind in ("k2", "k6", "k7"):
        d = ctx.zeros(np.int64, 1)
        if kind == "k2":
            ctx.region_count(cols[0][0], cols[1][0], n, *p, d, chrom_valid=cols[0][1], pos_valid=cols[1][1])
        else:
            (ctx.overlap_count if kind == "k6" else ctx.within_count)(cols[0][0], cols[0][1], cols[1][0], cols[1][1], cols[2][0], cols[2][1], n, *p, d)
        ctx.sync()
        return d.to_host(), none
    if kind == "k3":
        d = ctx.zeros(np.int64, p[3] + 1)
        ctx.flag_mapq_group_count(cols[0][0], cols[1][0], cols[1][1], cols[2][0], cols[2][1], n, p[0], p[1], p[2], p[3], d, flag_valid=cols[0][1])
        ctx.sync()
        return d.to_host(), none
    if kind == "k4f":
        dc, ds = ctx.zeros(np.int64, 2 * p[2]), ctx.zeros(np.float64, p[2])
        ctx.cmp_avg_by_group(cols[0][0], cols[0][1], cols[1][0], cols[1][1], cols[2][0], n, p[1], p[0], p[2], dc, ds)
        ctx.sync()
        return dc.to_host(), ds.to_host()
    plan = spec.plan(ctx)
    st = ctx.to_device(np.full(plan.n_i64 + plan.n_f64, 0x7B7B7B7B7B7B7B7B, np.int64))
    plan.launch(cols, n, st, overwrite=True)
    ctx.sync()
    words = st.to_host()
    plan.close()
    return words[:plan.n_i64], words[plan.n_i64:].view(np.float64)


@pytest.mark.parametrize("kind,with_bitmaps", [(k, b) for k in KINDS for b in (False, True) if any(SPECS[k].nullable) or not b])  # (K5 / K9 take no bitmap)
def test_rows_and_bits_past_n_are_not_counted(ctx, kind, with_bitmaps):
    table = Table(kind, max(TAIL_N), seed=9, p_valid=0.6)
    if not with_bitmaps:
        for v in table.valid:
            v[:] = True
    for n in TAIL_N:
        cols = device_columns(ctx, table, n, with_bitmaps)
        same(direct_launch(ctx, kind, cols, n), S.expect(table.spec.kind, table.spec.params, table.statement_cols(np.arange(n))))


@pytest.mark.parametrize("kind", FIXED_KINDS)
def test_a_recycled_slot_keeps_no_row_of_its_previous_fill(ctx, kind, monkeypatch):
    """Slots of 4096 rows.  Two full ones (the stream double-buffers, so the third fill reuses the first one's device buffers), every
    row passing and valid, a bitmap in every column (row 0 is NULL); then 1001 rows of the same values: rows 1001 ... 4095 of the
    recycled device buffers -- values and validity bits -- would all pass."""
    monkeypatch.setenv("EXON_HIP_COALESCE_ROWS", "4096")
    spec = SPECS[kind]
    table = Table(kind, 4096 + 4096 + 1001, seed=10)
    for c in range(spec.n_cols):
        table.values[c] = spec.passing[c](table.n)
        table.valid[c][:] = True
        if spec.nullable[c]:
            table.valid[c][[0, 4096, 8192]] = False
    table.seal()
    cuts = [(0, 4096, NULLS), (4096, 4096, NULLS), (8192, 1001, NULLS)]
    assert all(table.carries_bitmap(c, *cut) for cut in cuts for c in range(spec.n_cols) if spec.nullable[c])
    want = table.want(cuts)
    same(run_cuts(ctx, table, cuts), want)
    one = Table(kind, 4096, seed=10)
    one.values, one.valid = [v[:4096] for v in table.values], [v[:4096] for v in table.valid]
    same(want, S.fold(spec.kind, spec.params, [one.want([(0, 4096, NULLS)])] * 2 + [one.want([(0, 1001, NULLS)])]))  # the sum of the three fills


# ---- 3. refusals and ownership ----------------------------------------------------------------------------------------------------
def open_with_rows(ctx, kind, seed=12):
    """a stream that has accepted 300 rows (hand-built, so their release is counted too) -> (plan, stream, table, hands, state of those rows)"""
    cuts = chain([123, 177], [NULLS, UNKNOWN], start=2)
    table = Table(kind, end_of(cuts) + 64, cuts, seed=seed)
    plan = SPECS[kind].plan(ctx)
    st = plan.open()
    hands = [Hand(rows, hand_children(table, lo, rows, modes)) for lo, rows, modes in cuts]
    for h in hands:
        assert h.push(st) == 0
    return plan, st, table, hands, table.want(cuts)


def finish_close(plan, st, hands, want):
    same(st.finish(), want)
    st.close()
    plan.close()
    assert released_once(hands)


@pytest.mark.parametrize("kind", ["k2", "k4f", "k5"])
def test_push_after_finish_is_refused_and_the_batch_released(ctx, kind):
    plan, st, table, hands, want = open_with_rows(ctx, kind)
    same(st.finish(), want)
    late = Hand(50, hand_children(table, 10, 50, NONE))
    assert late.push(st) == ESTATE
    assert not late.arr.release and late.released == 1  # moved and released, error or not
    with pytest.raises(exon_amd.ExonHipError) as e:
        st.push(table.batch(0, 10, NONE))
    assert e.value.code == ESTATE
    finish_close(plan, st, hands + [late], want)


@pytest.mark.parametrize("later_push", [False, True])
@pytest.mark.parametrize("kind", UTF8_KINDS)
def test_a_null_fastq_line_is_unsupported_at_the_flush(ctx, kind, later_push, monkeypatch):
    import pyarrow as pa
    monkeypatch.setenv("EXON_HIP_COALESCE_ROWS", "100")
    spec = SPECS[kind]
    lines = [b"IIII", None, b"GGCC"] + [b"ACGT"] * 57
    bad = pa.RecordBatch.from_arrays([pa.array(lines if c == spec.n_cols - 1 else [b"ACGT"] * 60, pa.binary()) for c in range(spec.n_cols)], ["a", "b"][:spec.n_cols])
    plan = spec.plan(ctx)
    st = plan.open()
    st.push(bad)  # staged: nothing has looked at the rows yet
    with pytest.raises(exon_amd.ExonHipError) as e:
        if later_push:
            st.push(bad)  # 60 + 60 > 100: the flush in front of this batch fails, the batch is released unread
        else:
            st.finish()
    assert e.value.code == EUNSUPPORTED
    st.reset()  # the rows staged for the refused query go with it
    cuts = chain([70, 70, 1], NONE, start=3)
    table = Table(kind, end_of(cuts), seed=13)
    for cut in cuts:
        st.push(table.batch(*cut))
    same(st.finish(), table.want(cuts))
    st.close()
    plan.close()


@pytest.mark.parametrize("kind", ["k4f", "k4i", "k8"])
def test_a_nullable_group_key_is_unsupported_on_a_pure_push(ctx, kind):
    import pyarrow as pa
    table = Table(kind, 500, seed=14)
    ok = np.ones(500, bool)
    ok[[0, 77, 499]] = False
    arrays = [pa.array(table.values[0]), pa.array(table.values[1]), pa.array(table.values[2], mask=~ok)]
    plan = SPECS[kind].plan(ctx)
    st = plan.open()
    st.push(pa.RecordBatch.from_arrays(arrays, ["x", "y", "g"]))
    with pytest.raises(exon_amd.ExonHipError) as e:
        st.finish()
    assert e.value.code == EUNSUPPORTED
    st.reset()
    cuts = chain([250, 249], [NULLS, UNKNOWN], start=1)
    hands = []
    for cut in cuts:
        table.push(st, cut, hands)
    same(st.finish(), table.want(cuts))
    st.close()
    plan.close()
    assert released_once(hands)


@pytest.mark.parametrize("kind", ["k2", "k3", "k9"])
def test_a_child_shorter_than_the_batch_is_refused(ctx, kind):
    """(a) a child of 5 rows under a batch of 10; (b) a child of length 10 at offset 5 under a batch of offset 5 and length 10: its
    rows end at logical row 10, the batch asks for rows up to 15 (a child's length counts from its own offset).  Both are built
    with all the rows the batch asks for present in memory, so a check that lets one through still reads the test's own memory."""
    plan, st, table, hands, want = open_with_rows(ctx, kind)
    spec = SPECS[kind]
    last = spec.n_cols - 1
    a = hand_children(table, 5, 10, NULLS)
    a[last]["length"] = 5
    b = hand_children(table, 5, 10, NULLS, batch_offset=5, child_offsets=[5] * spec.n_cols)
    assert b[last]["length"] == 15 and b[last]["offset"] == 5
    b[last]["length"] = 10
    short = [Hand(10, a), Hand(10, b, offset=5)]
    for h in short:
        assert h.push(st) == EINVAL
        assert not h.arr.release and h.released == 1
    finish_close(plan, st, hands + short, want)


@pytest.mark.parametrize("kind", ["k6", "k4f", "k5", "k9"])
def test_malformed_batches_are_refused_and_released(ctx, kind):
    plan, st, table, hands, want = open_with_rows(ctx, kind)
    spec = SPECS[kind]
    last = spec.n_cols - 1
    listy = hand_children(table, 5, 10, NONE)
    listy[last]["n_children"] = 1  # a List<item> child
    few_buffers = hand_children(table, 5, 10, NONE)
    few_buffers[last]["n_buffers"] = 2 if spec.types[last] == "utf8" else 1
    null_child = Hand(10, hand_children(table, 5, 10, NONE))
    null_child.kids[last] = C.POINTER(L.ArrowArray)()
    cases = [(Hand(10, listy), EUNSUPPORTED), (Hand(10, hand_children(table, 5, 10, NONE), n_children=spec.n_cols - 1), EINVAL), (Hand(10, few_buffers), EINVAL),
             (null_child, EINVAL)]
    for h, code in cases:
        assert h.push(st) == code
        assert not h.arr.release and h.released == 1
    again = Hand(10, hand_children(table, 5, 10, NONE))
    again.arr.release = None  # an array that is already released: refused and left alone
    assert again.push(st) == EINVAL and again.released == 0
    finish_close(plan, st, hands + [h for h, _ in cases], want)


def device_batch(ctx, columns, n_rows, child_offset):
    """an ArrowDeviceArray over [(values DeviceBuffer, validity DeviceBuffer | None)] whose children all have `child_offset`"""
    h = Hand(n_rows, [{"length": n_rows, "offset": child_offset, "null_count": -1 if b else 0, "buffers": [b.ptr if b else None, v.ptr]} for v, b in columns])
    top = L.ArrowDeviceArray()
    top.array = h.arr
    top.device_id, top.device_type = ctx.device, L.ARROW_DEVICE_ROCM
    return top, h


@pytest.mark.parametrize("kind", ["k2", "k4f"])
def test_push_device_child_offsets(ctx, kind):
    """children at offset 1 (a bitmap that would start inside a byte; int32 values 4 bytes off their 16-byte alignment): EINVAL and
    nothing launched; at offset 64 with bitmaps: accepted, and the state is that of rows 64 ..."""
    spec = SPECS[kind]
    n = 3000
    table = Table(kind, n + 64, seed=15)
    dev = [(ctx.to_device(np.concatenate([v, spec.passing[c](64)])),
            ctx.to_device(np.concatenate([np.packbits(table.valid[c], bitorder="little"), np.full(72, 0xFF, np.uint8)])) if spec.nullable[c] else None)
           for c, v in enumerate(table.values)]
    ctx.sync()
    plan = spec.plan(ctx)
    st = plan.open()
    good, keep = device_batch(ctx, dev, n, 64)  # (`keep` owns the children the struct points to)
    assert ctx.lib.exon_hip_stream_push_device(st.h, C.byref(good)) == 0
    want = S.expect(spec.kind, spec.params, table.statement_cols(np.arange(64, 64 + n)))
    for columns in (dev, [(v, None) for v, _ in dev]):  # with bitmaps: the bit offset; without: the values pointer
        bad, keep_bad = device_batch(ctx, columns, n, 1)
        assert ctx.lib.exon_hip_stream_push_device(st.h, C.byref(bad)) == EINVAL
    same(st.finish(), want)
    st.close()
    plan.close()
