"""Plain-numpy statement of what a stream's finish() returns for every plan kind, from the FULL table the batches were cut from:
one (values, valid) pair per plan column -- values a numpy array (fixed width) or a list of bytes objects (Utf8), valid a boolean
array (all True where a column has no bitmap).  Never touches the library or the oracle; K8 and K9 reuse the two existing
statements (minmax_expect.py, read_stats_expect.py).  tests/test_stream_batches_expect.py checks this module against the oracle.

    expect(kind, params, cols) -> (counts int64[n_i64], sums float64[n_f64])     the packed state

kinds and their params (the arguments of the plan):
    "k2"  region count            cols chrom i32, pos i64                  rid, start, end (None: open)
    "k6"  overlap count           cols ref i32, start i64, end i64         rid, start, end (None: open)
    "k7"  within count            cols ref i32, start i64, end i64         rid, after, before (None: open)
    "k3"  flag / mapq group count cols flag i32, mapq u8, ref i32          mask, value, mapq_min, n_refs
    "k4"  cmp + AVG by group      cols x, y (f32 | i32), group i32         op, thr, n_groups, x_int, y_int
    "k8"  cmp + MIN / MAX         the same
    "k5"  quality x position      col quality Utf8                         lmax
    "k9"  per-read statistics     cols sequence Utf8, quality Utf8         lmax
"""
import numpy as np

import minmax_expect
import read_stats_expect

OPS = minmax_expect.OPS  # ">" ">=" "<" "<=" "=" "!="


def _i64(n):
    return np.array([n], np.int64)


NO_SUMS = np.zeros(0, np.float64)


def k2(cols, rid, start, end):
    (chrom, cv), (pos, pv) = cols
    pos = np.asarray(pos, np.int64)
    hit = np.asarray(cv, bool) & np.asarray(pv, bool) & (np.asarray(chrom) == rid) & (pos >= start)
    if end is not None:
        hit &= pos <= end
    return _i64(hit.sum()), NO_SUMS


def k6(cols, rid, start, end):
    """SemiLazyRecord::intersects: same reference, the record ends at or after the region's start and begins at or before its end"""
    (ref, rv), (s, sv), (e, ev) = cols
    hit = np.asarray(rv, bool) & np.asarray(sv, bool) & np.asarray(ev, bool) & (np.asarray(ref) == rid) & (np.asarray(e, np.int64) >= start)
    if end is not None:
        hit &= np.asarray(s, np.int64) <= end
    return _i64(hit.sum()), NO_SUMS


def k7(cols, rid, after, before):
    (ref, rv), (s, sv), (e, ev) = cols
    hit = np.asarray(rv, bool) & np.asarray(sv, bool) & np.asarray(ev, bool) & (np.asarray(ref) == rid) & (np.asarray(s, np.int64) > after)
    if before is not None:
        hit &= np.asarray(e, np.int64) < before
    return _i64(hit.sum()), NO_SUMS


def k3(cols, mask, value, mapq_min, n_refs):
    """COUNT(*) WHERE flag & mask = value AND mapq >= mapq_min GROUP BY reference; a NULL flag or mapq fails the predicate, a NULL
    reference is a group of its own, the last"""
    (flag, fv), (mapq, mv), (ref, rv) = cols
    keep = np.asarray(fv, bool) & np.asarray(mv, bool) & ((np.asarray(flag, np.int64) & mask) == value) & (np.asarray(mapq).astype(np.int64) >= mapq_min)
    gid = np.where(np.asarray(rv, bool), np.asarray(ref, np.int64), n_refs)
    return np.bincount(gid[keep], minlength=n_refs + 1).astype(np.int64), NO_SUMS


def k4(cols, op, thr, n_groups, x_int=False, y_int=False):
    """[COUNT(y)[G]] [COUNT(*)[G]] + [SUM(y)[G]] WHERE x <op> thr GROUP BY g.  The sums are added in float64 in row order: exact, and
    so the same in any order, when y comes from eighths (or small integers)."""
    (x, xv), (y, yv), (g, gv) = cols
    assert np.asarray(gv, bool).all(), "the group key is not nullable on a push"
    keep = minmax_expect.passes(x, xv, op, thr, x_int)
    both = keep & np.asarray(yv, bool)
    g = np.asarray(g, np.int64)
    counts = np.concatenate([np.bincount(g[both], minlength=n_groups), np.bincount(g[keep], minlength=n_groups)]).astype(np.int64)
    sums = np.zeros(n_groups, np.float64)
    np.add.at(sums, g[both], np.asarray(y)[both].astype(np.float64))
    return counts, sums


def k8(cols, op, thr, n_groups, x_int=False, y_int=False):
    (x, xv), (y, yv), (g, gv) = cols
    assert np.asarray(gv, bool).all(), "the group key is not nullable on a push"
    return minmax_expect.expect(x, xv, y, yv, g, n_groups, op, thr, x_int, y_int), NO_SUMS


def k5(cols, lmax):
    """hist[position][byte] over every quality line (all at most lmax bytes: a longer one is the device's error)"""
    ((quals, qv),) = cols
    assert np.asarray(qv, bool).all(), "quality_scores is not nullable"
    hist = np.zeros((lmax, 256), np.int64)
    lens = np.fromiter((len(q) for q in quals), np.int64, len(quals))
    assert (lens <= lmax).all()
    if lens.sum():
        data = np.frombuffer(b"".join(quals), np.uint8)
        pos = np.arange(len(data)) - np.repeat(np.cumsum(lens) - lens, lens)
        np.add.at(hist, (pos, data), 1)
    return hist.reshape(-1), NO_SUMS


def k9(cols, lmax):
    (seqs, sv), (quals, qv) = cols
    assert np.asarray(sv, bool).all() and np.asarray(qv, bool).all(), "sequence / quality_scores are not nullable"
    return read_stats_expect.expect_fast(list(seqs), list(quals), lmax), NO_SUMS


KINDS = {"k2": k2, "k6": k6, "k7": k7, "k3": k3, "k4": k4, "k8": k8, "k5": k5, "k9": k9}


def expect(kind, params, cols):
    return KINDS[kind](cols, *params)


def take(cols, idx):
    """the rows `idx` (an index array) of a table, as a table"""
    out = []
    for values, valid in cols:
        v = [values[i] for i in idx] if isinstance(values, list) else np.asarray(values)[idx]
        out.append((v, np.asarray(valid, bool)[idx]))
    return out


def fold(kind, params, states):
    """the state of several queries' rows taken together: everything adds, except K8's two extreme planes"""
    if kind == "k8":
        return minmax_expect.fold([s[0] for s in states], params[2]), NO_SUMS
    return sum(s[0] for s in states), sum(s[1] for s in states)
