"""What the covered-bases plan (kind 12) must give, in plain numpy, written from the words of include/exon_hip.h.

Rows and regions are 1-based inclusive.  A counted row [s, e] (all three values valid, its contig in the set, s <= e) covers
max(0, min(e, re) - max(s, rs) + 1) bases of a region [rs, re] of its contig; a region's `bases` is the sum over the counted rows.

`expect` is brute force, O(n M): every region clipped against every counted row.  `expect_pileup` is an independent second route for
small coordinates: a per-base difference array per contig, prefix-summed into depth, then summed over each region.  `expect_fast` sorts
the ROWS of each contig and takes searchsorted + prefix sums of the sorted starts and ends (the plan sorts the regions' boundaries
instead); the large GPU cases use it and test_region_bases_abi.py holds it against `expect`.  `expect_state` is the full state
(totals, Ns, Ss, Ne, Se), every row looked at one by one, the sums modulo 2^64.

Regions are (contig id, start, end) triples; the totals are (counted, null_rows, elsewhere, inverted), as kind 11's."""
import numpy as np

from region_set_expect import OPEN_END, _classes, pack_bits, slots  # noqa: F401  (the row classes are kind 11's, word for word)

MASK = (1 << 64) - 1


def expect(regions, ref, start, end, rv=None, sv=None, ev=None):
    """(totals[4], bases[M]) by brute force"""
    ref, start, end = np.asarray(ref), np.asarray(start, np.int64), np.asarray(end, np.int64)
    counted, totals = _classes(regions, ref, start, end, rv, sv, ev)
    r, s, e = ref[counted], start[counted], end[counted]
    bases = []
    for c, rs, re in regions:
        on = r == c
        lo, hi = np.maximum(s[on], rs), np.minimum(e[on], re)
        keep = hi >= lo
        bases.append(int((hi[keep] - lo[keep] + 1).sum()))
    return totals, np.array(bases, np.int64)


def expect_pileup(regions, ref, start, end, rv=None, sv=None, ev=None, span=None):
    """the same from per-base depth; coordinates (the regions' closed ends too) must be small"""
    ref, start, end = np.asarray(ref), np.asarray(start, np.int64), np.asarray(end, np.int64)
    counted, totals = _classes(regions, ref, start, end, rv, sv, ev)
    r, s, e = ref[counted], start[counted], end[counted]
    top = max([int(e.max()) if e.size else 1] + [re for _, _, re in regions if re != OPEN_END]) + 2 if span is None else span
    depth = {}
    for c in {x[0] for x in regions}:
        d = np.zeros(top + 2, np.int64)
        on = r == c
        np.add.at(d, s[on], 1)
        np.add.at(d, e[on] + 1, -1)
        depth[c] = np.cumsum(d)  # depth[c][x] = rows covering base x
    bases = [int(depth[c][rs:min(re, top) + 1].sum()) for c, rs, re in regions]
    return totals, np.array(bases, np.int64)


def expect_fast(regions, ref, start, end, rv=None, sv=None, ev=None):
    """the same by sorting the rows of each contig: with the starts and the ends of a contig's rows sorted,
    G(x) = bases at positions <= x = sum over starts <= x of (x + 1 - s)  -  sum over ends <= x of (x - e), modulo 2^64"""
    ref, start, end = np.asarray(ref), np.asarray(start, np.int64), np.asarray(end, np.int64)
    counted, totals = _classes(regions, ref, start, end, rv, sv, ev)
    r, s, e = ref[counted], start[counted], end[counted]
    rc = np.array([x[0] for x in regions], np.int64)
    rs = np.array([x[1] for x in regions], np.int64)
    re = np.array([x[2] for x in regions], np.int64)
    bases = np.zeros(len(regions), np.uint64)
    with np.errstate(over="ignore"):
        for c in np.unique(rc):
            on = r == c
            ss, es = np.sort(s[on]), np.sort(e[on])
            cs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(ss.astype(np.uint64), dtype=np.uint64)])
            ce = np.concatenate([np.zeros(1, np.uint64), np.cumsum(es.astype(np.uint64), dtype=np.uint64)])

            def G(x):
                a, b = np.searchsorted(ss, x, "right"), np.searchsorted(es, x, "right")
                xu = x.astype(np.uint64)
                return (xu + np.uint64(1)) * a.astype(np.uint64) - cs[a] - xu * b.astype(np.uint64) + ce[b]
            m = rc == c
            bases[m] = G(re[m]) - G(rs[m] - 1)
    return totals, bases.view(np.int64)


def points(regions):
    """per contig, in order of first appearance: the sorted unique values {rs - 1} U {re}"""
    order, _ = slots(regions)
    return [sorted({rs - 1 for c, rs, _ in regions if c == k} | {re for c, _, re in regions if c == k}) for k in order]


def layout(regions):
    """word offsets of totals, Ns, Ss, Ne, Se, and the word count: four sections of P + C words"""
    pts = points(regions)
    nb = sum(len(p) for p in pts) + len(pts)
    return (0, 4, 4 + nb, 4 + 2 * nb, 4 + 3 * nb, 4 + 4 * nb)


def expect_state(regions, ref, start, end, rv=None, sv=None, ev=None):
    """every word of the state: a counted row [s, e] of contig c adds 1 to Ns[base_c + p], s to Ss[base_c + p], 1 to Ne[base_c + q],
    e to Se[base_c + q]; p / q = index of the contig's first point >= s / >= e, base_c = (points of the contigs in front of c) + c"""
    ref, start, end = np.asarray(ref), np.asarray(start, np.int64), np.asarray(end, np.int64)
    counted, totals = _classes(regions, ref, start, end, rv, sv, ev)
    order, _ = slots(regions)
    pts = points(regions)
    at = layout(regions)
    st = [0] * at[5]
    st[:4] = [int(t) for t in totals]
    base, k = {}, 0
    for j, c in enumerate(order):
        base[c] = (k + j, pts[j])
        k += len(pts[j])
    for i in np.flatnonzero(counted):
        b, pt = base[int(ref[i])]
        s, e = int(start[i]), int(end[i])
        p = sum(1 for x in pt if x < s)
        q = sum(1 for x in pt if x < e)
        st[at[1] + b + p] += 1
        st[at[2] + b + p] = (st[at[2] + b + p] + s) & MASK
        st[at[3] + b + q] += 1
        st[at[4] + b + q] = (st[at[4] + b + q] + e) & MASK
    return np.array(st, np.uint64).view(np.int64)
