"""What the region-set overlap plan (kind 11) must give, in plain numpy.

`expect` is brute force, O(n M): every region against every row by K6's predicate.  `expect_fast` answers the same question by sorting
the ROWS (the plan sorts the regions): count_i = |{rows: start <= re_i}| - |{rows: end < rs_i}| over the counted rows of the region's
contig, two searchsorted calls per contig.  The large cases use it; test_region_set_abi.py holds it against `expect`.
`expect_state` is the full state (totals, A, B) by the header's definition, every row and region looked at one by one.

Regions are (contig id, start, end) triples, 1-based inclusive; the totals are (counted, null_rows, elsewhere, inverted)."""
import numpy as np

OPEN_END = 2**63 - 1


def _classes(regions, ref, start, end, rv=None, sv=None, ev=None):
    n = len(ref)
    valid = np.ones(n, bool)
    for v in (rv, sv, ev):
        if v is not None:
            valid &= np.asarray(v, bool)
    ids = np.array(sorted({r[0] for r in regions}), np.int64)
    on = valid & np.isin(np.asarray(ref, np.int64), ids)
    inverted = on & (np.asarray(end) < np.asarray(start))
    counted = on & ~inverted
    totals = np.array([counted.sum(), (~valid).sum(), (valid & ~on).sum(), inverted.sum()], np.int64)
    return counted, totals


def expect(regions, ref, start, end, rv=None, sv=None, ev=None):
    """(totals[4], counts[M]) by brute force"""
    ref, start, end = np.asarray(ref), np.asarray(start, np.int64), np.asarray(end, np.int64)
    counted, totals = _classes(regions, ref, start, end, rv, sv, ev)
    r, s, e = ref[counted], start[counted], end[counted]
    counts = np.array([int(((r == c) & (s <= re) & (e >= rs)).sum()) for (c, rs, re) in regions], np.int64)
    return totals, counts


def expect_fast(regions, ref, start, end, rv=None, sv=None, ev=None):
    """the same by sorting the rows of each contig"""
    ref, start, end = np.asarray(ref), np.asarray(start, np.int64), np.asarray(end, np.int64)
    counted, totals = _classes(regions, ref, start, end, rv, sv, ev)
    r, s, e = ref[counted], start[counted], end[counted]
    counts = np.zeros(len(regions), np.int64)
    rc = np.array([x[0] for x in regions], np.int64)
    rs = np.array([x[1] for x in regions], np.int64)
    re = np.array([x[2] for x in regions], np.int64)
    for c in np.unique(rc):
        on = r == c
        ss, es = np.sort(s[on]), np.sort(e[on])
        m = rc == c
        counts[m] = np.searchsorted(ss, re[m], "right") - np.searchsorted(es, rs[m], "left")
    return totals, counts


def slots(regions):
    """contig ids in order of first appearance (the state's contig order), and every region's slot"""
    order, slot = [], []
    for c, _, _ in regions:
        if c not in order:
            order.append(c)
        slot.append(order.index(c))
    return order, slot


def layout(regions):
    m, c = len(regions), len(slots(regions)[0])
    return (0, 4, 4 + m + c, 4 + 2 * (m + c))


def expect_state(regions, ref, start, end, rv=None, sv=None, ev=None):
    """every word of the state: a counted row [s, e] of contig c adds 1 to A[base_c + |{i on c: re_i < s}|] and to
    B[base_c + |{i on c: rs_i <= e}|], base_c = (regions of the contigs in front of c) + c"""
    ref, start, end = np.asarray(ref), np.asarray(start, np.int64), np.asarray(end, np.int64)
    counted, totals = _classes(regions, ref, start, end, rv, sv, ev)
    order, slot = slots(regions)
    at = layout(regions)
    st = np.zeros(at[3], np.int64)
    st[:4] = totals
    base, k = {}, 0
    for j, c in enumerate(order):
        base[c] = k + j
        k += slot.count(j)
    for i in np.flatnonzero(counted):
        c = int(ref[i])
        p = sum(1 for (rc, _, re) in regions if rc == c and re < start[i])
        q = sum(1 for (rc, rs, _) in regions if rc == c and rs <= end[i])
        st[at[1] + base[c] + p] += 1
        st[at[2] + base[c] + q] += 1
    return st


def pack_bits(valid, bit_offset=0):
    """Arrow LSB-first bitmap of `valid`, with `bit_offset` unused bits in front"""
    v = np.concatenate([np.zeros(bit_offset, bool), np.asarray(valid, bool)])
    return np.packbits(v, bitorder="little")
