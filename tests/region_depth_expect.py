"""What the region-set depth plan (kind 14) must give, in plain numpy, written from the words of include/exon_hip.h.

Rows and regions are 1-based inclusive.  The TARGET SPACE: contigs in order of first appearance; per contig the regions sorted and
merged (next start <= current end + 1) into disjoint intervals; a bin per target base and one terminator per contig.  The depth of a
target base is the number of counted rows (kind 11's row classes) that cover it; a region's `bases` is the sum of the depths of its
bases, `ge[t]` the number of its bases whose depth is at least thresholds[t].

`expect` is the per-base pileup: a difference array over every position from the contig's first target base to its last, summed up
and read at the target bases.  `expect_fast` reads the same depth from the sorted starts and ends of a contig's rows, for coordinates a
pileup cannot span.  `expect_state` is every word of the state, `decode` what the state's words say when nothing is known of the rows.

Regions are (contig id, start, end) triples; the totals are (counted, null_rows, elsewhere, inverted), as kind 11's."""
import numpy as np

from region_bases_expect import MASK, _classes, pack_bits, slots  # noqa: F401  (the row rules are kind 11's and 12's)


def merged(regions):
    """per contig, in order of first appearance: the merged intervals as [(start, end)], ascending"""
    order, _ = slots(regions)
    out = []
    for k in order:
        iv = []
        for s, e in sorted((s, e) for c, s, e in regions if c == k):
            if iv and s <= iv[-1][1] + 1:
                iv[-1][1] = max(iv[-1][1], e)
            else:
                iv.append([s, e])
        out.append([(s, e) for s, e in iv])
    return out


def layout(regions):
    """word offsets of the totals and of D, and the word count: T + C bins"""
    iv = merged(regions)
    return (0, 4, 4 + sum(e - s + 1 for c in iv for s, e in c) + len(iv))


def doffs(regions):
    """first bin of each contig: the target bases of the contigs in front of it, and one terminator each"""
    out, at = [], 0
    for c in merged(regions):
        out.append(at)
        at += sum(e - s + 1 for s, e in c) + 1
    return out


def intervals(regions):
    """(slot, start, end, bin of the first base) of every merged interval, in bin order"""
    out = []
    for j, (c, d) in enumerate(zip(merged(regions), doffs(regions))):
        for s, e in c:
            out.append((j, s, e, d))
            d += e - s + 1
    return out


def below(iv, x):
    """the target bases of one contig (its merged intervals `iv`) at positions <= x, for int64 arrays x"""
    x = np.asarray(x, np.int64)
    ms = np.array([s for s, _ in iv], np.int64)
    ln = np.array([e - s + 1 for s, e in iv], np.int64)
    cum = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    j = np.searchsorted(ms, x, "right")
    k = np.maximum(j - 1, 0)
    with np.errstate(over="ignore"):
        inside = np.minimum(x - ms[k], ln[k] - 1) + 1  # x >= ms[k] >= 1 where j > 0: no wrap there
    return np.where(j == 0, 0, cum[k] + inside)


def region_bins(regions):
    """(lo[M], hi[M]): region i is the bins [lo[i], hi[i]) of D, re - rs + 1 of them"""
    _, slot = slots(regions)
    slot = np.array(slot)
    rs = np.array([r[1] for r in regions], np.int64)
    re = np.array([r[2] for r in regions], np.int64)
    lo, hi = np.zeros(len(regions), np.int64), np.zeros(len(regions), np.int64)
    for j, (iv, d) in enumerate(zip(merged(regions), doffs(regions))):
        on = slot == j
        lo[on], hi[on] = d + below(iv, rs[on] - 1), d + below(iv, re[on])
    assert np.array_equal(hi - lo, re - rs + 1)
    return lo, hi


def positions(iv):
    return np.concatenate([np.arange(s, e + 1, dtype=np.int64) for s, e in iv])


def _per_base(regions, ref, start, end, rv, sv, ev, fast):
    ref, start, end = np.asarray(ref), np.asarray(start, np.int64), np.asarray(end, np.int64)
    counted, totals = _classes(regions, ref, start, end, rv, sv, ev)
    r, s, e = ref[counted], start[counted], end[counted]
    order, _ = slots(regions)
    depth = []
    for c, iv in zip(order, merged(regions)):
        on = r == c
        pos = positions(iv)
        if fast:
            depth.append(np.searchsorted(np.sort(s[on]), pos, "right") - np.searchsorted(np.sort(e[on]), pos, "left"))
            continue
        lo, hi = iv[0][0], iv[-1][1]
        sc, ec = np.clip(s[on], lo, hi + 1), np.clip(e[on], lo - 1, hi)  # clipped to the span; a row outside it becomes empty
        keep = ec >= sc
        d = np.zeros(hi - lo + 3, np.int64)
        np.add.at(d, sc[keep] - lo, 1)
        np.add.at(d, ec[keep] - lo + 1, -1)
        depth.append(np.cumsum(d)[pos - lo])
    return totals, depth


def expect(regions, thresholds, ref, start, end, rv=None, sv=None, ev=None, fast=False):
    """(totals[4], depth[T] in bin order, bases[M], ge[M, k]) from the pileup"""
    totals, depth = _per_base(regions, ref, start, end, rv, sv, ev, fast)
    lo, hi = region_bins(regions)
    # the depths laid out as the bins are, a 0 at every terminator
    at = np.concatenate([np.append(d, 0) for d in depth])
    bases = np.zeros(len(regions), np.int64)
    ge = np.zeros((len(regions), len(thresholds)), np.int64)
    for i in range(len(regions)):
        d = at[lo[i]:hi[i]]
        bases[i] = d.sum()
        ge[i] = [(d >= t).sum() for t in thresholds]
    return totals, np.concatenate(depth), bases, ge


def expect_state(regions, ref, start, end, rv=None, sv=None, ev=None):
    """every word of the state: a counted row [s, e] of contig c with lo = below(s - 1) (0 for s <= 1) and hi = below(e) adds 1 to
    D[doff_c + lo] and 2^64 - 1 to D[doff_c + hi] if hi > lo"""
    ref, start, end = np.asarray(ref), np.asarray(start, np.int64), np.asarray(end, np.int64)
    counted, totals = _classes(regions, ref, start, end, rv, sv, ev)
    order, _ = slots(regions)
    at = layout(regions)
    st = np.zeros(at[2], np.uint64)
    st[:4] = totals
    for c, iv, d in zip(order, merged(regions), doffs(regions)):
        on = counted & (ref == c)
        s, e = start[on], end[on]
        lo = below(iv, np.where(s <= 1, 0, s - np.int64(1)))
        hi = below(iv, e)
        add = hi > lo
        with np.errstate(over="ignore"):
            np.add.at(st, at[1] + d + lo[add], np.uint64(1))
            np.add.at(st, at[1] + d + hi[add], np.uint64(MASK))
    return st.view(np.int64)


def running(regions, state):
    """the running sum of the whole section D, modulo 2^64, as int64"""
    with np.errstate(over="ignore"):
        return np.cumsum(np.asarray(state, np.int64)[4:].view(np.uint64), dtype=np.uint64).view(np.int64)


def decode(regions, thresholds, state):
    """(depth[T], bases[M], ge[M, k]) from the state's words alone"""
    run = running(regions, state)
    iv, dof = merged(regions), doffs(regions)
    lo, hi = region_bins(regions)
    keep = np.ones(run.size, bool)
    keep[[d + sum(e - s + 1 for s, e in c) for c, d in zip(iv, dof)]] = False  # the terminators
    bases = np.zeros(len(regions), np.int64)
    ge = np.zeros((len(regions), len(thresholds)), np.int64)
    for i in range(len(regions)):
        d = run[lo[i]:hi[i]]
        with np.errstate(over="ignore"):
            bases[i] = np.array(d.view(np.uint64).sum(dtype=np.uint64)).view(np.int64)[()]
        ge[i] = [(d >= t).sum() for t in thresholds]
    return run[keep], bases, ge
