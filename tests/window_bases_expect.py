"""Plain numpy for plan kind 13 (bases per fixed-width window along each contig), written from the rules in include/exon_hip.h.

`contigs` is [(reference id, length)], `W` the window width.  Contig c has K_c = ceil(L_c / W) windows, window j = [j * W + 1,
min((j + 1) * W, L_c)]; the windows of all contigs, in the order given, are the B bins.  A row is counted when its three values are
valid, its id is one of the contigs' and end >= start; it is then clipped to [1, L_c] and may lie outside altogether.

  expect        the four totals and the bases per window by per-base pileup: every base of every clipped row is put in its window
  expect_fast   the same from sorted starts and ends: F(x) = bases at positions <= x, bases_j = F(window end) - F(window start - 1)
  expect_state  the E and D sections word by word, as the kernel's adds define them, in uint64 arithmetic that wraps
"""
import numpy as np


def pack_bits(valid):
    return np.packbits(np.asarray(valid, bool), bitorder="little")


def offsets(contigs, W):
    k = [(int(n) - 1) // int(W) + 1 for _, n in contigs]
    return np.concatenate([[0], np.cumsum(k)]).astype(np.int64)


def windows(contigs, W):
    """[(contig id, start, end)] of every window, in bin order"""
    out = []
    for c, n in contigs:
        for j in range((n - 1) // W + 1):
            out.append((c, j * W + 1, min((j + 1) * W, n)))
    return out


def classify(contigs, ref, start, end, rv=None, sv=None, ev=None):
    """-> totals[4], and for the counted rows: contig slot, clipped start, clipped end (rows outside their contig dropped)"""
    ref, start, end = np.asarray(ref, np.int64), np.asarray(start, np.int64), np.asarray(end, np.int64)
    n = len(ref)
    valid = np.ones(n, bool)
    for v in (rv, sv, ev):
        if v is not None:
            valid &= np.asarray(v, bool)
    keys = np.array([k for k, _ in contigs], np.int64)
    order = np.argsort(keys, kind="stable")
    pos = np.minimum(np.searchsorted(keys[order], ref), len(keys) - 1)
    slot = np.where(keys[order][pos] == ref, order[pos], -1)
    length = np.where(slot >= 0, np.array([ln for _, ln in contigs], np.int64)[slot], 0)
    on = valid & (slot >= 0)
    hit = on & (end >= start)
    totals = np.array([hit.sum(), (~valid).sum(), (valid & ~on).sum(), (on & ~hit).sum()], np.int64)
    s = np.maximum(start[hit], 1)
    e = np.minimum(end[hit], length[hit])
    inside = s <= e
    return totals, slot[hit][inside], s[inside], e[inside]


def expect(contigs, W, ref, start, end, rv=None, sv=None, ev=None):
    woff = offsets(contigs, W)
    totals, slot, s, e = classify(contigs, ref, start, end, rv, sv, ev)
    bases = np.zeros(int(woff[-1]), np.int64)
    for c, a, b in zip(slot.tolist(), s.tolist(), e.tolist()):
        np.add.at(bases, woff[c] + (np.arange(a, b + 1, dtype=np.int64) - 1) // W, 1)
    return totals, bases


def expect_fast(contigs, W, ref, start, end, rv=None, sv=None, ev=None):
    woff = offsets(contigs, W)
    totals, slot, s, e = classify(contigs, ref, start, end, rv, sv, ev)
    bases = np.zeros(int(woff[-1]), np.int64)
    for c, (_, ln) in enumerate(contigs):
        m = slot == c
        ss, ee = np.sort(s[m]), np.sort(e[m])
        cs, ce = np.concatenate([[0], np.cumsum(ss)]), np.concatenate([[0], np.cumsum(ee)])
        k = int(woff[c + 1] - woff[c])
        x = np.minimum(np.arange(0, k + 1, dtype=np.int64) * W, ln)  # window boundaries: 0, W, 2W, ..., L
        ns, ne = np.searchsorted(ss, x, side="right"), np.searchsorted(ee, x, side="right")
        f = ns * (x + 1) - cs[ns] - ne * x + ce[ne]  # F(x): a row with s <= x adds min(e, x) - s + 1
        bases[woff[c]:woff[c + 1]] = f[1:] - f[:-1]
    return totals, bases


def expect_state(contigs, W, ref, start, end, rv=None, sv=None, ev=None):
    woff = offsets(contigs, W)
    B = int(woff[-1])
    totals, slot, s, e = classify(contigs, ref, start, end, rv, sv, ev)
    E, D = np.zeros(B, np.uint64), np.zeros(B, np.uint64)
    base = woff[slot]
    js, je = (s - 1) // W, (e - 1) // W
    one = js == je
    with np.errstate(over="ignore"):
        np.add.at(E, base[one] + js[one], (e - s + 1)[one].astype(np.uint64))
        two = ~one
        np.add.at(E, base[two] + js[two], ((js + 1) * W - s + 1)[two].astype(np.uint64))
        np.add.at(E, base[two] + je[two], (e - je * W)[two].astype(np.uint64))
        mid = je > js + 1
        np.add.at(D, base[mid] + js[mid] + 1, np.uint64(1))
        np.add.at(D, base[mid] + je[mid], np.uint64(2**64 - 1))
    return np.concatenate([totals.astype(np.uint64), E, D]).view(np.int64)


def decode(contigs, W, state):
    """E[j] + W * (running sum of D within the contig), uint64 arithmetic"""
    woff = offsets(contigs, W)
    B = int(woff[-1])
    w = np.asarray(state, np.int64).view(np.uint64)
    E, D = w[4:4 + B], w[4 + B:4 + 2 * B]
    out = np.zeros(B, np.uint64)
    with np.errstate(over="ignore"):
        for c in range(len(contigs)):
            a, b = int(woff[c]), int(woff[c + 1])
            out[a:b] = E[a:b] + np.cumsum(D[a:b], dtype=np.uint64) * np.uint64(W)
    return out.view(np.int64)
