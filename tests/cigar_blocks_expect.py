"""What the aligned-blocks operator must give, in plain Python, written from the words of include/exon_hip.h -- no code shared with
exon_amd/csrc/host/cigar_blocks.h, and a different route: every counted op's interval is collected first, then touching intervals
are merged.  tests/test_cigar_blocks_expect.py holds it against a brute-force set of covered positions.

A CIGAR is a list of (length, code) pairs, code 0 .. 15 (BAM: "MIDNSHP=X" for 0 .. 8).  Positions are 1-based inclusive.  `mask` is
cover_ops: bit i = code i is covered; legal masks are the non-empty subsets of 0x18D."""
import numpy as np

REF_CODES = (0, 2, 3, 7, 8)  # the ops that consume the reference: M D N = X
LEGAL = 0x18D
ALIGNED, ALIGNED_DEL = 0x181, 0x185
LEGAL_MASKS = [m for m in range(1, 0x200) if m & ~LEGAL == 0]  # 31 of them
LETTERS = "MIDNSHP=X"


def cigar(text):
    """'10M5I10M' -> [(10, 0), (5, 1), (10, 0)]"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num), LETTERS.index(ch)))
            num = ""
    assert not num
    return out


def encode(ops):
    """BAM's u32 encoding, len << 4 | code"""
    return np.array([(ln << 4) | code for ln, code in ops], np.uint32)


def blocks(ops, start, mask):
    """the maximal runs of covered positions as [(first, last)], in order"""
    assert mask and mask & ~LEGAL == 0
    pos, counted = start, []
    for ln, code in ops:
        if code in REF_CODES:
            if ln > 0 and (mask >> code) & 1:
                counted.append((pos, pos + ln - 1))
            pos += ln
    out = []
    for a, b in counted:  # (already in increasing order and disjoint: the position never goes back)
        if out and a == out[-1][1] + 1:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


def covered_positions(ops, start, mask):
    """brute force: the set of covered positions, base by base"""
    pos, cov = start, set()
    for ln, code in ops:
        if code == 0 or code == 2 or code == 3 or code == 7 or code == 8:
            for _ in range(ln):
                if mask & (1 << code):
                    cov.add(pos)
                pos += 1
    return cov


def runs(positions):
    """a set of positions -> its maximal runs [(first, last)]"""
    out = []
    for x in sorted(positions):
        if out and x == out[-1][1] + 1:
            out[-1] = (out[-1][0], x)
        else:
            out.append((x, x))
    return out


def expand(ref, start, cigars, mask, rv=None, sv=None):
    """rows -> block rows (ref int32, start int64, end int64, valid bool): an invalid row gives one invalid row of zeros, a valid row
    without a block the valid row [start, start - 1], any other its blocks"""
    o_ref, o_s, o_e, o_v = [], [], [], []
    for i, ops in enumerate(cigars):
        if (rv is not None and not rv[i]) or (sv is not None and not sv[i]):
            o_ref.append(0), o_s.append(0), o_e.append(0), o_v.append(False)
            continue
        bl = blocks(ops, int(start[i]), mask) or [(int(start[i]), int(start[i]) - 1)]
        for a, b in bl:
            o_ref.append(int(ref[i])), o_s.append(a), o_e.append(b), o_v.append(True)
    return np.array(o_ref, np.int32), np.array(o_s, np.int64), np.array(o_e, np.int64), np.array(o_v, bool)


def pileup(n_refs, span, ref, start, end, valid):
    """per-base depth [n_refs][span + 1] of block rows (index = position; rows outside [1, span] or other contigs are cut / dropped)"""
    d = np.zeros((n_refs, span + 2), np.int64)
    for r, s, e, v in zip(ref, start, end, valid):
        if v and 0 <= r < n_refs and s <= e:
            lo, hi = max(int(s), 1), min(int(e), span)
            if lo <= hi:
                d[r, lo] += 1
                d[r, hi + 1] -= 1
    return np.cumsum(d, axis=1)[:, :span + 1]


def list_columns(cigars, first=0):
    """Arrow List<UInt32>: (offsets int32[n + 1] starting at `first`, ops with `first` filler words in front)"""
    lens = [len(c) for c in cigars]
    offsets = (first + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)
    flat = [op for c in cigars for op in c]
    ops = np.concatenate([np.full(first, 0xFFFFFFF0, np.uint32), encode(flat)]) if flat or first else np.zeros(0, np.uint32)
    return offsets, ops
