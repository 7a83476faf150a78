"""Expected state of the per-position quality histogram (K5, EXON_HIP_PLAN_QUAL_POS_HIST), in plain numpy.  Written from the
statement of the query in include/exon_hip.h; imports nothing of the package or the oracle, so it can be wrong only on its own.

    hist[p, b] = number of reads r with p < ends[r] - starts[r] and data[starts[r] + p] == b        int64 [lmax, 256]

The reads are views [starts[r], ends[r]) into `data`: an Arrow Utf8 column is the views (offsets[:-1], offsets[1:]); views may
leave gaps, overlap, repeat and come in any order.

The table of LENGTH CLASSES restates the head comment of the kernel (exon_amd/csrc/kernels.hip, "K5 qual_pos_hist"): a column
whose reads all have length L and sit back to back is taken by path A when 9 <= L <= 310 and its position pattern repeats after
P = L / gcd(L, 4) >= 8 dwords (with 1, 2 or 4 copies of the table), by path B for the other L <= 310 (when the first byte is 16-byte
aligned), by path G otherwise.  The tests use it to CHOOSE lengths and to label failures; the library does not report which path
ran, so nothing may assert it.
"""
from math import gcd

import numpy as np

PT_MAX = 310        # positions one workgroup keeps in LDS; uniform lengths beyond it are path G's
A_SLOTS = 320       # path A's table: 5 planes x 64 columns
JUNK_FRONT, JUNK_BACK, BACK_BYTES = 222, 223, 320


def hist(starts, ends, data, lmax):
    starts, ends = np.asarray(starts, np.int64).ravel(), np.asarray(ends, np.int64).ravel()
    data = np.asarray(data, np.uint8).ravel()
    if starts.size != ends.size:
        raise ValueError("starts and ends differ in length")
    if lmax < 1:
        raise ValueError("lmax < 1")
    lens = ends - starts
    if (lens < 0).any():
        raise ValueError("negative view length")
    if lens.size and int(lens.max()) > lmax:
        raise ValueError("read longer than lmax")  # the device refuses it: so does the reference
    total = int(lens.sum())
    if total == 0:
        return np.zeros((lmax, 256), np.int64)
    if int(starts[lens > 0].min()) < 0 or int(ends[lens > 0].max()) > data.size:
        raise ValueError("view outside the buffer")
    first = np.cumsum(lens) - lens                       # index of every read's first byte among all bytes, in read order
    pos = np.arange(total, dtype=np.int64) - np.repeat(first, lens)
    byte = data[np.repeat(starts, lens) + pos].astype(np.int64)
    return np.bincount(pos * 256 + byte, minlength=lmax * 256).astype(np.int64).reshape(lmax, 256)


def hist_column(offsets, data, lmax):
    """hist of an Arrow Utf8 column (offsets int32[n + 1], data)"""
    offsets = np.asarray(offsets, np.int64)
    return hist(offsets[:-1], offsets[1:], data, lmax)


def column(lens, shift=0, payload=None, rng=None):
    """(offsets int32[n + 1], data uint8) of a Utf8 column with the given read lengths: `shift` junk bytes (222) in front, so that
    offsets[0] == shift is the residue of the first byte in a buffer that starts aligned, and 320 junk bytes (223) behind.
    payload: the bytes of the reads, or a function total -> bytes; default: `rng` draws Phred+33 bytes 33..74."""
    lens = np.asarray(lens, np.int64).ravel()
    total = int(lens.sum())
    if payload is None:
        payload = (rng or np.random.default_rng(total)).integers(33, 75, total, dtype=np.uint8)
    elif callable(payload):
        payload = payload(total)
    payload = np.asarray(payload, np.uint8).ravel()
    if payload.size != total:
        raise ValueError("payload size")
    off = np.zeros(lens.size + 1, np.int64)
    off[1:] = np.cumsum(lens)
    off += shift
    if int(off[-1]) >= 2 ** 31:
        raise ValueError("offsets beyond int32")
    data = np.concatenate([np.full(shift, JUNK_FRONT, np.uint8), payload, np.full(BACK_BYTES, JUNK_BACK, np.uint8)])
    return off.astype(np.int32), data


# ---- length classes ----------------------------------------------------------------------------------------------------------
def period(L):
    """dwords after which the (dword -> positions) map of back-to-back reads of length L repeats"""
    return L // gcd(L, 4)


def copies(P):
    return 1 if P >= 32 else 2 if P >= 16 else 4


def length_class(L):
    """'B', 'A4', 'A2', 'A1' (path A with that many table copies) or 'G' for a uniform, back-to-back, 16-byte aligned column"""
    if L < 1 or L > PT_MAX:
        return "G"
    P = period(L)
    if P < 8:
        return "B"
    return "A%d" % copies(P)


def slots(L):
    """table slots path A needs for length L: copies x 4 ceil(L / 4)"""
    return copies(period(L)) * 4 * ((L + 3) // 4)


CLASSES = {L: length_class(L) for L in range(1, 401)}
B_LENGTHS = sorted(L for L, c in CLASSES.items() if c == "B")
