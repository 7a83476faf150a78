"""Expected state of the per-read FASTQ statistics plan (EXON_HIP_PLAN_READ_STATS_HIST, kind 9), in plain Python / numpy from a
list of (sequence bytes, quality bytes).  Written from the table in include/exon_hip.h; imports nothing of the package or the
oracle, so it can be wrong only on its own.

    totals       [4]         n_reads, sum len(s), sum gc(s), sum of every quality byte
    length       [lmax + 1]  bin len(s)
    gc_percent   [102]       bin floor(100 gc(s) / len(s)); 101 = empty sequence.  gc(s) = bytes equal to 'G' or 'C' (upper case only)
    mean_quality [257]       bin floor(sum(q) / len(q)) on the raw byte; 256 = empty quality line
"""
import numpy as np


def layout(lmax):
    """(totals, length, gc_percent, mean_quality, total words)"""
    return (0, 4, 4 + lmax + 1, 4 + lmax + 1 + 102, 4 + lmax + 1 + 102 + 257)


def gc_count(s):
    return s.count(b"G") + s.count(b"C")


def expect(reads, lmax):
    """reads: iterable of (bytes, bytes).  A sequence longer than lmax is the caller's error (the device refuses it)."""
    at = layout(lmax)
    st = np.zeros(at[4], np.int64)
    for s, q in reads:
        s, q = bytes(s), bytes(q)
        assert len(s) <= lmax and len(q) <= 65536
        gc, qs = gc_count(s), sum(q)
        st[0] += 1
        st[1] += len(s)
        st[2] += gc
        st[3] += qs
        st[at[1] + len(s)] += 1
        st[at[2] + ((100 * gc) // len(s) if s else 101)] += 1
        st[at[3] + (qs // len(q) if q else 256)] += 1
    return st


def expect_fast(seqs, quals, lmax):
    """The same for many reads: per-read figures by numpy over the concatenated bytes (lists of bytes objects)."""
    at = layout(lmax)
    st = np.zeros(at[4], np.int64)
    n = len(seqs)
    ls = np.fromiter((len(s) for s in seqs), np.int64, n)
    lq = np.fromiter((len(q) for q in quals), np.int64, n)
    assert n == len(quals) and (ls <= lmax).all() and (lq <= 65536).all()
    sb = np.frombuffer(b"".join(seqs), np.uint8)
    qb = np.frombuffer(b"".join(quals), np.uint8)
    isgc = np.concatenate([[0], np.cumsum((sb == 0x47) | (sb == 0x43), dtype=np.int64)])
    qcum = np.concatenate([[0], np.cumsum(qb, dtype=np.int64)])
    so = np.concatenate([[0], np.cumsum(ls)])
    qo = np.concatenate([[0], np.cumsum(lq)])
    gc = isgc[so[1:]] - isgc[so[:-1]]
    qs = qcum[qo[1:]] - qcum[qo[:-1]]
    st[0], st[1], st[2], st[3] = n, ls.sum(), gc.sum(), qs.sum()
    st[at[1]:at[2]] = np.bincount(ls, minlength=lmax + 1)
    gbin = np.where(ls > 0, (100 * gc) // np.maximum(ls, 1), 101)
    qbin = np.where(lq > 0, qs // np.maximum(lq, 1), 256)
    st[at[2]:at[3]] = np.bincount(gbin, minlength=102)
    st[at[3]:at[4]] = np.bincount(qbin, minlength=257)
    return st


def read_fastq(path):
    """(sequence, quality) of every record of a plain / gzip / BGZF FASTQ file: four lines per record, '\\n' or '\\r\\n'."""
    import gzip
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)  # (every member of a multi-member file)
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in raw.split(b"\n")]
    if lines and lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0
    return [(lines[i + 1], lines[i + 3]) for i in range(0, len(lines), 4)]
