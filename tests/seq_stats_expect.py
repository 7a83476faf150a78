"""What the per-record sequence statistics plan (kind 10) must compute, written from its table alone (plain numpy; no import of the
package, the library or the oracle).  s = a record's sequence bytes as the reader returns them (fasta_expect.records):

  totals       [3]         n_records, sum len(s), sum gc(s)
  composition  [256]       word b = number of sequence bytes equal to b, over all records
  length       [lmax + 2]  bin len(s) for len(s) <= lmax; bin lmax + 1 = every longer record
  length_log2  [32]        bin 0 = empty sequence; bin k = 2^(k-1) <= len(s) < 2^k
  gc_percent   [102]       bin floor(100 gc(s) / len(s)) as an exact integer; bin 101 = empty sequence

gc(s) counts the bytes 'G' and 'C', upper case only."""
import numpy as np

import fasta_expect

NAMES = ("totals", "composition", "length", "length_log2", "gc_percent")


def layout(lmax):
    """word offsets of the five sections, then the number of words"""
    assert 1 <= lmax <= 65536
    at = [0, 3, 3 + 256]
    at.append(at[2] + lmax + 2)
    at.append(at[3] + 32)
    at.append(at[4] + 102)
    return tuple(at)


def gc_count(s):
    return s.count(b"G") + s.count(b"C")


def expect(seqs, lmax):
    """the state of a list of sequences (bytes), record by record"""
    at = layout(lmax)
    st = np.zeros(at[5], np.int64)
    for s in seqs:
        n, gc = len(s), gc_count(s)
        st[0] += 1
        st[1] += n
        st[2] += gc
        for b in s:
            st[at[1] + b] += 1
        st[at[2] + (n if n <= lmax else lmax + 1)] += 1
        st[at[3] + n.bit_length()] += 1
        st[at[4] + (100 * gc // n if n else 101)] += 1
    return st


def expect_fast(seqs, lmax):
    """the same state, vectorised"""
    at = layout(lmax)
    st = np.zeros(at[5], np.int64)
    n = len(seqs)
    if n == 0:
        return st
    lens = np.fromiter((len(s) for s in seqs), np.int64, n)
    data = np.frombuffer(b"".join(seqs), np.uint8)
    is_gc = ((data == ord("G")) | (data == ord("C"))).astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(is_gc)])
    off = np.concatenate([[0], np.cumsum(lens)])
    gc = cum[off[1:]] - cum[off[:-1]]
    st[0], st[1], st[2] = n, int(lens.sum()), int(gc.sum())
    st[at[1]:at[2]] = np.bincount(data, minlength=256)
    st[at[2]:at[3]] = np.bincount(np.minimum(lens, lmax + 1), minlength=lmax + 2)
    log2 = np.zeros(n, np.int64)
    nz = lens > 0
    log2[nz] = np.floor(np.log2(lens[nz])).astype(np.int64) + 1  # (exact below 2^52)
    st[at[3]:at[4]] = np.bincount(log2, minlength=32)
    pct = np.full(n, 101, np.int64)
    pct[nz] = 100 * gc[nz] // lens[nz]
    st[at[4]:at[5]] = np.bincount(pct, minlength=102)
    return st


def sequences(text):
    """the sequence bytes of every record of a FASTA text"""
    return [r[2].encode("latin-1") for r in fasta_expect.records(text)]


def from_text(text, lmax):
    return expect_fast(sequences(text), lmax)


def identities(st, lmax):
    """the three identities of the table"""
    at = layout(lmax)
    return (st[at[1]:at[2]].sum() == st[1] and st[at[1] + ord("G")] + st[at[1] + ord("C")] == st[2]
            and all(st[at[k]:at[k + 1]].sum() == st[0] for k in (2, 3, 4)))
