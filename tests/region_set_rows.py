"""What the GPU tests of the two region-set plans (kinds 11 and 12) share: interval columns on the device, one launch over them, and
random rows and regions.  A test file subclasses Cols with `E` = its kind's reference (region_set_expect / region_bases_expect)."""
import numpy as np

from region_set_expect import OPEN_END, pack_bits


def full(regions):
    return [(c, s, OPEN_END if e is None else e) for c, s, e in regions]


class Cols:
    """three host columns (+ optional validity) on the device; `shift` = elements in front of each column's first row"""

    E = None  # the reference module: expect / expect_fast

    def __init__(self, ctx, ref, start, end, rv=None, sv=None, ev=None, shift=(0, 0, 0)):
        self.host = (np.asarray(ref, np.int32), np.asarray(start, np.int64), np.asarray(end, np.int64))
        self.valid = (rv, sv, ev)
        self.n = len(self.host[0])
        self.bufs, self.ptrs = [], []
        for a, k in zip(self.host, shift):
            b = ctx.to_device(np.concatenate([np.zeros(k, a.dtype), a, np.zeros(8, a.dtype)]))
            self.bufs.append(b)
            self.ptrs.append(b.ptr + k * a.dtype.itemsize)
        self.vbufs = [None if v is None else ctx.to_device(np.concatenate([pack_bits(v), np.zeros(64, np.uint8)])) for v in self.valid]

    def columns(self, lo=0, hi=None):
        """(values, validity, offsets) triples of rows [lo, hi); lo a multiple of 8"""
        assert lo % 8 == 0
        return [(p + lo * a.dtype.itemsize, None if v is None else v.ptr + lo // 8, None) for p, a, v in zip(self.ptrs, self.host, self.vbufs)]

    def expect(self, regions, fast=False):
        return (self.E.expect_fast if fast else self.E.expect)(full(regions), *self.host, *self.valid)


def launch(ctx, plan, cols, overwrite=True, d_state=None, lo=0, hi=None):
    hi = cols.n if hi is None else hi
    d_state = d_state if d_state is not None else ctx.zeros(np.int64, plan.n_i64)
    plan.launch(cols.columns(lo), hi - lo, d_state, overwrite=overwrite)
    ctx.sync()
    return d_state


def random_rows(rng, n, n_refs=6, span=2000, null=0.05, inverted=0.02):
    ref = rng.integers(-1, n_refs + 1, n).astype(np.int32)
    start = rng.integers(1, span, n)
    end = start + rng.integers(0, 150, n)
    inv = rng.random(n) < inverted
    end[inv] = start[inv] - rng.integers(1, 5, int(inv.sum()))
    return ref, start, end, rng.random(n) >= null, rng.random(n) >= null, rng.random(n) >= null


def random_regions(rng, m, contigs, span=2000, width=300):
    out = []
    for _ in range(m):
        s = int(rng.integers(1, span))
        out.append((int(rng.choice(contigs)), s, s + int(rng.integers(0, width))))
    return out
