"""cmp_avg_by_group (K4) in plain numpy, int64 / float64:

    WHERE CAST(x AS DOUBLE) <op> literal   SELECT g, COUNT(y), COUNT(*), SUM(CAST(y AS DOUBLE)) GROUP BY g

A Float32 x is widened to float64 and compared with the literal; an Int32 x is compared as the integer it is (every int32 is exact
in float64, so one float64 comparison of the widened integer says the same as the integer comparison).  A NULL x never passes.  (The tests keep NaN out of x: the device
orders a NaN x by totalOrder, above every number, which numpy's comparisons do not.)
COUNT(*) counts the passing rows of a group, COUNT(y) and the sum those of them whose y is not NULL.  The tests keep y a multiple
of 1/8 with |y| <= 4096 (or an Int32 with |y| <= 4096): a float64 sum of fewer than 2^37 such values is exact in any order, so the
comparison with the device is on the bits."""
import numpy as np

OPS = {">": np.greater, ">=": np.greater_equal, "<": np.less, "<=": np.less_equal, "==": np.equal, "!=": np.not_equal}


def keep(x, op, literal, xok=None):
    """the row predicate; xok: validity of x as booleans, None = no bitmap"""
    x = np.asarray(x)
    wide = x.astype(np.int64).astype(np.float64) if x.dtype.kind == "i" else x.astype(np.float64)
    k = OPS[op](wide, np.float64(literal))
    return k if xok is None else k & np.asarray(xok, bool)


def expect(gid, n_groups, kept, y, yok=None):
    """(COUNT(y), COUNT(*), sum) per group: int64, int64, float64; groups nothing contributed to hold 0, 0, +0.0"""
    gid = np.asarray(gid)
    live = kept if yok is None else kept & np.asarray(yok, bool)
    crow = np.bincount(gid[kept], minlength=n_groups).astype(np.int64)
    cnn = np.bincount(gid[live], minlength=n_groups).astype(np.int64)
    sums = np.bincount(gid[live], weights=np.asarray(y)[live].astype(np.float64), minlength=n_groups).astype(np.float64)
    return cnn, crow, sums


def state_words(cnn, crow, sums):
    """the packed state of a plan: [COUNT(y)[G]] [COUNT(*)[G]] [sum[G] as float64 bits], 3 * G int64 words"""
    return np.concatenate([cnn.astype(np.int64), crow.astype(np.int64), np.ascontiguousarray(sums, np.float64).view(np.int64)])


def bits(ok):
    """an Arrow validity bitmap from booleans"""
    return np.packbits(np.asarray(ok, np.uint8), bitorder="little")
