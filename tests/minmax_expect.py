"""Plain-numpy statement of MIN / MAX by group (plan kind 8) for the tests: the packed state
[count_y[G]] [count_rows[G]] [minw[G]] [maxw[G]] from host columns.  Independent of the library (no decode helper, no
oracle): keys come from viewing float32 as int32, the per-group maxima from np.maximum.at, the predicate from a float64
comparison (Float32 x) or an exact integer one (Int32 x)."""
import numpy as np

OPS = {">": np.greater, ">=": np.greater_equal, "<": np.less, "<=": np.less_equal, "=": np.equal, "!=": np.not_equal}

# the values the encoding has to get right: signed zeros, infinities, the largest and the smallest finite magnitudes, and the
# four NaNs at the ends of IEEE totalOrder (quiet NaN and all-ones payload, both signs)
SPECIAL_F32_BITS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001,
                             0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32)
SPECIAL_I32 = np.array([-2**31, -1, 0, 2**31 - 1], np.int32)


def ukey(values, is_int):
    """unsigned-ordered 32-bit key (as uint64) of an int32 array or of a float32 array's bit patterns"""
    b = np.ascontiguousarray(values).view(np.int32).astype(np.int64)
    ub = b & 0xFFFFFFFF
    if is_int:
        return (ub ^ 0x80000000).astype(np.uint64)
    return np.where(b < 0, ub ^ 0xFFFFFFFF, ub ^ 0x80000000).astype(np.uint64)


def min_word(values, is_int):
    return (np.uint64(1) + (np.uint64(0xFFFFFFFF) - ukey(values, is_int))).astype(np.int64)


def max_word(values, is_int):
    return (np.uint64(1) + ukey(values, is_int)).astype(np.int64)


def passes(x, x_valid, op, thr, x_is_int=False):
    """x valid AND x <op> thr.  Float32 x is widened to float64; Int32 x is compared as int64 (against a float literal:
    every int32 is exact in float64).  The caller keeps NaN and -0.0 out of x and thr, where IEEE and totalOrder differ."""
    xx = np.asarray(x).astype(np.int64) if x_is_int else np.asarray(x, np.float32).astype(np.float64)
    return np.asarray(x_valid, bool) & OPS[op](xx, thr)


def expect(x, x_valid, y, y_valid, gid, n_groups, op, thr, x_is_int=False, y_is_int=False):
    """the packed int64 state of 4 * n_groups words"""
    G = n_groups
    p = passes(x, x_valid, op, thr, x_is_int)
    gid = np.asarray(gid, np.int64)
    q = p & np.asarray(y_valid, bool)
    st = np.zeros(4 * G, np.int64)
    np.add.at(st[0:G], gid[q], 1)
    np.add.at(st[G:2 * G], gid[p], 1)
    yq = np.asarray(y)[q]
    np.maximum.at(st[2 * G:3 * G], gid[q], min_word(yq, y_is_int))
    np.maximum.at(st[3 * G:4 * G], gid[q], max_word(yq, y_is_int))
    return st


def fold(states, n_groups):
    """fold of several packed states: counts add, the two extreme planes take the max"""
    s = np.stack(states)
    G = n_groups
    return np.concatenate([s[:, :2 * G].sum(0), s[:, 2 * G:].max(0)])


def decode(words, is_min, is_int):
    """(values, valid) from state words -- numpy's own inverse of the key, for tests that compare VALUES"""
    w = np.asarray(words, np.int64)
    valid = w != 0
    k = np.where(valid, w - 1, 0).astype(np.uint64)
    u = (np.uint64(0xFFFFFFFF) - k) if is_min else k
    if is_int:
        bits = u ^ np.uint64(0x80000000)
    else:
        bits = np.where(u & np.uint64(0x80000000), u ^ np.uint64(0x80000000), u ^ np.uint64(0xFFFFFFFF))
    bits = bits.astype(np.uint32)
    return (bits.view(np.int32) if is_int else bits.view(np.float32)), valid
