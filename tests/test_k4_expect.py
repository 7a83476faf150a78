"""CPU: tests/k4_expect.py (the reference the K4 GPU tests compare with) on inputs worked by hand."""
import numpy as np

import k4_expect as E


def test_hand_worked_f32():
    #            row   0     1     2     3      4     5     6      7
    x = np.array([0.5, 0.25, 0.3, 0.01, 1.0, 0.26, -1.0, 0.2], np.float32)
    xok = np.array([1, 1, 0, 1, 1, 1, 1, 1], bool)
    y = np.array([1.5, 9.0, 2.0, 4.0, -0.125, 8.0, 3.0, 0.25], np.float32)
    yok = np.array([1, 1, 1, 1, 1, 0, 1, 1], bool)
    gid = np.array([2, 2, 2, 0, 2, 4, 0, 4], np.int32)
    # x > 0.25 in float64: rows 0, 2, 4 and 5 ; row 2's x is NULL
    k = E.keep(x, ">", 0.25, xok)
    assert k.tolist() == [True, False, False, False, True, True, False, False]
    cnn, crow, sums = E.expect(gid, 5, k, y, yok)
    assert crow.tolist() == [0, 0, 2, 0, 1]   # rows 0, 4 -> group 2; row 5 -> group 4
    assert cnn.tolist() == [0, 0, 2, 0, 0]    # row 5's y is NULL
    assert sums.tolist() == [0.0, 0.0, 1.375, 0.0, 0.0]
    assert np.array_equal(sums.view(np.int64)[[0, 1, 3, 4]], np.zeros(4, np.int64))  # +0.0, not -0.0
    # without bitmaps row 2 passes too and row 5 counts
    cnn, crow, sums = E.expect(gid, 5, E.keep(x, ">", 0.25), y)
    assert crow.tolist() == [0, 0, 3, 0, 1] and cnn.tolist() == [0, 0, 3, 0, 1] and sums.tolist() == [0.0, 0.0, 3.375, 0.0, 8.0]
    # != : every valid row but the 0.25 itself
    assert E.keep(x, "!=", 0.25, xok).tolist() == [True, False, False, True, True, True, True, True]
    w = E.state_words(cnn, crow, sums)
    assert w.dtype == np.int64 and w.size == 15 and w[:5].tolist() == [0, 0, 3, 0, 1] and w[12] == np.float64(3.375).view(np.int64)


def test_the_column_is_widened_not_the_literal():
    # 0.01f is 0.00999999977648258...: below the float64 literal 0.01, so `x > 0.01` is false and `x != 0.01` true
    x = np.array([0.01], np.float32)
    assert not E.keep(x, ">", 0.01)[0] and not E.keep(x, ">=", 0.01)[0] and E.keep(x, "!=", 0.01)[0] and E.keep(x, "<", 0.01)[0]


def test_hand_worked_i32():
    x = np.array([0, 1, -1, 2**31 - 1, -2**31, 16777217], np.int32)  # 16777217 is not a float32
    assert E.keep(x, ">", 0.25).tolist() == [False, True, False, True, False, True]
    assert E.keep(x, "==", 16777217).tolist() == [False] * 5 + [True]
    assert E.keep(x, "!=", 16777216).tolist() == [True] * 6
    y = np.array([4096, -4096, 7, 1, 2, 3], np.int32)
    cnn, crow, sums = E.expect(np.array([1, 1, 0, 0, 1, 0], np.int32), 2, E.keep(x, ">", 0.25), y)
    assert cnn.tolist() == [2, 1] and crow.tolist() == [2, 1] and sums.tolist() == [4.0, -4096.0]


def test_nan_and_empty():
    y = np.array([np.nan, 1.0], np.float32)
    kept = np.array([True, True])
    _, _, sums = E.expect(np.array([1, 0], np.int32), 3, kept, y)
    assert np.isnan(sums[1]) and sums[0] == 1.0 and sums[2] == 0.0
    cnn, crow, sums = E.expect(np.zeros(0, np.int32), 2, np.zeros(0, bool), np.zeros(0, np.float32))
    assert cnn.tolist() == [0, 0] and crow.tolist() == [0, 0] and sums.view(np.int64).tolist() == [0, 0]
    assert E.bits([1, 0, 0, 0, 0, 0, 0, 0, 1]).tolist() == [1, 1]
