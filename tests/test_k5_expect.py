"""The reference of the K5 limits tests (tests/k5_expect.py) checked on its own: against a triple Python loop on tiny inputs,
against the oracle the older fuzz test uses, and its table of length classes against the kernel's stated rules.  No GPU."""
import numpy as np
import pytest

import k5_expect as E


def loops(starts, ends, data, lmax):
    h = np.zeros((lmax, 256), np.int64)
    for p in range(lmax):
        for b in range(256):
            for r in range(len(starts)):
                if p < ends[r] - starts[r] and data[starts[r] + p] == b:
                    h[p, b] += 1
    return h


DATA = bytes([0, 127, 128, 255, 33, 74, 0, 255, 128, 127, 65, 66])
TINY = [
    # (starts, ends, lmax)
    ([], [], 1),                                      # no reads
    ([0], [0], 1),                                    # one empty read
    ([3, 3, 3], [3, 3, 3], 2),                        # only empty reads
    ([0], [4], 4),                                    # a read of exactly lmax: bytes 0 / 127 / 128 / 255
    ([0], [4], 6),                                    # ... and below it
    ([0, 4, 8], [4, 8, 12], 4),                       # an Arrow column
    ([0, 4, 4, 8], [4, 4, 8, 12], 5),                 # ... with an empty read inside
    ([0, 5, 9], [4, 8, 12], 4),                       # gaps
    ([0, 2, 1], [6, 8, 4], 6),                        # overlapping
    ([8, 4, 0], [12, 8, 4], 4),                       # out of order
    ([6, 6, 6, 6], [9, 9, 9, 9], 3),                  # one view repeated
    ([11, 0, 5, 5, 2], [12, 1, 5, 12, 9], 7),         # ragged, overlapping, out of order, empty, a single byte at either end
    ([0], [12], 12),                                  # the whole buffer
]


@pytest.mark.parametrize("case", range(len(TINY)))
def test_hist_equals_the_triple_loop(case):
    starts, ends, lmax = TINY[case]
    data = np.frombuffer(DATA, np.uint8)
    got = E.hist(starts, ends, data, lmax)
    assert got.shape == (lmax, 256) and got.dtype == np.int64
    assert np.array_equal(got, loops(starts, ends, data, lmax))
    assert got.sum() == sum(e - s for s, e in zip(starts, ends))


def test_a_read_longer_than_lmax_is_refused():
    data = np.frombuffer(DATA, np.uint8)
    assert E.hist([0], [4], data, 4)[3, 255] == 1
    with pytest.raises(ValueError, match="longer than lmax"):
        E.hist([0], [5], data, 4)
    with pytest.raises(ValueError, match="longer than lmax"):
        E.hist([0, 4, 0], [0, 8, 5], data, 4)
    with pytest.raises(ValueError):
        E.hist([4], [3], data, 4)
    with pytest.raises(ValueError):
        E.hist([10], [13], data, 4)


def test_column_helper():
    rng = np.random.default_rng(5)
    for shift in (0, 1, 17):
        off, data = E.column([3, 0, 5], shift, rng=rng)
        assert off.dtype == np.int32 and off.tolist() == [shift, shift + 3, shift + 3, shift + 8]
        assert data.dtype == np.uint8 and data.size == shift + 8 + 320
        assert (data[:shift] == 222).all() and (data[shift + 8:] == 223).all()
        assert ((data[shift:shift + 8] >= 33) & (data[shift:shift + 8] < 75)).all()
        h = E.hist_column(off, data, 5)
        assert h.sum() == 8 and h[:, 222].sum() == 0 and h[:, 223].sum() == 0 and h[3:].sum() == 2
    off, data = E.column([2, 2], 3, payload=lambda n: np.full(n, 255, np.uint8))
    assert data[3:7].tolist() == [255] * 4
    off, data = E.column([], 4)
    assert off.tolist() == [4] and data.size == 324


@pytest.mark.parametrize("seed", [0, 1])
def test_hist_equals_the_oracle(oracle, seed):
    """the new reference and the one tests/test_gpu_k5_fuzz.py compares with agree.  (The oracle's hash aggregate holds 32768
    distinct (position, byte) keys per thread -- oracle/exon_oracle.c, cap = 1 << 16, half full -- so the alphabets are kept to
    lmax x |alphabet| < 32768: 150 x 100 and 700 x 40.)"""
    rng = np.random.default_rng(77 + seed)
    lmax, nsym = ((150, 100), (700, 40))[seed]
    alphabet = np.concatenate([[0, 127, 128, 255], rng.choice(np.arange(1, 255), nsym - 4, replace=False)]).astype(np.uint8)
    assert lmax * len(set(alphabet.tolist()) | {0, 127, 128, 255}) < 32768
    lens = rng.integers(0, lmax + 1, 3000)
    lens[:3] = (0, lmax, lmax - 1)
    off, data = E.column(lens, (0, 13)[seed], payload=lambda n: alphabet[rng.integers(0, nsym, n)])
    want = oracle.c5_qual_pos_hist(off, data, lmax)[0]
    got = E.hist_column(off, data, lmax)
    assert np.array_equal(got, want.reshape(lmax, 256)) and got.sum() == lens.sum()


def test_length_classes():
    assert E.B_LENGTHS == [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28]
    assert {L for L in range(1, 311) if E.length_class(L) == "B"} == set(E.B_LENGTHS)
    for L in range(1, 401):
        c = E.length_class(L)
        assert c == E.CLASSES[L]
        if L > 310:
            assert c == "G"
        elif L not in E.B_LENGTHS:
            assert L >= 9 and c in ("A1", "A2", "A4") and E.period(L) >= 8
    # the three period rules: L odd -> L, L = 2 (mod 4) -> L / 2, L = 0 (mod 4) -> L / 4
    assert [E.period(L) for L in (9, 15, 18, 30, 32, 60, 17, 31, 34, 62, 64, 124, 33, 66, 128)] == [9, 15, 9, 15, 8, 15, 17, 31, 17, 31, 16, 31, 33, 33, 32]
    assert [E.length_class(L) for L in (9, 11, 15, 18, 30, 32, 60, 36)] == ["A4"] * 8
    assert [E.length_class(L) for L in (17, 31, 34, 62, 64, 124, 100)] == ["A2"] * 7  # (100: P = 25, the benchmark's length)
    assert [E.length_class(L) for L in (33, 63, 65, 66, 101, 127, 128, 129, 150, 151, 250, 251, 255, 256, 257, 301, 309, 310)] == ["A1"] * 18
    assert [E.length_class(L) for L in (0, 311, 312, 400)] == ["G"] * 4


def test_path_a_table_holds_every_length():
    """copies x 4 ceil(L / 4) slots fit the 5 planes x 64 columns of path A's table (K5_A_WORDS / 128)"""
    worst = 0
    for L in range(1, 311):
        if E.length_class(L).startswith("A"):
            assert E.slots(L) <= E.A_SLOTS, L
            worst = max(worst, E.slots(L))
    assert worst > 256  # the bound is not idle: some length needs the fifth plane
