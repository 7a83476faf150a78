"""No GPU: the three numpy references of the window plan (kind 13) -- per-base pileup, sorted starts and ends, and the E / D state the
kernel's adds define -- agree with each other, at every window seam and at both ends of a contig."""
import numpy as np
import pytest

import window_bases_expect as E

LENGTHS = [1, 5, 999, 1000, 1001, 2500]


def random_rows(rng, n, n_refs, span):
    ref = rng.integers(-1, n_refs + 1, n).astype(np.int32)
    start = rng.integers(-20, span + 30, n)  # below 1 and beyond the end
    end = start + rng.integers(-3, 160, n)   # some inverted
    rv, sv, ev = (rng.random(n) < 0.95 for _ in range(3))
    return ref, start, end, rv, sv, ev


@pytest.mark.parametrize("W", [1, 3, 7, 64, 1000])
def test_the_three_references_agree(W):
    rng = np.random.default_rng(W)
    contigs = [(2 * c + 1, ln) for c, ln in enumerate(LENGTHS)]  # ids 1, 3, .., 11: the even ids are elsewhere
    rows = random_rows(rng, 4000, 12, 2600)
    totals, bases = E.expect(contigs, W, *rows)
    assert totals.sum() == 4000 and totals.min() > 0
    assert bases.size == E.offsets(contigs, W)[-1] == sum((ln - 1) // W + 1 for ln in LENGTHS)
    fast = E.expect_fast(contigs, W, *rows)
    assert fast[0].tolist() == totals.tolist() and fast[1].tolist() == bases.tolist()
    st = E.expect_state(contigs, W, *rows)
    assert st.size == 4 + 2 * bases.size and st[:4].tolist() == totals.tolist()
    assert E.decode(contigs, W, st).tolist() == bases.tolist()
    assert bases.sum() > 0 and bases.min() >= 0
    # no window holds more than its length times the rows
    lens = np.array([e - s + 1 for _, s, e in E.windows(contigs, W)])
    assert (bases <= lens * totals[0]).all() and lens.min() >= 1


def test_one_row_by_hand():
    contigs = [(0, 35)]
    assert E.windows(contigs, 10) == [(0, 1, 10), (0, 11, 20), (0, 21, 30), (0, 31, 35)]
    for row, want in [((3, 7), [5, 0, 0, 0]), ((10, 11), [1, 1, 0, 0]), ((5, 25), [6, 10, 5, 0]), ((-5, 135), [10, 10, 10, 5]),
                      ((36, 40), [0, 0, 0, 0]), ((-3, 0), [0, 0, 0, 0]), ((31, 35), [0, 0, 0, 5]), ((1, 10), [10, 0, 0, 0])]:
        for f in (E.expect, E.expect_fast):
            totals, bases = f(contigs, 10, [0], [row[0]], [row[1]])
            assert totals.tolist() == [1, 0, 0, 0] and bases.tolist() == want, (row, f.__name__)
        assert E.decode(contigs, 10, E.expect_state(contigs, 10, [0], [row[0]], [row[1]])).tolist() == want
    # [5, 25]: E[0] += 6, E[2] += 5, D[1] += 1, D[2] -= 1
    st = E.expect_state(contigs, 10, [0], [5], [25])
    assert st.tolist() == [1, 0, 0, 0, 6, 0, 5, 0, 0, 1, -1, 0]
