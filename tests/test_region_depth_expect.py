"""No GPU: the numpy references of the region-set depth plan (kind 14) -- per-base pileup, sorted starts and ends, and the D state the
kernel's adds define -- agree with each other on random region sets and rows, and every contig's bins sum to 0."""
import numpy as np
import pytest

import region_depth_expect as E

THR = [1, 2, 5, 10]


def random_set(rng, m, contigs=(1, 3, 5), span=400, width=40):
    out = []
    for _ in range(m):
        s = int(rng.integers(1, span))
        out.append((int(rng.choice(contigs)), s, s + int(rng.integers(0, width))))
    return out


def random_rows(rng, n, n_refs=7, span=460):
    ref = rng.integers(-1, n_refs + 1, n).astype(np.int32)
    start = rng.integers(-20, span, n)      # below 1 and beyond every target
    end = start + rng.integers(-3, 90, n)   # some inverted
    rv, sv, ev = (rng.random(n) < 0.95 for _ in range(3))
    return ref, start, end, rv, sv, ev


@pytest.mark.parametrize("seed", range(12))
def test_decode_of_the_expected_state_is_the_pileup(seed):
    rng = np.random.default_rng(seed)
    regions = random_set(rng, int(rng.integers(1, 40)))
    rows = random_rows(rng, 200 if seed % 2 else 3000)
    totals, depth, bases, ge = E.expect(regions, THR, *rows)
    assert totals.sum() == len(rows[0])
    fast = E.expect(regions, THR, *rows, fast=True)
    assert all(np.array_equal(a, b) for a, b in zip(fast, (totals, depth, bases, ge)))
    st = E.expect_state(regions, *rows)
    at = E.layout(regions)
    assert st.size == at[2] and st[:4].tolist() == totals.tolist()
    d, b, g = E.decode(regions, THR, st)
    assert np.array_equal(d, depth) and np.array_equal(b, bases) and np.array_equal(g, ge)
    assert depth.size == at[2] - 4 - len(E.merged(regions)) and depth.min() >= 0
    # every contig's bins sum to 0 modulo 2^64, so the running sum of the whole section is 0 at every terminator
    run = E.running(regions, st)
    ends = E.doffs(regions)[1:] + [at[2] - 4]
    assert all(run[x - 1] == 0 for x in ends)
    # ge falls along the thresholds and stays within the region
    assert (np.diff(ge, axis=1) <= 0).all()
    assert (ge[:, 0] <= [e - s + 1 for _, s, e in regions]).all()
    assert (bases >= ge.sum(axis=1) * 0).all() and bases.sum() >= ge[:, 0].sum()


def test_merging_and_bins_by_hand():
    assert E.merged([(0, 11, 20), (0, 21, 30)]) == [[(11, 30)]]             # abutting
    assert E.merged([(0, 11, 20), (0, 31, 40)]) == [[(11, 20), (31, 40)]]   # a gap
    assert E.merged([(0, 11, 40), (0, 15, 20)]) == [[(11, 40)]]             # nested
    assert E.merged([(7, 5, 9), (2, 1, 1), (7, 5, 9)]) == [[(5, 9)], [(1, 1)]]  # duplicate; contigs by first appearance
    assert E.layout([(0, 11, 20), (0, 31, 40)]) == (0, 4, 4 + 21)
    assert E.intervals([(7, 5, 9), (2, 1, 1), (7, 20, 21)]) == [(0, 5, 9, 0), (0, 20, 21, 5), (1, 1, 1, 8)]
    iv = [(11, 20), (31, 40)]
    xs = [-2**63, 0, 10, 11, 12, 20, 21, 30, 31, 40, 41, 2**63 - 1]
    assert E.below(iv, xs).tolist() == [0, 0, 0, 1, 2, 10, 10, 10, 11, 20, 20, 20]


def test_one_row_by_hand():
    regions = [(0, 11, 20), (0, 31, 40)]
    for row, want in [((15, 35), (4, 10 + 5)), ((21, 30), None), ((1, 100), (0, 20)), ((20, 31), (9, 11)), ((-2**63, 2**63 - 1), (0, 20))]:
        st = E.expect_state(regions, [0], [row[0]], [row[1]])
        d = [0] * 21
        if want is not None:
            d[want[0]], d[want[1]] = 1, -1
        assert st.tolist() == [1, 0, 0, 0] + d, row
    totals, depth, bases, ge = E.expect(regions, [1, 2], [0, 0], [15, 18], [35, 19])
    assert depth.tolist() == [0] * 4 + [1, 1, 1, 2, 2, 1] + [1] * 5 + [0] * 5
    assert bases.tolist() == [8, 5] and ge.tolist() == [[6, 2], [5, 0]]
