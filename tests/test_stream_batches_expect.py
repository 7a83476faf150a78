"""CPU: tests/stream_batches_expect.py (the statement the stream-layer limits tests compare with) against the oracle's functions
for K2 / K3 / K4 / K5 / K6 / the within count, and against minmax_expect.py / read_stats_expect.py for K8 / K9, on tables of a few
hundred rows.  Where the oracle's function takes no bitmap for a column, the rows that are NULL there are taken out first: a NULL
operand fails every predicate."""
import numpy as np
import pytest

import minmax_expect
import read_stats_expect
import stream_batches_expect as S

PAD = np.zeros(64, np.uint8)  # (the oracle reads bitmaps in words)


def _bm(ok):
    return np.concatenate([np.packbits(np.asarray(ok, bool), bitorder="little"), PAD])


def _ok(rng, n, p=0.7):
    return rng.random(n) < p


@pytest.mark.parametrize("region", ["7:100-600", "7", "3:1-1", "X:250-10000"])
def test_k2_region_count(oracle, region):
    rng = np.random.default_rng(2)
    contigs = oracle.c2_contigs()
    n = 700
    chrom = rng.integers(0, len(contigs), n).astype(np.int32)
    chrom[::3] = contigs.index(region.split(":")[0])
    pos = rng.integers(1, 1000, n).astype(np.int64)
    name, a, b = oracle.parse_region(region)
    pos[::6] = a  # (rows on the region's first position, whatever its width)
    for cv, pv in ((np.ones(n, bool), np.ones(n, bool)), (_ok(rng, n), _ok(rng, n))):
        want, _ = oracle.c2_region_count(chrom, pos, contigs, region, _bm(cv), _bm(pv))
        got, sums = S.expect("k2", (contigs.index(name), a, b), [(chrom, cv), (pos, pv)])
        assert want > 0 and got.dtype == np.int64 and got.tolist() == [want] and sums.size == 0


def _intervals(rng, n, n_refs):
    ref = rng.integers(0, n_refs, n).astype(np.int32)
    start = rng.integers(1, 5000, n).astype(np.int64)
    return ref, start, start + rng.integers(0, 300, n)


def test_k6_overlap_and_within_count(oracle):
    rng = np.random.default_rng(6)
    names = oracle.c3_refs()[:5]
    n = 900
    ref, start, end = _intervals(rng, n, len(names))
    for valid in ([np.ones(n, bool)] * 3, [_ok(rng, n), _ok(rng, n), _ok(rng, n)]):
        cols = list(zip((ref, start, end), valid))
        bms = [_bm(v) for v in valid]
        for rid, a, b in ((2, 1000, 3000), (0, 1, None), (4, 4999, 4999), (1, 2500, 2500)):
            region = names[rid] + (f":{a}-{b}" if b is not None else "")
            want = oracle.c6_overlap_count(ref, bms[0], start, bms[1], end, bms[2], names, region)
            assert S.expect("k6", (rid, a, b), cols)[0].tolist() == [want] and want > 0
        for rid, after, before in ((2, 1000, 3000), (0, 0, None), (3, 4000, 4400), (1, 0, 2)):
            want = oracle.c7_within_count(ref, bms[0], start, bms[1], end, bms[2], names, names[rid], after, before)
            assert S.expect("k7", (rid, after, before), cols)[0].tolist() == [want]
    # at its borders: a record that ends ON the region's start overlaps it and is not within it
    one = [(np.array([0], np.int32), [True]), (np.array([10], np.int64), [True]), (np.array([20], np.int64), [True])]
    assert S.expect("k6", (0, 20, 30), one)[0][0] == 1 and S.expect("k6", (0, 21, 30), one)[0][0] == 0
    assert S.expect("k6", (0, 1, 10), one)[0][0] == 1 and S.expect("k6", (0, 1, 9), one)[0][0] == 0
    assert S.expect("k7", (0, 9, 21), one)[0][0] == 1 and S.expect("k7", (0, 10, 21), one)[0][0] == 0 and S.expect("k7", (0, 9, 20), one)[0][0] == 0


@pytest.mark.parametrize("where", [(1284, 0, 30), (4, 4, -1), (0, 0, 0), (1028, 1024, 60)])
def test_k3_flag_mapq_group_count(oracle, where):
    rng = np.random.default_rng(3)
    refs = oracle.c3_refs()
    R, n = len(refs), 1200
    flag = rng.choice(np.array([0, 4, 16, 99, 147, 256, 1024, 1028, 1284, 2048], np.int32), n)
    mapq = rng.integers(0, 61, n).astype(np.uint8)
    ref = rng.integers(0, R, n).astype(np.int32)
    fv, mv, rv = _ok(rng, n, 0.9), _ok(rng, n), _ok(rng, n)
    got, sums = S.expect("k3", (*where, R), [(flag, fv), (mapq, mv), (ref, rv)])
    keep = np.flatnonzero(fv)  # the oracle's flag has no bitmap: a NULL flag fails the predicate, so those rows leave first
    want, _ = oracle.c3_flag_mapq_group_count(flag[keep], np.concatenate([mapq[keep], PAD]), _bm(mv[keep]), ref[keep], _bm(rv[keep]), refs, *where)
    assert np.array_equal(got, want) and got[R] > 0 and got.sum() < n and sums.size == 0


@pytest.mark.parametrize("ints", [False, True])
@pytest.mark.parametrize("op", [">", ">=", "<", "<=", "=", "!="])
def test_k4_cmp_avg_by_group(oracle, op, ints):
    rng = np.random.default_rng(4)
    filters = oracle.c4_filters()
    G, n = len(filters), 1000
    g = rng.integers(0, G, n).astype(np.int32)
    xv, yv = _ok(rng, n), _ok(rng, n)
    if ints:  # small integers: the same values as float32 columns are what the oracle (Float32 only) is asked
        x, y, thr = rng.integers(-3, 4, n).astype(np.int32), rng.integers(0, 1000, n).astype(np.int32), 1.0
    else:
        x = rng.choice(np.array([0.0, 0.01, 0.25, 0.5, 1.0, -1.0], np.float32), n)
        # (0.01f < 0.01: the column is widened, not the literal -- which also means no row EQUALS 0.01)
        y, thr = (rng.integers(0, 8000, n) / 8.0).astype(np.float32), 0.25 if op == "=" else 0.01
    counts, sums = S.expect("k4", (op, thr, G, ints, ints), [(x, xv), (y, yv), (g, np.ones(n, bool))])
    s, cn, cr, _ = oracle.c4_cmp_avg_by_group(x.astype(np.float32), _bm(xv), y.astype(np.float32), _bm(yv), g, filters, thr, op)
    assert np.array_equal(counts[:G], cn) and np.array_equal(counts[G:], cr) and cr.sum() > cn.sum() > 0
    assert np.array_equal(sums, s)  # eighths / integers: exact in any order
    with pytest.raises(AssertionError):
        S.expect("k4", (op, thr, G, ints, ints), [(x, xv), (y, yv), (g, xv)])


def _lines(rng, n, lo, hi, alphabet=None):
    out = []
    for k in rng.integers(lo, hi, n):
        b = rng.integers(33, 75, int(k), dtype=np.uint8) if alphabet is None else np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), int(k))]
        out.append(b.tobytes())
    return out


def test_k5_qual_pos_hist(oracle):
    rng = np.random.default_rng(5)
    for lo, hi, lmax in ((100, 101, 100), (0, 40, 39), (0, 1, 7), (1, 160, 200)):
        quals = _lines(rng, 300, lo, hi)
        off = np.concatenate([[0], np.cumsum([len(q) for q in quals])]).astype(np.int32)
        data = np.frombuffer(b"".join(quals) + b"\0" * 64, np.uint8)
        want, _ = oracle.c5_qual_pos_hist(off, data, lmax)
        got, sums = S.expect("k5", (lmax,), [(quals, np.ones(300, bool))])
        assert np.array_equal(got.reshape(lmax, 256), want) and got.sum() == off[-1] and sums.size == 0


def test_k8_and_k9_are_the_existing_statements():
    rng = np.random.default_rng(8)
    n, G = 500, 7
    x, y = rng.choice(np.array([0.0, 0.25, 1.0], np.float32), n), rng.standard_normal(n).astype(np.float32)
    g, xv, yv = rng.integers(0, G, n).astype(np.int32), _ok(rng, n), _ok(rng, n)
    got, sums = S.expect("k8", ("<=", 0.25, G, False, False), [(x, xv), (y, yv), (g, np.ones(n, bool))])
    assert np.array_equal(got, minmax_expect.expect(x, xv, y, yv, g, G, "<=", 0.25)) and sums.size == 0
    a, b = S.expect("k8", (">", 0.0, G, False, False), [(x[:200], xv[:200]), (y[:200], yv[:200]), (g[:200], np.ones(200, bool))]), \
        S.expect("k8", (">", 0.0, G, False, False), [(x[200:], xv[200:]), (y[200:], yv[200:]), (g[200:], np.ones(300, bool))])
    whole = S.expect("k8", (">", 0.0, G, False, False), [(x, xv), (y, yv), (g, np.ones(n, bool))])
    assert np.array_equal(S.fold("k8", (">", 0.0, G, False, False), [a, b])[0], whole[0])
    seqs, quals = _lines(rng, 200, 0, 60, b"ACGTNacgt"), _lines(rng, 200, 0, 70)
    got, _ = S.expect("k9", (64,), [(seqs, np.ones(200, bool)), (quals, np.ones(200, bool))])
    assert np.array_equal(got, read_stats_expect.expect(zip(seqs, quals), 64))


def test_take_and_fold():
    cols = [(np.arange(10, dtype=np.int32), np.arange(10) % 2 == 0), ([b"a", b"", b"ccc"] + [b"x"] * 7, np.ones(10, bool))]
    t = S.take(cols, np.array([2, 0, 9]))
    assert t[0][0].tolist() == [2, 0, 9] and t[0][1].tolist() == [True, True, False] and t[1][0] == [b"ccc", b"a", b"x"]
    a = (np.array([1, 2], np.int64), np.array([0.5]))
    got = S.fold("k4", (">", 0.0, 1, False, False), [a, a, a])
    assert got[0].tolist() == [3, 6] and got[1].tolist() == [1.5]
