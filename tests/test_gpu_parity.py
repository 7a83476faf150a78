"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

Bit-exact for counts / interval hits / histograms; <= 1e-6 relative for f64 sums (north_star tolerance;
in practice ~1e-15: only the association order of the f64 adds differs).
"""
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-6


def bits(bm, n):
    return np.unpackbits(bm, bitorder="little")[:n].astype(bool)


# ---- the device generators are bit-identical to the oracle's ----------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 1000, 100_003])
def test_generators_match_oracle(ctx, oracle, n):
    c, p = ctx.gen_c2(2, n)
    oc, op = oracle.gen_c2(2, n)
    assert np.array_equal(c.to_host(), oc) and np.array_equal(p.to_host(), op)
    lo = 4096
    f, mq, mv, ref, rv = ctx.gen_c3(3, lo, lo + n)
    of, omq, omv, oref, orv = oracle.gen_c3(3, lo, lo + n)
    nb = (n + 7) // 8
    assert np.array_equal(f.to_host(), of) and np.array_equal(mq.to_host(n), omq)
    assert np.array_equal(mv.to_host(nb), omv) and np.array_equal(ref.to_host(), oref)
    assert np.array_equal(rv.to_host(nb), orv)
    af, av, q, qv, fid = ctx.gen_c4(4, lo, lo + n)
    oaf, oav, oq, oqv, ofid = oracle.gen_c4(4, lo, lo + n)
    assert np.array_equal(af.to_host().view(np.uint32), oaf.view(np.uint32))
    assert np.array_equal(q.to_host().view(np.uint32), oq.view(np.uint32))
    assert np.array_equal(av.to_host(nb), oav) and np.array_equal(qv.to_host(nb), oqv)
    assert np.array_equal(fid.to_host(), ofid)
    m = min(n, 5000)
    off, data = ctx.gen_c5(5, 8, 8 + m, 100)
    ooff, odata = oracle.gen_c5(5, 8, 8 + m, 100)
    assert np.array_equal(off.to_host(), ooff) and np.array_equal(data.to_host(m * 100), odata)


# ---- K2 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 5, 2047, 2048, 2049, 1_000_003, 10_000_000])
@pytest.mark.parametrize("region", ["7:50000000-100000000", "1", "X:1000000", "22:1-1", "nope"])
def test_k2_region_count(ctx, oracle, n, region):
    contigs = oracle.c2_contigs()
    name, a, b = oracle.parse_region(region)
    cid = contigs.index(name) if name in contigs else -1
    if n == 0:
        d = ctx.zeros(np.int64, 1)
        ctx.region_count(ctx.empty(np.int32, 4), ctx.empty(np.int64, 4), 0, cid, a, b, d)
        ctx.sync()
        assert d.to_host()[0] == 0
        return
    c, p = ctx.gen_c2(2, n)
    d = ctx.zeros(np.int64, 1)
    ctx.region_count(c, p, n, cid, a, b, d)
    ctx.sync()
    hc, hp = oracle.gen_c2(2, n)
    want, _ = oracle.c2_region_count(hc, hp, contigs, region)
    assert d.to_host()[0] == want


def test_k2_nulls_and_accumulate(ctx, oracle):
    rng = np.random.default_rng(7)
    n = 300_001
    hc, hp = oracle.gen_c2(2, n)
    cv = rng.integers(0, 256, (n + 7) // 8 + 64, dtype=np.uint8)
    pv = rng.integers(0, 256, (n + 7) // 8 + 64, dtype=np.uint8)
    contigs = oracle.c2_contigs()
    want, _ = oracle.c2_region_count(hc, hp, contigs, "2:1000-200000000", chrom_valid=cv, pos_valid=pv)
    d = ctx.zeros(np.int64, 1)
    dc, dp, dcv, dpv = ctx.to_device(hc), ctx.to_device(hp), ctx.to_device(cv), ctx.to_device(pv)
    for _ in range(3):  # state accumulates across launches
        ctx.region_count(dc, dp, n, 1, 1000, 200000000, d, chrom_valid=dcv, pos_valid=dpv)
    ctx.sync()
    assert d.to_host()[0] == 3 * want
    assert want == int((bits(cv, n) & bits(pv, n) & (hc == 1) & (hp >= 1000) & (hp <= 200000000)).sum())


# ---- K6 -----------------------------------------------------------------------------------------------
def _k6_inputs(n, seed, nulls=True):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 25, n, dtype=np.int32)
    start = rng.integers(1, 250_000_000, n, dtype=np.int64)
    end = start + rng.integers(0, 20_000, n, dtype=np.int64)
    nb = (n + 7) // 8 + 64
    mk = (lambda: rng.integers(0, 256, nb, dtype=np.uint8) | rng.integers(0, 256, nb, dtype=np.uint8)) if nulls else (lambda: None)
    return ref, mk(), start, mk(), end, mk()


@pytest.mark.parametrize("n", [1, 5, 2047, 2049, 1_000_003, 12_000_000])
@pytest.mark.parametrize("region", ["chr7:50000000-100000000", "chr1", "chr25:1000000", "chr3:77-77", "nope:1-5"])
def test_k6_overlap_count(ctx, oracle, n, region):
    names = [f"chr{i + 1}" for i in range(25)]
    ref, rv, start, sv, end, ev = _k6_inputs(n, 60 + n % 7)
    name, a, b = oracle.parse_region(region)
    rid = names.index(name) if name in names else -1
    d = ctx.zeros(np.int64, 1)
    dev = [ctx.to_device(x) for x in (ref, rv, start, sv, end, ev)]
    ctx.overlap_count(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], n, rid, a, b, d)
    ctx.sync()
    assert d.to_host()[0] == oracle.c6_overlap_count(ref, rv, start, sv, end, ev, names, region)


def test_k6_generated_alignments_match_the_oracle(ctx, oracle):
    """exon_hip_gen_c6 is bit-identical to the oracle's generator; K6 over it equals the oracle's count."""
    n = 3_000_001
    ref, rv, start, end, pv = ctx.gen_c6(6, 5, 5 + n)
    href, hrv, hst, hen, hpv = oracle.gen_c6(6, 5, 5 + n)
    nb = (n + 7) // 8
    assert np.array_equal(ref.to_host(), href) and np.array_equal(start.to_host(), hst) and np.array_equal(end.to_host(), hen)
    assert np.array_equal(rv.to_host()[:nb], hrv[:nb]) and np.array_equal(pv.to_host()[:nb], hpv[:nb])
    names = oracle.c3_refs()
    d = ctx.zeros(np.int64, 1)
    ctx.overlap_count(ref, rv, start, pv, end, pv, n, 6, 50_000_000, 100_000_000, d)
    ctx.sync()
    want = oracle.c6_overlap_count(href, hrv, hst, hpv, hen, hpv, names, names[6] + ":50000000-100000000")
    assert d.to_host()[0] == want and want > 1000


@pytest.mark.parametrize("n", [1, 2047, 300_000, 6_000_000])
@pytest.mark.parametrize("after,before", [(50_000_000, 100_000_000), (0, 5_000_000), (240_000_000, None), (7, 7)])
def test_k6_strict_within_count(ctx, oracle, n, after, before):
    """BED / GFF form: reference = r AND start > a AND end < b (StartEndIntervalPhysicalExpr), strict comparisons, NULLs drop."""
    ref, rv, st, en, pv = ctx.gen_c6(6, 0, n)
    d = ctx.zeros(np.int64, 1)
    ctx.within_count(ref, rv, st, pv, en, pv, n, 6, after, before, d)
    ctx.sync()
    href, hrv, hs, he, hpv = oracle.gen_c6(6, 0, n)
    names = [oracle.c3_refs()[i] for i in range(25)]
    assert d.to_host()[0] == oracle.c7_within_count(href, hrv, hs, hpv, he, hpv, names, names[6], after, before)


def test_k6_strict_boundaries_and_plan(ctx, oracle):
    """start == a and end == b are OUT in the strict form and IN in the overlap form; the plan layer runs the same kernel."""
    ref = np.zeros(6, np.int32)
    st = np.array([10, 11, 10, 11, 5, 30], np.int64)
    en = np.array([20, 19, 19, 20, 9, 40], np.int64)
    d_ref, d_st, d_en = ctx.to_device(ref), ctx.to_device(st), ctx.to_device(en)
    d = ctx.zeros(np.int64, 1)
    ctx.within_count(d_ref, None, d_st, None, d_en, None, 6, 0, 10, 20, d)
    ctx.sync()
    assert d.to_host()[0] == 1 == oracle.c7_within_count(ref, None, st, None, en, None, ["r"], "r", 10, 20)   # only (11, 19)
    d2 = ctx.zeros(np.int64, 1)
    ctx.overlap_count(d_ref, None, d_st, None, d_en, None, 6, 0, 10, 20, d2)
    ctx.sync()
    assert d2.to_host()[0] == 4
    plan = ctx.plan_within_count(0, 10, 20, columns=(0, 1, 2))
    state = ctx.to_device(np.full(1, 99, np.int64))
    plan.launch([(d_ref, None, None), (d_st, None, None), (d_en, None, None)], 6, state, overwrite=True)
    ctx.sync()
    assert state.to_host()[0] == 1
    plan.close()


def test_k6_no_bitmaps_boundaries_and_accumulate(ctx, oracle):
    names = ["a", "b"]
    # intervals that touch the region ends exactly (1-based inclusive on both sides)
    ref = np.array([0, 0, 0, 0, 1, 0], np.int32)
    start = np.array([1, 100, 201, 50, 100, 200], np.int64)
    end = np.array([99, 100, 300, 400, 200, 200], np.int64)
    d = ctx.zeros(np.int64, 1)
    dev = [ctx.to_device(x) for x in (ref, start, end)]
    for _ in range(2):
        ctx.overlap_count(dev[0], None, dev[1], None, dev[2], None, 6, 0, 100, 200, d)
    ctx.sync()
    want = oracle.c6_overlap_count(ref, None, start, None, end, None, names, "a:100-200")
    assert want == 3 and d.to_host()[0] == 2 * want


# ---- K3 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4097, 1_000_001, 20_000_000])
@pytest.mark.parametrize("mask,value,qmin", [(1284, 0, 30), (4, 4, 0), (0x10, 0x10, 60), (0, 0, -5), (1, 0, 0)])
def test_k3_flag_mapq_group_count(ctx, oracle, n, mask, value, qmin):
    refs = oracle.c3_refs()
    f, mq, mv, ref, rv = ctx.gen_c3(3, 0, n)
    d = ctx.zeros(np.int64, len(refs) + 1)
    ctx.flag_mapq_group_count(f, mq, mv, ref, rv, n, mask, value, qmin, len(refs), d)
    ctx.sync()
    hf, hmq, hmv, href, hrv = oracle.gen_c3(3, 0, n)
    want, _ = oracle.c3_flag_mapq_group_count(hf, hmq, hmv, href, hrv, refs, mask, value, qmin)
    assert np.array_equal(d.to_host(), want)


def test_k3_many_references_global_atomic_path(ctx):
    """More references than the LDS tables hold (EXON_HIP_MAX_GROUPS): counters are global atomics; bit-exact vs numpy."""
    rng = np.random.default_rng(33)
    n, R = 3_000_001, 60_000
    flag = rng.choice(np.array([99, 147, 83, 163, 4, 1024 + 99, 256], np.int32), n)
    mapq = rng.integers(0, 61, n).astype(np.uint8)
    ref = rng.integers(0, R, n, dtype=np.int32)
    nb = (n + 7) // 8 + 64
    mv, rv = rng.integers(0, 256, nb, dtype=np.uint8) | 0x0F, rng.integers(0, 256, nb, dtype=np.uint8) | 0xF0
    d = ctx.zeros(np.int64, R + 1)
    dev = [ctx.to_device(x) for x in (flag, np.concatenate([mapq, np.zeros(64, np.uint8)]), mv, ref, rv)]
    for _ in range(2):
        ctx.flag_mapq_group_count(dev[0], dev[1], dev[2], dev[3], dev[4], n, 1284, 0, 30, R, d)
    ctx.sync()
    mvb, rvb = bits(mv, n), bits(rv, n)
    ok = ((flag & 1284) == 0) & mvb & (mapq >= 30)
    want = np.bincount(np.where(rvb, ref, R)[ok], minlength=R + 1)
    assert np.array_equal(d.to_host(), 2 * want) and want[R] > 0


@pytest.mark.parametrize("R,n", [(25, 6_000_007), (3000, 5_000_000), (60_000, 3_000_001)])
def test_k3_sorted_runs_and_one_hot_reference(ctx, R, n):
    """Coordinate-sorted input: long runs of ONE reference (what a real BAM looks like), runs that change inside a wave's 256
    rows, and a single reference for the whole column.  The uniform-key path (one lane adds the group's count) and the
    per-row path must agree with numpy bit for bit -- per-wave LDS tables (R = 25), the 4-wave shape (R = 3000), and the
    global-atomic path beyond 4096 references (R = 60 000)."""
    rng = np.random.default_rng(R)
    flag = rng.choice(np.array([99, 147, 83, 163, 4, 1024 + 99, 256], np.int32), n)
    mapq = rng.integers(0, 61, n).astype(np.uint8)
    nb = (n + 7) // 8 + 64
    mv, rv = rng.integers(0, 256, nb, dtype=np.uint8) | 0x0F, np.full(nb, 0xFF, np.uint8)
    runs = np.sort(rng.integers(0, R, n // 100_000 + 2).astype(np.int32))     # sorted runs of ~100 k rows
    cuts = np.sort(rng.integers(0, n, len(runs) - 1))
    sorted_ref = np.repeat(runs, np.diff(np.concatenate([[0], cuts, [n]]))).astype(np.int32)
    short = (np.arange(n) // 37 % R).astype(np.int32)                        # runs of 37: every wave group is mixed
    for name, ref in (("sorted", sorted_ref), ("one", np.full(n, R - 1, np.int32)), ("short runs", short)):
        d = ctx.zeros(np.int64, R + 1)
        dev = [ctx.to_device(x) for x in (flag, np.concatenate([mapq, np.zeros(64, np.uint8)]), mv, ref, rv)]
        ctx.flag_mapq_group_count(dev[0], dev[1], dev[2], dev[3], dev[4], n, 1284, 0, 30, R, d)
        ctx.sync()
        ok = ((flag & 1284) == 0) & bits(mv, n) & (mapq >= 30)
        want = np.bincount(ref[ok], minlength=R + 1)
        assert np.array_equal(d.to_host(), want), name


def test_k4_one_hot_key_in_the_lds_tier_and_sorted_keys(ctx, oracle):
    """Every row carries dictionary id 10 (a hot key that lives in the LDS tier), then keys in sorted runs: the uniform-key
    path of K4's LDS tier (counts from ballots, the sum from a wave reduction) against numpy."""
    n, G = 6_000_000, 64
    af, av, q, qv, _ = oracle.gen_c4(4, 0, n)
    avb, qvb = bits(av, n), bits(qv, n)
    keep = avb & (af.astype(np.float64) > 0.01)
    d = [ctx.to_device(x) for x in (af, av, q, qv)]
    for name, fid in (("one hot key", np.full(n, 10, np.int32)), ("sorted runs", (np.arange(n) // 50_000 % G).astype(np.int32)),
                      ("runs of 100", (np.arange(n) // 100 % G).astype(np.int32))):
        dc, ds = ctx.zeros(np.int64, 2 * G), ctx.zeros(np.float64, G)
        ctx.cmp_avg_by_group(d[0], d[1], d[2], d[3], ctx.to_device(fid), n, 0.01, ">", G, dc, ds)
        ctx.sync()
        got = dc.to_host()
        assert np.array_equal(got[G:], np.bincount(fid[keep], minlength=G)), name
        assert np.array_equal(got[:G], np.bincount(fid[keep & qvb], minlength=G)), name
        want_s = np.bincount(fid[keep & qvb], weights=q[keep & qvb].astype(np.float64), minlength=G)
        assert np.allclose(ds.to_host(), want_s, rtol=RTOL, atol=0), name


# ---- K4 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2048, 99_999, 5_000_000])
@pytest.mark.parametrize("op,thr", [(">", 0.01), (">=", 0.01), ("<", 0.5), ("<=", 0.25), ("=", 0.25), ("!=", 0.01),
                                    (">", float(np.float32(0.01))), (">=", float(np.float32(0.01))), (">", -1.0),
                                    (">", 2.0)])
def test_k4_cmp_avg_by_group(ctx, oracle, n, op, thr):
    filters = oracle.c4_filters()
    G = len(filters)
    af, av, q, qv, fid = ctx.gen_c4(4, 0, n)
    dc, ds = ctx.zeros(np.int64, 2 * G), ctx.zeros(np.float64, G)
    ctx.cmp_avg_by_group(af, av, q, qv, fid, n, thr, op, G, dc, ds)
    ctx.sync()
    haf, hav, hq, hqv, hfid = oracle.gen_c4(4, 0, n)
    s, cn, cr, _ = oracle.c4_cmp_avg_by_group(haf, hav, hq, hqv, hfid, filters, thr, op)
    got_c, got_s = dc.to_host(), ds.to_host()
    assert np.array_equal(got_c[:G], cn) and np.array_equal(got_c[G:], cr)
    assert np.allclose(got_s, s, rtol=RTOL, atol=0)


def test_k4_special_values_total_order(ctx, oracle):
    """NaN / -0.0 / inf rows: arrow-rs compares floats in IEEE totalOrder (NaN > everything, -0 < +0)."""
    rng = np.random.default_rng(11)
    n = 70_000
    specials = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 0.01, 1e-45, -1e-45, 3.4e38], np.float32)
    af = specials[rng.integers(0, len(specials), n)]
    q = rng.random(n, dtype=np.float32) * 100
    fid = rng.integers(0, 3, n).astype(np.int32)
    av = rng.integers(0, 256, (n + 7) // 8 + 64, dtype=np.uint8)
    qv = rng.integers(0, 256, (n + 7) // 8 + 64, dtype=np.uint8)
    names = ["a", "b;c", ""]
    d = [ctx.to_device(x) for x in (af, av, q, qv, fid)]
    for op in (">", ">=", "<", "<=", "=", "!="):
        for thr in (0.0, -0.0, 0.01, float("inf")):
            dc, ds = ctx.zeros(np.int64, 6), ctx.zeros(np.float64, 3)
            ctx.cmp_avg_by_group(d[0], d[1], d[2], d[3], d[4], n, thr, op, 3, dc, ds)
            ctx.sync()
            s, cn, cr, _ = oracle.c4_cmp_avg_by_group(af, av, q, qv, fid, names, thr, op)
            got = dc.to_host()
            assert np.array_equal(got[:3], cn) and np.array_equal(got[3:], cr), (op, thr)
            assert np.allclose(ds.to_host(), s, rtol=RTOL, atol=0), (op, thr)


@pytest.mark.parametrize("G,n", [(9, 50_000), (40, 3_000_000), (300, 20_000_000), (4096, 500_000)])
def test_k4_more_than_8_groups_uses_lds_overflow(ctx, oracle, G, n):
    """ids 0..7 in registers, ids >= 8 through the LDS overflow table; skewed keys (most rows in the first ids)."""
    rng = np.random.default_rng(G)
    af, av, q, qv, _ = oracle.gen_c4(4, 0, n)
    fid = np.minimum((rng.exponential(3.0, n)).astype(np.int32), G - 1)
    fid[rng.integers(0, n, 1000)] = rng.integers(0, G, 1000)  # make sure the tail ids occur
    names = [f"f{i}" for i in range(G)]
    dc, ds = ctx.zeros(np.int64, 2 * G), ctx.zeros(np.float64, G)
    ctx.cmp_avg_by_group(ctx.to_device(af), ctx.to_device(av), ctx.to_device(q), ctx.to_device(qv), ctx.to_device(fid),
                         n, 0.01, ">", G, dc, ds)
    ctx.sync()
    s, cn, cr, _ = oracle.c4_cmp_avg_by_group(af, av, q, qv, fid, names, 0.01, ">")
    got = dc.to_host()
    assert np.array_equal(got[:G], cn) and np.array_equal(got[G:], cr)
    assert np.allclose(ds.to_host(), s, rtol=RTOL, atol=0)


@pytest.mark.parametrize("G,n", [(4097, 400_000), (100_000, 3_000_000), (1 << 20, 2_000_000)])
def test_k4_beyond_4096_groups_uses_the_global_table(ctx, oracle, G, n):
    """GROUP BY over a high-cardinality dictionary: the state arrays are the table, rows add with global atomics; counts
    bit-exact, sums within the budget; overwrite mode must clear the arrays first."""
    rng = np.random.default_rng(G)
    af, av, q, qv, _ = oracle.gen_c4(4, 0, n)
    fid = rng.integers(0, G, n).astype(np.int32)
    fid[:5] = [0, G - 1, G // 2, 1, G - 2]
    names = [f"f{i}" for i in range(G)] if G <= 8192 else None
    d = [ctx.to_device(x) for x in (af, av, q, qv, fid)]
    dc, ds = ctx.zeros(np.int64, 2 * G), ctx.zeros(np.float64, G)
    ctx.cmp_avg_by_group(d[0], d[1], d[2], d[3], d[4], n, 0.01, ">", G, dc, ds)
    ctx.sync()
    if G <= 8192:
        s, cn, cr, _ = oracle.c4_cmp_avg_by_group(af, av, q, qv, fid, names, 0.01, ">")
    else:
        # the oracle interns variable-width keys the way DataFusion does and is not built for 10^5+ groups of test data:
        # the same arithmetic column-wise (no NaN in the generated AF, so the plain f64 compare is the totalOrder one)
        avb, qvb = bits(av, n), bits(qv, n)
        keep = avb & (af.astype(np.float64) > 0.01)
        cr = np.bincount(fid[keep], minlength=G)
        cn = np.bincount(fid[keep & qvb], minlength=G)
        s = np.bincount(fid[keep & qvb], weights=q[keep & qvb].astype(np.float64), minlength=G)
    got = dc.to_host()
    assert np.array_equal(got[:G], cn) and np.array_equal(got[G:], cr)
    assert np.allclose(ds.to_host(), s, rtol=RTOL, atol=0)
    plan = ctx.plan_cmp_avg_by_group(">", 0.01, G)
    state = ctx.to_device(np.full(3 * G, 0x0101010101010101, np.int64))
    plan.launch([(d[0], d[1], None), (d[2], d[3], None), (d[4], None, None)], n, state, overwrite=True)
    ctx.sync()
    st = state.to_host()
    assert np.array_equal(st[:G], cn) and np.array_equal(st[G:2 * G], cr) and np.allclose(st[2 * G:].view(np.float64), s, rtol=RTOL, atol=0)
    plan.close()


@pytest.mark.parametrize("G,n,dist", [(4104, 300_000, "uniform"), (4105, 300_000, "uniform"), (20_000, 6_000_000, "zipf"),
                                      (20_000, 6_000_000, "uniform"), (64, 6_000_000, "uniform")])
def test_k4_three_tiers_registers_lds_global(ctx, oracle, G, n, dist):
    """The three tiers of the GROUP BY kernel as shipped since round 3: ids 0..3 in registers, 4..4099 in the LDS table, 4100.. in
    tier 3 (compact -> scatter -> aggregate; global atomics for launches without whole tiles) -- G = 4104 / 4105 put ids on both
    sides of the 4099 | 4100 boundary.  Checked against a column-wise numpy statement (no oracle involved), in overwrite mode and
    accumulating over two launches, small and big launch shapes, keys early-heavy (zipf) and uniform."""
    rng = np.random.default_rng(G + n)
    af, av, q, qv, _ = oracle.gen_c4(4, 0, n)
    if dist == "uniform":
        fid = rng.integers(0, G, n).astype(np.int32)
    else:
        fid = np.minimum(np.exp(rng.random(n) * np.log(G + 1.0)) - 1.0, G - 1).astype(np.int32)
    fid[:6] = [0, 7, 8, min(G - 1, 4103), min(G - 1, 4104), G - 1]
    avb, qvb = bits(av, n), bits(qv, n)
    keep = avb & (af.astype(np.float64) > 0.01)
    cr = np.bincount(fid[keep], minlength=G)
    cn = np.bincount(fid[keep & qvb], minlength=G)
    s = np.bincount(fid[keep & qvb], weights=q[keep & qvb].astype(np.float64), minlength=G)
    d = [ctx.to_device(x) for x in (af, av, q, qv, fid)]
    cols = [(d[0], d[1], None), (d[2], d[3], None), (d[4], None, None)]
    plan = ctx.plan_cmp_avg_by_group(">", 0.01, G)
    state = ctx.to_device(np.full(3 * G, 0x0101010101010101, np.int64))
    plan.launch(cols, n, state, overwrite=True)
    ctx.sync()
    st = state.to_host()
    assert np.array_equal(st[:G], cn) and np.array_equal(st[G:2 * G], cr)
    assert np.allclose(st[2 * G:].view(np.float64), s, rtol=RTOL, atol=0)
    plan.launch(cols, n, state, overwrite=False)  # accumulate: twice the table
    ctx.sync()
    st = state.to_host()
    assert np.array_equal(st[:G], 2 * cn) and np.array_equal(st[G:2 * G], 2 * cr)
    assert np.allclose(st[2 * G:].view(np.float64), 2 * s, rtol=RTOL, atol=0)
    plan.close()


@pytest.mark.parametrize("n", [100_000, 3_000_000, 10_000_000, 20_000_003])
def test_single_launch_fold_never_reads_a_stale_record(ctx, oracle, n):
    """Round 3: the last workgroup folds the per-workgroup records inside the main kernel (agent-scope atomics, no
    fences).  500 accumulating launches back to back on one stream -- small and big shapes, K2 / K3 / K4 interleaved so the
    workspace is reused with different record sizes -- must add up to exactly 500 x one launch: a fold that ever read a
    record of an earlier launch (or missed one) shows up in the integer counters."""
    reps = 500
    c, p = oracle.gen_c2(2, n, 0, n)
    f, mq, mv, ref, rv = oracle.gen_c3(3, 0, n)
    af, av, q, qv, fid = oracle.gen_c4(4, 0, n)
    d2 = [ctx.to_device(x) for x in (c, p)]
    d3 = [ctx.to_device(x) for x in (f, np.concatenate([mq, np.zeros(64, np.uint8)]), mv, ref, rv)]
    d4 = [ctx.to_device(x) for x in (af, av, q, qv, fid)]
    one2, one3 = ctx.zeros(np.int64, 1), ctx.zeros(np.int64, 26)
    one4c, one4s = ctx.zeros(np.int64, 10), ctx.zeros(np.float64, 5)
    acc2, acc3 = ctx.zeros(np.int64, 1), ctx.zeros(np.int64, 26)
    acc4c, acc4s = ctx.zeros(np.int64, 10), ctx.zeros(np.float64, 5)

    def launch(o2, o3, o4c, o4s):
        ctx.region_count(d2[0], d2[1], n, 6, 50_000_000, 100_000_000, o2)
        ctx.flag_mapq_group_count(d3[0], d3[1], d3[2], d3[3], d3[4], n, 1284, 0, 30, 25, o3)
        ctx.cmp_avg_by_group(d4[0], d4[1], d4[2], d4[3], d4[4], n, 0.01, ">", 5, o4c, o4s)
    launch(one2, one3, one4c, one4s)
    for _ in range(reps):
        launch(acc2, acc3, acc4c, acc4s)
    ctx.sync()
    assert acc2.to_host()[0] == reps * one2.to_host()[0] and one2.to_host()[0] > 0
    assert np.array_equal(acc3.to_host(), reps * one3.to_host()) and one3.to_host().sum() > 0
    assert np.array_equal(acc4c.to_host(), reps * one4c.to_host())
    assert np.allclose(acc4s.to_host(), reps * one4s.to_host(), rtol=1e-9, atol=0)
    # and against the oracle once
    r2, _ = oracle.c2_region_count(c, p, oracle.c2_contigs(), "7:50000000-100000000")
    assert one2.to_host()[0] == r2


def test_k4_deterministic(ctx):
    n = 3_000_000
    af, av, q, qv, fid = ctx.gen_c4(9, 0, n)
    outs = []
    for _ in range(3):
        dc, ds = ctx.zeros(np.int64, 10), ctx.zeros(np.float64, 5)
        ctx.cmp_avg_by_group(af, av, q, qv, fid, n, 0.01, ">", 5, dc, ds)
        ctx.sync()
        outs.append(ds.to_host().tobytes() + dc.to_host().tobytes())
    assert outs[0] == outs[1] == outs[2]


def test_k4_bad_group_id_is_reported(ctx):
    import exon_amd
    n = 5000
    af, av, q, qv, fid = ctx.gen_c4(4, 0, n)
    dc, ds = ctx.zeros(np.int64, 4), ctx.zeros(np.float64, 2)
    ctx.cmp_avg_by_group(af, av, q, qv, fid, n, 0.0, ">", 2, dc, ds)  # ids go up to 4
    with pytest.raises(exon_amd.ExonHipError):
        ctx.sync()


# ---- K5 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_reads,L", [(1, 100), (1000, 100), (200_000, 100), (5000, 151), (3000, 36), (70_000, 128),
                                       (40_000, 256), (30_000, 250), (9000, 301), (2000, 400), (50_000, 64), (100_001, 8),
                                       (77, 3), (1_000_000, 100),
                                       # path A (rows == r mod L/4, one column per lane): every kind of L/4 -- odd, even, prime,
                                       # < 16 (three lanes of a half share a dword-of-read), 32 < L/4 <= 64 (single copy), and
                                       # read counts that leave partial rows / idle waves
                                       (1, 32), (3, 36), (65_537, 32), (250_001, 44), (123_457, 76), (99_999, 92), (64, 100),
                                       (4_200_000, 100), (333_333, 124), (80_001, 132), (60_001, 148), (50_001, 200),
                                       (40_001, 252), (4096 * 16 + 1, 256),
                                       # path A for ANY uniform length (round 3): odd L (period L dwords), L = 2 mod 4 (period
                                       # L / 2), periods < 32 (two table copies) and < 16 (four), the 5-plane table (L > 256),
                                       # lengths that leave 1-3 trailing bytes, and enough reads for the steady state
                                       (800_003, 101), (530_001, 151), (540_001, 150), (1_600_001, 51), (1_600_003, 50),
                                       (4_500_001, 18), (9_000_001, 9), (2_400_001, 33), (260_001, 310), (270_003, 309),
                                       (280_001, 302), (320_001, 250), (1_000_001, 75), (3_000_001, 26), (5, 151), (63, 101),
                                       (1_000_003, 10), (6_000_001, 13)])
def test_k5_qual_pos_hist(ctx, oracle, n_reads, L):
    off, data = ctx.gen_c5(5, 0, n_reads, L)
    d = ctx.zeros(np.int64, L * 256)
    ctx.qual_pos_hist(off, data, n_reads, L, d)
    ctx.sync()
    hoff, hdata = oracle.gen_c5(5, 0, n_reads, L)
    want, _ = oracle.c5_qual_pos_hist(hoff, hdata, L)
    assert np.array_equal(d.to_host().reshape(L, 256), want)


def test_k5_non_ascii_bytes_and_unaligned_base(ctx, oracle):
    """bytes >= 128 take the global-atomic slow path; a sliced batch (offsets[0] != 0, unaligned) must still be exact."""
    rng = np.random.default_rng(5)
    n, L = 20_000, 100
    data = rng.integers(33, 75, n * L + 7, dtype=np.uint8)
    data[rng.integers(0, n * L, 500)] = rng.integers(128, 256, 500)
    for shift in (0, 4, 7):
        off = (np.arange(n + 1, dtype=np.int32) * L + shift).astype(np.int32)
        d = ctx.zeros(np.int64, L * 256)
        ctx.qual_pos_hist(ctx.to_device(off), ctx.to_device(np.concatenate([data, np.zeros(64, np.uint8)])), n, L, d)
        ctx.sync()
        want, _ = oracle.c5_qual_pos_hist(off, data, L)
        assert np.array_equal(d.to_host().reshape(L, 256), want), shift


def test_k5_path_a_with_non_ascii_bytes_lmax_above_read_length_and_accumulation(ctx, oracle):
    """Uniform reads (path A) holding bytes >= 128 (global-atomic side path) and control bytes < 32 (ordinary rows), with
    lmax larger than the read length and two launches accumulating into one state."""
    rng = np.random.default_rng(5)
    n, L, lmax = 70_001, 100, 180
    data = rng.integers(33, 75, n * L).astype(np.uint8)
    idx = rng.integers(0, n * L, 5000)
    data[idx] = rng.integers(0, 256, 5000).astype(np.uint8)
    off = (np.arange(n + 1, dtype=np.int64) * L).astype(np.int32)
    d = ctx.zeros(np.int64, lmax * 256)
    d_off, d_data = ctx.to_device(off), ctx.to_device(np.concatenate([data, np.zeros(64, np.uint8)]))
    ctx.qual_pos_hist(d_off, d_data, n, lmax, d)
    ctx.qual_pos_hist(d_off, d_data, n, lmax, d)
    ctx.sync()
    want, _ = oracle.c5_qual_pos_hist(off, data, lmax)
    assert np.array_equal(d.to_host().reshape(lmax, 256), 2 * want)
    assert want[:, 128:].sum() > 0 and want[:, :32].sum() > 0 and want[L:].sum() == 0


@pytest.mark.parametrize("n,L,n_bad", [(1_300_003, 100, 20_000), (900_001, 148, 3), (2_000_000, 64, 50_000), (700_000, 100, 1),
                                          (600_001, 151, 5000), (1_700_001, 50, 5000), (5_000_001, 13, 3000), (300_001, 301, 2000)])
def test_k5_path_a_steady_state_moves_non_ascii_bytes(ctx, oracle, n, L, n_bad):
    """Round 3's path A masks a dword to 7 bits per byte in its steady state (no branch per dword) and repairs, once per 24
    rows, the rows in which a byte >= 128 went to the bin of byte & 127.  The steady state needs >= 48 rows per wavefront
    (> 5e5 reads at L = 100), which the small cases above do not reach: here every wavefront runs it, with many, few and
    exactly one high byte, in two accumulating launches (the repair must not leak into the next launch)."""
    rng = np.random.default_rng(n_bad)
    data = rng.integers(33, 75, n * L).astype(np.uint8)
    idx = rng.integers(0, n * L, n_bad)
    data[idx] = rng.integers(128, 256, n_bad).astype(np.uint8)
    data[idx[: n_bad // 2] ^ 1] = 255  # neighbours in one dword
    off = (np.arange(n + 1, dtype=np.int64) * L).astype(np.int32)
    d = ctx.zeros(np.int64, L * 256)
    d_off, d_data = ctx.to_device(off), ctx.to_device(np.concatenate([data, np.zeros(64, np.uint8)]))
    ctx.qual_pos_hist(d_off, d_data, n, L, d)
    ctx.qual_pos_hist(d_off, d_data, n, L, d)
    ctx.sync()
    want, _ = oracle.c5_qual_pos_hist(off, data, L)
    got = d.to_host().reshape(L, 256)
    assert want[:, 128:].sum() >= 1
    assert np.array_equal(got, 2 * want)


@pytest.mark.parametrize("n,L,shift", [(900_001, 100, 7), (700_001, 151, 3), (1_200_001, 76, 130), (800_001, 101, 255), (600_001, 64, 1),
                                       (3, 100, 250), (2, 151, 255), (1, 36, 254), (700, 100, 253), (1_000_003, 50, 2)])
def test_k5_path_a_on_any_base_alignment(ctx, oracle, n, L, shift):
    """Path A reads 256-byte rows of MEMORY and shifts the positions by where the column's first byte sits in its row, so a
    sliced batch (offsets[0] != 0), a byte-unaligned base and batches packed back to back all keep the fast path; the rows a
    chunk covers only in part (first and last) are added byte by byte.  Large cases reach the steady state; the tiny ones put
    the whole column inside one or two rows.  A few bytes >= 128 ride along."""
    rng = np.random.default_rng(shift)
    data = rng.integers(33, 75, n * L + shift, dtype=np.uint8)
    bad = rng.integers(shift, n * L + shift, max(1, n * L // 50_000))
    data[bad] = rng.integers(128, 256, len(bad)).astype(np.uint8)
    data[:shift] = 200  # bytes in front of the column must not be counted
    off = (np.arange(n + 1, dtype=np.int64) * L + shift).astype(np.int32)
    d = ctx.zeros(np.int64, L * 256)
    ctx.qual_pos_hist(ctx.to_device(off), ctx.to_device(np.concatenate([data, np.full(300, 201, np.uint8)])), n, L, d)
    ctx.sync()
    want, _ = oracle.c5_qual_pos_hist(off, data, L)
    got = d.to_host().reshape(L, 256)
    assert got.sum() == n * L
    assert np.array_equal(got, want)


def _k5_chunk(rng, n, L, shift=0, ragged=False, lmax=None):
    """(offsets, bytes) of one Utf8 batch: uniform length L, or ragged lengths in [0, lmax]"""
    lens = rng.integers(0, lmax + 1, n) if ragged else np.full(n, L)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(lens)
    data = rng.integers(33, 75, int(off[-1]) + shift, dtype=np.uint8)
    if off[-1]:
        k = max(1, int(off[-1]) // 997)
        data[shift + rng.integers(0, int(off[-1]), k)] = rng.integers(128, 256, k)  # a few bytes on the global-atomic side path
    return (off + shift).astype(np.int32), data


@pytest.mark.parametrize("case", ["path_a", "path_a_one_chunk_misaligned", "path_b", "mixed_lengths", "ragged", "more_than_64"])
def test_k5_chunked_column_equals_per_chunk_launches(ctx, oracle, case):
    """exon_hip_qual_pos_hist_chunks (one scan + one main kernel + one fold for up to 64 Arrow batches) against the oracle
    applied chunk by chunk, for every device-side path decision: all chunks uniform and aligned (A), one chunk starting at
    an odd byte (the whole launch must leave path A), L % 4 != 0 (B), chunks of different uniform lengths and ragged
    chunks (G), more chunks than one launch holds, empty chunks in between; accumulate semantics."""
    rng = np.random.default_rng(77)
    lmax = 120
    if case == "path_a":
        specs = [(30_001, 100, 0, False), (1, 100, 0, False), (64, 100, 4, False), (70_000, 100, 0, False), (0, 100, 0, False), (12_345, 100, 8, False)]
    elif case == "path_a_one_chunk_misaligned":
        specs = [(20_000, 100, 0, False), (20_000, 100, 3, False), (5_000, 100, 0, False)]
    elif case == "path_b":
        specs = [(20_000, 99, 0, False), (33_333, 99, 16, False), (7, 99, 0, False)]
    elif case == "mixed_lengths":
        specs = [(20_000, 100, 0, False), (20_000, 96, 0, False), (100, 120, 0, False)]
    elif case == "ragged":
        specs = [(20_000, 100, 0, False), (15_000, 0, 5, True), (0, 0, 0, True), (9_999, 0, 0, True)]
    else:
        specs = [(500 + 13 * i, 100, 0, False) for i in range(150)]
    chunks, want = [], np.zeros((lmax, 256), np.int64)
    for n, L, shift, ragged in specs:
        off, data = _k5_chunk(rng, n, L, shift, ragged, lmax)
        chunks.append((ctx.to_device(off), ctx.to_device(np.concatenate([data, np.zeros(64, np.uint8)])), n))
        if n:
            want += oracle.c5_qual_pos_hist(off, data, lmax)[0]
    d = ctx.zeros(np.int64, lmax * 256)
    ctx.qual_pos_hist_chunks(chunks, lmax, d)
    ctx.sync()
    assert np.array_equal(d.to_host().reshape(lmax, 256), want), case
    ctx.qual_pos_hist_chunks(chunks, lmax, d)  # accumulates
    ctx.sync()
    assert np.array_equal(d.to_host().reshape(lmax, 256), 2 * want), case
    # the plan form: OVERWRITE defines the state whatever was in it, then ACCUMULATE adds
    plan = ctx.plan_qual_pos_hist(lmax)
    plan.launch_chunks([([(dd, None, o)], n) for (o, dd, n) in chunks], d, overwrite=True)
    ctx.sync()
    assert np.array_equal(d.to_host().reshape(lmax, 256), want), case
    plan.launch_chunks([([(dd, None, o)], n) for (o, dd, n) in chunks[:2]], d, overwrite=False)
    plan.launch_chunks([], d, overwrite=False)
    ctx.sync()
    plan.launch_chunks([([(dd, None, o)], 0) for (o, dd, n) in chunks[:1]], d, overwrite=True)  # only empty chunks: state := 0
    ctx.sync()
    assert not d.to_host().any()
    plan.close()


def test_plan_launch_chunks_on_a_row_plan(ctx, oracle):
    """kinds other than the histogram launch per chunk: K2 over three chunks == K2 over the concatenation"""
    n = 300_000
    chrom, pos = ctx.gen_c2(2, n, 0, n)
    plan = ctx.plan_region_count(6, 50_000_000, 100_000_000)
    st = ctx.zeros(np.int64, 1)
    plan.launch([(chrom, None, None), (pos, None, None)], n, st, overwrite=True)
    ctx.sync()
    whole = int(st.to_host()[0])
    cuts = [0, 100_000, 100_000, 250_004, n]  # chunk starts stay 16-byte aligned (i32: 4 rows)
    chunks = [([(chrom.ptr + 4 * a, None, None), (pos.ptr + 8 * a, None, None)], b - a) for a, b in zip(cuts, cuts[1:])]
    st2 = ctx.to_device(np.array([12345], np.int64))
    plan.launch_chunks(chunks, st2, overwrite=True)
    ctx.sync()
    assert int(st2.to_host()[0]) == whole and whole > 0
    plan.launch_chunks(chunks, st2)
    ctx.sync()
    assert int(st2.to_host()[0]) == 2 * whole
    plan.close()


def test_k5_read_longer_than_lmax_is_reported(ctx):
    import exon_amd
    off, data = ctx.gen_c5(5, 0, 1000, 100)
    d = ctx.zeros(np.int64, 50 * 256)
    ctx.qual_pos_hist(off, data, 1000, 50, d)
    with pytest.raises(exon_amd.ExonHipError):
        ctx.sync()


def test_k5_ragged_reads(ctx, oracle):
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 180, 20_000)
    lens[:5] = [0, 1, 179, 0, 64]
    off = np.zeros(len(lens) + 1, np.int32)
    off[1:] = np.cumsum(lens)
    data = rng.integers(33, 75, off[-1], dtype=np.uint8)
    d = ctx.zeros(np.int64, 180 * 256)
    ctx.qual_pos_hist(ctx.to_device(off), ctx.to_device(np.concatenate([data, np.zeros(64, np.uint8)])), len(lens), 180, d)
    ctx.sync()
    want, _ = oracle.c5_qual_pos_hist(off, data, 180)
    assert np.array_equal(d.to_host().reshape(180, 256), want)


@pytest.mark.parametrize("G,dist", [(4105, "uniform"), (20_000, "uniform"), (100_000, "uniform"), (100_000, "early"), (4100 + 64 * 8192, "uniform"),
                                    (4100 + 64 * 8192 + 1, "uniform"), (4100 + 130 * 8192 + 5, "uniform")])
def test_k4_tier3_big_launches_with_many_id_ranges(ctx, G, dist):
    """Launches big enough for the 1024-thread shape (>= 16384 rows per CU) with id ranges beyond the LDS table: tier 3 with
    1, 2, 12, 64, 65 and 131 id ranges of 8192 ids -- the direct partition where its chunk pool fits the scratch, compact ->
    scatter -> aggregate otherwise and always beyond 128 ranges.  Counts bit-exact vs numpy, sums within the budget; a second
    launch accumulates; the row count is not a multiple of the tile (remainder rows: atomic form).  (Round 4's opt-in partition
    inside the main kernel, which this test was written for, was removed in round 5: bit-identical, not faster.)"""
    from oracle import Oracle
    orc = Oracle()
    n = 6_000_000 + 4321
    rng = np.random.default_rng(G + len(dist))
    af, av, q, qv, _ = orc.gen_c4(4, 0, n)
    if dist == "uniform":
        fid = rng.integers(0, G, n).astype(np.int32)
    else:  # most rows on early ids, a long thin tail
        fid = np.minimum((rng.exponential(G / 30.0, n)).astype(np.int64), G - 1).astype(np.int32)
    fid[:5] = [0, G - 1, G // 2, 1, G - 2]
    avb, qvb = bits(av, n), bits(qv, n)
    keep = avb & (af.astype(np.float64) > 0.01)
    cr = np.bincount(fid[keep], minlength=G)
    cn = np.bincount(fid[keep & qvb], minlength=G)
    s = np.bincount(fid[keep & qvb], weights=q[keep & qvb].astype(np.float64), minlength=G)
    d = [ctx.to_device(x) for x in (af, av, q, qv, fid)]
    plan = ctx.plan_cmp_avg_by_group(">", 0.01, G)
    state = ctx.to_device(np.full(3 * G, 0x0101010101010101, np.int64))
    cols = [(d[0], d[1], None), (d[2], d[3], None), (d[4], None, None)]
    plan.launch(cols, n, state, overwrite=True)
    ctx.sync()
    st = state.to_host()
    assert np.array_equal(st[:G], cn) and np.array_equal(st[G:2 * G], cr)
    assert np.allclose(st[2 * G:].view(np.float64), s, rtol=RTOL, atol=0)
    plan.launch(cols, n, state, overwrite=False)
    ctx.sync()
    st = state.to_host()
    assert np.array_equal(st[:G], 2 * cn) and np.array_equal(st[G:2 * G], 2 * cr)
    assert np.allclose(st[2 * G:].view(np.float64), 2 * s, rtol=RTOL, atol=0)


@pytest.mark.parametrize("G,n", [(4100 + 8192, 40_000_000 + 77), (30_000, 40_000_000), (100_000, 64_000_000 + 5)])
def test_k4_direct_partition_fills_many_chunks_per_stream(ctx, G, n):
    """Tier 3's direct partition (round 6): enough tier-3 records per workgroup and stream that every stream walks through
    several 2048-record chunks (the 6 M-row cases above stay inside their first chunk): counts bit-exact vs numpy, sums within
    the budget.  test_k4_tier3_big_launches_with_many_id_ranges covers the compact -> scatter path (131 id ranges)."""
    rng = np.random.default_rng(G)
    af = rng.random(n, dtype=np.float32)
    q = (rng.random(n, dtype=np.float32) * 100).astype(np.float32)
    fid = rng.integers(0, G, n).astype(np.int32)
    qvb = rng.random(n) < 0.9
    qv = np.packbits(qvb, bitorder="little")
    keep = af.astype(np.float64) > 0.5
    cr = np.bincount(fid[keep], minlength=G)
    cn = np.bincount(fid[keep & qvb], minlength=G)
    s_ = np.bincount(fid[keep & qvb], weights=q[keep & qvb].astype(np.float64), minlength=G)
    d = [ctx.to_device(x) for x in (af, q, qv, fid)]
    plan = ctx.plan_cmp_avg_by_group(">", 0.5, G)
    state = ctx.to_device(np.zeros(3 * G, np.int64))
    plan.launch([(d[0], None, None), (d[1], d[2], None), (d[3], None, None)], n, state, overwrite=True)
    ctx.sync()
    st = state.to_host()
    assert np.array_equal(st[:G], cn) and np.array_equal(st[G:2 * G], cr)
    assert np.allclose(st[2 * G:].view(np.float64), s_, rtol=RTOL, atol=0)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_k4_tier3_random_shapes_against_numpy(ctx, seed):
    """Random row counts (whole tiles + remainders, small and big launch shapes), key counts from just above the LDS table to 1.1 M
    (1 .. 135 id ranges: the direct partition with 1 and 4 streams per range, and the scatter path beyond 128 ranges), uniform and
    skewed keys, NULLs in x and y: counts bit-exact vs numpy, sums within the budget, twice (the second launch accumulates)."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([70_001, 2_500_000 + int(rng.integers(0, 9000)), 9_000_000 + int(rng.integers(0, 20000))]))
    G = int(rng.choice([4101, 4100 + 8192, 4100 + 8193, 50_000, 300_000, 4100 + 130 * 8192 + 5]))
    af = rng.random(n, dtype=np.float32)
    q = (rng.random(n, dtype=np.float32) * 50).astype(np.float32)
    if rng.random() < 0.5:
        fid = rng.integers(0, G, n).astype(np.int32)
    else:
        fid = np.minimum(rng.exponential(G / 12.0, n).astype(np.int64), G - 1).astype(np.int32)
    avb, qvb = rng.random(n) < 0.97, rng.random(n) < 0.9
    av, qv = np.packbits(avb, bitorder="little"), np.packbits(qvb, bitorder="little")
    keep = avb & (af.astype(np.float64) > 0.3)
    cr = np.bincount(fid[keep], minlength=G)
    cn = np.bincount(fid[keep & qvb], minlength=G)
    s_ = np.bincount(fid[keep & qvb], weights=q[keep & qvb].astype(np.float64), minlength=G)
    d = [ctx.to_device(x) for x in (af, av, q, qv, fid)]
    plan = ctx.plan_cmp_avg_by_group(">", 0.3, G)
    state = ctx.to_device(np.full(3 * G, 0x0101010101010101, np.int64))
    cols = [(d[0], d[1], None), (d[2], d[3], None), (d[4], None, None)]
    for k in (1, 2):
        plan.launch(cols, n, state, overwrite=(k == 1))
        ctx.sync()
        st = state.to_host()
        assert np.array_equal(st[:G], k * cn) and np.array_equal(st[G:2 * G], k * cr), (n, G, k)
        assert np.allclose(st[2 * G:].view(np.float64), k * s_, rtol=RTOL, atol=0)
