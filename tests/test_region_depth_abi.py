"""No GPU: the region-set depth plan (kind 14) is declared in every layer, its constructor refuses what the header says it refuses, and
its host-only helpers -- layout, intervals, per_base and decode -- answer on hand-made and on expected states, modulo 2^64.  A plan
created without a context is host-only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L

import region_bases_expect as E12
import region_depth_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["exon_hip_plan_create_region_set_depth", "exon_hip_region_depth_layout", "exon_hip_region_depth_intervals", "exon_hip_region_depth_per_base",
         "exon_hip_region_depth_decode", "exon_hip_region_depth_reduce", "exon_hip_region_set_depth"]
EINVAL, EUNSUPPORTED = -1, -4
OPEN_END = 2**63 - 1


def host_plan(regions, thresholds=(1, 2), columns=(2, 3, 4)):
    return exon_amd.RegionDepthPlan(None, regions, thresholds, columns)


def test_every_layer_carries_the_names_and_the_constants():
    lib = exon_amd.load()
    header = open(os.path.join(ROOT, "include", "exon_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    kernels_h = open(os.path.join(ROOT, "exon_amd", "csrc", "kernels.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
        assert re.search(r"\bint %s\(" % name, header), name
        assert re.search(r"\bpub fn %s\(" % name, sys_rs), name
    assert re.search(r"#define EXON_HIP_PLAN_REGION_SET_DEPTH 14\b", header)
    assert re.search(r"#define EXON_HIP_REGION_DEPTH_MAX_BINS %d\b" % (1 << 26), header)
    assert re.search(r"#define EXON_HIP_REGION_DEPTH_MAX_THRESHOLDS 8\b", header)
    assert re.search(r"pub const EXON_HIP_PLAN_REGION_SET_DEPTH: i32 = 14;", sys_rs)
    assert re.search(r"pub const EXON_HIP_REGION_DEPTH_MAX_BINS: i32 = %d;" % (1 << 26), sys_rs)
    assert re.search(r"pub const EXON_HIP_REGION_DEPTH_MAX_THRESHOLDS: i32 = 8;", sys_rs)
    assert L.PLAN_REGION_SET_DEPTH == 14 and L.REGION_DEPTH_MAX_BINS == exon_amd.REGION_DEPTH_MAX_BINS == 1 << 26 and L.REGION_DEPTH_MAX_THRESHOLDS == 8
    assert lib.exon_hip_abi_version() == 5  # additive
    # the bounds the GPU tests aim at are the kernels' own
    bound = int(re.search(r"constexpr int REGION_DEPTH_LDS_MAX = (\d+);", kernels_h).group(1))
    assert bound == exon_amd.REGION_DEPTH_LDS_MAX == L.REGION_DEPTH_LDS_MAX == 8192
    assert 16 * bound <= 160 * 1024  # the bins, and the interval table beside them while both fit
    tile = int(re.search(r"constexpr int REGION_DEPTH_REDUCE_TILE = (\d+);", kernels_h).group(1))
    assert tile == exon_amd.REGION_DEPTH_REDUCE_TILE == L.REGION_DEPTH_REDUCE_TILE
    for name in ("launch_region_set_depth", "launch_region_depth_reduce", "struct RegionDepthTables"):
        assert name in kernels_h
    for attr in ("plan_region_set_depth", "region_set_depth"):
        assert callable(getattr(exon_amd.Context, attr)), attr
    for attr in ("layout", "intervals", "per_base", "decode", "reduce"):
        assert callable(getattr(exon_amd.RegionDepthPlan, attr)), attr
    assert issubclass(exon_amd.RegionDepthPlan, exon_amd.RegionSetPlan)
    for name in ("RegionDepthPlan", "REGION_DEPTH_LDS_MAX", "REGION_DEPTH_REDUCE_TILE", "REGION_DEPTH_MAX_BINS"):
        assert name in exon_amd.__all__
    assert "region_depth.o" in open(os.path.join(ROOT, "exon_amd", "csrc", "Makefile")).read()
    assert "k_region_set_depth" in open(os.path.join(ROOT, "exon_amd", "csrc", "region_depth.hip")).read()
    k14 = header[header.index("K14:"):header.index("#define EXON_HIP_PLAN_REGION_SET_DEPTH")]
    assert "NOT LINEAR" in k14 and "CIGAR" in k14 and "BED source" in k14 and "open-ended" in k14 and "word for word" in k14


SETS = [
    ([(0, 11, 20)], [(0, 11, 20, 0)]),                                                  # one region
    ([(0, 11, 20), (0, 21, 30)], [(0, 11, 30, 0)]),                                     # abutting: one interval
    ([(0, 11, 20), (0, 31, 40)], [(0, 11, 20, 0), (0, 31, 40, 10)]),                    # a gap
    ([(0, 11, 40), (0, 15, 20)], [(0, 11, 40, 0)]),                                     # nested
    ([(0, 15, 20), (0, 11, 40), (0, 30, 45)], [(0, 11, 45, 0)]),                        # overlapping, not in order
    ([(3, 5, 9), (3, 5, 9)], [(0, 5, 9, 0)]),                                           # duplicate
    ([(7, 5, 9), (2, 1, 1), (7, 20, 21)], [(0, 5, 9, 0), (0, 20, 21, 5), (1, 1, 1, 8)]),  # two contigs, by first appearance
    ([(0, 2**62, 2**62 + 9), (0, 1, 1)], [(0, 1, 1, 0), (0, 2**62, 2**62 + 9, 1)]),     # far apart
]


@pytest.mark.parametrize("regions,want", SETS)
def test_layout_intervals_and_state_size(regions, want):
    p = host_plan(regions)
    T = sum(e - s + 1 for _, s, e, _ in want)
    Cn = len({c for c, _, _ in regions})
    assert p.n_i64 == 4 + T + Cn and p.n_f64 == 0
    assert p.layout() == (0, 4, 4 + T + Cn) == E.layout(regions)
    slot, start, end, bins = p.intervals()
    assert list(zip(slot.tolist(), start.tolist(), end.tolist(), bins.tolist())) == want == E.intervals(regions)
    zero = np.zeros(p.n_i64, np.int64)
    assert p.per_base(zero).tolist() == [0] * T
    bases, ge = p.decode(zero)
    assert bases.tolist() == [0] * len(regions) and ge.shape == (len(regions), 2) and not ge.any()
    p.close()


def test_per_base_and_decode_hand_made_states():
    regions = [(0, 11, 20), (0, 31, 40), (5, 3, 4), (0, 16, 20)]
    p = host_plan(regions, [1, 2, 3])
    assert p.layout() == (0, 4, 4 + 20 + 1 + 2 + 1)
    st = np.zeros(p.n_i64, np.int64)
    st[4 + 4], st[4 + 15] = 1, -1    # the row [15, 35] on contig 0
    st[4 + 7] += 2
    st[4 + 9] -= 2                   # two rows [18, 19]
    st[4 + 21], st[4 + 22] = 1, -1   # the row [3, 3] on contig 5
    depth = [0] * 4 + [1, 1, 1, 3, 3, 1] + [1] * 5 + [0] * 5 + [1, 0]
    assert p.per_base(st).tolist() == depth
    bases, ge = p.decode(st)
    assert bases.tolist() == [10, 5, 1, 9]
    assert ge.tolist() == [[6, 2, 2], [5, 0, 0], [1, 0, 0], [5, 2, 2]]
    d, b, g = E.decode(regions, [1, 2, 3], st)
    assert d.tolist() == depth and b.tolist() == bases.tolist() and g.tolist() == ge.tolist()
    # the running sum is ONE array over the section: a +1 left open on contig 0 reaches contig 5, on the host as on the device
    st = np.zeros(p.n_i64, np.int64)
    st[4 + 19] = 1
    assert p.per_base(st).tolist() == [0] * 19 + [1] + [1, 1]
    # depths are read as int64: 2^64 - 1 is -1 and passes no threshold, and `bases` wraps
    st = np.zeros(p.n_i64, np.int64)
    st[4 + 0], st[4 + 2] = -1, 1
    bases, ge = p.decode(st)
    assert p.per_base(st)[:3].tolist() == [-1, -1, 0] and bases[0] == -2 and not ge[0].any()
    with pytest.raises(ValueError):
        p.decode(st[:-1])
    with pytest.raises(ValueError):
        p.per_base(st[:-1])
    p.close()


@pytest.mark.parametrize("k", [0, 1, 8])
def test_decode_of_the_expected_state_and_partial_states(k):
    rng = np.random.default_rng(40 + k)
    regions = [(int(rng.choice([1, 3, 5])), s, s + int(rng.integers(0, 60))) for s in rng.integers(1, 900, 50).tolist()]
    thr = [1, 2, 3, 5, 8, 13, 21, 34][:k]
    n = 4000
    ref = rng.integers(-1, 8, n).astype(np.int32)
    start = rng.integers(-20, 1000, n)
    end = start + rng.integers(-3, 120, n)
    rows = (ref, start, end) + tuple(rng.random(n) < 0.95 for _ in range(3))
    p = host_plan(regions, thr)
    st = E.expect_state(regions, *rows)
    totals, depth, bases, ge = E.expect(regions, thr, *rows)
    assert st.size == p.n_i64 and st[:4].tolist() == totals.tolist()
    assert p.per_base(st).tolist() == depth.tolist()
    got = p.decode(st)
    assert got[0].tolist() == bases.tolist() and got[1].tolist() == ge.tolist() and got[1].shape == (50, k)
    assert bases.sum() > 0
    # the sum of two partial states decodes to the whole; bases adds, ge of the parts does not
    half = n // 2
    a = E.expect_state(regions, *(x[:half] for x in rows))
    b = E.expect_state(regions, *(x[half:] for x in rows))
    assert np.array_equal(a + b, st)
    whole = p.decode(a + b)
    assert whole[0].tolist() == bases.tolist() and whole[1].tolist() == ge.tolist()
    assert (p.decode(a)[0] + p.decode(b)[0]).tolist() == bases.tolist()
    if k:
        assert (p.decode(a)[1] + p.decode(b)[1]).tolist() != ge.tolist()
    p.close()


def test_bases_is_kind_12s():
    rng = np.random.default_rng(12)
    regions = [(int(rng.choice([0, 2])), s, s + int(rng.integers(0, 80))) for s in rng.integers(1, 700, 40).tolist()]
    n = 3000
    rows = (rng.integers(-1, 4, n).astype(np.int32), rng.integers(-5, 800, n), None)
    rows = (rows[0], rows[1], rows[1] + rng.integers(-2, 100, n))
    p14, p12 = host_plan(regions), exon_amd.RegionBasesPlan(None, regions)
    want = p12.decode(E12.expect_state(regions, *rows))
    assert p14.decode(E.expect_state(regions, *rows))[0].tolist() == want.tolist() and want.sum() > 0
    p14.close()
    p12.close()


def _create(regions, thr=(1,), names=None, n=None, columns=(2, 3, 4), n_thr=None):
    lib = exon_amd.load()
    h = C.c_void_p()
    ids = np.array([r[0] for r in regions], np.int32)
    starts = np.array([r[1] for r in regions], np.int64)
    ends = np.array([r[2] for r in regions], np.int64)
    t = np.array(list(thr) + [0], np.int64)
    rc = lib.exon_hip_plan_create_region_set_depth(None, (C.c_int32 * 3)(*columns), names, len(names) if names else 0, None if names else ids.ctypes.data,
                                                   starts.ctypes.data, ends.ctypes.data, len(regions) if n is None else n, t.ctypes.data,
                                                   len(thr) if n_thr is None else n_thr, C.byref(h))
    msg = lib.exon_hip_last_error(None).decode()
    if rc == 0:
        lib.exon_hip_plan_destroy(h)
    return rc, msg


def test_constructor_refusals():
    ok = [(0, 11, 20)]
    assert _create(ok)[0] == 0
    assert _create(ok, thr=())[0] == 0                       # no thresholds: bases alone
    assert _create(ok, thr=range(1, 9))[0] == 0
    rc, msg = _create(ok, thr=range(1, 10))                  # 9 thresholds
    assert rc == EINVAL and "n_thresholds" in msg
    assert _create(ok, n_thr=-1)[0] == EINVAL
    for thr in ([0], [5, 5], [10, 1], [1, 2, 2], [-3]):
        rc, msg = _create(ok, thr=thr)
        assert rc == EINVAL and "strictly increasing" in msg, thr
    rc, msg = _create([(0, 11, 20), (0, 5, OPEN_END)])
    assert rc == EUNSUPPORTED and "region 1" in msg and "open end" in msg
    assert _create([(0, 5, OPEN_END - 1)])[0] == EUNSUPPORTED  # finite, and far beyond the bins
    # T + C = 2^26 exactly, and one more (one region: a host plan allocates nothing per base)
    assert _create([(0, 1, (1 << 26) - 1)])[0] == 0
    rc, msg = _create([(0, 1, 1 << 26)])
    assert rc == EUNSUPPORTED and str(1 << 26) in msg
    assert _create([(0, 1, (1 << 26) - 3), (1, 7, 7)])[0] == 0
    assert _create([(0, 1, (1 << 26) - 3), (1, 7, 8)])[0] == EUNSUPPORTED
    # kind 11 / 12's rules
    assert _create(ok, n=0)[0] == EINVAL
    assert _create([(0, 0, 5)])[0] == EINVAL and _create([(0, 9, 8)])[0] == EINVAL
    rc, msg = _create([(0, 1, 2), (-1, 1, 2)])
    assert rc == EINVAL and "negative reference id" in msg
    assert _create([(1 << 24, 1, 2)])[0] == EUNSUPPORTED
    assert _create([(0, 1, 2), (0, 4, 5)], names=b"chr1\0")[0] == EINVAL
    assert _create([(0, 1, 2), (0, 4, 5)], names=b"chr1\0\0")[0] == EINVAL
    assert _create([(0, 1, 2), (0, 4, 5)], names=b"chr1\0chr2\0")[0] == 0
    assert _create(ok, columns=(0, -1, 2))[0] == EINVAL
    lib = exon_amd.load()
    h = C.c_void_p()
    one = np.ones(1, np.int64)
    assert lib.exon_hip_plan_create_region_set_depth(None, (C.c_int32 * 3)(2, 3, 4), None, 0, None, one.ctypes.data, one.ctypes.data, 1, None, 0, C.byref(h)) == EINVAL
    assert lib.exon_hip_plan_create_region_set_depth(None, (C.c_int32 * 3)(2, 3, 4), None, 0, np.zeros(1, np.int32).ctypes.data, one.ctypes.data, one.ctypes.data, 1, None, 2,
                                                     C.byref(h)) == EINVAL


def test_too_many_regions():
    m = (1 << 20) + 1
    lib = exon_amd.load()
    h = C.c_void_p()
    ids, pos = np.zeros(m, np.int32), np.ones(m, np.int64)
    assert lib.exon_hip_plan_create_region_set_depth(None, (C.c_int32 * 3)(2, 3, 4), None, 0, ids.ctypes.data, pos.ctypes.data, pos.ctypes.data, m, None, 0,
                                                     C.byref(h)) == EUNSUPPORTED


def test_plan_create_refuses_kind_14_and_names_the_constructor():
    lib = exon_amd.load()
    d = L.PlanDesc(kind=L.PLAN_REGION_SET_DEPTH)
    h = C.c_void_p()
    assert lib.exon_hip_plan_create(None, C.byref(d), C.byref(h)) == EINVAL
    assert "use exon_hip_plan_create_region_set_depth" in lib.exon_hip_last_error(None).decode()
    assert not h.value


def test_helpers_refuse_the_other_kinds_plans_and_null():
    lib = exon_amd.load()
    out = (C.c_int64 * 6)()
    n = C.c_int32()
    state = np.zeros(64, np.int64)
    res = np.zeros(64, np.int64)
    assert lib.exon_hip_region_depth_layout(None, out) == EINVAL
    assert lib.exon_hip_region_depth_intervals(None, C.byref(n), None, None, None, None) == EINVAL
    assert lib.exon_hip_region_depth_per_base(None, state.ctypes.data, res.ctypes.data) == EINVAL
    assert lib.exon_hip_region_depth_decode(None, state.ctypes.data, res.ctypes.data) == EINVAL
    assert lib.exon_hip_region_depth_reduce(None, None, None, state.ctypes.data, res.ctypes.data) == EINVAL
    p = host_plan([(0, 1, 2)])
    assert lib.exon_hip_region_depth_layout(p.h, None) == EINVAL
    assert lib.exon_hip_region_depth_intervals(p.h, None, None, None, None, None) == EINVAL
    assert lib.exon_hip_region_depth_per_base(p.h, None, None) == EINVAL
    assert lib.exon_hip_region_depth_decode(p.h, None, None) == EINVAL
    assert lib.exon_hip_region_depth_reduce(None, None, p.h, state.ctypes.data, res.ctypes.data) == EINVAL  # a host-only plan has no context
    others = [exon_amd.RegionSetPlan(None, [(0, 1, 2)]), exon_amd.RegionBasesPlan(None, [(0, 1, 2)]), exon_amd.WindowBasesPlan(None, [(0, 35)], 10)]
    for k in others:  # kind 14's helpers on kinds 11, 12 and 13
        assert lib.exon_hip_region_depth_layout(k.h, out) == EINVAL
        assert "kind 14" in lib.exon_hip_last_error(None).decode()
        assert lib.exon_hip_region_depth_intervals(k.h, C.byref(n), None, None, None, None) == EINVAL
        assert lib.exon_hip_region_depth_per_base(k.h, state.ctypes.data, res.ctypes.data) == EINVAL
        assert lib.exon_hip_region_depth_decode(k.h, state.ctypes.data, res.ctypes.data) == EINVAL
        assert lib.exon_hip_region_depth_reduce(None, None, k.h, state.ctypes.data, res.ctypes.data) == EINVAL
        assert lib.exon_hip_region_set_depth(None, None, None, None, None, 0, k.h, None) == EINVAL
    # kind 11's, 12's and 13's helpers on kind 14
    assert lib.exon_hip_region_set_layout(p.h, out) == EINVAL
    assert "kind 11" in lib.exon_hip_last_error(None).decode()
    assert lib.exon_hip_region_set_decode(p.h, state.ctypes.data, res.ctypes.data) == EINVAL
    assert lib.exon_hip_region_set_overlap(None, None, None, None, None, 0, p.h, None) == EINVAL
    assert lib.exon_hip_region_bases_layout(p.h, out) == EINVAL
    assert "kind 12" in lib.exon_hip_last_error(None).decode()
    assert lib.exon_hip_region_bases_decode(p.h, state.ctypes.data, res.ctypes.data) == EINVAL
    assert lib.exon_hip_region_set_bases(None, None, None, None, None, 0, p.h, None) == EINVAL
    assert lib.exon_hip_window_bases_layout(p.h, out) == EINVAL
    assert "kind 13" in lib.exon_hip_last_error(None).decode()
    assert lib.exon_hip_window_bases_offsets(p.h, res.ctypes.data) == EINVAL
    assert lib.exon_hip_window_bases_decode(p.h, state.ctypes.data, res.ctypes.data) == EINVAL
    assert lib.exon_hip_window_bases(None, None, None, None, None, 0, p.h, None) == EINVAL
    # a host-only plan cannot be executed
    h = C.c_void_p()
    assert lib.exon_hip_stream_open(p.h, 0, C.byref(h)) == EINVAL
    assert "host-only" in lib.exon_hip_last_error(None).decode()
    p.close()
    for k in others:
        k.close()


def test_names_form_host_plan():
    p = host_plan([("chr2", 5, 9), ("chr1", 1, 1), ("chr2", 10, 12)])
    assert p.by_name and p.layout() == (0, 4, 4 + 9 + 2)
    assert [x.tolist() for x in p.intervals()] == [[0, 1], [5, 1], [12, 1], [0, 9]]
    p.close()
    with pytest.raises(ValueError):
        host_plan([("chr2", 1, 2), (1, 1, 2)])
