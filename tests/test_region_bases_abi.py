"""No GPU: the covered-bases plan (kind 12) is declared in every layer, its constructor refuses what kind 11's refuses, and its
host-only helpers -- layout and decode -- answer on hand-made and on expected states, modulo 2^64.  A plan created without a context
is host-only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L

import region_bases_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["exon_hip_plan_create_region_set_bases", "exon_hip_region_bases_layout", "exon_hip_region_bases_decode", "exon_hip_region_set_bases"]
EINVAL, EUNSUPPORTED = -1, -4


def host_plan(regions, columns=(2, 3, 4)):
    return exon_amd.RegionBasesPlan(None, regions, columns)


def full(regions):
    return [(c, s, E.OPEN_END if e is None else e) for c, s, e in regions]


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
    assert re.search(r"#define EXON_HIP_PLAN_REGION_SET_BASES 12\b", header)
    assert re.search(r"pub const EXON_HIP_PLAN_REGION_SET_BASES: i32 = 12;", sys_rs)
    assert L.PLAN_REGION_SET_BASES == 12
    assert lib.exon_hip_abi_version() == 5  # additive
    # the tier bound the GPU tests aim at is the kernel's own: 8 B of point table and 24 B of bins per unit, inside the CU's 160 KiB
    bound = int(re.search(r"constexpr int REGION_BASES_LDS_MAX = (\d+);", kernels_h).group(1))
    assert bound == exon_amd.REGION_BASES_LDS_MAX == L.REGION_BASES_LDS_MAX
    assert 32 * bound <= 160 * 1024
    assert "launch_region_set_bases" in kernels_h
    for attr in ("plan_region_set_bases", "region_set_bases"):
        assert callable(getattr(exon_amd.Context, attr)), attr
    for name in ("region_bases_layout", "region_bases_decode", "RegionBasesPlan", "REGION_BASES_LDS_MAX"):
        assert name in exon_amd.__all__
    assert "region_bases.o" in open(os.path.join(ROOT, "exon_amd", "csrc", "Makefile")).read()
    assert "k_region_set_bases" in open(os.path.join(ROOT, "exon_amd", "csrc", "region_bases.hip")).read()
    assert "modulo 2^64" in header.lower() and "DECISION" in header


def test_layout_of_a_hand_made_set():
    # contig 3: points {9, 20} U {20, 30} U {0, OPEN} = 0, 9, 20, 30, OPEN (20 is shared: one point); contig 1: {4, 5} U {5, 8} = 4, 5, 8
    regions = [(3, 10, 20), (1, 5, 5), (3, 21, 30), (3, 1, None), (1, 6, 8)]
    p = host_plan(regions)
    assert E.points(full(regions)) == [[0, 9, 20, 30, E.OPEN_END], [4, 5, 8]]
    nb = (5 + 3) + 2  # P + C
    assert p.n_i64 == 4 + 4 * nb and p.n_f64 == 0
    assert p.layout() == exon_amd.region_bases_layout(p) == (0, 4, 4 + nb, 4 + 2 * nb, 4 + 3 * nb, 4 + 4 * nb) == E.layout(full(regions))
    q = host_plan([("chr1", 1, 2)] * 4 + [("chrX", 1, 2)])  # duplicates share their two points
    assert q.by_name and q.layout() == (0, 4, 4 + 6, 4 + 12, 4 + 18, 4 + 24)
    # contig 3's bins start at 0, contig 1's at (5 points) + 1: a row [7, 7] on contig 1 lands in bin 6 + 2 of Ns and of Ne
    st = E.expect_state(full(regions), [1], [7], [7])
    at = p.layout()
    assert np.flatnonzero(st).tolist() == [0, at[1] + 8, at[2] + 8, at[3] + 8, at[4] + 8]
    assert p.decode(st).tolist() == [0, 0, 0, 0, 1]


def test_decode_a_hand_made_state_with_a_single_row():
    regions = [(0, 10, 20), (0, 15, 15), (0, 21, 30), (0, 1, None)]
    p = host_plan(regions)
    at = p.layout()
    # points 0, 9, 14, 15, 20, 30, OPEN; the row [12, 22]: first point >= 12 is index 2, first point >= 22 is index 5
    st = np.zeros(p.n_i64, np.int64)
    st[0] = 1
    st[at[1] + 2], st[at[2] + 2] = 1, 12
    st[at[3] + 5], st[at[4] + 5] = 1, 22
    assert p.decode(st).tolist() == [9, 1, 2, 11]
    assert exon_amd.region_bases_decode(p, st).tolist() == [9, 1, 2, 11]
    assert np.array_equal(st, E.expect_state(full(regions), [0], [12], [22]))
    with pytest.raises(ValueError):
        p.decode(st[:-1])


def random_case(seed, shift=0):
    rng = np.random.default_rng(seed)
    m, n = int(rng.integers(1, 40)), 300
    regions = []
    for _ in range(m):
        s = int(rng.integers(1, 60))
        regions.append((int(rng.integers(0, 4)) * 2, s + shift, s + shift + int(rng.integers(0, 25)) if rng.random() < 0.9 else None))
    regions += regions[:3]  # duplicates: each has its own sum
    ref = rng.integers(-1, 9, n).astype(np.int32)
    start = rng.integers(1, 80, n) + shift
    end = start + rng.integers(-2, 20, n)  # some inverted
    rv, sv, ev = (rng.random(n) < 0.95 for _ in range(3))
    return regions, (ref, start, end, rv, sv, ev)


@pytest.mark.parametrize("shift", [0, 2**40, 2**62], ids=["small", "2^40", "2^62"])
@pytest.mark.parametrize("seed", range(6))
def test_decode_of_the_expected_state_is_the_brute_force_sum(seed, shift):
    """shift 2^40: the coordinate sums leave 32 bits far behind; 2^62: Ss and Se themselves wrap (more than four rows a bin), and
    with an open end x + 1 wraps too -- the decoded sums stay exact"""
    regions, rows = random_case(seed, shift)
    ref, start, end, rv, sv, ev = rows
    st = E.expect_state(full(regions), *rows)
    totals, bases = E.expect(full(regions), *rows)
    assert totals.sum() == len(ref) and st[:4].tolist() == totals.tolist()
    p = host_plan(regions)
    assert st.size == p.n_i64
    assert p.decode(st).tolist() == bases.tolist()
    assert E.expect_fast(full(regions), *rows)[1].tolist() == bases.tolist()
    # the second route: per-base depth, on the same case moved back to small coordinates (covered bases do not move with the origin)
    small = [(c, s - shift, e if e == E.OPEN_END else e - shift) for c, s, e in full(regions)]
    assert E.expect_pileup(small, ref, start - shift, end - shift, rv, sv, ev)[1].tolist() == bases.tolist()
    assert bases.sum() > 0
    at = p.layout()
    assert st[at[1]:at[2]].sum() == totals[0] == st[at[3]:at[4]].sum()
    # decoding is linear: two partitions' states (added with wrap)
    half = len(ref) // 2
    a = E.expect_state(full(regions), *(x[:half] for x in rows))
    b = E.expect_state(full(regions), *(x[half:] for x in rows))
    with np.errstate(over="ignore"):
        assert np.array_equal(a + b, st)
        assert np.array_equal(p.decode(a) + p.decode(b), p.decode(a + b))


def test_the_sums_wrapped_in_the_2_62_case():
    regions, rows = random_case(0, 2**62)
    st = E.expect_state(full(regions), *rows)
    at = E.layout(full(regions))
    ns, ss = st[at[1]:at[2]], st[at[2]:at[3]].view(np.uint64)
    # a bin with five rows or more holds 5 * 2^62 > 2^64: what is stored is the sum modulo 2^64
    assert ns.max() >= 5 and int(ss[ns.argmax()]) < int(ns.max()) * 2**62


def _create(n, ids=None, names=None, starts=None, ends=None, columns=(2, 3, 4)):
    lib = exon_amd.load()
    h = C.c_void_p()
    arr = lambda v, t: None if v is None else np.array(v, t)  # noqa: E731
    ids_a, st_a, en_a = arr(ids, np.int32), arr(starts, np.int64), arr(ends, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib.exon_hip_plan_create_region_set_bases(None, (C.c_int32 * 3)(*columns), names, len(names) if names else 0, ptr(ids_a), ptr(st_a), ptr(en_a), n,
                                                   C.byref(h))
    msg = lib.exon_hip_last_error(None).decode()
    if rc == 0:
        lib.exon_hip_plan_destroy(h)
    return rc, msg


def test_constructor_refusals():
    assert _create(0, [0], None, [1], [2])[0] == EINVAL
    big = 1048577
    rc, msg = _create(big, np.zeros(big, np.int32), None, np.ones(big, np.int64), np.ones(big, np.int64))
    assert rc == EUNSUPPORTED and "1048576" in msg
    assert _create(1048576, np.zeros(1048576, np.int32), None, np.ones(1048576, np.int64), np.ones(1048576, np.int64))[0] == 0
    rc, msg = _create(2, [0, 0], None, [1, 0], [5, 5])
    assert rc == EINVAL and "region 1" in msg and "1 <= start <= end" in msg
    rc, msg = _create(2, [0, 0], None, [1, 7], [5, 6])
    assert rc == EINVAL and "region 1" in msg
    rc, msg = _create(2, [0, -1], None, [1, 1], [5, 5])
    assert rc == EINVAL and "negative reference id" in msg
    assert _create(1, [1 << 24], None, [1], [5])[0] == EUNSUPPORTED
    assert _create(1, [0], None, [1], [5], columns=(0, -1, 2))[0] == EINVAL
    assert _create(1, None, None, [1], [5])[0] == EINVAL  # neither names nor ids
    assert _create(2, None, b"chr1\0", [1, 1], [5, 5])[0] == EINVAL  # one name for two regions
    assert _create(2, None, b"chr1\0\0", [1, 1], [5, 5])[0] == EINVAL  # an empty name
    assert _create(2, None, b"chr1\0chr1\0", [1, 1], [5, 2**63 - 1])[0] == 0
    assert _create(1, [0], None, [5], [5])[0] == 0  # a region of one base


def test_plan_create_refuses_kind_12_and_names_the_constructor():
    lib = exon_amd.load()
    d = L.PlanDesc(kind=L.PLAN_REGION_SET_BASES)
    h = C.c_void_p()
    assert lib.exon_hip_plan_create(None, C.byref(d), C.byref(h)) == EINVAL
    assert "use exon_hip_plan_create_region_set_bases" in lib.exon_hip_last_error(None).decode()
    assert not h.value


def test_helpers_of_kinds_11_and_12_refuse_each_others_plans_and_null():
    lib = exon_amd.load()
    out = (C.c_int64 * 6)()
    state = np.zeros(64, np.int64)
    res = np.zeros(4, np.int64)
    assert lib.exon_hip_region_bases_layout(None, out) == EINVAL
    assert lib.exon_hip_region_bases_decode(None, state.ctypes.data, res.ctypes.data) == EINVAL
    p = host_plan([(0, 1, 2)])
    assert lib.exon_hip_region_bases_layout(p.h, None) == EINVAL
    assert lib.exon_hip_region_bases_decode(p.h, None, None) == EINVAL
    k11 = exon_amd.RegionSetPlan(None, [(0, 1, 2)])
    assert lib.exon_hip_region_bases_layout(k11.h, out) == EINVAL
    assert "kind 12" in lib.exon_hip_last_error(None).decode()
    assert lib.exon_hip_region_bases_decode(k11.h, state.ctypes.data, res.ctypes.data) == EINVAL
    assert lib.exon_hip_region_set_bases(None, None, None, None, None, 0, k11.h, None) == EINVAL
    assert lib.exon_hip_region_set_layout(p.h, out) == EINVAL
    assert "kind 11" in lib.exon_hip_last_error(None).decode()
    assert lib.exon_hip_region_set_decode(p.h, state.ctypes.data, res.ctypes.data) == EINVAL
    assert lib.exon_hip_region_set_overlap(None, None, None, None, None, 0, p.h, None) == EINVAL
    # a host-only plan cannot be executed
    h = C.c_void_p()
    assert lib.exon_hip_stream_open(p.h, 0, C.byref(h)) == EINVAL
    assert "host-only" in lib.exon_hip_last_error(None).decode()
    p.close()
    k11.close()
