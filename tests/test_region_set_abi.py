"""No GPU: the region-set overlap plan (kind 11) is declared in every layer, its constructor refuses what the header says it refuses,
and its host-only helpers -- layout and decode -- answer on hand-made states.  A plan created without a context is host-only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L

import region_set_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["exon_hip_plan_create_region_set", "exon_hip_region_set_layout", "exon_hip_region_set_decode", "exon_hip_region_set_overlap"]
EINVAL, EUNSUPPORTED = -1, -4


def host_plan(regions, columns=(2, 3, 4)):
    return exon_amd.RegionSetPlan(None, regions, columns)


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
    assert re.search(r"#define EXON_HIP_PLAN_REGION_SET_OVERLAP 11\b", header)
    assert re.search(r"pub const EXON_HIP_PLAN_REGION_SET_OVERLAP: i32 = 11;", sys_rs)
    assert L.PLAN_REGION_SET_OVERLAP == 11
    assert lib.exon_hip_abi_version() == 5  # additive
    # the tier bound and the tiles the GPU tests aim at are the kernel's own
    assert int(re.search(r"constexpr int REGION_SET_LDS_MAX = (\d+);", kernels_h).group(1)) == exon_amd.REGION_SET_LDS_MAX == L.REGION_SET_LDS_MAX
    assert re.search(r"constexpr int RS_J = 2;", kernels_h) and re.search(r"RS_TILE_SMALL = 4 \* 256 \* RS_J, RS_TILE_BIG = 16 \* 256 \* RS_J;", kernels_h)
    assert (L.REGION_SET_TILE_SMALL, L.REGION_SET_TILE_BIG) == (2048, 8192)
    assert L.REGION_SET_MAX_REGIONS == 1048576 and re.search(r"#define EXON_HIP_REGION_SET_MAX_REGIONS 1048576\b", header)
    # 24 bytes of LDS per word of the bound, inside the CU's 160 KiB
    assert 24 * exon_amd.REGION_SET_LDS_MAX <= 160 * 1024
    for attr in ("plan_region_set_overlap", "region_set_overlap"):
        assert callable(getattr(exon_amd.Context, attr)), attr
    for name in ("region_set_layout", "region_set_decode", "RegionSetPlan", "REGION_SET_LDS_MAX"):
        assert name in exon_amd.__all__
    assert "region_set.o" in open(os.path.join(ROOT, "exon_amd", "csrc", "Makefile")).read()
    assert "DECISION" in header and "inverted" in header


def test_layout():
    p = host_plan([(3, 10, 20), (1, 5, 5), (3, 1, None), (7, 2, 9), (1, 6, 8)])
    assert p.n_i64 == 4 + 2 * (5 + 3) and p.n_f64 == 0
    assert p.layout() == exon_amd.region_set_layout(p) == (0, 4, 12, 20) == E.layout(p.regions)
    q = host_plan([("chr1", 1, 2)] * 4 + [("chrX", 1, 2)])
    assert q.by_name and q.layout() == (0, 4, 4 + (5 + 2), 4 + 2 * (5 + 2))


def test_decode_hand_made_states_with_ties():
    # one contig, ends (20, 20, 30) and starts (10, 5, 10): ties in both orders
    regions = [(0, 10, 20), (0, 5, 20), (0, 10, 30)]
    p = host_plan(regions)
    at = p.layout()
    st = np.zeros(p.n_i64, np.int64)
    # a row [21, 25]: p = ends below 21 = 2, q = starts <= 25 = 3 -> only region 2 holds it
    st[at[1] + 2] += 1
    st[at[2] + 3] += 1
    assert p.decode(st).tolist() == [0, 0, 1]
    # a row [6, 9]: p = 0, q = 1 (start 5) -> region 1 alone
    st[at[1] + 0] += 1
    st[at[2] + 1] += 1
    assert p.decode(st).tolist() == [0, 1, 1]
    # a row [1, 4]: p = 0, q = 0 -> nobody; a row [20, 20]: p = 0, q = 3 -> everybody
    st[at[1] + 0] += 2
    st[at[2] + 0] += 1
    st[at[2] + 3] += 1
    assert p.decode(st).tolist() == [1, 2, 2]
    assert exon_amd.region_set_decode(p, st).tolist() == [1, 2, 2]
    with pytest.raises(ValueError):
        p.decode(st[:-1])


@pytest.mark.parametrize("seed", range(6))
def test_decode_of_the_expected_state_is_the_brute_force_count(seed):
    rng = np.random.default_rng(seed)
    m, n = int(rng.integers(1, 40)), 300
    regions = []
    for _ in range(m):
        s = int(rng.integers(1, 60))
        regions.append((int(rng.integers(0, 4)) * 2, s, s + int(rng.integers(0, 25)) if rng.random() < 0.9 else None))
    regions += regions[:3]  # duplicates: each has its own count
    ref = rng.integers(-1, 9, n).astype(np.int32)
    start = rng.integers(1, 80, n)
    end = start + rng.integers(-2, 20, n)  # some inverted
    rv, sv, ev = (rng.random(n) < 0.95 for _ in range(3))
    full = [(c, s, E.OPEN_END if e is None else e) for c, s, e in regions]
    st = E.expect_state(full, ref, start, end, rv, sv, ev)
    totals, counts = E.expect(full, ref, start, end, rv, sv, ev)
    assert totals.sum() == n and st[:4].tolist() == totals.tolist()
    p = host_plan(regions)
    assert st.size == p.n_i64
    assert p.decode(st).tolist() == counts.tolist()
    assert E.expect_fast(full, ref, start, end, rv, sv, ev)[1].tolist() == counts.tolist()
    # decoding is linear: two partitions' states
    half = n // 2
    a = E.expect_state(full, ref[:half], start[:half], end[:half], rv[:half], sv[:half], ev[:half])
    b = E.expect_state(full, ref[half:], start[half:], end[half:], rv[half:], sv[half:], ev[half:])
    assert np.array_equal(a + b, st)
    assert np.array_equal(p.decode(a) + p.decode(b), p.decode(a + b))


def _create(n, ids=None, names=None, starts=None, ends=None, columns=(2, 3, 4)):
    lib = exon_amd.load()
    h = C.c_void_p()
    arr = lambda v, t: None if v is None else np.array(v, t)  # noqa: E731
    ids_a, st_a, en_a = arr(ids, np.int32), arr(starts, np.int64), arr(ends, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib.exon_hip_plan_create_region_set(None, (C.c_int32 * 3)(*columns), names, len(names) if names else 0, ptr(ids_a), ptr(st_a), ptr(en_a), n, C.byref(h))
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


def test_plan_create_refuses_kind_11_and_names_the_constructor():
    lib = exon_amd.load()
    d = L.PlanDesc(kind=L.PLAN_REGION_SET_OVERLAP)
    h = C.c_void_p()
    assert lib.exon_hip_plan_create(None, C.byref(d), C.byref(h)) == EINVAL
    assert "use exon_hip_plan_create_region_set" in lib.exon_hip_last_error(None).decode()
    assert not h.value


def test_helpers_refuse_other_plans_and_null():
    lib = exon_amd.load()
    out = (C.c_int64 * 4)()
    assert lib.exon_hip_region_set_layout(None, out) == EINVAL
    p = host_plan([(0, 1, 2)])
    assert lib.exon_hip_region_set_layout(p.h, None) == EINVAL
    assert lib.exon_hip_region_set_decode(p.h, None, None) == EINVAL
    # a host-only plan cannot be executed
    h = C.c_void_p()
    assert lib.exon_hip_stream_open(p.h, 0, C.byref(h)) == EINVAL
    assert "host-only" in lib.exon_hip_last_error(None).decode()
    p.close()
