"""No GPU: the window plan (kind 13) is declared in every layer, its constructor refuses what the header says it refuses, and its
host-only helpers -- layout, offsets and decode -- answer on hand-made and on expected states, modulo 2^64.  A plan created without a
context is host-only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L

import window_bases_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["exon_hip_plan_create_window_bases", "exon_hip_window_bases_layout", "exon_hip_window_bases_offsets", "exon_hip_window_bases_decode",
         "exon_hip_window_bases", "exon_hip_scan_reference_lengths"]
EINVAL, EUNSUPPORTED = -1, -4


def host_plan(contigs, W, columns=(2, 3, 4)):
    return exon_amd.WindowBasesPlan(None, contigs, W, columns)


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
    assert re.search(r"#define EXON_HIP_PLAN_WINDOW_BASES 13\b", header)
    assert re.search(r"#define EXON_HIP_WINDOW_MAX_BINS %d\b" % (1 << 25), header)
    assert re.search(r"pub const EXON_HIP_PLAN_WINDOW_BASES: i32 = 13;", sys_rs)
    assert L.PLAN_WINDOW_BASES == 13 and L.WINDOW_MAX_BINS == 1 << 25
    assert lib.exon_hip_abi_version() == 5  # additive
    # the tier bound the GPU tests aim at is the kernel's own: two u64 bins a window, inside the 160 KiB a workgroup may take
    bound = int(re.search(r"constexpr int WINDOW_BASES_LDS_MAX = (\d+);", kernels_h).group(1))
    assert bound == exon_amd.WINDOW_BASES_LDS_MAX == L.WINDOW_BASES_LDS_MAX == 8192
    assert 16 * bound <= 160 * 1024
    assert "launch_window_bases" in kernels_h and "struct WindowBasesTables" in kernels_h
    for attr in ("plan_window_bases", "window_bases"):
        assert callable(getattr(exon_amd.Context, attr)), attr
    assert callable(exon_amd.Scan.reference_lengths)
    for name in ("WindowBasesPlan", "WINDOW_BASES_LDS_MAX"):
        assert name in exon_amd.__all__
    assert "window_bases.o" in open(os.path.join(ROOT, "exon_amd", "csrc", "Makefile")).read()
    assert "k_window_bases" in open(os.path.join(ROOT, "exon_amd", "csrc", "window_bases.hip")).read()
    k13 = header[header.index("K13:"):header.index("#define EXON_HIP_PLAN_WINDOW_BASES")]
    assert "DECISIONS" in k13 and "CLIPPED" in k13 and "CIGAR" in k13 and "per-base track" in k13 and "BED source" in k13


@pytest.mark.parametrize("lengths,W", [
    ([35], 10), ([5], 10), ([10], 10), ([11], 10), ([7, 1, 3], 1), ([1], 1), ([999, 1000, 1001, 2500], 1000), ([2**31 - 1], 2**31 - 1),
    ([2**31 - 1], 2**20 + 1), ([2**31 - 1, 4], 2**40), ([100, 200, 300], 64)])
def test_layout_offsets_and_state_size(lengths, W):
    contigs = [(3 * c, ln) for c, ln in enumerate(lengths)]
    p = host_plan(contigs, W)
    k = [-(-ln // W) for ln in lengths]
    B = sum(k)
    assert p.n_i64 == 4 + 2 * B and p.n_f64 == 0
    assert p.layout() == (0, 4, 4 + B, 4 + 2 * B)
    assert p.offsets().tolist() == np.concatenate([[0], np.cumsum(k)]).tolist() == E.offsets(contigs, W).tolist()
    assert p.decode(np.zeros(p.n_i64, np.int64)).tolist() == [0] * B
    p.close()


def test_decode_hand_made_states():
    p = host_plan([(0, 35), (7, 12)], 10)  # windows 1-10, 11-20, 21-30, 31-35 | 1-10, 11-12
    at = p.layout()
    assert at == (0, 4, 10, 16) and p.offsets().tolist() == [0, 4, 6]
    st = np.zeros(16, np.int64)
    st[at[1] + 0], st[at[1] + 2] = 6, 5    # the row [5, 25] on contig 0: the ends
    st[at[2] + 1], st[at[2] + 2] = 1, -1   # ... and window 1 whole
    assert p.decode(st).tolist() == [6, 10, 5, 0, 0, 0]
    assert np.array_equal(st[4:], E.expect_state([(0, 35), (7, 12)], 10, [0], [5], [25])[4:])
    # the running sum of D stops at the contig's end: a +1 left open on contig 0 does not reach contig 7
    st = np.zeros(16, np.int64)
    st[at[2] + 3] = 1
    assert p.decode(st).tolist() == [0, 0, 0, 10, 0, 0]
    # modulo 2^64: E = 2^64 - 10 and one whole window on top is 0
    st = np.zeros(16, np.int64)
    st[at[1] + 5], st[at[2] + 5] = -10, 1
    assert p.decode(st).tolist() == [0, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError):
        p.decode(st[:-1])
    p.close()


@pytest.mark.parametrize("W", [1, 3, 7, 64, 1000])
def test_decode_of_the_expected_state_is_the_pileup_and_is_linear(W):
    rng = np.random.default_rng(100 + W)
    contigs = [(c, ln) for c, ln in enumerate([1, 5, 999, 1000, 1001, 2500])]
    n = 3000
    ref = rng.integers(-1, 8, n).astype(np.int32)
    start = rng.integers(-20, 2600, n)
    end = start + rng.integers(-3, 3 * W + 100, n)
    rows = (ref, start, end) + tuple(rng.random(n) < 0.95 for _ in range(3))
    p = host_plan(contigs, W)
    st = E.expect_state(contigs, W, *rows)
    totals, bases = E.expect(contigs, W, *rows)
    assert st.size == p.n_i64 and st[:4].tolist() == totals.tolist()
    assert p.decode(st).tolist() == bases.tolist() == E.decode(contigs, W, st).tolist()
    assert bases.sum() > 0
    half = n // 2
    a = E.expect_state(contigs, W, *(x[:half] for x in rows))
    b = E.expect_state(contigs, W, *(x[half:] for x in rows))
    with np.errstate(over="ignore"):
        assert np.array_equal(a + b, st)
        assert np.array_equal(p.decode(a) + p.decode(b), p.decode(a + b))
        junk = rng.integers(-2**63, 2**63 - 1, p.n_i64)  # any words at all: decode is a ring homomorphism
        assert np.array_equal(p.decode(junk) + p.decode(st), p.decode(junk + st))
    p.close()


def _create(n, ids=None, names=None, lengths=None, W=10, columns=(2, 3, 4)):
    lib = exon_amd.load()
    h = C.c_void_p()
    arr = lambda v, t: None if v is None else np.array(v, t)  # noqa: E731
    ids_a, len_a = arr(ids, np.int32), arr(lengths, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib.exon_hip_plan_create_window_bases(None, (C.c_int32 * 3)(*columns), names, len(names) if names else 0, ptr(ids_a), ptr(len_a), n, W, C.byref(h))
    msg = lib.exon_hip_last_error(None).decode()
    if rc == 0:
        lib.exon_hip_plan_destroy(h)
    return rc, msg


def test_constructor_refusals():
    assert _create(1, [0], None, [35])[0] == 0
    assert _create(0, [0], None, [35])[0] == EINVAL
    rc, msg = _create(2, [0, -1], None, [5, 5])
    assert rc == EINVAL and "contig 1" in msg and "negative reference id" in msg
    assert _create(1, [1 << 24], None, [5])[0] == EUNSUPPORTED
    assert _create(1, [(1 << 24) - 1], None, [5])[0] == 0
    assert _create(2, None, b"chr1\0", [5, 5])[0] == EINVAL    # one name for two contigs
    assert _create(2, None, b"chr1\0\0", [5, 5])[0] == EINVAL  # an empty name
    assert _create(2, None, b"chr1\0chr2\0", [5, 5])[0] == 0
    rc, msg = _create(3, [4, 9, 4], None, [5, 5, 5])
    assert rc == EINVAL and "contig 2" in msg and "twice" in msg
    rc, msg = _create(2, None, b"chrX\0chrX\0", [5, 6])
    assert rc == EINVAL and "chrX" in msg and "twice" in msg
    for w in (0, -1, -2**63):
        rc, msg = _create(1, [0], None, [35], W=w)
        assert rc == EINVAL and "window" in msg
    for ln in (0, -1, 2**31, 2**40):
        rc, msg = _create(2, [0, 1], None, [35, ln])
        assert rc == EINVAL and "contig 1" in msg and "length" in msg
    assert _create(1, [0], None, [2**31 - 1], W=64)[0] == 0  # 2^25 windows exactly
    rc, msg = _create(2, [0, 1], None, [2**31 - 1, 1], W=64)  # ... and one more
    assert rc == EUNSUPPORTED and str(1 << 25) in msg
    rc, msg = _create(1, [0], None, [(1 << 25) + 1], W=1)
    assert rc == EUNSUPPORTED and str((1 << 25) + 1) in msg
    assert _create(1, [0], None, [1 << 25], W=1)[0] == 0
    assert _create(1, [0], None, [35], columns=(0, -1, 2))[0] == EINVAL
    assert _create(1, None, None, [35])[0] == EINVAL  # neither names nor ids
    assert _create(1, [0], None, None)[0] == EINVAL   # no lengths


def test_plan_create_refuses_kind_13_and_names_the_constructor():
    lib = exon_amd.load()
    d = L.PlanDesc(kind=L.PLAN_WINDOW_BASES)
    h = C.c_void_p()
    assert lib.exon_hip_plan_create(None, C.byref(d), C.byref(h)) == EINVAL
    assert "use exon_hip_plan_create_window_bases" in lib.exon_hip_last_error(None).decode()
    assert not h.value


def test_helpers_refuse_the_other_kinds_plans_and_null():
    lib = exon_amd.load()
    out = (C.c_int64 * 6)()
    state = np.zeros(64, np.int64)
    res = np.zeros(8, np.int64)
    assert lib.exon_hip_window_bases_layout(None, out) == EINVAL
    assert lib.exon_hip_window_bases_offsets(None, res.ctypes.data) == EINVAL
    assert lib.exon_hip_window_bases_decode(None, state.ctypes.data, res.ctypes.data) == EINVAL
    p = host_plan([(0, 35)], 10)
    assert lib.exon_hip_window_bases_layout(p.h, None) == EINVAL
    assert lib.exon_hip_window_bases_offsets(p.h, None) == EINVAL
    assert lib.exon_hip_window_bases_decode(p.h, None, None) == EINVAL
    others = [exon_amd.RegionSetPlan(None, [(0, 1, 2)]), exon_amd.RegionBasesPlan(None, [(0, 1, 2)])]
    for k in others:  # kind 13's helpers on kinds 11 and 12
        assert lib.exon_hip_window_bases_layout(k.h, out) == EINVAL
        assert "kind 13" in lib.exon_hip_last_error(None).decode()
        assert lib.exon_hip_window_bases_offsets(k.h, res.ctypes.data) == EINVAL
        assert lib.exon_hip_window_bases_decode(k.h, state.ctypes.data, res.ctypes.data) == EINVAL
        assert lib.exon_hip_window_bases(None, None, None, None, None, 0, k.h, None) == EINVAL
    # kind 11's and 12's helpers on kind 13
    assert lib.exon_hip_region_set_layout(p.h, out) == EINVAL
    assert "kind 11" in lib.exon_hip_last_error(None).decode()
    assert lib.exon_hip_region_set_decode(p.h, state.ctypes.data, res.ctypes.data) == EINVAL
    assert lib.exon_hip_region_set_overlap(None, None, None, None, None, 0, p.h, None) == EINVAL
    assert lib.exon_hip_region_bases_layout(p.h, out) == EINVAL
    assert "kind 12" in lib.exon_hip_last_error(None).decode()
    assert lib.exon_hip_region_bases_decode(p.h, state.ctypes.data, res.ctypes.data) == EINVAL
    assert lib.exon_hip_region_set_bases(None, None, None, None, None, 0, p.h, None) == EINVAL
    # a host-only plan cannot be executed
    h = C.c_void_p()
    assert lib.exon_hip_stream_open(p.h, 0, C.byref(h)) == EINVAL
    assert "host-only" in lib.exon_hip_last_error(None).decode()
    p.close()
    for k in others:
        k.close()


def test_names_form_host_plan():
    p = host_plan([("chr2", 25), ("chr1", 10)], 10)
    assert p.by_name and p.offsets().tolist() == [0, 3, 4] and p.layout() == (0, 4, 8, 12)
    p.close()
    with pytest.raises(ValueError):
        host_plan([("chr2", 25), (1, 10)], 10)
