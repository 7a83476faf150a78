"""No GPU: the Python statement of the aligned-blocks rule (cigar_blocks_expect.py) against a brute-force set of covered positions,
and exon_hip_cigar_blocks_host == it on the same inputs: a few thousand random CIGARs over all 16 op codes, zero-length ops
included, under every one of the 31 legal masks.  Then the host function's error classes, and the names in every layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L
from exon_amd.engine import cigar_blocks_host, cover_ops_mask

import cigar_blocks_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECAPACITY = -1, -6


def random_cigars(rng, n):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, 13))
        codes = rng.integers(0, 16, k) if rng.random() < 0.5 else rng.choice([0, 0, 0, 1, 2, 3, 4, 7, 8], k)
        lens = rng.choice([0, 0, 1, 1, 2, 3, 5, 9], k)
        out.append([(int(ln), int(c)) for ln, c in zip(lens, codes)])
    return out


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(20)
    cigars = random_cigars(rng, 3000)
    starts = rng.choice([1, 1, 2, 100, 0, -3, 2**31 - 1, 2**40], len(cigars))
    return [(c, int(s)) for c, s in zip(cigars, starts)]


def test_there_are_31_legal_masks_and_the_named_ones_are_among_them():
    assert len(E.LEGAL_MASKS) == 31 and E.ALIGNED in E.LEGAL_MASKS and E.ALIGNED_DEL in E.LEGAL_MASKS and E.LEGAL in E.LEGAL_MASKS
    assert E.ALIGNED == sum(1 << "MIDNSHP=X".index(c) for c in "M=X") and E.ALIGNED_DEL == E.ALIGNED | 1 << 2


def test_the_examples_of_the_header():
    assert E.blocks(E.cigar("10M5I10M"), 100, E.ALIGNED) == [(100, 119)]
    assert E.blocks(E.cigar("5M0N5M"), 1, E.ALIGNED) == [(1, 10)]
    assert E.blocks(E.cigar("5M3D5M"), 1, E.ALIGNED) == [(1, 5), (9, 13)]
    assert E.blocks(E.cigar("5M3D5M"), 1, E.ALIGNED_DEL) == [(1, 13)]
    assert E.blocks(E.cigar("50M10000N50M"), 1000, E.ALIGNED_DEL) == [(1000, 1049), (11050, 11099)]
    assert E.blocks(E.cigar("50M10000N50M"), 1000, E.LEGAL) == [(1000, 11099)]
    assert E.blocks(E.cigar("0M"), 7, E.ALIGNED) == [] == E.blocks(E.cigar("5S3I"), 7, E.LEGAL) == E.blocks([], 7, E.ALIGNED)
    assert E.blocks(E.cigar("4N"), 7, 1 << 3) == [(7, 10)] and E.blocks(E.cigar("4N"), 7, E.ALIGNED) == []
    assert E.blocks([(3, 9), (2, 0), (4, 15), (2, 0)], 1, E.ALIGNED) == [(1, 4)]  # codes 9 .. 15 advance nothing


def test_expectation_against_brute_force(cases):
    seen = set()
    for ops, start in cases:
        for mask in E.LEGAL_MASKS:
            got = E.blocks(ops, start, mask)
            assert got == E.runs(E.covered_positions(ops, start, mask)), (ops, start, hex(mask))
            seen.add(min(len(got), 4))
    assert seen == {0, 1, 2, 3, 4}


def test_the_span_mask_gives_one_block_equal_to_the_span(cases):
    for ops, start in cases:
        span = sum(ln for ln, c in ops if c in E.REF_CODES)
        assert E.blocks(ops, start, E.LEGAL) == ([(start, start + span - 1)] if span else [])


def test_host_function_equals_the_expectation(cases):
    for ops, start in cases:
        enc = E.encode(ops)
        for mask in E.LEGAL_MASKS:
            assert cigar_blocks_host(enc, start, mask) == E.blocks(ops, start, mask), (ops, start, hex(mask))


def test_host_function_takes_the_longest_ops_and_the_names():
    top = (1 << 28) - 1
    assert cigar_blocks_host(E.encode([(top, 0), (top, 3), (top, 8)]), 1, "aligned") == [(1, top), (2 * top + 1, 3 * top)]
    assert cigar_blocks_host(E.encode(E.cigar("5M3D5M")), 1, "aligned+del") == [(1, 13)]
    assert cover_ops_mask("aligned") == L.COVER_ALIGNED == 0x181 and cover_ops_mask("aligned+del") == L.COVER_ALIGNED_DEL == 0x185
    with pytest.raises(ValueError):
        cover_ops_mask("span")


@pytest.mark.parametrize("mask", [0, 0x2, 0x10, 0x20, 0x40, 0x200, 0x18D | 0x2, 0x8000, 1 << 16, 0xFFFFFFFF])
def test_host_function_refuses_illegal_mask_bits(mask):
    with pytest.raises(exon_amd.ExonHipError) as e:
        cigar_blocks_host(E.encode(E.cigar("5M")), 1, mask)
    assert e.value.code == EINVAL and "0x18D" in str(e.value)


def test_host_function_capacity_and_empty_input():
    lib = exon_amd.load()
    ops = E.encode(E.cigar("1M1N" * 5))
    want = E.blocks(E.cigar("1M1N" * 5), 10, E.ALIGNED)
    assert len(want) == 5
    assert cigar_blocks_host(ops, 10, E.ALIGNED, cap=5) == want
    for cap in (4, 1, 0):
        s, e = np.full(8, -7, np.int64), np.full(8, -7, np.int64)
        k = C.c_int32(-1)
        rc = lib.exon_hip_cigar_blocks_host(ops.ctypes.data, len(ops), 10, E.ALIGNED, s.ctypes.data, e.ctypes.data, cap, C.byref(k))
        assert rc == ECAPACITY and k.value == 5
        assert list(zip(s[:cap].tolist(), e[:cap].tolist())) == want[:cap] and (s[cap:] == -7).all() and (e[cap:] == -7).all()
    k = C.c_int32(-1)
    assert lib.exon_hip_cigar_blocks_host(ops.ctypes.data, len(ops), 10, E.ALIGNED, None, None, 0, C.byref(k)) == ECAPACITY and k.value == 5  # the need alone
    assert lib.exon_hip_cigar_blocks_host(None, 0, 10, E.ALIGNED, None, None, 0, C.byref(k)) == 0 and k.value == 0                             # n_ops = 0
    assert cigar_blocks_host([], 10, E.ALIGNED) == []
    assert lib.exon_hip_cigar_blocks_host(None, 3, 10, E.ALIGNED, None, None, 0, C.byref(k)) == EINVAL
    assert lib.exon_hip_cigar_blocks_host(ops.ctypes.data, -1, 10, E.ALIGNED, None, None, 0, C.byref(k)) == EINVAL
    assert lib.exon_hip_cigar_blocks_host(ops.ctypes.data, len(ops), 10, E.ALIGNED, None, None, -1, C.byref(k)) == EINVAL
    assert lib.exon_hip_cigar_blocks_host(ops.ctypes.data, len(ops), 10, E.ALIGNED, None, None, 5, C.byref(k)) == EINVAL
    assert lib.exon_hip_cigar_blocks_host(ops.ctypes.data, len(ops), 10, E.ALIGNED, None, None, 0, None) == EINVAL


def test_pileup_of_block_rows_is_the_covered_positions(cases):
    rng = np.random.default_rng(21)
    picked = [cases[i] for i in rng.choice(len(cases), 200, replace=False)]
    cig = [c for c, _ in picked]
    ref = rng.integers(0, 3, len(cig))
    start = rng.integers(1, 60, len(cig))
    for mask in (E.ALIGNED, E.ALIGNED_DEL, E.LEGAL):
        r, s, e, v = E.expand(ref, start, cig, mask)
        assert v.all() and (e >= s - 1).all()
        want = np.zeros((3, 201), np.int64)
        for c, st, rf in zip(cig, start, ref):
            for x in E.covered_positions(c, int(st), mask):
                want[rf, x] += 1
        assert np.array_equal(E.pileup(3, 200, r, s, e, v), want)


def test_every_layer_carries_the_names():
    lib = exon_amd.load()
    header = open(os.path.join(ROOT, "include", "exon_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    assert callable(exon_amd.Scan.set_cover_ops)
    assert hasattr(lib, "exon_hip_bam_parser_cigar_blocks") and re.search(r"\bint exon_hip_bam_parser_cigar_blocks\(", header)
    for name in ("exon_hip_cigar_blocks", "exon_hip_cigar_blocks_host", "exon_hip_scan_set_cover_ops"):
        assert hasattr(lib, name) and name in L.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header) and re.search(r"\bpub fn %s\(" % name, sys_rs)
    assert re.search(r"#define EXON_HIP_COVER_ALIGNED 0x181u\b", header) and re.search(r"#define EXON_HIP_COVER_ALIGNED_DEL 0x185u\b", header)
    assert "pub const EXON_HIP_COVER_ALIGNED: u32 = 0x181;" in sys_rs and "pub const EXON_HIP_COVER_ALIGNED_DEL: u32 = 0x185;" in sys_rs
    assert lib.exon_hip_abi_version() == 5  # additive
    assert callable(exon_amd.Context.cigar_blocks) and "cigar_blocks_host" in exon_amd.__all__
    assert "cigar_blocks.o" in open(os.path.join(ROOT, "exon_amd", "csrc", "Makefile")).read()
    rule = open(os.path.join(ROOT, "exon_amd", "csrc", "host", "cigar_blocks.h")).read()
    assert "walk_blocks" in rule and "DECISIONS" in rule and "CG" in rule
    hip = open(os.path.join(ROOT, "exon_amd", "csrc", "cigar_blocks.hip")).read()
    assert hip.count("walk_blocks(") == 1 and "count_blocks(" in hip  # the two passes call the header's one walk
