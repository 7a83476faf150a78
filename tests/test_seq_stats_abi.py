"""No GPU: the per-record sequence statistics plan (kind 10) is declared in every layer -- the built library, the ctypes table, the
public header and the Rust shim's prototypes --, its host-only layout helper answers, and the expectation module the GPU tests
compare against gives the pinned numbers on the reference's own FASTA fixture."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L

import seq_stats_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["exon_hip_seq_stats_hist", "exon_hip_seq_stats_hist_views", "exon_hip_seq_stats_layout"]
CONSTANT = "EXON_HIP_PLAN_SEQ_STATS_HIST"


def test_every_layer_carries_the_names_and_the_constant():
    lib = exon_amd.load()
    header = open(os.path.join(ROOT, "include", "exon_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
        assert re.search(r"\bint %s\(" % name, header), name
        assert re.search(r"\bpub fn %s\(" % name, sys_rs), name
    assert re.search(r"#define %s 10\b" % CONSTANT, header)
    assert re.search(r"pub const %s: i32 = 10;" % CONSTANT, sys_rs)
    assert L.PLAN_SEQ_STATS_HIST == 10
    assert lib.exon_hip_abi_version() == 5  # additive
    for attr in ("seq_stats_hist", "seq_stats_hist_views", "plan_seq_stats_hist"):
        assert callable(getattr(exon_amd.Context, attr)), attr
    assert callable(exon_amd.seq_stats_layout) and "seq_stats_layout" in exon_amd.__all__
    cli = open(os.path.join(ROOT, "exon_amd", "csrc", "cli.cpp")).read()
    assert cli.count("fasta_seq_stats") >= 3  # the head comment, the query, the usage text
    assert "seq_stats.o" in open(os.path.join(ROOT, "exon_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("lmax", [1, 100, 2046, 65536])
def test_layout(lmax):
    want = (0, 3, 259, 259 + lmax + 2, 259 + lmax + 2 + 32, 259 + lmax + 2 + 32 + 102)
    assert exon_amd.seq_stats_layout(lmax) == want == E.layout(lmax)
    assert want[5] == 3 + 256 + (lmax + 2) + 32 + 102


@pytest.mark.parametrize("lmax", [0, 65537, -1])
def test_layout_refuses_lmax_out_of_range(lmax):
    with pytest.raises(exon_amd.ExonHipError) as e:
        exon_amd.seq_stats_layout(lmax)
    assert e.value.code == -1 and "out of range" in str(e.value)  # EXON_HIP_EINVAL
    out = (C.c_int64 * 6)()
    assert exon_amd.load().exon_hip_seq_stats_layout(lmax, out) == -1
    assert exon_amd.load().exon_hip_seq_stats_layout(100, None) == -1


def test_expectation_on_the_reference_fixture():
    text = open(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "fasta", "test.fasta"), "rb").read()
    seqs = E.sequences(text)
    at = E.layout(512)
    for st in (E.expect(seqs, 512), E.expect_fast(seqs, 512), E.from_text(text, 512)):
        assert st[:3].tolist() == [2, 8, 4]
        assert [int(st[at[1] + b]) for b in b"ACGT"] == [2, 2, 2, 2] and st[at[1]:at[2]].sum() == 8
        assert st[at[2] + 4] == 2 and st[at[2]:at[3]].sum() == 2
        assert st[at[3] + 3] == 2 and st[at[3]:at[4]].sum() == 2
        assert st[at[4] + 50] == 2 and st[at[4]:at[5]].sum() == 2
        assert E.identities(st, 512)


def test_expectation_forms_agree_on_edge_records():
    rng = np.random.default_rng(3)
    seqs = [b"", b"", b"G", b"gcGC", bytes(range(256)), b"C" * 65536, b"A" * 65537, b"N" * 1023, b"N" * 1024]
    seqs += [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 300, 50)]
    for lmax in (1, 300, 65536):
        a = E.expect(seqs, lmax)
        assert np.array_equal(a, E.expect_fast(seqs, lmax)) and E.identities(a, lmax)
        at = E.layout(lmax)
        assert a[at[4] + 101] == 2 and a[at[3]] == 2 and a[at[4] + 50] >= 1  # 'gcGC': two of four
        assert a[at[3] + 10] >= 1 and a[at[3] + 11] >= 1 and a[at[3] + 17] == 2  # 1023 | 1024 | 65536, 65537
        assert a[at[2] + lmax + 1] >= (1 if lmax == 65536 else 4)
    assert not E.expect_fast([], 5).any() and not E.expect([], 5).any()


def test_from_text_follows_the_fasta_rules():
    text = b"stray\n>a\r\nAC\r\nG T\n\n>b\n>c x\nG>C\rA\n"
    assert E.sequences(text) == [b"ACG T", b"", b"G>C\rA"]
    assert np.array_equal(E.from_text(text, 8), E.expect([b"ACG T", b"", b"G>C\rA"], 8))
