"""No GPU: the per-read FASTQ statistics plan (kind 9) is declared in every layer -- the built library, the ctypes table, the
public header and the Rust shim's prototypes --, its host-only layout helper answers, and the expectation module the GPU tests
compare against gives the pinned numbers on the reference's own fixture."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import exon_amd
from exon_amd import _lib as L

import read_stats_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["exon_hip_read_stats_hist", "exon_hip_read_stats_hist_views", "exon_hip_read_stats_layout"]
CONSTANT = "EXON_HIP_PLAN_READ_STATS_HIST"


def test_every_layer_carries_the_names_and_the_constant():
    lib = exon_amd.load()
    header = open(os.path.join(ROOT, "include", "exon_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
        assert re.search(r"\bint %s\(" % name, header), name
        assert re.search(r"\bpub fn %s\(" % name, sys_rs), name
    assert re.search(r"#define %s 9\b" % CONSTANT, header)
    assert re.search(r"pub const %s: i32 = 9;" % CONSTANT, sys_rs)
    assert L.PLAN_READ_STATS_HIST == 9
    assert lib.exon_hip_abi_version() == 5  # additive
    for attr in ("read_stats_hist", "read_stats_hist_views", "plan_read_stats_hist"):
        assert callable(getattr(exon_amd.Context, attr)), attr
    assert callable(exon_amd.read_stats_layout)


@pytest.mark.parametrize("lmax", [1, 100, 65536])
def test_layout(lmax):
    want = (0, 4, 4 + lmax + 1, 4 + lmax + 1 + 102, 4 + lmax + 1 + 102 + 257)
    assert exon_amd.read_stats_layout(lmax) == want == E.layout(lmax)


@pytest.mark.parametrize("lmax", [0, 65537, -1])
def test_layout_refuses_lmax_out_of_range(lmax):
    with pytest.raises(exon_amd.ExonHipError) as e:
        exon_amd.read_stats_layout(lmax)
    assert e.value.args[0] == -1 or "out of range" in str(e.value)  # EXON_HIP_EINVAL
    out = (C.c_int64 * 5)()
    assert exon_amd.load().exon_hip_read_stats_layout(lmax, out) == -1
    assert exon_amd.load().exon_hip_read_stats_layout(100, None) == -1


def test_expectation_on_the_reference_fixture():
    reads = E.read_fastq(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "fastq", "test.fastq"))
    assert [(len(s), len(q)) for s, q in reads] == [(64, 60), (64, 60)]  # each line by its own length
    for st in (E.expect(reads, 512), E.expect_fast([s for s, _ in reads], [q for _, q in reads], 512)):
        at = E.layout(512)
        assert st[:4].tolist() == [2, 128, 34, 5768]
        assert st[at[1] + 64] == 2 and st[at[1]:at[2]].sum() == 2
        assert st[at[2] + 26] == 2 and st[at[2]:at[3]].sum() == 2
        assert st[at[3] + 48] == 2 and st[at[3]:at[4]].sum() == 2  # Phred 15
    for name in ("test.fastq.gz", "test_bgzip.fastq.gz"):
        assert E.read_fastq(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "fastq", name)) == reads


def test_expectation_forms_agree_on_edge_reads():
    rng = np.random.default_rng(3)
    reads = [(b"", b""), (b"", b"I"), (b"G", b""), (b"gcGC", b"\xff\x00"), (bytes(range(256)), bytes(range(256)))]
    reads += [(rng.integers(0, 256, int(n), dtype=np.uint8).tobytes(), rng.integers(0, 256, int(m), dtype=np.uint8).tobytes())
              for n, m in rng.integers(0, 300, (50, 2))]
    a = E.expect(reads, 300)
    assert np.array_equal(a, E.expect_fast([s for s, _ in reads], [q for _, q in reads], 300))
    at = E.layout(300)
    assert a[at[2] + 101] == 2 and a[at[3] + 256] >= 2 and a[at[2] + 50] >= 1  # 'gcGC': two of four
