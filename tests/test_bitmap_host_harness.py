"""CPU: the bit appender of the staging layer (exon_amd/csrc/host/bitmap.h: append_bits, what exon_hip_stream_push appends every
batch's validity with) in a stand-alone program (tests/bitmap_host_harness.cpp) built with AddressSanitizer and
UndefinedBehaviorSanitizer, compared with np.packbits through the program's printed output.  Every source and destination block is
a heap allocation of its exact size, so a byte read or written too far is reported.  Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("bitmaph")
    exe = str(d / "bitmap_host_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "exon_amd", "csrc"),
                    os.path.join(ROOT, "tests", "bitmap_host_harness.cpp"), "-o", exe], check=True)

    def run(cases):
        """cases: [(start, [(n, src_off, source bools | None)])] -> asserts the program prints what numpy packs"""
        script, want = [], []
        for start, runs in cases:
            total = start + sum(n for n, _, _ in runs)
            bits = np.zeros(total, bool)
            script.append(f"case {start} {total}")
            pos = start
            for n, src_off, src in runs:
                if src is None:
                    bits[pos:pos + n] = True
                    hexed = "-"
                else:
                    assert len(src) == (src_off + n if n else 0)  # the block ends with the run's last bit's byte
                    bits[pos:pos + n] = src[src_off:src_off + n]
                    hexed = np.packbits(src, bitorder="little").tobytes().hex() or "."
                script.append(f"run {n} {src_off} {hexed}")
                pos += n
            script.append("end")
            want.append(np.packbits(bits, bitorder="little").tobytes().hex() or ".")
        p = d / "script.txt"
        p.write_text("\n".join(script) + "\n")
        r = subprocess.run([exe, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]  # (a sanitizer report ends the program with a status)
        got = r.stdout.decode().split("\n")[:-1]
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (i, cases[i][0], [(n, o, s is None) for n, o, s in cases[i][1]])

    return run


def _src(rng, n, src_off, p=0.5):
    return (rng.random(src_off + n) < p) if n else np.zeros(0, bool)


def test_every_residue_pair_and_every_short_length(harness):
    """one run into a destination that ends with it: (source bit offset mod 8) x (destination bit mod 8) x lengths 0 ... 200, the
    source's offset once below 8 and once some bytes in"""
    rng = np.random.default_rng(71)
    cases = []
    for s in range(8):
        for d in range(8):
            for n in range(201):
                src_off = s + 8 * int(rng.integers(0, 2) * rng.integers(0, 5))
                cases.append((d + 8 * int(rng.integers(0, 3)), [(n, src_off, _src(rng, n, src_off))]))
    harness(cases)


def test_all_valid_runs_at_every_destination_residue(harness):
    """src == nullptr: head bits up to the byte border, whole bytes, a tail -- alone, and between two runs that carry a source"""
    rng = np.random.default_rng(73)
    cases = []
    for d in range(8):
        for n in range(201):
            cases.append((d, [(n, 0, None)]))
            a, b = int(rng.integers(0, 30)), int(rng.integers(0, 30))
            sa, sb = int(rng.integers(0, 16)), int(rng.integers(0, 16))
            cases.append((d, [(a, sa, _src(rng, a, sa)), (n, 0, None), (b, sb, _src(rng, b, sb))]))
    harness(cases)


def test_long_runs_and_random_sequences(harness):
    """a few runs of 10^5 bits at every path (aligned copy, bit by bit, all valid) and sequences of short random runs, the way a
    slot's bitmap grows batch by batch"""
    rng = np.random.default_rng(79)
    cases = []
    for d, s in ((0, 0), (0, 8), (3, 0), (0, 5), (7, 7), (5, 2)):
        n = 100_000 + int(rng.integers(0, 9))
        so = s + 8 * int(rng.integers(0, 3))
        cases.append((d, [(n, so, _src(rng, n, so, p=0.9)), (n, 0, None), (7, 1, _src(rng, 7, 1))]))
        cases.append((d, [(n, 0, None)]))
    for _ in range(300):
        runs = []
        for _ in range(int(rng.integers(1, 12))):
            n = int(rng.choice([0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 61, 63, 64, 65, 127, 129, int(rng.integers(0, 2000))]))
            if rng.integers(0, 4) == 0:
                runs.append((n, 0, None))
            else:
                so = int(rng.integers(0, 70))
                runs.append((n, so, _src(rng, n, so, p=float(rng.choice([0.05, 0.5, 0.95])))))
        cases.append((int(rng.integers(0, 20)), runs))
    harness(cases)
