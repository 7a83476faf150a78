"""CPU: the aligned-blocks rule (exon_amd/csrc/host/cigar_blocks.h: walk_blocks, what both device passes and
exon_hip_cigar_blocks_host call) in a stand-alone program (tests/cigar_blocks_host_harness.cpp) built with AddressSanitizer and
UndefinedBehaviorSanitizer, compared with cigar_blocks_expect.py through the program's printed output.  The ops and the outputs are
heap blocks of exactly their size -- 0, 1 and 65 535 ops, an output of exactly k and of exactly k - 1 entries -- so an element read
or written too far is reported.  Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cigar_blocks_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("cigarh")
    exe = str(d / "cigar_blocks_host_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "exon_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cigar_blocks_host_harness.cpp"), "-o", exe], check=True)

    def run(cases):
        """cases: [(ops, start, mask)] -> asserts the program prints the expected blocks of each"""
        p = d / "script.txt"
        p.write_text("".join(f"{start} {mask} {len(ops)} {' '.join(str(int(v)) for v in E.encode(ops))}\n" for ops, start, mask in cases))
        r = subprocess.run([exe, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]  # (a sanitizer report ends the program with a status)
        got = r.stdout.decode().split("\n")[:-1]
        assert len(got) == len(cases)
        for line, (ops, start, mask) in zip(got, cases):
            want = E.blocks(ops, start, mask)
            assert [int(x) for x in line.split()] == [len(want)] + [v for b in want for v in b], (ops[:8], len(ops), start, hex(mask))

    run.exe, run.dir = exe, d
    return run


def test_sam_cigar_texts_accepted_and_refused(harness):
    """DECISION (b): an op longer than 2^28 - 1, an op without a count, a count without an op, a letter outside MIDNSHP=X and the empty
    text are refused; '*' and leading zeros are not"""
    good = ["*", "1M", "10M5I10M", "268435455M", "0M", "007S3M", "1M1I1D1N1S1H1P1=1X"]
    bad = ["", "M", "10", "10M5", "10M5Q", "268435456M", "99999999999M", "1m", "1M*", "**", "-1M", "1 M", "4294967297M"]
    p = harness.dir / "texts.txt"
    p.write_text("".join(t + "\n" for t in good + bad))
    r = subprocess.run([harness.exe, "text", str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert r.stdout.decode().split() == ["1"] * len(good) + ["0"] * len(bad)


def test_no_op_one_op_and_the_most_a_bam_record_holds(harness):
    cases = []
    for mask in (E.ALIGNED, E.ALIGNED_DEL, E.LEGAL, 1 << 3):
        cases.append(([], 5, mask))                                          # 0 ops: 0 blocks, outputs of 0 bytes
        for code in range(16):
            cases += [([(7, code)], 5, mask), ([(0, code)], 5, mask)]        # 1 op: k = 1 (then k - 1 = 0 entries) or k = 0
        cases.append(([(1, 0), (1, 3)] * 32767 + [(1, 0)], 1, mask))         # 65 535 ops, one-base blocks: k = 32 768 under ALIGNED
        cases.append(([((1 << 28) - 1, 0)] * 65535, 2**31 - 1, mask))        # 65 535 longest ops from the largest BAM position
        cases.append(([(3, 4)] * 65535, 1, mask))                            # 65 535 ops that cover nothing
    harness(cases)


def test_random_cigars_under_every_legal_mask(harness):
    rng = np.random.default_rng(31)
    cases = []
    for i in range(400):
        k = int(rng.integers(0, 40))
        ops = [(int(ln), int(c)) for ln, c in zip(rng.choice([0, 1, 2, 3, 50, (1 << 28) - 1], k), rng.integers(0, 16, k))]
        start = int(rng.choice([1, -5, 0, 2**31 - 1, -2**63, 2**63 - 1 - 40 * (1 << 28)]))
        for mask in E.LEGAL_MASKS:
            cases.append((ops, start, mask))
    harness(cases)
