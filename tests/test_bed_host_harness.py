"""CPU: exon_amd/csrc/host/bed.h in a stand-alone program (tests/bed_host_harness.cpp) built with AddressSanitizer and
UndefinedBehaviorSanitizer: every rule case on a heap copy of exactly its bytes, and 60 000 generated rows through BEDBatchReader
with one thread and with the slab-parallel reader, compared with tests/bed_expect.py through the program's printed output.
Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import bed_expect
from test_bed_scan import RULES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("bedh") / "bed_host_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "exon_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "bed_host_harness.cpp"), "-o", exe, "-lz", "-ldl", "-lpthread"], check=True)

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]  # (a sanitizer report ends the program with a status)
        return r.stdout.split(b"\n")[:-1]

    return run


def printed(rec):
    chrom, start, end, name, score, strand = rec
    return b"\t".join([chrom, b"%d" % start, b"%d" % end, b"\\N" if name is None else name, b"\\N" if score is None else b"%d" % score,
                       b"\\N" if strand is None else bed_expect.STRANDS[strand].encode()])


def test_every_rule_case(harness, tmp_path):
    p = tmp_path / "rules.txt"
    p.write_bytes(b"".join(line + b"\n" for line, _ in RULES))
    out = harness("lines", p)
    assert len(out) == len(RULES)
    for (line, want), got in zip(RULES, out):
        if want is None:
            assert got.startswith(b"ERROR BED line '"), (line, got)
        else:
            assert got == printed(want), line


@pytest.mark.parametrize("threads", [1, 4])
def test_60000_generated_rows(harness, tmp_path, threads):
    p = tmp_path / "gen.bed"
    subprocess.check_call([GEN, "bed", "60000", str(p), "mix"])
    text = open(p, "rb").read()
    big = tmp_path / "big.bed"  # three copies: past the 8 MiB at which the reader parses slabs in parallel
    big.write_bytes(text * 3)
    assert os.path.getsize(big) >= 8 << 20
    want = [printed(r) for r in bed_expect.records(text)]
    assert len(want) == 60000
    assert harness("scan", big, threads, 8192) == want * 3
    assert harness("scan", p, threads, 7) == want
    # a CRLF file whose last line has no terminator, and an error in the last line: rows up to it, then the error
    crlf = tmp_path / "crlf.bed"
    crlf.write_bytes(text.replace(b"\n", b"\r\n") + b"chrY\t1\t2")
    assert harness("scan", crlf, threads, 8192) == want + [b"chrY\t1\t2\t\\N\t\\N\t\\N"]
    bad = tmp_path / "bad.bed"
    bad.write_bytes(text * 3 + b"chrY\t1\t2\tn\t65536")
    out = harness("scan", bad, threads, 1 << 20)
    assert out[-1].startswith(b"ERROR BED line 'chrY\t1\t2\tn\t65536': invalid score")
