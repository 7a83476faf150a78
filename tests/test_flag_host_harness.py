"""CPU: the flag / mapping-quality filter of the BAM and SAM host readers (exon_amd/csrc/host/formats.h: bam_flag_hit, sam_flag_hit
and the two readers' record loops) in a stand-alone program (tests/flag_host_harness.cpp) built with AddressSanitizer and
UndefinedBehaviorSanitizer, compared with tests/flag_predicate_expect.py through the program's printed output.  Nothing sanitized
is loaded into Python."""
import os
import shutil
import struct
import subprocess

import pytest

import flag_predicate_expect as E
from test_flag_predicate import FLAGS, MAPQ_MINS, MAPQS, PAIRS, mixed, write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("flagh") / "flag_host_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "exon_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "flag_host_harness.cpp"), "-o", exe, "-lz", "-ldl", "-lpthread"], check=True)

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]  # (a sanitizer report ends the program with a status)
        return r.stdout.decode().split("\n")[:-1]

    return run


# FLAG / MAPQ texts that are no number for the device parser let the record through: (flag text, mapq text)
MALFORMED = [("", "0"), ("4x", "0"), ("x", "0"), ("-4", "0"), ("+4", "0"), ("65536", "0"), ("4294967300", "0"), ("99999999999999999999", "0"), ("4", ""), ("4", "q"),
             ("4", "256"), ("4", "-1"), ("4", "3 "), (" 4", "3"), ("4", "1e1")]


def test_the_two_fields_of_a_sam_line(harness, tmp_path):
    pairs = [(str(f), str(q)) for f in FLAGS for q in MAPQS] + [("0004", "030"), ("65535", "255"), ("0", "0")]
    p = tmp_path / "fields.txt"
    p.write_text("".join(f"{f}\t{q}\n" for f, q in pairs + MALFORMED))
    for mask, value in PAIRS:
        for mapq_min in MAPQ_MINS:
            want = ["1" if E.passes(int(f), int(q), mask, value, mapq_min) else "0" for f, q in pairs] + ["1"] * len(MALFORMED)
            assert harness("fields", p, mask, value, mapq_min) == want, (mask, value, mapq_min)


def test_the_fixed_fields_of_a_bam_record(harness, tmp_path):
    pairs = [(f, q) for f in FLAGS for q in MAPQS]
    p = tmp_path / "fixed.bin"
    p.write_bytes(b"".join(struct.pack("<iiBBHHHiiii", 0, 0, 1, q, 4680, 0, f, 0, -1, -1, 0) for f, q in pairs))
    for mask, value in PAIRS:
        for mapq_min in MAPQ_MINS:
            want = ["1" if E.passes(f, q, mask, value, mapq_min) else "0" for f, q in pairs]
            assert harness("fixed", p, mask, value, mapq_min) == want, (mask, value, mapq_min)


@pytest.mark.parametrize("fmt", ["bam", "sam", "sam.gz", "sam.bgz"])
def test_the_readers_with_the_predicate_in_their_config(harness, tmp_path, fmt):
    recs = mixed(2000, seed=13)
    path = write(tmp_path, "h", recs, fmt)

    def printed(kept):
        null = "\\N"
        return ["\t".join([str(recs[i]["flag"]), null if recs[i]["mapq"] == 255 else str(recs[i]["mapq"]), null if recs[i]["name"] == "*" else recs[i]["name"],
                           str(len(recs[i]["qual"]))]) for i in kept]

    for batch_size in (1, 8192):
        for where in ((4, 0, -1), (1284, 0, 30), (4, 5, -1), (0, 0, 256)):
            assert harness("scan", fmt[:3], path, batch_size, *where) == printed(E.keep(recs, *where))
    both = E.keep(recs, 1284, 0, 30, region=("r1", 1000, 4000))
    assert both and harness("scan", fmt[:3], path, 8192, 1284, 0, 30, "r1:1000-4000") == printed(both)
    if fmt == "sam":  # a line that ends before its MAPQ field: the builder's error behind the rows before it
        lines = open(path).read().split("\n")
        cut = next(i for i, ln in enumerate(lines) if not ln.startswith("@")) + 100
        lines[cut] = "\t".join(lines[cut].split("\t")[:4])
        bad = tmp_path / "short.sam"
        bad.write_text("\n".join(lines))
        out = harness("scan", "sam", bad, 64, 4, 0, -1)
        before = E.keep(recs[:100], 4, 0)  # whole batches of 64 kept rows come out, the batch with the line does not
        assert len(before) > 64 and out == printed(before[:64]) + ["ERROR SAM record has fewer than 6 fields"]
