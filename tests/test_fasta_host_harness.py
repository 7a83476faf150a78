"""CPU: what the GPU pipeline asks of the FASTA host reader (host/formats.h: first_byte, take_stream, data_offset; host/io.h:
BufReader::peek) in a stand-alone program built with -fsanitize=address,undefined (tests/fasta_host_harness.cpp): the look at the
first byte loses nothing, the stream handed over is the whole decompressed input, and the rows are fasta_expect's either way."""
import gzip
import os
import shutil
import subprocess

import pytest

import fasta_expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("fastah") / "fasta_host_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "exon_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "fasta_host_harness.cpp"), "-o", exe, "-lz", "-ldl", "-lpthread"], check=True)

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]  # (a sanitizer report ends the program with a status)
        return r.stdout
    return run


def escaped(s):
    return "\\N" if s is None else "".join(c if 0x21 <= ord(c) <= 0x7e and c != "\\" else "\\x%02X" % ord(c) for c in s)


def big_text():
    rows = [(b"r%d d %d" % (i, i) if i % 3 else b"r%d" % i, [bytes([65 + (i + j) % 26]) * ((i * 7 + j) % 90) for j in range(i % 6)]) for i in range(30000)]
    return fasta_expect.write_text(rows)


TEXTS = {"small": b">a d\nAC\nGT\n>b\n", "crlf, no final newline": b">a \t d \r\nA C\r\n\r\n>b\r\nGG", "leading text": b"x\n\n>a\nAC\n", "empty": b"",
         "two buffers": None}


@pytest.mark.parametrize("name", list(TEXTS))
@pytest.mark.parametrize("gz", [False, True])
def test_first_byte_loses_nothing_and_the_stream_is_the_whole_input(harness, tmp_path, name, gz):
    text = TEXTS[name] if TEXTS[name] is not None else big_text()  # (> 1 MiB: the reader's buffer is refilled)
    p = tmp_path / ("t.fasta.gz" if gz else "t.fasta")
    p.write_bytes(gzip.compress(text) if gz else text)
    want = fasta_expect.records(text)
    first = b"FIRST %d\n" % (text[0] if text else -1)
    for peek in (0, 1):
        out = harness("rows", p, 7, peek)
        if peek:
            assert out.startswith(first)
            out = out[len(first):]
        assert out.decode().split("\n")[:-1] == ["\t".join(escaped(c) for c in r) for r in want], (name, peek)
    out = harness("stream", p)
    head = first + b"OFFSET 0\nBYTES %d\n" % len(text)
    assert out[:len(head)] == head and out[len(head):] == text, name
