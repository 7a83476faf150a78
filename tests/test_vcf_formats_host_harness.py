"""CPU: the per-item walk of the `formats` column (exon_amd/csrc/host/vcf_sample_walk.h -- what the k_fmt_* kernels of
text_columns.hip instantiate, a thread a sample) in a stand-alone program (tests/vcf_formats_host_harness.cpp) built with
AddressSanitizer and UndefinedBehaviorSanitizer: measured, then filled into a buffer of exactly the measured size with guard bytes
behind it, next to exon::vcf_formats_string (host/vcf_text.h, the authority) on the same input, both against
oracle/decode.py: formats_string.  Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import vcf_formats_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("fmth")
    exe = str(d / "vcf_formats_host_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "exon_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "vcf_formats_host_harness.cpp"), "-o", exe, "-lz", "-ldl", "-lpthread"], check=True)

    def run(rows):
        """rows: (FORMAT or None, samples) -> [(walk string | None, host string | None)] and the oracle's column; len / guard asserted here"""
        inp = d / "rows.txt"
        with open(inp, "w", newline="") as f:
            f.write(",".join(f"{k}={t}" for k, t in K.FORMAT_TYPES.items()) + "\n")
            f.writelines(K.tail(fmt, samples) + "\n" for fmt, samples in rows)
        r = subprocess.run([exe, str(inp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]  # (a sanitizer report ends the program with a status)
        out = r.stdout.decode().split("\n")[:-1]
        assert len(out) == 4 * len(rows)
        got = []
        for i in range(len(rows)):
            walk, host, ln, guard = out[4 * i:4 * i + 4]
            assert ln == "len=1" and guard == "guard=1", (i, rows[i], ln, guard)
            got.append((None if walk == "UNDECIDED" else walk, None if host == "ERROR" else host))
        return got, K.oracle_formats(K.write_vcf(d / "rows.vcf", rows))

    return run


def check(rows, got, want, oracle_differs=()):
    """-> the rows the walk hands over though the host prints them"""
    over = 0
    for row, (walk, host), orc in zip(rows, got, want):
        if row not in oracle_differs:
            assert host == orc, (row, host, orc)
        if walk is not None:
            assert walk == host, (row, walk, host)
        over += walk is None and host is not None
    return over


def test_the_spelled_out_rows_and_the_rows_the_reference_cannot_print(harness):
    rows = [(f, s) for f, s, _ in K.SPELLED] + K.ERRORS
    got, want = harness(rows)
    assert check(rows, got, want) == 0
    assert [w for w, _ in got[:5]] == [t for _, _, t in K.SPELLED] == want[:5]
    assert got[5:] == [(None, None), (None, None)]


def test_the_walk_at_its_limits(harness):
    """Genotypes of 1 - 4 alleles with leading zeros and 12-digit alleles, exactly 16 and 17 keys, more values than keys and fewer,
    an empty key, FORMAT '.', '' and absent."""
    got, want = harness(K.LIMITS)
    by = {(f, tuple(s)): g for (f, s), g in zip(K.LIMITS, got)}
    over = check(K.LIMITS, got, want)
    assert over == 1 and by[(":".join(K.KEYS16 + ["XT"]), (":".join(K.VALS16 + ["z"]),))][0] is None  # 17 keys: handed over, the host prints it
    assert by[("GT", ("1/02|3/004",))][0] == "GT\t1/2/3|4"
    assert by[("GT", ("000000000012/123456789012",))][0] == "GT\t12/123456789012"
    assert by[("GT", ("123456789012|000000000000|1|.",))][0] == "GT\t123456789012|0|1|."
    assert by[("GT", ("0|1/2", "0/1|2", "0|1|2|3"))][0] == "GT\t0/1|2\t0/1/2\t0|1|2|3"
    assert by[(":".join(K.KEYS16), (":".join(K.VALS16), ":".join(K.VALS16[:5])))][0] == ":".join(K.KEYS16) + "\t0|1:0.5:7:t:5:0.00001,.:q:a:b:c:d:e:f:g:h:0\t0|1:0.5:7:t:5"
    assert by[("GT:XQ", ("0/1:0.5:extra:values", "1|1:1.0:9"))][0] == "GT:XQ\t0/1:0.5\t1|1:1"
    assert by[("GT:XQ:XP:XT", ("0/1", "0/1:0.5", "1/1:2:3"))][0] == "GT:XQ:XP:XT\t0/1\t0/1:0.5\t1/1:2:3"
    assert by[("GT::DP", ("0/1:x:07", "1/1:y:+3"))][0] == "GT::DP\t0/1:x:7\t1/1:y:3"
    assert by[(".", ("0/1", "anything:at:all"))][0] == by[(".", ())][0] == by[(None, ())][0] == by[("", ("0/1",))][0] == "\t"
    assert by[("XQ", ("inf", "-inf", "nan", "1e38", "3.4028235e38", "0.1234567", "1e-45"))][0] == (
        "XQ\tinf\t-inf\tNaN\t100000000000000000000000000000000000000\t340282350000000000000000000000000000000\t0.1234567\t0.000000000000000000000000000000000000000000001")


def test_rows_the_walk_hands_over(harness):
    """Every row the host raises on is undecided; so are those the device cannot decide though the host prints them."""
    got, want = harness(K.HANDED_OVER)
    # a line that has FORMAT and ends there: the host reader raises on its empty sample (vcf_formats_string walks one sample of no
    # bytes), the oracle's zip over no samples prints "GT\t"; the host reader is what a scan serves, and the walk hands the row to it
    check(K.HANDED_OVER, got, want, oracle_differs=[("GT", [])])
    assert want[K.HANDED_OVER.index(("GT", []))] == "GT\t"
    assert all(w is None for w, _ in got)
    assert [h is None for _, h in got] == [True] * 8 + [True, True, True, False, True]


def test_fuzz_against_the_host_function_and_the_oracle(harness):
    """5 000 rows of the host fuzz generator with 0 - 40 samples: no key list beyond 16, no byte >= 0x80, so the walk decides every one."""
    rows = [(f, s) for _, f, s in K.fuzz_rows(5000, 29, 40)]
    got, want = harness(rows)
    assert check(rows, got, want) == 0
    assert all(w is not None for w, _ in got) and max(len(s) for _, s in rows) == 40
