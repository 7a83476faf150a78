"""Rows for the tests of the `formats` Utf8 column (tests/test_vcf_formats_host_harness.py, tests/test_gpu_vcf_formats_text.py): the
spelled-out rows and the fuzz generator of tests/test_scan_projection.py (restated with the number of samples as a parameter), the
rows at the column's limits, and the oracle's column of a file."""
import numpy as np

from oracle import decode
from test_scan_projection import TEXT_HEAD

HEAD = TEXT_HEAD
# the ##FORMAT lines of HEAD as exon_hip_vcf_parser_set_format_key_types takes them (GT is typed String there: it is known by name)
FORMAT_TYPES = {"GT": "s", "XQ": "f", "XP": "i", "XT": "s"}

# (FORMAT or None, samples) of test_host_vcf_info_and_formats_text_are_printed_again_not_copied, and the exact strings
SPELLED = [("GT:XQ:XP:XT", ["0|1:0.250:0,03,26:x,y", "1/2:1e2:1,.,3:z"], "GT:XQ:XP:XT\t0|1:0.25:0,3,26:x,y\t1/2:100:1,.,3:z"),
           ("GT", ["0/1/2", "0|1|2"], "GT\t0/1/2\t0|1|2"),
           ("GT:XQ", ["0|1/2:7", ".|1:0.1234567"], "GT:XQ\t0/1|2:7\t.|1:0.1234567"),
           ("XP", ["1", "2"], "XP\t1\t2"),
           (None, [], "\t")]
# the two `formats` rows of test_host_vcf_text_columns_report_what_the_reference_cannot_print
ERRORS = [("GT:XQ", ["0/1:.", "0/1:."]), ("GT", ["0/x", "0/x"])]

KEYS16 = ["GT", "XQ", "XP", "XT", "DP", "GL", "FT", "K8", "K9", "KA", "KB", "KC", "KD", "KE", "KF", "XP"]
VALS16 = ["0|1", "0.50", "007", "t", "+5", "1e-5,.", "q", "a", "b", "c", "d", "e", "f", "g", "h", "-0"]
# (FORMAT or None, samples): what the fuzz does not reach.  The walk may hand over rows the host prints (17 keys).
LIMITS = [
    ("GT", ["0"]), ("GT", ["007"]), ("GT", ["00/01"]), ("GT", ["0|00|1"]), ("GT", ["1/02|3/004"]), ("GT", ["000000000012/123456789012"]),
    ("GT", ["123456789012|000000000000|1|."]), ("GT", ["./."]), ("GT", [".|.|."]), ("GT", ["0|1/2", "0/1|2", "0|1|2|3"]),
    (":".join(KEYS16), [":".join(VALS16), ":".join(VALS16[:5])]),
    (":".join(KEYS16 + ["XT"]), [":".join(VALS16 + ["z"])]),
    ("GT:XQ", ["0/1:0.5:extra:values", "1|1:1.0:9"]), ("GT:XQ:XP:XT", ["0/1", "0/1:0.5", "1/1:2:3"]),
    ("GT::DP", ["0/1:x:07", "1/1:y:+3"]), (".", ["0/1", "anything:at:all"]), (".", []), (None, []), ("", ["0/1"]),
    ("XT", ["a,b,.", ".,."]), ("XQ", ["inf", "-inf", "nan", "1e38", "3.4028235e38", "0.1234567", "1e-45"]),
    ("XP", ["2147483647", "-2147483648", "-0", "+0", "1,.,-3"]), ("GL:DP:FT", ["-0.5,.,1e3:010:PASS", "0,0,0:0:q10;s50"]),
    ("GT:XQ", ["0/1:1.50", "1/1:0.10"]), ("XT:GT", ["a:0/1", "b:1|0"]),
]
# rows the device hands over: the host raises on the first five kinds, prints the others
HANDED_OVER = [("GT:XQ", ["0/1:."]), ("GT:XQ", ["0/1:"]), ("GT", ["0/x"]), ("GT", ["0//1"]), ("GT", ["/1"]), ("GT", ["1|"]), ("GT", [""]), ("GT", []),
               ("XP", ["2147483648"]), ("XP", ["1x"]), ("XP", ["-"]), ("XQ", ["0.12345678901234567890123"]), ("GT:XQ", ["0/1:0.5", "."])]


def tail(fmt, samples):
    """what follows the INFO field of the data line: "" without a FORMAT field"""
    return "" if fmt is None else "\t" + "\t".join([fmt] + list(samples))


def data_line(i, fmt, samples, info=".", chrom="1"):
    return "\t".join([chrom, str(i + 1), ".", "A", "C", ".", ".", info]) + tail(fmt, samples)


def fuzz_rows(n, seed, max_samples):
    """The generator of test_host_vcf_text_columns_fuzz_against_the_oracle with 0 .. max_samples samples a record:
    -> [(info, FORMAT or None, samples)].  No key list beyond 16, no byte >= 0x80, no missing value."""
    rng = np.random.default_rng(seed)
    ints = ["0", "7", "007", "+5", "-3", "2147483647", "-2147483648", "10"]
    floats = ["0.5", "0.50", "1e-5", "1E3", "1.0", "-0", "0.1234567", "16777217", "3.4028235e38", "1e-45", "123456.789", ".5", "5.", "inf", "-inf", "nan"]
    strs = ["a", "x_y", "1.50", "007", "a|b", "Hello"]

    def val(kind):
        if kind == "i":
            return str(rng.choice(ints))
        if kind == "f":
            return str(rng.choice(floats))
        if kind == "I":
            return ",".join(str(rng.choice(ints + ["."])) for _ in range(rng.integers(1, 4))) if rng.random() < 0.9 else "5"
        if kind == "F":
            return ",".join(str(rng.choice(floats + ["."])) for _ in range(rng.integers(1, 4)))
        if kind == "c":
            return str(rng.choice(list("ACGTq")))
        if kind == "C":
            return ",".join(str(rng.choice(list("ACG."))) for _ in range(rng.integers(2, 4)))
        return ",".join(str(rng.choice(strs + ["."])) for _ in range(rng.integers(1, 3)))

    def gt():
        t = str(rng.choice(["0", "1", "2", "."]))
        for _ in range(int(rng.integers(1, 4)) - 1):
            t += str(rng.choice(["/", "|"])) + str(rng.choice(["0", "1", "02", "."]))
        return t if t != "." else "0"

    info_keys = {"XF": "f", "XL": "F", "XI": "i", "XJ": "I", "XB": "b", "XC": "c", "XD": "C", "XS": "s", "AF": "F", "DP": "i", "DB": "b", "ZZ": "s", "MQ": "f"}
    fmt_keys = {"XQ": "f", "XP": "I", "XT": "s", "DP": "i", "GL": "F", "FT": "s"}
    rows = []
    for _ in range(n):
        ks = [k for k in info_keys if rng.random() < 0.35]
        info = ";".join(k if info_keys[k] == "b" else f"{k}={val(info_keys[k])}" for k in ks) or "."
        info = ";".join(e for e in info.split(";") if not e.endswith("=.")) or "."
        fmt, samples = None, []
        ns = int(rng.integers(0, max_samples + 1))
        if ns:
            fk = ["GT"] * (rng.random() < 0.7) + [k for k in fmt_keys if rng.random() < 0.4]
            if fk:
                fmt = ":".join(fk)
                for _ in range(ns):
                    vals = [gt() if k == "GT" else val(fmt_keys[k]) for k in fk]
                    samples.append(":".join(v if v != "." else "1" for v in vals))
        rows.append((info, fmt, samples))
    return rows


def write_vcf(path, rows, eol="\n", chrom=None):
    """rows: (FORMAT or None, samples) or (info, FORMAT or None, samples); chrom: a function of the row's index"""
    with open(path, "w", newline="") as f:
        f.write(HEAD.replace("\n", eol))
        for i, r in enumerate(rows):
            info, fmt, samples = r if len(r) == 3 else (".",) + tuple(r)
            f.write(data_line(i, fmt, samples, info, chrom(i) if chrom else "1") + eol)
    return str(path)


def oracle_formats(path):
    """the column by oracle/decode.py: a string a record, None where the reference cannot print it"""
    v = decode.decode_vcf(str(path))
    out = []
    for i in range(len(v["chrom"])):
        try:
            out.append(decode.formats_string(v, i))
        except ValueError:
            out.append(None)
    return out
