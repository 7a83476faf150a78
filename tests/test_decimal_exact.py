"""CPU: the exact decimal -> binary32 reference of the numeric-limits tests (tests/decimal_exact.py), glibc's strtof and the host
VCF reader agree bit for bit on every decimal the device parsers are asked to decide (tests/test_gpu_numeric_limits.py); the
texts the device hands over get the host reader's value or its error; oracle/decode.py rounds a Float field to the nearest
binary32, not through a double."""
import ctypes
import struct

import numpy as np
import pytest

import decimal_exact as dx
import exon_amd
from oracle import decode

HEAD = ('##fileformat=VCFv4.3\n##contig=<ID=1>\n##INFO=<ID=AF,Number=1,Type=Float,Description="x">\n'
        '##INFO=<ID=MQS,Number=.,Type=Float,Description="x">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n')
CASES = dx.float_cases()


def strtof_bits(texts):
    libc = ctypes.CDLL(None)
    libc.strtof.restype = ctypes.c_float
    libc.strtof.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    return np.array([libc.strtof(t.encode(), None) for t in texts], np.float32).view(np.uint32)


def host_columns(path, info_field="AF"):
    s = exon_amd.Scan(str(path), "vcf", info_field=info_field, gpu_parse=False)
    qual, info = [], []
    for b in s:
        qual += b.field(2).to_pylist()
        info += b.field(4).to_pylist()
    s.close()
    return qual, info


def bits_of(values):
    return np.array(values, np.float32).view(np.uint32)


@pytest.mark.parametrize("text,bits", [
    ("1.000000059604644776", 0x3F800001), ("1.000000059604644775", 0x3F800000), ("1.000000178813934326", 0x3F800001), ("1.000000178813934327", 0x3F800002), ("16777217", 0x4B800000),
    ("16777219", 0x4B800002), ("8388607.5", 0x4AFFFFFF), ("8388608.5", 0x4B000000), ("8388609.5", 0x4B000002), ("0.1", 0x3DCCCCCD), ("3.4028235e38", 0x7F7FFFFF), ("3.4028235677973366e38", 0x7F7FFFFF),
    ("3.4028235677973367e38", 0x7F800000), ("1e39", 0x7F800000), ("1.17549435e-38", 0x00800000), ("1.1754942e-38", 0x007FFFFF), ("1.4e-45", 1),
    ("7.1e-46", 1), ("7.0e-46", 0), ("7.006492321624085354e-46", 0), ("7.006492321624085355e-46", 1), ("1e-70", 0), ("-0", 0x80000000),
    ("-.5e-3", 0xBA03126F), ("0e999999", 0), ("1e99999999999", 0x7F800000), ("-inf", 0xFF800000), ("NaN", 0x7FC00000), ("5.", 0x40A00000)])
def test_the_exact_reference_on_known_bit_patterns(text, bits):
    """patterns from the binary32 format itself: 1 + 2^-24 is the tie above 1.0 (...4775 is below it with 19 digits, ...4776 above; 1 + 3 * 2^-24 = ...934326171875 likewise);
    2^24 + 1 and 2^24 + 3 are ties (to even: down, up); FLT_MAX + half an ulp = 3.40282356779733661637...e38 goes to inf;
    2^-150 = 7.00649232162408535461...e-46 is the tie between 0 and the smallest subnormal (to even: 0)"""
    assert dx.f32_bits(text) == bits


def test_the_grammar_predicate():
    assert all(dx.device_decides(t) for t in ["0", "5.", ".5", "-.5e-3", "+0e0", "1234567890123456789", "0.0001234567890123456789", "1e0005"])
    for t, _ in dx.FLOAT_UNDECIDABLE + dx.FLOAT_UNDECIDABLE_SCALAR_ONLY:
        assert not dx.device_decides(t), t
    assert not dx.device_decides("") and not dx.device_decides(".")
    assert len(CASES) > 2000 and len(set(CASES)) == len(CASES)


def test_exact_reference_strtof_and_host_reader_agree_on_every_decidable_case(tmp_path):
    """Two references that share nothing must agree before the device is asked; the host reader (Clinger's fast path + strtof in
    host/formats.h) is the third.  QUAL carries case i, AF case n - 1 - i."""
    want = np.array([dx.f32_bits(t) for t in CASES], np.uint32)
    libc = strtof_bits(CASES)
    diff = np.flatnonzero(want != libc)
    assert diff.size == 0, [(CASES[i], hex(want[i]), hex(libc[i])) for i in diff[:10]]
    p = tmp_path / "cases.vcf"
    n = len(CASES)
    p.write_text(HEAD + "".join(f"1\t{i + 1}\t.\tA\tC\t{t}\tPASS\tAF={CASES[n - 1 - i]}\n" for i, t in enumerate(CASES)))
    qual, info = host_columns(p)
    assert None not in qual and None not in info and len(qual) == n
    for got, name in ((bits_of(qual), "QUAL"), (bits_of(info)[::-1], "AF")):
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, (name, [(CASES[i], hex(want[i]), hex(got[i])) for i in diff[:10]])


@pytest.mark.parametrize("text,ok", dx.FLOAT_UNDECIDABLE + dx.FLOAT_UNDECIDABLE_SCALAR_ONLY)
def test_what_the_device_hands_over_has_a_host_answer(tmp_path, text, ok):
    """the case list's `ok` column against the host reader: a value (the exact reference's; NaN by being NaN) or its error"""
    p = tmp_path / "t.vcf"
    p.write_bytes((HEAD + f"1\t5\t.\tA\tC\t{text}\tPASS\tAF={text}\n").encode())
    if not ok:
        with pytest.raises(exon_amd.ExonHipError, match="float"):
            host_columns(p)
        with pytest.raises(ValueError):
            dx.f32_bits(text)
        return
    qual, info = host_columns(p)
    want = dx.f32_bits(text)
    for got in (bits_of(qual)[0], bits_of(info)[0]):
        assert (np.isnan(np.uint32(want).view(np.float32)) and np.isnan(np.uint32(got).view(np.float32))) or got == want


def test_oracle_decoder_rounds_to_the_nearest_binary32(tmp_path):
    """1.000000059604644776 lies above the midpoint of 0x3F800000 and 0x3F800001; as a double it IS the midpoint, which then
    rounds to even: np.float32(text) gives 0x3F800000.  QUAL, a scalar Float and a Float list item of the oracle's decoder."""
    t = "1.000000059604644776"
    assert struct.unpack("<I", struct.pack("<f", np.float32(t)))[0] == 0x3F800000, "numpy no longer rounds through a double: the note above is stale"
    p = tmp_path / "t.vcf"
    p.write_text(HEAD + f"1\t5\t.\tA\tC\t{t}\tPASS\tAF={t};MQS=0.5,{t}\n")
    v = decode.decode_vcf(str(p))
    assert bits_of([v["qual"][0]])[0] == 0x3F800001
    assert bits_of(decode.typed_info(v, "AF")[1])[0] == 0x3F800001
    assert bits_of(decode.typed_info(v, "MQS")[1][0]).tolist() == [0x3F000000, 0x3F800001]
    assert decode.info_string(v, 0) == "AF=1.0000001;MQS=0.5,1.0000001"
    qual, info = host_columns(p)
    assert bits_of(qual)[0] == 0x3F800001 and bits_of(info)[0] == 0x3F800001
