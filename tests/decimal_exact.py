"""The exact decimal -> binary32 reference (oracle/decimal_exact.py: rational arithmetic, no product code, no libc) and the
shared case lists of the numeric-limits tests: every decimal the device parsers must decide bit for bit (FLOAT_CASES), the
texts they must hand over (FLOAT_UNDECIDABLE), and the integer lists of POS / Integer INFO.  Built deterministically, no random
numbers: a failure names its text."""
from fractions import Fraction

from oracle.decimal_exact import bits_of_ratio, device_decides, f32, f32_bits, split_decimal  # noqa: F401  (re-exported)


def value_of_bits(b):
    """the rational a (positive, finite or one past the top) binary32 pattern stands for; 0x7F800000 reads as 2^128"""
    e, m = b >> 23, b & 0x7FFFFF
    if e == 0:
        return Fraction(m, 1 << 149)
    return Fraction((1 << 23) | m, 1 << 23) * Fraction(2) ** (e - 127)


def _digits_and_exp(x):
    """exact decimal expansion of a positive dyadic rational: (digit string without leading zeros, e) with x = 0.d1d2... * 10^e"""
    k = 0
    while x.denominator != 1:  # the denominator is a power of two: k multiplications by ten clear it
        x *= 10
        k += 1
    s = str(x.numerator)
    return s, len(s) - k


def _spell(s, e, plain):
    """the digits `s` with the decimal point behind the first e of them (e as returned by _digits_and_exp)"""
    if not plain:
        return f"{s[0]}.{s[1:]}e{e - 1}" if len(s) > 1 else f"{s}e{e - 1}"
    if e <= 0:
        return "0." + "0" * -e + s
    if e >= len(s):
        return s + "0" * (e - len(s))
    return s[:e] + "." + s[e:]


def tie_cases():
    """around the midpoint between a binary32 and the next one: its exact decimal cut to 17, 18 and 19 significant digits, and
    the cut +- 1 in its last place; exponent fields across the range (subnormals, the smallest and largest normals, both sides of
    2^24 and of 1), mantissa 0, all ones, odd and even last bits"""
    out = []
    for e in (0, 1, 2, 10, 30, 50, 64, 90, 100, 117, 126, 127, 128, 140, 149, 150, 151, 152, 170, 190, 220, 253, 254):
        for m in (0, 1, 2, 0x2AAAAB, 0x400000, 0x555554, 0x7FFFFE, 0x7FFFFF):
            b = (e << 23) | m
            if b == 0:
                continue
            mid = (value_of_bits(b) + value_of_bits(b + 1)) / 2
            s, de = _digits_and_exp(mid)
            for cut in (17, 18, 19):
                if len(s) < cut:
                    continue
                for d in (-1, 0, 1):
                    t = str(int(s[:cut]) + d)
                    if len(t) != cut:
                        continue
                    out.append(_spell(t, de, False))
                    if -12 <= de <= 30:  # also without an exponent (at most 40 characters)
                        out.append(_spell(t, de, True))
    # ties that fit in 19 digits exactly: round to even both ways
    out += ["16777217", "16777219", "33554434", "33554438", "8388607.5", "8388608.5", "0.500000029802322387", "1.00000005960464477",
            "1.000000059604644775", "1.000000059604644776", "1.000000178813934326", "4503599761588224", "9007199791611905"]
    return out


def window_tie_cases():
    """exact ties at every power of ten where one can exist: w * 10^q is halfway between two binary32 values iff its odd part
    has exactly 25 bits, so 5^|q| must fit in 25 bits beside an odd factor (q <= 10) and in 19 digits beside a 25-bit one
    (q >= -16): the window in which a decimal -> binary32 routine must look for ties and round them to even"""
    out = []
    for q in range(0, 12):
        p = 5 ** q
        ks = [k for k in range(1, 2 ** 25 // p + 2) if k & 1 and 2 ** 24 < p * k < 2 ** 25] if p < 2 ** 25 else []
        for k in ks[:2] + ks[-2:]:
            out += [f"{k}e{q}", f"{k * 8}e{q}", f"{k}{'0' * q}"[:39]]
    for q in range(1, 18):
        p = 5 ** q
        for odd in (2 ** 24 + 1, 2 ** 24 + 3, 0x1555555, 2 ** 25 - 3, 2 ** 25 - 1):
            w = odd * p
            if w < 10 ** 19:
                s = str(w).rjust(q + 1, "0")
                out += [f"{w}e-{q}", s[:-q] + "." + s[-q:]]
    return out


def digit_count_cases():
    """1 to 19 significant digits; leading zeros in front of the point, up to 40 zeros behind it, trailing zeros"""
    src = "9876543211234567898"
    out = []
    for n in range(1, 20):
        d = src[:n]
        out += [d, "000" + d, d + ".0", "0." + d, "0.000" + d, d[:1] + "." + d[1:] + ("0" if n < 19 else ""), d[:(n + 1) // 2] + "." + d[(n + 1) // 2:] + ("" if n > 1 else "0")]
        if n + 3 <= 19:
            out += [d + "000", d + ".000", "0." + d + "000"]
    for z in (1, 8, 9, 10, 11, 20, 39, 40):
        out += ["0." + "0" * z + "1", "0." + "0" * z + "1234567", "0." + "0" * z + src, "00.0" + "0" * (z - 1) + "5e" + str(z)]
    out += ["0000000000000000000000001", "0.0000000000000000000000000000000000000000", "000000000000000000000.5", "1000000000000000000", "1234567890123456789e-19"]
    return out


def border_cases():
    """significands on both sides of 2^24 (one exact division below it, Eisel-Lemire from it on), with 0, 10 and 11 fraction digits
    (the division's power of ten is exact up to 10^10)"""
    out = []
    for w in (2**24 - 1, 2**24, 2**24 + 1):
        s = str(w)
        out += [s, "0." + "0" * (10 - len(s)) + s, "0." + "0" * (11 - len(s)) + s, s + "e-10", s + "e-11", s[:2] + "." + s[2:]]
    return out


def exponent_cases():
    out = ["1e5", "1E5", "1e+5", "1E+5", "1e-5", "1E-5", "1e0005", "1e-0005", "1e+0000", "12.5e1", "12.5E-1", "0.0125e+3"]
    # the power of ten after the fraction digits are counted, on the table's borders (-65 .. 38)
    for q in (-66, -65, -64, 37, 38, 39):
        out += [f"1e{q}", f"3e{q}", f"9e{q}", f"1.5e{q + 1}", f"12.25e{q + 2}", f"1234567e{q}", f"1234567890123456789e{q}"]
    out += ["12345678901234567e-62", "1234567890123456789e-64", "9999999999999999999e-65", "1e-65", "0.1e-64", "34028235e31", "0.00034028235e42"]
    # the top: FLT_MAX, the largest decimals that still round to it, the first that round to inf
    out += ["3.4028235e38", "3.4028234e38", "3.40282346e38", "3.402823466e38", "3.4028235677973366e38", "3.402823567797336e38",
            "3.40282356779733661e38", "3.402823567797336616e38", "3.402823567797336617e38", "3.4028235677973367e38", "3.4028236e38",
            "340282356779733661600000000000000000000", "340282356779733661700000000000000000000",  # (20+ digits only by zeros: undecidable, filtered below)
            "1e39", "9e38", "1e99999999999", "1e100000", "1.5e100001", "123e4294967296"]
    # the bottom: FLT_MIN and its neighbours, the subnormals, the smallest one, half of it, below
    out += ["1.17549435e-38", "1.17549436e-38", "1.17549434e-38", "1.1754943e-38", "1.1754944e-38", "1.1754942e-38", "1.175494350822287508e-38",
            "1.175494280757364291e-38", "1.17549421e-38", "1.1754942107e-38", "5.877471754e-39"]
    for k in range(39, 46):
        out += [f"1e-{k}", f"2.5e-{k}", f"9.999e-{k}", f"123456789e-{k + 8}"]
    out += ["1.4e-45", "1.5e-45", "1.401298464e-45", "2.1e-45", "2.2e-45", "2.8e-45", "7.1e-46", "7.0e-46", "7.006492321624085354e-46",
            "7.006492321624085355e-46", "7.00649232162408536e-46", "7e-46", "1e-46", "1e-70", "1e-99999999999", "5e-100000", "0.001e-43"]
    out += ["0e999999", "0e-999999", "0.0e5", "-0e999999", "0E0"]
    return out


def sign_cases():
    return ["-0", "-0.0", "+0", "+1.5", "-1.5", "5.", ".5", "-.5e-3", "+.5", "-5.", "+0e0", "-1e-46", "-1e39", "+16777217", "-3.4028235e38",
            "5.e1", ".5e1", "+5.e-1"]


def float_cases():
    """every text the device must decide (each passes device_decides), without repeats, in a fixed order"""
    seen, out = set(), []
    for s in tie_cases() + window_tie_cases() + digit_count_cases() + border_cases() + exponent_cases() + sign_cases():
        if s not in seen and device_decides(s):
            seen.add(s)
            out.append(s)
    return out


# what the device must count as undecided.  ok: the host reader (Rust's grammar) takes it as a value.  scalar_only: in a list the
# text is not one item (`1,5` is two); "." and "" are the NULL spellings of a VCF value and are listed where they are not
FLOAT_UNDECIDABLE = [
    # (text, ok)
    ("+", False), ("-", False), ("e5", False), ("1e", False), ("1e+", False), ("1.2.3", False), ("0x1p3", False), (" 1", False), ("1 ", False),
    ("1_0", False), ("1f", False), ("..", False), ("1e5.5", False), ("--1", False), ("+-1", False), ("1e--5", False), ("١", False),
    ("inf", True), ("-Infinity", True), ("NaN", True), ("INF", True), ("+infinity", True), ("-nan", True), ("nan(1)", False), ("infinit", False),
    ("12345678901234567890", True), ("0.12345678901234567890", True), ("10000000000000000000000", True), ("1.0000000000000000000", True),
    ("340282356779733661700000000000000000000", True),
]
FLOAT_UNDECIDABLE_SCALAR_ONLY = [("1,5", False)]

# POS (VCF) and start / end (GFF): Rust's usize::from_str -- one optional '+', then digits; the device takes up to 18 digits
POS_CASES = ([("1" + "0" * (n - 1), 10 ** (n - 1)) for n in range(1, 19)] + [("9" * n, 10 ** n - 1) for n in range(1, 19)]
             + [("+" + "7" * n, int("7" * n)) for n in (1, 15, 16, 17, 18)] + [("0" * (18 - n) + "5" * n, int("5" * n)) for n in (1, 2, 15, 16, 17)]
             + [("+" + "0" * 16 + "1", 1), ("+00000000000000042", 42), ("123456789012345678", 123456789012345678), ("2147483648", 2**31), ("4294967296", 2**32)])
POS_ZERO = ["0", "+0", "00", "000000000000000000", "+00000000000000000"]  # NULL in VCF; an error in GFF (the host rejects it)
POS_UNDECIDABLE = ["1" + "0" * 18, "9" * 19, "9" * 20, "18446744073709551616", "0" * 18 + "1", "++1", "1+", "-1", "+", "", "1.0", " 1", "1 ", "1e3", "12x", "+-5",
                   "1234567890123456x", "x234567890123456", "12345678901234567x"]

# Integer INFO values (scalar 'i' and list items 'I'): [+-] digits, at most 10 of them, within int32
INT_CASES = [("-2147483648", -2**31), ("2147483647", 2**31 - 1), ("-2147483647", -2**31 + 1), ("-0", 0), ("+0", 0), ("0", 0), ("+7", 7), ("-7", -7),
             ("0000000012", 12), ("-0000000012", -12), ("+2147483647", 2**31 - 1), ("1000000000", 10**9), ("-1000000000", -10**9), ("999999999", 999999999),
             ("16777217", 16777217), ("-16777217", -16777217), ("1", 1), ("0000000000", 0)]
INT_UNDECIDABLE = ["2147483648", "-2147483649", "9999999999", "-9999999999", "4294967296", "4294967297", "12345678901", "00000000012", "-00000000012",
                   "-", "+", "--1", "1-", "1.0", "+-1", " 1", "1 ", "1e3", "0x10", "99999999999999999999"]
