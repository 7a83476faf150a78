"""Decimal text -> the nearest binary32 (ties to even), in exact integer arithmetic (TEST INFRASTRUCTURE ONLY).

Shares no code with the product (host/decimal_f32.h) or with libc: the value is the rational `digits * 10^exp`, its binary
exponent is found by comparing integers, and the one division that rounds is an integer division whose remainder is compared
with half the divisor.  `np.float32(text)` is NOT this function: it rounds to a double first and the double to binary32, which
is wrong next to a binary32 tie ("1.000000059604644776" is above the midpoint of 0x3F800000 and 0x3F800001, its double is the
midpoint itself and rounds to even, 0x3F800000).

grammar (Rust's `f32::from_str`, what the reference parses QUAL and Float INFO values with):
    [+-] ( digits [. digits] | . digits | digits . ) [ (e|E) [+-] digits ]   |   [+-] ( inf | infinity | nan )   (any letter case)
"""
import re
import struct

_DECIMAL = re.compile(r"([+-]?)([0-9]*)(?:\.([0-9]*))?(?:[eE]([+-]?[0-9]+))?", re.ASCII)
_SPECIAL = {"inf": 0x7F800000, "infinity": 0x7F800000, "nan": 0x7FC00000}


def split_decimal(text):
    """-> (negative, digits as an integer, power of ten, number of significant digits) of a plain decimal, or None when the text
    is not one.  Leading zeros on either side of the point are not significant, trailing zeros are."""
    m = _DECIMAL.fullmatch(text)
    if not m:
        return None
    sign, ip, fp, ex = m.groups()
    fp = fp or ""
    if not ip and not fp:
        return None
    alld = ip + fp
    return sign == "-", int(alld), (int(ex) if ex else 0) - len(fp), len(alld.lstrip("0"))


def _round_ratio(num, den):
    """round(num / den) to an integer, ties to even"""
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and q & 1):
        q += 1
    return q


def bits_of_ratio(num, den):
    """bit pattern (sign excluded) of the binary32 nearest to the non-negative rational num / den"""
    if num == 0:
        return 0
    # e = floor(log2(num / den)), from the bit lengths and one comparison
    e = num.bit_length() - den.bit_length()
    if (num << -e if e < 0 else num) < (den << e if e > 0 else den):
        e -= 1
    e = max(e, -126)  # below 2^-126 the spacing stays 2^-149: subnormals
    # m = round(value / 2^(e - 23)): 2^23 <= m <= 2^24 for a normal value, below 2^23 for a subnormal one
    sh = e - 23
    m = _round_ratio(num << -sh, den) if sh < 0 else _round_ratio(num, den << sh)
    if m == 1 << 24:  # rounded up into the next binade
        m, e = 1 << 23, e + 1
    if e > 127:
        return 0x7F800000
    if m < 1 << 23:  # subnormal (or 0): exponent field 0
        return m
    return ((e + 127) << 23) | (m - (1 << 23))


def f32_bits(text):
    """bit pattern of Rust's `text.parse::<f32>()`; ValueError where that is an error"""
    d = split_decimal(text)
    if d is None:
        body = text[1:] if text[:1] in ("+", "-") else text
        if body.lower() in _SPECIAL and body.isascii():
            return _SPECIAL[body.lower()] | (0x80000000 if text[0] == "-" else 0)
        raise ValueError(f"invalid float literal {text!r}")
    neg, w, q, _ = d
    sign = 0x80000000 if neg else 0
    if w == 0:
        return sign
    # far outside binary32 whatever the digits say (keeps 10^q small: "1e99999999999")
    nd = len(str(w))
    if q + nd > 40:
        return sign | 0x7F800000
    if q + nd < -50:
        return sign
    return sign | (bits_of_ratio(w * 10**q, 1) if q >= 0 else bits_of_ratio(w, 10**-q))


def f32(text):
    """the binary32 nearest to the decimal `text`, as a python float (exactly that binary32's value)"""
    return struct.unpack("<f", struct.pack("<I", f32_bits(text)))[0]


def device_decides(text):
    """the grammar the device parsers claim to decide: a plain decimal (no inf / nan) with at most 19 significant digits"""
    d = split_decimal(text)
    return d is not None and d[3] <= 19
