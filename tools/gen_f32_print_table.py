#!/usr/bin/env python3
"""Regenerates kPow10G of exon_amd/csrc/host/f32_print.h with exact integers.

For k in [-31, 45]: 10^k = beta * 2^r with 2^63 <= beta < 2^64, r = floor(log2(10^k)) - 63; the table holds g = ceil(beta)
(R. Giulietti, "The Schubfach way to render doubles", section 9.8).  The script also checks the two fixed-point logarithms the
header uses over the ranges it uses them in.

    python3 tools/gen_f32_print_table.py          # prints the table's lines
"""
import math

K_MIN, K_MAX = -31, 45


def floor_log2_pow10(k):
    p = 10 ** abs(k)
    if k >= 0:
        return p.bit_length() - 1
    # 10^k = 1 / p, p no power of two for k < 0: 2^(bl-1) < p < 2^bl
    return -p.bit_length()


def g_of(k):
    r = floor_log2_pow10(k) - 63
    if k >= 0:
        p = 10 ** k
        return ((p + (1 << r) - 1) >> r) if r >= 0 else (p << -r)
    p = 10 ** -k
    return -((-(1 << -r)) // p)  # ceil(2^-r / p)


def main():
    for k in range(K_MIN, K_MAX + 1):
        g = g_of(k)
        assert 1 << 63 <= g < 1 << 64
        assert (k * 1741647) >> 19 == floor_log2_pow10(k), k  # floor(log2(10^k)) as the header computes it
        print("    0x%016xULL,  // %d" % (g, k))
    for q in range(-149, 105):  # every binary exponent of a binary32
        assert (q * 1262611) >> 22 == math.floor(q * math.log10(2)), q  # floor(log10(2^q))
        exact = (3 ** 1) * (2 ** (q + 149))  # 3/4 * 2^q scaled by 2^151: 3 * 2^(q + 149)
        k = 0  # floor(log10(3/4 * 2^q)) by exact integers
        scale = 2 ** 151

        def at_most(k):  # 10^k <= 3/4 * 2^q
            return 10 ** k * scale <= exact if k >= 0 else scale <= exact * 10 ** -k

        while not at_most(k):
            k -= 1
        while at_most(k + 1):
            k += 1
        assert (q * 1262611 - 524031) >> 22 == k, q
        assert K_MIN <= -((q * 1262611) >> 22) <= K_MAX and K_MIN <= -k <= K_MAX


if __name__ == "__main__":
    main()
