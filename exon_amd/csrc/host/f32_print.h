// f32_print.h -- Rust's `{}` of an f32 without libc, usable in device code: the shortest decimal digits that read back as the
// same binary32 (the closest to the value among the shortest), written positionally, never with an exponent.
//
//   NaN -> "NaN"   +-inf -> "inf" / "-inf"   -0 -> "-0"   1.0 -> "1"   0.5 -> "0.5"   1e-5 -> "0.00001"   1e38 -> "1" + 38 zeros
//
// What the reference prints for the Float values of `info` / `formats` (host/vcf_text.h: rust_f32_display, which gets the digits
// from std::to_chars); the device printer of text_columns.hip (k_vcf_info_measure / k_vcf_info_fill) uses this header, and
// tools/check_f32_print.cpp compares the two over all 2^32 bit patterns.
//
// The digits are Schubfach's (R. Giulietti, "The Schubfach way to render doubles", 2020; the binary32 instance): one table
// lookup of g = ceil(10^-k / 2^r) (64 bits) and three 64 x 32 -> 96-bit products bound the value and its two rounding-interval
// ends on a scale where the answer is an integer of at most 9 digits.  No libm, no floating-point arithmetic at all, no private
// array: the characters go straight to the caller's buffer.
//
// LENGTH.  The decimal is d * 10^e with 1 <= d < 10^9 and -45 <= e <= 38 - (digits of d - 1): the coarsest grid that separates
// the subnormals (spacing 2^-149 = 1.4e-45) is 10^-45, and FLT_MAX is 3.4028235e38.  So the longest output is
//   '-' + "0." + 45 places = 48 bytes  (-1.1754942e-38 .. : "-0." + 37 zeros + 8 digits; the smallest subnormal: "-0." + 44 zeros + "1")
// and the longest integer '-' + 39 digits = 40.  kF32PrintMax = 48; the checker asserts it over every bit pattern.
#pragma once
#include <stdint.h>

#include "decimal_f32.h"  // EXON_HD, dec::mul64

namespace exon {
namespace f32p {

constexpr int kF32PrintMax = 48;
constexpr int kPow10Min = -31, kPow10Max = 45;

// g(k) = ceil(10^k / 2^(floor(log2(10^k)) - 63)) for k in [-31, 45]: tools/gen_f32_print_table.py regenerates the lines below
// with exact integers (and checks the fixed-point logarithms of floor_log2_pow10 / floor_log10_pow2 over the ranges used here).
#if defined(__HIP_DEVICE_COMPILE__)
__device__
#endif
static const uint64_t kPow10G[77] = {
    0x81ceb32c4b43fcf5ULL,  // -31
    0xa2425ff75e14fc32ULL,  // -30
    0xcad2f7f5359a3b3fULL,  // -29
    0xfd87b5f28300ca0eULL,  // -28
    0x9e74d1b791e07e49ULL,  // -27
    0xc612062576589ddbULL,  // -26
    0xf79687aed3eec552ULL,  // -25
    0x9abe14cd44753b53ULL,  // -24
    0xc16d9a0095928a28ULL,  // -23
    0xf1c90080baf72cb2ULL,  // -22
    0x971da05074da7befULL,  // -21
    0xbce5086492111aebULL,  // -20
    0xec1e4a7db69561a6ULL,  // -19
    0x9392ee8e921d5d08ULL,  // -18
    0xb877aa3236a4b44aULL,  // -17
    0xe69594bec44de15cULL,  // -16
    0x901d7cf73ab0acdaULL,  // -15
    0xb424dc35095cd810ULL,  // -14
    0xe12e13424bb40e14ULL,  // -13
    0x8cbccc096f5088ccULL,  // -12
    0xafebff0bcb24aaffULL,  // -11
    0xdbe6fecebdedd5bfULL,  // -10
    0x89705f4136b4a598ULL,  // -9
    0xabcc77118461cefdULL,  // -8
    0xd6bf94d5e57a42bdULL,  // -7
    0x8637bd05af6c69b6ULL,  // -6
    0xa7c5ac471b478424ULL,  // -5
    0xd1b71758e219652cULL,  // -4
    0x83126e978d4fdf3cULL,  // -3
    0xa3d70a3d70a3d70bULL,  // -2
    0xcccccccccccccccdULL,  // -1
    0x8000000000000000ULL,  // 0
    0xa000000000000000ULL,  // 1
    0xc800000000000000ULL,  // 2
    0xfa00000000000000ULL,  // 3
    0x9c40000000000000ULL,  // 4
    0xc350000000000000ULL,  // 5
    0xf424000000000000ULL,  // 6
    0x9896800000000000ULL,  // 7
    0xbebc200000000000ULL,  // 8
    0xee6b280000000000ULL,  // 9
    0x9502f90000000000ULL,  // 10
    0xba43b74000000000ULL,  // 11
    0xe8d4a51000000000ULL,  // 12
    0x9184e72a00000000ULL,  // 13
    0xb5e620f480000000ULL,  // 14
    0xe35fa931a0000000ULL,  // 15
    0x8e1bc9bf04000000ULL,  // 16
    0xb1a2bc2ec5000000ULL,  // 17
    0xde0b6b3a76400000ULL,  // 18
    0x8ac7230489e80000ULL,  // 19
    0xad78ebc5ac620000ULL,  // 20
    0xd8d726b7177a8000ULL,  // 21
    0x878678326eac9000ULL,  // 22
    0xa968163f0a57b400ULL,  // 23
    0xd3c21bcecceda100ULL,  // 24
    0x84595161401484a0ULL,  // 25
    0xa56fa5b99019a5c8ULL,  // 26
    0xcecb8f27f4200f3aULL,  // 27
    0x813f3978f8940985ULL,  // 28
    0xa18f07d736b90be6ULL,  // 29
    0xc9f2c9cd04674edfULL,  // 30
    0xfc6f7c4045812297ULL,  // 31
    0x9dc5ada82b70b59eULL,  // 32
    0xc5371912364ce306ULL,  // 33
    0xf684df56c3e01bc7ULL,  // 34
    0x9a130b963a6c115dULL,  // 35
    0xc097ce7bc90715b4ULL,  // 36
    0xf0bdc21abb48db21ULL,  // 37
    0x96769950b50d88f5ULL,  // 38
    0xbc143fa4e250eb32ULL,  // 39
    0xeb194f8e1ae525feULL,  // 40
    0x92efd1b8d0cf37bfULL,  // 41
    0xb7abc627050305aeULL,  // 42
    0xe596b7b0c643c71aULL,  // 43
    0x8f7e32ce7bea5c70ULL,  // 44
    0xb35dbf821ae4f38cULL,  // 45
};

EXON_HD int floor_log2_pow10(int e) { return (e * 1741647) >> 19; }                       // floor(log2(10^e)), |e| <= 1233
EXON_HD int floor_log10_pow2(int e) { return (e * 1262611) >> 22; }                       // floor(log10(2^e)), |e| <= 1500
EXON_HD int floor_log10_three_quarters_pow2(int e) { return (e * 1262611 - 524031) >> 22; }  // floor(log10(3/4 * 2^e))

// floor(g * cp / 2^64), with bit 0 set when bits [33, 64) of the product are not all zero ("round to odd": the two bits below the
// integer part keep enough of the fraction for the comparisons below)
EXON_HD uint32_t round_to_odd(uint64_t g, uint32_t cp) {
  uint64_t hi, lo;
  dec::mul64(g, (uint64_t)cp, &hi, &lo);
  return (uint32_t)hi | (uint32_t)((uint32_t)(lo >> 32) > 1u);
}

// the shortest decimal of a finite, non-zero binary32 (sign excluded): value = *digits * 10^*exp10, *digits without trailing zeros
EXON_HD void shortest(uint32_t bits, uint32_t* digits, int* exp10) {
  const uint32_t sig = bits & 0x7FFFFFu, ex = (bits >> 23) & 0xFFu;
  uint32_t c;
  int q;
  if (ex != 0) {
    c = sig | 0x800000u;
    q = (int)ex - 150;
  } else {
    c = sig;
    q = -149;
  }
  uint32_t d;
  int k;
  if (ex != 0 && q <= 0 && q > -24 && (c & ((1u << -q) - 1u)) == 0) {  // an integer below 2^24: itself
    d = c >> -q;
    k = 0;
  } else {
    const bool even = (c & 1u) == 0;
    const bool lower_closer = sig == 0 && ex > 1;  // the value below a power of two is half as far away
    const uint32_t cbl = 4 * c - 2 + (lower_closer ? 1u : 0u), cb = 4 * c, cbr = 4 * c + 2;
    k = lower_closer ? floor_log10_three_quarters_pow2(q) : floor_log10_pow2(q);
    const int h = q + floor_log2_pow10(-k) + 1;  // 1 <= h <= 4
    const uint64_t g = kPow10G[-k - kPow10Min];
    const uint32_t vbl = round_to_odd(g, cbl << h), vb = round_to_odd(g, cb << h), vbr = round_to_odd(g, cbr << h);
    const uint32_t lower = vbl + (even ? 0u : 1u), upper = vbr - (even ? 0u : 1u);
    const uint32_t s = vb / 4;
    bool done = false;
    d = 0;
    if (s >= 10) {  // a digit fewer, when exactly one of the two candidates lies inside the rounding interval
      const uint32_t sp = s / 10;
      const bool up_in = lower <= 40 * sp, wp_in = 40 * sp + 40 <= upper;
      if (up_in != wp_in) {
        d = sp + (wp_in ? 1u : 0u);
        ++k;
        done = true;
      }
    }
    if (!done) {
      const bool u_in = lower <= 4 * s, w_in = 4 * s + 4 <= upper;
      if (u_in != w_in) {
        d = s + (w_in ? 1u : 0u);
      } else {  // both or neither: the closer one, ties to even
        const uint32_t mid = 4 * s + 2;
        d = s + ((vb > mid || (vb == mid && (s & 1u))) ? 1u : 0u);
      }
    }
  }
  while (d % 10u == 0) {  // (d != 0; at most 9 rounds)
    d /= 10u;
    ++k;
  }
  *digits = d;
  *exp10 = k;
}

EXON_HD int digit_count(uint32_t d) {  // 1 <= d < 10^9
  return 1 + (d >= 10u) + (d >= 100u) + (d >= 1000u) + (d >= 10000u) + (d >= 100000u) + (d >= 1000000u) + (d >= 10000000u) + (d >= 100000000u);
}

// Rust's `{}` of the f32 with these bits.  out == nullptr: the length alone (the measure pass); else the characters are written
// to out[0 .. length) -- never more than kF32PrintMax, no terminator -- and the length is returned.
template <class Byte>
EXON_HD int print(uint32_t bits, Byte* out) {
  const bool neg = (bits >> 31) != 0;
  const uint32_t mag = bits & 0x7FFFFFFFu;
  if (mag > 0x7F800000u) {
    if (out) out[0] = (Byte)'N', out[1] = (Byte)'a', out[2] = (Byte)'N';
    return 3;
  }
  int n = 0;
  if (neg) {
    if (out) out[0] = (Byte)'-';
    n = 1;
  }
  if (mag == 0x7F800000u) {
    if (out) out[n] = (Byte)'i', out[n + 1] = (Byte)'n', out[n + 2] = (Byte)'f';
    return n + 3;
  }
  if (mag == 0) {
    if (out) out[n] = (Byte)'0';
    return n + 1;
  }
  uint32_t d;
  int e;
  shortest(mag, &d, &e);
  const int nd = digit_count(d);
  // the digits occupy [at, at + nd) with a '.' inside them (point > 0: behind digit `point`), zeros around them otherwise
  const int point = nd + e;  // digits in front of the decimal point (<= 0: "0." and -point zeros first)
  int at, len;
  if (e >= 0) {
    at = n;
    len = n + nd + e;
  } else if (point > 0) {
    at = n;
    len = n + nd + 1;
  } else {
    at = n + 2 - point;
    len = at + nd;
  }
  if (!out) return len;
  if (e >= 0) {
    for (int i = 0; i < e; ++i) out[n + nd + i] = (Byte)'0';
  } else if (point <= 0) {
    out[n] = (Byte)'0';
    out[n + 1] = (Byte)'.';
    for (int i = 0; i < -point; ++i) out[n + 2 + i] = (Byte)'0';
  }
  for (int i = nd - 1; i >= 0; --i) {  // last digit first; the ones behind the point sit a byte further right
    const int shift = (e < 0 && point > 0 && i >= point) ? 1 : 0;
    out[at + i + shift] = (Byte)('0' + d % 10u);
    d /= 10u;
  }
  if (e < 0 && point > 0) out[at + point] = (Byte)'.';
  return len;
}

// the length alone
EXON_HD int length(uint32_t bits) { return print<char>(bits, (char*)0); }

}  // namespace f32p
}  // namespace exon
