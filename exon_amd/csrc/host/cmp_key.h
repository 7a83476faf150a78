// cmp_key.h -- `x <op> literal` folded into an inclusive range of 32-bit totalOrder keys: the one comparison rule of the fused
// kernels (kernels.hip: K4, K8, k_value_mask evaluate it with cmp_key_passes) and of the host reader's pushed-down value predicate
// (formats.h: vcf_value_hit evaluates it with cmp_key_hit).  Host only, no HIP.
#pragma once
#include <cstdint>
#include <cstring>

namespace exon {

// the f32 with totalOrder key k, and the totalOrder keys of an f32 / an f64 (sign-magnitude bits -> two's complement order)
inline float h_key_f32(int32_t k) {
  int32_t b = k ^ ((k >> 31) & 0x7FFFFFFF);
  float f;
  memcpy(&f, &b, 4);
  return f;
}
inline int32_t h_f32_key(float f) {
  int32_t b;
  memcpy(&b, &f, 4);
  return b ^ ((b >> 31) & 0x7FFFFFFF);
}
inline int64_t h_f64_key(double d) {
  int64_t b;
  memcpy(&b, &d, 8);
  return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFLL);
}
// smallest key k in [INT32_MIN, INT32_MAX + 1] whose column value compares >= t (or > t) with the literal.
//   Float32 column: the value of key k is the f32 with that totalOrder key, widened to f64, compared in totalOrder;
//   Int32 column (x_is_int): the value IS k.  DataFusion compares Int32 with an Int64 literal as integers and with a
//   Float64 literal after casting the column to Float64; every int32 is exact in f64, so one f64 comparison covers both
//   (an integer literal beyond 2^53 is beyond int32 anyway: the range saturates the same way).  A NaN or -0.0 literal
//   behaves as in arrow-rs' totalOrder float compare: NaN above every number, (f64)0 = +0.0 above -0.0.
inline int64_t first_key_not_less(int64_t t, bool strict_greater, bool x_is_int) {
  int64_t lo = INT32_MIN, hi = (int64_t)INT32_MAX + 1;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const int64_t km = h_f64_key(x_is_int ? (double)(int32_t)mid : (double)h_key_f32((int32_t)mid));
    const bool ok = strict_greater ? (km > t) : (km >= t);
    if (ok) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
inline bool cmp_to_key_range(double thr, int cmp_op, bool x_is_int, int32_t* klo, int32_t* khi, int32_t* negate) {
  const int64_t t = h_f64_key(thr);
  const int64_t ge = first_key_not_less(t, false, x_is_int);  // first key with value >= thr
  const int64_t gt = first_key_not_less(t, true, x_is_int);   // first key with value >  thr
  int64_t lo, hi;
  *negate = 0;
  switch (cmp_op) {
    case 0: lo = gt; hi = INT32_MAX; break;            // >
    case 1: lo = ge; hi = INT32_MAX; break;            // >=
    case 2: lo = INT32_MIN; hi = ge - 1; break;        // <
    case 3: lo = INT32_MIN; hi = gt - 1; break;        // <=
    case 4: lo = ge; hi = gt - 1; break;               // =
    case 5: lo = ge; hi = gt - 1; *negate = 1; break;  // !=
    default: return false;
  }
  if (lo > hi) {  // empty range: encode as an impossible interval
    *klo = INT32_MAX;
    *khi = INT32_MIN;
  } else {
    *klo = (int32_t)lo;
    *khi = (int32_t)hi;
  }
  return true;
}
// a VALID value's key against the folded range: cmp_key_passes (kernels.hip) on the host, bit for bit
inline bool cmp_key_hit(int32_t key, int32_t klo, int32_t khi, int32_t negate) { return ((key >= klo) & (key <= khi)) != (negate != 0); }

}  // namespace exon
