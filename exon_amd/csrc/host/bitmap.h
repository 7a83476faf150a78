// bitmap.h -- bit utilities of the staging layer (Arrow LSB-first validity bitmaps).  Host only, no dependencies: stream.cpp
// appends every pushed batch's validity through append_bits, and tests/bitmap_host_harness.cpp runs the same function under
// AddressSanitizer / UndefinedBehaviorSanitizer on buffers of their exact size.
#pragma once

#include <cstdint>
#include <cstring>

namespace exon {

// OR bits [src_off, src_off + n) of `src` into `dst` at bit dst_off (the destination bits are 0 before: staging bitmaps are
// zeroed when a slot is recycled).  src == nullptr: n set bits (a batch without a validity buffer behind one that had one).
// Touches bytes [dst_off / 8, (dst_off + n + 7) / 8) of dst and [src_off / 8, (src_off + n + 7) / 8) of src, nothing else.
inline void append_bits(uint8_t* dst, int64_t dst_off, const uint8_t* src, int64_t src_off, int64_t n) {
  if (n <= 0) return;
  if (src == nullptr) {  // all valid
    int64_t i = 0;
    while (i < n && ((dst_off + i) & 7)) {
      dst[(dst_off + i) >> 3] |= (uint8_t)(1u << ((dst_off + i) & 7));
      ++i;
    }
    const int64_t full = (n - i) / 8;
    if (full > 0) memset(dst + ((dst_off + i) >> 3), 0xFF, (size_t)full);
    i += full * 8;
    for (; i < n; ++i) dst[(dst_off + i) >> 3] |= (uint8_t)(1u << ((dst_off + i) & 7));
    return;
  }
  if (((dst_off | src_off) & 7) == 0) {
    const int64_t full = n / 8;
    memcpy(dst + (dst_off >> 3), src + (src_off >> 3), (size_t)full);
    for (int64_t i = full * 8; i < n; ++i)
      if ((src[(src_off + i) >> 3] >> ((src_off + i) & 7)) & 1) dst[(dst_off + i) >> 3] |= (uint8_t)(1u << ((dst_off + i) & 7));
    return;
  }
  for (int64_t i = 0; i < n; ++i)
    if ((src[(src_off + i) >> 3] >> ((src_off + i) & 7)) & 1) dst[(dst_off + i) >> 3] |= (uint8_t)(1u << ((dst_off + i) & 7));
}

}  // namespace exon
