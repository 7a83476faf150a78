// window_bases.h -- host side of plan kind 13 (bases per fixed-width window along each contig): the contigs and their lengths, the
// window offsets, and the decode.  No device code: exon_hip_window_bases_layout / _offsets / _decode work without a GPU.
//
// Contig c of length L_c has K_c = ceil(L_c / W) windows, window j = [j * W + 1, min((j + 1) * W, L_c)], and owns bins
// [woff[c], woff[c + 1]) of the sections E and D.  A counted row, clipped to [1, L_c], with js = (s - 1) / W and je = (e - 1) / W adds
//   js == je:     E[js] += e - s + 1
//   otherwise:    E[js] += (js + 1) * W - s + 1,  E[je] += e - je * W
//   je > js + 1:  D[js + 1] += 1,  D[je] -= 1
// and bases_j = E[j] + W * (D[0] + ... + D[j]) within the contig.  ALL of it modulo 2^64.
#pragma once
#include <stdint.h>

#include <vector>

#include "region_set.h"

namespace exon {

// RegionSetSpec's contigs (by id or by name, slot = the caller's order); it has no regions: M stays 0
struct WindowBases : RegionSetSpec {
  int64_t W = 0;                 // the caller's width; a width beyond 2^31 - 1 cuts no contig (lengths are int32)
  int64_t B = 0;                 // windows of all contigs
  std::vector<int32_t> len;      // [C]
  std::vector<int32_t> woff;     // [C + 1] windows in front of each contig

  static constexpr int64_t MAX_BINS = (int64_t)1 << 25;

  int64_t words() const { return 4 + 2 * B; }
  static int64_t windows_of(int64_t L, int64_t W) { return (L - 1) / W + 1; }

  // len, W and C are set: B, and woff if B is within MAX_BINS (false: it is not)
  bool build() {
    B = 0;
    for (int32_t c = 0; c < C; ++c) B += windows_of(len[(size_t)c], W);
    if (B > MAX_BINS) return false;
    woff.assign((size_t)C + 1, 0);
    for (int32_t c = 0; c < C; ++c) woff[(size_t)c + 1] = woff[(size_t)c] + (int32_t)windows_of(len[(size_t)c], W);
    return true;
  }

  // window b of contig c, 1-based closed
  int64_t window_start(int64_t j) const { return j * W + 1; }
  int64_t window_end(int32_t c, int64_t j) const { return j + 1 == woff[(size_t)c + 1] - woff[(size_t)c] ? (int64_t)len[(size_t)c] : (j + 1) * W; }

  // linear in the state, modulo 2^64: decode(x + y) = decode(x) + decode(y)
  void decode(const int64_t* state, int64_t* out) const {
    const uint64_t* E = reinterpret_cast<const uint64_t*>(state) + 4;
    const uint64_t* D = E + B;
    for (int32_t c = 0; c < C; ++c) {
      uint64_t f = 0;
      for (int64_t b = woff[(size_t)c]; b < woff[(size_t)c + 1]; ++b) {
        f += D[b];
        out[b] = (int64_t)(E[b] + f * (uint64_t)W);
      }
    }
  }
};

}  // namespace exon
