// region_set.h -- host side of plan kind 11 (region-set overlap counts): the sorted tables the kernel searches, the ranks the decode
// needs, and the decode itself.  No device code: exon_hip_region_set_layout / _decode work without a GPU.
//
// Per contig c with regions i (caller order kept): ends sorted ascending, starts sorted ascending; rank_a[i] / rank_b[i] = position of
// region i's end / start in its contig's sorted order (ties: caller order, any fixed order does).  A row adds 1 to A[p], p = regions
// with end < row start, and to B[q], q = regions with start <= row end; then
//   count_i = sum(A[0 .. rank_a[i]]) - sum(B[0 .. rank_b[i]])      
// Contig c's bins are words [off[c] + c, off[c] + c + m_c] of A and of B.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace exon {

struct RegionSetSpec {  // what the caller gave: regions and their contigs (kinds 11 and 12 alike; stream.cpp fills it)
  int32_t M = 0, C = 0;
  bool by_name = false;
  std::vector<std::string> contig_names;  // [C], names form, in order of first appearance
  std::vector<int32_t> contig_ids;        // [C], ids form
  std::vector<int32_t> slot;              // [M] contig slot of region i
  std::vector<int64_t> starts, ends;      // [M] caller order
};
struct RegionSet : RegionSetSpec {
  std::vector<int32_t> off;               // [C + 1]
  std::vector<int64_t> sorted_ends, sorted_starts;  // [M], contig c at [off[c], off[c + 1])
  std::vector<int32_t> rank_a, rank_b;    // [M]

  int64_t words() const { return 4 + 2 * ((int64_t)M + C); }

  // slot[], starts, ends and C are set: the rest
  void build() {
    off.assign((size_t)C + 1, 0);
    for (int32_t i = 0; i < M; ++i) ++off[(size_t)slot[(size_t)i] + 1];
    for (int32_t c = 0; c < C; ++c) off[(size_t)c + 1] += off[(size_t)c];
    std::vector<int32_t> order((size_t)M), fill(off.begin(), off.end() - 1);
    for (int32_t i = 0; i < M; ++i) order[(size_t)fill[(size_t)slot[(size_t)i]]++] = i;  // regions grouped by contig, caller order within
    sorted_ends.resize((size_t)M), sorted_starts.resize((size_t)M), rank_a.resize((size_t)M), rank_b.resize((size_t)M);
    std::vector<int32_t> tmp;
    for (int32_t c = 0; c < C; ++c) {
      const int32_t lo = off[(size_t)c], m = off[(size_t)c + 1] - lo;
      for (int pass = 0; pass < 2; ++pass) {
        const std::vector<int64_t>& key = pass ? starts : ends;
        tmp.assign(order.begin() + lo, order.begin() + lo + m);
        std::stable_sort(tmp.begin(), tmp.end(), [&](int32_t x, int32_t y) { return key[(size_t)x] < key[(size_t)y]; });
        for (int32_t k = 0; k < m; ++k) {
          (pass ? sorted_starts : sorted_ends)[(size_t)(lo + k)] = key[(size_t)tmp[(size_t)k]];
          (pass ? rank_b : rank_a)[(size_t)tmp[(size_t)k]] = k;
        }
      }
    }
  }

  // linear in the state: decode(x + y) = decode(x) + decode(y)
  void decode(const int64_t* state, int64_t* out) const {
    const int64_t* A = state + 4;
    const int64_t* B = A + M + C;
    std::vector<int64_t> pa((size_t)M + C), pb((size_t)M + C);
    for (int32_t c = 0; c < C; ++c) {
      const size_t b0 = (size_t)off[(size_t)c] + c, b1 = (size_t)off[(size_t)c + 1] + c + 1;
      int64_t sa = 0, sb = 0;
      for (size_t k = b0; k < b1; ++k) {
        pa[k] = (sa += A[k]);
        pb[k] = (sb += B[k]);
      }
    }
    for (int32_t i = 0; i < M; ++i) {
      const size_t base = (size_t)off[(size_t)slot[(size_t)i]] + (size_t)slot[(size_t)i];
      out[i] = pa[base + (size_t)rank_a[(size_t)i]] - pb[base + (size_t)rank_b[(size_t)i]];
    }
  }
};

}  // namespace exon
