// region_bases.h -- host side of plan kind 12 (covered bases per region of a set): the point table the kernel searches, the point
// indices the decode needs, and the decode itself.  No device code: exon_hip_region_bases_layout / _decode work without a GPU.
//
// Per contig c the POINTS are the sorted unique values { rs_i - 1 } U { re_i } of its regions: k_c points x_0 < ... < x_{k_c - 1}.  A
// counted row [s, e] finds p = |{ points < s }| and q = |{ points < e }| (the same lower bound, both in [0, k_c]) and adds 1 to
// Ns[p], s to Ss[p], 1 to Ne[q], e to Se[q].  With inclusive prefix sums cNs, cSs, cNe, cSe over the contig's bins
//   G(x_r)  = (x_r + 1) * cNs[r] - cSs[r] - x_r * cNe[r] + cSe[r]     bases of the contig's rows at positions <= x_r
//   bases_i = G(re_i) - G(rs_i - 1)                                   
// ALL of it modulo 2^64: the four words and the decode are unsigned 64-bit ring arithmetic, so the result is exact whenever the true
// bases_i fits an int64 -- for re_i = EXON_HIP_REGION_OPEN_END, where x + 1 wraps, and for coordinate sums beyond 2^63 alike.
// Contig c's bins are words [poff[c] + c, poff[c] + c + k_c] of each of the four sections.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "region_set.h"

namespace exon {

struct RegionBases : RegionSetSpec {
  int32_t P = 0;                          // points
  std::vector<int32_t> poff;              // [C + 1] points in front of each contig
  std::vector<int64_t> points;            // [P], contig c at [poff[c], poff[c + 1]), ascending and unique
  std::vector<int32_t> idx_lo, idx_hi;    // [M] index of rs_i - 1 / re_i among its contig's points

  int64_t bins() const { return (int64_t)P + C; }
  int64_t words() const { return 4 + 4 * bins(); }

  // slot[], starts, ends and C are set: the rest
  void build() {
    std::vector<std::vector<int64_t>> per((size_t)C);
    for (int32_t i = 0; i < M; ++i) {
      per[(size_t)slot[(size_t)i]].push_back(starts[(size_t)i] - 1);
      per[(size_t)slot[(size_t)i]].push_back(ends[(size_t)i]);
    }
    poff.assign((size_t)C + 1, 0);
    points.clear();
    for (int32_t c = 0; c < C; ++c) {
      std::vector<int64_t>& v = per[(size_t)c];
      std::sort(v.begin(), v.end());
      v.erase(std::unique(v.begin(), v.end()), v.end());
      points.insert(points.end(), v.begin(), v.end());
      poff[(size_t)c + 1] = (int32_t)points.size();
    }
    P = (int32_t)points.size();
    idx_lo.resize((size_t)M), idx_hi.resize((size_t)M);
    for (int32_t i = 0; i < M; ++i) {
      const std::vector<int64_t>& v = per[(size_t)slot[(size_t)i]];
      idx_lo[(size_t)i] = (int32_t)(std::lower_bound(v.begin(), v.end(), starts[(size_t)i] - 1) - v.begin());
      idx_hi[(size_t)i] = (int32_t)(std::lower_bound(v.begin(), v.end(), ends[(size_t)i]) - v.begin());
    }
  }

  // linear in the state, modulo 2^64: decode(x + y) = decode(x) + decode(y)
  void decode(const int64_t* state, int64_t* out) const {
    const size_t nb = (size_t)bins();
    const uint64_t* Ns = reinterpret_cast<const uint64_t*>(state) + 4;
    const uint64_t *Ss = Ns + nb, *Ne = Ss + nb, *Se = Ne + nb;
    std::vector<uint64_t> g((size_t)P);  // G at every point
    for (int32_t c = 0; c < C; ++c) {
      const size_t p0 = (size_t)poff[(size_t)c], k = (size_t)poff[(size_t)c + 1] - p0, b0 = p0 + (size_t)c;
      uint64_t ns = 0, ss = 0, ne = 0, se = 0;
      for (size_t r = 0; r < k; ++r) {
        ns += Ns[b0 + r], ss += Ss[b0 + r], ne += Ne[b0 + r], se += Se[b0 + r];
        const uint64_t x = (uint64_t)points[p0 + r];
        g[p0 + r] = (x + 1) * ns - ss - x * ne + se;
      }
    }
    for (int32_t i = 0; i < M; ++i) {
      const size_t p0 = (size_t)poff[(size_t)slot[(size_t)i]];
      out[i] = (int64_t)(g[p0 + (size_t)idx_hi[(size_t)i]] - g[p0 + (size_t)idx_lo[(size_t)i]]);
    }
  }
};

}  // namespace exon
