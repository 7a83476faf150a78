// region_depth.h -- host side of plan kind 14 (per-base depth over a region set): the target space, the compressed coordinate, the
// per-base depth and the threshold counts per region.  No device code: exon_hip_region_depth_layout / _intervals / _per_base / _decode
// work without a GPU.
//
// TARGET SPACE.  Contigs in order of first appearance.  Per contig the regions are sorted and merged into disjoint intervals
// [ms_j, me_j] (two merge when the next start <= the current end + 1: overlapping and abutting regions alike); cum_j = the bases of the
// contig's intervals in front of interval j, T_c its target bases, T = sum of T_c.  Contig c owns T_c + 1 consecutive bins of the one
// section D, from doff_c = (T of the contigs in front) + c: one bin per target base and a terminator.
//
// COMPRESSED COORDINATE.  below_c(x) = the contig's target bases at positions <= x: with j = |{ intervals : ms <= x }|, 0 if j = 0,
// else cum_{j-1} + min(x - ms_{j-1} + 1, len_{j-1}).  A region [rs, re] is the bins [below(rs - 1), below(re)) of its contig, re - rs + 1
// of them.  A counted row [s, e] with lo = below(s - 1) (0 for s <= 1) and hi = below(e) adds +1 to D[doff_c + lo] and 2^64 - 1 to
// D[doff_c + hi] if hi > lo, else nothing.  Every contig's bins then sum to 0 modulo 2^64, so THE DEPTH OF BIN b IS THE RUNNING SUM OF
// THE WHOLE SECTION UP TO b, taken as one array: host and device define it so and agree word for word on any input.
//
// The decode is NOT linear: bases_i (the sum of the depths of the region's bins) adds over partial states, ge_t (the bins whose depth,
// read as int64, is >= thresholds[t]) does not.  Partial states are added first, then decoded.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "region_set.h"

namespace exon {

struct RegionDepth : RegionSetSpec {
  std::vector<int64_t> thresholds;   // [k] strictly increasing, each >= 1
  int32_t I = 0;                     // merged intervals of all contigs
  int64_t T = 0;                     // target bases of all contigs
  std::vector<int32_t> ioff;         // [C + 1] intervals in front of each contig
  std::vector<int32_t> doff;         // [C] first bin of each contig
  std::vector<int64_t> ms, me;       // [I] merged intervals, contig c at [ioff[c], ioff[c + 1]), ascending
  std::vector<int32_t> cum, len;     // [I] target bases of the contig in front of the interval, and its own
  std::vector<int32_t> lo, hi;       // [M] region i is the bins [lo[i], hi[i]) of D

  static constexpr int64_t MAX_BINS = (int64_t)1 << 26;
  static constexpr int MAX_THRESHOLDS = 8;

  int64_t bins() const { return T + C; }
  int64_t words() const { return 4 + bins(); }
  int32_t k() const { return (int32_t)thresholds.size(); }

  // the contig's target bases at positions <= x, for every int64 x
  int64_t below(int32_t c, int64_t x) const {
    const int64_t* b = ms.data() + ioff[(size_t)c];
    const int64_t* e = ms.data() + ioff[(size_t)c + 1];
    const int64_t j = std::upper_bound(b, e, x) - b;
    if (j == 0) return 0;
    const size_t at = (size_t)ioff[(size_t)c] + (size_t)j - 1;
    const uint64_t d = (uint64_t)x - (uint64_t)ms[at];  // x >= ms >= 1: no wrap
    return (int64_t)cum[at] + (int64_t)std::min<uint64_t>(d, (uint64_t)len[at] - 1) + 1;
  }

  // slot[], starts, ends and C are set: the merged intervals and T; false (nothing else is built): T + C is beyond MAX_BINS
  bool build() {
    std::vector<std::vector<std::pair<int64_t, int64_t>>> per((size_t)C);
    for (int32_t i = 0; i < M; ++i) per[(size_t)slot[(size_t)i]].emplace_back(starts[(size_t)i], ends[(size_t)i]);
    ioff.assign((size_t)C + 1, 0);
    ms.clear(), me.clear();
    for (int32_t c = 0; c < C; ++c) {
      auto& v = per[(size_t)c];
      std::sort(v.begin(), v.end());
      for (const auto& r : v) {
        // (ends are below INT64_MAX: the constructor refuses an open end)
        if ((int32_t)ms.size() > ioff[(size_t)c] && r.first <= me.back() + 1) me.back() = std::max(me.back(), r.second);
        else ms.push_back(r.first), me.push_back(r.second);
      }
      ioff[(size_t)c + 1] = (int32_t)ms.size();
    }
    I = (int32_t)ms.size();
    const uint64_t sat = (uint64_t)1 << 62;  // T saturates here: an interval may hold 2^63 - 2 bases
    uint64_t total = 0;
    for (int32_t j = 0; j < I; ++j) total = std::min(total + std::min((uint64_t)me[(size_t)j] - (uint64_t)ms[(size_t)j] + 1, sat), sat);
    T = (int64_t)total;
    if (T + C > MAX_BINS) return false;
    cum.resize((size_t)I), len.resize((size_t)I), doff.resize((size_t)C);
    int64_t front = 0;
    for (int32_t c = 0; c < C; ++c) {
      doff[(size_t)c] = (int32_t)(front + c);
      int64_t within = 0;
      for (int32_t j = ioff[(size_t)c]; j < ioff[(size_t)c + 1]; ++j) {
        cum[(size_t)j] = (int32_t)within;
        len[(size_t)j] = (int32_t)(me[(size_t)j] - ms[(size_t)j] + 1);
        within += len[(size_t)j];
      }
      front += within;
    }
    lo.resize((size_t)M), hi.resize((size_t)M);
    for (int32_t i = 0; i < M; ++i) {
      const int32_t c = slot[(size_t)i];
      lo[(size_t)i] = doff[(size_t)c] + (int32_t)below(c, starts[(size_t)i] - 1);
      hi[(size_t)i] = doff[(size_t)c] + (int32_t)below(c, ends[(size_t)i]);
    }
    return true;
  }

  // bin of the first base of merged interval j (j counts over all contigs)
  int64_t interval_bin(int32_t c, int32_t j) const { return (int64_t)doff[(size_t)c] + cum[(size_t)j]; }

  // the running sum of the whole section: out[b] = D[0] + ... + D[b] modulo 2^64, NB words
  void running(const int64_t* state, uint64_t* out) const {
    const uint64_t* D = reinterpret_cast<const uint64_t*>(state) + 4;
    uint64_t f = 0;
    for (int64_t b = 0, nb = bins(); b < nb; ++b) out[b] = (f += D[b]);
  }
  // the depth of every target base in bin order, the C terminator bins left out
  void per_base(const int64_t* state, int64_t* out) const {
    std::vector<uint64_t> run((size_t)bins());
    running(state, run.data());
    int64_t o = 0;
    for (int32_t c = 0; c < C; ++c) {
      const int64_t b0 = doff[(size_t)c], b1 = c + 1 < C ? (int64_t)doff[(size_t)c + 1] - 1 : bins() - 1;
      for (int64_t b = b0; b < b1; ++b) out[o++] = (int64_t)run[(size_t)b];
    }
  }
  // row-major [M][1 + k]: bases_i, then ge_t for every threshold
  void decode(const int64_t* state, int64_t* out) const {
    std::vector<uint64_t> run((size_t)bins());
    running(state, run.data());
    const int32_t kk = k();
    for (int32_t i = 0; i < M; ++i) {
      uint64_t bases = 0, ge[MAX_THRESHOLDS] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int64_t b = lo[(size_t)i]; b < hi[(size_t)i]; ++b) {
        bases += run[(size_t)b];
        for (int32_t t = 0; t < kk; ++t) ge[t] += (int64_t)run[(size_t)b] >= thresholds[(size_t)t];
      }
      int64_t* row = out + (size_t)i * (size_t)(1 + kk);
      row[0] = (int64_t)bases;
      for (int32_t t = 0; t < kk; ++t) row[1 + t] = (int64_t)ge[t];
    }
  }
};

}  // namespace exon
