// region_bases.hip -- K12 region_set_bases: the bases of the rows that fall inside every region of a set, in one pass over the rows
// (plan kind 12), a translation unit of its own so that kernels.o and region_set.o stay what they were.
//
//   WHAT IS SUMMED.  Rows and regions are 1-based inclusive, as in K6 / K11.  A row [s, e] with s <= e on a region's contig covers
//   max(0, min(e, re_i) - max(s, rs_i) + 1) bases of the region [rs_i, re_i]; bases_i is the sum of that over the counted rows.  The
//   alignment span counts as covered, deletions and reference skips included: that is what the `end` column holds.
//
//   THE STATE ADDS.  Per contig the POINTS are the sorted unique values { rs_i - 1 } U { re_i }, k points
//   x_0 < ... < x_{k - 1}.  A counted row computes p = |{ points < s }| and q = |{ points < e }| (one lower bound, one table, both in
//   [0, k]) and adds 1 to Ns[p], s to Ss[p], 1 to Ne[q], e to Se[q].  With inclusive prefix sums over the contig's bins
//       G(x_r)  = (x_r + 1) * cNs[r] - cSs[r] - x_r * cNe[r] + cSe[r]       bases of the contig's rows at positions <= x_r
//       bases_i = G(re_i) - G(rs_i - 1)
//   Two binary searches and four adds per row, whatever M is.  Every word and the decode are unsigned 64-bit arithmetic MODULO 2^64:
//   all steps are ring operations, so bases_i is exact whenever it fits an int64, with an open end (x + 1 wraps) and with coordinate
//   sums beyond 2^63.  A row with e < s is counted in `inverted` and for no region (the DECISION in include/exon_hip.h).
//
//   State: [counted, null_rows, elsewhere, inverted] [Ns] [Ss] [Ne] [Se], four sections of P + C int64 words; contig c (k_c points,
//   the points of the contigs in front of it sum to poff[c]) owns bins [poff[c] + c, poff[c] + c + k_c] of each section.
//
//   TABLES (device, owned by the plan; a names-form plan gets the map from the scan): map[ref id] -> contig slot or -1, poff[C + 1],
//   the points sorted within each contig.
//
//   TWO TIERS, chosen per plan.  P + C <= REGION_BASES_LDS_MAX: each workgroup copies the point table into LDS and adds there, the
//   counts into u32 bins (ds_add_u32) and the sums into u64 bins (ds_add_u64), then adds its non-zero bins to the state with one
//   global atomic each.  Beyond: the searches read the table through L2 and every add is a global 64-bit atomic.  In both, the lanes
//   of a wave that hit the bin of the wave's first live lane are combined once there are 16 of them: ONE add of their count, and
//   ONE add of the sum of their values, which a 6-step DPP scan over the wave makes (region_rows.h's wave_sum, shared with K13).  A
//   coordinate-sorted file sends whole waves to one bin; left alone that is 64 serialised adds on one address, twice.  Fewer lanes
//   add for themselves: the scan costs more.
//
//   ROWS.  region_rows.h walks them (shared with K11): the loads, the head rule, the map lookup, the four totals and the launches.
//   This file holds what a row ADDS: the point table and its LDS copy, the two searches, the combined adds and the LDS flush.
#include "region_rows.h"

namespace exon {
namespace {

using namespace region_rows;

// cnt[idx] += 1 and sum[idx] += val (modulo 2^64) for every lane with `act`.  When RB_COMBINE_MIN lanes or more share the bin of the
// wave's first live lane, they become one add of their count and one add of the sum of their values (region_rows.h's wave_sum);
// every other lane adds for itself.  Called by whole waves (the ballots and the scan need every lane).
constexpr int RB_COMBINE_MIN = COMBINE_MIN;
template <typename T>
__device__ __forceinline__ void rb_add(T* cnt, unsigned long long* sum, int idx, unsigned long long val, bool act, int lane) {
  const unsigned long long live = __ballot(act);
  if (!live) return;
  int first = -1;
  unsigned long long sm = 0;
  if (__popcll(live) >= RB_COMBINE_MIN) {  // (wave-uniform, as everything decided from a ballot)
    first = __ffsll((long long)live) - 1;
    const int k = __builtin_amdgcn_readlane(idx, first);  // (no trip through the LDS pipeline)
    sm = __ballot(act && idx == k);
  }
  if (__popcll(sm) >= RB_COMBINE_MIN) {
    const bool same = (sm >> lane) & 1;
    const unsigned long long tot = wave_sum(same ? val : 0ull);
    if (lane == first) {
      atomicAdd(&cnt[idx], (T)__popcll(sm));
      atomicAdd(&sum[idx], tot);
    } else if (act && !same) {
      atomicAdd(&cnt[idx], (T)1);
      atomicAdd(&sum[idx], val);
    }
  } else if (act) {
    atomicAdd(&cnt[idx], (T)1);
    atomicAdd(&sum[idx], val);
  }
}

template <typename W>
struct RBSections {
  W *Ns, *Ne;
  unsigned long long *Ss, *Se;
};

template <int THREADS, bool LDS>
__global__ __launch_bounds__(THREADS) void k_region_set_bases(const Rows a, const RegionBasesTables t) {
  typedef typename BinWord<LDS>::type word;
  extern __shared__ __align__(16) unsigned char rb_lds[];
  __shared__ unsigned long long tot[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int P = t.P, NB = t.P + t.C;
  const int64_t* points = t.points;
  RBSections<word> b;
  if (LDS) {  // [points: P x 8] [Ss: NB x 8] [Se: NB x 8] [Ns: NB x 4] [Ne: NB x 4]
    int64_t* l_points = reinterpret_cast<int64_t*>(rb_lds);
    unsigned long long* l_sums = reinterpret_cast<unsigned long long*>(l_points + P);
    unsigned* l_cnts = reinterpret_cast<unsigned*>(l_sums + 2 * NB);
    for (int i = tid; i < P; i += THREADS) l_points[i] = t.points[i];
    for (int i = tid; i < 2 * NB; i += THREADS) {
      l_sums[i] = 0;
      l_cnts[i] = 0;
    }
    points = l_points;
    b.Ss = l_sums, b.Se = l_sums + NB;
    b.Ns = reinterpret_cast<word*>(l_cnts), b.Ne = reinterpret_cast<word*>(l_cnts + NB);
  } else {
    b.Ns = reinterpret_cast<word*>(a.state + 4);
    b.Ss = a.state + 4 + NB;
    b.Ne = reinterpret_cast<word*>(a.state + 4 + 2 * (int64_t)NB);
    b.Se = a.state + 4 + 3 * (int64_t)NB;
  }
  if (tid < 4) tot[tid] = 0;
  __syncthreads();

  walk<THREADS>(a, tot, [&](int32_t slot, int64_t s, int64_t e) {
    const bool hit = slot >= 0;
    int lo = 0, m = 0;
    if (hit) {
      lo = t.poff[slot];
      m = t.poff[slot + 1] - lo;
    }
    const int p = count_below<false>(points + lo, m, s);
    const int q = count_below<false>(points + lo, m, e);
    const int base = hit ? lo + slot : 0;
    rb_add(b.Ns, b.Ss, base + p, (unsigned long long)s, hit, lane);
    rb_add(b.Ne, b.Se, base + q, (unsigned long long)e, hit, lane);
  });

  if (LDS) {  // the workgroup's non-zero bins, one global atomic each; sections in state order Ns, Ss, Ne, Se
    const unsigned long long* l_sums = reinterpret_cast<const unsigned long long*>(rb_lds + (size_t)P * 8);
    const unsigned* l_cnts = reinterpret_cast<const unsigned*>(l_sums + 2 * NB);
    for (int i = tid; i < NB; i += THREADS) {
      if (const unsigned v = l_cnts[i]) atomicAdd(&a.state[4 + i], (unsigned long long)v);
      if (const unsigned long long v = l_sums[i]) atomicAdd(&a.state[4 + (int64_t)NB + i], v);
      if (const unsigned v = l_cnts[NB + i]) atomicAdd(&a.state[4 + 2 * (int64_t)NB + i], (unsigned long long)v);
      if (const unsigned long long v = l_sums[NB + i]) atomicAdd(&a.state[4 + 3 * (int64_t)NB + i], v);
    }
  }
}

template <int THREADS, bool LDS>
hipError_t rb_launch(hipStream_t s, const LaunchCfg& cfg, const Rows& a, const RegionBasesTables& t, int64_t span) {
  return launch<THREADS, k_region_set_bases<THREADS, LDS>>(s, cfg, a, t, span, LDS ? region_bases_lds_bytes(t.P, t.C) : 0, REGION_BASES_LDS_MAX * 32);
}

}  // namespace

hipError_t launch_region_set_bases(hipStream_t s, const LaunchCfg& cfg, const uint8_t* ones, const int32_t* ref, const uint8_t* ref_valid,
                                   const int64_t* start, const uint8_t* start_valid, const int64_t* end, const uint8_t* end_valid, int64_t n,
                                   const RegionBasesTables& t, int64_t* d_state) {
  const Rows all{ref, ref_valid, start, start_valid, end, end_valid, ones, n, 0, 0, t.map, t.n_map, t.C, reinterpret_cast<unsigned long long*>(d_state)};
  // (a contig has two points or more: rs - 1 < re)
  const bool ok = !(t.C < 1 || t.P < 2 * (int64_t)t.C || t.P > 2 * REGION_SET_MAX_REGIONS || t.n_map < 0);
  const bool lds = t.P + t.C <= REGION_BASES_LDS_MAX;
  return run(s, cfg, all, region_bases_words(t.P, t.C), ok, [&](bool big, const Rows& a, int64_t span) {
    if (lds) return big ? rb_launch<1024, true>(s, cfg, a, t, span) : rb_launch<256, true>(s, cfg, a, t, span);
    return big ? rb_launch<1024, false>(s, cfg, a, t, span) : rb_launch<256, false>(s, cfg, a, t, span);
  });
}

}  // namespace exon
