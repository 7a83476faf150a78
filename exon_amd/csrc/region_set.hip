// region_set.hip -- K11 region_set_overlap: overlap counts for a whole region set in one pass over the rows (plan kind 11), a
// translation unit of its own so that kernels.o stays what it was.
//
//   WHAT IS COUNTED.  K6's predicate, 1-based inclusive, for each of M regions at once: row [s, e] on reference r and region
//   [rs_i, re_i] on the same reference overlap iff s <= re_i AND e >= rs_i, with r, s, e all valid.
//
//   THE STATE ADDS.  A row and a region of its contig do NOT overlap iff re_i < s or rs_i > e, and for s <= e the
//   two exclude each other.  With the contig's region ends sorted (region i has rank a_i there) and its starts sorted (rank b_i),
//   a row computes  p = |{ i : re_i < s }|  (lower bound of s in the ends) and  q = |{ i : rs_i <= e }|  (upper bound of e in the
//   starts), both in [0, m], and adds 1 to A[p] and 1 to B[q].  Then
//       count_i = sum(A[0 .. a_i]) - sum(B[0 .. b_i])
//   = (rows with re_i >= s) - (rows with rs_i > e).  Two binary searches and two histogram adds per row, whatever M is, and every
//   state word adds: launches, streams, ranks and files merge by addition.  A row with e < s would break the identity and is
//   counted in `inverted` and for no region (the DECISION in include/exon_hip.h).
//
//   State: [counted, null_rows, elsewhere, inverted] [A: M + C] [B: M + C] int64 words; contig c (m_c regions, the regions of the
//   contigs in front of it sum to off[c]) owns bins [off[c] + c, off[c] + c + m_c] of A and of B.
//
//   TABLES (device, owned by the plan; a names-form plan gets the map from the scan): map[ref id] -> contig slot or -1, off[C + 1],
//   the ends and the starts sorted within each contig.
//
//   TWO TIERS, chosen per plan.  M + C <= REGION_SET_LDS_MAX: each workgroup copies both sorted tables into LDS and counts into a
//   u32 histogram pair there (ds_add_u32), then adds its non-zero bins to the state with one global atomic each.  Beyond: the
//   searches read the tables through L2 and every add is a global int64 atomic.  In both, lanes of a wave that hit the bin of the
//   wave's first live lane are combined into ONE add of their count (a coordinate-sorted file sends whole waves to one bin; left
//   alone that is 64 serialised adds on one address).
//
//   ROWS.  region_rows.h walks them (shared with K12): the loads, the head rule, the map lookup, the four totals and the launches.
//   This file holds what a row ADDS: the tables and their LDS copy, the two searches, the combined adds and the LDS flush.
#include "region_rows.h"

namespace exon {
namespace {

using namespace region_rows;

// bins[idx] += 1 for every lane with `act`; the lanes that share the bin of the wave's first live lane become one add of their
// count.  Called by whole waves (the ballots need every lane).
template <typename T>
__device__ __forceinline__ void rs_add(T* bins, int idx, bool act, int lane) {
  const unsigned long long live = __ballot(act);
  if (!live) return;
  const int first = __ffsll((long long)live) - 1;
  const int k = __shfl(idx, first, 64);
  const bool same = act && idx == k;
  const unsigned long long sm = __ballot(same);
  if (lane == first) atomicAdd(&bins[k], (T)__popcll(sm));
  else if (act && !same) atomicAdd(&bins[idx], (T)1);
}

template <int THREADS, bool LDS>
__global__ __launch_bounds__(THREADS) void k_region_set_overlap(const Rows a, const RegionSetTables t) {
  typedef typename BinWord<LDS>::type word;
  extern __shared__ __align__(16) unsigned char rs_lds[];
  __shared__ unsigned long long tot[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int M = t.M, NB = t.M + t.C;
  const int64_t* ends = t.ends;
  const int64_t* starts = t.starts;
  word *A, *B;
  if (LDS) {  // [ends: M x 8] [starts: M x 8] [A: NB x 4] [B: NB x 4]
    int64_t* l_ends = reinterpret_cast<int64_t*>(rs_lds);
    int64_t* l_starts = l_ends + M;
    unsigned* l_bins = reinterpret_cast<unsigned*>(l_starts + M);
    for (int i = tid; i < M; i += THREADS) {
      l_ends[i] = t.ends[i];
      l_starts[i] = t.starts[i];
    }
    for (int i = tid; i < 2 * NB; i += THREADS) l_bins[i] = 0;
    ends = l_ends, starts = l_starts;
    A = reinterpret_cast<word*>(l_bins);
    B = reinterpret_cast<word*>(l_bins + NB);
  } else {
    A = reinterpret_cast<word*>(a.state + 4);
    B = reinterpret_cast<word*>(a.state + 4 + NB);
  }
  if (tid < 4) tot[tid] = 0;
  __syncthreads();

  walk<THREADS>(a, tot, [&](int32_t slot, int64_t s, int64_t e) {
    const bool hit = slot >= 0;
    int lo = 0, m = 0;
    if (hit) {
      lo = t.off[slot];
      m = t.off[slot + 1] - lo;
    }
    const int p = count_below<false>(ends + lo, m, s);
    const int q = count_below<true>(starts + lo, m, e);
    const int base = hit ? lo + slot : 0;
    rs_add(A, base + p, hit, lane);
    rs_add(B, base + q, hit, lane);
  });

  if (LDS) {  // the workgroup's non-zero bins, one global atomic each
    const unsigned* l_bins = reinterpret_cast<const unsigned*>(rs_lds + (size_t)M * 16);
    for (int i = tid; i < 2 * NB; i += THREADS)
      if (const unsigned v = l_bins[i]) atomicAdd(&a.state[4 + i], (unsigned long long)v);
  }
}

template <int THREADS, bool LDS>
hipError_t rs_launch(hipStream_t s, const LaunchCfg& cfg, const Rows& a, const RegionSetTables& t, int64_t span) {
  return launch<THREADS, k_region_set_overlap<THREADS, LDS>>(s, cfg, a, t, span, LDS ? region_set_lds_bytes(t.M, t.C) : 0,
                                                            (int)region_set_lds_bytes(REGION_SET_LDS_MAX - 1, 1));
}

}  // namespace

hipError_t launch_region_set_overlap(hipStream_t s, const LaunchCfg& cfg, const uint8_t* ones, const int32_t* ref, const uint8_t* ref_valid,
                                     const int64_t* start, const uint8_t* start_valid, const int64_t* end, const uint8_t* end_valid, int64_t n,
                                     const RegionSetTables& t, int64_t* d_state) {
  const Rows all{ref, ref_valid, start, start_valid, end, end_valid, ones, n, 0, 0, t.map, t.n_map, t.C, reinterpret_cast<unsigned long long*>(d_state)};
  const bool ok = !(t.M < 1 || t.C < 1 || t.C > t.M || t.M > REGION_SET_MAX_REGIONS || t.n_map < 0);
  const bool lds = t.M + t.C <= REGION_SET_LDS_MAX;
  return run(s, cfg, all, region_set_words(t.M, t.C), ok, [&](bool big, const Rows& a, int64_t span) {
    if (lds) return big ? rs_launch<1024, true>(s, cfg, a, t, span) : rs_launch<256, true>(s, cfg, a, t, span);
    return big ? rs_launch<1024, false>(s, cfg, a, t, span) : rs_launch<256, false>(s, cfg, a, t, span);
  });
}

}  // namespace exon
