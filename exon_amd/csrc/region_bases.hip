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
//   ONE add of the sum of their values, which a 6-step DPP scan over the wave makes.  A coordinate-sorted file sends whole waves to
//   one bin; left alone that is 64 serialised adds on one address, twice.  Fewer lanes add for themselves: the scan costs more.
//
//   ROWS.  K11's loop: per lane 4 consecutive rows = one 16-byte load of the ids and two of each coordinate, validity by nibble.
//   Column bases need their element's alignment only: the host finds the `head` (0 .. 3 rows) behind which all three columns
//   are 16-byte aligned; rows in front of it and behind the last whole tile are read one by one, by whole waves, and columns that
//   never line up (head = n) are read one by one throughout.
#include <algorithm>

#include "kernels.h"

namespace exon {
namespace {

typedef int rb_v4i __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ T rb_ld16(const void* p) {  // streaming 16-byte load
  static_assert(sizeof(T) == 16, "16-byte vector expected");
  const rb_v4i v = __builtin_nontemporal_load(reinterpret_cast<const rb_v4i*>(p));
  T r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}
template <typename T>
__device__ __forceinline__ T rb_ld16_plain(const void* p) {  // the second half of a lane's 32 bytes: the line is already there
  static_assert(sizeof(T) == 16, "16-byte vector expected");
  const rb_v4i v = *reinterpret_cast<const rb_v4i*>(p);
  T r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}
// validity bits of rows [r, r + 4) (all below n); a NULL bitmap reads the 64 bytes of 0xFF instead: no branch in the tile loop
__device__ __forceinline__ unsigned rb_valid4(const uint8_t* __restrict__ bm, const uint8_t* __restrict__ ones, int64_t r) {
  const uint8_t* p0 = bm ? bm + (r >> 3) : ones;
  const uint8_t* p1 = bm ? bm + ((r + 3) >> 3) : ones;
  return ((unsigned(*p0) | unsigned(*p1) << 8) >> (r & 7)) & 0xFu;
}
__device__ __forceinline__ bool rb_valid1(const uint8_t* __restrict__ bm, int64_t r) { return bm == nullptr ? true : ((bm[r >> 3] >> (r & 7)) & 1); }

struct RBArgs {
  const int32_t* ref;
  const uint8_t* rv;
  const int64_t* start;
  const uint8_t* sv;
  const int64_t* end;
  const uint8_t* ev;
  const uint8_t* ones;
  int64_t n, head, ntiles;  // rows [head, head + ntiles * TILE) are read 16 bytes at a time
  RegionBasesTables t;
  unsigned long long* state;
};

// |{ i < m : tab[i] < x }|: branch-free halving, ceil(log2 m) dependent loads
__device__ __forceinline__ int rb_search(const int64_t* __restrict__ tab, int m, int64_t x) {
  if (m <= 0) return 0;
  int base = 0, len = m;
  while (len > 1) {
    const int half = len >> 1;
    base += tab[base + half - 1] < x ? half : 0;
    len -= half;
  }
  return base + (tab[base] < x ? 1 : 0);
}

// the sum of `v` over the 64 lanes of a wave, modulo 2^64, in every lane.  Called by whole waves.  An inclusive scan by DPP row
// shifts (1, 2, 4, 8 within a row of 16 lanes, lanes shifted in from outside read 0), then lane 15 of rows 0 and 2 added to rows 1
// and 3 and lane 31 to rows 2 and 3: lane 63 holds the total.  VALU only -- a __shfl_xor butterfly is 12 ds_bpermute per sum, on the
// LDS pipeline the searches and the adds need.
__device__ __forceinline__ unsigned long long rb_wave_sum(unsigned long long v) {
#define RB_DPP_ADD(CTRL, ROWS)                                                                                  \
  {                                                                                                             \
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, ROWS, 0xf, true);         \
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, ROWS, 0xf, true); \
    v += (unsigned long long)hi << 32 | lo;                                                                     \
  }
  RB_DPP_ADD(0x111, 0xf)  // row_shr:1
  RB_DPP_ADD(0x112, 0xf)  // row_shr:2
  RB_DPP_ADD(0x114, 0xf)  // row_shr:4
  RB_DPP_ADD(0x118, 0xf)  // row_shr:8
  RB_DPP_ADD(0x142, 0xa)  // row_bcast:15 into rows 1 and 3 (the other rows add `old` = 0)
  RB_DPP_ADD(0x143, 0xc)  // row_bcast:31 into rows 2 and 3
#undef RB_DPP_ADD
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return (unsigned long long)hi << 32 | lo;
}

// cnt[idx] += 1 and sum[idx] += val (modulo 2^64) for every lane with `act`.  When RB_COMBINE_MIN lanes or more share the bin of the
// wave's first live lane, they become one add of their count and one add of the sum of their values; every other lane adds for
// itself.  Called by whole waves (the ballots and the scan need every lane).  The threshold: the scan is about 30 VALU instructions
// a sum, a few lanes on one address serialise for a few cycles each; measured, combining from two lanes on cost rows in random order
// 0.2 ms per 1e8 (profiles/region_set_bases.md), while whole waves on one bin -- a coordinate-sorted file -- need it.
constexpr int RB_COMBINE_MIN = 16;
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
    const unsigned long long tot = rb_wave_sum(same ? val : 0ull);
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

template <bool LDS>
struct RBBins;
template <>
struct RBBins<true> {
  typedef unsigned word;
};
template <>
struct RBBins<false> {
  typedef unsigned long long word;
};

struct RBTotals {
  unsigned counted = 0, null_rows = 0, elsewhere = 0, inverted = 0;
};

template <typename W>
struct RBSections {
  W *Ns, *Ne;
  unsigned long long *Ss, *Se;
};

// one row, by a whole wave: `live` is false for lanes that have none
template <bool LDS>
__device__ __forceinline__ void rb_row(const RBArgs& a, const int64_t* __restrict__ points, const RBSections<typename RBBins<LDS>::word>& b, bool live,
                                       int32_t r, int64_t s, int64_t e, bool valid, RBTotals& t, int lane) {
  valid = live && valid;
  int32_t slot = -1;
  if (valid && (uint32_t)r < (uint32_t)a.t.n_map) slot = a.t.map[r];  // (an id below 0 is beyond the map as unsigned)
  const bool on = slot >= 0 && slot < a.t.C;
  const bool hit = on && e >= s;
  t.null_rows += live && !valid;
  t.elsewhere += valid && !on;
  t.inverted += on && !hit;
  t.counted += hit;
  int lo = 0, m = 0;
  if (hit) {
    lo = a.t.poff[slot];
    m = a.t.poff[slot + 1] - lo;
  }
  const int p = rb_search(points + lo, m, s);
  const int q = rb_search(points + lo, m, e);
  const int base = hit ? lo + slot : 0;
  rb_add(b.Ns, b.Ss, base + p, (unsigned long long)s, hit, lane);
  rb_add(b.Ne, b.Se, base + q, (unsigned long long)e, hit, lane);
}

template <int THREADS, bool LDS>
__global__ __launch_bounds__(THREADS) void k_region_set_bases(const RBArgs a) {
  constexpr int WAVES = THREADS / 64, WT = 256 * RS_J, TILE = WAVES * WT;
  typedef typename RBBins<LDS>::word word;
  extern __shared__ __align__(16) unsigned char rb_lds[];
  __shared__ unsigned long long tot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = a.t.P, NB = a.t.P + a.t.C;
  const int64_t* points = a.t.points;
  RBSections<word> b;
  if (LDS) {  // [points: P x 8] [Ss: NB x 8] [Se: NB x 8] [Ns: NB x 4] [Ne: NB x 4]
    int64_t* l_points = reinterpret_cast<int64_t*>(rb_lds);
    unsigned long long* l_sums = reinterpret_cast<unsigned long long*>(l_points + P);
    unsigned* l_cnts = reinterpret_cast<unsigned*>(l_sums + 2 * NB);
    for (int i = tid; i < P; i += THREADS) l_points[i] = a.t.points[i];
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

  RBTotals t;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t wbase = a.head + tile * TILE + (int64_t)wave * WT;
    int4 c[RS_J];
    longlong2 s0[RS_J], s1[RS_J], e0[RS_J], e1[RS_J];
    unsigned rm[RS_J], sm[RS_J], em[RS_J];
#pragma unroll
    for (int j = 0; j < RS_J; ++j) {
      const int64_t r = wbase + j * 256 + lane * 4;
      c[j] = rb_ld16<int4>(a.ref + r);
      s0[j] = rb_ld16<longlong2>(a.start + r);
      s1[j] = rb_ld16_plain<longlong2>(a.start + r + 2);
      e0[j] = rb_ld16<longlong2>(a.end + r);
      e1[j] = rb_ld16_plain<longlong2>(a.end + r + 2);
      rm[j] = rb_valid4(a.rv, a.ones, r);
      sm[j] = rb_valid4(a.sv, a.ones, r);
      em[j] = rb_valid4(a.ev, a.ones, r);
    }
#pragma unroll
    for (int j = 0; j < RS_J; ++j) {
      const unsigned v = rm[j] & sm[j] & em[j];
      rb_row<LDS>(a, points, b, true, c[j].x, s0[j].x, e0[j].x, v >> 0 & 1, t, lane);
      rb_row<LDS>(a, points, b, true, c[j].y, s0[j].y, e0[j].y, v >> 1 & 1, t, lane);
      rb_row<LDS>(a, points, b, true, c[j].z, s1[j].x, e1[j].x, v >> 2 & 1, t, lane);
      rb_row<LDS>(a, points, b, true, c[j].w, s1[j].y, e1[j].y, v >> 3 & 1, t, lane);
    }
  }
  // the rows in front of `head` and behind the last whole tile, one by one; they go to the LAST workgroups, which have a tile less
  // when the tiles do not divide evenly.  Whole waves walk the loop (rb_add's ballots).
  const int64_t vec_rows = a.ntiles * TILE, scalar_rows = a.n - vec_rows;
  for (int64_t k0 = (int64_t)(gridDim.x - 1u - blockIdx.x) * THREADS; k0 < scalar_rows; k0 += (int64_t)gridDim.x * THREADS) {
    const int64_t k = k0 + tid;
    const bool live = k < scalar_rows;
    const int64_t r = !live ? 0 : k < a.head ? k : k + vec_rows;
    int32_t id = 0;
    int64_t s = 0, e = 0;
    bool valid = false;
    if (live) {
      id = a.ref[r], s = a.start[r], e = a.end[r];
      valid = rb_valid1(a.rv, r) && rb_valid1(a.sv, r) && rb_valid1(a.ev, r);
    }
    rb_row<LDS>(a, points, b, live, id, s, e, valid, t, lane);
  }

  // totals: lanes -> wave -> workgroup -> state
  unsigned long long w[4] = {t.counted, t.null_rows, t.elsewhere, t.inverted};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w[i] += __shfl_down(w[i], o, 64);
    if (lane == 0 && w[i]) atomicAdd(&tot[i], w[i]);
  }
  __syncthreads();
  if (tid < 4 && tot[tid]) atomicAdd(&a.state[tid], tot[tid]);
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
hipError_t rb_launch(hipStream_t s, const LaunchCfg& cfg, RBArgs a, int64_t span) {
  constexpr int TILE = THREADS / 64 * 256 * RS_J;
  const size_t lds = LDS ? region_bases_lds_bytes(a.t.P, a.t.C) : 0;
  if (lds > 48 * 1024) {
    static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_region_set_bases<THREADS, LDS>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, REGION_BASES_LDS_MAX * 32);
    if (attr != hipSuccess) return attr;
  }
  a.ntiles = span / TILE;
  // a persistent grid: what is co-resident, at most one workgroup per tile; rows read one by one count as tiles of THREADS rows
  int resident = 1;  // (asked per launch for the small shape only: the LDS a workgroup takes is the plan's)
  if (THREADS < 1024 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, k_region_set_bases<THREADS, LDS>, THREADS, lds) != hipSuccess || resident < 1))
    resident = 1;
  const int per_cu = THREADS >= 1024 ? 1 : std::min(std::max(cfg.blocks_per_cu, 1), resident);
  const int64_t work = a.ntiles + (a.n - a.ntiles * TILE + THREADS - 1) / THREADS;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)std::max(cfg.compute_units, 1) * per_cu, work));
  hipLaunchKernelGGL((k_region_set_bases<THREADS, LDS>), dim3((unsigned)grid), dim3(THREADS), lds, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_region_set_bases(hipStream_t s, const LaunchCfg& cfg, const uint8_t* ones, const int32_t* ref, const uint8_t* ref_valid,
                                   const int64_t* start, const uint8_t* start_valid, const int64_t* end, const uint8_t* end_valid, int64_t n,
                                   const RegionBasesTables& t, int64_t* d_state) {
  hipError_t e;
  if (cfg.overwrite && (e = hipMemsetAsync(d_state, 0, (size_t)region_bases_words(t.P, t.C) * 8, s)) != hipSuccess) return e;  // the kernel adds
  if (n <= 0) return hipSuccess;
  // (a contig has two points or more: rs - 1 < re)
  if (t.C < 1 || t.P < 2 * (int64_t)t.C || t.P > 2 * REGION_SET_MAX_REGIONS || t.n_map < 0) return hipErrorInvalidValue;
  // the head behind which all three columns are 16-byte aligned (their elements are aligned: capi.cpp); none: every row one by one
  int64_t head = n;
  for (int h = 0; h < 4; ++h)
    if (!((reinterpret_cast<uintptr_t>(ref + h) | reinterpret_cast<uintptr_t>(start + h) | reinterpret_cast<uintptr_t>(end + h)) & 15)) {
      head = std::min<int64_t>(h, n);
      break;
    }
  const bool lds = t.P + t.C <= REGION_BASES_LDS_MAX;
  // u32 counts in LDS: a launch covers at most 2^31 rows
  for (int64_t o = 0; o < n; o += REGION_SET_LAUNCH_ROWS) {
    const int64_t m = std::min(n - o, REGION_SET_LAUNCH_ROWS);
    RBArgs a;
    a.ref = ref + o, a.start = start + o, a.end = end + o;
    // (REGION_SET_LAUNCH_ROWS is a multiple of 8: the bitmaps move by whole bytes)
    a.rv = ref_valid ? ref_valid + (o >> 3) : nullptr, a.sv = start_valid ? start_valid + (o >> 3) : nullptr, a.ev = end_valid ? end_valid + (o >> 3) : nullptr;
    a.ones = ones;
    a.n = m;
    a.head = std::min(head, m);
    a.ntiles = 0;
    a.t = t;
    a.state = reinterpret_cast<unsigned long long*>(d_state);
    const int64_t span = m - a.head;
    const bool big = span / RS_TILE_BIG >= std::max(cfg.compute_units, 1);
    if (lds) e = big ? rb_launch<1024, true>(s, cfg, a, span) : rb_launch<256, true>(s, cfg, a, span);
    else e = big ? rb_launch<1024, false>(s, cfg, a, span) : rb_launch<256, false>(s, cfg, a, span);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace exon
