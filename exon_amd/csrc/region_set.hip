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
//   ROWS.  K6's loads: per lane 4 consecutive rows = one 16-byte load of the ids and two of each coordinate, validity by nibble.
//   Column bases need their element's alignment only: the host finds the `head` (0 .. 3 rows) behind which all three columns
//   are 16-byte aligned; rows in front of it and behind the last whole tile are read one by one, and columns that never line up
//   (head = n) are read one by one throughout.
#include <algorithm>

#include "kernels.h"

namespace exon {
namespace {

typedef int rs_v4i __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ T rs_ld16(const void* p) {  // streaming 16-byte load
  static_assert(sizeof(T) == 16, "16-byte vector expected");
  const rs_v4i v = __builtin_nontemporal_load(reinterpret_cast<const rs_v4i*>(p));
  T r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}
template <typename T>
__device__ __forceinline__ T rs_ld16_plain(const void* p) {  // the second half of a lane's 32 bytes: the line is already there
  static_assert(sizeof(T) == 16, "16-byte vector expected");
  const rs_v4i v = *reinterpret_cast<const rs_v4i*>(p);
  T r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}
// validity bits of rows [r, r + 4) (all below n); a NULL bitmap reads the 64 bytes of 0xFF instead: no branch in the tile loop
__device__ __forceinline__ unsigned rs_valid4(const uint8_t* __restrict__ bm, const uint8_t* __restrict__ ones, int64_t r) {
  const uint8_t* p0 = bm ? bm + (r >> 3) : ones;
  const uint8_t* p1 = bm ? bm + ((r + 3) >> 3) : ones;
  return ((unsigned(*p0) | unsigned(*p1) << 8) >> (r & 7)) & 0xFu;
}
__device__ __forceinline__ bool rs_valid1(const uint8_t* __restrict__ bm, int64_t r) { return bm == nullptr ? true : ((bm[r >> 3] >> (r & 7)) & 1); }

struct RSArgs {
  const int32_t* ref;
  const uint8_t* rv;
  const int64_t* start;
  const uint8_t* sv;
  const int64_t* end;
  const uint8_t* ev;
  const uint8_t* ones;
  int64_t n, head, ntiles;  // rows [head, head + ntiles * TILE) are read 16 bytes at a time
  RegionSetTables t;
  unsigned long long* state;
};

// |{ i < m : tab[i] < x }| (UPPER: <= x): branch-free halving, ceil(log2 m) dependent loads
template <bool UPPER>
__device__ __forceinline__ int rs_search(const int64_t* __restrict__ tab, int m, int64_t x) {
  if (m <= 0) return 0;
  int base = 0, len = m;
  while (len > 1) {
    const int half = len >> 1;
    const int64_t v = tab[base + half - 1];
    base += (UPPER ? v <= x : v < x) ? half : 0;
    len -= half;
  }
  const int64_t v = tab[base];
  return base + ((UPPER ? v <= x : v < x) ? 1 : 0);
}

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

template <bool LDS>
struct RSBins;
template <>
struct RSBins<true> {
  typedef unsigned word;
};
template <>
struct RSBins<false> {
  typedef unsigned long long word;
};

struct RSTotals {
  unsigned counted = 0, null_rows = 0, elsewhere = 0, inverted = 0;
};

// one row, by a whole wave: `live` is false for lanes that have none
template <bool LDS>
__device__ __forceinline__ void rs_row(const RSArgs& a, const int64_t* __restrict__ ends, const int64_t* __restrict__ starts,
                                       typename RSBins<LDS>::word* A, typename RSBins<LDS>::word* B, bool live, int32_t r, int64_t s,
                                       int64_t e, bool valid, RSTotals& t, int lane) {
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
    lo = a.t.off[slot];
    m = a.t.off[slot + 1] - lo;
  }
  const int p = rs_search<false>(ends + lo, m, s);
  const int q = rs_search<true>(starts + lo, m, e);
  const int base = hit ? lo + slot : 0;
  rs_add(A, base + p, hit, lane);
  rs_add(B, base + q, hit, lane);
}

template <int THREADS, bool LDS>
__global__ __launch_bounds__(THREADS) void k_region_set_overlap(const RSArgs a) {
  constexpr int WAVES = THREADS / 64, WT = 256 * RS_J, TILE = WAVES * WT;
  typedef typename RSBins<LDS>::word word;
  extern __shared__ __align__(16) unsigned char rs_lds[];
  __shared__ unsigned long long tot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.t.M, NB = a.t.M + a.t.C;
  const int64_t* ends = a.t.ends;
  const int64_t* starts = a.t.starts;
  word *A, *B;
  if (LDS) {
    int64_t* l_ends = reinterpret_cast<int64_t*>(rs_lds);
    int64_t* l_starts = l_ends + M;
    unsigned* l_bins = reinterpret_cast<unsigned*>(l_starts + M);
    for (int i = tid; i < M; i += THREADS) {
      l_ends[i] = a.t.ends[i];
      l_starts[i] = a.t.starts[i];
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

  RSTotals t;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t wbase = a.head + tile * TILE + (int64_t)wave * WT;
    int4 c[RS_J];
    longlong2 s0[RS_J], s1[RS_J], e0[RS_J], e1[RS_J];
    unsigned rm[RS_J], sm[RS_J], em[RS_J];
#pragma unroll
    for (int j = 0; j < RS_J; ++j) {
      const int64_t r = wbase + j * 256 + lane * 4;
      c[j] = rs_ld16<int4>(a.ref + r);
      s0[j] = rs_ld16<longlong2>(a.start + r);
      s1[j] = rs_ld16_plain<longlong2>(a.start + r + 2);
      e0[j] = rs_ld16<longlong2>(a.end + r);
      e1[j] = rs_ld16_plain<longlong2>(a.end + r + 2);
      rm[j] = rs_valid4(a.rv, a.ones, r);
      sm[j] = rs_valid4(a.sv, a.ones, r);
      em[j] = rs_valid4(a.ev, a.ones, r);
    }
#pragma unroll
    for (int j = 0; j < RS_J; ++j) {
      const unsigned v = rm[j] & sm[j] & em[j];
      rs_row<LDS>(a, ends, starts, A, B, true, c[j].x, s0[j].x, e0[j].x, v >> 0 & 1, t, lane);
      rs_row<LDS>(a, ends, starts, A, B, true, c[j].y, s0[j].y, e0[j].y, v >> 1 & 1, t, lane);
      rs_row<LDS>(a, ends, starts, A, B, true, c[j].z, s1[j].x, e1[j].x, v >> 2 & 1, t, lane);
      rs_row<LDS>(a, ends, starts, A, B, true, c[j].w, s1[j].y, e1[j].y, v >> 3 & 1, t, lane);
    }
  }
  // the rows in front of `head` and behind the last whole tile, one by one; they go to the LAST workgroups, which have a tile less
  // when the tiles do not divide evenly.  Whole waves walk the loop (rs_add's ballots).
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
      valid = rs_valid1(a.rv, r) && rs_valid1(a.sv, r) && rs_valid1(a.ev, r);
    }
    rs_row<LDS>(a, ends, starts, A, B, live, id, s, e, valid, t, lane);
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
  if (LDS) {
    const unsigned* l_bins = reinterpret_cast<const unsigned*>(rs_lds + (size_t)M * 16);
    for (int i = tid; i < 2 * NB; i += THREADS)
      if (const unsigned v = l_bins[i]) atomicAdd(&a.state[4 + i], (unsigned long long)v);
  }
}

template <int THREADS, bool LDS>
hipError_t rs_launch(hipStream_t s, const LaunchCfg& cfg, RSArgs a, int64_t span) {
  constexpr int TILE = THREADS / 64 * 256 * RS_J;
  const size_t lds = LDS ? region_set_lds_bytes(a.t.M, a.t.C) : 0;
  if (lds > 48 * 1024) {
    static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_region_set_overlap<THREADS, LDS>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)region_set_lds_bytes(REGION_SET_LDS_MAX - 1, 1));
    if (attr != hipSuccess) return attr;
  }
  a.ntiles = span / TILE;
  // a persistent grid: what is co-resident, at most one workgroup per tile; rows read one by one count as tiles of THREADS rows
  int resident = 1;  // (asked per launch for the small shape only: the LDS a workgroup takes is the plan's)
  if (THREADS < 1024 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, k_region_set_overlap<THREADS, LDS>, THREADS, lds) != hipSuccess || resident < 1))
    resident = 1;
  const int per_cu = THREADS >= 1024 ? 1 : std::min(std::max(cfg.blocks_per_cu, 1), resident);
  const int64_t work = a.ntiles + (a.n - a.ntiles * TILE + THREADS - 1) / THREADS;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)std::max(cfg.compute_units, 1) * per_cu, work));
  hipLaunchKernelGGL((k_region_set_overlap<THREADS, LDS>), dim3((unsigned)grid), dim3(THREADS), lds, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_region_set_overlap(hipStream_t s, const LaunchCfg& cfg, const uint8_t* ones, const int32_t* ref, const uint8_t* ref_valid,
                                     const int64_t* start, const uint8_t* start_valid, const int64_t* end, const uint8_t* end_valid, int64_t n,
                                     const RegionSetTables& t, int64_t* d_state) {
  hipError_t e;
  if (cfg.overwrite && (e = hipMemsetAsync(d_state, 0, (size_t)region_set_words(t.M, t.C) * 8, s)) != hipSuccess) return e;  // the kernel adds
  if (n <= 0) return hipSuccess;
  if (t.M < 1 || t.C < 1 || t.C > t.M || t.M > REGION_SET_MAX_REGIONS || t.n_map < 0) return hipErrorInvalidValue;
  // the head behind which all three columns are 16-byte aligned (their elements are aligned: capi.cpp); none: every row one by one
  int64_t head = n;
  for (int h = 0; h < 4; ++h)
    if (!((reinterpret_cast<uintptr_t>(ref + h) | reinterpret_cast<uintptr_t>(start + h) | reinterpret_cast<uintptr_t>(end + h)) & 15)) {
      head = std::min<int64_t>(h, n);
      break;
    }
  const bool lds = t.M + t.C <= REGION_SET_LDS_MAX;
  // u32 bins in LDS: a launch covers at most 2^31 rows
  for (int64_t o = 0; o < n; o += REGION_SET_LAUNCH_ROWS) {
    const int64_t m = std::min(n - o, REGION_SET_LAUNCH_ROWS);
    RSArgs a;
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
    if (lds) e = big ? rs_launch<1024, true>(s, cfg, a, span) : rs_launch<256, true>(s, cfg, a, span);
    else e = big ? rs_launch<1024, false>(s, cfg, a, span) : rs_launch<256, false>(s, cfg, a, span);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace exon
