// region_rows.h -- the row walk that the region-set kernels share (K11 region_set.hip, K12 region_bases.hip, K13 window_bases.hip, K14 region_depth.hip): how a kernel gets from
// the three interval columns to "this row is on contig slot c with coordinates [s, e]", and how the host cuts the rows into launches.
// What a row then ADDS is the including kernel's business: it hands walk() a functor.  Included by .hip files only.
//
//   ROWS.  K6's loads: per lane 4 consecutive rows = one 16-byte load of the ids and two of each coordinate, validity by nibble.
//   Column bases need their element's alignment only: the host finds the `head` (0 .. 3 rows) behind which all three columns
//   are 16-byte aligned; rows in front of it and behind the last whole tile are read one by one, by whole waves, and columns that
//   never line up (head = n) are read one by one throughout.  (kernels.hip keeps loads of its own: its valid4_ones relies on a
//   256-row-aligned wave base, which the head rule gives up.)
#pragma once
#include <algorithm>

#include "kernels.h"

namespace exon {
namespace region_rows {

typedef int v4i __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ T ld16(const void* p) {  // streaming 16-byte load
  static_assert(sizeof(T) == 16, "16-byte vector expected");
  const v4i v = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(p));
  T r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}
template <typename T>
__device__ __forceinline__ T ld16_plain(const void* p) {  // the second half of a lane's 32 bytes: the line is already there
  static_assert(sizeof(T) == 16, "16-byte vector expected");
  const v4i v = *reinterpret_cast<const v4i*>(p);
  T r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}
// validity bits of rows [r, r + 4) (all below n); a NULL bitmap reads the 64 bytes of 0xFF instead: no branch in the tile loop
__device__ __forceinline__ unsigned valid4(const uint8_t* __restrict__ bm, const uint8_t* __restrict__ ones, int64_t r) {
  const uint8_t* p0 = bm ? bm + (r >> 3) : ones;
  const uint8_t* p1 = bm ? bm + ((r + 3) >> 3) : ones;
  return ((unsigned(*p0) | unsigned(*p1) << 8) >> (r & 7)) & 0xFu;
}
__device__ __forceinline__ bool valid1(const uint8_t* __restrict__ bm, int64_t r) { return bm == nullptr ? true : ((bm[r >> 3] >> (r & 7)) & 1); }

// the rows of one launch, the id -> contig slot map and the state the totals go to; a kernel's own tables travel beside it
struct Rows {
  const int32_t* ref;
  const uint8_t* rv;
  const int64_t* start;
  const uint8_t* sv;
  const int64_t* end;
  const uint8_t* ev;
  const uint8_t* ones;
  int64_t n, head, ntiles;  // rows [head, head + ntiles * TILE) are read 16 bytes at a time
  const int32_t* map;
  int32_t n_map, C;
  unsigned long long* state;
};

struct Totals {
  unsigned counted = 0, null_rows = 0, elsewhere = 0, inverted = 0;
};

// one row -> its contig slot, or -1 for a row that adds to no bin (`live` is false for lanes that have no row); counts it in `t`
__device__ __forceinline__ int32_t classify(const Rows& a, bool live, int32_t r, int64_t s, int64_t e, bool valid, Totals& t) {
  valid = live && valid;
  int32_t slot = -1;
  if (valid && (uint32_t)r < (uint32_t)a.n_map) slot = a.map[r];  // (an id below 0 is beyond the map as unsigned)
  const bool on = slot >= 0 && slot < a.C;
  const bool hit = on && e >= s;
  t.null_rows += live && !valid;
  t.elsewhere += valid && !on;
  t.inverted += on && !hit;
  t.counted += hit;
  return hit ? slot : -1;
}

// Every row of the launch that is this workgroup's: row(slot, s, e) is called by WHOLE WAVES -- the functors ballot -- with
// slot = -1 in the lanes that add nothing.  Then the four totals go lanes -> wave -> workgroup -> state.  `tot`: four LDS words
// that the kernel has zeroed, with a barrier behind it.  walk() ends behind a barrier of its own: every row() of the workgroup is
// done, the kernel may flush what they added to LDS.
template <int THREADS, typename Row>
__device__ __forceinline__ void walk(const Rows& a, unsigned long long* tot, Row row) {
  constexpr int WAVES = THREADS / 64, WT = 256 * RS_J, TILE = WAVES * WT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  Totals t;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t wbase = a.head + tile * TILE + (int64_t)wave * WT;
    int4 c[RS_J];
    longlong2 s0[RS_J], s1[RS_J], e0[RS_J], e1[RS_J];
    unsigned rm[RS_J], sm[RS_J], em[RS_J];
#pragma unroll
    for (int j = 0; j < RS_J; ++j) {
      const int64_t r = wbase + j * 256 + lane * 4;
      c[j] = ld16<int4>(a.ref + r);
      s0[j] = ld16<longlong2>(a.start + r);
      s1[j] = ld16_plain<longlong2>(a.start + r + 2);
      e0[j] = ld16<longlong2>(a.end + r);
      e1[j] = ld16_plain<longlong2>(a.end + r + 2);
      rm[j] = valid4(a.rv, a.ones, r);
      sm[j] = valid4(a.sv, a.ones, r);
      em[j] = valid4(a.ev, a.ones, r);
    }
#pragma unroll
    for (int j = 0; j < RS_J; ++j) {
      const unsigned v = rm[j] & sm[j] & em[j];
      row(classify(a, true, c[j].x, s0[j].x, e0[j].x, v >> 0 & 1, t), s0[j].x, e0[j].x);
      row(classify(a, true, c[j].y, s0[j].y, e0[j].y, v >> 1 & 1, t), s0[j].y, e0[j].y);
      row(classify(a, true, c[j].z, s1[j].x, e1[j].x, v >> 2 & 1, t), s1[j].x, e1[j].x);
      row(classify(a, true, c[j].w, s1[j].y, e1[j].y, v >> 3 & 1, t), s1[j].y, e1[j].y);
    }
  }
  // the rows in front of `head` and behind the last whole tile, one by one; they go to the LAST workgroups, which have a tile less
  // when the tiles do not divide evenly.  Whole waves walk the loop (the functors' ballots).
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
      valid = valid1(a.rv, r) && valid1(a.sv, r) && valid1(a.ev, r);
    }
    row(classify(a, live, id, s, e, valid, t), s, e);
  }

  unsigned long long w[4] = {t.counted, t.null_rows, t.elsewhere, t.inverted};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w[i] += __shfl_down(w[i], o, 64);
    if (lane == 0 && w[i]) atomicAdd(&tot[i], w[i]);
  }
  __syncthreads();
  if (tid < 4 && tot[tid]) atomicAdd(&a.state[tid], tot[tid]);
}

// |{ i < m : tab[i] < x }| (UPPER: <= x): branch-free halving, ceil(log2 m) dependent loads
template <bool UPPER>
__device__ __forceinline__ int count_below(const int64_t* __restrict__ tab, int m, int64_t x) {
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

// the sum of `v` over the 64 lanes of a wave, modulo 2^64, in every lane.  Called by whole waves.  An inclusive scan by DPP row
// shifts (1, 2, 4, 8 within a row of 16 lanes, lanes shifted in from outside read 0), then lane 15 of rows 0 and 2 added to rows 1
// and 3 and lane 31 to rows 2 and 3: lane 63 holds the total.  VALU only -- a __shfl_xor butterfly is 12 ds_bpermute per sum, on the
// LDS pipeline the searches and the adds need.
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#define RR_DPP_ADD(CTRL, ROWS)                                                                                  \
  {                                                                                                             \
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, ROWS, 0xf, true);         \
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, ROWS, 0xf, true); \
    v += (unsigned long long)hi << 32 | lo;                                                                     \
  }
  RR_DPP_ADD(0x111, 0xf)  // row_shr:1
  RR_DPP_ADD(0x112, 0xf)  // row_shr:2
  RR_DPP_ADD(0x114, 0xf)  // row_shr:4
  RR_DPP_ADD(0x118, 0xf)  // row_shr:8
  RR_DPP_ADD(0x142, 0xa)  // row_bcast:15 into rows 1 and 3 (the other rows add `old` = 0)
  RR_DPP_ADD(0x143, 0xc)  // row_bcast:31 into rows 2 and 3
#undef RR_DPP_ADD
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return (unsigned long long)hi << 32 | lo;
}
// The lanes of a wave that add to the bin of the wave's first live lane are combined into one add (K12's rb_add, K13's wb_add) once
// there are this many of them.  The scan is about 30 VALU instructions a sum, a few lanes on one address serialise for a few cycles
// each; measured on K12, combining from two lanes on cost rows in random order 0.2 ms per 1e8 (profiles/region_set_bases.md), while
// whole waves on one bin -- a coordinate-sorted file -- need it.
constexpr int COMBINE_MIN = 16;

// the word of a count bin: u32 in a workgroup's LDS (at most REGION_SET_LAUNCH_ROWS rows a launch), the state's 64 bits in memory
template <bool LDS>
struct BinWord {
  typedef unsigned long long type;
};
template <>
struct BinWord<true> {
  typedef unsigned type;
};

// one launch of KERNEL(rows, tables) with `lds` bytes of dynamic LDS (`lds_max`: the most any plan asks of this kernel) over
// a.n rows, `span` of them behind the head
template <int THREADS, auto KERNEL, typename Tables>
hipError_t launch(hipStream_t s, const LaunchCfg& cfg, Rows a, const Tables& t, int64_t span, size_t lds, int lds_max) {
  constexpr int TILE = THREADS / 64 * 256 * RS_J;
  if (lds > 48 * 1024) {
    static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    if (attr != hipSuccess) return attr;
  }
  a.ntiles = span / TILE;
  // a persistent grid: what is co-resident, at most one workgroup per tile; rows read one by one count as tiles of THREADS rows
  int resident = 1;  // (asked per launch for the small shape only: the LDS a workgroup takes is the plan's)
  if (THREADS < 1024 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, KERNEL, THREADS, lds) != hipSuccess || resident < 1)) resident = 1;
  const int per_cu = THREADS >= 1024 ? 1 : std::min(std::max(cfg.blocks_per_cu, 1), resident);
  const int64_t work = a.ntiles + (a.n - a.ntiles * TILE + THREADS - 1) / THREADS;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((int64_t)std::max(cfg.compute_units, 1) * per_cu, work));
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(THREADS), lds, s, a, t);
  return hipGetLastError();
}

// All rows of `all` (head and ntiles are set here) into its state of `words` words: shape(big, rows, span) launches one kernel
// over at most REGION_SET_LAUNCH_ROWS of them, 1024 threads if `big`, else 256.  `tables_ok`: the kernel's tables are what it expects.
template <typename Shape>
hipError_t run(hipStream_t s, const LaunchCfg& cfg, const Rows& all, int64_t words, bool tables_ok, Shape shape) {
  hipError_t e;
  if (cfg.overwrite && (e = hipMemsetAsync(all.state, 0, (size_t)words * 8, s)) != hipSuccess) return e;  // the kernel adds
  const int64_t n = all.n;
  if (n <= 0) return hipSuccess;
  if (!tables_ok) return hipErrorInvalidValue;
  // the head behind which all three columns are 16-byte aligned (their elements are aligned: capi.cpp); none: every row one by one
  int64_t head = n;
  for (int h = 0; h < 4; ++h)
    if (!((reinterpret_cast<uintptr_t>(all.ref + h) | reinterpret_cast<uintptr_t>(all.start + h) | reinterpret_cast<uintptr_t>(all.end + h)) & 15)) {
      head = std::min<int64_t>(h, n);
      break;
    }
  // u32 count bins in LDS: a launch covers at most 2^31 rows
  for (int64_t o = 0; o < n; o += REGION_SET_LAUNCH_ROWS) {
    Rows a = all;
    a.n = std::min(n - o, REGION_SET_LAUNCH_ROWS);
    a.ref += o, a.start += o, a.end += o;
    // (REGION_SET_LAUNCH_ROWS is a multiple of 8: the bitmaps move by whole bytes)
    if (a.rv) a.rv += o >> 3;
    if (a.sv) a.sv += o >> 3;
    if (a.ev) a.ev += o >> 3;
    a.head = std::min(head, a.n);
    a.ntiles = 0;
    const int64_t span = a.n - a.head;
    const bool big = span / RS_TILE_BIG >= std::max(cfg.compute_units, 1);
    if ((e = shape(big, a, span)) != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace region_rows
}  // namespace exon
