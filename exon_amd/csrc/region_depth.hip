// region_depth.hip -- K14 region_set_depth: the per-base depth over the bases a region set covers, in one pass over the rows (plan kind
// 14), and the reduce that turns its state into bases and threshold counts per region on the device.  A translation unit of its own
// as K11 - K13 are.
//
//   TARGET SPACE (host/region_depth.h builds it).  Per contig the set's regions are merged into disjoint intervals [ms_j, me_j];
//   cum_j = the contig's target bases in front of interval j, T_c its target bases.  Contig c owns T_c + 1 bins of the one section D from
//   doff_c on: a bin per target base and a terminator.  below_c(x) = the contig's target bases at positions <= x: with
//   j = |{ ms <= x }|, 0 if j = 0, else cum_{j-1} + min(x - ms_{j-1} + 1, len_{j-1}).
//
//   THE STATE ADDS.  A counted row [s, e]: lo = below(s - 1) (0 for s <= 1), hi = below(e); if hi > lo, D[doff_c + lo]
//   += 1 and D[doff_c + hi] += 2^64 - 1, else nothing -- a read inside a gap adds nothing, one across a gap is still one pair.  Every
//   contig's bins sum to 0 modulo 2^64, so the depth of bin b is the running sum of the WHOLE section up to b.
//
//   State: [counted, null_rows, elsewhere, inverted] [D: T + C].
//
//   THREE TIERS, chosen per plan (kernels.h, region_depth_tier).  NB = T + C <= REGION_DEPTH_LDS_MAX: the bins sit in LDS as u64
//   (ds_add_u64) and the workgroup adds its non-zero bins to the state with one global atomic each; the interval table sits beside them
//   (tier 2) unless the two pass 128 KiB (tier 1: searched through L2).  Beyond the bound (tier 0): the searches go through L2 and every
//   add is a global 64-bit atomic.  In all, the lanes of a wave that hit the bin of the wave's first live lane are combined once there
//   are COMBINE_MIN of them: every lane of one call adds the same value, so the sum is that value times a popcount.
//
//   ROWS.  region_rows.h walks them (shared with K11 - K13).  This file holds what a row ADDS, and the reduce.
#include "region_rows.h"

namespace exon {
namespace {

using namespace region_rows;

// bins[idx] += val (modulo 2^64) for every lane with `act`; `val` is the same in every lane.  COMBINE_MIN lanes or more on the bin of
// the wave's first live lane become one add.  Called by whole waves.
__device__ __forceinline__ void rd_add(unsigned long long* bins, int idx, unsigned long long val, bool act, int lane) {
  const unsigned long long live = __ballot(act);
  if (!live) return;
  int first = -1;
  unsigned long long sm = 0;
  if (__popcll(live) >= COMBINE_MIN) {  // (wave-uniform, as everything decided from a ballot)
    first = __ffsll((long long)live) - 1;
    const int k = __builtin_amdgcn_readlane(idx, first);
    sm = __ballot(act && idx == k);
  }
  if (__popcll(sm) >= COMBINE_MIN) {
    const bool same = (sm >> lane) & 1;
    if (lane == first) atomicAdd(&bins[idx], val * (unsigned long long)__popcll(sm));
    else if (act && !same) atomicAdd(&bins[idx], val);
  } else if (act) {
    atomicAdd(&bins[idx], val);
  }
}

// below(x) of a contig whose m intervals start at ms / cl; m = 0 (a lane without a row) gives 0
__device__ __forceinline__ int rd_below(const int64_t* __restrict__ ms, const int2* __restrict__ cl, int m, int64_t x) {
  const int j = count_below<true>(ms, m, x);
  if (j == 0) return 0;
  const int2 c = cl[j - 1];
  const unsigned long long d = (unsigned long long)x - (unsigned long long)ms[j - 1];  // x >= ms >= 1: no wrap
  const unsigned long long top = (unsigned long long)(c.y - 1);
  return c.x + (int)(d < top ? d : top) + 1;
}

template <int THREADS, int TIER>
__global__ __launch_bounds__(THREADS) void k_region_set_depth(const Rows a, const RegionDepthTables t) {
  extern __shared__ __align__(16) unsigned char rd_lds[];
  __shared__ unsigned long long tot[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int NB = t.NB;
  unsigned long long* D = a.state + 4;
  const int64_t* ms = t.ms;
  const int2* cl = t.cl;
  if (TIER > 0) {  // [D: NB x 8] [ms: I x 8] [cl: I x 8]
    D = reinterpret_cast<unsigned long long*>(rd_lds);
    for (int i = tid; i < NB; i += THREADS) D[i] = 0;
  }
  if (TIER == 2) {
    int64_t* l_ms = reinterpret_cast<int64_t*>(rd_lds) + NB;
    int2* l_cl = reinterpret_cast<int2*>(l_ms + t.I);
    for (int i = tid; i < t.I; i += THREADS) {
      l_ms[i] = t.ms[i];
      l_cl[i] = t.cl[i];
    }
    ms = l_ms, cl = l_cl;
  }
  if (tid < 4) tot[tid] = 0;
  __syncthreads();

  walk<THREADS>(a, tot, [&](int32_t slot, int64_t s, int64_t e) {
    const bool hit = slot >= 0;
    int i0 = 0, m = 0, base = 0;
    if (hit) {
      i0 = t.ioff[slot];
      m = t.ioff[slot + 1] - i0;
      base = t.doff[slot];
    }
    const int lo = rd_below(ms + i0, cl + i0, m, s <= 1 ? 0 : s - 1);  // (no interval starts below 1)
    const int hi = rd_below(ms + i0, cl + i0, m, e);
    const bool add = hit && hi > lo;
    rd_add(D, base + lo, 1ull, add, lane);
    rd_add(D, base + hi, ~0ull, add, lane);
  });

  if (TIER > 0)  // the workgroup's non-zero bins, one global atomic each
    for (int i = tid; i < NB; i += THREADS)
      if (const unsigned long long v = D[i]) atomicAdd(&a.state[4 + i], v);
}

constexpr size_t rd_lds_bytes(int tier, const RegionDepthTables& t) { return tier == 0 ? 0 : (size_t)t.NB * 8 + (tier == 2 ? (size_t)t.I * 16 : 0); }

template <int THREADS, int TIER>
hipError_t rd_launch(hipStream_t s, const LaunchCfg& cfg, const Rows& a, const RegionDepthTables& t, int64_t span) {
  return launch<THREADS, k_region_set_depth<THREADS, TIER>>(s, cfg, a, t, span, rd_lds_bytes(TIER, t), REGION_DEPTH_LDS_MAX * 16);
}

// ---- the reduce ------------------------------------------------------------------------------------------------------------------------
constexpr int RT = REGION_DEPTH_REDUCE_TILE;
static_assert(RT == 256, "a tile is one wave, 4 bins a lane");

// the 4 bins of this lane in `tile` (0 beyond the section) as inclusive sums within the lane
__device__ __forceinline__ void rd_tile_load(const unsigned long long* __restrict__ D, int NB, int tile, int lane, unsigned long long d[4]) {
  const int b0 = tile * RT + lane * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) d[q] = b0 + q < NB ? D[b0 + q] : 0ull;
  d[1] += d[0], d[2] += d[1], d[3] += d[2];
}
__device__ __forceinline__ unsigned long long rd_wave_total(unsigned long long v) {  // the sum over the wave, in every lane
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// tsum[tile] = the sum of the tile's bins; a wave per tile
__global__ __launch_bounds__(256) void k_rd_tile_sums(const unsigned long long* __restrict__ D, int NB, int ntiles, unsigned long long* __restrict__ tsum) {
  const int lane = threadIdx.x & 63;
  for (int tile = blockIdx.x * 4 + (threadIdx.x >> 6); tile < ntiles; tile += gridDim.x * 4) {
    unsigned long long d[4];
    rd_tile_load(D, NB, tile, lane, d);
    const unsigned long long v = rd_wave_total(d[3]);
    if (lane == 0) tsum[tile] = v;
  }
}

// toff[tile] = the sum of the tiles in front of it; ONE workgroup: a run of tiles per thread, the threads' totals scanned in LDS
__global__ __launch_bounds__(1024) void k_rd_tile_scan(const unsigned long long* __restrict__ tsum, int ntiles, unsigned long long* __restrict__ toff) {
  __shared__ unsigned long long part[1024];
  const int tid = threadIdx.x, chunk = (ntiles + 1023) / 1024;
  const int lo = min(tid * chunk, ntiles), hi = min(lo + chunk, ntiles);
  unsigned long long s = 0;
  for (int i = lo; i < hi; ++i) s += tsum[i];
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const unsigned long long v = tid >= o ? part[tid - o] : 0ull;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  unsigned long long run = part[tid] - s;
  for (int i = lo; i < hi; ++i) {
    toff[i] = run;
    run += tsum[i];
  }
}

// a wave per piece: piece p belongs to region i = the last one with pfx[i] <= p and is its (p - pfx[i])-th tile
__global__ __launch_bounds__(256) void k_rd_pieces(const RegionDepthReduce r, const unsigned long long* __restrict__ D, const unsigned long long* __restrict__ toff,
                                                   unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int k = r.k;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < r.n_pieces; p += (int64_t)gridDim.x * 4) {
    const int i = count_below<true>(r.pfx, r.M, p) - 1;  // (pfx[0] = 0 <= p)
    const int lo = r.lo[i], hi = r.hi[i];
    const int tile = lo / RT + (int)(p - r.pfx[i]);
    unsigned long long d[4];
    rd_tile_load(D, r.NB, tile, lane, d);
    unsigned long long incl = d[3];  // inclusive scan of the lanes' totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    const unsigned long long base = toff[tile] + incl - d[3];
    const int b0 = tile * RT + lane * 4;
    unsigned long long bases = 0;
    unsigned ge[REGION_DEPTH_MAX_THRESHOLDS] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned long long depth = base + d[q];
      const bool in = b0 + q >= lo && b0 + q < hi;
      bases += in ? depth : 0ull;
#pragma unroll
      for (int t = 0; t < REGION_DEPTH_MAX_THRESHOLDS; ++t) ge[t] += in && t < k && (int64_t)depth >= r.thr[t];
    }
    unsigned long long* row = out + (int64_t)i * (1 + k);
    bases = rd_wave_total(bases);
    if (lane == 0 && bases) atomicAdd(&row[0], bases);
#pragma unroll
    for (int t = 0; t < REGION_DEPTH_MAX_THRESHOLDS; ++t) {
      if (t >= k) break;  // (wave-uniform)
      const unsigned long long g = rd_wave_total((unsigned long long)ge[t]);
      if (lane == 0 && g) atomicAdd(&row[1 + t], g);
    }
  }
}

}  // namespace

hipError_t launch_region_set_depth(hipStream_t s, const LaunchCfg& cfg, const uint8_t* ones, const int32_t* ref, const uint8_t* ref_valid,
                                   const int64_t* start, const uint8_t* start_valid, const int64_t* end, const uint8_t* end_valid, int64_t n,
                                   const RegionDepthTables& t, int64_t* d_state) {
  const Rows all{ref, ref_valid, start, start_valid, end, end_valid, ones, n, 0, 0, t.map, t.n_map, t.C, reinterpret_cast<unsigned long long*>(d_state)};
  // (a contig has an interval or more, an interval a base or more)
  const bool ok = !(t.C < 1 || t.I < t.C || (int64_t)t.NB < (int64_t)t.I + t.C || t.NB > REGION_DEPTH_MAX_BINS || t.n_map < 0);
  const int tier = region_depth_tier(t.NB, t.I);
  return run(s, cfg, all, region_depth_words(t.NB), ok, [&](bool big, const Rows& a, int64_t span) {
    if (tier == 2) return big ? rd_launch<1024, 2>(s, cfg, a, t, span) : rd_launch<256, 2>(s, cfg, a, t, span);
    if (tier == 1) return big ? rd_launch<1024, 1>(s, cfg, a, t, span) : rd_launch<256, 1>(s, cfg, a, t, span);
    return big ? rd_launch<1024, 0>(s, cfg, a, t, span) : rd_launch<256, 0>(s, cfg, a, t, span);
  });
}

hipError_t launch_region_depth_reduce(hipStream_t s, const LaunchCfg& cfg, const RegionDepthReduce& r, const int64_t* d_state, unsigned long long* scratch,
                                      int64_t* d_out) {
  if (r.M < 1 || r.NB < 1 || r.NB > REGION_DEPTH_MAX_BINS || r.k < 0 || r.k > REGION_DEPTH_MAX_THRESHOLDS || r.n_pieces < r.M) return hipErrorInvalidValue;
  hipError_t e;
  if ((e = hipMemsetAsync(d_out, 0, (size_t)r.M * (size_t)(1 + r.k) * 8, s)) != hipSuccess) return e;  // the pieces add
  const unsigned long long* D = reinterpret_cast<const unsigned long long*>(d_state) + 4;
  const int ntiles = (int)region_depth_reduce_tiles(r.NB);
  unsigned long long *tsum = scratch, *toff = scratch + ntiles;
  const int64_t resident = (int64_t)std::max(cfg.compute_units, 1) * 8;
  hipLaunchKernelGGL(k_rd_tile_sums, dim3((unsigned)std::min<int64_t>(resident, (ntiles + 3) / 4)), dim3(256), 0, s, D, r.NB, ntiles, tsum);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_rd_tile_scan, dim3(1), dim3(1024), 0, s, tsum, ntiles, toff);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_rd_pieces, dim3((unsigned)std::min<int64_t>(resident, (r.n_pieces + 3) / 4)), dim3(256), 0, s, r, D, toff,
                     reinterpret_cast<unsigned long long*>(d_out));
  return hipGetLastError();
}

}  // namespace exon
