// window_bases.hip -- K13 window_bases: the bases of the rows that fall inside every fixed-width window along each contig, in one pass
// over the rows (plan kind 13), a translation unit of its own as K11 and K12 are.
//
//   WHAT IS SUMMED.  Rows are 1-based inclusive, as in K6 / K11 / K12.  Contig c of length L_c is cut into K_c = ceil(L_c / W) windows,
//   window j = [j * W + 1, min((j + 1) * W, L_c)].  A counted row [s, e] is clipped to [1, L_c]; a row wholly outside (s > L_c or
//   e < 1) stays counted and adds nothing.  bases_j is the sum over the counted rows of the bases of the clipped row inside window j.
//   The alignment span counts as covered, as in K12.
//
//   THE STATE ADDS.  With js = (s - 1) / W and je = (e - 1) / W of the clipped row:
//       js == je:      E[js] += e - s + 1                                   one add: the common case, reads shorter than windows
//       otherwise:     E[js] += (js + 1) * W - s + 1,  E[je] += e - je * W   the partly covered windows at both ends
//       je > js + 1:   D[js + 1] += 1,  D[je] -= 1                           the windows in between are covered whole
//   and bases_j = E[j] + W * (D[0] + ... + D[j]) per contig: a window strictly between two others is never a contig's short last
//   window, so the factor is W.  Every word is unsigned 64-bit arithmetic MODULO 2^64 (the -1 is an add of 2^64 - 1).
//
//   State: [counted, null_rows, elsewhere, inverted] [E: B] [D: B]; contig c owns bins [woff[c], woff[c + 1]) of each section.
//
//   THE WINDOW OF A COORDINATE is a division by a number the whole launch shares: x - 1 < 2^31, so floor((x - 1) / W) is one
//   32 x 32 -> 64 bit multiply by a reciprocal the host made and a shift (kernels.h, window_bases_reciprocal) -- exact, no search, no
//   64-bit divide, and no 32-bit divide either (about ten instructions more a quotient; measured 5 - 6 % slower in the LDS tier,
//   profiles/window_bases.md).
//
//   TWO TIERS, chosen per plan.  B <= WINDOW_BASES_LDS_MAX: E and D sit in LDS as u64 (ds_add_u64), and the workgroup adds its non-zero
//   bins to the state with one global atomic each.  Beyond: every add is a global 64-bit atomic on the state.  In both, the lanes of a
//   wave that hit the bin of the wave's first live lane are combined once there are 16 of them (region_rows.h: wave_sum, COMBINE_MIN):
//   a coordinate-sorted file sends whole waves to one E bin.
//
//   ROWS.  region_rows.h walks them (shared with K11 and K12).  This file holds what a row ADDS.
#include "region_rows.h"

namespace exon {
namespace {

using namespace region_rows;

// bins[idx] += val (modulo 2^64) for every lane with `act`; COMBINE_MIN lanes or more on the bin of the wave's first live lane become
// one add of the sum of their values.  Called by whole waves.
__device__ __forceinline__ void wb_add(unsigned long long* bins, int idx, unsigned long long val, bool act, int lane) {
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
    const unsigned long long tot = wave_sum(same ? val : 0ull);
    if (lane == first) atomicAdd(&bins[idx], tot);
    else if (act && !same) atomicAdd(&bins[idx], val);
  } else if (act) {
    atomicAdd(&bins[idx], val);
  }
}

template <int THREADS, bool LDS>
__global__ __launch_bounds__(THREADS) void k_window_bases(const Rows a, const WindowBasesTables t) {
  extern __shared__ __align__(16) unsigned char wb_lds[];
  __shared__ unsigned long long tot[4];
  const int tid = threadIdx.x, lane = tid & 63;
  const int B = t.B;
  unsigned long long *E, *D;
  if (LDS) {  // [E: B x 8] [D: B x 8], the state's order
    E = reinterpret_cast<unsigned long long*>(wb_lds);
    D = E + B;
    for (int i = tid; i < 2 * B; i += THREADS) E[i] = 0;
  } else {
    E = a.state + 4;
    D = a.state + 4 + (int64_t)B;
  }
  if (tid < 4) tot[tid] = 0;
  __syncthreads();

  const uint32_t W = t.W, mul = t.mul, shift = t.shift;
  walk<THREADS>(a, tot, [&](int32_t slot, int64_t s, int64_t e) {
    bool hit = slot >= 0;
    int base = 0;
    int64_t L = 1;
    if (hit) {
      base = t.woff[slot];
      L = t.len[slot];
    }
    s = s < 1 ? 1 : s;  // clipped to [1, L]: both are in [1, 2^31 - 1] from here on if the row touches the contig at all
    e = e > L ? L : e;
    hit = hit && s <= e;
    const uint32_t x0 = hit ? (uint32_t)(s - 1) : 0u, x1 = hit ? (uint32_t)(e - 1) : 0u;
    const uint32_t js = (uint32_t)((uint64_t)x0 * mul >> shift), je = (uint32_t)((uint64_t)x1 * mul >> shift);
    const bool one = js == je;
    const unsigned long long head = one ? (unsigned long long)(x1 - x0) + 1 : (unsigned long long)(js + 1) * W - x0;
    wb_add(E, base + (int)js, head, hit, lane);
    wb_add(E, base + (int)je, (unsigned long long)x1 + 1 - (unsigned long long)je * W, hit && !one, lane);
    const bool mid = hit && je > js + 1;
    wb_add(D, base + (int)js + 1, 1ull, mid, lane);
    wb_add(D, base + (int)je, ~0ull, mid, lane);
  });

  if (LDS)  // the workgroup's non-zero bins, one global atomic each
    for (int i = tid; i < 2 * B; i += THREADS)
      if (const unsigned long long v = E[i]) atomicAdd(&a.state[4 + i], v);
}

template <int THREADS, bool LDS>
hipError_t wb_launch(hipStream_t s, const LaunchCfg& cfg, const Rows& a, const WindowBasesTables& t, int64_t span) {
  return launch<THREADS, k_window_bases<THREADS, LDS>>(s, cfg, a, t, span, LDS ? (size_t)t.B * 16 : 0, WINDOW_BASES_LDS_MAX * 16);
}

}  // namespace

hipError_t launch_window_bases(hipStream_t s, const LaunchCfg& cfg, const uint8_t* ones, const int32_t* ref, const uint8_t* ref_valid,
                               const int64_t* start, const uint8_t* start_valid, const int64_t* end, const uint8_t* end_valid, int64_t n,
                               const WindowBasesTables& t, int64_t* d_state) {
  const Rows all{ref, ref_valid, start, start_valid, end, end_valid, ones, n, 0, 0, t.map, t.n_map, t.C, reinterpret_cast<unsigned long long*>(d_state)};
  uint32_t mul = 0, shift = 0;
  if (t.W >= 1 && t.W < (1u << 31)) window_bases_reciprocal(t.W, &mul, &shift);
  // (a contig has one window or more; the reciprocal is the one this W has)
  const bool ok = !(t.C < 1 || t.B < t.C || t.B > WINDOW_BASES_MAX_BINS || t.n_map < 0 || t.W < 1 || t.W >= (1u << 31) || mul != t.mul || shift != t.shift);
  const bool lds = t.B <= WINDOW_BASES_LDS_MAX;
  return run(s, cfg, all, window_bases_words(t.B), ok, [&](bool big, const Rows& a, int64_t span) {
    if (lds) return big ? wb_launch<1024, true>(s, cfg, a, t, span) : wb_launch<256, true>(s, cfg, a, t, span);
    return big ? wb_launch<1024, false>(s, cfg, a, t, span) : wb_launch<256, false>(s, cfg, a, t, span);
  });
}

}  // namespace exon
