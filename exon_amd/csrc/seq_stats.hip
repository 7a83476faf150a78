// seq_stats.hip -- K10 seq_stats_hist: per-record FASTA statistics (plan kind 10), a translation unit of its own so that
// kernels.o stays what it was.
//
//   State (include/exon_hip.h): [n_records, sum len, sum gc] [composition: 256] [length: lmax + 2] [length_log2: 32]
//   [gc_percent: 102]; every word adds.  gc = bytes equal to 'G' or 'C' (gc_content, exon-core/src/udfs/sequence/gc_content.rs:52-71),
//   the percent bin is the exact integer floor.
//
//   TWO INPUT FORMS, ONE ALGORITHM.  Both describe runs of sequence bytes inside one byte range of one buffer:
//     Arrow   record r is the run [off[r], off[r + 1]) of `values`; the range is [off[0], off[n]) (read on the device: a launch needs
//             nothing back from it)
//     views   (exon_hip_fasta_parser_parse) line l adds the run [begin_l, begin_l + line_dst[l + 1] - line_dst[l]) of text_base, which
//             is empty for definition and empty lines and leaves a CR out; record r reaches from its '>' to the next record's and its
//             length is seq_offsets[r + 1] - seq_offsets[r]; the range is [first_line_start, first_line_start + consumed_bytes)
//   Positions are taken from the 16-byte aligned address at or below the range's first byte ("x").
//
//   WORK IS DIVIDED BY SOURCE BYTES: the range is cut into tiles of SS_T bytes of x, workgroups take tiles grid-stride, and no loop
//   walks a record or a line: one 20 MB record and a million 50-byte records both give every workgroup the same tiles.  Per tile:
//     1. every lane loads 16-byte chunks (aligned; a chunk the range covers partly is read byte by byte, so NO byte outside the
//        range is loaded) and turns them into 16 G/C bits by K9's exact SWAR test; the bits of the tile sit in LDS
//     2. the tile's sequence-byte mask: Arrow -- the range; views -- the tile's lines (found by one binary search in line_end) toggle a
//        bit at each end of their run, a prefix XOR over the tile turns the toggles into the mask
//     3. a prefix sum of popcount(G/C & sequence) per 32-byte word makes the G/C count of ANY run inside the tile two LDS reads
//     4. composition: one ds_add_u32 per sequence byte into h[byte][lane & 31] -- every lane of a 32-lane half has its own copy, so
//        no two lanes of a half share an address or a bank, whatever the text is made of (DNA puts every byte on four values)
//     5. the records that START in the tile (one binary search in the offsets / the '>' positions): one that also ends in it is binned
//        here; one that leaves it ("spans": at most one per tile) adds its G/C count inside the tile to the tile's u32 slot, and the
//        one record that enters the tile from an earlier one adds its part to the slot of the tile that holds its start
//   k_seq_stats_span, one thread per tile, then bins the spanning record of every tile from its slot.  Workspace: one u32 per tile.
//   The histograms live in LDS across a workgroup's tiles and reach the state by one global atomic per nonzero word; u32 counters
//   cannot overflow: a launch covers less than 2 GiB.
#include <algorithm>

#include "kernels.h"

namespace exon {
namespace {

constexpr int SS_THREADS = 512;
constexpr int SS_WORDS = SS_T / 32;           // mask words of a tile: one per thread
constexpr int SS_CPT = SS_T / 16 / SS_THREADS;  // 16-byte chunks per thread and tile
constexpr int SS_LEN_LDS = 2048;              // length bins kept in LDS; the others are global atomics
static_assert(SS_WORDS == SS_THREADS, "one mask word per thread");

struct SSArgs {
  const uint8_t* bytes;  // Arrow: values; views: text_base
  int64_t n;             // records
  const int32_t* off;    // Arrow: [n + 1]
  // views
  const int32_t* head_start;
  const int32_t* seq_off;
  const uint32_t* line_end;
  const uint32_t* line_dst;
  int64_t n_lines, xb, xe;
  uint32_t seq_bytes;
  int lmax;
  unsigned* slots;            // [tiles]
  unsigned long long* state;
};

// where the sections start
__device__ __forceinline__ int ss_comp_at() { return 3; }
__device__ __forceinline__ int ss_len_at() { return 3 + 256; }
__device__ __forceinline__ int ss_log_at(int lmax) { return 3 + 256 + lmax + 2; }
__device__ __forceinline__ int ss_gc_at(int lmax) { return 3 + 256 + lmax + 2 + 32; }

// the byte range and the records of a launch, in x
template <bool V>
struct SSView {
  const uint8_t* base;  // x = 0: 16-byte aligned
  int64_t xb, xe, shift, n;
  const int32_t *off, *head, *seq_off;
  __device__ __forceinline__ explicit SSView(const SSArgs& a) {
    n = a.n, off = a.off, head = a.head_start, seq_off = a.seq_off;
    if (V) {
      base = a.bytes, xb = a.xb, xe = a.xe, shift = 0;
    } else {
      const int64_t b0 = a.off[0], b1 = max((int64_t)a.off[a.n], b0);
      const int64_t s = (int64_t)((reinterpret_cast<uintptr_t>(a.bytes) + (uintptr_t)b0) & 15);
      base = a.bytes + b0 - s, xb = s, xe = s + (b1 - b0), shift = s - b0;
    }
  }
  __device__ __forceinline__ int64_t tiles() const { return max((xe + SS_T - 1) / SS_T, (int64_t)1); }
  __device__ __forceinline__ int64_t raw_start(int64_t r) const { return V ? (int64_t)head[r] - 1 : (int64_t)off[r] + shift; }
  __device__ __forceinline__ int64_t start(int64_t r) const { return min(max(raw_start(r), xb), xe); }
  __device__ __forceinline__ int64_t len(int64_t r) const {
    return V ? max((int64_t)seq_off[r + 1] - seq_off[r], (int64_t)0) : max((int64_t)off[r + 1] - off[r], (int64_t)0);
  }
  // (clamped into the range: offsets that do not ascend bin nonsense, they do not reach outside the tile's bits)
  __device__ __forceinline__ int64_t end(int64_t r, int64_t s) const {
    const int64_t e = V ? (r + 1 < n ? (int64_t)head[r + 1] - 1 : xe) : s + len(r);
    return min(max(e, s), xe);
  }
  // first record whose start is at or behind th
  __device__ int64_t lower(int64_t th) const {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (raw_start(mid) < th) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  }
  // the records that start in tile t: [first, last)
  __device__ __forceinline__ int64_t first_of(int64_t t) const { return t == 0 ? 0 : lower(t * SS_T); }
  __device__ __forceinline__ int64_t last_of(int64_t t, int64_t n_tiles) const { return t == n_tiles - 1 ? n : lower((t + 1) * SS_T); }
};

// 16 bits: byte i of the chunk is 'C' or 'G' (K9's test: (x & 0xFB) ^ 0x43 is zero for exactly these two bytes)
__device__ __forceinline__ unsigned ss_gc_nibble(unsigned x) {
  const unsigned y = (x & 0xFBFBFBFBu) ^ 0x43434343u;
  const unsigned t = ((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y;  // bit 7 of a byte is clear <=> the byte of y is zero
  const unsigned h = (~t & 0x80808080u) >> 7;                // bits 0, 8, 16, 24
  return ((h * 0x00204081u) >> 21) & 0xFu;                   // gathered (the partial products share no bit)
}
__device__ __forceinline__ unsigned ss_gc16(uint4 v) {
  return ss_gc_nibble(v.x) | ss_gc_nibble(v.y) << 4 | ss_gc_nibble(v.z) << 8 | ss_gc_nibble(v.w) << 12;
}
__device__ __forceinline__ unsigned ss_ones(int64_t k) { return k <= 0 ? 0u : k >= 32 ? ~0u : (1u << (int)k) - 1u; }
// G/C bytes among the tile's sequence bytes in front of bit p (0 <= p <= SS_T; mg[SS_WORDS] = 0)
__device__ __forceinline__ unsigned ss_count(const unsigned* mg, const unsigned* pre, int p) {
  return pre[p >> 5] + __popc(mg[p >> 5] & ((1u << (p & 31)) - 1u));
}

struct SSBins {
  unsigned *hlen, *hlog, *hgc;  // LDS, or null: everything by global atomics
  unsigned long long* state;
  int lmax;
};
__device__ __forceinline__ void ss_bin(const SSBins& b, int64_t len, unsigned gc) {
  const int lb = len <= b.lmax ? (int)len : b.lmax + 1;
  const int kb = len ? 64 - __clzll((long long)len) : 0;
  const int gb = !len ? 101 : len < (1 << 24) ? (int)(100u * gc / (unsigned)len) : (int)(100ull * gc / (unsigned long long)len);
  if (b.hlen && lb < SS_LEN_LDS) atomicAdd(&b.hlen[lb], 1u);
  else atomicAdd(&b.state[ss_len_at() + lb], 1ull);
  if (b.hlen) {
    atomicAdd(&b.hlog[kb], 1u);
    atomicAdd(&b.hgc[gb], 1u);
  } else {
    atomicAdd(&b.state[ss_log_at(b.lmax) + kb], 1ull);
    atomicAdd(&b.state[ss_gc_at(b.lmax) + gb], 1ull);
  }
}

template <bool V>
__global__ __launch_bounds__(SS_THREADS) void k_seq_stats_main(const SSArgs a) {
  __shared__ unsigned comp[256 * 32];  // [byte][lane & 31]
  __shared__ unsigned hlen[SS_LEN_LDS], hlog[32], hgc[102];
  __shared__ unsigned mg[SS_WORDS + 1], ms[SS_WORDS], pre[SS_WORDS + 1];
  __shared__ unsigned wpar[SS_THREADS / 64], wsum[SS_THREADS / 64];
  __shared__ long long sh_first, sh_last, sh_line;
  const SSView<V> v(a);
  const int64_t n_tiles = v.tiles();
  if ((int64_t)blockIdx.x >= n_tiles) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 256 * 32; i += SS_THREADS) comp[i] = 0;
  for (int i = tid; i < SS_LEN_LDS; i += SS_THREADS) hlen[i] = 0;
  if (tid < 32) hlog[tid] = 0;
  if (tid < 102) hgc[tid] = 0;
  if (tid == 0) mg[SS_WORDS] = 0;
  __syncthreads();
  const SSBins bins{hlen, hlog, hgc, a.state, a.lmax};
  unsigned short* const mg16 = reinterpret_cast<unsigned short*>(mg);
  const unsigned short* const ms16 = reinterpret_cast<const unsigned short*>(ms);
  unsigned* const my = comp + (lane & 31);
  unsigned long long t_rec = 0, t_len = 0, t_gc = 0;

  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t ts = tile * SS_T, te = ts + SS_T;
    // ---- the tile's records and lines; the bytes; their G/C bits
    if (tid == 0) sh_first = v.first_of(tile);
    if (tid == 64) sh_last = v.last_of(tile, n_tiles);
    if (V && tid == 128) {
      int64_t lo = 0, hi = a.n_lines;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)a.line_end[mid] < ts) lo = mid + 1;
        else hi = mid;
      }
      sh_line = lo;
    }
    if (V) ms[tid] = 0;
    uint4 d[SS_CPT];
#pragma unroll
    for (int k = 0; k < SS_CPT; ++k) {
      const int c = tid + k * SS_THREADS;
      const int64_t cx = ts + 16 * c;
      if (cx >= v.xb && cx + 16 <= v.xe) {
        d[k] = *reinterpret_cast<const uint4*>(v.base + cx);
      } else {  // a chunk the range covers partly (its first and its last) or not at all: byte by byte, nothing outside
        unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (cx + i >= v.xb && cx + i < v.xe) w[i >> 2] |= (unsigned)v.base[cx + i] << (8 * (i & 3));
        d[k] = make_uint4(w[0], w[1], w[2], w[3]);
      }
      mg16[c] = (unsigned short)ss_gc16(d[k]);  // (bytes outside the range are zero: no G, no C)
    }
    __syncthreads();
    // ---- the sequence mask
    unsigned x;
    if (V) {
      for (int64_t l = sh_line + tid; l < a.n_lines; l += SS_THREADS) {
        const int64_t begin = l ? (int64_t)a.line_end[l - 1] + 1 : v.xb;
        const uint32_t d0 = a.line_dst[l];
        if (begin >= te || begin >= v.xe || d0 >= a.seq_bytes) break;  // behind the tile, or a line of the record that stays behind
        const int64_t lo = max(begin, ts), hi = min(min(begin + (int64_t)(a.line_dst[l + 1] - d0), te), v.xe);
        if (lo < hi) {
          atomicXor(&ms[(lo - ts) >> 5], 1u << ((lo - ts) & 31));
          if (hi < te) atomicXor(&ms[(hi - ts) >> 5], 1u << ((hi - ts) & 31));
        }
      }
      __syncthreads();
      x = ms[tid];  // bit i := XOR of the toggles at or below i
      x ^= x << 1, x ^= x << 2, x ^= x << 4, x ^= x << 8, x ^= x << 16;
      const unsigned long long odd = __ballot(x >> 31);
      if (__popcll(odd & ((1ull << lane) - 1ull)) & 1) x = ~x;
      if (lane == 0) wpar[wave] = __popcll(odd) & 1;
      __syncthreads();
      unsigned carry = 0;
      for (int w = 0; w < wave; ++w) carry ^= wpar[w];
      if (carry) x = ~x;
      ms[tid] = x;
    } else {
      const int64_t w0 = ts + 32 * tid;
      x = ss_ones(v.xe - w0) & ~ss_ones(v.xb - w0);
      ms[tid] = x;
    }
    // ---- G/C among the sequence bytes, and its prefix sums
    const unsigned m = mg[tid] & x;
    mg[tid] = m;
    unsigned inc = __popc(m);
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
      const unsigned o = __shfl_up(inc, dlt);
      if (lane >= dlt) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    pre[tid] = before + inc - __popc(m);
    if (tid == SS_THREADS - 1) pre[SS_WORDS] = before + inc;
    __syncthreads();
    // ---- composition: one LDS add per sequence byte, lane-private copies
#pragma unroll
    for (int k = 0; k < SS_CPT; ++k) {
      const unsigned sm = ms16[tid + k * SS_THREADS];
      const unsigned w[4] = {d[k].x, d[k].y, d[k].z, d[k].w};
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (sm >> i & 1) atomicAdd(&my[((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) << 5], 1u);
    }
    // ---- the records that start here
    const int64_t r_first = sh_first, r_last = sh_last;
    for (int64_t r = r_first + tid; r < r_last; r += SS_THREADS) {
      const int64_t s = v.start(r), e = v.end(r, s), len = v.len(r);
      const int p0 = (int)min(max(s - ts, (int64_t)0), (int64_t)SS_T), p1 = (int)min(max(e - ts, (int64_t)p0), (int64_t)SS_T);
      const unsigned gc = ss_count(mg, pre, p1) - ss_count(mg, pre, p0);
      if (e > te) {  // spans tiles: k_seq_stats_span bins it
        atomicAdd(&a.slots[tile], gc);
      } else {
        ss_bin(bins, len, gc);
        t_rec += 1, t_len += (unsigned long long)len, t_gc += gc;
      }
    }
    // ---- the record that enters from an earlier tile: its part goes to the slot of the tile of its start
    if (tid == 0 && tile > 0 && r_first > 0) {
      const int64_t r = r_first - 1, s = v.start(r), e = v.end(r, s);
      if (s < ts && e > ts) atomicAdd(&a.slots[s / SS_T], ss_count(mg, pre, (int)(min(e, te) - ts)));
    }
    __syncthreads();  // (the masks are the next tile's)
  }

#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    t_rec += __shfl_down(t_rec, dlt);
    t_len += __shfl_down(t_len, dlt);
    t_gc += __shfl_down(t_gc, dlt);
  }
  if (lane == 0 && t_rec) {
    atomicAdd(&a.state[0], t_rec);
    atomicAdd(&a.state[1], t_len);
    atomicAdd(&a.state[2], t_gc);
  }
  // thread i adds 16 copies of byte i / 2; the pair's sum goes out
  {
    unsigned sum = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum += comp[tid * 16 + i];
    sum += __shfl_xor(sum, 1);
    if (!(tid & 1) && sum) atomicAdd(&a.state[ss_comp_at() + (tid >> 1)], (unsigned long long)sum);
  }
  const int n_len = min(a.lmax + 2, SS_LEN_LDS);
  for (int i = tid; i < n_len; i += SS_THREADS)
    if (const unsigned c = hlen[i]) atomicAdd(&a.state[ss_len_at() + i], (unsigned long long)c);
  if (tid < 32 && hlog[tid]) atomicAdd(&a.state[ss_log_at(a.lmax) + tid], (unsigned long long)hlog[tid]);
  if (tid < 102 && hgc[tid]) atomicAdd(&a.state[ss_gc_at(a.lmax) + tid], (unsigned long long)hgc[tid]);
}

// one thread per tile: the record that starts in the tile and leaves it (the last one that starts there, if any does)
template <bool V>
__global__ __launch_bounds__(256) void k_seq_stats_span(const SSArgs a) {
  const SSView<V> v(a);
  const int64_t n_tiles = v.tiles(), tile = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (tile >= n_tiles) return;
  const int64_t r = v.last_of(tile, n_tiles) - 1;
  if (r < 0 || r < v.first_of(tile)) return;
  const int64_t s = v.start(r), e = v.end(r, s);
  if (e <= (tile + 1) * SS_T) return;
  const int64_t len = v.len(r);
  const unsigned gc = a.slots[tile];
  ss_bin(SSBins{nullptr, nullptr, nullptr, a.state, a.lmax}, len, gc);
  atomicAdd(&a.state[0], 1ull);
  atomicAdd(&a.state[1], (unsigned long long)len);
  atomicAdd(&a.state[2], (unsigned long long)gc);
}

template <bool V>
hipError_t ss_launch(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, SSArgs a, int64_t max_tiles) {
  if (!ws.partials || ws.partial_capacity * 8 < (size_t)max_tiles * 4) return hipErrorInvalidValue;
  a.slots = reinterpret_cast<unsigned*>(ws.partials);
  hipError_t e;
  if ((e = hipMemsetAsync(a.slots, 0, (size_t)max_tiles * 4, s)) != hipSuccess) return e;
  const int grid = (int)std::min<int64_t>(max_tiles, (int64_t)cfg.compute_units * 3);  // three workgroups of this LDS size fit a CU
  hipLaunchKernelGGL(k_seq_stats_main<V>, dim3(grid), dim3(SS_THREADS), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_seq_stats_span<V>, dim3((unsigned)((max_tiles + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

size_t seq_stats_partial_words() { return ((size_t)SS_MAX_TILES * 4 + 7) / 8; }

hipError_t launch_seq_stats_hist(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const uint8_t* values, const int32_t* offsets,
                                 int64_t n_records, int lmax, int64_t* d_state) {
  if (lmax < 1 || lmax > 65536) return hipErrorInvalidValue;
  hipError_t e;
  if (cfg.overwrite && (e = hipMemsetAsync(d_state, 0, (size_t)seq_stats_words(lmax) * 8, s)) != hipSuccess) return e;  // the kernels add
  // the payload's size is known on the device alone: every tile an int32-offset payload can have gets its slot
  for (int64_t r = 0; r < n_records; r += (int64_t)1 << 31) {
    SSArgs a{};
    a.bytes = values, a.off = offsets + r;
    a.n = std::min<int64_t>(n_records - r, (int64_t)1 << 31);
    a.lmax = lmax;
    a.state = reinterpret_cast<unsigned long long*>(d_state);
    if ((e = ss_launch<false>(s, cfg, ws, a, SS_MAX_TILES)) != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_seq_stats_hist_views(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const uint8_t* text_base, int64_t first_line_start,
                                       int64_t consumed_bytes, int64_t n_records, int64_t n_lines, int64_t seq_bytes, const int32_t* head_start,
                                       const int32_t* seq_offsets, const uint32_t* line_end, const uint32_t* line_dst, int lmax, int64_t* d_state) {
  if (lmax < 1 || lmax > 65536 || first_line_start < 0 || consumed_bytes < 0 || first_line_start + consumed_bytes > ((int64_t)1 << 31) ||
      (reinterpret_cast<uintptr_t>(text_base) & 15))
    return hipErrorInvalidValue;
  hipError_t e;
  if (cfg.overwrite && (e = hipMemsetAsync(d_state, 0, (size_t)seq_stats_words(lmax) * 8, s)) != hipSuccess) return e;
  if (n_records <= 0) return hipSuccess;
  SSArgs a{};
  a.bytes = text_base, a.n = n_records;
  a.head_start = head_start, a.seq_off = seq_offsets, a.line_end = line_end, a.line_dst = line_dst;
  a.n_lines = n_lines, a.xb = first_line_start, a.xe = first_line_start + consumed_bytes;
  a.seq_bytes = (uint32_t)seq_bytes;
  a.lmax = lmax;
  a.state = reinterpret_cast<unsigned long long*>(d_state);
  return ss_launch<true>(s, cfg, ws, a, std::max<int64_t>((a.xe + SS_T - 1) / SS_T, 1));
}

}  // namespace exon
