// gpu_parse.hip -- VCF record parsing ON THE GPU: raw text in HBM -> device-layout columns in HBM.
//
// The host decoders (host/formats.h, host/parallel.h) top out at ~150 Mrows/s on the GPU boxes' 16-CPU quota while the
// filter+aggregate kernels consume 500 000 Mrows/s; text crossing PCIe as-is and being parsed on the device lifts
// the decode stage to the PCIe rate ("GPU-side parse later").  Semantics are those of
// LazyVCFArrayBuilder::append (exon-vcf/src/array_builder/lazy_array_builder.rs:159-216) restricted to the columns
// of the device layout: chrom -> dictionary id, pos (0 / '.' -> NULL), qual ('.' -> NULL, correctly rounded f32),
// filter -> dictionary id of the ';'-joined list ('.' -> empty list), one typed INFO field (Number=1 Float/Integer,
// missing key / '.' -> NULL).
//
// Pipeline for one slab of complete lines:
//   k_index_lines      positions of all newlines, in order (line i = (nl[i-1], nl[i])), in ONE pass: decoupled look-back over
//                      the tiles' counts (LineIndex, shared with the FASTQ and SAM parsers below)
//   k_parse_lines      one thread per line: split on tabs, parse, look names up in hash tables, ballot the validity
//                      bitmaps; FILTER lists not seen before are inserted with atomicCAS (slot = provisional id)
//   k_assign_filters   dense ids for newly inserted FILTER lists, their text copied to a persistent pool
//   k_remap_filters    provisional slot -> dense id; every row's text is compared with its key's text in the pool (a 64-bit
//                      hash match of two different texts sets the table's overflow flag: the slab goes to the host reader)
// Rows the device cannot decide (a float with > 19 significant digits, a contig missing from the header, a malformed
// line) are counted; the caller then re-decodes that slab on the host, so results never differ from the CPU path.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "host/decimal_f32.h"
#include "internal.h"
#include "list_kernels.h"

namespace {

constexpr int TPB = 256;
constexpr int FILTER_SLOTS = 8192;  // open addressing; at most EXON_HIP_MAX_GROUPS distinct lists are supported
constexpr int FILTER_POOL = EXON_DICT_POOL;

__host__ __device__ inline uint64_t fnv1a(const uint8_t* p, int n) {
  uint64_t h = 0xCBF29CE484222325ULL;
  for (int i = 0; i < n; ++i) {
    h ^= p[i];
    h *= 0x100000001B3ULL;
  }
  return h | 1ULL;  // never 0 (0 = empty slot)
}

__device__ __forceinline__ int count_nl16(uint4 v) {
  int c = 0;
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c += ((w[i] & 0xFF) == 0x0A) + (((w[i] >> 8) & 0xFF) == 0x0A) + (((w[i] >> 16) & 0xFF) == 0x0A) + ((w[i] >> 24) == 0x0A);
  }
  return c;
}

// `text` is 16-byte aligned; the slab proper starts `skip` (< 16) bytes into it: those bytes read as zeros
__device__ __forceinline__ uint4 load16(const uint8_t* text, int64_t n, int64_t off, unsigned skip) {
  uint4 v = {0, 0, 0, 0};
  unsigned* w = &v.x;
  if (off + 16 <= n) {
    v = *reinterpret_cast<const uint4*>(text + off);
  } else {
    for (int i = 0; i < 16 && off + i < n; ++i) w[i >> 2] |= (unsigned)text[off + i] << (8 * (i & 3));
  }
  if (off == 0 && skip) {
    for (unsigned i = 0; i < skip; ++i) w[i >> 2] &= ~(0xFFu << (8 * (i & 3)));
  }
  return v;
}

// ---- the line index in ONE pass over the text (round 5) -------------------------------------------------------------------------
// A workgroup takes its tile off a counter (so tile t runs only after tiles 0 .. t-1 have started), counts its newlines, publishes
// the count, finds the number of newlines in front of its tile by looking BACK over its predecessors' published words -- a word is
// (generation, value, flag): flag 1 = the tile's own count, flag 2 = the count of everything up to and including the tile; a wave
// reads 64 predecessors at a time and stops at the first "inclusive" word -- and writes the positions of its newlines.  Decoupled
// look-back; the words are written and read with agent-scope atomics (the 8 XCDs do not share an L2), the generation makes last
// slab's words read as "not there yet" (no clearing pass), and the counter wraps to 0 by itself (atomicInc).  A look-back that does
// not see its predecessor within LOOKBACK_SPINS reads gives up, poisons its own word (the tiles behind it give up at once) and marks
// the slab "one undecided record": the host decoder takes it -- a hang is not possible.  (Rounds 1-4 counted, scanned and filled in
// three launches that read the slab twice.)
constexpr unsigned LOOKBACK_SPINS = 1u << 22;
__device__ __forceinline__ void st_agent_u64(unsigned long long* p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ld_agent_u64(const unsigned long long* p) {
  return __hip_atomic_load(const_cast<unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Tiles are 64 KiB (1024 threads x 64 bytes): the look-back advances 64 tiles per round trip through the L2 atomics (~1 us), so with
// the 16 KiB tiles of the first version a 516 MB slab's 31.5 k tiles took 0.47 ms -- 1.1 TB/s, bound by the chain, not by HBM.
#ifndef EXON_IDX_TPB
#define EXON_IDX_TPB 1024
#endif
#ifndef EXON_IDX_BPT
#define EXON_IDX_BPT 64
#endif
constexpr int IDX_TPB = EXON_IDX_TPB, IDX_BPT = EXON_IDX_BPT;
__global__ __launch_bounds__(IDX_TPB) void k_index_lines(const uint8_t* __restrict__ text, int64_t n, unsigned skip, unsigned long long* __restrict__ words,
                                                         unsigned* __restrict__ tile_ctr, unsigned nblocks, unsigned gen, unsigned* __restrict__ nl_pos,
                                                         unsigned cap, unsigned* __restrict__ scalars) {
  constexpr int TPB = IDX_TPB, BYTES_PER_THREAD = IDX_BPT;  // (this kernel's own tile: shadows the other kernels' TPB)
  __shared__ unsigned wave_tot[TPB / 64];
  __shared__ unsigned s_tile, s_prefix, s_bad;
  if (threadIdx.x == 0) {
    s_tile = atomicInc(tile_ctr, nblocks - 1u);
    s_bad = 0;
  }
  __syncthreads();
  const unsigned tile = s_tile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t off = ((int64_t)tile * TPB + threadIdx.x) * BYTES_PER_THREAD;
  constexpr int Q = BYTES_PER_THREAD / 16;
  uint4 v[Q];
  unsigned c = 0;
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    v[j] = uint4{0, 0, 0, 0};
    if (off + 16 * j < n) {
      v[j] = load16(text, n, off + 16 * j, skip);
      c += (unsigned)count_nl16(v[j]);
    }
  }
  unsigned incl = c;  // inclusive scan within the wave
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  unsigned T = 0;
#pragma unroll
  for (int w = 0; w < TPB / 64; ++w) T += wave_tot[w];
  const unsigned long long g = (unsigned long long)(gen & 0x3FFFFFFFu) << 34;
  if (wave == 0) {
    if (lane == 0) st_agent_u64(&words[tile], g | ((unsigned long long)T << 2) | (tile == 0 ? 2ull : 1ull));
    unsigned prefix = 0;
    bool bad = false;
    if (tile != 0) {
      for (int64_t j0 = (int64_t)tile - 1;; j0 -= 64) {
        const int64_t j = j0 - lane;
        unsigned long long w = 0;
        if (j >= 0) {
          unsigned spins = 0;
          do {
            w = ld_agent_u64(&words[j]);
          } while (((w >> 34) != (g >> 34) || (w & 3ull) == 0) && ++spins < LOOKBACK_SPINS);
          if ((w >> 34) != (g >> 34) || (w & 3ull) == 0 || (w & 3ull) == 3ull) bad = true;  // (3: a predecessor gave up)
        }
        if (__any(bad)) {
          bad = true;
          break;
        }
        const unsigned long long incl_lanes = __ballot(j >= 0 && (w & 3ull) == 2ull);
        const int first = incl_lanes ? __ffsll((long long)incl_lanes) - 1 : 64;
        unsigned add = (j >= 0 && lane <= first) ? (unsigned)(w >> 2) : 0u;
        for (int o = 32; o > 0; o >>= 1) add += __shfl_xor(add, o, 64);
        prefix += add;
        if (incl_lanes || j0 < 64) break;
      }
    }
    if (lane == 0) {
      s_prefix = prefix;
      s_bad = bad ? 1u : 0u;
      if (bad) st_agent_u64(&words[tile], g | 3ull);  // the tiles behind this one give up at once
      else if (tile != 0) st_agent_u64(&words[tile], g | ((unsigned long long)(prefix + T) << 2) | 2ull);
    }
  }
  __syncthreads();
  if (s_bad) {
    // no lines, one undecided record: the kernels behind do nothing, the caller hands the slab to the host decoder.  The verdict
    // is STICKY in tile_ctr[1] (= this launch's generation; no tile ever clears it): a tile further on may have read this tile's
    // aggregate before it gave up, finish its look-back, and -- as the last tile -- publish a total and zero scalars[1..3] AFTER
    // the two stores below.  k_index_verdict, ordered behind this kernel, re-applies the verdict from the sticky word.
    if (threadIdx.x == 0) {
      atomicExch(&tile_ctr[1], gen);
      scalars[0] = 0;
      scalars[1] = 1;
    }
    return;
  }
  unsigned base = s_prefix;
  for (int w = 0; w < wave; ++w) base += wave_tot[w];
  unsigned k = base + incl - c;
  if (c) {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const unsigned w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
      if ((w[0] | w[1] | w[2] | w[3]) == 0) continue;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (((w[i >> 2] >> (8 * (i & 3))) & 0xFF) == 0x0A) {
          if (k < cap) nl_pos[k] = (unsigned)(off + 16 * j + i);
          ++k;
        }
    }
  }
  // the last tile in tile order holds the total; it also clears words 1..3 of the slab's scalar block {lines, exceptions,
  // consumed, -}, which only the kernels BEHIND this one add to (no 16-byte memset per slab)
  if (tile == nblocks - 1u && threadIdx.x < 4) {
    if (threadIdx.x == 0) scalars[0] = s_prefix + T;
    else scalars[threadIdx.x] = 0;
  }
}
// behind k_index_lines on the same stream: a tile that gave up wins over whatever the last tile published
__global__ void k_index_verdict(const unsigned* __restrict__ tile_ctr, unsigned gen, unsigned* __restrict__ scalars) {
  if (tile_ctr[1] == gen) {
    scalars[0] = 0;
    scalars[1] = 1;
  }
}

// The line index of the VCF, FASTQ and SAM parsers: k_index_lines' look-back words (one per tile, then the tile counter and the
// sticky verdict word), the newline positions, the slab's scalars {lines, undecided, consumed bytes, -} and their pinned mirror.
struct LineIndex {
  static constexpr int64_t TILE_BYTES = (int64_t)IDX_TPB * IDX_BPT;
  unsigned long long* words = nullptr;
  unsigned* nl = nullptr;
  unsigned* d_scalars = nullptr;
  unsigned* h_scalars = nullptr;
  int64_t max_bytes = 0;
  unsigned tiles = 0, cap = 0, gen = 0;  // cap: newlines `nl` holds

  void alloc(PoolBufs& b, int64_t max_bytes_, int64_t max_lines) {
    max_bytes = max_bytes_;
    tiles = (unsigned)((max_bytes + TILE_BYTES - 1) / TILE_BYTES);
    cap = (unsigned)max_lines;
    words = b.take<unsigned long long>(((size_t)tiles + 1) * 8, 0);  // (zero: no word of any generation, the tile counter at 0)
    nl = b.take<unsigned>((size_t)max_lines * 4);
    d_scalars = b.take<unsigned>(16);
    h_scalars = b.pinned<unsigned>(16);
  }
  // the kernels read aligned 16-byte groups: start at the aligned address at or below the slab and ignore the `skip` bytes before it
  int align(exon_hip_ctx* ctx, const uint8_t** text, int64_t* n_bytes, unsigned* skip) const {
    *skip = (unsigned)(reinterpret_cast<uintptr_t>(*text) & 15);
    *text -= *skip;
    *n_bytes += *skip;
    if (*n_bytes > max_bytes) return fail(ctx, EXON_HIP_EINVAL, "slab of %lld bytes exceeds the parser's %lld", (long long)*n_bytes, (long long)max_bytes);
    return EXON_HIP_OK;
  }
  void launch(hipStream_t s, const uint8_t* text, int64_t n_bytes, unsigned skip) {
    gen = (gen + 1u) & 0x3FFFFFFFu;
    if (gen == 0) gen = 1;
    const unsigned ntiles = (unsigned)std::max<int64_t>(1, (n_bytes + TILE_BYTES - 1) / TILE_BYTES);  // (<= tiles: the words fit)
    unsigned* tile_ctr = reinterpret_cast<unsigned*>(words + tiles);
    hipLaunchKernelGGL(k_index_lines, dim3(ntiles), dim3(IDX_TPB), 0, s, text, n_bytes, skip, words, tile_ctr, ntiles, gen, nl, cap, d_scalars);
    hipLaunchKernelGGL(k_index_verdict, dim3(1), dim3(1), 0, s, tile_ctr, gen, d_scalars);
  }
  // the scalars, once everything queued on `s` has run
  int read_back(exon_hip_ctx* ctx, hipStream_t s) {
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_scalars, d_scalars, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return EXON_HIP_OK;
  }
  int64_t consumed(unsigned skip) const { return h_scalars[2] > skip ? (int64_t)h_scalars[2] - skip : 0; }
};

// scalars[2] = bytes up to and including the last newline (what a caller may discard after this slab)
__global__ void k_last_newline(const unsigned* __restrict__ nl_pos, unsigned* __restrict__ scalars, unsigned cap) {
  const unsigned n = scalars[0];
  scalars[2] = (n && n <= cap) ? nl_pos[n - 1] + 1u : 0u;
}

struct NameTable {  // open-addressing table of strings (contigs): hash -> id, text verified
  const uint64_t* keys;
  const int32_t* ids;
  const uint32_t* text_off;
  const uint32_t* text_len;
  const uint8_t* pool;
  int mask;
};

struct FilterTable {
  unsigned long long* keys;  // 0 = empty
  int32_t* ids;              // -1 until k_assign_filters has run
  uint32_t* text_off;        // provisional: offset into the CURRENT slab; after assignment: offset into pool
  uint32_t* text_len;
  uint8_t* pool;
  int32_t* counters;  // [0] = ids claimed, [1] = pool bytes claimed, [2] = overflow (or hash collision) flag, [3] = rows without a value
};

constexpr int MAX_INFO = EXON_HIP_MAX_INFO_FIELDS;  // 16: the by-value key table below is 16 x 9 bytes of kernel arguments
// the typed INFO fields a parser extracts (InfosBuilder children: exon-vcf/src/array_builder/info_builder.rs:152-309):
// kind 'f' = Number=1 Float -> f32 + validity; 'i' = Number=1 Integer -> i32 + validity (the 4-byte column holds the bit
// pattern); 'b' = Flag -> presence bitmap (value true where valid); 'F' / 'I' = any other Number of Float / Integer ->
// List<f32> / List<i32> (info_builder.rs:258-305): k_parse_lines records where the value text is and how many items it has,
// k_list_fill parses the items behind an exclusive scan of the counts (offsets), k_pack_bits turns the per-item flags
// into the child validity bitmap.  info_valid[q] is the LIST validity (NULL list: key absent, `key=.`, INFO '.')
struct InfoKeys {
  int n;
  int len[MAX_INFO];
  int off[MAX_INFO];  // into `text`
  char kind[MAX_INFO];
  const uint8_t* text;
};
struct ParseOut {
  int32_t* chrom_id;
  int64_t* pos;
  uint8_t* pos_valid;
  float* qual;
  uint8_t* qual_valid;
  int32_t* filter_id;
  uint32_t* filter_off;  // where the row's FILTER text is in the slab, and its length ('.' -> 0): k_remap_filters verifies it
  uint32_t* filter_len;
  float* info[MAX_INFO];
  uint8_t* info_valid[MAX_INFO];
  uint32_t* lv_off[MAX_INFO];  // list kinds: offset of the value text in the slab / number of items, per row
  uint32_t* lv_cnt[MAX_INFO];
  unsigned* exceptions;  // [0] = count of rows the device could not decide
};

__device__ __forceinline__ void store_valid(uint8_t* bm, int64_t row0_of_wave, int64_t n_rows, bool v, int lane) {
  const unsigned long long m = __ballot(v);
  if (lane < 8) {
    const int64_t r = row0_of_wave + lane * 8;
    if (r < n_rows) bm[r >> 3] = (uint8_t)(m >> (lane * 8));
  }
}

// bit b = byte b of the 16-byte group equals `c` (splat as c * 0x01010101).  ONE mask per group and one loop over its bits: an inner
// loop per dword -- four divergent regions per group -- is exec-mask bookkeeping on the CU's scalar unit, which bounds k_parse_lines.
__device__ __forceinline__ unsigned eq_mask16(const uint4& v, uint32_t splat) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = w[k] ^ splat;  // equal bytes become 0
    const uint32_t m = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 exactly in the zero bytes
    const uint32_t t = m >> 7;                                                 // bits 0, 8, 16, 24
    mask |= ((t | (t >> 7) | (t >> 14) | (t >> 21)) & 0xFu) << (4 * k);
  }
  return mask;
}
// ... restricted to the bytes [begin, end) of the slab, the group starting at byte a
__device__ __forceinline__ unsigned clip_mask16(unsigned mask, unsigned a, unsigned begin, unsigned end) {
  if (begin > a) mask &= 0xFFFFu << (begin - a);
  if (end - a < 16u) mask &= (1u << (end - a)) - 1u;
  return mask;
}

__global__ __launch_bounds__(TPB) void k_parse_lines(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl_pos,
                                                     const unsigned* __restrict__ n_lines_p, NameTable contigs,
                                                     FilterTable filters, InfoKeys ik, ParseOut out, unsigned cap, unsigned skip,
                                                     unsigned n_total) {
  const int64_t n_rows = min(*n_lines_p, cap);
  // an aligned 16-byte group of the slab; the last one is read byte by byte (nothing behind n_total is touched)
  auto group16 = [&](unsigned a) {
    uint4 v = {0, 0, 0, 0};
    if (a + 16u <= n_total) {
      v = *reinterpret_cast<const uint4*>(text + a);
    } else {
      unsigned* w = &v.x;
      for (unsigned i = 0; a + i < n_total; ++i) w[i >> 2] |= (unsigned)text[a + i] << (8 * (i & 3));
    }
    return v;
  };
  const int64_t row = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool pos_ok = false, qual_ok = false, bad = false;
  unsigned info_ok = 0;  // bit q: INFO field q has a value in this row (bit masks, not arrays: up to 16 keys stay in registers)
  if (row < n_rows) {
    const unsigned begin = row ? nl_pos[row - 1] + 1 : skip;
    unsigned end = nl_pos[row];
    if (end > begin && text[end - 1] == '\r') --end;
    // split the first 8 fields
    unsigned fs[9];
    int nf = 0;
    fs[0] = begin;
    // tabs, 16 bytes per load (aligned groups; `text` is 16-byte aligned and padded): the byte-at-a-time version of this
    // loop was a chain of ~35 dependent loads per line, a quarter of the kernel's memory waits
    for (unsigned a = begin & ~15u; a < end && nf < 8; a += 16) {
      unsigned m = clip_mask16(eq_mask16(group16(a), 0x09090909u), a, begin, end);  // the group's tabs
      while (m && nf < 8) {
        fs[++nf] = a + (unsigned)__ffs((int)m);  // the field starts behind the tab
        m &= m - 1;
      }
    }
    // field f spans [fs[f], fs[f+1] - 1) for f < nf, the last one ends at `end` (INFO may be followed by FORMAT...)
    auto fbeg = [&](int f) { return fs[f]; };
    auto fend = [&](int f) { return f < nf ? fs[f + 1] - 1 : end; };
    if (nf < 7 || begin == end || text[begin] == '#') {
      bad = true;  // not a data line with 8 fields
      // the row's slots still get defined values: k_remap_filters indexes a table with filter_id, and the buffers are
      // recycled between scans (a corrupted file after other scans faulted there: found by tools/fuzz_gpu_decode.py)
      out.chrom_id[row] = 0;
      out.pos[row] = 0;
      out.qual[row] = 0.f;
      out.filter_id[row] = -1;  // no slot: k_remap_filters writes id 0 and compares nothing
      for (int q = 0; q < ik.n; ++q)
        if (ik.kind[q] == 'F' || ik.kind[q] == 'I') out.lv_cnt[q][row] = 0;  // summed by the offsets scan
    } else {
#ifndef EXON_PARSE_SKIP  // (profiling builds: bit 0 CHROM, 1 POS, 2 QUAL, 3 FILTER, 4 INFO left out)
#define EXON_PARSE_SKIP 0
#endif
      // CHROM
      if (!(EXON_PARSE_SKIP & 1)) {
        const uint8_t* p = text + fbeg(0);
        const int len = (int)(fend(0) - fbeg(0));
        const uint64_t h = fnv1a(p, len);
        int slot = (int)(h & (uint64_t)contigs.mask), id = -1;
        for (int probe = 0; probe <= contigs.mask; ++probe) {
          const uint64_t k = contigs.keys[slot];
          if (k == 0) break;
          if (k == h && (int)contigs.text_len[slot] == len) {
            bool same = true;
            for (int i = 0; i < len && same; ++i) same = contigs.pool[contigs.text_off[slot] + i] == p[i];
            if (same) {
              id = contigs.ids[slot];
              break;
            }
          }
          slot = (slot + 1) & contigs.mask;
        }
        if (id < 0) bad = true;  // contig not in the header: host decides the id
        out.chrom_id[row] = id < 0 ? 0 : id;
      }
      // POS
      if (!(EXON_PARSE_SKIP & 2)) {
        uint64_t v = 0;  // (unsigned: a spoiled or over-long value wraps, it never overflows a signed integer)
        unsigned pb = fbeg(1), pn = fend(1) - fbeg(1);
        if (pn && text[pb] == '+') ++pb, --pn;  // usize::from_str takes one leading '+' (host/formats.h parse_pos)
        bool ok = pn > 0;
        if (pn <= 16 && pb + 16u <= n_total) {  // the digits from two (unaligned) 8-byte loads instead of a chain of byte loads
          uint64_t w[2];
          __builtin_memcpy(w, text + pb, 16);
          for (unsigned k = 0; k < pn; ++k) {  // (no branch inside: a non-digit spoils v, which is then not used)
            const unsigned d = ((unsigned)(w[k >> 3] >> (8 * (k & 7))) & 0xFFu) - (unsigned)'0';
            ok &= d <= 9u;
            v = v * 10 + d;
          }
        } else {
          for (unsigned i = pb; i < pb + pn && ok; ++i) {
            const uint8_t c = text[i];
            if (c < '0' || c > '9') ok = false;
            else v = v * 10 + (c - '0');
          }
        }
        if (pn > 18) ok = false;  // beyond 18 digits the host decides (usize overflow is an error there)
        pos_ok = ok && v > 0;
        if (!ok) bad = true;  // not a number: `variant_start().transpose()?` is an error in the reference -- the host reports it
        out.pos[row] = pos_ok ? (int64_t)v : 0;
      }
      // QUAL
      if (!(EXON_PARSE_SKIP & 4)) {
        const int len = (int)(fend(5) - fbeg(5));
        float q = 0.f;
        if (!(len == 1 && text[fbeg(5)] == '.')) {
          uint32_t bits;
          if (exon::dec::parse_f32(reinterpret_cast<const char*>(text + fbeg(5)), len, &bits)) {
            q = __uint_as_float(bits);
            qual_ok = true;
          } else {
            bad = true;
          }
        }
        out.qual[row] = q;
      }
      // FILTER: '.' -> the empty list
      if (!(EXON_PARSE_SKIP & 8)) {
        const uint8_t* p = text + fbeg(6);
        int len = (int)(fend(6) - fbeg(6));
        if (len == 1 && p[0] == '.') len = 0;
        const unsigned long long h = fnv1a(p, len);
        int slot = (int)(h & (FILTER_SLOTS - 1));
        int found = -1;
        for (int probe = 0; probe < FILTER_SLOTS; ++probe) {
          unsigned long long k = filters.keys[slot];
          if (k == 0) {
            k = atomicCAS(&filters.keys[slot], 0ull, h);
            if (k == 0) {  // this thread inserted the key: remember where its text lives in this slab
              filters.text_off[slot] = fbeg(6);
              filters.text_len[slot] = (uint32_t)len;
              found = slot;
              break;
            }
          }
          if (k == h) {
            found = slot;
            break;
          }
          slot = (slot + 1) & (FILTER_SLOTS - 1);
        }
        if (found < 0) atomicExch(&filters.counters[2], 1);  // table full (found -1: no slot)
        out.filter_id[row] = found;  // provisional: slot index
        out.filter_off[row] = fbeg(6);
        out.filter_len[row] = (uint32_t)len;
      }
      // INFO: `key=value` (or a bare Flag key) among ';'-separated entries; the first occurrence of a key wins
      if (ik.n > 0 && !(EXON_PARSE_SKIP & 16)) {
        unsigned seen = 0;  // bit q: key q was met (the first occurrence wins); values are stored as they are parsed
        int left = ik.n;
        const unsigned ib = fbeg(7), ie = fend(7);
        if (!(ie - ib == 1 && text[ib] == '.')) {  // INFO '.': the whole struct is NULL
          // entries are separated by ';': find the separators 16 bytes per load, test the keys at every entry start
          unsigned i = ib;  // start of the current entry
          auto entry = [&](unsigned j) {  // the entry [i, j)
            for (int q = 0; q < ik.n; ++q) {
              const int kl = ik.len[q];
              if ((seen >> q & 1u) || (int)(j - i) < kl) continue;
              const bool valued = (int)(j - i) > kl && text[i + kl] == '=';
              if (!valued && (int)(j - i) != kl) continue;
              bool same = true;
              for (int k = 0; k < kl && same; ++k) same = text[i + k] == ik.text[ik.off[q] + k];
              if (!same) continue;
              seen |= 1u << q;
              --left;
              if (ik.kind[q] == 'b') {
                info_ok |= 1u << q;  // a Flag is true by being there
              } else if (valued) {
                const unsigned vb = i + kl + 1;
                const int vl = (int)(j - vb);
                if (!(vl == 0 || (vl == 1 && text[vb] == '.'))) {
                  uint32_t bits;
                  if (ik.kind[q] == 's') {  // String / Character: the value's text; its dictionary id comes from k_info_string_ids
                    out.lv_off[q][row] = vb;
                    out.lv_cnt[q][row] = (uint32_t)vl;
                    info_ok |= 1u << q;
                  } else if (ik.kind[q] == 'F' || ik.kind[q] == 'I') {
                    unsigned items = 1;  // items are separated by ','; they are parsed by k_list_fill
                    for (int k = 0; k < vl; ++k) items += text[vb + k] == ',';
                    out.lv_off[q][row] = vb;
                    out.lv_cnt[q][row] = items;
                    info_ok |= 1u << q;
                  } else if (ik.kind[q] == 'i') {
                    // Type=Integer: exact int32 ([+-] digits); the value travels as its bit pattern in the 4-byte column.
                    // Anything else (including out of range) is the reference's parse error: the row is left to the host
                    int k = 0;
                    const bool neg = text[vb] == '-';
                    if (neg || text[vb] == '+') k = 1;
                    int64_t iv = 0;
                    bool ok = k < vl && vl - k <= 10;
                    for (; k < vl && ok; ++k) {
                      const unsigned d = (unsigned)text[vb + k] - '0';
                      ok = d <= 9u;
                      iv = iv * 10 + d;
                    }
                    if (neg) iv = -iv;
                    if (ok && iv >= INT32_MIN && iv <= INT32_MAX) {
                      out.info[q][row] = __int_as_float((int32_t)iv);
                      info_ok |= 1u << q;
                    } else {
                      bad = true;
                    }
                  } else if (exon::dec::parse_f32(reinterpret_cast<const char*>(text + vb), vl, &bits)) {
                    out.info[q][row] = __uint_as_float(bits);
                    info_ok |= 1u << q;
                  } else {
                    bad = true;
                  }
                }
              }
            }
            i = j + 1;
          };
          for (unsigned a = ib & ~15u; a < ie && left > 0; a += 16) {
            unsigned m = clip_mask16(eq_mask16(group16(a), 0x3B3B3B3Bu), a, ib, ie);  // the group's ';'
            while (m && left > 0) {
              entry(a + (unsigned)__ffs((int)m) - 1u);
              m &= m - 1;
            }
          }
          if (left > 0 && i < ie) entry(ie);  // the last entry has no ';' behind it
        }
        for (int q = 0; q < ik.n; ++q) {
          if (info_ok >> q & 1u) continue;
          if (ik.kind[q] == 'F' || ik.kind[q] == 'I') out.lv_cnt[q][row] = 0;  // NULL list: no items
          else if (ik.kind[q] != 'b') out.info[q][row] = 0.f;                   // NULL slots hold a defined value
        }
      }
    }
  }
  const int64_t wave_row0 = row - lane;
  store_valid(out.pos_valid, wave_row0, n_rows, pos_ok, lane);
  store_valid(out.qual_valid, wave_row0, n_rows, qual_ok, lane);
  for (int q = 0; q < ik.n; ++q) store_valid(out.info_valid[q], wave_row0, n_rows, (info_ok >> q & 1u) != 0, lane);
  const unsigned long long nb = __ballot(bad);
  if (lane == 0 && nb) atomicAdd(out.exceptions, (unsigned)__popcll(nb));
}

// Number=1 String / Character INFO key (info_builder.rs:152-309 builds a Utf8 column; here: dictionary ids + the dictionary, like
// FILTER): every row with a value hashes its text into the key's table -- provisional slot in ids[row], replaced by the dense id
// by k_remap_filters once k_assign_filters has numbered the new values.  counters[3] += rows WITHOUT a value (a consumer that
// groups by the key needs to know whether there is a NULL group).
__global__ __launch_bounds__(TPB) void k_info_string_ids(const uint8_t* __restrict__ text, const uint32_t* __restrict__ voff, const uint32_t* __restrict__ vlen,
                                                         const uint8_t* __restrict__ valid, const unsigned* __restrict__ n_lines_p, unsigned cap, FilterTable t,
                                                         int32_t* __restrict__ ids, int null_as_value) {
  const unsigned n = min(*n_lines_p, cap);
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  bool has = false;
  if (row < n) {
    has = (valid[row >> 3] >> (row & 7)) & 1;
    int found = -1;  // -1: no slot (no value, or the table is full): k_remap_filters writes id 0 and compares nothing
    // null_as_value (a fused plan groups by this key): a row without a value takes the id of the EMPTY text -- a value no row can
    // carry ("key=" is a missing value) -- so that NULL is a group of its own, as in DataFusion's GROUP BY
    if (has || null_as_value) {
      const uint8_t* p = text + (has ? voff[row] : 0u);
      const int len = has ? (int)vlen[row] : 0;
      const unsigned long long h = fnv1a(p, len);
      int slot = (int)(h & (FILTER_SLOTS - 1));
      found = -1;
      for (int probe = 0; probe < FILTER_SLOTS; ++probe) {
        unsigned long long k = t.keys[slot];
        if (k == 0) {
          k = atomicCAS(&t.keys[slot], 0ull, h);
          if (k == 0) {
            t.text_off[slot] = has ? voff[row] : 0u;
            t.text_len[slot] = (uint32_t)len;
            found = slot;
            break;
          }
        }
        if (k == h) {
          found = slot;
          break;
        }
        slot = (slot + 1) & (FILTER_SLOTS - 1);
      }
      if (found < 0) atomicExch(&t.counters[2], 1);
    }
    ids[row] = found;
  }
  const unsigned long long miss = __ballot(row < n && !has && !null_as_value);
  if ((threadIdx.x & 63) == 0 && miss) atomicAdd(&t.counters[3], __popcll(miss));
  // (null_as_value: counters[3] stays 0 = "no row without an id": the consumer then takes the ids without the bitmap)
}

// dense ids for FILTER lists inserted during the last parse, text copied into the persistent pool.  New lists are
// rare, so every thread scans its share of the slots and claims ids / pool space with atomics (ids are arbitrary
// but stable; names are recovered through exon_hip_vcf_parser_filters).  A slot that finds no room is marked -2: it
// keeps no id, and its text stays in the slab (an id it claimed is a hole that table_names stops at).
__global__ __launch_bounds__(256) void k_assign_filters(const uint8_t* __restrict__ text, FilterTable f) {
  for (int s = threadIdx.x; s < FILTER_SLOTS; s += 256)
    if (f.keys[s] != 0 && f.ids[s] == -1) {
      const uint32_t len = f.text_len[s], src = f.text_off[s];
      const int id = atomicAdd(&f.counters[0], 1);
      const int po = atomicAdd(&f.counters[1], (int)len);
      if (id >= EXON_HIP_MAX_GROUPS || po < 0 || po + (int64_t)len > FILTER_POOL) {
        f.counters[2] = 1;
        f.ids[s] = -2;
        continue;
      }
      for (uint32_t i = 0; i < len; ++i) f.pool[po + i] = text[src + i];
      f.text_off[s] = (uint32_t)po;
      f.ids[s] = id;
    }
}

// provisional slot -> dense id, and the text check: a key matched by its 64-bit hash alone may be another text (FNV-1a is no
// cryptographic hash and the values are free file text), so each row compares its own bytes [off, off + len) with its key's
// text in the pool.  A mismatch sets the overflow flag: the slab, like one that overflows the table, goes to the host reader.
// valid: NULL (FILTER: every row with a slot has its text) or the String key's bitmap (a row without a value that took a slot
// under null_as_value has the EMPTY text).  Rows without a slot (-1) get id 0.  An overflowed table compares nothing: its
// slab is undecided already, and a slot without an id has no text in the pool.
__global__ __launch_bounds__(TPB) void k_remap_filters(int32_t* __restrict__ ids_io, const unsigned* __restrict__ n_lines_p, unsigned cap,
                                                       FilterTable t, const uint8_t* __restrict__ text, const uint32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ len, const uint8_t* __restrict__ valid) {
  const int64_t n = min(*n_lines_p, cap);
  const bool check = t.counters[2] == 0;
  bool differs = false;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
    const unsigned slot = (unsigned)ids_io[i];
    if (slot >= (unsigned)FILTER_SLOTS) {
      ids_io[i] = 0;
      continue;
    }
    const int id = t.ids[slot];
    ids_io[i] = id < 0 ? 0 : id;
    if (!check) continue;
    const bool has = !valid || ((valid[i >> 3] >> (i & 7)) & 1);
    const uint32_t l = has ? len[i] : 0u, to = t.text_off[slot];
    if (t.text_len[slot] != l || (uint64_t)to + l > (uint64_t)FILTER_POOL) {
      differs = true;
      continue;
    }
    const uint8_t* a = text + (has ? off[i] : 0u);
    const uint8_t* b = t.pool + to;
    for (uint32_t k = 0; k < l; ++k)
      if (a[k] != b[k]) {
        differs = true;
        break;
      }
  }
  if (differs) atomicExch(&t.counters[2], 1);
}

}  // namespace

// Upload an open-addressing name table (names[i] -> id i) into buffers of `b` (a failure stays in b.status()).
static void build_name_table(PoolBufs& b, const char* const* names_in, int32_t n, NameTable* out) {
  int cap = 16;
  while (cap < 2 * n + 1) cap <<= 1;
  std::vector<uint64_t> keys((size_t)cap, 0);
  std::vector<int32_t> ids((size_t)cap, -1);
  std::vector<uint32_t> toff((size_t)cap, 0), tlen((size_t)cap, 0);
  std::string pool;
  for (int i = 0; i < n; ++i) {
    const std::string nm = names_in[i];
    const uint64_t h = fnv1a(reinterpret_cast<const uint8_t*>(nm.data()), (int)nm.size());
    int slot = (int)(h & (uint64_t)(cap - 1));
    while (keys[(size_t)slot] != 0) slot = (slot + 1) & (cap - 1);
    keys[(size_t)slot] = h;
    ids[(size_t)slot] = i;
    toff[(size_t)slot] = (uint32_t)pool.size();
    tlen[(size_t)slot] = (uint32_t)nm.size();
    pool += nm;
  }
  uint64_t* d_keys = b.take<uint64_t>((size_t)cap * 8);
  int32_t* d_ids = b.take<int32_t>((size_t)cap * 4);
  uint32_t* d_toff = b.take<uint32_t>((size_t)cap * 4);
  uint32_t* d_tlen = b.take<uint32_t>((size_t)cap * 4);
  uint8_t* d_pool = b.take<uint8_t>(pool.size() + 16);
  b.upload(d_keys, keys.data(), (size_t)cap * 8);
  b.upload(d_ids, ids.data(), (size_t)cap * 4);
  b.upload(d_toff, toff.data(), (size_t)cap * 4);
  b.upload(d_tlen, tlen.data(), (size_t)cap * 4);
  b.upload(d_pool, pool.data(), pool.size());
  *out = NameTable{d_keys, d_ids, d_toff, d_tlen, d_pool, cap - 1};
}

// a dictionary the device builds (FILTER lists, the values of a String INFO key): keys 0 (empty), ids -1, counters 0
static FilterTable take_filter_table(PoolBufs& b) {
  FilterTable t;
  t.keys = b.take<unsigned long long>(FILTER_SLOTS * 8, 0);
  t.ids = b.take<int32_t>(FILTER_SLOTS * 4, 0xFF);
  t.text_off = b.take<uint32_t>(FILTER_SLOTS * 4);
  t.text_len = b.take<uint32_t>(FILTER_SLOTS * 4);
  t.pool = b.take<uint8_t>(FILTER_POOL);
  t.counters = b.take<int32_t>(16, 0);
  return t;
}

// ------------------------------------------------------------------------------------------------------------
// ---- list-valued INFO fields ('F' / 'I'): offsets by a scan of the per-row item counts (list_kernels.h), then the items ------
// offsets[row] = exclusive prefix of cnt (block_offsets = scanned block sums), offsets[n_rows] = total; every row parses its
// items into values[offsets[row] ..]: '.' or an empty item -> NULL item (flag 0), anything unparsable -> undecided (host)
__global__ __launch_bounds__(LIST_TPB) void k_list_fill(const uint8_t* __restrict__ text, unsigned n_total, const uint32_t* __restrict__ lv_off,
                                                        const uint32_t* __restrict__ cnt, const unsigned* __restrict__ block_offsets,
                                                        const unsigned* __restrict__ n_rows_p, unsigned cap, unsigned cap_items, char kind,
                                                        int32_t* __restrict__ offsets, float* __restrict__ values,
                                                        uint8_t* __restrict__ item_flags, unsigned* __restrict__ exceptions) {
  const unsigned n_rows = min(*n_rows_p, cap);
  const unsigned row = blockIdx.x * LIST_TPB + threadIdx.x;
  const unsigned c = row < n_rows ? cnt[row] : 0u;
  const unsigned first = list_first_item(c, block_offsets);
  if (row < n_rows) offsets[row] = (int32_t)first;
  if (row + 1 == n_rows) offsets[n_rows] = (int32_t)(first + c);
  if (row == 0 && n_rows == 0) offsets[0] = 0;
  if (row >= n_rows || c == 0) return;
  if ((uint64_t)first + c > cap_items) {  // comma-dense values ("AF=,,,,": one EMPTY item per byte) can exceed slab bytes / 2 + 1: host decoder
    atomicAdd(exceptions, 1u);
    return;
  }
  unsigned a = lv_off[row];
  bool bad = false;
  for (unsigned i = 0; i < c; ++i) {
    unsigned e = a;
    while (e < n_total && text[e] != ',' && text[e] != ';' && text[e] != '\t' && text[e] != '\n' && text[e] != '\r') ++e;
    const int len = (int)(e - a);
    uint32_t bits = 0;
    bool ok = false;
    if (!(len == 0 || (len == 1 && text[a] == '.'))) {
      if (kind == 'I') {
        int k = 0;
        const bool neg = text[a] == '-';
        if (neg || text[a] == '+') k = 1;
        int64_t iv = 0;
        ok = k < len && len - k <= 10;
        for (; k < len && ok; ++k) {
          const unsigned d = (unsigned)text[a + k] - '0';
          ok = d <= 9u;
          iv = iv * 10 + d;
        }
        if (neg) iv = -iv;
        ok = ok && iv >= INT32_MIN && iv <= INT32_MAX;
        bits = (uint32_t)(int32_t)iv;
      } else {
        ok = exon::dec::parse_f32(reinterpret_cast<const char*>(text + a), len, &bits);
      }
      if (!ok) bad = true;
    }
    values[first + i] = __uint_as_float(ok ? bits : 0u);
    item_flags[first + i] = ok ? 1 : 0;
    a = e + 1;
  }
  if (bad) atomicAdd(exceptions, 1u);
}
struct exon_hip_vcf_parser {
  exon_hip_ctx* ctx;
  PoolBufs bufs;
  int64_t max_rows = 0, cap_items = 0;
  std::string info_field;  // "name[:kind],..." as given; kinds f (default) / b
  InfoKeys ik{};
  LineIndex idx;  // scalars: [0] n_lines, [1] exceptions, [2] consumed bytes
  NameTable contigs{};
  FilterTable filters{};
  ParseOut out{};
  InfoBufs info[MAX_INFO];
  unsigned* d_list_blocks = nullptr;  // per-workgroup sums of the item counts (scanned in place)
  FilterTable str_tables[MAX_INFO] = {};  // kind 's': the key's value dictionary, built on the device like the FILTER dictionary
  int null_as_value = 0;  // exon_hip_vcf_parser_set_null_key: rows without a value of a String key take the id of the empty text
  int32_t h_str_stat[MAX_INFO][2] = {{0, 0}};  // per 's' key, last slab: {dictionary overflow, rows without a value}
  int32_t h_filter_stat = 0;                   // the FILTER dictionary's overflow flag after the last slab
  // the `info` text column (exon_hip_vcf_parser_set_key_types / _info_text): the header's key types on the device, the slab of
  // the last parse call as the caller passed it (last_rows < 0: none, or one with undecided rows) and the column's buffers
  PoolBufs key_bufs, format_key_bufs;
  ExonVcfKeyTable key_table{}, format_key_table{};  // the INFO keys' types; the FORMAT keys' (exon_hip_vcf_parser_set_format_key_types / _formats_text)
  const uint8_t* last_text = nullptr;
  int64_t last_bytes = 0, last_rows = -1;
  ExonTextScratch* info_scratch = nullptr;
  explicit exon_hip_vcf_parser(exon_hip_ctx* c) : ctx(c), bufs(c), key_bufs(c), format_key_bufs(c) {}
  ~exon_hip_vcf_parser() { exon_text_scratch_destroy(info_scratch); }
};

extern "C" {

int exon_hip_vcf_parser_create(exon_hip_ctx* ctx, const char* const* contig_names, int32_t n_contigs,
                               const char* info_field, int64_t max_bytes, exon_hip_vcf_parser** outp) {
  if (!ctx || !outp || (n_contigs > 0 && !contig_names) || max_bytes < 16)
    return fail(ctx, EXON_HIP_EINVAL, "exon_hip_vcf_parser_create: bad argument");
  if (max_bytes > 0xF0000000LL) return fail(ctx, EXON_HIP_EINVAL, "slab size must stay below 4 GiB (32-bit line offsets)");
  *outp = nullptr;
  exon_hip_vcf_parser* p = new (std::nothrow) exon_hip_vcf_parser(ctx);
  if (!p) return fail(ctx, EXON_HIP_ENOMEM, "out of host memory");
  p->max_rows = max_bytes / 16 + 1;  // a VCF data line has 8 fields: >= 15 bytes + newline
  p->info_field = info_field ? info_field : "";
  hipSetDevice(ctx->device);
  PoolBufs& b = p->bufs;
  build_name_table(b, contig_names, n_contigs, &p->contigs);
  p->filters = take_filter_table(b);
  p->idx.alloc(b, max_bytes, p->max_rows);
  // INFO keys: "AF,DP:f,DB:b" -> names back to back + (offset, length, kind) per key
  std::string key_text;
  {
    size_t i = 0;
    const std::string& f = p->info_field;
    while (i < f.size()) {
      size_t j = f.find(',', i);
      if (j == std::string::npos) j = f.size();
      std::string item = f.substr(i, j - i);
      char kind = 'f';
      const size_t c = item.rfind(':');
      if (c != std::string::npos && c + 2 == item.size() && (item[c + 1] == 'f' || item[c + 1] == 'b' || item[c + 1] == 'i' || item[c + 1] == 'F' || item[c + 1] == 'I' || item[c + 1] == 's')) {
        kind = item[c + 1];
        item.resize(c);
      }
      if (!item.empty()) {
        if (p->ik.n == MAX_INFO) {
          delete p;
          return fail(ctx, EXON_HIP_EUNSUPPORTED, "at most %d INFO fields per parser", MAX_INFO);
        }
        p->ik.off[p->ik.n] = (int)key_text.size();
        p->ik.len[p->ik.n] = (int)item.size();
        p->ik.kind[p->ik.n] = kind;
        key_text += item;
        ++p->ik.n;
      }
      i = j + 1;
    }
  }
  uint8_t* d_key_text = b.take<uint8_t>(key_text.size() + 16);
  b.upload(d_key_text, key_text.data(), key_text.size());
  p->ik.text = d_key_text;
  const size_t r = (size_t)p->max_rows, rb = r / 8 + 64;
  p->out.chrom_id = b.take<int32_t>(r * 4);
  p->out.pos = b.take<int64_t>(r * 8);
  p->out.pos_valid = b.take<uint8_t>(rb);
  p->out.qual = b.take<float>(r * 4);
  p->out.qual_valid = b.take<uint8_t>(rb);
  p->out.filter_id = b.take<int32_t>(r * 4);
  p->out.filter_off = b.take<uint32_t>(r * 4);
  p->out.filter_len = b.take<uint32_t>(r * 4);
  p->cap_items = max_bytes / 2 + 1;  // a non-empty item and its separator take at least two bytes of the slab; a slab of mostly EMPTY
                                     // items (legal: "AF=,,,,") overflows this and is decoded by the host reader (k_list_fill / k_pack_bits clamp)
  for (int q = 0; q < p->ik.n; ++q) {
    const char kind = p->ik.kind[q];
    InfoBufs& k = p->info[q];
    if (kind == 'f' || kind == 'i' || kind == 's') k.value = b.take<float>(r * 4);
    k.valid = b.take<uint8_t>(rb);
    if (kind == 's') {  // Number=1 String / Character: where the value text is (k_parse_lines), then dictionary ids (k_info_string_ids)
      k.lv_off = b.take<uint32_t>(r * 4);
      k.lv_cnt = b.take<uint32_t>(r * 4);
      p->str_tables[q] = take_filter_table(b);
    }
    if (kind == 'F' || kind == 'I') {
      k.take_list(b, r, (size_t)p->cap_items);
      if (!p->d_list_blocks) p->d_list_blocks = b.take<unsigned>((r / LIST_TPB + 2) * 4);
    }
    p->out.info[q] = (kind == 'F' || kind == 'I') ? k.items : k.value;
    p->out.info_valid[q] = static_cast<uint8_t*>(k.valid);
    p->out.lv_off[q] = k.lv_off;
    p->out.lv_cnt[q] = k.lv_cnt;
  }
  if (b.status() != hipSuccess) {
    const std::string msg = hipGetErrorString(b.status());
    delete p;
    return fail(ctx, EXON_HIP_ENOMEM, "vcf parser allocation: %s", msg.c_str());
  }
  p->out.exceptions = p->idx.d_scalars + 1;
  *outp = p;
  return EXON_HIP_OK;
}

int exon_hip_vcf_parser_destroy(exon_hip_vcf_parser* p) {
  delete p;
  return EXON_HIP_OK;
}

int exon_hip_vcf_parser_parse(exon_hip_vcf_parser* p, void* stream, const uint8_t* d_text, int64_t n_bytes,
                              exon_hip_vcf_columns* cols) {
  if (!p || !cols || (n_bytes > 0 && !d_text)) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_vcf_parser_parse: NULL argument");
  exon_hip_ctx* ctx = p->ctx;
  memset(cols, 0, sizeof *cols);
  p->last_rows = -1;
  if (n_bytes == 0) return EXON_HIP_OK;
  LineIndex& idx = p->idx;
  const uint8_t* const text_given = d_text;
  const int64_t bytes_given = n_bytes;
  unsigned skip;
  if (int rc = idx.align(ctx, &d_text, &n_bytes, &skip)) return rc;
  hipStream_t s = pick_stream(ctx, stream);
  idx.launch(s, d_text, n_bytes, skip);
  hipLaunchKernelGGL(k_last_newline, dim3(1), dim3(1), 0, s, idx.nl, idx.d_scalars, idx.cap);
  // the number of lines is bounded by n_bytes / 16 + 1 for well-formed data lines; launch for that bound
  const int64_t row_bound = std::min<int64_t>(p->max_rows, n_bytes / 16 + 1);
  const int pblocks = (int)((row_bound + TPB - 1) / TPB);
  hipLaunchKernelGGL(k_parse_lines, dim3(pblocks), dim3(TPB), 0, s, d_text, idx.nl, idx.d_scalars, p->contigs, p->filters,
                     p->ik, p->out, (unsigned)row_bound, skip, (unsigned)n_bytes);
  hipLaunchKernelGGL(k_assign_filters, dim3(1), dim3(256), 0, s, d_text, p->filters);
  hipLaunchKernelGGL(k_remap_filters, dim3(std::min(pblocks, 4096)), dim3(TPB), 0, s, p->out.filter_id, idx.d_scalars, (unsigned)row_bound, p->filters,
                     d_text, p->out.filter_off, p->out.filter_len, (const uint8_t*)nullptr);
  HIP_TRY(ctx, hipMemcpyAsync(&p->h_filter_stat, p->filters.counters + 2, 4, hipMemcpyDeviceToHost, s));  // overflow or collision
  const int lblocks = (int)((row_bound + LIST_TPB - 1) / LIST_TPB);
  const unsigned cap_items = (unsigned)std::min<int64_t>(p->cap_items, 0xFFFFFFFFLL);
  for (int q = 0; q < p->ik.n; ++q) {  // list-valued fields: counts -> offsets -> items -> child validity
    const char kind = p->ik.kind[q];
    if (kind != 'F' && kind != 'I') continue;
    const InfoBufs& k = p->info[q];
    launch_list_scan(s, k.lv_cnt, idx.d_scalars, (unsigned)row_bound, lblocks, p->d_list_blocks, idx.d_scalars + 3);
    hipLaunchKernelGGL(k_list_fill, dim3(lblocks), dim3(LIST_TPB), 0, s, d_text, (unsigned)n_bytes, k.lv_off, k.lv_cnt, p->d_list_blocks,
                       idx.d_scalars, (unsigned)row_bound, cap_items, kind, k.offsets, k.items, k.item_flags, p->out.exceptions);
    k.pack_bits(s, idx.d_scalars, (unsigned)row_bound, cap_items);
  }
  for (int q = 0; q < p->ik.n; ++q) {  // String / Character keys: value text -> dictionary ids
    if (p->ik.kind[q] != 's') continue;
    FilterTable& t = p->str_tables[q];
    HIP_TRY(ctx, hipMemsetAsync(t.counters + 3, 0, 4, s));
    hipLaunchKernelGGL(k_info_string_ids, dim3(pblocks), dim3(TPB), 0, s, d_text, p->out.lv_off[q], p->out.lv_cnt[q], p->out.info_valid[q], idx.d_scalars, (unsigned)row_bound, t,
                       (int32_t*)p->out.info[q], p->null_as_value);
    hipLaunchKernelGGL(k_assign_filters, dim3(1), dim3(256), 0, s, d_text, t);
    hipLaunchKernelGGL(k_remap_filters, dim3(std::min(pblocks, 4096)), dim3(TPB), 0, s, (int32_t*)p->out.info[q], idx.d_scalars, (unsigned)row_bound, t,
                       d_text, p->out.lv_off[q], p->out.lv_cnt[q], (const uint8_t*)p->out.info_valid[q]);
    HIP_TRY(ctx, hipMemcpyAsync(p->h_str_stat[q], t.counters + 2, 8, hipMemcpyDeviceToHost, s));  // {overflow, rows without a value}
  }
  if (int rc = idx.read_back(ctx, s)) return rc;
  const int64_t n_lines = idx.h_scalars[0];
  if (n_lines > row_bound) return fail(ctx, EXON_HIP_EINVAL, "slab has %lld lines, more than its byte size allows for VCF records", (long long)n_lines);
  cols->n_rows = n_lines;
  cols->n_undecided = idx.h_scalars[1] + (p->h_filter_stat ? 1 : 0);  // FILTER lists beyond the dictionary: the host reader's
  cols->consumed_bytes = idx.consumed(skip);
  cols->chrom_id = p->out.chrom_id;
  cols->pos = p->out.pos;
  cols->pos_valid = p->out.pos_valid;
  cols->qual = p->out.qual;
  cols->qual_valid = p->out.qual_valid;
  cols->filter_id = p->out.filter_id;
  cols->info = p->ik.n ? p->out.info[0] : nullptr;
  cols->info_valid = p->ik.n ? p->out.info_valid[0] : nullptr;
  cols->n_info = p->ik.n;
  for (int q = 0; q < p->ik.n; ++q) {
    cols->infos[q] = p->out.info[q];  // NULL for a Flag: its column IS the presence bitmap
    cols->infos_valid[q] = p->out.info_valid[q];
    cols->info_kinds[q] = p->ik.kind[q];
    cols->info_nulls[q] = p->ik.kind[q] == 's' ? p->h_str_stat[q][1] : -1;
    if (p->ik.kind[q] == 's' && p->h_str_stat[q][0]) ++cols->n_undecided;  // more distinct values than the dictionary holds: the host reader's
    if (p->ik.kind[q] == 'F' || p->ik.kind[q] == 'I') {
      cols->list_offsets[q] = p->info[q].offsets;
      cols->list_item_valid[q] = p->info[q].item_bits;
    }
  }
  if (cols->n_undecided == 0) {
    p->last_text = text_given;
    p->last_bytes = bytes_given;
    p->last_rows = n_lines;
  }
  return EXON_HIP_OK;
}

int exon_hip_vcf_parser_set_key_types(exon_hip_vcf_parser* p, const char* packed_keys, const char* kinds, int32_t n) {
  if (!p || n < 0 || (n > 0 && (!packed_keys || !kinds))) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_vcf_parser_set_key_types: bad argument");
  for (int32_t k = 0; k < n; ++k)
    if (!strchr("ifbcs", kinds[k]) || !kinds[k]) return fail(p->ctx, EXON_HIP_EINVAL, "exon_hip_vcf_parser_set_key_types: kind '%c' of key %d (i f b c s)", kinds[k], k);
  return exon_vcf_key_table_build(p->ctx, &p->key_bufs, packed_keys, kinds, n, ExonVcfKeySeed::Info, &p->key_table);
}

int exon_hip_vcf_parser_set_format_key_types(exon_hip_vcf_parser* p, const char* packed_keys, const char* kinds, int32_t n) {
  if (!p || n < 0 || (n > 0 && (!packed_keys || !kinds))) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_vcf_parser_set_format_key_types: bad argument");
  for (int32_t k = 0; k < n; ++k)  // (a Flag is no FORMAT type)
    if (!strchr("ifcs", kinds[k]) || !kinds[k]) return fail(p->ctx, EXON_HIP_EINVAL, "exon_hip_vcf_parser_set_format_key_types: kind '%c' of key %d (i f c s)", kinds[k], k);
  return exon_vcf_key_table_build(p->ctx, &p->format_key_bufs, packed_keys, kinds, n, ExonVcfKeySeed::Format, &p->format_key_table);
}

int exon_hip_vcf_parser_info_text(exon_hip_vcf_parser* p, void* stream, exon_hip_vcf_info_text* out) {
  if (!p || !out) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_vcf_parser_info_text: NULL argument");
  memset(out, 0, sizeof *out);
  if (!p->key_table.hash) return fail(p->ctx, EXON_HIP_ESTATE, "exon_hip_vcf_parser_info_text: no key types (call exon_hip_vcf_parser_set_key_types first)");
  if (p->last_rows < 0) return fail(p->ctx, EXON_HIP_ESTATE, "exon_hip_vcf_parser_info_text: no slab to build from (parse first; a slab with undecided rows has none)");
  ExonTextColumns t;
  int64_t und = 0;
  if (int rc = exon_text_vcf(p->ctx, stream, &p->info_scratch, p->last_text, p->last_bytes, p->idx.nl, p->last_rows, EXON_HIP_PROJECT_VCF_INFO, &p->key_table, nullptr, &t, &und)) return rc;
  HIP_TRY(p->ctx, hipStreamSynchronize(pick_stream(p->ctx, stream)));
  out->n_undecided = und;
  if (und || !t.n_roots) return EXON_HIP_OK;  // (a slab of no rows has no column)
  const ExonTextNode& info = t.nodes[t.roots[0]];
  out->n_bytes = info.n_values;
  out->offsets = info.offsets;
  out->values = static_cast<const uint8_t*>(info.values);
  return EXON_HIP_OK;
}

int exon_hip_vcf_parser_formats_text(exon_hip_vcf_parser* p, void* stream, exon_hip_vcf_info_text* out) {
  if (!p || !out) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_vcf_parser_formats_text: NULL argument");
  memset(out, 0, sizeof *out);
  if (!p->format_key_table.hash) return fail(p->ctx, EXON_HIP_ESTATE, "exon_hip_vcf_parser_formats_text: no key types (call exon_hip_vcf_parser_set_format_key_types first)");
  if (p->last_rows < 0) return fail(p->ctx, EXON_HIP_ESTATE, "exon_hip_vcf_parser_formats_text: no slab to build from (parse first; a slab with undecided rows has none)");
  ExonTextColumns t;
  int64_t und = 0;
  if (int rc = exon_text_vcf(p->ctx, stream, &p->info_scratch, p->last_text, p->last_bytes, p->idx.nl, p->last_rows, EXON_HIP_PROJECT_VCF_FORMATS | EXON_HIP_PROJECT_VCF_FORMATS_ON_DEVICE,
                             nullptr, &p->format_key_table, &t, &und))
    return rc;
  HIP_TRY(p->ctx, hipStreamSynchronize(pick_stream(p->ctx, stream)));
  out->n_undecided = und;
  if (und || !t.n_roots) return EXON_HIP_OK;  // (a slab of no rows has no column)
  const ExonTextNode& formats = t.nodes[t.roots[0]];
  out->n_bytes = formats.n_values;
  out->offsets = formats.offsets;
  out->values = static_cast<const uint8_t*>(formats.values);
  return EXON_HIP_OK;
}

}  // extern "C"
const unsigned* exon_hip_vcf_parser_newlines(exon_hip_vcf_parser* p) { return p ? p->idx.nl : nullptr; }
const ExonVcfKeyTable* exon_hip_vcf_parser_key_table(exon_hip_vcf_parser* p) { return p ? &p->key_table : nullptr; }
const ExonVcfKeyTable* exon_hip_vcf_parser_format_key_table(exon_hip_vcf_parser* p) { return p ? &p->format_key_table : nullptr; }
extern "C" {

// a device-built dictionary (FILTER lists, or the values of a String INFO key) in id order: names '\0'-separated into `buf`.
// so_far: an overflowed (or colliding) table still yields the names it assigned, up to the first id that got no name -- those of
// every slab parsed before the overflow (the exporter names a slab's batches after the NEXT slab has been parsed)
static int table_names(exon_hip_ctx* ctx, const FilterTable& t, const char* what, char* buf, size_t cap, int32_t* n_names, bool so_far) {
  int32_t counters[4];
  HIP_TRY(ctx, hipMemcpy(counters, t.counters, 16, hipMemcpyDeviceToHost));
  if (counters[2] && !so_far)
    return fail(ctx, EXON_HIP_EUNSUPPORTED, "more than %d distinct %s (or their text pool exhausted, or two of them hash alike)", EXON_HIP_MAX_GROUPS, what);
  counters[0] = std::min(counters[0], EXON_HIP_MAX_GROUPS);
  counters[1] = std::min(counters[1], FILTER_POOL);
  std::vector<unsigned long long> keys(FILTER_SLOTS);
  std::vector<int32_t> ids(FILTER_SLOTS);
  std::vector<uint32_t> toff(FILTER_SLOTS), tlen(FILTER_SLOTS);
  std::vector<uint8_t> pool((size_t)std::max(counters[1], 1));
  HIP_TRY(ctx, hipMemcpy(keys.data(), t.keys, FILTER_SLOTS * 8, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(ids.data(), t.ids, FILTER_SLOTS * 4, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(toff.data(), t.text_off, FILTER_SLOTS * 4, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(tlen.data(), t.text_len, FILTER_SLOTS * 4, hipMemcpyDeviceToHost));
  if (counters[1] > 0) HIP_TRY(ctx, hipMemcpy(pool.data(), t.pool, (size_t)counters[1], hipMemcpyDeviceToHost));
  std::vector<std::string> names((size_t)counters[0]);
  std::vector<char> named((size_t)counters[0], 0);
  for (int s = 0; s < FILTER_SLOTS; ++s)
    if (keys[(size_t)s] != 0 && ids[(size_t)s] >= 0 && ids[(size_t)s] < counters[0] && (size_t)toff[(size_t)s] + tlen[(size_t)s] <= pool.size()) {
      names[(size_t)ids[(size_t)s]] = std::string(reinterpret_cast<const char*>(pool.data()) + toff[(size_t)s], tlen[(size_t)s]);
      named[(size_t)ids[(size_t)s]] = 1;
    }
  size_t n = 0;
  while (n < names.size() && named[n]) ++n;
  if (n < names.size() && !counters[2]) return fail(ctx, EXON_HIP_EDEVICE, "%s: id %zu has no name", what, n);
  names.resize(n);
  size_t need = 0;
  for (const auto& nm : names) need += nm.size() + 1;
  *n_names = (int32_t)n;
  if (buf) {
    if (need > cap) return fail(ctx, EXON_HIP_EINVAL, "name buffer too small (%zu needed)", need);
    size_t o = 0;
    for (const auto& nm : names) {
      memcpy(buf + o, nm.c_str(), nm.size() + 1);
      o += nm.size() + 1;
    }
  }
  return EXON_HIP_OK;
}
// FILTER dictionary discovered so far: names are written '\0'-separated into `buf` (id order); returns the count
int exon_hip_vcf_parser_filters(exon_hip_vcf_parser* p, char* buf, size_t cap, int32_t* n_filters) { return exon_vcf_parser_filter_names(p, buf, cap, n_filters, false); }
// on != 0: a row without a value of a String / Character key gets the dictionary id of the EMPTY text (no row can carry it) and
// counts as valid: NULL becomes a group key of its own for a plan that groups by the key.  Off (default): NULL stays NULL.
int exon_hip_vcf_parser_set_null_key(exon_hip_vcf_parser* p, int32_t on) {
  if (!p) return fail(nullptr, EXON_HIP_EINVAL, "exon_hip_vcf_parser_set_null_key: NULL argument");
  p->null_as_value = on ? 1 : 0;
  return EXON_HIP_OK;
}
// the value dictionary of INFO key `key` (its index in the parser's key list; kind 's') in id order
int exon_hip_vcf_parser_info_values(exon_hip_vcf_parser* p, int32_t key, char* buf, size_t cap, int32_t* n_values) { return exon_vcf_parser_info_value_names(p, key, buf, cap, n_values, false); }

}  // extern "C"

int exon_vcf_parser_filter_names(exon_hip_vcf_parser* p, char* buf, size_t cap, int32_t* n_filters, bool so_far) {
  if (!p || !n_filters) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_vcf_parser_filters: NULL argument");
  return table_names(p->ctx, p->filters, "FILTER lists", buf, cap, n_filters, so_far);
}
int exon_vcf_parser_info_value_names(exon_hip_vcf_parser* p, int32_t key, char* buf, size_t cap, int32_t* n_values, bool so_far) {
  if (!p || !n_values) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_vcf_parser_info_values: NULL argument");
  if (key < 0 || key >= p->ik.n || p->ik.kind[key] != 's') return fail(p->ctx, EXON_HIP_EINVAL, "exon_hip_vcf_parser_info_values: key %d is not a String / Character key of this parser", key);
  return table_names(p->ctx, p->str_tables[key], "values of a String INFO key", buf, cap, n_values, so_far);
}

// ------------------------------------------------------------------------------------------------------------
// FASTQ: the newline index above is all the "parsing" a histogram over quality (or sequence) lines needs.  Read r
// is lines 4r .. 4r+3; its views are byte ranges into the slab itself, consumed in place by K5's ragged / fixed
// paths (kernels.hip) -- the text is read from HBM once for the index and once for the histogram.
namespace {

// scalars: [0] n_lines (in), [1] undecided (+=), [2] consumed bytes (out)
__global__ __launch_bounds__(TPB) void k_fastq_views(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl,
                                                     unsigned* __restrict__ scalars, unsigned cap_lines, int final_slab,
                                                     int32_t* __restrict__ seq_s, int32_t* __restrict__ seq_e,
                                                     int32_t* __restrict__ qual_s, int32_t* __restrict__ qual_e, int32_t* __restrict__ head_s,
                                                     int32_t* __restrict__ head_e, unsigned skip) {
  const unsigned n_lines = scalars[0];
  const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (n_lines > cap_lines) {  // the index was truncated: nothing can be trusted
    if (r == 0) atomicAdd(&scalars[1], 1u);
    return;
  }
  const unsigned n_reads = n_lines / 4;
  if (r == 0) {
    scalars[2] = n_reads ? nl[4 * n_reads - 1] + 1u : 0u;
    if (final_slab && (n_lines & 3u)) atomicAdd(&scalars[1], 1u);
  }
  if (r >= n_reads) return;
  const unsigned l0 = r ? nl[4 * r - 1] + 1u : skip;
  const unsigned e0 = nl[4 * r], e1 = nl[4 * r + 1], e2 = nl[4 * r + 2], e3 = nl[4 * r + 3];
  const bool bad = text[l0] != '@' || text[e1 + 1] != '+';
  unsigned se = e1, qe = e3;
  if (se > e0 + 1 && text[se - 1] == '\r') --se;
  if (qe > e2 + 1 && text[qe - 1] == '\r') --qe;
  seq_s[r] = (int32_t)(e0 + 1);
  seq_e[r] = (int32_t)se;
  qual_s[r] = (int32_t)(e2 + 1);
  qual_e[r] = (int32_t)qe;
  unsigned he = e0;  // the header line behind its '@', CR dropped (name + description: exon-fastq/src/array_builder.rs:68-102)
  if (he > l0 + 1 && text[he - 1] == '\r') --he;
  head_s[r] = (int32_t)(l0 + 1);
  head_e[r] = (int32_t)he;
  if (bad) atomicAdd(&scalars[1], 1u);
}

}  // namespace

struct exon_hip_fastq_parser {
  exon_hip_ctx* ctx;
  PoolBufs bufs;
  LineIndex idx;
  int32_t* d_views = nullptr;  // 6 arrays of max_lines / 4 + 1
  size_t per = 0;              // ... that long
  explicit exon_hip_fastq_parser(exon_hip_ctx* c) : ctx(c), bufs(c) {}
};

extern "C" {

int exon_hip_fastq_parser_create(exon_hip_ctx* ctx, int64_t max_bytes, exon_hip_fastq_parser** outp) {
  if (!ctx || !outp || max_bytes < 16) return fail(ctx, EXON_HIP_EINVAL, "exon_hip_fastq_parser_create: bad argument");
  if (max_bytes > 0x7FFF0000LL) return fail(ctx, EXON_HIP_EINVAL, "slab size must stay below 2 GiB (32-bit views)");
  *outp = nullptr;
  exon_hip_fastq_parser* p = new (std::nothrow) exon_hip_fastq_parser(ctx);
  if (!p) return fail(ctx, EXON_HIP_ENOMEM, "out of host memory");
  const int64_t max_lines = max_bytes / 4 + 8;  // records of >= 16 bytes; denser text is handed back to the host decoder
  hipSetDevice(ctx->device);
  p->idx.alloc(p->bufs, max_bytes, max_lines);
  p->per = (size_t)(max_lines / 4 + 1);
  p->d_views = p->bufs.take<int32_t>(p->per * 6 * 4);
  if (p->bufs.status() != hipSuccess) {
    const std::string msg = hipGetErrorString(p->bufs.status());
    delete p;
    return fail(ctx, EXON_HIP_ENOMEM, "fastq parser allocation: %s", msg.c_str());
  }
  *outp = p;
  return EXON_HIP_OK;
}

int exon_hip_fastq_parser_destroy(exon_hip_fastq_parser* p) {
  delete p;
  return EXON_HIP_OK;
}

int exon_hip_fastq_parser_parse(exon_hip_fastq_parser* p, void* stream, const uint8_t* d_text, int64_t n_bytes,
                                int32_t final_slab, exon_hip_fastq_views* views) {
  if (!p || !views || (n_bytes > 0 && !d_text)) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_fastq_parser_parse: NULL argument");
  exon_hip_ctx* ctx = p->ctx;
  memset(views, 0, sizeof *views);
  if (n_bytes == 0) return EXON_HIP_OK;
  LineIndex& idx = p->idx;
  unsigned skip;
  if (int rc = idx.align(ctx, &d_text, &n_bytes, &skip)) return rc;
  hipStream_t s = pick_stream(ctx, stream);
  const size_t per = p->per;
  int32_t* v = p->d_views;
  idx.launch(s, d_text, n_bytes, skip);
  const int64_t read_bound = std::min<int64_t>((int64_t)per, n_bytes / 4 + 1);  // a record holds 4 newlines
  hipLaunchKernelGGL(k_fastq_views, dim3((unsigned)((read_bound + TPB - 1) / TPB)), dim3(TPB), 0, s, d_text, idx.nl, idx.d_scalars,
                     idx.cap, (int)final_slab, v, v + per, v + 2 * per, v + 3 * per, v + 4 * per, v + 5 * per, skip);
  if (int rc = idx.read_back(ctx, s)) return rc;
  views->n_undecided = idx.h_scalars[1];
  views->n_reads = idx.h_scalars[0] > idx.cap ? 0 : idx.h_scalars[0] / 4;
  views->consumed_bytes = idx.consumed(skip);
  views->text_base = d_text;
  views->seq_start = v;
  views->seq_end = v + per;
  views->qual_start = v + 2 * per;
  views->qual_end = v + 3 * per;
  views->head_start = v + 4 * per;
  views->head_end = v + 5 * per;
  return EXON_HIP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------
// FASTA.  THE RULES -- what the host reader returns (host/formats.h: FASTABatchReader + FASTAArrayBuilder; exon-fasta/src/
// batch_reader.rs:72-99, array_builder.rs:114-132), byte for byte; text_columns.hip (exon_text_fasta) builds the columns by them:
//   * Lines end at '\n'.  One '\r' in front of it is dropped -- on definition lines and on sequence lines alike.
//   * A line whose first byte is '>' starts a record; the definition is the rest of that line.
//   * id = the definition up to its first ' ' or '\t' (it may be empty); description = what follows the run of ' ' / '\t' behind
//     the id, NULL when nothing follows.
//   * sequence = every following line up to the next '>' line or the end of the input, concatenated as it stands: inner blanks
//     are kept, empty lines add nothing, a record without sequence lines has "".  A '>' anywhere but at a line's start is a byte
//     of that line like any other.
//   * The host reader skips text in front of the first '>' line; the device never sees such text: exon_hip_scan_bind_ctx refuses
//     an input whose first byte is not '>', and a slab that does not start with '>' is undecided here.
// A record is a variable number of lines and one record may be most of a slab, so nothing here walks a record.  Over the line
// index (LineIndex, as for FASTQ):
//   k_fasta_classify   one thread per line: is_def[line] (first byte '>'), seq_len[line] (0 for a definition line, else the
//                      line's length without its CR)
//   two exclusive scans (list_kernels.h: block sums, one workgroup over them; the in-block prefixes are taken by the kernel
//                      below): the rank of the definition lines is the record number, the prefix of seq_len every line's
//                      destination in the compacted sequence bytes
//   k_fasta_records    one thread per line again: line_dst[line] (written over seq_len, with the total behind the last line);
//                      a definition line writes its record's head_start / head_end and the Arrow offset seq_offsets[record] =
//                      its own scanned value; the closing offset comes from the last definition line (the record it starts is not
//                      emitted) or, in the final slab, from the total
// Slab rules: final_slab == 0 -- the last record is never known to be complete: n_records = definition lines - 1, consumed_bytes
// ends directly in front of the last definition line; fewer than two definition lines consume nothing (scan.cpp hands the file
// over when that slab cannot grow: GpuTextSource carries at most its gap, a quarter of a slab and at least 1 MiB, so a record
// beyond roughly a quarter slab -- 20 MB at the default 80 MB -- is the host reader's: whole chromosomes stay a host format,
// protein sets, transcriptomes, contigs and reads are the device's).  final_slab != 0 -- every record is complete, consumed_bytes
// is the whole text.  Undecided: a first line without '>', or more lines than the index holds.
// LINE CAPACITY: max_slab_bytes / 8 + 8 lines.  FASTA lines are 60 - 80 bytes wide and a one-line-per-record read set has a
// definition of ten bytes or more next to every read, so real files stay below one line per 30 bytes; 8 bytes a line leaves a
// factor of four for short records and costs 20 bytes of index per line = 2.5 bytes per slab byte (the newline position, is_def,
// seq_len / line_dst, and head_start / head_end / seq_offsets sized for a record per line).  Denser text (runs of empty lines,
// sequence wrapped below seven columns) is undecided and goes to the host reader.
namespace {

// scalars: [0] n_lines (in), [1] undecided (+=)
__global__ __launch_bounds__(TPB) void k_fasta_classify(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned* __restrict__ scalars,
                                                        unsigned cap_lines, unsigned skip, uint32_t* __restrict__ is_def, uint32_t* __restrict__ seq_len) {
  const unsigned n_lines = scalars[0];
  const unsigned line = blockIdx.x * TPB + threadIdx.x;
  if (n_lines > cap_lines) {  // the index was truncated: nothing can be trusted
    if (line == 0) atomicAdd(&scalars[1], 1u);
    return;
  }
  if (line >= n_lines) return;
  const unsigned begin = line ? nl[line - 1] + 1u : skip, end = nl[line];  // (begin <= end: text[begin] is the line's first byte or its '\n')
  const bool def = text[begin] == '>';
  unsigned len = end - begin;
  if (len && text[end - 1] == '\r') --len;
  is_def[line] = def ? 1u : 0u;
  seq_len[line] = def ? 0u : len;
  if (line == 0 && !def) atomicAdd(&scalars[1], 1u);
}

// tot: [0] definition lines, [1] sequence bytes of the slab (both from the scans), [2] (out) sequence bytes of the records emitted;
// scalars[2] (out): consumed bytes.  seq_len becomes line_dst in place: a thread reads its own entry and then writes it.
__global__ __launch_bounds__(LIST_TPB) void k_fasta_records(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned* __restrict__ scalars,
                                                            unsigned cap_lines, unsigned skip, int final_slab, const uint32_t* __restrict__ is_def,
                                                            uint32_t* __restrict__ seq_len, const unsigned* __restrict__ def_sums,
                                                            const unsigned* __restrict__ len_sums, unsigned* __restrict__ tot, int32_t* __restrict__ head_s,
                                                            int32_t* __restrict__ head_e, int32_t* __restrict__ seq_off) {
  const unsigned n_lines = scalars[0];
  if (n_lines > cap_lines) return;  // (uniform: k_fasta_classify has counted the slab undecided)
  const unsigned line = blockIdx.x * LIST_TPB + threadIdx.x;
  const bool in = line < n_lines;
  const unsigned d = in ? is_def[line] : 0u, c = in ? seq_len[line] : 0u;
  const unsigned rank = list_first_item(d, def_sums);
  __syncthreads();  // (list_first_item's wave totals are one LDS array: the first call's readers before the second call's writers)
  const unsigned dst = list_first_item(c, len_sums);
  if (!in) return;
  const unsigned n_defs = tot[0];
  const unsigned n_records = final_slab ? n_defs : (n_defs ? n_defs - 1u : 0u);
  const unsigned begin = line ? nl[line - 1] + 1u : skip;
  seq_len[line] = dst;
  if (line == n_lines - 1u) {
    seq_len[n_lines] = dst + c;
    if (final_slab) {
      seq_off[n_records] = (int32_t)(dst + c);
      tot[2] = dst + c;
      scalars[2] = nl[line] + 1u;
    }
  }
  if (!d) return;
  if (rank < n_records) {
    unsigned he = nl[line];
    if (he > begin + 1u && text[he - 1] == '\r') --he;
    head_s[rank] = (int32_t)(begin + 1u);
    head_e[rank] = (int32_t)he;
    seq_off[rank] = (int32_t)dst;
  } else {  // the last definition line of a slab that is not the input's last: the record it starts stays behind
    seq_off[rank] = (int32_t)dst;
    tot[2] = dst;
    scalars[2] = begin;
  }
}

}  // namespace

struct exon_hip_fasta_parser {
  exon_hip_ctx* ctx;
  PoolBufs bufs;
  LineIndex idx;
  uint32_t *is_def = nullptr, *seq_len = nullptr;  // [cap] and [cap + 1] (seq_len turns into line_dst)
  unsigned *def_sums = nullptr, *len_sums = nullptr;
  unsigned *d_tot = nullptr, *h_tot = nullptr;  // device / pinned [4]
  int32_t *head_s = nullptr, *head_e = nullptr, *seq_off = nullptr;  // [cap], [cap], [cap + 1]: a record is a line at least
  explicit exon_hip_fasta_parser(exon_hip_ctx* c) : ctx(c), bufs(c) {}
};

extern "C" {

int exon_hip_fasta_parser_create(exon_hip_ctx* ctx, int64_t max_bytes, exon_hip_fasta_parser** outp) {
  if (!ctx || !outp || max_bytes < 16) return fail(ctx, EXON_HIP_EINVAL, "exon_hip_fasta_parser_create: bad argument");
  if (max_bytes > 0x7FFF0000LL) return fail(ctx, EXON_HIP_EINVAL, "slab size must stay below 2 GiB (32-bit views)");
  *outp = nullptr;
  exon_hip_fasta_parser* p = new (std::nothrow) exon_hip_fasta_parser(ctx);
  if (!p) return fail(ctx, EXON_HIP_ENOMEM, "out of host memory");
  const int64_t max_lines = max_bytes / 8 + 8;  // LINE CAPACITY above; denser text is handed back to the host decoder
  hipSetDevice(ctx->device);
  p->idx.alloc(p->bufs, max_bytes, max_lines);
  const size_t cap = (size_t)max_lines, nb = (cap + LIST_TPB - 1) / LIST_TPB;
  p->is_def = p->bufs.take<uint32_t>(cap * 4);
  p->seq_len = p->bufs.take<uint32_t>((cap + 1) * 4);
  p->def_sums = p->bufs.take<unsigned>((nb + 1) * 4);
  p->len_sums = p->bufs.take<unsigned>((nb + 1) * 4);
  p->d_tot = p->bufs.take<unsigned>(16, 0);
  p->h_tot = p->bufs.pinned<unsigned>(16);
  p->head_s = p->bufs.take<int32_t>(cap * 4);
  p->head_e = p->bufs.take<int32_t>(cap * 4);
  p->seq_off = p->bufs.take<int32_t>((cap + 1) * 4);
  if (p->bufs.status() != hipSuccess) {
    const std::string msg = hipGetErrorString(p->bufs.status());
    delete p;
    return fail(ctx, EXON_HIP_ENOMEM, "fasta parser allocation: %s", msg.c_str());
  }
  *outp = p;
  return EXON_HIP_OK;
}

int exon_hip_fasta_parser_destroy(exon_hip_fasta_parser* p) {
  delete p;
  return EXON_HIP_OK;
}

int exon_hip_fasta_parser_parse(exon_hip_fasta_parser* p, void* stream, const uint8_t* d_text, int64_t n_bytes, int32_t final_slab,
                                exon_hip_fasta_views* views) {
  if (!p || !views || (n_bytes > 0 && !d_text)) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_fasta_parser_parse: NULL argument");
  exon_hip_ctx* ctx = p->ctx;
  memset(views, 0, sizeof *views);
  if (n_bytes == 0) return EXON_HIP_OK;
  LineIndex& idx = p->idx;
  unsigned skip;
  if (int rc = idx.align(ctx, &d_text, &n_bytes, &skip)) return rc;
  hipStream_t s = pick_stream(ctx, stream);
  idx.launch(s, d_text, n_bytes, skip);
  // a line is a byte at least (its '\n'): the launches cover the lines the slab can hold, the kernels read the count on the device
  const unsigned bound = (unsigned)std::min<int64_t>((int64_t)idx.cap, n_bytes);
  const int nb = (int)((bound + LIST_TPB - 1) / LIST_TPB);
  hipLaunchKernelGGL(k_fasta_classify, dim3((bound + TPB - 1) / TPB), dim3(TPB), 0, s, d_text, idx.nl, idx.d_scalars, idx.cap, skip, p->is_def, p->seq_len);
  launch_list_scan(s, p->is_def, idx.d_scalars, idx.cap, nb, p->def_sums, p->d_tot);
  launch_list_scan(s, p->seq_len, idx.d_scalars, idx.cap, nb, p->len_sums, p->d_tot + 1);
  hipLaunchKernelGGL(k_fasta_records, dim3(nb), dim3(LIST_TPB), 0, s, d_text, idx.nl, idx.d_scalars, idx.cap, skip, (int)final_slab, p->is_def, p->seq_len, p->def_sums,
                     p->len_sums, p->d_tot, p->head_s, p->head_e, p->seq_off);
  HIP_TRY(ctx, hipMemcpyAsync(p->h_tot, p->d_tot, 16, hipMemcpyDeviceToHost, s));
  if (int rc = idx.read_back(ctx, s)) return rc;
  views->n_undecided = idx.h_scalars[1];
  views->text_base = d_text;
  views->text_bytes = n_bytes;
  views->first_line_start = skip;
  const unsigned n_lines = idx.h_scalars[0], n_defs = p->h_tot[0];
  if (n_lines == 0 || n_lines > idx.cap || views->n_undecided) return EXON_HIP_OK;  // nothing else was written, or nothing of it counts
  views->n_lines = n_lines;
  views->n_records = final_slab ? n_defs : (n_defs ? n_defs - 1 : 0);
  views->consumed_bytes = idx.consumed(skip);
  views->seq_bytes = p->h_tot[2];
  views->head_start = p->head_s;
  views->head_end = p->head_e;
  views->seq_offsets = p->seq_off;
  views->line_end = idx.nl;
  views->line_dst = p->seq_len;
  return EXON_HIP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------
// SAM text: the first six tab-separated fields of every alignment line -> the BAM device layout (flag, mapq, reference
// id, start, end).  Field rules of host/formats.h's SAM reader (schema of exon-sam/src/schema_builder.rs:371-402, same
// columns as BAM): RNAME through the header's @SQ order ('*' or unknown -> NULL), POS 0 -> NULL, MAPQ 255 -> NULL,
// end = POS + (sum of M/D/N/=/X lengths) - 1.  Lines the device cannot decide (fewer than 6 fields, non-digits in a
// numeric field, header or empty lines in the middle) are counted: the caller decodes on the host instead.
namespace {

struct SamOut {
  int32_t* flag;
  uint8_t* mapq;
  uint8_t* mapq_valid;
  int32_t* ref_id;
  uint8_t* ref_valid;
  int64_t* start;
  int64_t* end;
  uint8_t* pos_valid;
};

__device__ __forceinline__ bool parse_uint(const uint8_t* text, unsigned b, unsigned e, int64_t* out) {
  if (e <= b || e - b > 18) return false;
  int64_t v = 0;
  for (unsigned i = b; i < e; ++i) {
    const uint8_t c = text[i];
    if (c < '0' || c > '9') return false;
    v = v * 10 + (c - '0');
  }
  *out = v;
  return true;
}

__global__ __launch_bounds__(TPB) void k_parse_sam_lines(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl_pos,
                                                         unsigned* __restrict__ scalars, NameTable refs, SamOut out, unsigned cap,
                                                         unsigned skip) {
  const int64_t n_rows = min(scalars[0], cap);
  const int64_t row = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool mq_ok = false, ref_ok = false, pos_ok = false, bad = false;
  if (row < n_rows) {
    const unsigned begin = row ? nl_pos[row - 1] + 1 : skip;
    unsigned end = nl_pos[row];
    if (end > begin && text[end - 1] == '\r') --end;
    unsigned fs[7];
    int nf = 0;
    fs[0] = begin;
    for (unsigned i = begin; i < end && nf < 6; ++i)
      if (text[i] == '\t') fs[++nf] = i + 1;
    auto fbeg = [&](int f) { return fs[f]; };
    auto fend = [&](int f) { return f < nf ? fs[f + 1] - 1 : end; };
    int64_t flag = 0, pos1 = 0, mapq = 0;
    if (begin == end || text[begin] == '@' || nf < 5) {
      bad = true;
    } else if (!parse_uint(text, fbeg(1), fend(1), &flag) || !parse_uint(text, fbeg(3), fend(3), &pos1) ||
               !parse_uint(text, fbeg(4), fend(4), &mapq) || flag > 0xFFFF || mapq > 255 || pos1 > 0x7FFFFFFF) {
      bad = true;
    } else {
      // RNAME
      int id = -1;
      const unsigned rb = fbeg(2), re = fend(2);
      const int len = (int)(re - rb);
      if (!(len == 1 && text[rb] == '*')) {
        const uint64_t h = fnv1a(text + rb, len);
        int slot = (int)(h & (uint64_t)refs.mask);
        for (int probe = 0; probe <= refs.mask; ++probe) {
          const uint64_t k = refs.keys[slot];
          if (k == 0) break;
          if (k == h && (int)refs.text_len[slot] == len) {
            bool same = true;
            for (int i = 0; i < len && same; ++i) same = refs.pool[refs.text_off[slot] + i] == text[rb + i];
            if (same) {
              id = refs.ids[slot];
              break;
            }
          }
          slot = (slot + 1) & refs.mask;
        }
      }
      // CIGAR: reference length
      int64_t ref_len = 0, num = 0;
      const unsigned cb = fbeg(5), ce = fend(5);
      if (!(ce - cb == 1 && text[cb] == '*'))
        for (unsigned i = cb; i < ce; ++i) {
          const uint8_t ch = text[i];
          if (ch >= '0' && ch <= '9') num = num * 10 + (ch - '0');
          else {
            if (ch == 'M' || ch == 'D' || ch == 'N' || ch == '=' || ch == 'X') ref_len += num;
            num = 0;
          }
        }
      out.flag[row] = (int32_t)flag;
      out.mapq[row] = (uint8_t)mapq;
      out.ref_id[row] = id;
      mq_ok = mapq != 255;
      ref_ok = id >= 0;
      pos_ok = pos1 >= 1;
      out.start[row] = pos_ok ? pos1 : 0;
      out.end[row] = pos_ok ? pos1 + ref_len - 1 : 0;
    }
  }
  const int64_t row0 = ((int64_t)blockIdx.x * TPB + threadIdx.x) - lane;
  store_valid(out.mapq_valid, row0, n_rows, mq_ok, lane);
  store_valid(out.ref_valid, row0, n_rows, ref_ok, lane);
  store_valid(out.pos_valid, row0, n_rows, pos_ok, lane);
  const unsigned long long bm = __ballot(bad);
  if (lane == 0 && bm) atomicAdd(&scalars[1], (unsigned)__popcll(bm));
}

}  // namespace

struct exon_hip_sam_parser {
  exon_hip_ctx* ctx;
  PoolBufs bufs;
  int64_t max_rows = 0;
  LineIndex idx;
  NameTable refs{};
  SamOut out{};
  explicit exon_hip_sam_parser(exon_hip_ctx* c) : ctx(c), bufs(c) {}
};
const unsigned* exon_hip_sam_parser_newlines(exon_hip_sam_parser* p) { return p ? p->idx.nl : nullptr; }

extern "C" {

int exon_hip_sam_parser_create(exon_hip_ctx* ctx, const char* const* ref_names, int32_t n_refs, int64_t max_bytes,
                               exon_hip_sam_parser** outp) {
  if (!ctx || !outp || (n_refs > 0 && !ref_names) || max_bytes < 16) return fail(ctx, EXON_HIP_EINVAL, "exon_hip_sam_parser_create: bad argument");
  if (max_bytes > 0xF0000000LL) return fail(ctx, EXON_HIP_EINVAL, "slab size must stay below 4 GiB (32-bit line offsets)");
  *outp = nullptr;
  exon_hip_sam_parser* p = new (std::nothrow) exon_hip_sam_parser(ctx);
  if (!p) return fail(ctx, EXON_HIP_ENOMEM, "out of host memory");
  p->max_rows = max_bytes / 12 + 1;  // 11 fields: >= 21 bytes + newline; be generous
  hipSetDevice(ctx->device);
  PoolBufs& b = p->bufs;
  build_name_table(b, ref_names, n_refs, &p->refs);
  p->idx.alloc(b, max_bytes, p->max_rows);
  const size_t r = (size_t)p->max_rows, rb = r / 8 + 64;
  p->out.flag = b.take<int32_t>(r * 4);
  p->out.mapq = b.take<uint8_t>(r + 64);
  p->out.mapq_valid = b.take<uint8_t>(rb);
  p->out.ref_id = b.take<int32_t>(r * 4);
  p->out.ref_valid = b.take<uint8_t>(rb);
  p->out.start = b.take<int64_t>(r * 8);
  p->out.end = b.take<int64_t>(r * 8);
  p->out.pos_valid = b.take<uint8_t>(rb);
  if (b.status() != hipSuccess) {
    const std::string msg = hipGetErrorString(b.status());
    delete p;
    return fail(ctx, EXON_HIP_ENOMEM, "sam parser allocation: %s", msg.c_str());
  }
  *outp = p;
  return EXON_HIP_OK;
}

int exon_hip_sam_parser_destroy(exon_hip_sam_parser* p) {
  delete p;
  return EXON_HIP_OK;
}

int exon_hip_sam_parser_parse(exon_hip_sam_parser* p, void* stream, const uint8_t* d_text, int64_t n_bytes, exon_hip_bam_columns* cols) {
  if (!p || !cols || (n_bytes > 0 && !d_text)) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_sam_parser_parse: NULL argument");
  exon_hip_ctx* ctx = p->ctx;
  memset(cols, 0, sizeof *cols);
  if (n_bytes == 0) return EXON_HIP_OK;
  LineIndex& idx = p->idx;
  unsigned skip;
  if (int rc = idx.align(ctx, &d_text, &n_bytes, &skip)) return rc;
  hipStream_t s = pick_stream(ctx, stream);
  idx.launch(s, d_text, n_bytes, skip);
  hipLaunchKernelGGL(k_last_newline, dim3(1), dim3(1), 0, s, idx.nl, idx.d_scalars, idx.cap);
  const int64_t row_bound = std::min<int64_t>(p->max_rows, n_bytes / 12 + 1);
  const int pblocks = (int)((row_bound + TPB - 1) / TPB);
  hipLaunchKernelGGL(k_parse_sam_lines, dim3(pblocks), dim3(TPB), 0, s, d_text, idx.nl, idx.d_scalars, p->refs, p->out, (unsigned)row_bound, skip);
  if (int rc = idx.read_back(ctx, s)) return rc;
  const int64_t n_lines = idx.h_scalars[0];
  cols->n_rows = n_lines;
  cols->n_undecided = idx.h_scalars[1] + (n_lines > row_bound ? 1 : 0);
  cols->consumed_bytes = idx.consumed(skip);
  cols->flag = p->out.flag;
  cols->mapq = p->out.mapq;
  cols->mapq_valid = p->out.mapq_valid;
  cols->ref_id = p->out.ref_id;
  cols->ref_valid = p->out.ref_valid;
  cols->start = p->out.start;
  cols->end = p->out.end;
  cols->pos_valid = p->out.pos_valid;
  return EXON_HIP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------
// GFF3 text: the first eight tab-separated fields of every record line -> the GFF device layout (host/gff.h states the line
// rules once; exon-gff/src/array_builder.rs is the schema).  GFF has no header: seqname, source and type are free text whose
// dictionaries are built on the device, each in a FilterTable of its own (claim in the line kernel, k_assign_filters,
// k_remap_filters with the text compare, exactly as the FILTER dictionary).  Lines that start with '#' are no rows, so a row's
// number is its RANK among the lines that are: k_gff_classify marks them, the offsets scan (list_kernels.h) ranks them, and a
// slab without any '#' line -- every slab but a file's first, usually -- takes the identity (row = line, validity by ballot).
// Rows the device cannot decide (a malformed field, more than 18 digits, a float the Eisel-Lemire path leaves open, an empty
// line, a "##FASTA" line, a dictionary past its limits) are counted: the caller decodes the file on the host, which reports.
namespace {

struct GffOut {
  int32_t* id[3];    // seqname, source, type: provisional slot, then the dense id (k_remap_filters)
  uint32_t* off[3];  // where the field's text is in the slab, and its length: k_remap_filters verifies it
  uint32_t* len[3];
  int64_t* start;
  int64_t* end;
  float* score;
  int32_t* strand;
  int32_t* phase;
  uint8_t *score_valid, *strand_valid, *phase_valid;
  uint8_t* vflags;  // ranked slabs: bit 0 score, 1 strand, 2 phase of every row (k_gff_pack_valid makes the bitmaps of them)
};

// scalars: [0] lines (in), [1] undecided (+=), [2] consumed bytes, [3] rows (the offsets scan's total)
__global__ __launch_bounds__(TPB) void k_gff_classify(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl_pos, unsigned* __restrict__ scalars,
                                                      unsigned cap, unsigned skip, uint32_t* __restrict__ is_row) {
  const unsigned n_lines = min(scalars[0], cap);
  const unsigned line = blockIdx.x * TPB + threadIdx.x;
  if (line >= n_lines) return;
  const unsigned begin = line ? nl_pos[line - 1] + 1 : skip, end = nl_pos[line];
  const bool row = text[begin] != '#';  // (an empty line reads its own '\n': a row, and an undecided one)
  is_row[line] = row ? 1u : 0u;
  if (!row && end - begin >= 7u) {
    const uint8_t* p = text + begin;
    if (p[1] == '#' && p[2] == 'F' && p[3] == 'A' && p[4] == 'S' && p[5] == 'T' && p[6] == 'A') atomicAdd(&scalars[1], 1u);
  }
}

// the slot of text [off, off + len) in `t`, claimed if it is new (k_parse_lines' FILTER lookup); -1: the table is full
__device__ __forceinline__ int table_claim(const FilterTable& t, const uint8_t* __restrict__ text, unsigned off, int len) {
  const unsigned long long h = fnv1a(text + off, len);
  int slot = (int)(h & (FILTER_SLOTS - 1));
  for (int probe = 0; probe < FILTER_SLOTS; ++probe) {
    unsigned long long k = t.keys[slot];
    if (k == 0) {
      k = atomicCAS(&t.keys[slot], 0ull, h);
      if (k == 0) {
        t.text_off[slot] = off;
        t.text_len[slot] = (uint32_t)len;
        return slot;
      }
    }
    if (k == h) return slot;
    slot = (slot + 1) & (FILTER_SLOTS - 1);
  }
  atomicExch(&t.counters[2], 1);
  return -1;
}

// start / end: Rust's usize::from_str (one '+', digits) and >= vmin (GFF / GTF: 1; BED is 0-based: 0); up to 18 digits here,
// longer ones are the host's
__device__ __forceinline__ bool gff_position(const uint8_t* __restrict__ text, unsigned pb, unsigned pe, unsigned n_total, uint64_t vmin, int64_t* out) {
  unsigned pn = pe - pb;
  if (pn && text[pb] == '+') ++pb, --pn;
  bool ok = pn > 0 && pn <= 18;
  uint64_t v = 0;  // (unsigned: a spoiled value wraps, it is then not used)
  if (pn <= 16 && pb + 16u <= n_total) {  // the digits from two (unaligned) 8-byte loads, no branch per digit
    uint64_t w[2];
    __builtin_memcpy(w, text + pb, 16);
    for (unsigned k = 0; k < pn; ++k) {
      const unsigned d = ((unsigned)(w[k >> 3] >> (8 * (k & 7))) & 0xFFu) - (unsigned)'0';
      ok &= d <= 9u;
      v = v * 10 + d;
    }
  } else {
    for (unsigned i = pb; i < pb + pn && ok; ++i) {
      const unsigned d = (unsigned)text[i] - (unsigned)'0';
      ok = d <= 9u;
      v = v * 10 + d;
    }
  }
  ok = ok && v >= vmin;
  *out = ok ? (int64_t)v : 0;
  return ok;
}

// ATTR (the scan projects `attributes`): where every row's ninth field lies, for text_columns.hip's k_gff_attr_measure / _fill.
// The two pointers trail the arguments and the ATTR = false instantiation never reads them: its code is the kernel's as it
// was before the column existed.
// GTF (host/gtf.h: the same eight fields by the same rules but one): a '?' strand makes the row undecided.  A compile-time
// dialect, so the GFF instantiations are the code they were.
template <bool ATTR, bool GTF = false>
__global__ __launch_bounds__(TPB) void k_parse_gff_lines(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl_pos, unsigned* __restrict__ scalars,
                                                         const uint32_t* __restrict__ is_row, const unsigned* __restrict__ block_offsets, FilterTable t0,
                                                         FilterTable t1, FilterTable t2, GffOut out, unsigned cap, unsigned skip, unsigned n_total,
                                                         uint32_t* __restrict__ attr_off, uint32_t* __restrict__ attr_len) {
  static_assert(TPB == LIST_TPB, "list_first_item ranks a workgroup of LIST_TPB lines");
  const unsigned n_lines = min(scalars[0], cap), n_rows = scalars[3];
  const bool identity = n_rows == n_lines;  // no '#' line in the slab (the same for every thread of the launch)
  const unsigned line = blockIdx.x * TPB + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const unsigned c = line < n_lines ? is_row[line] : 0u;
  const unsigned row = identity ? line : list_first_item(c, block_offsets);
  auto group16 = [&](unsigned a) {  // an aligned 16-byte group of the slab; the last one byte by byte
    uint4 v = {0, 0, 0, 0};
    if (a + 16u <= n_total) {
      v = *reinterpret_cast<const uint4*>(text + a);
    } else {
      unsigned* w = &v.x;
      for (unsigned i = 0; a + i < n_total; ++i) w[i >> 2] |= (unsigned)text[a + i] << (8 * (i & 3));
    }
    return v;
  };
  bool score_ok = false, strand_ok = false, phase_ok = false, bad = false;
  if (c) {
    const unsigned begin = line ? nl_pos[line - 1] + 1 : skip;
    unsigned end = nl_pos[line];
    if (end > begin && text[end - 1] == '\r') --end;
    unsigned fs[9];  // field f spans [fs[f], fs[f + 1] - 1); the ninth is whatever follows the eighth tab
    int nf = 0;
    fs[0] = begin;
    for (unsigned a = begin & ~15u; a < end && nf < 8; a += 16) {
      unsigned m = clip_mask16(eq_mask16(group16(a), 0x09090909u), a, begin, end);
      while (m && nf < 8) {
        fs[++nf] = a + (unsigned)__ffs((int)m);
        m &= m - 1;
      }
    }
    int64_t start = 0, stop = 0;
    float score = 0.f;
    int32_t strand = 0, phase = 0, slot[3] = {-1, -1, -1};
    if (nf < 8) {
      bad = true;  // an empty line, or fewer than nine fields
      for (int k = 0; k < 9; ++k) fs[k] = begin;  // (the row's slots below get defined values)
    } else {
      slot[0] = table_claim(t0, text, fs[0], (int)(fs[1] - 1 - fs[0]));
      slot[1] = table_claim(t1, text, fs[1], (int)(fs[2] - 1 - fs[1]));
      slot[2] = table_claim(t2, text, fs[2], (int)(fs[3] - 1 - fs[2]));
      bad |= !gff_position(text, fs[3], fs[4] - 1, n_total, 1, &start);
      bad |= !gff_position(text, fs[4], fs[5] - 1, n_total, 1, &stop);
      const int sl = (int)(fs[6] - 1 - fs[5]);
      if (!(sl == 1 && text[fs[5]] == '.')) {
        uint32_t bits;
        if (exon::dec::parse_f32(reinterpret_cast<const char*>(text + fs[5]), sl, &bits)) {
          score = __uint_as_float(bits);
          score_ok = true;
        } else {
          bad = true;  // not a number, or one the host decides (more than 19 digits, inf / nan)
        }
      }
      const unsigned sc = fs[7] - 1 - fs[6] == 1u ? text[fs[6]] : 0u;
      strand_ok = sc == '+' || sc == '-';
      strand = sc == '-' ? 1 : 0;
      bad |= !(strand_ok || sc == '.' || (!GTF && sc == '?'));
      const unsigned pc = fs[8] - 1 - fs[7] == 1u ? text[fs[7]] : 0u;
      phase_ok = pc - (unsigned)'0' <= 2u;
      phase = phase_ok ? (int32_t)(pc - '0') : 0;
      bad |= !(phase_ok || pc == '.');
    }
    for (int k = 0; k < 3; ++k) {
      out.id[k][row] = slot[k];  // -1: no slot, k_remap_filters writes id 0 and compares nothing
      out.off[k][row] = fs[k];
      out.len[k][row] = nf < 8 ? 0u : fs[k + 1] - 1 - fs[k];
    }
    out.start[row] = start;
    out.end[row] = stop;
    out.score[row] = score;
    out.strand[row] = strand;
    out.phase[row] = phase;
    if (ATTR) {  // (a short record: an empty field, the row is undecided anyway)
      attr_off[row] = fs[8];
      attr_len[row] = nf < 8 ? 0u : end - fs[8];
    }
    if (!identity) out.vflags[row] = (uint8_t)((score_ok ? 1 : 0) | (strand_ok ? 2 : 0) | (phase_ok ? 4 : 0));
  }
  if (identity) {
    const int64_t row0 = (int64_t)line - lane;
    store_valid(out.score_valid, row0, n_rows, score_ok, lane);
    store_valid(out.strand_valid, row0, n_rows, strand_ok, lane);
    store_valid(out.phase_valid, row0, n_rows, phase_ok, lane);
  }
  const unsigned long long nb = __ballot(bad);
  if (lane == 0 && nb) atomicAdd(&scalars[1], (unsigned)__popcll(nb));
}

// a ranked slab's validity bitmaps from the rows' flag bytes (nothing to do when the line kernel took the identity)
__global__ __launch_bounds__(256) void k_gff_pack_valid(const unsigned* __restrict__ scalars, unsigned cap, const uint8_t* __restrict__ vflags,
                                                        uint8_t* __restrict__ score_valid, uint8_t* __restrict__ strand_valid, uint8_t* __restrict__ phase_valid) {
  const unsigned n = scalars[3];
  if (n == min(scalars[0], cap)) return;
  for (unsigned b = blockIdx.x * 256 + threadIdx.x; b * 8 < n; b += gridDim.x * 256) {
    unsigned s = 0, t = 0, p = 0;
    for (unsigned k = 0; k < 8 && b * 8 + k < n; ++k) {
      const unsigned f = vflags[b * 8 + k];
      s |= (f & 1u) << k;
      t |= ((f >> 1) & 1u) << k;
      p |= ((f >> 2) & 1u) << k;
    }
    score_valid[b] = (uint8_t)s;
    strand_valid[b] = (uint8_t)t;
    phase_valid[b] = (uint8_t)p;
  }
}

}  // namespace

struct exon_hip_gff_parser {
  exon_hip_ctx* ctx;
  PoolBufs bufs;
  int64_t max_rows = 0;
  LineIndex idx;  // scalars: [0] lines, [1] undecided, [2] consumed bytes, [3] rows
  FilterTable tables[3] = {};
  GffOut out{};
  uint32_t* d_is_row = nullptr;
  unsigned* d_blocks = nullptr;   // per-workgroup sums of is_row (scanned in place)
  int32_t h_stat[3] = {0, 0, 0};  // the dictionaries' overflow flags after the last slab
  // the `attributes` column (exon_hip_gff_parser_want_attributes): every row's ninth field, recorded by the line kernel, and the
  // slab of the last parse call (aligned) for exon_hip_gff_parser_attributes
  bool want_attr = false;
  bool gtf = false;  // exon_hip_gff_parser_set_dialect: the GTF line rules and its attributes column
  PoolBufs attr_bufs;  // (of their own: a failed allocation is released and does not stick to the parser's)
  uint32_t *d_attr_off = nullptr, *d_attr_len = nullptr;
  ExonTextScratch* attr_scratch = nullptr;
  const uint8_t* last_text = nullptr;
  int64_t last_bytes = 0, last_rows = -1;
  explicit exon_hip_gff_parser(exon_hip_ctx* c) : ctx(c), bufs(c), attr_bufs(c) {}
  ~exon_hip_gff_parser() { exon_text_scratch_destroy(attr_scratch); }
};

// names[i] -> id i of a device-built dictionary before the first slab: keys, ids, the text pool and the two claim counters
static int seed_filter_table(exon_hip_ctx* ctx, PoolBufs& b, const FilterTable& t, const char* const* names, int32_t n) {
  if (n <= 0) return EXON_HIP_OK;
  if (n > EXON_HIP_MAX_GROUPS) return fail(ctx, EXON_HIP_EINVAL, "%d seed names: a device-built dictionary holds %d", n, EXON_HIP_MAX_GROUPS);
  std::vector<unsigned long long> keys(FILTER_SLOTS, 0);
  std::vector<int32_t> ids(FILTER_SLOTS, -1);
  std::vector<uint32_t> toff(FILTER_SLOTS, 0), tlen(FILTER_SLOTS, 0);
  std::string pool;
  for (int32_t i = 0; i < n; ++i) {
    const std::string nm = names[i] ? names[i] : "";
    if (pool.size() + nm.size() > (size_t)FILTER_POOL) return fail(ctx, EXON_HIP_EINVAL, "seed names exceed the dictionary's %d-byte text pool", FILTER_POOL);
    const unsigned long long h = fnv1a(reinterpret_cast<const uint8_t*>(nm.data()), (int)nm.size());
    int slot = (int)(h & (FILTER_SLOTS - 1));
    while (keys[(size_t)slot] != 0) {
      if (keys[(size_t)slot] == h) return fail(ctx, EXON_HIP_EINVAL, "seed name '%s' is given twice (or hashes like another)", nm.c_str());
      slot = (slot + 1) & (FILTER_SLOTS - 1);
    }
    keys[(size_t)slot] = h;
    ids[(size_t)slot] = i;
    toff[(size_t)slot] = (uint32_t)pool.size();
    tlen[(size_t)slot] = (uint32_t)nm.size();
    pool += nm;
  }
  const int32_t counters[4] = {n, (int32_t)pool.size(), 0, 0};
  b.upload(t.keys, keys.data(), FILTER_SLOTS * 8);
  b.upload(t.ids, ids.data(), FILTER_SLOTS * 4);
  b.upload(t.text_off, toff.data(), FILTER_SLOTS * 4);
  b.upload(t.text_len, tlen.data(), FILTER_SLOTS * 4);
  b.upload(t.pool, pool.data(), pool.size());
  b.upload(t.counters, counters, sizeof counters);
  return EXON_HIP_OK;
}

extern "C" {

int exon_hip_gff_parser_create(exon_hip_ctx* ctx, const char* const* seed_seqnames, int32_t n_seed, int64_t max_bytes, exon_hip_gff_parser** outp) {
  if (!ctx || !outp || n_seed < 0 || (n_seed > 0 && !seed_seqnames) || max_bytes < 16) return fail(ctx, EXON_HIP_EINVAL, "exon_hip_gff_parser_create: bad argument");
  if (max_bytes > 0xF0000000LL) return fail(ctx, EXON_HIP_EINVAL, "slab size must stay below 4 GiB (32-bit line offsets)");
  *outp = nullptr;
  exon_hip_gff_parser* p = new (std::nothrow) exon_hip_gff_parser(ctx);
  if (!p) return fail(ctx, EXON_HIP_ENOMEM, "out of host memory");
  p->max_rows = max_bytes / 16 + 1;  // a record has eight tabs and eight fields of a byte or more in front of its newline; a slab of
                                     // shorter lines ('#' comments, empty lines) than that on average is handed to the host reader
  hipSetDevice(ctx->device);
  PoolBufs& b = p->bufs;
  for (auto& t : p->tables) t = take_filter_table(b);
  p->idx.alloc(b, max_bytes, p->max_rows);
  const size_t r = (size_t)p->max_rows, rb = r / 8 + 64;
  for (int k = 0; k < 3; ++k) {
    p->out.id[k] = b.take<int32_t>(r * 4);
    p->out.off[k] = b.take<uint32_t>(r * 4);
    p->out.len[k] = b.take<uint32_t>(r * 4);
  }
  p->out.start = b.take<int64_t>(r * 8);
  p->out.end = b.take<int64_t>(r * 8);
  p->out.score = b.take<float>(r * 4);
  p->out.strand = b.take<int32_t>(r * 4);
  p->out.phase = b.take<int32_t>(r * 4);
  p->out.score_valid = b.take<uint8_t>(rb);
  p->out.strand_valid = b.take<uint8_t>(rb);
  p->out.phase_valid = b.take<uint8_t>(rb);
  p->out.vflags = b.take<uint8_t>(r + 64);
  p->d_is_row = b.take<uint32_t>(r * 4);
  p->d_blocks = b.take<unsigned>((r / LIST_TPB + 2) * 4);
  int rc = EXON_HIP_OK;
  if (b.status() == hipSuccess) rc = seed_filter_table(ctx, b, p->tables[0], seed_seqnames, n_seed);
  if (rc) {
    delete p;
    return rc;
  }
  if (b.status() != hipSuccess) {
    const std::string msg = hipGetErrorString(b.status());
    delete p;
    return fail(ctx, EXON_HIP_ENOMEM, "gff parser allocation: %s", msg.c_str());
  }
  *outp = p;
  return EXON_HIP_OK;
}

int exon_hip_gff_parser_destroy(exon_hip_gff_parser* p) {
  delete p;
  return EXON_HIP_OK;
}

int exon_hip_gff_parser_parse(exon_hip_gff_parser* p, void* stream, const uint8_t* d_text, int64_t n_bytes, exon_hip_gff_columns* cols) {
  if (!p || !cols || (n_bytes > 0 && !d_text)) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_gff_parser_parse: NULL argument");
  exon_hip_ctx* ctx = p->ctx;
  memset(cols, 0, sizeof *cols);
  if (n_bytes == 0) return EXON_HIP_OK;
  LineIndex& idx = p->idx;
  unsigned skip;
  if (int rc = idx.align(ctx, &d_text, &n_bytes, &skip)) return rc;
  hipStream_t s = pick_stream(ctx, stream);
  idx.launch(s, d_text, n_bytes, skip);
  hipLaunchKernelGGL(k_last_newline, dim3(1), dim3(1), 0, s, idx.nl, idx.d_scalars, idx.cap);
  const int64_t row_bound = std::min<int64_t>(p->max_rows, n_bytes / 16 + 1);
  const int pblocks = (int)((row_bound + TPB - 1) / TPB);
  const GffOut& o = p->out;
  hipLaunchKernelGGL(k_gff_classify, dim3(pblocks), dim3(TPB), 0, s, d_text, idx.nl, idx.d_scalars, (unsigned)row_bound, skip, p->d_is_row);
  launch_list_scan(s, p->d_is_row, idx.d_scalars, (unsigned)row_bound, pblocks, p->d_blocks, idx.d_scalars + 3);
  auto* const line_kernel = p->gtf ? (p->want_attr ? k_parse_gff_lines<true, true> : k_parse_gff_lines<false, true>)
                                   : (p->want_attr ? k_parse_gff_lines<true, false> : k_parse_gff_lines<false, false>);
  hipLaunchKernelGGL(line_kernel, dim3(pblocks), dim3(TPB), 0, s, d_text, idx.nl, idx.d_scalars, p->d_is_row, p->d_blocks, p->tables[0], p->tables[1], p->tables[2], o,
                     (unsigned)row_bound, skip, (unsigned)n_bytes, p->want_attr ? p->d_attr_off : (uint32_t*)nullptr, p->want_attr ? p->d_attr_len : (uint32_t*)nullptr);
  hipLaunchKernelGGL(k_gff_pack_valid, dim3(std::min(pblocks, 1024)), dim3(256), 0, s, idx.d_scalars, (unsigned)row_bound, o.vflags, o.score_valid,
                     o.strand_valid, o.phase_valid);
  for (int k = 0; k < 3; ++k) {
    hipLaunchKernelGGL(k_assign_filters, dim3(1), dim3(256), 0, s, d_text, p->tables[k]);
    hipLaunchKernelGGL(k_remap_filters, dim3(std::min(pblocks, 4096)), dim3(TPB), 0, s, o.id[k], idx.d_scalars + 3, (unsigned)row_bound, p->tables[k], d_text,
                       o.off[k], o.len[k], (const uint8_t*)nullptr);
    HIP_TRY(ctx, hipMemcpyAsync(&p->h_stat[k], p->tables[k].counters + 2, 4, hipMemcpyDeviceToHost, s));  // overflow or collision
  }
  if (int rc = idx.read_back(ctx, s)) return rc;
  const int64_t n_lines = idx.h_scalars[0];
  cols->n_rows = idx.h_scalars[3];
  cols->n_undecided = idx.h_scalars[1] + (n_lines > row_bound ? 1 : 0);  // more lines than the slab's bytes allow for records: the host reader's
  for (int k = 0; k < 3; ++k) cols->n_undecided += p->h_stat[k] ? 1 : 0;  // a dictionary past its limits (or two texts that hash alike)
  cols->consumed_bytes = idx.consumed(skip);
  p->last_text = d_text;
  p->last_bytes = n_bytes;
  p->last_rows = p->want_attr && cols->n_undecided == 0 ? cols->n_rows : -1;
  cols->seqname_id = o.id[0];
  cols->source_id = o.id[1];
  cols->type_id = o.id[2];
  cols->start = o.start;
  cols->end = o.end;
  cols->score = o.score;
  cols->score_valid = o.score_valid;
  cols->strand_id = o.strand;
  cols->strand_valid = o.strand_valid;
  cols->phase_id = o.phase;
  cols->phase_valid = o.phase_valid;
  return EXON_HIP_OK;
}

int exon_hip_gff_parser_want_attributes(exon_hip_gff_parser* p, int32_t on) {
  if (!p) return fail(nullptr, EXON_HIP_EINVAL, "exon_hip_gff_parser_want_attributes: NULL argument");
  if (on && !p->d_attr_off) {
    hipSetDevice(p->ctx->device);
    p->d_attr_off = p->attr_bufs.take<uint32_t>((size_t)p->max_rows * 4);
    p->d_attr_len = p->attr_bufs.take<uint32_t>((size_t)p->max_rows * 4);
    if (p->attr_bufs.status() != hipSuccess) {
      (void)hipGetLastError();
      p->attr_bufs.release();
      p->d_attr_off = p->d_attr_len = nullptr;
      return fail(p->ctx, EXON_HIP_ENOMEM, "gff parser: the rows' attribute fields (%lld rows)", (long long)p->max_rows);
    }
  }
  p->want_attr = on != 0;
  p->last_rows = -1;
  return EXON_HIP_OK;
}

int exon_hip_gff_parser_attributes(exon_hip_gff_parser* p, void* stream, exon_hip_gff_attributes* out) {
  if (!p || !out) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_gff_parser_attributes: NULL argument");
  memset(out, 0, sizeof *out);
  if (p->gtf) return fail(p->ctx, EXON_HIP_ESTATE, "exon_hip_gff_parser_attributes: the parser reads GTF (exon_hip_gff_parser_gtf_attributes builds its Map<Utf8, Utf8>)");
  if (p->last_rows < 0)
    return fail(p->ctx, EXON_HIP_ESTATE, "exon_hip_gff_parser_attributes: no slab to build from (call exon_hip_gff_parser_want_attributes, then parse; a slab with undecided rows has none)");
  ExonTextColumns t;
  int64_t und = 0;
  if (int rc = exon_text_gff(p->ctx, stream, &p->attr_scratch, p->last_text, p->last_bytes, p->d_attr_off, p->d_attr_len, p->last_rows, &t, &und)) return rc;
  HIP_TRY(p->ctx, hipStreamSynchronize(pick_stream(p->ctx, stream)));
  out->n_undecided = und;
  if (und || !t.n_roots) return EXON_HIP_OK;  // (a slab of no rows has no column)
  const ExonTextNode &map = t.nodes[t.roots[0]], &entries = t.nodes[map.kid[0]], &keys = t.nodes[entries.kid[0]], &lists = t.nodes[entries.kid[1]], &items = t.nodes[lists.kid[0]];
  out->n_entries = entries.length;
  out->n_items = items.length;
  out->n_key_bytes = keys.n_values;
  out->n_item_bytes = items.n_values;
  out->map_offsets = map.offsets;
  out->key_offsets = keys.offsets;
  out->key_values = static_cast<const uint8_t*>(keys.values);
  out->list_offsets = lists.offsets;
  out->item_offsets = items.offsets;
  out->item_values = static_cast<const uint8_t*>(items.values);
  return EXON_HIP_OK;
}

int exon_hip_gff_parser_set_dialect(exon_hip_gff_parser* p, int32_t format) {
  if (!p || (format != EXON_HIP_FORMAT_GFF && format != EXON_HIP_FORMAT_GTF))
    return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_gff_parser_set_dialect: EXON_HIP_FORMAT_GFF or EXON_HIP_FORMAT_GTF");
  p->gtf = format == EXON_HIP_FORMAT_GTF;
  p->last_rows = -1;
  return EXON_HIP_OK;
}

int exon_hip_gff_parser_gtf_attributes(exon_hip_gff_parser* p, void* stream, exon_hip_gtf_attributes* out) {
  if (!p || !out) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_gff_parser_gtf_attributes: NULL argument");
  memset(out, 0, sizeof *out);
  if (!p->gtf) return fail(p->ctx, EXON_HIP_ESTATE, "exon_hip_gff_parser_gtf_attributes: the parser reads GFF3 (exon_hip_gff_parser_set_dialect)");
  if (p->last_rows < 0)
    return fail(p->ctx, EXON_HIP_ESTATE, "exon_hip_gff_parser_gtf_attributes: no slab to build from (call exon_hip_gff_parser_want_attributes, then parse; a slab with undecided rows has none)");
  ExonTextColumns t;
  int64_t und = 0;
  if (int rc = exon_text_gtf(p->ctx, stream, &p->attr_scratch, p->last_text, p->last_bytes, p->d_attr_off, p->d_attr_len, p->last_rows, &t, &und)) return rc;
  HIP_TRY(p->ctx, hipStreamSynchronize(pick_stream(p->ctx, stream)));
  out->n_undecided = und;
  if (und || !t.n_roots) return EXON_HIP_OK;  // (a slab of no rows has no column)
  const ExonTextNode &map = t.nodes[t.roots[0]], &entries = t.nodes[map.kid[0]], &keys = t.nodes[entries.kid[0]], &values = t.nodes[entries.kid[1]];
  out->n_entries = entries.length;
  out->n_key_bytes = keys.n_values;
  out->n_value_bytes = values.n_values;
  out->map_offsets = map.offsets;
  out->key_offsets = keys.offsets;
  out->key_values = static_cast<const uint8_t*>(keys.values);
  out->value_offsets = values.offsets;
  out->value_values = static_cast<const uint8_t*>(values.values);
  return EXON_HIP_OK;
}

// the dictionary of column 0 (seqname), 1 (source) or 2 (type) discovered so far, '\0'-separated in id order
int exon_hip_gff_parser_names(exon_hip_gff_parser* p, int32_t column, char* buf, size_t cap, int32_t* n_names) { return exon_gff_parser_column_names(p, column, buf, cap, n_names, false); }

}  // extern "C"

void exon_hip_gff_parser_attr_fields(exon_hip_gff_parser* p, const uint8_t** text, int64_t* n_bytes, const uint32_t** off, const uint32_t** len) {
  *text = p->last_text;
  *n_bytes = p->last_bytes;
  *off = p->d_attr_off;
  *len = p->d_attr_len;
}

int exon_gff_parser_column_names(exon_hip_gff_parser* p, int32_t column, char* buf, size_t cap, int32_t* n_names, bool so_far) {
  if (!p || !n_names || column < 0 || column > 2) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_gff_parser_names: bad argument");
  static const char* const what[3] = {"seqnames", "sources", "feature types"};
  return table_names(p->ctx, p->tables[column], what[column], buf, cap, n_names, so_far);
}

// ------------------------------------------------------------------------------------------------------------
// BED text: every line decoded by its own field count -> the BED device layout (host/bed.h states the line rules once;
// exon-bed/src/schema.rs is the schema, batch_reader.rs:92-231 the decode by field count).  The shape is k_parse_gff_lines': one
// line per lane, '#' lines ranked away (k_gff_classify, the offsets scan; the identity when the slab has none), column 0 a
// dictionary built on the device (table_claim, k_assign_filters, k_remap_filters).  What differs: the WHOLE line is scanned --
// the field count must be exact up to the 13th TAB, and any byte >= 0x80 makes the row undecided (the line must be valid UTF-8,
// ignored fields included: the host's to check) -- and the same 16-byte groups give both masks.  Everything the rules call an
// error, and a position of more than 18 digits, is an undecided row: the host reader raises the error with the line quoted.
namespace {

struct BedOut {
  int32_t* id;    // reference_sequence_name: provisional slot, then the dense id (k_remap_filters)
  uint32_t* off;  // where the field's text is in the slab, and its length: k_remap_filters verifies it
  uint32_t* len;
  int64_t* start;
  int64_t* end;
  // PROJ only (exon_hip_bed_parser_want):
  int64_t* score;
  int32_t* strand;
  uint32_t* name_off;
  uint32_t* name_len;
  uint8_t *score_valid, *strand_valid, *name_valid;
  uint8_t* vflags;  // ranked slabs: bit 0 score, 1 strand, 2 name of every row (k_gff_pack_valid makes the bitmaps of them)
};

// bit b = byte b of the 16-byte group is >= 0x80
__device__ __forceinline__ unsigned high_mask16(const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t t = (w[k] & 0x80808080u) >> 7;  // bits 0, 8, 16, 24
    mask |= ((t | (t >> 7) | (t >> 14) | (t >> 21)) & 0xFu) << (4 * k);
  }
  return mask;
}

// PROJ = false (a fused plan: K2 / K6 / K7 read columns 0, 1, 2): the three operand columns and nothing else; the line is
// validated in full all the same.
template <bool PROJ>
__global__ __launch_bounds__(TPB) void k_parse_bed_lines(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl_pos, unsigned* __restrict__ scalars,
                                                         const uint32_t* __restrict__ is_row, const unsigned* __restrict__ block_offsets, FilterTable t0, BedOut out,
                                                         unsigned cap, unsigned skip, unsigned n_total) {
  static_assert(TPB == LIST_TPB, "list_first_item ranks a workgroup of LIST_TPB lines");
  const unsigned n_lines = min(scalars[0], cap), n_rows = scalars[3];
  const bool identity = n_rows == n_lines;  // no '#' line in the slab (the same for every thread of the launch)
  const unsigned line = blockIdx.x * TPB + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const unsigned c = line < n_lines ? is_row[line] : 0u;
  const unsigned row = identity ? line : list_first_item(c, block_offsets);
  auto group16 = [&](unsigned a) {  // an aligned 16-byte group of the slab; the last one byte by byte
    uint4 v = {0, 0, 0, 0};
    if (a + 16u <= n_total) {
      v = *reinterpret_cast<const uint4*>(text + a);
    } else {
      unsigned* w = &v.x;
      for (unsigned i = 0; a + i < n_total; ++i) w[i >> 2] |= (unsigned)text[a + i] << (8 * (i & 3));
    }
    return v;
  };
  bool score_ok = false, strand_ok = false, name_ok = false, bad = false;
  if (c) {
    const unsigned begin = line ? nl_pos[line - 1] + 1 : skip;
    unsigned end = nl_pos[line];
    if (end > begin && text[end - 1] == '\r') --end;
    unsigned fs[7];  // field f (0..5) spans [fs[f], fs[f + 1] - 1)
    int nt = 0;      // TABs seen, up to 13: the field count is nt + 1
    unsigned high = 0;
    fs[0] = begin;
    for (unsigned a = begin & ~15u; a < end && nt < 13; a += 16) {
      const uint4 v = group16(a);
      unsigned m = clip_mask16(eq_mask16(v, 0x09090909u), a, begin, end);
      high |= clip_mask16(high_mask16(v), a, begin, end);
      while (m) {
        if (nt < 6) fs[nt + 1] = a + (unsigned)__ffs((int)m);
        ++nt;
        m &= m - 1;
      }
    }
    const int nf = nt + 1;
    const bool counted = nf == 3 || nf == 4 || nf == 5 || nf == 6 || nf == 12;
    bad = !counted || high != 0;  // (13 TABs end the scan early: the row is undecided whatever lies behind them)
    int64_t start = 0, stop = 0, score = 0;
    int32_t strand = 0, slot = -1;
    unsigned name_off = begin, name_len = 0;
    if (!counted) {
      for (int k = 0; k < 7; ++k) fs[k] = begin;  // (the row's slots below get defined values)
    } else {
      if (nt < 6) fs[nt + 1] = end + 1;  // the last field ends at the line's end
      slot = table_claim(t0, text, fs[0], (int)(fs[1] - 1 - fs[0]));
      bad |= !gff_position(text, fs[1], fs[2] - 1, n_total, 0, &start);
      bad |= !gff_position(text, fs[2], fs[3] - 1, n_total, 0, &stop);
      if (nf >= 5) {
        name_ok = true;
        name_off = fs[3];
        name_len = fs[4] - 1 - fs[3];
        unsigned sb = fs[4], sn = fs[5] - 1 - fs[4];  // u16::from_str: one '+', digits; more than 5 digits (leading zeros) are the host's
        if (sn && text[sb] == '+') ++sb, --sn;
        score_ok = sn >= 1 && sn <= 5;
        unsigned v = 0;
        for (unsigned i = 0; i < sn && score_ok; ++i) {
          const unsigned d = (unsigned)text[sb + i] - (unsigned)'0';
          score_ok = d <= 9u;
          v = v * 10 + d;
        }
        score_ok = score_ok && v <= 65535u;
        score = score_ok ? (int64_t)v : 0;
        bad |= !score_ok;
      }
      if (nf >= 6) {
        const unsigned sc = fs[6] - 1 - fs[5] == 1u ? text[fs[5]] : 0u;
        strand_ok = sc == '+' || sc == '-';
        strand = sc == '-' ? 1 : 0;
        bad |= !(strand_ok || sc == '.');
      }
    }
    out.id[row] = slot;  // -1: no slot, k_remap_filters writes id 0 and compares nothing
    out.off[row] = fs[0];
    out.len[row] = counted ? fs[1] - 1 - fs[0] : 0u;
    out.start[row] = start;
    out.end[row] = stop;
    if (PROJ) {
      out.score[row] = score;
      out.strand[row] = strand;
      out.name_off[row] = name_off;
      out.name_len[row] = name_len;
      if (!identity) out.vflags[row] = (uint8_t)((score_ok ? 1 : 0) | (strand_ok ? 2 : 0) | (name_ok ? 4 : 0));
    }
  }
  if (PROJ && identity) {
    const int64_t row0 = (int64_t)line - lane;
    store_valid(out.score_valid, row0, n_rows, score_ok, lane);
    store_valid(out.strand_valid, row0, n_rows, strand_ok, lane);
    store_valid(out.name_valid, row0, n_rows, name_ok, lane);
  }
  const unsigned long long nb = __ballot(bad);
  if (lane == 0 && nb) atomicAdd(&scalars[1], (unsigned)__popcll(nb));
}

}  // namespace

struct exon_hip_bed_parser {
  exon_hip_ctx* ctx;
  PoolBufs bufs;
  int64_t max_rows = 0;
  LineIndex idx;  // scalars: [0] lines, [1] undecided, [2] consumed bytes, [3] rows
  FilterTable table = {};
  BedOut out{};
  uint32_t* d_is_row = nullptr;
  unsigned* d_blocks = nullptr;  // per-workgroup sums of is_row (scanned in place)
  int32_t h_stat = 0;            // the dictionary's overflow flag after the last slab
  bool proj = false;             // exon_hip_bed_parser_want: score, strand and the names' places
  const uint8_t* last_text = nullptr;  // the slab of the last parse call (aligned), for the scan's `name` column
  int64_t last_bytes = 0;
  PoolBufs proj_bufs;            // (of their own: a failed allocation is released and does not stick to the parser's)
  explicit exon_hip_bed_parser(exon_hip_ctx* c) : ctx(c), bufs(c), proj_bufs(c) {}
};

extern "C" {

int exon_hip_bed_parser_create(exon_hip_ctx* ctx, const char* const* seed_names, int32_t n_seed, int64_t max_bytes, exon_hip_bed_parser** outp) {
  if (!ctx || !outp || n_seed < 0 || (n_seed > 0 && !seed_names) || max_bytes < 16) return fail(ctx, EXON_HIP_EINVAL, "exon_hip_bed_parser_create: bad argument");
  if (max_bytes > 0xF0000000LL) return fail(ctx, EXON_HIP_EINVAL, "slab size must stay below 4 GiB (32-bit line offsets)");
  *outp = nullptr;
  exon_hip_bed_parser* p = new (std::nothrow) exon_hip_bed_parser(ctx);
  if (!p) return fail(ctx, EXON_HIP_ENOMEM, "out of host memory");
  p->max_rows = max_bytes / 8 + 1;  // "chr1", two positions, two tabs and the newline are nine bytes; a slab of shorter lines than
                                    // eight bytes on average ('#' alone, empty lines, one-letter names) is handed to the host reader
  hipSetDevice(ctx->device);
  PoolBufs& b = p->bufs;
  p->table = take_filter_table(b);
  p->idx.alloc(b, max_bytes, p->max_rows);
  const size_t r = (size_t)p->max_rows;
  p->out.id = b.take<int32_t>(r * 4);
  p->out.off = b.take<uint32_t>(r * 4);
  p->out.len = b.take<uint32_t>(r * 4);
  p->out.start = b.take<int64_t>(r * 8);
  p->out.end = b.take<int64_t>(r * 8);
  p->d_is_row = b.take<uint32_t>(r * 4);
  p->d_blocks = b.take<unsigned>((r / LIST_TPB + 2) * 4);
  int rc = EXON_HIP_OK;
  if (b.status() == hipSuccess) rc = seed_filter_table(ctx, b, p->table, seed_names, n_seed);
  if (rc) {
    delete p;
    return rc;
  }
  if (b.status() != hipSuccess) {
    const std::string msg = hipGetErrorString(b.status());
    delete p;
    return fail(ctx, EXON_HIP_ENOMEM, "bed parser allocation: %s", msg.c_str());
  }
  *outp = p;
  return EXON_HIP_OK;
}

int exon_hip_bed_parser_destroy(exon_hip_bed_parser* p) {
  delete p;
  return EXON_HIP_OK;
}

int exon_hip_bed_parser_want(exon_hip_bed_parser* p, uint64_t projection) {
  if (!p) return fail(nullptr, EXON_HIP_EINVAL, "exon_hip_bed_parser_want: NULL argument");
  if (projection & ~0xFF8ull) return fail(p->ctx, EXON_HIP_EUNSUPPORTED, "exon_hip_bed_parser_want: projection 0x%llx (EXON_HIP_PROJECT_BED_*: bits 3 .. 11)", (unsigned long long)projection);
  const bool on = (projection & (EXON_HIP_PROJECT_BED_NAME | EXON_HIP_PROJECT_BED_SCORE | EXON_HIP_PROJECT_BED_STRAND)) != 0;  // (columns 6 .. 11 are NULL: nothing to parse)
  if (on && !p->out.score) {
    hipSetDevice(p->ctx->device);
    PoolBufs& b = p->proj_bufs;
    const size_t r = (size_t)p->max_rows, rb = r / 8 + 64;
    BedOut& o = p->out;
    o.score = b.take<int64_t>(r * 8);
    o.strand = b.take<int32_t>(r * 4);
    o.name_off = b.take<uint32_t>(r * 4);
    o.name_len = b.take<uint32_t>(r * 4);
    o.score_valid = b.take<uint8_t>(rb);
    o.strand_valid = b.take<uint8_t>(rb);
    o.name_valid = b.take<uint8_t>(rb);
    o.vflags = b.take<uint8_t>(r + 64);
    if (b.status() != hipSuccess) {
      (void)hipGetLastError();
      b.release();
      o.score = nullptr;
      return fail(p->ctx, EXON_HIP_ENOMEM, "bed parser: the projected columns (%lld rows)", (long long)p->max_rows);
    }
  }
  p->proj = on;
  return EXON_HIP_OK;
}

int exon_hip_bed_parser_parse(exon_hip_bed_parser* p, void* stream, const uint8_t* d_text, int64_t n_bytes, exon_hip_bed_columns* cols) {
  if (!p || !cols || (n_bytes > 0 && !d_text)) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_bed_parser_parse: NULL argument");
  exon_hip_ctx* ctx = p->ctx;
  memset(cols, 0, sizeof *cols);
  if (n_bytes == 0) return EXON_HIP_OK;
  LineIndex& idx = p->idx;
  unsigned skip;
  if (int rc = idx.align(ctx, &d_text, &n_bytes, &skip)) return rc;
  hipStream_t s = pick_stream(ctx, stream);
  idx.launch(s, d_text, n_bytes, skip);
  hipLaunchKernelGGL(k_last_newline, dim3(1), dim3(1), 0, s, idx.nl, idx.d_scalars, idx.cap);
  const int64_t row_bound = std::min<int64_t>(p->max_rows, n_bytes / 8 + 1);
  const int pblocks = (int)((row_bound + TPB - 1) / TPB);
  const BedOut& o = p->out;
  hipLaunchKernelGGL(k_gff_classify, dim3(pblocks), dim3(TPB), 0, s, d_text, idx.nl, idx.d_scalars, (unsigned)row_bound, skip, p->d_is_row);
  launch_list_scan(s, p->d_is_row, idx.d_scalars, (unsigned)row_bound, pblocks, p->d_blocks, idx.d_scalars + 3);
  hipLaunchKernelGGL(p->proj ? k_parse_bed_lines<true> : k_parse_bed_lines<false>, dim3(pblocks), dim3(TPB), 0, s, d_text, idx.nl, idx.d_scalars, p->d_is_row, p->d_blocks,
                     p->table, o, (unsigned)row_bound, skip, (unsigned)n_bytes);
  if (p->proj)
    hipLaunchKernelGGL(k_gff_pack_valid, dim3(std::min(pblocks, 1024)), dim3(256), 0, s, idx.d_scalars, (unsigned)row_bound, o.vflags, o.score_valid, o.strand_valid,
                       o.name_valid);
  hipLaunchKernelGGL(k_assign_filters, dim3(1), dim3(256), 0, s, d_text, p->table);
  hipLaunchKernelGGL(k_remap_filters, dim3(std::min(pblocks, 4096)), dim3(TPB), 0, s, o.id, idx.d_scalars + 3, (unsigned)row_bound, p->table, d_text, o.off, o.len,
                     (const uint8_t*)nullptr);
  HIP_TRY(ctx, hipMemcpyAsync(&p->h_stat, p->table.counters + 2, 4, hipMemcpyDeviceToHost, s));  // overflow or collision
  if (int rc = idx.read_back(ctx, s)) return rc;
  const int64_t n_lines = idx.h_scalars[0];
  cols->n_rows = idx.h_scalars[3];
  cols->n_undecided = idx.h_scalars[1] + (n_lines > row_bound ? 1 : 0);  // more lines than the slab's bytes allow for records: the host reader's
  cols->n_undecided += p->h_stat ? 1 : 0;                                // the dictionary past its limits (or two texts that hash alike)
  cols->consumed_bytes = idx.consumed(skip);
  p->last_text = d_text;
  p->last_bytes = n_bytes;
  cols->chrom_id = o.id;
  cols->start = o.start;
  cols->end = o.end;
  if (p->proj) {
    cols->score = o.score;
    cols->score_valid = o.score_valid;
    cols->strand_id = o.strand;
    cols->strand_valid = o.strand_valid;
    cols->name_off = o.name_off;
    cols->name_len = o.name_len;
    cols->name_valid = o.name_valid;
    cols->text = d_text;
  }
  return EXON_HIP_OK;
}

// the reference_sequence_name dictionary discovered so far, '\0'-separated in id order
int exon_hip_bed_parser_names(exon_hip_bed_parser* p, char* buf, size_t cap, int32_t* n_names) { return exon_bed_parser_reference_names(p, buf, cap, n_names, false); }

}  // extern "C"

void exon_hip_bed_parser_name_fields(exon_hip_bed_parser* p, const uint8_t** text, int64_t* n_bytes, const uint32_t** off, const uint32_t** len, const uint8_t** valid) {
  *text = p->last_text;
  *n_bytes = p->last_bytes;
  *off = p->proj ? p->out.name_off : nullptr;
  *len = p->proj ? p->out.name_len : nullptr;
  *valid = p->proj ? p->out.name_valid : nullptr;
}

int exon_bed_parser_reference_names(exon_hip_bed_parser* p, char* buf, size_t cap, int32_t* n_names, bool so_far) {
  if (!p || !n_names) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_bed_parser_names: bad argument");
  return table_names(p->ctx, p->table, "reference sequence names", buf, cap, n_names, so_far);
}
