// take_rows.hip -- the rows a pushed-down predicate (a VCF value comparison, a BAM / SAM flag / mapping-quality test) keeps, taken out of a slab's columns ON THE DEVICE, so that only they cross
// PCIe and the batches still go out as views (scan.cpp: export_slab).  Free of formats: a fixed-width column is a width (SlabLayout),
// a text column a tree of ExonTextNode kinds (host/text_nodes.h); the host's row-by-row counterpart is slab_gather / text_gather.
//   exon_take_index   row mask -> rows[K], the kept row indices in ascending order (k_mask_block_counts, the shared block scan of
//                     list_kernels.h, k_mask_rows_fill); K stays on the device for everything behind it and comes back once
//   exon_take_fixed   out[i] = in[rows[i]] for widths 1, 4, 8 (k_take_fixed); validity and Flag bitmaps bit by bit (k_take_bits)
//   exon_text_take    one recursion over the node tree, the mirror of text_gather: UTF8 = lengths of the kept rows, scanned into new
//                     offsets, spans copied by copy_run (a thread to a row, or 16 lanes to a row where rows are long); LIST = item counts scanned into new offsets and the kept rows' item ranges
//                     expanded into an ascending item-index list, which is the child's `rows`.  A LIST over an INT64 leaf (BAM / SAM
//                     quality_score, List<Int64>) builds no such list: its items are whole spans of 8-byte values, which
//                     k_take_item_spans copies span by span, 16 lanes to a row (128 bytes a step).  Every count of a level below the
//                     rows is known on the device only: the kernels are launched over the INPUT's capacity and read their count
//                     from the device (as launch_list_scan takes n_rows_p); the totals come back in one small copy at the end.
// Every write is bounded by the destination's capacity and every index is checked against its source's length before use -- never
// out of range by construction (a compacted buffer is no larger than its input, and the scratch is sized from the inputs: the table
// above text_columns.hip's scratch_for), but checked, as k_bed_name_fill and VcfInfoFill are.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>

#include "internal.h"
#include "list_kernels.h"

namespace {

constexpr int TAKE_TPB = LIST_TPB;  // 256: four waves, the block the shared scan's in-block prefix (list_first_item) is written for
constexpr int TAKE_RES_WORDS = 2 * ExonTextColumns::MAX_NODES + 2;
constexpr int64_t TAKE_WIDE_MEAN_BYTES = 32;  // a UTF8 column whose rows are this long on average is copied 16 lanes to a row (k_take_spans_wide)

// bit r of a bitmap
__device__ __forceinline__ bool bit_of(const uint8_t* __restrict__ bm, unsigned r) { return (bm[r >> 3] >> (r & 7)) & 1; }

// ---- mask -> rows -------------------------------------------------------------------------------------------------------------------
// kept rows of every block of TAKE_TPB rows: a ballot and a popcount per wave
__global__ __launch_bounds__(TAKE_TPB) void k_mask_block_counts(const uint8_t* __restrict__ mask, unsigned n, unsigned* __restrict__ block_sums) {
  __shared__ unsigned red[TAKE_TPB / 64];
  const unsigned r = blockIdx.x * TAKE_TPB + threadIdx.x;
  const unsigned long long m = __ballot(r < n && bit_of(mask, r));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (unsigned)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_sums[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// block_offsets: the scanned block sums.  Every kept row writes its index at base + (kept rows below it in its wave)
__global__ __launch_bounds__(TAKE_TPB) void k_mask_rows_fill(const uint8_t* __restrict__ mask, unsigned n, const unsigned* __restrict__ block_offsets,
                                                             uint32_t* __restrict__ rows, unsigned cap) {
  __shared__ unsigned wave_tot[TAKE_TPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned r = blockIdx.x * TAKE_TPB + threadIdx.x;
  const bool keep = r < n && bit_of(mask, r);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_tot[wave] = (unsigned)__popcll(m);
  __syncthreads();
  unsigned base = block_offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) base += wave_tot[w];
  const unsigned at = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
  if (keep && at < cap) rows[at] = r;
}

// ---- fixed-width columns ------------------------------------------------------------------------------------------------------------
// out[i] = in[rows[i]], i < min(*n_p, cap); the indices ascend, so a wave's loads are monotone.  n_in: the rows `in` holds
template <typename T>
__global__ __launch_bounds__(TAKE_TPB) void k_take_fixed(const T* __restrict__ in, const uint32_t* __restrict__ rows, const unsigned* __restrict__ n_p, unsigned cap,
                                                         unsigned n_in, T* __restrict__ out) {
  const unsigned n = min(*n_p, cap);
  for (unsigned i = blockIdx.x * TAKE_TPB + threadIdx.x; i < n; i += gridDim.x * TAKE_TPB) {
    const unsigned r = rows[i];
    if (r < n_in) out[i] = in[r];
  }
}
// bit i of out = bit rows[i] of in: whole waves, 8 bytes of bitmap per ballot
__global__ __launch_bounds__(TAKE_TPB) void k_take_bits(const uint8_t* __restrict__ in, const uint32_t* __restrict__ rows, const unsigned* __restrict__ n_p, unsigned cap,
                                                        unsigned n_in, uint8_t* __restrict__ out) {
  const unsigned n = min(*n_p, cap);
  const unsigned n64 = (n + 63u) & ~63u;
  const unsigned lane = threadIdx.x & 63;
  for (unsigned i = blockIdx.x * TAKE_TPB + threadIdx.x; i < n64; i += gridDim.x * TAKE_TPB) {
    bool b = false;
    if (i < n) {
      const unsigned r = rows[i];
      b = r < n_in && bit_of(in, r);
    }
    const unsigned long long m = __ballot(b);
    if (lane < 8) {
      const unsigned i0 = i - lane + lane * 8;
      if (i0 < n) out[i0 >> 3] = (uint8_t)(m >> (lane * 8));
    }
  }
}

// ---- text columns -------------------------------------------------------------------------------------------------------------------
// len[i] = off[rows[i] + 1] - off[rows[i]]: a kept row's bytes (UTF8) or items (LIST)
__global__ __launch_bounds__(TAKE_TPB) void k_take_len(const int32_t* __restrict__ off, const uint32_t* __restrict__ rows, const unsigned* __restrict__ n_p, unsigned cap,
                                                       unsigned n_in, uint32_t* __restrict__ len) {
  const unsigned n = min(*n_p, cap);
  for (unsigned i = blockIdx.x * TAKE_TPB + threadIdx.x; i < n; i += gridDim.x * TAKE_TPB) {
    const unsigned r = rows[i];
    int32_t c = 0;
    if (r < n_in) c = off[r + 1] - off[r];
    len[i] = c > 0 ? (uint32_t)c : 0u;
  }
}
// the scanned lengths as Arrow offsets [n + 1] (k_write_offsets of text_columns.hip with its count on the device)
__global__ __launch_bounds__(TAKE_TPB) void k_take_offsets(const uint32_t* __restrict__ len, const unsigned* __restrict__ n_p, unsigned cap,
                                                           const unsigned* __restrict__ block_offsets, int32_t* __restrict__ offsets) {
  const unsigned n = min(*n_p, cap);
  const unsigned i = blockIdx.x * TAKE_TPB + threadIdx.x;
  const unsigned c = i < n ? len[i] : 0u;
  const unsigned first = list_first_item(c, block_offsets);
  if (i < n) offsets[i] = (int32_t)first;
  if (i + 1 == n) offsets[n] = (int32_t)(first + c);
  if (n == 0 && i == 0) offsets[0] = 0;
}
// the kept rows' spans of `in` back to back in `out`
__global__ __launch_bounds__(TAKE_TPB) void k_take_spans(const uint8_t* __restrict__ in, unsigned in_bytes, const int32_t* __restrict__ off, const uint32_t* __restrict__ rows,
                                                         const unsigned* __restrict__ n_p, unsigned cap, unsigned n_in, const int32_t* __restrict__ new_off,
                                                         uint8_t* __restrict__ out, unsigned out_cap) {
  const unsigned n = min(*n_p, cap);
  for (unsigned i = blockIdx.x * TAKE_TPB + threadIdx.x; i < n; i += gridDim.x * TAKE_TPB) {
    const unsigned r = rows[i];
    if (r >= n_in) continue;
    const unsigned a = (unsigned)off[r], o = (unsigned)new_off[i], c = (unsigned)(new_off[i + 1] - new_off[i]);
    if ((uint64_t)a + c <= in_bytes && (uint64_t)o + c <= out_cap) copy_run(out + o, in + a, c);
  }
}
// the same for a column of LONG rows (BAM / SAM `sequence`: a read's 100-250 bases), k_take_item_spans' shape over bytes: 16 lanes to
// a kept row, lane l moves bytes [8 l, 8 l + 8) of every 128.  exon_text_take picks it by the input's mean row length
// (TAKE_WIDE_MEAN_BYTES); short rows -- every VCF column, names, CIGARs -- keep k_take_spans, where a row is one or two 8-byte steps
__global__ __launch_bounds__(TAKE_TPB) void k_take_spans_wide(const uint8_t* __restrict__ in, unsigned in_bytes, const int32_t* __restrict__ off,
                                                              const uint32_t* __restrict__ rows, const unsigned* __restrict__ n_p, unsigned cap, unsigned n_in,
                                                              const int32_t* __restrict__ new_off, uint8_t* __restrict__ out, unsigned out_cap) {
  constexpr unsigned GROUP = 16, GROUPS = TAKE_TPB / GROUP;
  const unsigned n = min(*n_p, cap);
  const unsigned l = threadIdx.x & (GROUP - 1);
  for (unsigned i = blockIdx.x * GROUPS + threadIdx.x / GROUP; i < n; i += gridDim.x * GROUPS) {
    const unsigned r = rows[i];
    if (r >= n_in) continue;
    const unsigned a = (unsigned)off[r], o = (unsigned)new_off[i], c = (unsigned)(new_off[i + 1] - new_off[i]);
    if ((uint64_t)a + c > in_bytes || (uint64_t)o + c > out_cap) continue;
    for (unsigned j = l * 8; j < c; j += GROUP * 8) copy_run(out + o + j, in + a + j, min(8u, c - j));
  }
}
// the kept rows' item ranges as an ascending list of item indices: the child's `rows`
__global__ __launch_bounds__(TAKE_TPB) void k_take_items(const int32_t* __restrict__ off, const uint32_t* __restrict__ rows, const unsigned* __restrict__ n_p, unsigned cap,
                                                         unsigned n_in, const int32_t* __restrict__ new_off, unsigned n_items_in, uint32_t* __restrict__ item_rows) {
  const unsigned n = min(*n_p, cap);
  for (unsigned i = blockIdx.x * TAKE_TPB + threadIdx.x; i < n; i += gridDim.x * TAKE_TPB) {
    const unsigned r = rows[i];
    if (r >= n_in) continue;
    const unsigned a = (unsigned)off[r], o = (unsigned)new_off[i], c = (unsigned)(new_off[i + 1] - new_off[i]);
    for (unsigned j = 0; j < c; ++j)
      if (a + j < n_items_in && o + j < n_items_in) item_rows[o + j] = a + j;  // (kept items are no more than the items there are)
  }
}

// the kept rows' item spans of an INT64 leaf back to back in `out`: [off[r], off[r + 1]) -> [new_off[i], new_off[i + 1]).  A group of 16
// lanes (one DPP row) owns a kept row and lane l moves items l, l + 16, ...: a group's step is one 128-byte line on either side, where
// one thread per row would walk a read's 100-250 qualities alone.  n_items_in: the items `in` holds; out_cap: the items `out` holds
__global__ __launch_bounds__(TAKE_TPB) void k_take_item_spans(const uint64_t* __restrict__ in, unsigned n_items_in, const int32_t* __restrict__ off,
                                                              const uint32_t* __restrict__ rows, const unsigned* __restrict__ n_p, unsigned cap, unsigned n_in,
                                                              const int32_t* __restrict__ new_off, uint64_t* __restrict__ out, unsigned out_cap) {
  constexpr unsigned GROUP = 16, GROUPS = TAKE_TPB / GROUP;
  const unsigned n = min(*n_p, cap);
  const unsigned l = threadIdx.x & (GROUP - 1);
  for (unsigned i = blockIdx.x * GROUPS + threadIdx.x / GROUP; i < n; i += gridDim.x * GROUPS) {
    const unsigned r = rows[i];
    if (r >= n_in) continue;
    const unsigned a = (unsigned)off[r], o = (unsigned)new_off[i], c = (unsigned)(new_off[i + 1] - new_off[i]);
    if ((uint64_t)a + c > n_items_in || (uint64_t)o + c > out_cap) continue;
    for (unsigned j = l; j < c; j += GROUP) out[o + j] = in[a + j];
  }
}

unsigned grid_of(size_t cap) { return (unsigned)std::min<size_t>(std::max<size_t>((cap + TAKE_TPB - 1) / TAKE_TPB, 1), 2048); }

// one device buffer, grown on demand, handed out in 256-byte-aligned parts
struct TakeBuf {
  PoolBufs bufs;
  uint8_t* base = nullptr;
  size_t cap = 0, used = 0;
  explicit TakeBuf(exon_hip_ctx* ctx) : bufs(ctx) {}
  // room for `need` bytes, nothing handed out yet (the stream is drained before an old buffer goes: the copies of the slab before may read it)
  bool reset(hipStream_t hs, size_t need) {
    used = 0;
    if (cap >= need) return true;
    if (base && hipStreamSynchronize(hs) != hipSuccess) return false;
    bufs.release();
    base = nullptr;
    cap = 0;
    const size_t want = need + need / 4 + 4096;
    base = bufs.take<uint8_t>(want);
    if (!base) {
      (void)hipGetLastError();
      bufs.release();
      return false;
    }
    cap = want;
    return true;
  }
  static size_t part(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  template <class T>
  T* take(size_t bytes) {
    const size_t b = part(bytes);
    if (used + b > cap) return nullptr;  // (never: reset() was given the sum of the parts)
    T* p = reinterpret_cast<T*>(base + used);
    used += b;
    return p;
  }
};

}  // namespace

struct ExonTakeScratch {
  TakeBuf index, fixed, text;
  PoolBufs host;
  unsigned* h_res = nullptr;  // pinned [TAKE_RES_WORDS]
  // of the last exon_take_index
  uint32_t* rows = nullptr;
  unsigned* d_K = nullptr;
  unsigned n_rows = 0;
  explicit ExonTakeScratch(exon_hip_ctx* ctx) : index(ctx), fixed(ctx), text(ctx), host(ctx) {}
};

void exon_take_scratch_destroy(ExonTakeScratch* s) { delete s; }

int exon_take_index(exon_hip_ctx* ctx, void* stream, ExonTakeScratch** sp, const uint8_t* d_mask, int64_t n_rows, const uint32_t** d_rows, const unsigned** d_K,
                    int64_t* K) {
  if (n_rows <= 0 || n_rows > (int64_t)0x7FFFFFFF) return fail(ctx, EXON_HIP_EINVAL, "exon_take_index: %lld rows", (long long)n_rows);
  hipStream_t hs = pick_stream(ctx, stream);
  hipSetDevice(ctx->device);
  if (!*sp) {
    ExonTakeScratch* s = new (std::nothrow) ExonTakeScratch(ctx);
    if (!s) return fail(ctx, EXON_HIP_ENOMEM, "out of host memory");
    s->h_res = s->host.pinned<unsigned>(TAKE_RES_WORDS * 4);
    if (!s->h_res) {
      (void)hipGetLastError();
      delete s;
      return fail(ctx, EXON_HIP_ENOMEM, "pinned result words of the take-rows step");
    }
    *sp = s;
  }
  ExonTakeScratch* s = *sp;
  const unsigned n = (unsigned)n_rows;
  const int nb = (int)((n + TAKE_TPB - 1) / TAKE_TPB);
  const size_t rows_bytes = ((size_t)n + 64) * 4, sums_bytes = ((size_t)nb + 4) * 4;
  if (!s->index.reset(hs, TakeBuf::part(rows_bytes) + TakeBuf::part(sums_bytes) + TakeBuf::part(16)))
    return fail(ctx, EXON_HIP_ENOMEM, "row list of a slab of %u rows", n);
  s->rows = s->index.take<uint32_t>(rows_bytes);
  unsigned* sums = s->index.take<unsigned>(sums_bytes);
  s->d_K = s->index.take<unsigned>(16);
  s->n_rows = n;
  hipLaunchKernelGGL(k_mask_block_counts, dim3(nb), dim3(TAKE_TPB), 0, hs, d_mask, n, sums);
  hipLaunchKernelGGL(k_list_scan_blocks, dim3(1), dim3(256), 0, hs, sums, nb, s->d_K);
  hipLaunchKernelGGL(k_mask_rows_fill, dim3(nb), dim3(TAKE_TPB), 0, hs, d_mask, n, sums, s->rows, n);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(s->h_res, s->d_K, 4, hipMemcpyDeviceToHost, hs));
  HIP_TRY(ctx, hipStreamSynchronize(hs));
  if (s->h_res[0] > n) return fail(ctx, EXON_HIP_ESTATE, "take-rows: %u rows kept of %u", s->h_res[0], n);  // (never)
  *d_rows = s->rows;
  *d_K = s->d_K;
  *K = s->h_res[0];
  return EXON_HIP_OK;
}

int exon_take_fixed(exon_hip_ctx* ctx, void* stream, ExonTakeScratch* s, ExonTakeColumn* cols, int n_cols) {
  if (!s || !s->rows) return fail(ctx, EXON_HIP_ESTATE, "exon_take_fixed before exon_take_index");
  hipStream_t hs = pick_stream(ctx, stream);
  const unsigned n = s->n_rows;
  const size_t bits_bytes = (size_t)n / 8 + 64;
  size_t need = 0;
  for (int c = 0; c < n_cols; ++c) {
    if (cols[c].width != 0 && cols[c].width != 1 && cols[c].width != 4 && cols[c].width != 8) return fail(ctx, EXON_HIP_EINVAL, "exon_take_fixed: a column %d bytes wide", cols[c].width);
    if (cols[c].width && cols[c].values) need += TakeBuf::part((size_t)n * (size_t)cols[c].width + 64);
    if (cols[c].validity) need += TakeBuf::part(bits_bytes);
  }
  if (!s->fixed.reset(hs, need)) return fail(ctx, EXON_HIP_ENOMEM, "taken columns of a slab of %u rows", n);
  const unsigned grid = grid_of(n);
  for (int c = 0; c < n_cols; ++c) {
    ExonTakeColumn& col = cols[c];
    col.out_values = nullptr;
    col.out_validity = nullptr;
    if (col.validity) {
      col.out_validity = s->fixed.take<uint8_t>(bits_bytes);
      hipLaunchKernelGGL(k_take_bits, dim3(grid), dim3(TAKE_TPB), 0, hs, col.validity, s->rows, s->d_K, n, n, col.out_validity);
    }
    if (!col.width || !col.values) continue;
    void* out = s->fixed.take<uint8_t>((size_t)n * (size_t)col.width + 64);
    col.out_values = out;
    if (col.width == 1)
      hipLaunchKernelGGL(k_take_fixed<uint8_t>, dim3(grid), dim3(TAKE_TPB), 0, hs, static_cast<const uint8_t*>(col.values), s->rows, s->d_K, n, n, static_cast<uint8_t*>(out));
    else if (col.width == 4)
      hipLaunchKernelGGL(k_take_fixed<uint32_t>, dim3(grid), dim3(TAKE_TPB), 0, hs, static_cast<const uint32_t*>(col.values), s->rows, s->d_K, n, n, static_cast<uint32_t*>(out));
    else
      hipLaunchKernelGGL(k_take_fixed<uint64_t>, dim3(grid), dim3(TAKE_TPB), 0, hs, static_cast<const uint64_t*>(col.values), s->rows, s->d_K, n, n, static_cast<uint64_t*>(out));
  }
  HIP_TRY(ctx, hipGetLastError());
  return EXON_HIP_OK;
}

namespace {

// one exon_text_take: the recursion's state
struct TextTake {
  hipStream_t hs;
  ExonTakeScratch* s;
  const ExonTextColumns* in;
  ExonTextColumns* out;
  unsigned* res;  // device [TAKE_RES_WORDS]: word 0 the rows kept, then a total per node that has one
  int n_res = 1;
  int len_word[ExonTextColumns::MAX_NODES], val_word[ExonTextColumns::MAX_NODES];  // by OUT node: where its length / its bytes are in res (-1: 0)
  bool short_buffer = false;
};
// (never: text_need adds up the very parts take_node takes) -- no kernel is launched on a part that was not had
int short_of(TextTake& t) {
  t.short_buffer = true;
  return -1;
}
// the device buffers node i and everything below it take, for rows lists of up to `cap` entries
size_t text_need(const ExonTextColumns& in, int i, size_t cap) {
  const ExonTextNode& nd = in.nodes[i];
  size_t need = 0;
  if (nd.validity) need += TakeBuf::part(cap / 8 + 64);
  if (nd.offsets) need += TakeBuf::part((cap + 64) * 4) + TakeBuf::part((cap + 65) * 4) + TakeBuf::part((cap / TAKE_TPB + 4) * 4);  // lengths, offsets, block sums
  if (nd.kind == ExonTextNode::UTF8 && nd.offsets) need += TakeBuf::part((size_t)nd.n_values + 64);
  if (nd.kind == ExonTextNode::LIST && nd.offsets && nd.kid[0] >= 0) {
    const size_t items = (size_t)in.nodes[nd.kid[0]].length;
    if (in.nodes[nd.kid[0]].kind == ExonTextNode::INT64) need += TakeBuf::part((items + 8) * 8);  // the kept spans of 8-byte items; no index list
    else need += TakeBuf::part((items + 64) * 4) + text_need(in, nd.kid[0], items);
  }
  return need;
}
// node i of `in` (UTF8 or LIST, an INT64 leaf is taken by its LIST: exon_text_take has looked) at rows[0 .. *d_n) (at most `cap` of them; the node's own length is what the rows index) -> its node in `out`
int take_node(TextTake& t, int i, const uint32_t* rows, const unsigned* d_n, int n_word, unsigned cap) {
  const ExonTextNode& nd = t.in->nodes[i];
  const unsigned n_in = (unsigned)nd.length;
  const unsigned grid = grid_of(cap);
  const int nb = (int)((cap + TAKE_TPB - 1) / TAKE_TPB);
  ExonTextNode o = nd;
  o.kid[0] = o.kid[1] = -1;
  o.length = 0;
  o.n_values = 0;
  int items_word = -1, bytes_word = -1;
  if (nd.validity) {
    uint8_t* v = t.s->text.take<uint8_t>((size_t)cap / 8 + 64);
    if (!v) return short_of(t);
    hipLaunchKernelGGL(k_take_bits, dim3(grid), dim3(TAKE_TPB), 0, t.hs, nd.validity, rows, d_n, cap, n_in, v);
    o.validity = v;
  }
  int32_t* new_off = nullptr;
  if (nd.offsets) {  // lengths of the kept rows -> new offsets, their total -> a result word
    uint32_t* len = t.s->text.take<uint32_t>(((size_t)cap + 64) * 4);
    new_off = t.s->text.take<int32_t>(((size_t)cap + 65) * 4);
    unsigned* sums = t.s->text.take<unsigned>(((size_t)cap / TAKE_TPB + 4) * 4);
    if (!len || !new_off || !sums || t.n_res >= TAKE_RES_WORDS) return short_of(t);
    const int w = t.n_res++;
    hipLaunchKernelGGL(k_take_len, dim3(grid), dim3(TAKE_TPB), 0, t.hs, nd.offsets, rows, d_n, cap, n_in, len);
    launch_list_scan(t.hs, len, d_n, cap, std::max(nb, 1), sums, t.res + w);
    hipLaunchKernelGGL(k_take_offsets, dim3(std::max(nb, 1)), dim3(TAKE_TPB), 0, t.hs, len, d_n, cap, sums, new_off);
    o.offsets = new_off;
    (nd.kind == ExonTextNode::UTF8 ? bytes_word : items_word) = w;
  }
  int kid = -1;
  if (nd.kind == ExonTextNode::UTF8) {
    if (nd.offsets && nd.values) {
      const unsigned in_bytes = (unsigned)nd.n_values;
      uint8_t* v = t.s->text.take<uint8_t>((size_t)in_bytes + 64);
      if (!v) return short_of(t);
      if (nd.n_values >= TAKE_WIDE_MEAN_BYTES * nd.length)
        hipLaunchKernelGGL(k_take_spans_wide, dim3(grid_of((size_t)cap * 16)), dim3(TAKE_TPB), 0, t.hs, static_cast<const uint8_t*>(nd.values), in_bytes, nd.offsets, rows, d_n, cap, n_in,
                           new_off, v, in_bytes);
      else
        hipLaunchKernelGGL(k_take_spans, dim3(grid), dim3(TAKE_TPB), 0, t.hs, static_cast<const uint8_t*>(nd.values), in_bytes, nd.offsets, rows, d_n, cap, n_in, new_off, v, in_bytes);
      o.values = v;
    }
  } else if (nd.kid[0] >= 0) {
    if (nd.offsets && t.in->nodes[nd.kid[0]].kind == ExonTextNode::INT64) {  // List<Int64>: the kept rows' spans of 8-byte items, copied as spans
      const ExonTextNode& leaf = t.in->nodes[nd.kid[0]];
      const unsigned items_in = (unsigned)leaf.length;
      uint64_t* v = t.s->text.take<uint64_t>(((size_t)items_in + 8) * 8);
      if (!v) return short_of(t);
      if (leaf.values)
        hipLaunchKernelGGL(k_take_item_spans, dim3(grid_of((size_t)cap * 16)), dim3(TAKE_TPB), 0, t.hs, static_cast<const uint64_t*>(leaf.values), items_in, nd.offsets, rows, d_n, cap,
                           n_in, new_off, v, items_in);
      ExonTextNode ol = leaf;
      ol.values = v;
      ol.length = ol.n_values = 0;
      kid = t.out->add(ol);
      if (kid >= 0) t.len_word[kid] = t.val_word[kid] = items_word;  // (an INT64 node's n_values is its length)
    } else if (nd.offsets) {  // the kept rows' items, by index, are the child's rows
      const unsigned items_in = (unsigned)t.in->nodes[nd.kid[0]].length;
      uint32_t* item_rows = t.s->text.take<uint32_t>(((size_t)items_in + 64) * 4);
      if (!item_rows) return short_of(t);
      hipLaunchKernelGGL(k_take_items, dim3(grid), dim3(TAKE_TPB), 0, t.hs, nd.offsets, rows, d_n, cap, n_in, new_off, items_in, item_rows);
      kid = take_node(t, nd.kid[0], item_rows, t.res + items_word, items_word, items_in);
    } else {  // a LIST without offsets has no items: its child goes over as it is
      kid = t.out->add(t.in->nodes[nd.kid[0]]);
      if (kid >= 0) t.len_word[kid] = t.val_word[kid] = -1;
    }
    if (kid < 0) return -1;
  }
  o.kid[0] = (int8_t)kid;
  const int at = t.out->add(o);
  if (at >= 0) {
    t.len_word[at] = n_word;
    t.val_word[at] = bytes_word;
  }
  return at;
}

}  // namespace

int exon_text_take(exon_hip_ctx* ctx, void* stream, ExonTakeScratch* s, const ExonTextColumns& in, const uint32_t* d_rows, const unsigned* d_K, ExonTextColumns* out) {
  *out = ExonTextColumns();
  if (!s || !s->h_res) return fail(ctx, EXON_HIP_ESTATE, "exon_text_take before exon_take_index");
  if (in.n_roots == 0) return EXON_HIP_OK;
  for (int i = 0; i < in.n_nodes; ++i)  // STRUCT2: no format with a map has a predicate
    if (in.nodes[i].kind == ExonTextNode::STRUCT2) return fail(ctx, EXON_HIP_EUNSUPPORTED, "take-rows of a struct (map) column on the device");
  for (int i = 0; i < in.n_nodes; ++i) {  // an INT64 node is the item leaf of a LIST (BAM / SAM quality_score), never a column or a UTF8 node's child
    const ExonTextNode& nd = in.nodes[i];
    const bool int64_kid = nd.kid[0] >= 0 && nd.kid[0] < in.n_nodes && in.nodes[nd.kid[0]].kind == ExonTextNode::INT64;
    if (int64_kid && nd.kind != ExonTextNode::LIST) return fail(ctx, EXON_HIP_EUNSUPPORTED, "take-rows of an Int64 node that is no list's items");
    if (nd.kind == ExonTextNode::INT64 && (nd.length < 0 || nd.length > (int64_t)0x7FFFFFFF)) return fail(ctx, EXON_HIP_EINVAL, "exon_text_take: %lld list items", (long long)nd.length);
  }
  for (int k = 0; k < in.n_roots; ++k)
    if (in.nodes[in.roots[k]].kind == ExonTextNode::INT64) return fail(ctx, EXON_HIP_EUNSUPPORTED, "take-rows of a bare Int64 text column on the device");
  hipStream_t hs = pick_stream(ctx, stream);
  hipSetDevice(ctx->device);
  size_t need = TakeBuf::part(TAKE_RES_WORDS * 4);
  unsigned cap = 0;
  for (int k = 0; k < in.n_roots; ++k) {
    const ExonTextNode& root = in.nodes[in.roots[k]];
    if (root.length <= 0 || root.length > (int64_t)0x7FFFFFFF || root.n_values > (int64_t)0x7FFFFFFF) return fail(ctx, EXON_HIP_EINVAL, "exon_text_take: a column of %lld rows", (long long)root.length);
    cap = std::max(cap, (unsigned)root.length);
    need += text_need(in, in.roots[k], (size_t)root.length);
  }
  if (!s->text.reset(hs, need)) return fail(ctx, EXON_HIP_ENOMEM, "taken string columns of a slab of %u rows", cap);
  TextTake t{hs, s, &in, out, s->text.take<unsigned>(TAKE_RES_WORDS * 4)};
  HIP_TRY(ctx, hipMemsetAsync(t.res, 0, TAKE_RES_WORDS * 4, hs));
  HIP_TRY(ctx, hipMemcpyAsync(t.res, d_K, 4, hipMemcpyDeviceToDevice, hs));
  for (int k = 0; k < in.n_roots; ++k) {
    const int at = take_node(t, in.roots[k], d_rows, d_K, 0, (unsigned)in.nodes[in.roots[k]].length);
    if (t.short_buffer) return fail(ctx, EXON_HIP_ESTATE, "take-rows: the scratch of a slab's string columns is smaller than its parts");
    out->root(at);
  }
  HIP_TRY(ctx, hipGetLastError());
  if (out->overflow || t.n_res > TAKE_RES_WORDS) return fail(ctx, EXON_HIP_ESTATE, "more device-built text columns than ExonTextColumns holds");
  // ONE readback: the rows kept and every level's total
  HIP_TRY(ctx, hipMemcpyAsync(s->h_res, t.res, TAKE_RES_WORDS * 4, hipMemcpyDeviceToHost, hs));
  HIP_TRY(ctx, hipStreamSynchronize(hs));
  for (int i = 0; i < out->n_nodes; ++i) {
    ExonTextNode& nd = out->nodes[i];
    nd.length = t.len_word[i] >= 0 ? (int64_t)s->h_res[t.len_word[i]] : 0;
    nd.n_values = t.val_word[i] >= 0 ? (int64_t)s->h_res[t.val_word[i]] : 0;
  }
  return EXON_HIP_OK;
}
