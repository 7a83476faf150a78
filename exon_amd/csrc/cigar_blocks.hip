// cigar_blocks.hip -- alignment rows -> their aligned blocks as rows (ref_id, start, end) for the coverage plans (kinds 12 - 14):
// exon_hip_cigar_blocks (list form), the ctx-free exon_hip_cigar_blocks_host, and the stage between the BAM / SAM device parsers and
// the plans of a blocks-mode scan (exon_cigar_blocks_slab; exon_hip_scan_set_cover_ops).  DESIGN.md 3.9.  A translation unit of its
// own: nothing here is seen by the fused kernels, which read block rows as they read any other interval rows.
//
//   THE RULE is host/cigar_blocks.h's walk_blocks; both passes below call it on the same operands.
//
//   ROWS IN, BLOCK ROWS OUT.  Input row r: ref_id, start (each with an optional validity bitmap), an optional row mask, and its ops.
//   It emits max(1, k) output rows and ONE validity bit per output row, shared by the three columns:
//     an invalid row (NULL ref_id, NULL start or mask bit 0)  -> one invalid row, its three values 0;
//     a valid row of k = 0 blocks                 -> one valid row [start, start - 1] (what such a record is in span mode: `inverted`);
//     a valid row of k >= 1 blocks                -> its k blocks in order.
//
//   THREE OP SOURCES, one template.  ListSrc: Arrow list columns, offsets i32[n + 1] and aligned u32 ops.  BamSrc: the record's byte
//   offset in the slab (rec_of_row) -> 36 + l_read_name, n_cigar_op unaligned u32.  SamSrc: field 6 of the row's line, found through
//   the parser's newline index and its `skip`.
//
//   TWO PASSES.  k_blocks_count: rows -> u32 counts.  The offsets scan of list_kernels.h: per-workgroup sums, scanned in place, the
//   total in one word.  k_blocks_fill: every row finds its first output row (list_first_item) and walks its ops again.
//   One thread per row: a record of thousands of ops is rare and is walked by one lane, as k_bam_extract walks it.
//
//   SAFETY IS THE KERNELS' OWN.  Every source checks what it is about to load against what it was handed -- a list row's offsets in
//   order inside [offsets[0], offsets[n]]; a BAM record's header, extent and CIGAR inside the slab and inside its block_size, whatever
//   k_bam_extract has checked before; a SAM line inside the text -- and a row that fails loads nothing more, raises a status bit and
//   emits one invalid row.  The fill pass writes no output row at or beyond `cap` and none beyond the row's own count, whatever the
//   count pass left behind: it raises ST_OVERFLOW instead.  The host turns every bit into an error or a hand-over to the host reader.
#include <algorithm>
#include <new>

#include "host/cigar_blocks.h"
#include "list_kernels.h"

namespace {

using namespace exon::cigar;

// status bits: ST_OFFSETS list offsets out of order; ST_OVERFLOW the fill pass met the capacity; ST_RECORD a BAM record or SAM line
// that does not fit what was handed over; ST_CG the CG-tag placeholder (DECISION a); ST_CIGAR a SAM CIGAR refused by text_ops_ok (b)
constexpr unsigned ST_OFFSETS = 1, ST_OVERFLOW = 2, ST_RECORD = 4, ST_CG = 8, ST_CIGAR = 16;

struct BlockRowsIn {
  const int32_t* ref;
  const uint8_t* ref_valid;
  const int64_t* start;
  const uint8_t* start_valid;
  const uint8_t* row_mask;
  unsigned n;
  uint32_t cover_ops;
};
struct BlockRowsOut {
  int32_t* ref;
  int64_t *start, *end;
  unsigned* valid;  // 32 rows a word, all ones before the fill pass: an invalid row clears its bit
  unsigned cap;
};

__device__ __forceinline__ bool bit_set(const uint8_t* __restrict__ bits, unsigned i) { return !bits || ((bits[i >> 3] >> (i & 7)) & 1); }
__device__ __forceinline__ bool row_valid(const BlockRowsIn& a, unsigned row) {
  return bit_set(a.ref_valid, row) && bit_set(a.start_valid, row) && bit_set(a.row_mask, row);
}

// ---- the op sources: open(row, &ops) -> 0, or the status bit of what is wrong (nothing may be loaded for the row then) --------------
struct ListSrc {
  using Ops = ArrayOps;
  const int32_t* offsets;  // [n + 1]
  const uint32_t* ops;
  unsigned n;
  __device__ __forceinline__ unsigned open(unsigned row, Ops* o) const {
    const int32_t lo = offsets[0], hi = offsets[n];
    const int32_t o0 = offsets[row], o1 = offsets[row + 1];
    if (lo < 0 || o0 < lo || o1 < o0 || o1 > hi) return ST_OFFSETS;
    *o = ArrayOps{ops + o0, (uint32_t)(o1 - o0)};
    return 0;
  }
};
struct BamSrc {
  using Ops = ByteOps;
  const uint8_t* d;
  uint32_t n_bytes;
  const uint32_t* rec_of_row;
  __device__ __forceinline__ uint32_t le(uint32_t at, int bytes) const {
    uint32_t v = 0;
    for (int i = 0; i < bytes; ++i) v |= (uint32_t)d[at + i] << (8 * i);
    return v;
  }
  __device__ __forceinline__ unsigned open(unsigned row, Ops* o) const {
    const uint32_t r = rec_of_row[row];
    if ((uint64_t)r + 36 > n_bytes) return ST_RECORD;
    const uint32_t bs = le(r, 4);
    if (bs < 32 || (uint64_t)r + 4 + bs > n_bytes) return ST_RECORD;
    const uint32_t l_name = d[r + 12], n_cigar = le(r + 16, 2), l_seq = le(r + 20, 4);
    const uint32_t co = 32 + l_name;
    if (co + 4 * n_cigar > bs) return ST_RECORD;
    *o = ByteOps{d + r + 4 + co, n_cigar};
    return is_cg_placeholder(*o, l_seq) ? ST_CG : 0;
  }
};
struct SamSrc {
  using Ops = TextOps;
  const uint8_t* text;  // 16-byte aligned; the slab proper starts `skip` bytes in
  const unsigned* nl;   // where every row's '\n' is
  unsigned skip, n_total;
  __device__ __forceinline__ unsigned open(unsigned row, Ops* o) const {
    const unsigned begin = row ? nl[row - 1] + 1 : skip;
    unsigned end = nl[row];
    if (end >= n_total || begin > end) return ST_RECORD;
    if (end > begin && text[end - 1] == '\r') --end;
    unsigned at = begin, tabs = 0;
    for (; at < end && tabs < 5; ++at) tabs += text[at] == '\t';
    if (tabs < 5) return ST_RECORD;
    unsigned stop = at;
    while (stop < end && text[stop] != '\t') ++stop;
    if (!text_ops_ok(text + at, text + stop)) return ST_CIGAR;
    if (stop - at == 1 && text[at] == '*') stop = at;
    *o = TextOps{text + at, text + stop};
    return 0;
  }
};

template <typename Src>
__global__ __launch_bounds__(LIST_TPB) void k_blocks_count(const BlockRowsIn a, const Src src, uint32_t* __restrict__ cnt, unsigned* __restrict__ status) {
  const unsigned row = blockIdx.x * LIST_TPB + threadIdx.x;
  if (row >= a.n) return;
  unsigned c = 1;
  if (row_valid(a, row)) {
    typename Src::Ops o;
    if (const unsigned bad = src.open(row, &o)) atomicOr(status, bad);
    else c = max(1u, count_blocks(o, a.start[row], a.cover_ops));
  }
  cnt[row] = c;
}

template <typename Src>
__global__ __launch_bounds__(LIST_TPB) void k_blocks_fill(const BlockRowsIn a, const Src src, const uint32_t* __restrict__ cnt, const unsigned* __restrict__ block_offsets,
                                                          const BlockRowsOut out, unsigned* __restrict__ status) {
  const unsigned row = blockIdx.x * LIST_TPB + threadIdx.x;
  const unsigned c = row < a.n ? cnt[row] : 0u;
  const unsigned first = list_first_item(c, block_offsets);  // (every thread of the workgroup)
  if (row >= a.n) return;
  // the output rows this row may write: its own count, cut at the capacity
  const unsigned room = first < out.cap ? min(c, out.cap - first) : 0u;
  if (room < c) atomicOr(status, ST_OVERFLOW);
  typename Src::Ops o;
  const bool valid = row_valid(a, row) && src.open(row, &o) == 0;
  if (!valid) {
    if (room) {
      out.ref[first] = 0, out.start[first] = 0, out.end[first] = 0;
      atomicAnd(&out.valid[first >> 5], ~(1u << (first & 31)));
    }
    return;
  }
  const int32_t ref = a.ref[row];
  const int64_t start = a.start[row];
  const unsigned k = walk_blocks(o, start, a.cover_ops, [&](uint32_t j, int64_t s, int64_t e) {
    if (j < room) out.ref[first + j] = ref, out.start[first + j] = s, out.end[first + j] = e;
  });
  if (k == 0 && room) out.ref[first] = ref, out.start[first] = start, out.end[first] = (int64_t)((uint64_t)start - 1);
  if (max(k, 1u) != c) atomicOr(status, ST_OVERFLOW);  // (the two passes read the same operands: this cannot happen)
}

size_t pow2_at_least(size_t x) {
  size_t p = 4096;
  while (p < x) p <<= 1;
  return p;
}

// Both passes over `a.n` rows on `s`, synchronously.  scratch: [cnt: n] [block sums: nb] [total] [status].  After the count pass
// room(total, &out) provides the output (a non-zero return ends the call with it).  *status_out: the bits raised by either pass; the
// fill pass is not run when the count pass raised one.
template <typename Src, typename Room>
int run_blocks(exon_hip_ctx* ctx, hipStream_t s, const BlockRowsIn& a, const Src& src, uint32_t* scratch, int64_t* n_blocks, unsigned* status_out, Room room) {
  const int nb = (int)((a.n + LIST_TPB - 1) / LIST_TPB);
  uint32_t* cnt = scratch;
  unsigned *sums = cnt + a.n, *total = sums + nb, *status = total + 1;
  unsigned back[2] = {0, 0};  // total, status
  HIP_TRY(ctx, hipMemsetAsync(total, 0, 8, s));
  hipLaunchKernelGGL(k_blocks_count<Src>, dim3(nb), dim3(LIST_TPB), 0, s, a, src, cnt, status);
  launch_list_scan(s, cnt, nullptr, a.n, nb, sums, total);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(back, total, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  *n_blocks = (int64_t)back[0];
  *status_out = back[1];
  if (back[1]) return EXON_HIP_OK;
  BlockRowsOut out{};
  if (const int rc = room((int64_t)back[0], &out)) return rc;
  HIP_TRY(ctx, hipMemsetAsync(out.valid, 0xFF, ((size_t)back[0] + 31) / 32 * 4, s));
  hipLaunchKernelGGL(k_blocks_fill<Src>, dim3(nb), dim3(LIST_TPB), 0, s, a, src, cnt, sums, out, status);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(back, total, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));  // (for the status word alone: ST_OVERFLOW becomes this call's error, not a later one's)
  *status_out = back[1];
  return EXON_HIP_OK;
}

}  // namespace

// ---- the stage of a blocks-mode scan (scan.cpp) ---------------------------------------------------------------------------------------
// The scan's own buffers, like its row mask: they grow geometrically, the stream is synchronised before a regrow (the plan's kernel
// over the previous slab may still read them), every column starts 16-byte aligned, nothing is sized by a worst case per slab byte.
struct ExonBlockBufs {
  uint32_t* scratch = nullptr;
  size_t scratch_words = 0;
  uint8_t* out = nullptr;
  size_t out_rows = 0;  // a multiple of 64
};
void exon_cigar_blocks_free(ExonBlockBufs* b) {
  if (!b) return;
  if (b->scratch) hipFree(b->scratch);
  if (b->out) hipFree(b->out);
  delete b;
}
// One slab's rows -> block rows in the scan's buffers: cols[0 .. 3) = ref_id, start, end sharing one validity bitmap, *n_blocks rows.
// *undecided: the device will not decide a record (a BAM record or SAM line beyond what was handed over, the CG placeholder, a SAM
// CIGAR the rule refuses): nothing was produced, the host reader takes the file and reports what is wrong.  Synchronises `stream` twice:
// for the total between the passes, and for the fill pass's status word -- nothing else needs the second one (the slab's release is
// stream-ordered, as the views launches over d_text rely on): it could be read once per file instead.
int exon_cigar_blocks_slab(exon_hip_ctx* ctx, void* stream, ExonBlockBufs** bufs, const ExonBlockSlab& in, exon_hip_column* cols, int64_t* n_blocks, int* undecided) {
  static const char* who = "aligned blocks of a slab";
  *n_blocks = 0;
  *undecided = 0;
  if (!cover_ops_ok(in.cover_ops) || in.n_rows <= 0 || in.n_rows > INT32_MAX || in.n_bytes <= 0 || in.n_bytes > UINT32_MAX - 16) return fail(ctx, EXON_HIP_EINVAL, "%s: bad argument", who);
  if (!*bufs) *bufs = new (std::nothrow) ExonBlockBufs();
  ExonBlockBufs* b = *bufs;
  if (!b) return fail(ctx, EXON_HIP_ENOMEM, "%s: out of host memory", who);
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)in.n_rows, words = n + (n + LIST_TPB - 1) / LIST_TPB + 2;
  if (b->scratch_words < words) {
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (b->scratch) hipFree(b->scratch);
    b->scratch = nullptr;
    b->scratch_words = 0;
    const size_t cap = words + words / 2;
    if (hipMalloc((void**)&b->scratch, cap * 4) != hipSuccess) return fail(ctx, EXON_HIP_ENOMEM, "%s: %zu bytes of counts", who, cap * 4);
    b->scratch_words = cap;
  }
  const BlockRowsIn a{in.ref, in.ref_valid, in.start, in.pos_valid, in.row_mask, (unsigned)n, in.cover_ops};
  auto room = [&](int64_t total, BlockRowsOut* out) -> int {
    if (b->out_rows < (size_t)total) {
      HIP_TRY(ctx, hipStreamSynchronize(s));
      if (b->out) hipFree(b->out);
      b->out = nullptr;
      b->out_rows = 0;
      const size_t cap = ((size_t)total + (size_t)total / 2 + 63) / 64 * 64;
      if (hipMalloc((void**)&b->out, cap * 20 + cap / 8) != hipSuccess) return fail(ctx, EXON_HIP_ENOMEM, "%s: %zu block rows", who, cap);
      b->out_rows = cap;
    }
    const size_t cap = b->out_rows;  // [start: 8 cap] [end: 8 cap] [ref: 4 cap] [valid: cap / 8], each a multiple of 16 bytes
    *out = BlockRowsOut{reinterpret_cast<int32_t*>(b->out + 16 * cap), reinterpret_cast<int64_t*>(b->out), reinterpret_cast<int64_t*>(b->out + 8 * cap),
                        reinterpret_cast<unsigned*>(b->out + 20 * cap), (unsigned)std::min<size_t>(cap, UINT32_MAX)};
    return EXON_HIP_OK;
  };
  unsigned status = 0;
  int rc;
  if (in.rec_of_row) {
    rc = run_blocks(ctx, s, a, BamSrc{in.data, (uint32_t)in.n_bytes, in.rec_of_row}, b->scratch, n_blocks, &status, room);
  } else {
    const unsigned skip = (unsigned)(reinterpret_cast<uintptr_t>(in.data) & 15);
    rc = run_blocks(ctx, s, a, SamSrc{in.data - skip, in.newlines, skip, (unsigned)in.n_bytes + skip}, b->scratch, n_blocks, &status, room);
  }
  if (rc) return rc;
  if (status & ST_OVERFLOW) return fail(ctx, EXON_HIP_EDEVICE, "%s: the fill pass disagreed with the count pass (status %u)", who, status);
  if (status) {
    *undecided = 1;
    *n_blocks = 0;
    return EXON_HIP_OK;
  }
  const size_t cap = b->out_rows;
  const uint8_t* valid = b->out + 20 * cap;
  cols[0] = exon_hip_column{b->out + 16 * cap, valid, nullptr, *n_blocks};
  cols[1] = exon_hip_column{b->out, valid, nullptr, *n_blocks};
  cols[2] = exon_hip_column{b->out + 8 * cap, valid, nullptr, *n_blocks};
  return EXON_HIP_OK;
}

extern "C" {

int exon_hip_cigar_blocks_host(const uint32_t* ops, int32_t n_ops, int64_t start, uint32_t cover_ops, int64_t* out_start, int64_t* out_end, int32_t cap,
                               int32_t* n_blocks) {
  static const char* who = "exon_hip_cigar_blocks_host";
  if (!n_blocks) return fail(nullptr, EXON_HIP_EINVAL, "%s: n_blocks is NULL", who);
  *n_blocks = 0;
  if (!cover_ops_ok(cover_ops))
    return fail(nullptr, EXON_HIP_EINVAL, "%s: cover_ops 0x%X is not a non-empty subset of 0x18D (M D N = X, the ops that consume the reference)", who, cover_ops);
  if (n_ops < 0 || cap < 0 || (n_ops > 0 && !ops)) return fail(nullptr, EXON_HIP_EINVAL, "%s: n_ops / cap below 0, or ops is NULL", who);
  if (cap > 0 && (!out_start || !out_end)) return fail(nullptr, EXON_HIP_EINVAL, "%s: an output array is NULL", who);
  const uint32_t k = fill_blocks(ArrayOps{ops, (uint32_t)n_ops}, start, cover_ops, out_start, out_end, (uint32_t)cap);
  *n_blocks = (int32_t)k;  // (k <= n_ops)
  if (k > (uint32_t)cap) return fail(nullptr, EXON_HIP_ECAPACITY, "%s: %u blocks, room for %d", who, k, cap);
  return EXON_HIP_OK;
}

int exon_hip_cigar_blocks(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id, const exon_hip_column* start, const int32_t* d_cigar_offsets,
                          const uint32_t* d_cigar_ops, int64_t n, uint32_t cover_ops, int32_t* d_out_ref, int64_t* d_out_start, int64_t* d_out_end,
                          uint8_t* d_out_valid, int64_t cap, int64_t* n_blocks) {
  static const char* who = "exon_hip_cigar_blocks";
  if (!ctx || !n_blocks) return fail(ctx, EXON_HIP_EINVAL, "%s: NULL argument", who);
  *n_blocks = 0;
  if (!cover_ops_ok(cover_ops))
    return fail(ctx, EXON_HIP_EINVAL, "%s: cover_ops 0x%X is not a non-empty subset of 0x18D (M D N = X, the ops that consume the reference)", who, cover_ops);
  if (n < 0 || cap < 0) return fail(ctx, EXON_HIP_EINVAL, "%s: n or cap below 0", who);
  if (n == 0) return EXON_HIP_OK;
  // (counts and their total are 32-bit words: a row emits at most max(1, its ops) rows and int32 offsets hold fewer than 2^31 ops)
  if (n > INT32_MAX) return fail(ctx, EXON_HIP_EUNSUPPORTED, "%s: %lld rows in one call; split the batch below 2^31 rows", who, (long long)n);
  const exon_hip_column* cols[2] = {ref_id, start};
  static const char* names[2] = {"ref_id", "start"};
  for (int c = 0; c < 2; ++c) {
    if (!cols[c] || !cols[c]->values) return fail(ctx, EXON_HIP_EINVAL, "%s: column %s is NULL", who, names[c]);
    if (cols[c]->length < n) return fail(ctx, EXON_HIP_EINVAL, "%s: %s: length %lld < n %lld", who, names[c], (long long)cols[c]->length, (long long)n);
    if (reinterpret_cast<uintptr_t>(cols[c]->values) & (c ? 7 : 3)) return fail(ctx, EXON_HIP_EINVAL, "%s: %s: values must be %d-byte aligned", who, names[c], c ? 8 : 4);
  }
  if (!d_cigar_offsets || !d_cigar_ops) return fail(ctx, EXON_HIP_EINVAL, "%s: the CIGAR list's offsets or ops are NULL", who);
  if ((reinterpret_cast<uintptr_t>(d_cigar_offsets) | reinterpret_cast<uintptr_t>(d_cigar_ops)) & 3) return fail(ctx, EXON_HIP_EINVAL, "%s: offsets and ops must be 4-byte aligned", who);
  if (cap > 0 && (!d_out_ref || !d_out_start || !d_out_end || !d_out_valid)) return fail(ctx, EXON_HIP_EINVAL, "%s: an output buffer is NULL", who);
  if ((reinterpret_cast<uintptr_t>(d_out_ref) | reinterpret_cast<uintptr_t>(d_out_valid)) & 3) return fail(ctx, EXON_HIP_EINVAL, "%s: d_out_ref and d_out_valid must be 4-byte aligned", who);
  if ((reinterpret_cast<uintptr_t>(d_out_start) | reinterpret_cast<uintptr_t>(d_out_end)) & 7) return fail(ctx, EXON_HIP_EINVAL, "%s: d_out_start and d_out_end must be 8-byte aligned", who);

  hipStream_t s = pick_stream(ctx, stream);
  uint32_t* scratch = static_cast<uint32_t*>(exon_pool_alloc(ctx, pow2_at_least(((size_t)n + (size_t)(n + LIST_TPB - 1) / LIST_TPB + 2) * 4)));
  if (!scratch) return fail(ctx, EXON_HIP_ENOMEM, "%s: scratch for %lld rows", who, (long long)n);
  const BlockRowsIn in{(const int32_t*)ref_id->values, ref_id->validity, (const int64_t*)start->values, start->validity, nullptr, (unsigned)n, cover_ops};
  unsigned status = 0;
  int rc = run_blocks(ctx, s, in, ListSrc{d_cigar_offsets, d_cigar_ops, (unsigned)n}, scratch, n_blocks, &status, [&](int64_t total, BlockRowsOut* out) -> int {
    if (total > cap) return fail(ctx, EXON_HIP_ECAPACITY, "%s: %lld block rows, room for %lld; nothing was written", who, (long long)total, (long long)cap);
    *out = BlockRowsOut{d_out_ref, d_out_start, d_out_end, reinterpret_cast<unsigned*>(d_out_valid), (unsigned)std::min<int64_t>(cap, UINT32_MAX)};
    return EXON_HIP_OK;
  });
  if (rc == EXON_HIP_EDEVICE) hipStreamSynchronize(s);  // (a failed call in flight must not outlive the scratch)
  exon_pool_free(ctx, scratch);
  if (rc) return rc;
  if (status) *n_blocks = 0;
  if (status & ST_OFFSETS) return fail(ctx, EXON_HIP_EINVAL, "%s: the CIGAR list's offsets are not in order inside [offsets[0], offsets[n]]", who);
  if (status) return fail(ctx, EXON_HIP_EDEVICE, "%s: the fill pass disagreed with the count pass (status %u); the output is not complete", who, status);
  return EXON_HIP_OK;
}

}  // extern "C"
