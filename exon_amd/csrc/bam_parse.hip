// bam_parse.hip -- BAM record splitting + field extraction ON THE GPU: inflated BAM bytes in HBM -> device-layout
// columns (flag, mapping_quality, reference id, start, end) in HBM.
//
// Reference semantics: BAMArrayBuilder::append (exon-bam/src/array_builder.rs:102-218) restricted to the columns of
// the device layout -- flag = raw u16 bits as Int32 (:114-117), reference = refID (NULL if -1, :118-127), start =
// pos + 1 (NULL if pos < 0), end = start + (sum of M/D/N/=/X lengths) - 1, mapping_quality NULL when 255 (:136-143);
// record layout: SAM specification section 4.2.  Undecided (the host reader reports what is wrong): a CIGAR that does not fit in
// block_size, a reference id beyond the header's (the reference indexes its name table with it, :118-122).
//
// Records are found by the parallel chain walk of chain_walk.h (64 KiB segments, guessed starts proven by induction);
//   k_bam_extract  one thread per record: fixed fields, CIGAR walk for the reference length, columns + validity bits.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>

#include "chain_walk.h"
#include "internal.h"

namespace {

using chain::ld16;
using chain::ld32;
using chain::SEG;
using chain::SegInfo;

// BAM record: int32 block_size, then block_size bytes (SAM spec 4.2)
struct BamFormat {
  static constexpr uint32_t MIN_HEADER = 36, MIN_RECORD = 36, LEN_BYTES = 4;
  int32_t n_ref;
  __device__ __forceinline__ uint32_t record_bytes(const uint8_t* d, uint32_t r) const {
    const uint32_t bs = ld32(d + r);
    return bs < 32 || bs > (1u << 28) ? 0u : 4u + bs;
  }
  // Is there a well-formed record header at offset r?  Only what is needed to tell record starts from arbitrary bytes;
  // the walk itself trusts block_size alone, as the host decoder does.
  __device__ bool plausible(const uint8_t* d, uint32_t n, uint32_t r) const {
    if ((uint64_t)r + 36 > n) return false;
    const uint32_t bs = ld32(d + r);
    if (bs < 32 || bs > (1u << 24)) return false;
    const int32_t ref = (int32_t)ld32(d + r + 4), pos = (int32_t)ld32(d + r + 8);
    if (ref < -1 || ref >= n_ref || pos < -1) return false;
    const uint32_t l_name = d[r + 12], n_cigar = ld16(d + r + 16);
    const int32_t l_seq = (int32_t)ld32(d + r + 20);
    const int32_t mref = (int32_t)ld32(d + r + 24), mpos = (int32_t)ld32(d + r + 28);
    if (l_name == 0 || l_seq < 0 || mref < -1 || mref >= n_ref || mpos < -1) return false;
    const uint64_t need = 32ull + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
    if (need > bs) return false;
    if ((uint64_t)r + 36 + l_name <= n && d[r + 36 + l_name - 1] != 0) return false;  // read name is NUL-terminated
    return true;
  }
};
constexpr uint32_t SEG_CAP = chain::seg_cap<BamFormat>();

struct BamOut {
  int32_t* flag;
  uint8_t* mapq;
  uint32_t* mapq_valid;  // validity bitmaps as 32-bit words
  int32_t* ref_id;
  uint32_t* ref_valid;
  int64_t* start;
  int64_t* end;
  uint32_t* pos_valid;
  uint32_t* rec_of_row;  // byte offset of every row's record (the string columns are built from it: text_columns.hip)
};

__global__ __launch_bounds__(256) void k_bam_extract(const uint8_t* __restrict__ d, const SegInfo* __restrict__ seg,
                                                     const uint32_t* __restrict__ base, const uint32_t* __restrict__ rec_off, BamOut o,
                                                     int32_t n_ref, unsigned* __restrict__ scalars) {
  const uint32_t s = blockIdx.x;
  if (scalars[1] != 0) return;  // the segmentation was not proven: nothing here can be trusted
  const uint32_t cnt = seg[s].count, row0 = base[s];
  const uint32_t* offs = rec_off + (size_t)s * SEG_CAP;
  // validity bits: ONE atomicOr per 32-row word and wave (a wave's 64 consecutive rows touch at most three words; words at segment
  // seams are shared with the neighbouring workgroup) instead of one per row and column -- three global atomics per record were
  // most of this kernel's time
  const uint32_t lane = threadIdx.x & 63u;
  auto publish = [&](uint32_t* bitmap, bool bit, uint32_t wave_row) {
    const unsigned long long b = __ballot(bit);
    if (b == 0) return;
    const uint32_t sh = wave_row & 31u;
    const unsigned long long x = b << sh;
    const uint32_t part = lane == 0 ? (uint32_t)x : lane == 1 ? (uint32_t)(x >> 32) : (sh ? (uint32_t)(b >> (64u - sh)) : 0u);
    if (lane < 3 && part) atomicOr(&bitmap[(wave_row >> 5) + lane], part);
  };
  for (uint32_t k = threadIdx.x; k < cnt; k += 256) {
    const uint32_t r = offs[k], row = row0 + k;
    const uint32_t bs = ld32(d + r);
    const int32_t ref = (int32_t)ld32(d + r + 4), pos = (int32_t)ld32(d + r + 8);
    const uint32_t l_name = d[r + 12], mapq = d[r + 13], n_cigar = ld16(d + r + 16), flag = ld16(d + r + 18);
    const uint32_t co = 32 + l_name;
    const bool ok = co + 4 * n_cigar <= bs && ref < n_ref;  // else "corrupt BAM cigar" / "BAM reference id out of range" on the host
    if (!ok) atomicAdd(&scalars[1], 1u);
    int64_t ref_len = 0;
    for (uint32_t c = 0; ok && c < n_cigar; ++c) {
      const uint32_t op = ld32(d + r + 4 + co + 4 * c);
      const uint32_t code = op & 0xF;
      if (code == 0 || code == 2 || code == 3 || code == 7 || code == 8) ref_len += op >> 4;
    }
    const bool pv = pos >= 0;
    if (ok) {
      o.flag[row] = (int32_t)flag;
      o.mapq[row] = (uint8_t)mapq;
      o.ref_id[row] = ref < 0 ? -1 : ref;
      o.start[row] = pv ? (int64_t)pos + 1 : 0;
      o.end[row] = pv ? (int64_t)pos + ref_len : 0;
      o.rec_of_row[row] = r;
    }
    const uint32_t wave_row = row - lane;  // the row of the wave's lane 0 (rows are consecutive across a wave's lanes)
    publish(o.mapq_valid, ok && mapq != 255, wave_row);
    publish(o.ref_valid, ok && ref >= 0, wave_row);
    publish(o.pos_valid, ok && pv, wave_row);
  }
}

}  // namespace

struct exon_hip_bam_parser {
  exon_hip_ctx* ctx;
  PoolBufs bufs;
  int32_t n_ref = 0;
  int64_t max_bytes = 0;
  chain::ChainState chain;
  BamOut out{};
  ExonBlockBufs* blocks = nullptr;  // exon_hip_bam_parser_cigar_blocks: the block rows of the last slab (cigar_blocks.hip)
  explicit exon_hip_bam_parser(exon_hip_ctx* c) : ctx(c), bufs(c) {}
  ~exon_hip_bam_parser() { exon_cigar_blocks_free(blocks); }
};

extern "C" {

int exon_hip_bam_parser_create(exon_hip_ctx* ctx, int32_t n_references, int64_t max_bytes, exon_hip_bam_parser** outp) {
  if (!ctx || !outp || max_bytes < 64 || n_references < 0) return fail(ctx, EXON_HIP_EINVAL, "exon_hip_bam_parser_create: bad argument");
  if (max_bytes > 0xF0000000LL) return fail(ctx, EXON_HIP_EINVAL, "slab size must stay below 4 GiB (32-bit record offsets)");
  *outp = nullptr;
  exon_hip_bam_parser* p = new (std::nothrow) exon_hip_bam_parser(ctx);
  if (!p) return fail(ctx, EXON_HIP_ENOMEM, "out of host memory");
  p->n_ref = n_references;
  p->max_bytes = max_bytes;
  hipSetDevice(ctx->device);
  PoolBufs& b = p->bufs;
  p->chain.alloc<BamFormat>(b, max_bytes);
  const size_t r = (size_t)(max_bytes / 36 + 1), w = (r + 31) / 32 * 4 + 64;
  p->out.flag = b.take<int32_t>(r * 4);
  p->out.mapq = b.take<uint8_t>(r + 64);
  p->out.mapq_valid = b.take<uint32_t>(w);
  p->out.ref_id = b.take<int32_t>(r * 4);
  p->out.ref_valid = b.take<uint32_t>(w);
  p->out.start = b.take<int64_t>(r * 8);
  p->out.end = b.take<int64_t>(r * 8);
  p->out.pos_valid = b.take<uint32_t>(w);
  p->out.rec_of_row = b.take<uint32_t>(r * 4);
  if (b.status() != hipSuccess) {
    const std::string msg = hipGetErrorString(b.status());
    delete p;
    return fail(ctx, EXON_HIP_ENOMEM, "bam parser allocation: %s", msg.c_str());
  }
  *outp = p;
  return EXON_HIP_OK;
}

int exon_hip_bam_parser_destroy(exon_hip_bam_parser* p) {
  delete p;
  return EXON_HIP_OK;
}

int exon_hip_bam_parser_parse(exon_hip_bam_parser* p, void* stream, const uint8_t* d_data, int64_t n_bytes, exon_hip_bam_columns* cols) {
  if (!p || !cols || (n_bytes > 0 && !d_data)) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "exon_hip_bam_parser_parse: NULL argument");
  exon_hip_ctx* ctx = p->ctx;
  if (n_bytes > p->max_bytes) return fail(ctx, EXON_HIP_EINVAL, "slab of %lld bytes exceeds the parser's %lld", (long long)n_bytes, (long long)p->max_bytes);
  memset(cols, 0, sizeof *cols);
  if (n_bytes == 0) return EXON_HIP_OK;
  hipStream_t s = pick_stream(ctx, stream);
  chain::ChainState& c = p->chain;
  const uint32_t n = (uint32_t)n_bytes, n_seg = (n + SEG - 1) / SEG;
  // rows of this slab <= n / 36: the validity words they can touch are cleared by k_chain_check, the scalars by k_chain_walk
  chain::ZeroList zl{};
  zl.p[0] = p->out.mapq_valid;
  zl.p[1] = p->out.ref_valid;
  zl.p[2] = p->out.pos_valid;
  zl.n = 3;
  zl.words = (uint32_t)(((size_t)n / 36 + 1 + 31) / 32 + 1);
  c.launch(s, d_data, n, BamFormat{p->n_ref}, zl);
  hipLaunchKernelGGL(k_bam_extract, dim3(n_seg), dim3(256), 0, s, d_data, c.seg, c.base, c.rec_off, p->out, p->n_ref, c.d_scalars);
  if (int rc = c.read_back(ctx, s)) return rc;
  if (getenv("EXON_HIP_CHAIN_TRACE")) fprintf(stderr, "[exon-hip chain] %u segments, %u rows, plain proof %u\n", n_seg, c.h_scalars[0], c.h_scalars[3]);
  cols->n_rows = c.h_scalars[0];
  cols->n_undecided = c.h_scalars[1];
  cols->consumed_bytes = c.h_scalars[2];
  cols->flag = p->out.flag;
  cols->mapq = p->out.mapq;
  cols->mapq_valid = (uint8_t*)p->out.mapq_valid;
  cols->ref_id = p->out.ref_id;
  cols->ref_valid = (uint8_t*)p->out.ref_valid;
  cols->start = p->out.start;
  cols->end = p->out.end;
  cols->pos_valid = (uint8_t*)p->out.pos_valid;
  return EXON_HIP_OK;
}

// The stage a blocks-mode scan runs per slab (scan.cpp, launch_blocks), for a caller that drives the parser itself
int exon_hip_bam_parser_cigar_blocks(exon_hip_bam_parser* p, void* stream, const uint8_t* d_data, int64_t n_bytes, const exon_hip_bam_columns* cols,
                                     const uint8_t* d_row_mask, uint32_t cover_ops, exon_hip_column* out, int64_t* n_blocks, int64_t* n_undecided) {
  static const char* who = "exon_hip_bam_parser_cigar_blocks";
  if (!p || !cols || !out || !n_blocks || !n_undecided || !d_data) return fail(p ? p->ctx : nullptr, EXON_HIP_EINVAL, "%s: NULL argument", who);
  exon_hip_ctx* ctx = p->ctx;
  *n_blocks = *n_undecided = 0;
  if (cols->n_undecided != 0) return fail(ctx, EXON_HIP_ESTATE, "%s: the parser left the slab undecided: decode it on the host", who);
  if (cols->ref_id != p->out.ref_id || cols->start != p->out.start || n_bytes <= 0 || n_bytes > p->max_bytes)
    return fail(ctx, EXON_HIP_EINVAL, "%s: cols / n_bytes are not what the last exon_hip_bam_parser_parse call of this parser returned", who);
  if (cover_ops == 0 || (cover_ops & ~0x18Du)) return fail(ctx, EXON_HIP_EINVAL, "%s: cover_ops 0x%X is not a non-empty subset of 0x18D (M D N = X, the ops that consume the reference)", who, cover_ops);
  if (cols->n_rows == 0) return EXON_HIP_OK;
  ExonBlockSlab in{};
  in.data = d_data;
  in.n_bytes = n_bytes;
  in.rec_of_row = p->out.rec_of_row;
  in.ref = cols->ref_id;
  in.ref_valid = cols->ref_valid;
  in.start = cols->start;
  in.pos_valid = cols->pos_valid;
  in.row_mask = d_row_mask;
  in.n_rows = cols->n_rows;
  in.cover_ops = cover_ops;
  int undecided = 0;
  const int rc = exon_cigar_blocks_slab(ctx, pick_stream(ctx, stream), &p->blocks, in, out, n_blocks, &undecided);
  *n_undecided = undecided;
  return rc;
}

}  // extern "C"

const uint32_t* exon_hip_bam_parser_row_records(exon_hip_bam_parser* p) { return p ? p->out.rec_of_row : nullptr; }
