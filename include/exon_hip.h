/*
 * exon_hip.h -- C ABI of the MI355X-native scan -> filter -> aggregate engine (libexon_hip.so).
 *
 * This is the drop-in boundary for Exon's hot path.  Every entry point is
 * extern "C", takes plain pointers / sizes / opaque handles, returns an int status and never
 * throws.  Data crosses as the Arrow C Data Interface (host batches) or the Arrow C Device Data
 * Interface (HBM-resident batches, device_type = ARROW_DEVICE_ROCM).  A Rust binding needs only
 * `extern "C"` declarations of the functions below plus arrow-rs `arrow::ffi` (already enabled in
 * the reference: exon/exon-core/Cargo.toml:73-77, exon/exon-core/src/ffi/mod.rs:58-73); see
 * INTEGRATION.md for the shim.
 *
 * What each group replaces in the reference (paths relative to /root/reference/exon):
 *   exon_hip_plan_* / exon_hip_stream_*   ExecutionPlan::execute of the operator chain
 *        AggregateExec(Partial) <- [CoalesceBatchesExec] <- FilterExec <- {VCF,BAM,FASTQ}Scan
 *        (exon-core/src/datasources/vcf/scanner.rs:142-162, bam/scanner.rs:138-158; the
 *        FilterExec/AggregateExec themselves are DataFusion 44, not vendored)
 *   exon_hip_region_count                 RegionPhysicalExpr::evaluate
 *        (exon-core/src/physical_plan/region_physical_expr.rs:220-240), region_match UDF
 *        (exon-core/src/udfs/vcf/mod.rs:65-131), IndexedAsyncBatchStream::filter
 *        (exon-vcf/src/indexed_async_batch_stream.rs:99-116) + COUNT(*)
 *   exon_hip_flag_mapq_group_count        sam_flag_function (exon-core/src/udfs/sam/samflags.rs:26-47)
 *        + CAST(mapping_quality AS INT) >= q + COUNT(*) GROUP BY reference over the columns of
 *        BAMArrayBuilder::append (exon-bam/src/array_builder.rs:102-218)
 *   exon_hip_cmp_avg_by_group             info."AF" > lit, AVG(qual), COUNT(*) GROUP BY filter over
 *        LazyVCFArrayBuilder columns (exon-vcf/src/array_builder/lazy_array_builder.rs:205-216,
 *        info_builder.rs:152-309)
 *   exon_hip_cmp_minmax_by_group          the same filter, MIN(qual), MAX(qual), COUNT(*) GROUP BY filter: DataFusion 44's
 *        MinAccumulator / MaxAccumulator (datafusion-functions-aggregate min_max.rs, not vendored) behind the same FilterExec
 *   exon_hip_qual_pos_hist                QualityScoreStringToList::invoke
 *        (exon-core/src/udfs/sequence/quality_score_string_to_list.rs:56-117) + unnest + GROUP BY
 *   exon_hip_read_stats_hist              GCContent::invoke (exon-core/src/udfs/sequence/gc_content.rs:52-71), the read length
 *        and the per-row mean of quality_scores_to_list, each binned (integers) and counted: GROUP BY bin, COUNT(*)
 *   exon_hip_seq_stats_hist               GCContent::invoke (exon-core/src/udfs/sequence/gc_content.rs:52-71) and length(sequence) over
 *        FASTA (or any Utf8 sequence column), each binned (integers) and counted: GROUP BY bin, COUNT(*); plus the byte composition
 *   exon_hip_regroup_files_by_size        regroup_files_by_size
 *        (exon-core/src/datasources/exon_file_scan_config.rs:79-110) -- the multi-GPU shard rule
 */
#ifndef EXON_HIP_H
#define EXON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Arrow C Data Interface (verbatim ABI; https://arrow.apache.org/docs/format/CDataInterface.html) */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};
#endif
#ifndef ARROW_C_DEVICE_DATA_INTERFACE
#define ARROW_C_DEVICE_DATA_INTERFACE
typedef int32_t ArrowDeviceType;
#define ARROW_DEVICE_CPU 1
#define ARROW_DEVICE_ROCM 10
#define ARROW_DEVICE_ROCM_HOST 11
struct ArrowDeviceArray {
  struct ArrowArray array;
  int64_t device_id;
  ArrowDeviceType device_type;
  void* sync_event; /* hipEvent_t* or NULL */
  int64_t reserved[3];
};
#endif

/* ---- status codes ------------------------------------------------------------------------- */
#define EXON_HIP_OK 0
#define EXON_HIP_EINVAL (-1)       /* bad argument / schema mismatch / misaligned buffer */
#define EXON_HIP_ENOMEM (-2)
#define EXON_HIP_EDEVICE (-3)      /* HIP runtime error (text in exon_hip_last_error) */
#define EXON_HIP_EUNSUPPORTED (-4) /* valid request this build does not implement */
#define EXON_HIP_ESTATE (-5)       /* call out of order (e.g. push after finish) */
#define EXON_HIP_ECAPACITY (-6)    /* more distinct group keys than the plan's n_groups: the stream's state and dictionary are
                                      unchanged (the offending scan's rows were not added) -- finish the stream, emit its state,
                                      and continue on a fresh one, or create the plan for more groups (round 5; EINVAL before) */

typedef struct exon_hip_ctx exon_hip_ctx;
typedef struct exon_hip_plan exon_hip_plan;
typedef struct exon_hip_stream exon_hip_stream;

/* ---- context ------------------------------------------------------------------------------ */
typedef struct exon_hip_device_info {
  char name[64];
  char gcn_arch[32];
  int32_t compute_units;
  int32_t wavefront_size;
  int64_t hbm_bytes;
  int32_t clock_khz;
  int32_t reserved;
} exon_hip_device_info;

int exon_hip_abi_version(void); /* 5 (round 6: the CONTRACT of exon_hip_stream_push changed in round 5 -- batches of up to 131072 rows are held and
                                      their release callback runs at the slot flush, not before push returns; key overflow is ECAPACITY,
                                      not EINVAL -- so a caller built against 4 must not load this library unchanged; also new: scan
                                      projection, plain-gzip inputs on the device, exon_hip_read_probe, collective fault votes;
                                      round 4: group keys by value -- exon_hip_stream_keys / _set_keys / _reconcile_keys, exon_hip_keys_union,
                                      exon_hip_stream_set_region_contig; round 3: plan_desc.x_type / y_type, 16 typed INFO fields, rccl_comm_count) */
int exon_hip_device_count(int* out);
int exon_hip_ctx_create(int device, exon_hip_ctx** out);
int exon_hip_ctx_destroy(exon_hip_ctx* ctx);
int exon_hip_ctx_info(exon_hip_ctx* ctx, exon_hip_device_info* out);
/* Text of the last error on this ctx (or, with ctx == NULL, of the calling thread).  Owned by the
 * library, valid until the next failing call on the same ctx/thread. */
const char* exon_hip_last_error(const exon_hip_ctx* ctx);
/* Threads.  Different streams, scans and parsers of one ctx may be driven from different threads at the same time (one thread per
 * partition: every stream has its own hipStream_t, workspace and status word; the ctx's buffer pool, the slab buffers a scan
 * borrows, the inflate scratch, the pinned export blocks and the staging threads are shared and locked inside the library).
 * One HANDLE -- a stream, a scan, a parser, a plan being destroyed -- belongs to one thread at a time; a plan may be shared by the
 * streams opened from it.  exon_hip_timer_start / _stop_ms use ONE event pair per ctx: time from one thread at a time.
 * exon_hip_last_error(ctx) is the last failure of ANY thread on that ctx (and its pointer is only good until another thread
 * fails there); exon_hip_last_error(NULL) is the calling thread's own last failure, which is what a caller that runs several
 * partitions should read first.  tests/test_gpu_concurrent_partitions.py pins this contract. */

/* Device-memory helpers so a host without its own HIP binding can stage columns.  `stream` is a
 * hipStream_t passed as void* (NULL = the ctx's own stream). */
int exon_hip_malloc(exon_hip_ctx* ctx, size_t bytes, void** dptr);
int exon_hip_free(exon_hip_ctx* ctx, void* dptr);
int exon_hip_memcpy_h2d(exon_hip_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
int exon_hip_memcpy_d2h(exon_hip_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
int exon_hip_memset(exon_hip_ctx* ctx, void* dst, int value, size_t bytes, void* stream);
int exon_hip_sync(exon_hip_ctx* ctx, void* stream);
/* Wall time of `reps` back-to-back launches measured with hipEvents on `stream` is available to
 * hosts through these two calls (bench.py uses torch events on the same stream instead). */
/* (ABI 5) What this box streams out of HBM through the access pattern of the fused kernels: `reps` bare read passes over the
 * first `bytes_each` bytes (whole 64 KiB tiles) of 1..4 device buffers walked in lock-step -- same persistent grid, same
 * 16 B/lane non-temporal loads, no predicate and no aggregate -- timed by a HIP event pair on `stream`.  bench.py reports
 * bytes_per_pass / ms_per_pass as roofline.box_read_ceiling_GBps next to the kernel's own figure: boxes of one pool differ by
 * a few percent in what their HBM delivers, and a roofline fraction against the spec peak cannot tell a slow box from a slow
 * kernel.  Measurement aid: not on the reference's path. */
int exon_hip_read_probe(exon_hip_ctx* ctx, void* stream, const void* const* buffers, int32_t n_buffers, int64_t bytes_each,
                        int32_t reps, double* ms_per_pass, int64_t* bytes_per_pass);
int exon_hip_timer_start(exon_hip_ctx* ctx, void* stream);
int exon_hip_timer_stop_ms(exon_hip_ctx* ctx, void* stream, float* ms);

/* ---- device column ------------------------------------------------------------------------ */
/* One Arrow array already resident in HBM.  `values` must be 16-byte aligned, `validity` is the
 * Arrow LSB-first bitmap (NULL = no nulls) whose bit 0 is row 0 of `values` (no bit offset),
 * `offsets` is the int32 offsets buffer of a Utf8/Binary column (NULL otherwise). */
typedef struct exon_hip_column {
  const void* values;
  const uint8_t* validity;
  const int32_t* offsets;
  int64_t length;
} exon_hip_column;

/* comparison operators of exon_hip_cmp_avg_by_group */
#define EXON_HIP_GT 0
#define EXON_HIP_GE 1
#define EXON_HIP_LT 2
#define EXON_HIP_LE 3
#define EXON_HIP_EQ 4
#define EXON_HIP_NE 5

#define EXON_HIP_MAX_REG_GROUPS 8   /* group ids kept in registers; ids 8.. use an LDS overflow table */
#define EXON_HIP_MAX_GROUPS 4096    /* group tables kept in LDS */
#define EXON_HIP_MAX_GROUPS_GLOBAL (1 << 24) /* K4: beyond EXON_HIP_MAX_GROUPS the state arrays are updated with global atomics */
#define EXON_HIP_MAX_REFERENCES (1 << 24) /* K3: beyond EXON_HIP_MAX_GROUPS references the counters are global atomics */
#define EXON_HIP_REGION_OPEN_END INT64_MAX

/* ---- operator launches (asynchronous on `stream`; results ACCUMULATE into the state buffers,
 *      which the caller zeroes once per query: hipMemsetAsync / exon_hip_memset -- or see
 *      exon_hip_plan_launch with EXON_HIP_LAUNCH_OVERWRITE, which needs no zeroing pass) ------ */

/* K2.  d_count[0] += |{ i : chrom_id[i] valid && == region_chrom_id && pos[i] valid &&
 *                           start <= pos[i] <= end }|   (1-based inclusive; Kleene AND, keep TRUE) */
int exon_hip_region_count(exon_hip_ctx* ctx, void* stream, const exon_hip_column* chrom_id /*i32*/,
                          const exon_hip_column* pos /*i64*/, int64_t n, int32_t region_chrom_id,
                          int64_t start, int64_t end, int64_t* d_count);

/* K3.  rows with (flag & flag_mask) == flag_value AND mapq valid AND mapq >= mapq_min are counted
 *      into d_counts[ref_id] or, when ref_id is NULL, d_counts[n_refs].  d_counts has n_refs+1. */
int exon_hip_flag_mapq_group_count(exon_hip_ctx* ctx, void* stream, const exon_hip_column* flag /*i32*/,
                                   const exon_hip_column* mapq /*u8*/, const exon_hip_column* ref_id /*i32*/,
                                   int64_t n, int32_t flag_mask, int32_t flag_value, int32_t mapq_min,
                                   int32_t n_refs, int64_t* d_counts);

/* K6.  *d_count += |{ i : ref_id[i] = region_ref_id AND start[i] <= region_end AND end[i] >= region_start }|, all three
 *      valid (a missing reference / start / end never matches).  SemiLazyRecord::intersects
 *      (exon-bam/src/indexed_async_batch_stream.rs:66-87) = bam_region_filter.  1-based inclusive. */
int exon_hip_overlap_count(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id /*i32*/,
                           const exon_hip_column* start /*i64*/, const exon_hip_column* end /*i64*/, int64_t n,
                           int32_t region_ref_id, int64_t region_start, int64_t region_end, int64_t* d_count);
/* K6, strict form: *d_count += |{ i : ref_id[i] = region_ref_id AND start[i] > after AND end[i] < before }|, all three valid.
 *      The BED / GFF interval predicate: StartEndIntervalPhysicalExpr keeps `start > a` / `end < b` BinaryExprs and evaluates
 *      them as written (exon-core/src/physical_plan/start_end_interval_physical_expr.rs:93-139, 186-191): strictly inside
 *      (after, before).  `start > a` alone: before = INT64_MAX; `end < b` alone: after = 0 (its constructor's default). */
int exon_hip_within_count(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id /*i32*/,
                          const exon_hip_column* start /*i64*/, const exon_hip_column* end /*i64*/, int64_t n,
                          int32_t region_ref_id, int64_t after, int64_t before, int64_t* d_count);

/* K4.  For rows with x valid AND (double)x <cmp_op> threshold (f32 widened to f64, as DataFusion
 *      coerces Float32 vs a Float64 literal), per dictionary id g = group_id[i] in [0, n_groups):
 *        d_counts[g]            += (y valid)            -- COUNT(y) / AVG denominator
 *        d_counts[n_groups + g] += 1                    -- COUNT(*)
 *        d_sums[g]              += (double)y if y valid -- AVG numerator
 *      Sums are reduced in a fixed order: bit-reproducible run to run for a given launch shape (up to EXON_HIP_MAX_GROUPS
 *      groups; beyond that, up to EXON_HIP_MAX_GROUPS_GLOBAL, global atomics: exact counts, sums in atomic order). */
int exon_hip_cmp_avg_by_group(exon_hip_ctx* ctx, void* stream, const exon_hip_column* x /*f32*/,
                              const exon_hip_column* y /*f32*/, const exon_hip_column* group_id /*i32*/,
                              int64_t n, double threshold, int32_t cmp_op, int32_t n_groups,
                              int64_t* d_counts /*[2*n_groups]*/, double* d_sums /*[n_groups]*/);

/* K8.  K4's predicate (x valid AND x <cmp_op> threshold: f32 through its totalOrder key, Int32 exactly), then per dictionary id
 *      g = group_id[i] in [0, n_groups), with d_state = [count_y[G]] [count_rows[G]] [minw[G]] [maxw[G]] (4 * n_groups int64):
 *        count_y[g]    += (y valid)                                      -- COUNT(y)
 *        count_rows[g] += 1                                              -- COUNT(*)
 *        minw[g] = max(minw[g], 1 + (0xFFFFFFFF - u(y)))  if y valid     -- MIN(y)
 *        maxw[g] = max(maxw[g], 1 + u(y))                 if y valid     -- MAX(y)
 *      u(y) is the unsigned-ordered 32-bit key of y: Float32 with bits b: b ^ (b < 0 ? 0xFFFFFFFF : 0x80000000) -- IEEE totalOrder,
 *      -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, the order K4's predicate uses and arrow-rs' / DataFusion's ungrouped
 *      MinAccumulator (min_max.rs, total_cmp) --; Int32: b ^ 0x80000000.  A word of 0 means "no value yet" and BOTH extreme planes
 *      fold by unsigned max, so a zeroed state is the empty state and two states merge by add (counts) / max (extremes):
 *      exon_hip_plan_fold_states.  exon_hip_minmax_decode turns the words back into values.
 *      1 <= n_groups <= EXON_HIP_MAX_GROUPS; more is EXON_HIP_EUNSUPPORTED (K4's tier beyond the LDS table is not extended to this
 *      operator).  Nullable group ids are refused and an id outside [0, n_groups) is reported as for K4.  Accumulates.  The bare
 *      operator takes Float32 x and y, like K4's; Int32 columns go through a plan (exon_hip_plan_desc.x_type / y_type). */
int exon_hip_cmp_minmax_by_group(exon_hip_ctx* ctx, void* stream, const exon_hip_column* x /*f32*/,
                                 const exon_hip_column* y /*f32*/, const exon_hip_column* group_id /*i32*/,
                                 int64_t n, double threshold, int32_t cmp_op, int32_t n_groups,
                                 int64_t* d_state /*[4*n_groups]*/);
/* Host-only: n state words of K8's min plane (is_min != 0) or max plane -> values.  y_type: EXON_HIP_X_FLOAT32 / EXON_HIP_X_INT32.
 * out_values receives n 4-byte values (float or int32 bit patterns), out_valid n bytes: 0 where the word is 0 (no value). */
int exon_hip_minmax_decode(const int64_t* words, int64_t n, int32_t is_min, int32_t y_type, void* out_values /*n x 4 bytes*/,
                           uint8_t* out_valid /*n bytes*/);

/* K5.  d_hist[p*256 + b] += |{ reads r, p < len(r) : bytes[offsets[r] + p] == b }| for p < lmax;
 *      positions >= lmax are an error (status word, reported by exon_hip_stream_finish / sync). */
int exon_hip_qual_pos_hist(exon_hip_ctx* ctx, void* stream, const exon_hip_column* quality_scores /*utf8*/,
                           int64_t n_reads, int32_t lmax, int64_t* d_hist /*[lmax*256]*/);

/* K5 over a column held as several Arrow batches ("chunks": a Utf8 column has int32 offsets, so a quality column beyond
 * 2^31 bytes IS several batches -- the reference streams 8192-row batches into one accumulator).  chunks[c] is a utf8
 * column of n_reads[c] reads; chunks with n_reads[c] == 0 are skipped.  Equivalent to calling exon_hip_qual_pos_hist per
 * chunk, but up to 64 chunks share ONE offsets scan, ONE main kernel (the per-workgroup LDS histograms live across
 * chunks) and ONE fold instead of three launches each. */
int exon_hip_qual_pos_hist_chunks(exon_hip_ctx* ctx, void* stream, const exon_hip_column* chunks /*utf8 each*/,
                                  int32_t n_chunks, const int64_t* n_reads, int32_t lmax, int64_t* d_hist /*[lmax*256]*/);

/* K5 over independent views: read r is bytes[starts[r] .. ends[r]) of `d_bytes` (all device pointers).  Used for
 * the quality (or sequence) lines of raw FASTQ text resident in HBM (exon_hip_fastq_parser_parse): no Arrow
 * column is materialised. */
int exon_hip_qual_pos_hist_views(exon_hip_ctx* ctx, void* stream, const uint8_t* d_bytes, const int32_t* d_starts,
                                 const int32_t* d_ends, int64_t n_reads, int32_t lmax, int64_t* d_hist /*[lmax*256]*/);

/* K9.  Per-READ statistics of FASTQ reads (s = sequence bytes, q = quality bytes; each line measured by its OWN length), integers
 *      only.  d_state holds 4 + (lmax + 1) + 102 + 257 int64 words (exon_hip_read_stats_layout), and every word adds:
 *        totals       [4]         n_reads, sum len(s), sum gc(s), sum over all q bytes of the raw byte
 *        length       [lmax + 1]  bin L = reads with len(s) == L
 *        gc_percent   [102]       bin floor(100 gc(s) / len(s)) (0 .. 100); bin 101 = reads with an empty sequence (gc_content's 0/0).
 *                                 gc(s) = bytes equal to 'G' or 'C', upper case only (exon-core/src/udfs/sequence/gc_content.rs:52-71).
 *                                 The bin is the exact integer floor, not floor(gc_content(s) * 100) in Float32
 *        mean_quality [257]       bin floor(sum of q's bytes / len(q)) on the RAW byte (Phred = bin - 33); bin 256 = empty quality line
 *      1 <= lmax <= 65536.  A read with len(s) > lmax, or len(q) > 65536, is an error (status word, reported by
 *      exon_hip_stream_finish / sync, as K5's position >= lmax); such a read adds nothing.  Accumulates. */
int exon_hip_read_stats_hist(exon_hip_ctx* ctx, void* stream, const exon_hip_column* sequence /*utf8*/,
                             const exon_hip_column* quality /*utf8*/, int64_t n_reads, int32_t lmax, int64_t* d_state);
/* K9 over independent views into `d_bytes` (raw FASTQ text resident in HBM, exon_hip_fastq_parser_parse): read r has the sequence
 * bytes [seq_s[r], seq_e[r]) and the quality bytes [qual_s[r], qual_e[r]).  No byte outside a line is loaded. */
int exon_hip_read_stats_hist_views(exon_hip_ctx* ctx, void* stream, const uint8_t* d_bytes, const int32_t* seq_s, const int32_t* seq_e,
                                   const int32_t* qual_s, const int32_t* qual_e, int64_t n_reads, int32_t lmax, int64_t* d_state);
/* Host-only: out[0..3] = word offset of K9's totals / length / gc_percent / mean_quality sections, out[4] = the state's words.
 * EXON_HIP_EINVAL outside 1 <= lmax <= 65536.  Needs no device. */
int exon_hip_read_stats_layout(int32_t lmax, int64_t* out /*[5]*/);

/* ---- synthetic inputs generated in HBM (DESIGN.md "Synthetic inputs"; bit-identical to the
 *      oracle's generators, which the parity tests check) ------------------------------------- */
int exon_hip_gen_c2(exon_hip_ctx* ctx, void* stream, uint64_t seed, int64_t n_total, int64_t lo, int64_t hi,
                    int32_t* d_chrom_id, int64_t* d_pos);
int exon_hip_gen_c3(exon_hip_ctx* ctx, void* stream, uint64_t seed, int64_t lo, int64_t hi, int32_t* d_flag,
                    uint8_t* d_mapq, uint8_t* d_mapq_valid, int32_t* d_ref_id, uint8_t* d_ref_valid);
int exon_hip_gen_c4(exon_hip_ctx* ctx, void* stream, uint64_t seed, int64_t lo, int64_t hi, float* d_af,
                    uint8_t* d_af_valid, float* d_qual, uint8_t* d_qual_valid, int32_t* d_filter_id);
/* alignments for K6: reference id (+validity), start / end (+ one shared validity; unmapped rows have neither) */
int exon_hip_gen_c6(exon_hip_ctx* ctx, void* stream, uint64_t seed, int64_t lo, int64_t hi, int32_t* d_ref_id,
                    uint8_t* d_ref_valid, int64_t* d_start, int64_t* d_end, uint8_t* d_pos_valid);
int exon_hip_gen_c5(exon_hip_ctx* ctx, void* stream, uint64_t seed, int64_t lo, int64_t hi, int32_t read_len,
                    int32_t* d_offsets, uint8_t* d_bytes);

/* ---- host-side planning helpers ------------------------------------------------------------ */
/* noodles Region grammar `name[:start[-end]]`, 1-based inclusive; end = EXON_HIP_REGION_OPEN_END
 * when open (exon-core/src/physical_plan/infer_region.rs:25-42). */
int exon_hip_parse_region(const char* region, char* name_out, size_t name_cap, int64_t* start, int64_t* end);
/* Whole files, ascending size, dealt round-robin into min(target, n) groups.  group_of[i] = group of
 * file i; returns the number of groups (or a negative status). */
int exon_hip_regroup_files_by_size(const int64_t* sizes, int32_t n_files, int32_t target_groups, int32_t* group_of);

/* ---- plan / stream: the ExecutionPlan-shaped surface -------------------------------------- */
#define EXON_HIP_PLAN_REGION_COUNT 2
#define EXON_HIP_PLAN_FLAG_MAPQ_GROUP_COUNT 3
#define EXON_HIP_PLAN_CMP_AVG_BY_GROUP 4
#define EXON_HIP_PLAN_QUAL_POS_HIST 5
#define EXON_HIP_PLAN_OVERLAP_COUNT 6 /* region_chrom_id / region_start / region_end; columns: ref_id, start, end */
#define EXON_HIP_PLAN_WITHIN_COUNT 7  /* same fields, strict form: start > region_start AND end < region_end */
/* K4's fields (cmp_op, threshold, x_type, y_type, n_groups <= EXON_HIP_MAX_GROUPS, columns x, y, group_id); state: 4 * n_groups int64.
 * The min / max words are keys of y's TYPE, so the type belongs to a stream's state: exon_hip_stream_consume_scan takes it from
 * the first file's header and refuses (EXON_HIP_ESTATE, the stream unchanged) a later file that types the argument otherwise;
 * exon_hip_stream_reset starts over.  Ranks that merge such states must have agreed on the type (the plan's, or the same files' headers). */
#define EXON_HIP_PLAN_CMP_MINMAX_BY_GROUP 8
/* K9: lmax, columns: sequence, quality_scores (both Utf8; (2, 3) of a FASTQ scan); state: exon_hip_read_stats_layout words, all add */
#define EXON_HIP_PLAN_READ_STATS_HIST 9
/* K10: lmax, columns: sequence (Utf8; column 2 of a FASTA scan and of a FASTQ scan); state: exon_hip_seq_stats_layout words, all add */
#define EXON_HIP_PLAN_SEQ_STATS_HIST 10

#define EXON_HIP_X_FLOAT32 0
#define EXON_HIP_X_INT32 1
typedef struct exon_hip_plan_desc {
  int32_t kind;          /* EXON_HIP_PLAN_* */
  int32_t n_groups;      /* K3: n_refs; K4 / K8: dictionary size; else 0 */
  /* K2 */
  int32_t region_chrom_id;
  /* K4: type of the compared column x.  EXON_HIP_X_FLOAT32 (0): Float32, widened to Float64 and compared in IEEE totalOrder.
   * EXON_HIP_X_INT32 (1): Int32 -- an INFO field of Type=Integer (exon-core/src/datasources/vcf/schema_builder.rs:197-205);
   * compared exactly (DataFusion: as Int64 against an integer literal, as Float64 against a float literal -- every int32
   * is exact in both), never through f32.  exon_hip_stream_consume_scan takes the type from the file's header instead. */
  int32_t x_type;
  int64_t region_start, region_end;
  /* K3 */
  int32_t flag_mask, flag_value, mapq_min;
  /* K4 */
  int32_t cmp_op;
  double threshold;
  /* K5 */
  int32_t lmax;
  /* K4: type of AVG's argument y, EXON_HIP_X_FLOAT32 / EXON_HIP_X_INT32 (DataFusion's avg casts either to Float64) */
  int32_t y_type;
  /* input column indexes into the batch's children, in operator argument order
   * (K2: chrom_id,pos  K3: flag,mapq,ref_id  K4: x,y,group_id  K5: quality_scores  K6: ref_id,start,end  K9: sequence,quality_scores  K10: sequence) */
  int32_t columns[4];
} exon_hip_plan_desc;

int exon_hip_plan_create(exon_hip_ctx* ctx, const exon_hip_plan_desc* desc, exon_hip_plan** out);
int exon_hip_plan_destroy(exon_hip_plan* plan);
/* number of int64 / float64 words of the partial-aggregate state of this plan */
int exon_hip_plan_state_size(const exon_hip_plan* plan, int64_t* n_i64, int64_t* n_f64);

/* ---- K11: overlap counts for a whole region set in one pass (plan kind 11) -------------------------------------------------------
 * K6's question for M regions at once -- what `bedtools multicov` / `intersect -c` answer, a join + GROUP BY in the reference: for
 * every region i, the rows with ref_id = the region's contig AND start <= re_i AND end >= rs_i, all three valid, 1-based inclusive.
 * Every row is visited once, whatever M is: per contig the region ends and the region starts are sorted; a row [s, e] finds
 * p = |{ i : re_i < s }| and q = |{ i : rs_i <= e }| by two binary searches and adds 1 to A[p] and to B[q]; region i of rank a_i among
 * the ends and b_i among the starts then has  count_i = sum(A[0 .. a_i]) - sum(B[0 .. b_i])  (DESIGN.md 3.5).
 *
 * The region set does not fit exon_hip_plan_desc, so the plan has a constructor of its own (exon_hip_plan_create with kind 11 is
 * EXON_HIP_EINVAL and names it).  columns: ref_id (Int32), start (Int64), end (Int64) -- K6's order.
 *   1 <= n_regions <= 1048576 (more: EXON_HIP_EUNSUPPORTED); every region 1 <= start <= end, end may be EXON_HIP_REGION_OPEN_END;
 *   duplicate, nested and overlapping regions are legal, each has its own count.
 *   ids form (packed_contig_names NULL): ref_ids[i] is the caller's or the file's own id, as K6's region_chrom_id; a negative id is
 *     EXON_HIP_EINVAL, one of EXON_HIP_MAX_REFERENCES or more EXON_HIP_EUNSUPPORTED (the id -> contig map is a dense table).
 *   names form: n_regions '\0'-terminated names in packed_bytes bytes.  exon_hip_stream_consume_scan resolves every distinct name in
 *     that scan's contig / reference dictionary by exon_hip_stream_set_region_contig's rule (a name the file lacks contributes no
 *     rows; formats without a header may intern it), so files with different header orders add up in one stream.  Such a plan has
 *     no ids of its own: exon_hip_stream_push, exon_hip_stream_push_device, exon_hip_plan_launch and the bare operator are
 *     EXON_HIP_ESTATE.
 *   ctx may be NULL: a host-only plan that serves exon_hip_region_set_layout / _decode / exon_hip_plan_state_size and nothing else.
 *
 * State: 4 + 2 * (M + C) int64 words, n_f64 = 0; M = regions, C = distinct contigs of the set.  Every word adds, so streams, chunked
 * launches, exon_hip_plan_fold_states, exon_hip_stream_all_reduce and the file pipelines carry it like K9's and K10's; the words are
 * keyed by the region set, not by a file's dictionary.
 *   totals[4]  counted, null_rows (any of the three values invalid), elsewhere (the contig is not in the set: also an id below 0 or
 *              beyond the map), inverted (end < start); the four sum to the rows seen
 *   A[M + C], B[M + C]  contig c (in order of first appearance in the set, m_c regions) owns m_c + 1 consecutive bins of each
 * DECISION: a row with end < start adds to `inverted` and to NO region.  K6 would count such a row for a region that strictly
 * contains the gap between end and start; the identity above needs s <= e, and no reader here emits such a row for a valid file.
 *
 * The device tables (id -> contig map, per-contig offsets, sorted ends and starts) are built once and owned by the plan.  Sets with
 * M + C <= 6144 are searched and counted in LDS; larger ones search through L2 and count with global atomics.  The columns' values
 * need their element's alignment only (4 / 8 / 8 bytes). */
#define EXON_HIP_PLAN_REGION_SET_OVERLAP 11
#define EXON_HIP_REGION_SET_MAX_REGIONS 1048576
int exon_hip_plan_create_region_set(exon_hip_ctx* ctx, const int32_t* columns /*[3]*/,
                                    const char* packed_contig_names /* n_regions '\0'-terminated names, or NULL */, size_t packed_bytes,
                                    const int32_t* ref_ids /* used when names are NULL */, const int64_t* starts, const int64_t* ends,
                                    int32_t n_regions, exon_hip_plan** out);
/* host only: out = word offsets of totals, A, B, and the word count */
int exon_hip_region_set_layout(const exon_hip_plan* plan, int64_t* out /*[4]*/);
/* host only: the state's words -> one count per region, in the caller's region order.  Linear: decoded partial states add up to the
 * decoded merged state. */
int exon_hip_region_set_decode(const exon_hip_plan* plan, const int64_t* state, int64_t* out_counts /*[M]*/);
/* K11, bare operator (ids form; `ctx` is the plan's): d_state (exon_hip_plan_state_size words) += this batch */
int exon_hip_region_set_overlap(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id /*i32*/, const exon_hip_column* start /*i64*/,
                                const exon_hip_column* end /*i64*/, int64_t n, const exon_hip_plan* plan, int64_t* d_state);

/* ---- K12: covered bases per region of a set in one pass (plan kind 12) ------------------------------------------------------------
 * The depth question over K11's inputs -- the sum `samtools bedcov` / `bedtools coverage` print; mean depth is that sum divided by
 * the region's length.  Rows and regions are 1-based inclusive.  A row [s, e] with s <= e on a region's contig, all three values
 * valid, covers  max(0, min(e, re_i) - max(s, rs_i) + 1)  bases of the region [rs_i, re_i]; bases_i is the sum over such rows.
 * Every row is visited once, whatever M is.  Per contig the POINTS are the sorted unique values { rs_i - 1 } U { re_i }: k_c points
 * x_0 < ... < x_{k_c - 1}.  A counted row finds p = the index of the first point >= s and q = the index of the first point >= e (the
 * same lower bound in the same table, both in [0, k_c]) and adds 1 to Ns[p], s to Ss[p], 1 to Ne[q], e to Se[q].  With inclusive
 * prefix sums cNs, cSs, cNe, cSe over the contig's bins
 *     G(x_r)  = (x_r + 1) * cNs[r] - cSs[r] - x_r * cNe[r] + cSe[r]      bases of the contig's rows at positions <= x_r
 *     bases_i = G(re_i) - G(rs_i - 1)                                    
 * ARITHMETIC IS MODULO 2^64: the four sections and the decode use unsigned 64-bit arithmetic that wraps.  Every step is a ring
 * operation, so bases_i is exact whenever its true value fits an int64 -- also for re_i = EXON_HIP_REGION_OPEN_END, where x + 1
 * wraps, and for coordinate sums beyond 2^63.  A single word of Ss / Se is therefore meaningful only modulo 2^64.
 *
 * What it does not compute: the alignment span [start, end] counts as covered, deletions and reference skips included, as the `end`
 * column defines it (the CIGAR-aware rows are exon_hip_cigar_blocks'); there is no per-base depth, only the sum per region; a BED
 * source is not served.
 *
 * exon_hip_plan_create_region_set_bases takes exon_hip_plan_create_region_set's arguments under the same rules and error classes
 * (ids form or names form, 1 <= start <= end with an open end allowed, at most 1048576 regions, ctx may be NULL for a host-only
 * plan; exon_hip_plan_create with kind 12 is EXON_HIP_EINVAL and names the constructor).  A names-form plan is resolved per consumed
 * scan exactly as kind 11's and refuses pushes, device pushes, plan launches and the bare operator with EXON_HIP_ESTATE.  Duplicate,
 * nested and overlapping regions are legal, each has its own sum.  Kind 11's helpers refuse a kind-12 plan and these refuse kind 11's.
 *
 * State: 4 + 4 * (P + C) int64 words, n_f64 = 0; P = sum of k_c, C = distinct contigs of the set.  Every word adds (modulo 2^64), so
 * streams, chunked launches, exon_hip_plan_fold_states, exon_hip_stream_all_reduce and the file pipelines carry it like K11's.
 *   totals[4]  counted, null_rows, elsewhere, inverted: exactly kind 11's
 *   Ns[P + C], Ss[P + C], Ne[P + C], Se[P + C]  contig c (in order of first appearance in the set) owns k_c + 1 consecutive bins
 *              of each section, starting at (points of the contigs in front of it) + c
 * DECISION (kind 11's): a row with end < start adds to `inverted` and to NO region.
 *
 * Sets with P + C <= 4096 are searched and summed in LDS; larger ones search through L2 and add with global atomics.  The columns'
 * values need their element's alignment only (4 / 8 / 8 bytes).  finish_arrow: contig, start, end, bases (Int64), one row per region
 * in the caller's order. */
#define EXON_HIP_PLAN_REGION_SET_BASES 12
int exon_hip_plan_create_region_set_bases(exon_hip_ctx* ctx, const int32_t* columns /*[3]*/,
                                          const char* packed_contig_names /* n_regions '\0'-terminated names, or NULL */, size_t packed_bytes,
                                          const int32_t* ref_ids /* used when names are NULL */, const int64_t* starts, const int64_t* ends,
                                          int32_t n_regions, exon_hip_plan** out);
/* host only: out = word offsets of totals, Ns, Ss, Ne, Se, and the word count */
int exon_hip_region_bases_layout(const exon_hip_plan* plan, int64_t* out /*[6]*/);
/* host only: the state's words -> the covered bases of every region, in the caller's region order.  Linear modulo 2^64: decoded
 * partial states add up to the decoded merged state. */
int exon_hip_region_bases_decode(const exon_hip_plan* plan, const int64_t* state, int64_t* out_bases /*[M]*/);
/* K12, bare operator (ids form; `ctx` is the plan's): d_state (exon_hip_plan_state_size words) += this batch */
int exon_hip_region_set_bases(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id /*i32*/, const exon_hip_column* start /*i64*/,
                              const exon_hip_column* end /*i64*/, int64_t n, const exon_hip_plan* plan, int64_t* d_state);

/* ---- K13: bases per fixed-width window along each contig in one pass (plan kind 13) -------------------------------------------------
 * The depth question without a BED file -- what `mosdepth --by W`, `bedtools makewindows | bedtools coverage` and every coverage
 * track compute; mean depth is bases / window length.  Inputs are K6 / K11 / K12's three columns, 1-based inclusive.  The plan holds
 * a window width W >= 1 and C >= 1 contigs of lengths 1 <= L_c <= 2^31 - 1 (BAM's own limit).  Contig c has K_c = ceil(L_c / W)
 * windows, window j = [j * W + 1, min((j + 1) * W, L_c)]; B = sum of K_c, woff[c] = windows in front of contig c.  B may be at most
 * EXON_HIP_WINDOW_MAX_BINS (a state of 512 MiB); more is EXON_HIP_EUNSUPPORTED.  bases_j is the sum over the counted rows [s, e] of
 * the bases of the row inside window j.  The row classes and the four totals are exactly kind 11's.
 * DECISIONS: a counted row is CLIPPED to [1, L_c]; a counted row with s > L_c or e < 1 stays `counted` and adds to no window.
 *
 * Every row is visited once and the window of a coordinate is a division, not a search.  With js = (s - 1) / W and je = (e - 1) / W
 * of the clipped row:
 *     js == je:      E[js] += e - s + 1
 *     otherwise:     E[js] += (js + 1) * W - s + 1,   E[je] += e - je * W
 *     je > js + 1:   D[js + 1] += 1,   D[je] -= 1
 * and per contig  bases_j = E[j] + W * (D[0] + ... + D[j])  (DESIGN.md 3.7): a window strictly between two others is never a contig's
 * short last window.  ARITHMETIC IS MODULO 2^64, as kind 12's; the -1 is an add of 2^64 - 1.
 *
 * What it does not compute: the alignment span [start, end] counts as covered, deletions and reference skips included (the
 * CIGAR-aware rows are exon_hip_cigar_blocks'); there is no per-base track, only the sum per window (W = 1 gives one, at 16 bytes a
 * base); a BED source is not served.
 *
 * exon_hip_plan_create_window_bases names its contigs by kind 11 / 12's rules and error classes: ids form (packed_contig_names NULL;
 * a negative id is EXON_HIP_EINVAL, one of EXON_HIP_MAX_REFERENCES or more EXON_HIP_EUNSUPPORTED) or names form (n_contigs
 * '\0'-terminated names; an empty name or too few names is EXON_HIP_EINVAL; resolved per consumed scan; exon_hip_stream_push,
 * exon_hip_stream_push_device, exon_hip_plan_launch and the bare operator are EXON_HIP_ESTATE).  A contig given twice, window < 1,
 * n_contigs < 1 and a length outside [1, 2^31 - 1] are EXON_HIP_EINVAL.  ctx may be NULL: a host-only plan for the three helpers
 * below and exon_hip_plan_state_size.  exon_hip_plan_create with kind 13 is EXON_HIP_EINVAL and names this constructor.  Kind 11 /
 * 12's helpers refuse a kind-13 plan and these refuse kinds 11 / 12.
 *
 * State: 4 + 2 * B int64 words, n_f64 = 0: totals[4] (counted, null_rows, elsewhere, inverted), E[B], D[B]; contig c (in the caller's
 * order) owns bins [woff[c], woff[c + 1]) of E and of D.  Every word adds (modulo 2^64), so streams, chunked launches,
 * exon_hip_plan_fold_states, exon_hip_stream_all_reduce and the file pipelines carry it like kind 11's and 12's.
 *
 * Plans with B <= 8192 add in LDS; larger ones add to the state with global atomics.  The columns' values need their element's
 * alignment only (4 / 8 / 8 bytes).  finish_arrow: contig (Int32, or Utf8 in the names form), start, end (Int64, 1-based closed),
 * bases (Int64), one row per window in contig order, then window order. */
#define EXON_HIP_PLAN_WINDOW_BASES 13
#define EXON_HIP_WINDOW_MAX_BINS 33554432
int exon_hip_plan_create_window_bases(exon_hip_ctx* ctx, const int32_t* columns /*[3]*/,
                                      const char* packed_contig_names /* n_contigs '\0'-terminated names, or NULL */, size_t packed_bytes,
                                      const int32_t* ref_ids /* used when names are NULL */, const int64_t* lengths, int32_t n_contigs,
                                      int64_t window, exon_hip_plan** out);
/* host only: out = word offsets of totals, E, D, and the word count */
int exon_hip_window_bases_layout(const exon_hip_plan* plan, int64_t* out /*[4]*/);
/* host only: woff[c] = windows in front of contig c; woff[C] = B */
int exon_hip_window_bases_offsets(const exon_hip_plan* plan, int64_t* woff /*[C + 1]*/);
/* host only: the state's words -> the bases of every window, contig by contig.  Linear modulo 2^64: decoded partial states add up to
 * the decoded merged state. */
int exon_hip_window_bases_decode(const exon_hip_plan* plan, const int64_t* state, int64_t* out_bases /*[B]*/);
/* K13, bare operator (ids form; `ctx` is the plan's): d_state (exon_hip_plan_state_size words) += this batch */
int exon_hip_window_bases(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id /*i32*/, const exon_hip_column* start /*i64*/,
                          const exon_hip_column* end /*i64*/, int64_t n, const exon_hip_plan* plan, int64_t* d_state);

/* ---- K14: per-base depth over a region set, threshold counts per region, in one pass (plan kind 14) ----------------------------------
 * The QC question on a target list -- how much of each target is covered at least 1x, 10x, 20x, 30x: `mosdepth --thresholds`, Picard's
 * PCT_TARGET_BASES_20X; `samtools depth -b targets.bed` lists the per-base values.  None of it follows from kind 12's or 13's sums.
 * Inputs are K6 / K11 - K13's three columns, 1-based inclusive; the row classes and the four totals are exactly kind 11's.
 *
 * TARGET SPACE.  Contigs in order of first appearance in the set.  Per contig the regions are sorted and merged into disjoint
 * intervals [ms_j, me_j]: two merge when the next start <= the current end + 1, so overlapping and abutting regions both merge.
 * cum_j = the bases of the contig's intervals in front of interval j, T_c = the contig's target bases, T = sum of T_c.  Contig c owns
 * T_c + 1 consecutive bins from doff_c = (T of the contigs in front) + c: a bin per target base, then a terminator.  T + C may be at
 * most EXON_HIP_REGION_DEPTH_MAX_BINS (a state of 512 MiB, kind 13's bound; more is EXON_HIP_EUNSUPPORTED): panels, exomes and the
 * smaller chromosomes whole; kind 13 stays the answer for whole genomes.
 * COMPRESSED COORDINATE.  below_c(x) = the contig's target bases at positions <= x: with j = the intervals with ms <= x, 0 if j = 0,
 * else cum_{j-1} + min(x - ms_{j-1} + 1, len_{j-1}), computed without overflow for every int64 x.  A region [rs, re] is the bins
 * [below(rs - 1), below(re)) of its contig, re - rs + 1 of them.
 *
 * State: 4 + T + C int64 words, n_f64 = 0: totals[4] (counted, null_rows, elsewhere, inverted), D[T + C].  A counted row [s, e] takes
 * lo = below(s - 1) (0 when s <= 1) and hi = below(e); if hi > lo it adds 1 to D[doff_c + lo] and 2^64 - 1 to D[doff_c + hi], else
 * nothing: a read across the gap between two targets is still one pair of adds, a read inside a gap none.  Every word adds MODULO
 * 2^64, so streams, chunked launches, exon_hip_plan_fold_states, exon_hip_stream_all_reduce and the file pipelines carry the state
 * like kinds 11 - 13's.  Each contig's bins sum to 0 in every state that adds can produce, so THE DEPTH OF BIN b IS DEFINED AS THE
 * RUNNING SUM OF THE WHOLE SECTION D[0] + ... + D[b], one array, on the host and on the device: the two agree word for word on any
 * input.  DECISION (kind 11's): a row with end < start adds to `inverted` and to no bin.
 * THE DECODE IS NOT LINEAR: bases_i adds over partial states, the threshold counts do not.  Add the states, then decode or reduce.
 *
 * What it does not compute: the alignment span [start, end] counts as covered, deletions and reference skips included (the
 * CIGAR-aware rows are exon_hip_cigar_blocks'); a BED source is not served; there are no open-ended regions.
 *
 * exon_hip_plan_create_region_set_depth takes exon_hip_plan_create_region_set's region arguments under the same rules and error
 * classes (ids form or names form, 1 <= start <= end, at most 1048576 regions, duplicate, nested and overlapping regions legal and
 * each with its own result, ctx may be NULL for a host-only plan; exon_hip_plan_create with kind 14 is EXON_HIP_EINVAL and names the
 * constructor; a names-form plan refuses pushes, device pushes, plan launches and the bare operator with EXON_HIP_ESTATE).  Its own:
 * end == EXON_HIP_REGION_OPEN_END is EXON_HIP_EUNSUPPORTED (a per-base state needs a finite end); 0 <= n_thresholds <=
 * EXON_HIP_REGION_DEPTH_MAX_THRESHOLDS, every threshold >= 1, the list strictly increasing, anything else EXON_HIP_EINVAL.  Kind 11 /
 * 12 / 13's helpers refuse a kind-14 plan and these refuse the other kinds.
 *
 * Plans with T + C <= 8192 add in LDS (the interval table beside the bins when both fit 128 KiB); larger ones search through L2 and
 * add with global atomics.  The columns' values need their element's alignment only (4 / 8 / 8 bytes).  finish_arrow runs the reduce
 * on the device and copies M * (1 + k) words: contig (Int32, or Utf8 in the names form), start, end, bases, then ge_<T> for each
 * threshold T, all Int64, one row per region in the caller's order. */
#define EXON_HIP_PLAN_REGION_SET_DEPTH 14
#define EXON_HIP_REGION_DEPTH_MAX_BINS 67108864
#define EXON_HIP_REGION_DEPTH_MAX_THRESHOLDS 8
int exon_hip_plan_create_region_set_depth(exon_hip_ctx* ctx, const int32_t* columns /*[3]*/,
                                          const char* packed_contig_names /* n_regions '\0'-terminated names, or NULL */, size_t packed_bytes,
                                          const int32_t* ref_ids /* used when names are NULL */, const int64_t* starts, const int64_t* ends,
                                          int32_t n_regions, const int64_t* thresholds, int32_t n_thresholds, exon_hip_plan** out);
/* host only: out = word offsets of totals and D, and the word count */
int exon_hip_region_depth_layout(const exon_hip_plan* plan, int64_t* out /*[3]*/);
/* host only: the merged intervals in bin order: *n of them, each with its contig slot, its 1-based closed [start, end] and the bin of
 * its first base.  Any of the four arrays may be NULL; all NULL asks for *n alone. */
int exon_hip_region_depth_intervals(const exon_hip_plan* plan, int32_t* n, int32_t* slot, int64_t* start, int64_t* end, int64_t* bin);
/* host only: the state's words -> the depth of every target base in bin order, the C terminator bins left out (what `samtools depth
 * -b` lists) */
int exon_hip_region_depth_per_base(const exon_hip_plan* plan, const int64_t* state, int64_t* out_depth /*[T]*/);
/* host only: the state's words -> row-major [M][1 + k], per region in the caller's order: bases = the sum of the depths over the
 * region's bins (kind 12's bases_i for the same rows and regions), then ge_t = the region's bases whose depth, read as int64, is
 * >= thresholds[t] */
int exon_hip_region_depth_decode(const exon_hip_plan* plan, const int64_t* state, int64_t* out /*[M * (1 + k)]*/);
/* the same table made on the device, on the caller's stream (`ctx` is the plan's), equal to _decode word for word.  d_state is only
 * read; nothing proportional to T crosses to or from the host.  The running sum is taken in tiles of 256 bins. */
int exon_hip_region_depth_reduce(exon_hip_ctx* ctx, void* stream, const exon_hip_plan* plan, const int64_t* d_state, int64_t* d_out /*[M * (1 + k)]*/);
/* K14, bare operator (ids form; `ctx` is the plan's): d_state (exon_hip_plan_state_size words) += this batch */
int exon_hip_region_set_depth(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id /*i32*/, const exon_hip_column* start /*i64*/,
                              const exon_hip_column* end /*i64*/, int64_t n, const exon_hip_plan* plan, int64_t* d_state);

/* ---- aligned blocks: alignment rows -> the CIGAR-aware interval rows of kinds 12 - 14 (additive; the ABI stays 5) -------------------
 * Kinds 12 - 14 count a row's whole span [start, end].  For alignments that is `bedtools`' / `samtools bedcov`'s default and the wrong
 * answer for `samtools depth` and `bedcov -j`: the intron of a spliced read (50M10000N50M) and every deletion count as covered.  All
 * three plans add per base, so a read may be replaced by its disjoint aligned blocks with no change to any plan: this operator makes
 * the block rows, the plans' operators (or exon_hip_stream_push_device) take them as they take any interval rows.
 *
 * cover_ops: bit i = "the reference positions under a CIGAR op of BAM code i are covered" (codes: M 0, I 1, D 2, N 3, S 4, H 5, P 6,
 * = 7, X 8).  Legal bits are the ops that consume the reference, M D N = X: a non-empty subset of 0x18D, anything else is
 * EXON_HIP_EINVAL.  EXON_HIP_COVER_ALIGNED (M = X) is `samtools depth` and `bedcov -j`, EXON_HIP_COVER_ALIGNED_DEL (+ D) is `samtools
 * depth -J`, 0x18D gives the span back.
 * THE RULE (exon_amd/csrc/host/cigar_blocks.h, one function for the host and both device passes).  Walk the ops from `start`: an op
 * whose code is in 0x18D advances the position by its length, counted or not; every other op (codes 9 - 15 included) advances
 * nothing.  The covered positions are the union of the counted ops' intervals, and a BLOCK is a maximal run of consecutive covered
 * positions, 1-based inclusive like its row: 10M5I10M is one block, 5M0N5M is one, 5M3D5M without D is two, a zero-length counted op
 * makes none.  A record has k >= 0 blocks.  Ops are u32 in BAM's encoding, len << 4 | code.
 *
 * exon_hip_cigar_blocks: n rows of ref_id (i32) and start (i64), each with an optional validity bitmap, and an Arrow List<UInt32> of
 * ops on the device: d_cigar_offsets[n + 1] (int32, the first may be non-zero, in order) and d_cigar_ops.  Row r emits max(1, k)
 * rows of (d_out_ref, d_out_start, d_out_end) and one bit each of d_out_valid, ONE bitmap for the three columns: a row whose ref_id or
 * start is NULL emits one invalid row (values 0); a valid row of k = 0 emits the valid row [start, start - 1], which the plans count
 * as `inverted`, as they count such a record in span mode; a valid row of k >= 1 emits its blocks in order.  So the plans' four
 * totals count BLOCK ROWS, not records.  cap = the rows the three value buffers hold; d_out_valid holds 4 * ceil(cap / 32) bytes and
 * is 4-byte aligned (bits behind the last row of its last word are 1).  *n_blocks = the rows emitted.  When cap is too small the call
 * is EXON_HIP_ECAPACITY, *n_blocks is the need and NOTHING has been written (cap = 0 with NULL buffers asks for the need alone).
 * Offsets out of order are EXON_HIP_EINVAL; no op is loaded from outside [offsets[0], offsets[n]).  n = 0 is OK and launches nothing;
 * n >= 2^31 is EXON_HIP_EUNSUPPORTED.  SYNCHRONOUS on `stream` (the total comes back in one small copy between the two passes).  Values
 * need their element's alignment only.  A BAM record whose CIGAR is the two-op placeholder of a CG tag cannot be told from its ops
 * alone: a caller that decodes BAM itself must expand or refuse it before this call.
 * exon_hip_cigar_blocks_host: the rule for ONE record on the host, no ctx and no device: the first min(k, cap) blocks into out_start /
 * out_end, *n_blocks = k; k > cap is EXON_HIP_ECAPACITY, n_ops = 0 gives k = 0.
 * BAM and SAM scans make the same rows themselves: exon_hip_scan_set_cover_ops.  Not here: CRAM, the CG tag, mate-overlap
 * correction. */
#define EXON_HIP_COVER_ALIGNED 0x181u     /* M = X */
#define EXON_HIP_COVER_ALIGNED_DEL 0x185u /* M D = X */
int exon_hip_cigar_blocks(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id /*i32*/, const exon_hip_column* start /*i64*/,
                          const int32_t* d_cigar_offsets /*[n + 1]*/, const uint32_t* d_cigar_ops, int64_t n, uint32_t cover_ops,
                          int32_t* d_out_ref, int64_t* d_out_start, int64_t* d_out_end, uint8_t* d_out_valid, int64_t cap, int64_t* n_blocks);
int exon_hip_cigar_blocks_host(const uint32_t* ops, int32_t n_ops, int64_t start, uint32_t cover_ops, int64_t* out_start, int64_t* out_end,
                               int32_t cap, int32_t* n_blocks);

/* Stateless form of a push: run the plan's fused kernel over HBM-resident columns (`columns[i]` = operator argument i, see
 * exon_hip_plan_desc.columns for the order; n_columns must match the plan) on the caller's hipStream_t into a caller-owned
 * packed partial state [n_i64 x int64][n_f64 x float64] (exon_hip_plan_state_size; 8-byte aligned device memory).
 * EXON_HIP_LAUNCH_ACCUMULATE: state += this batch.  EXON_HIP_LAUNCH_OVERWRITE: state := this batch -- the first batch of a
 * query then needs no zeroing kernel in front of it (AggregateExec(Partial) starting from empty accumulators). */
#define EXON_HIP_LAUNCH_ACCUMULATE 0
#define EXON_HIP_LAUNCH_OVERWRITE 1
int exon_hip_plan_launch(exon_hip_plan* plan, void* stream, const exon_hip_column* columns, int32_t n_columns, int64_t n,
                         int32_t flags, void* d_state);
/* The same over a table held as n_chunks batches: columns[c * n_columns + i] = operator argument i of chunk c, n[c] its rows.
 * `flags` applies to the whole call (OVERWRITE: state := all chunks).  Plans of kind QUAL_POS_HIST fuse up to 64 chunks per
 * kernel launch (exon_hip_qual_pos_hist_chunks); the other kinds launch once per chunk. */
int exon_hip_plan_launch_chunks(exon_hip_plan* plan, void* stream, const exon_hip_column* columns, int32_t n_columns,
                                int32_t n_chunks, const int64_t* n, int32_t flags, void* d_state);

/* ---- merge of partial states across GPUs (AggregateExec(Final) over RCCL / xGMI; one process per GPU) -------------------
 * The reference merges partitions in AggregateExec(Final) behind a RepartitionExec / CoalescePartitionsExec (DataFusion 44,
 * reached from exon-core/src/session_context/exon_context_ext.rs:297-311); file groups come from regroup_files_by_size
 * (exon-core/src/datasources/exon_file_scan_config.rs:79-110).  Here every rank holds one packed state; the merge is ONE
 * ncclAllGather of it plus a fold in rank order 0..world-1, so all ranks end with bit-identical float64 sums whatever
 * algorithm RCCL picks.  librccl.so is dlopen'ed at the first call. */
/* out[v] = sum over r < world of gathered[r][v]  (gathered = `world` packed states, rank-major; d_out may not alias it) */
int exon_hip_fold_states(exon_hip_ctx* ctx, void* stream, const void* d_gathered, int32_t world, int64_t n_i64,
                         int64_t n_f64, void* d_out);
/* all-gather d_state into d_gather (world x state bytes) on `stream`, fold into d_out (may be d_state).  d_gather == NULL:
 * in-place ncclAllReduce of an integer-only state (n_f64 == 0, d_out == d_state) -- for states too large to gather. */
int exon_hip_merge_states(exon_hip_ctx* ctx, void* stream, void* rccl_comm, void* d_state, int64_t n_i64, int64_t n_f64,
                          void* d_gather, void* d_out);
/* The fold by the PLAN's own layout: `world` packed states of this plan, rank-major, folded in rank order -- add for count and
 * sum words, unsigned max for the two extreme planes of a CMP_MINMAX_BY_GROUP plan.  Works for every plan kind; for the kinds
 * whose words all add it is bit-identical to exon_hip_fold_states.  exon_hip_stream_all_reduce applies the same fold; the in-place
 * ncclAllReduce form of exon_hip_merge_states is sum-only and is never taken for a plan with max planes.  `stream`: hipStream_t,
 * NULL = the ctx's own.  d_out may not alias d_gathered. */
int exon_hip_plan_fold_states(const exon_hip_plan* plan, void* stream, const void* d_gathered, int32_t world, void* d_out);
/* ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy for hosts without an RCCL binding: rank 0 makes the 128-byte id and
 * ships it to the other ranks by any means; every rank then calls comm_init (collective) on its own ctx / GPU. */
/* ---- communicators (ABI 5: the handle is OPAQUE -- made by one of the two calls below, never a bare ncclComm_t) --------------------
 * exon_hip_rccl_comm_init: ncclGetUniqueId / ncclCommInitRank for hosts without an RCCL binding of their own (rank 0 creates the id,
 * ships its 128 bytes to the other ranks by any means; one process per GPU).  exon_hip_comm_from_callbacks: the same collectives over
 * an all-gather of HOST buffers the caller supplies (torch.distributed / gloo, MPI ...): `all_gather(user, send, recv, bytes)` copies
 * `bytes` from every rank's `send` into recv[rank * bytes ...] on every rank and returns 0 -- for hosts that already own a transport,
 * and for machines where RCCL cannot form the communicator (several ranks on one GPU: tests/test_collective_faults.py).
 * Every collective entry point of a stream VOTES before it exchanges data: a rank that cannot go on (stream finished, undeclared keys,
 * out of memory) says so in a 16-byte all-gather and EVERY rank returns that error -- none is left waiting in a collective for a peer
 * that has returned.  A peer that never enters at all is met by a bounded wait (EXON_HIP_COLLECTIVE_TIMEOUT_S, default 120):
 * the RCCL communicator is aborted (ncclCommAbort), the call fails with EXON_HIP_EDEVICE, the handle is unusable afterwards.
 * EXON_HIP_FAULT="site@rank[,...]" makes a named site fail on one rank (reconcile_enter, reconcile_malloc, reconcile_rekey,
 * allreduce_enter, allreduce_malloc, stall): how the tests reach every one of those paths. */
typedef int (*exon_hip_allgather_fn)(void* user, const void* send, void* recv, size_t bytes_per_rank);
int exon_hip_comm_from_callbacks(int32_t world, int32_t rank, exon_hip_allgather_fn all_gather, void* user, void** comm);
/* a host that made its ncclComm_t itself wraps it (not owned: exon_hip_rccl_comm_destroy frees the handle, not the ncclComm_t) */
int exon_hip_comm_wrap_rccl(void* nccl_comm, void** comm);
int exon_hip_rccl_unique_id(uint8_t* id128);
int exon_hip_rccl_comm_init(exon_hip_ctx* ctx, const uint8_t* id128, int32_t world, int32_t rank, void** rccl_comm);
int exon_hip_rccl_comm_destroy(void* rccl_comm);
/* ranks of a communicator and this one's index (ncclCommCount / ncclCommUserRank for the RCCL kind; rank may be NULL): what a
 * launcher prints to prove how many GPUs merged */
int exon_hip_rccl_comm_count(void* rccl_comm, int32_t* world, int32_t* rank);

/* One stream per partition (= per file group); single-threaded handle, owns one HIP stream, a
 * device-resident partial state and pinned staging buffers. */
int exon_hip_stream_open(exon_hip_plan* plan, int32_t partition, exon_hip_stream** out);
/* Host Arrow struct batch (children = columns).  The batch is MOVED (Arrow C Data Interface: on return `batch->release` is
 * NULL and the stream owns the array), WHATEVER the call returns: a batch that is refused (a finished stream, a column that is
 * missing, nested, short of buffers or shorter than the batch, a failed flush) is released before the call returns with its
 * error.  Only a NULL argument or a batch that is already released (release == NULL) leaves the struct untouched.  The
 * library calls the array's release callback exactly once, after its buffers have
 * been copied -- for a batch of up to 131072 rows of fixed-width columns that may be AFTER this call returns: such batches are
 * held and copied together, by a pool of threads, when their staging slot is flushed (the next push that fills it, sync,
 * state, finish, reset or close).  Everything the array points to must therefore stay valid until the callback runs, as the
 * interface requires of any exported array (an array whose children or buffer tables live on the caller's stack is not one).
 * EXON_HIP_HOLD_SMALL_BATCHES=0: copy and release inside the call.  Dictionary-encoded int32 indices are accepted for id
 * columns (the dictionary itself stays with the caller). */
int exon_hip_stream_push(exon_hip_stream* s, struct ArrowArray* batch);
/* HBM-resident batch (device_type must be ARROW_DEVICE_ROCM on this ctx's device).  Not moved:
 * buffers must stay alive until the next exon_hip_stream_sync/finish. */
int exon_hip_stream_push_device(exon_hip_stream* s, const struct ArrowDeviceArray* batch);
/* Device pointers of the partial state ([n_i64] int64 then [n_f64] float64, one allocation) so the
 * host can all-reduce them over RCCL, plus the hipStream_t the kernels run on. */
int exon_hip_stream_state(exon_hip_stream* s, int64_t** d_i64, double** d_f64, void** hip_stream);
/* The merge across GPUs in native code on the stream's hipStream_t: afterwards the state of every rank is the sum over all
 * ranks.  One all-gather + fixed-order fold (exon_hip_merge_states); `rccl_comm` is a communicator of this library (one rank
 * per GPU: exon_hip_rccl_comm_init).
 * (ABI 5) Collective, and it FAILS TOGETHER: what stops one rank -- the stream finished, a state keyed by its own dictionary
 * (EXON_HIP_ESTATE: call exon_hip_stream_reconcile_keys first wherever keys come from files), staged rows that cannot be
 * launched, no memory for the gather buffer -- goes into a 16-byte vote in front of the merge, and every rank returns that
 * error without entering the data exchange.  (Until ABI 4 these checks were rank-local and the peers of a failing rank waited
 * in ncclAllGather for ever.)  The vote synchronises the stream; the merge behind it is enqueued.  exon_hip_merge_states is
 * the bare form for callers that own the buffers and the step budget (bench.py's timed region). */
int exon_hip_stream_all_reduce(exon_hip_stream* s, void* rccl_comm);
/* ---- group keys by VALUE (ABI 4) --------------------------------------------------------------------------------------------
 * K3 / K4 states are indexed by dictionary id, and ids are per FILE: FILTER lists are numbered in order of first appearance in
 * a scan, reference ids follow each BAM's own @SQ order.  The reference merges partitions by key VALUE (AggregateExec(Final)
 * over the file groups of exon-core/src/datasources/exon_file_scan_config.rs:79-110).  So a stream fed by
 * exon_hip_stream_consume_scan remembers the value behind every state index: the first scan's dictionary becomes the stream's,
 * every further scan is aggregated under its own ids and added in under the stream's (new values are appended; more distinct
 * values than the plan's n_groups is EXON_HIP_ECAPACITY and leaves the stream as it was).  Across ranks, exon_hip_stream_all_reduce REFUSES (EXON_HIP_ESTATE) a
 * state keyed by a rank-local dictionary until the ranks have agreed on one -- exon_hip_stream_reconcile_keys, or
 * exon_hip_stream_keys on every rank + exon_hip_keys_union + exon_hip_stream_set_keys when the host moves the names itself.
 * Names are packed as '\0'-terminated strings back to back ("" is a legal key: the empty FILTER list); K3's NULL-reference
 * group is not a key (it stays the last word of the state).  Streams that are only ever pushed to (caller-owned dictionary
 * ids) are not tracked; exon_hip_stream_set_keys lets such a caller declare what its ids mean. */
/* the stream's dictionary in state-index order: *n_keys names, *bytes in all (buf may be NULL to size it);
 * *agreed (optional) = 1 once set_keys / reconcile_keys has run and no scan was consumed since */
int exon_hip_stream_keys(exon_hip_stream* s, char* buf, size_t cap, int32_t* n_keys, size_t* bytes, int32_t* agreed);
/* adopt `names` (n_keys packed strings, no duplicates, at most the plan's n_groups): every key the stream holds must be among
 * them; the state is permuted into the new order on the device.  On a stream without keys: a declaration / a seed. */
int exon_hip_stream_set_keys(exon_hip_stream* s, const char* packed_names, size_t packed_bytes, int32_t n_keys);
/* host-only: union of `world` dictionaries (packed back to back, n_keys[r] names each) in rank order, first appearance first --
 * deterministic, so every rank computes the same.  out (may be NULL to size it) receives the packed union, maps (optional,
 * sum of n_keys entries, rank-major) the union id of every input key. */
int exon_hip_keys_union(const char* packed, size_t packed_bytes, const int32_t* n_keys, int32_t world, char* out, size_t cap,
                        int32_t* n_out, size_t* out_bytes, int32_t* maps);
/* collective over `rccl_comm` (every rank calls it, between its last consume_scan and exon_hip_stream_all_reduce): small
 * all-gathers move the dictionaries, every rank forms the same union and permutes its state into it.  A rank that cannot take
 * part (its stream finished; rows pushed under undeclared ids) says so INSIDE the first exchange, one that runs out of memory for
 * the exchange or the re-keying buffers says so in a vote in front of the second: every rank then returns that error (EXON_HIP_ESTATE
 * / EXON_HIP_ENOMEM), none hangs, no state has been touched.  A union larger than the plan's n_groups is EXON_HIP_ECAPACITY on
 * every rank (all ranks compute the same union). */
int exon_hip_stream_reconcile_keys(exon_hip_stream* s, void* rccl_comm);
/* Region plans (K2 / K6 / K7) fed by files: name the contig instead of fixing exon_hip_plan_desc.region_chrom_id -- every
 * exon_hip_stream_consume_scan then resolves the name in that file's own contig / reference dictionary (a BAM without such
 * a reference contributes no rows). */
int exon_hip_stream_set_region_contig(exon_hip_stream* s, const char* name);
/* Start a new query on this stream: the next launch DEFINES the state (overwrite mode, no zeroing kernel); rows staged but
 * not yet launched are dropped; a finished stream can be pushed to again. */
int exon_hip_stream_reset(exon_hip_stream* s);
int exon_hip_stream_sync(exon_hip_stream* s);
/* Copies the (possibly all-reduced) state to host: counts[n_i64], sums[n_f64]. */
int exon_hip_stream_finish(exon_hip_stream* s, int64_t* counts, double* sums);
/* Same result as one Arrow struct array in DataFusion's partial-aggregate state layout
 * (see DESIGN.md "State schema"); caller releases out/out_schema. */
int exon_hip_stream_finish_arrow(exon_hip_stream* s, struct ArrowArray* out, struct ArrowSchema* out_schema);
int exon_hip_stream_close(exon_hip_stream* s);

/* ---- scan: native decoders + device-layout array builders (host memory) --------------------------------
 * FileOpener::open + BatchReader::read_batch of the reference
 * (exon-core/src/datasources/vcf/file_opener/unindex_file_opener.rs:48-92, exon-vcf/src/async_batch_stream.rs:80-109,
 *  exon-bam/src/batch_reader.rs:44-108, exon-fastq/src/batch_reader.rs:63-82, exon-fasta/src/batch_reader.rs:72-99).
 * Batches are Arrow struct arrays in the DEVICE LAYOUT (dictionary<int32,utf8> keys, u8 mapq) ready for
 * exon_hip_stream_push.  Column order:
 *   VCF   0 chrom(dict) 1 pos:i64? 2 qual:f32? 3 filter(dict of ';'-joined lists, "" = []) [4.. info.<F>: f32? | bool? | dict?]
 *   BAM   0 flag:i32 1 mapping_quality:u8? 2 reference(dict)? 3 start:i64? 4 end:i64?
 *   FASTQ 0 name 1 description? 2 sequence 3 quality_scores      FASTA 0 id 1 description? 2 sequence
 *   GFF   0 seqname(dict) 1 source(dict) 2 type(dict) 3 start:i64 4 end:i64 5 score:f32? 6 strand(dict ["+","-"])? 7 phase(dict
 *         ["0","1","2"])?  -- the reference's schema order (exon-gff/src/array_builder.rs); the three leading dictionaries are
 *         built from the file (GFF has no header).  With EXON_HIP_PROJECT_GFF_ATTRIBUTES column 8 is `attributes`, the
 *         reference's Map<Utf8, List<Utf8>> (Arrow "+m", not NULL, keys unsorted; entries{keys: Utf8, values: List<item:
 *         Utf8>?}; exon-gff/src/config.rs:81-108), by the ATTRIBUTE RULES of exon_amd/csrc/host/gff.h: split at ';' then the
 *         first '=' then ',', percent-decoded, validated on every record.  Built by the host reader and by the GPU pipeline
 *         (text_columns.hip); any other GFF projection bit is EXON_HIP_EUNSUPPORTED.  A region
 *         is the reference reader's own filter (exon-gff/src/batch_reader.rs:76-97): seqname = name AND start inside the
 *         interval; with use_index the chunks come from <path>.tbi (GFF preset, read from the index header).  A ##FASTA
 *         section is EXON_HIP_EUNSUPPORTED.  Plans address the columns by index: K2 (0, 3); K6 / K7 (0, 3, 4).
 *   GTF   0 seqname(dict) 1 source(dict) 2 type(dict) 3 start:i64 4 end:i64 5 score:f32? 6 strand(dict ["+","-"])? 7 frame(dict
 *         ["0","1","2"])?  -- the reference's schema order (exon-gtf/src/config.rs); dictionaries as for GFF.  With
 *         EXON_HIP_PROJECT_GTF_ATTRIBUTES column 8 is `attributes`, the reference's Map<Utf8, Utf8> (Arrow "+m", not NULL, keys
 *         unsorted; entries{keys: Utf8, values: Utf8?}, no value is ever NULL; exon-gtf/src/config.rs:28-41), by the ATTRIBUTE
 *         RULES of exon_amd/csrc/host/gtf.h: `key "value"; key value;`, a ';' inside quotes belongs to the value, quotes
 *         dropped, nothing decoded, validated on every record.  Built by the host reader and by the GPU pipeline; any other
 *         GTF projection bit is EXON_HIP_EUNSUPPORTED.  A region is the GFF reader's filter (seqname = name AND start inside
 *         the interval); use_index is EXON_HIP_EUNSUPPORTED (the reference has no indexed GTF table).  A '?' strand is an
 *         error (GFF3 reads it as NULL).  Plans address the columns as for GFF.
 *   BED   0 reference_sequence_name(dict, built from the file, never NULL) 1 start:i64 2 end:i64 -- the interval kernels'
 *         operands and nothing else: K2 (0, 1); K6 / K7 (0, 1, 2); a region's contig travels by name
 *         (exon_hip_stream_set_region_contig) and is resolved in each file's dictionary, as for GFF.  The other columns of the
 *         reference's schema (exon-bed/src/schema.rs:27-48) are EXON_HIP_PROJECT_BED_* bits, each bit the column's index there,
 *         appended in bit order: 3 name Utf8?, 4 score i64?, 5 strand(dict ["+","-"])?, 6 thick_start i64?, 7 thick_end i64?,
 *         8 color Utf8?, 9 block_count i64?, 10 block_sizes Utf8?, 11 block_starts Utf8? -- 6..11 are NULL on every row, as in
 *         the reference, whose n_fields = k (table_options.rs:34-45) is the mask of bits 3 .. k - 1.  Any other bit is
 *         EXON_HIP_EUNSUPPORTED.  A line is decoded by its own field count (3, 4, 5, 6 or 12; anything else is an error) and
 *         validated in full whatever is projected; start and end are 0-based as they stand.  Rules and DECISIONs:
 *         exon_amd/csrc/host/bed.h.  `region` and `use_index` are EXON_HIP_EUNSUPPORTED (the reference has neither for BED);
 *         info_field must be NULL.
 * CPU-only: no ctx needed; errors are reported through exon_hip_last_error(NULL). */
#define EXON_HIP_FORMAT_VCF 1
#define EXON_HIP_FORMAT_BAM 2
#define EXON_HIP_FORMAT_FASTQ 3
#define EXON_HIP_FORMAT_FASTA 4
#define EXON_HIP_FORMAT_SAM 5 /* text SAM: same columns as BAM */
#define EXON_HIP_FORMAT_BCF 6 /* BCF2: same columns as VCF */
#define EXON_HIP_FORMAT_CRAM 7 /* CRAM 3.0 (raw / gzip / bzip2 / lzma / rANS 4x8 blocks), host decoder: same columns as BAM */
#define EXON_HIP_FORMAT_GFF 8 /* GFF3 text (additive; the ABI stays 5): columns above; GTF and BED are formats of their own */
#define EXON_HIP_FORMAT_GTF 9 /* GTF text (additive; the ABI stays 5): columns above */
#define EXON_HIP_FORMAT_BED 10 /* BED text (additive; the ABI stays 5): columns above */
#define EXON_HIP_COMPRESSION_AUTO 0 /* sniff the gzip/BGZF magic */
#define EXON_HIP_COMPRESSION_NONE 1
#define EXON_HIP_COMPRESSION_GZIP 2
/* zstd / bzip2 / xz inputs (file_compression_type.convert_stream of the reference's openers) are recognised by their magic
 * numbers and refused by exon_hip_scan_open with EXON_HIP_EUNSUPPORTED and a text naming the codec. */

typedef struct exon_hip_scan exon_hip_scan;
typedef struct exon_hip_scan_options {
  int32_t format;       /* EXON_HIP_FORMAT_* */
  int32_t compression;  /* EXON_HIP_COMPRESSION_* */
  int64_t batch_size;   /* 0 = 8192 (exon-common/src/lib.rs:27) */
  const char* info_field; /* VCF / BCF: typed INFO fields to extract (exon.vcf_parse_info), up to 16 comma-separated header
                             IDs ("AF,DP,DB"), NULL = none.  They become scan columns 4, 5, ..., typed from the header as the
                             reference does (schema_builder.rs:197-249): Number=1 Float -> f32?, Number=1 Integer -> i32?,
                             Flag -> bool? (true when present, NULL when absent), Number=1 String / Character -> dictionary? (VCF text: built on the device too),
                             any other Number -> List<f32 | i32 | dictionary>? (items '.' are NULL items; host decoders);
                             INFO '.' makes all of them NULL (the struct itself is NULL in the reference) */
  const char* region;     /* pushed-down vcf_region_filter / bam_region_filter ("chr1:1-100"), NULL = none */
  int32_t use_index;      /* with `region`: plan BGZF chunks from <path>.tbi / <path>.bai (INDEXED_VCF / INDEXED_BAM / INDEXED_GFF) */
  int32_t gpu_parse;      /* VCF, BCF, FASTQ, BAM, SAM, GFF, GTF, BED: exon_hip_stream_consume_scan ships the file's bytes to HBM and decodes
                             them on the GPU (exon_hip_bgzf_inflate, exon_hip_vcf_parser_* / exon_hip_fastq_parser_* /
                             exon_hip_bam_parser_* ...).  exon_hip_scan_next on such a scan needs exon_hip_scan_bind_ctx first
                             (batches then come out of the same GPU pipeline); without a bound ctx it returns ESTATE.
                             FASTA: the request is remembered for exon_hip_scan_bind_ctx (batches from the GPU pipeline,
                             exon_hip_fasta_parser_*) and for exon_hip_stream_consume_scan under the one fused FASTA plan,
                             EXON_HIP_PLAN_SEQ_STATS_HIST (exon_hip_seq_stats_hist_views over every slab's views; an input that does
                             not start with '>', an undecided slab or a record beyond the carry limit is handed to the host reader).
                             A stream of any other plan kind reads such a scan through the host reader, and exon_hip_scan_next
                             without a bound ctx returns the host reader's batches (that reader defers nothing) */
  uint64_t projection;    /* (ABI 5) EXON_HIP_PROJECT_* bits: columns of the reference's schema beyond the fused kernels' operands,
                             appended BEHIND the default ones in bit order (0 = none: the hot path ships only what a plan reads).
                             VCF text: id List<Utf8>?, ref Utf8, alt List<Utf8>? (lazy_array_builder.rs:169-205; the alt list has no
                             items, as in the reference -- see text_columns.hip); BAM: name Utf8?, cigar Utf8, sequence Utf8,
                             quality_score List<Int64> (exon-bam/src/array_builder.rs:105-201).  Built by the host readers (one
                             thread) and by the GPU pipeline (exon_hip_scan_bind_ctx); EXON_HIP_EUNSUPPORTED for other formats.
                             VCF text also: info Utf8, formats Utf8 -- the unparsed forms of the reference's default schema, which
                             are the parsed entries PRINTED AGAIN, not the fields' bytes ("AF=0.50" -> "AF=0.5", a Flag ->
                             "DB=true", formats = keys TAB samples; lazy_array_builder.rs:216-297, :310-423; host/vcf_text.h).
                             info comes from the host reader and from the GPU pipeline (text_columns.hip: k_vcf_info_measure /
                             k_vcf_info_fill print the entries on the device; a row the device does not decide -- a missing
                             value, an integer outside i32, a float of more than 19 significant digits, a byte >= 0x80
                             -- hands the file to the host reader).  formats is built by the host reader: a gpu_parse scan that
                             asks for it decodes on the host, UNLESS it also sets the modifier EXON_HIP_PROJECT_VCF_FORMATS_ON_DEVICE
                             (32; no column of its own, valid only next to bit 16, EXON_HIP_EINVAL without it): then the column
                             comes from the GPU pipeline too (text_columns.hip: k_fmt_*, one thread a sample), and a row the
                             device does not decide -- a missing sample value, an allele that is no number, more than 16 FORMAT
                             keys, a byte >= 0x80, what `info` hands over for its numbers -- hands the file to the host reader.
                             BCF: id List<Utf8>, ref Utf8, alt List<Utf8> through the reference's EAGER builder (lists with their
                             items, never NULL: eager_array_builder.rs:112-134); SAM: the BAM columns from the line's fields
                             (exon-sam/src/array_builder.rs:101-185); both from the host readers and from the GPU pipeline.
                             GFF: attributes Map<Utf8, List<Utf8>> (exon-gff/src/array_builder.rs:141-165), bit 8 = the column's
                             index in the reference's schema; from the host reader and from the GPU pipeline.
                             GTF: attributes Map<Utf8, Utf8> (exon-gtf/src/array_builder.rs:82-87), the same bit.
                             BED: bits 3 .. 11 = columns 3 .. 11 of the reference's schema (name .. block_starts) */
} exon_hip_scan_options;
#define EXON_HIP_PROJECT_VCF_ID 1ull
#define EXON_HIP_PROJECT_VCF_REF 2ull
#define EXON_HIP_PROJECT_VCF_ALT 4ull
#define EXON_HIP_PROJECT_VCF_INFO 8ull     /* host reader and GPU pipeline (the entries are printed again on the device) */
#define EXON_HIP_PROJECT_VCF_FORMATS 16ull /* host reader; the GPU pipeline only with the modifier below (else a gpu_parse scan decodes on the host) */
#define EXON_HIP_PROJECT_VCF_FORMATS_ON_DEVICE 32ull /* (additive; the ABI stays 5) a modifier, not a column: with bit 16, `formats` is printed on the device */
#define EXON_HIP_PROJECT_BAM_NAME 1ull
#define EXON_HIP_PROJECT_BAM_CIGAR 2ull
#define EXON_HIP_PROJECT_BAM_SEQUENCE 4ull
#define EXON_HIP_PROJECT_BAM_QUALITY_SCORES 8ull
#define EXON_HIP_PROJECT_GFF_ATTRIBUTES 256ull /* (additive; the ABI stays 5) bit 8: `attributes` is column 8 of the reference's schema */
#define EXON_HIP_PROJECT_GTF_ATTRIBUTES 256ull /* (additive) GTF's `attributes` is column 8 of the reference's schema too */
/* (additive; the ABI stays 5) BED: bit k = column k of the reference's schema; n_fields = k is the mask of bits 3 .. k - 1 */
#define EXON_HIP_PROJECT_BED_NAME (1ull << 3)
#define EXON_HIP_PROJECT_BED_SCORE (1ull << 4)
#define EXON_HIP_PROJECT_BED_STRAND (1ull << 5)
#define EXON_HIP_PROJECT_BED_THICK_START (1ull << 6)
#define EXON_HIP_PROJECT_BED_THICK_END (1ull << 7)
#define EXON_HIP_PROJECT_BED_COLOR (1ull << 8)
#define EXON_HIP_PROJECT_BED_BLOCK_COUNT (1ull << 9)
#define EXON_HIP_PROJECT_BED_BLOCK_SIZES (1ull << 10)
#define EXON_HIP_PROJECT_BED_BLOCK_STARTS (1ull << 11)

int exon_hip_scan_open(const char* path, const exon_hip_scan_options* options, exon_hip_scan** out);
int exon_hip_scan_schema(exon_hip_scan* scan, struct ArrowSchema* out);
/* 0 = a batch was written to *out (caller releases or moves it); 1 = end of stream; <0 = error */
int exon_hip_scan_next(exon_hip_scan* scan, struct ArrowArray* out);
/* dictionary of a dict-encoded column (VCF 0/3, BAM 2, GFF and GTF 0/1/2/6/7, BED 0 and strand's column when projected): current size, and id of `name` (interned if new) */
int exon_hip_scan_dictionary_size(exon_hip_scan* scan, int32_t column, int32_t* size);
int exon_hip_scan_dictionary_intern(exon_hip_scan* scan, int32_t column, const char* name, int32_t* id);
int exon_hip_scan_dictionary_value(exon_hip_scan* scan, int32_t column, int32_t id, const char** name);
int exon_hip_scan_rows(exon_hip_scan* scan, int64_t* rows_emitted);
/* the reference lengths of a BAM, SAM or CRAM header in dictionary-id order (the order of exon_hip_scan_dictionary_value on the
 * reference column), with the host and with the GPU decoders alike: *n = their number, and the first min(*n, cap) go to out (out may
 * be NULL when cap is 0).  A SAM @SQ line without LN reports 0.  Any other format: EXON_HIP_EUNSUPPORTED. */
int exon_hip_scan_reference_lengths(exon_hip_scan* scan, int64_t* out, int32_t cap, int32_t* n);
/* (round 5, additive) Batches of a scan opened with gpu_parse = 1 come out of the GPU decode pipeline on `ctx`: after this
 * call exon_hip_scan_next drives the same slab pipeline exon_hip_stream_consume_scan drives (file bytes to HBM, BGZF inflate,
 * record parse, pushed-down region mask on the device), copies every slab's columns back and returns them as batch_size-row
 * batches in the host readers' layout and file order -- for queries that do NOT end in one of the fused kernels (the surface
 * of <Fmt>Scan::execute, exon/exon-core/src/datasources/vcf/scanner.rs:142-162, bam/scanner.rs:138-158).  A producer thread
 * fills a bounded queue; if the device cannot decide a record the host reader takes over behind the last row emitted.
 * VCF / BCF (chrom, pos, qual, filter, Float / Integer / Flag INFO keys), BAM, SAM, and (round 6) FASTQ -- name, description,
 * sequence, quality_scores as Utf8 columns built on the device (exon-fastq/src/array_builder.rs:68-102), plain, gzip or BGZF;
 * GFF, GTF, BED; FASTA -- id, description, sequence as Utf8 columns built on the device (the rules next to
 * exon_hip_fasta_parser_create), plain, gzip or BGZF: EXON_HIP_EUNSUPPORTED when the input is empty or its first decompressed byte
 * is not '>' (text in front of the first definition line is the host reader's to skip), and a record larger than the carried tail
 * of a slab may be (a quarter of a slab, 20 MB at the default size) hands the file to the host reader: whole chromosomes stay a
 * host format.  EXON_HIP_EUNSUPPORTED for CRAM and for scans whose batches the host reader must build (opened without gpu_parse,
 * list-valued INFO keys, the formats text column).  Call before the first
 * exon_hip_scan_next; `ctx` must outlive the scan.  A scan with a pushed-down value predicate (exon_hip_scan_set_predicate) masks
 * every slab on the device, takes the surviving rows of every column there and copies only those back. */
int exon_hip_scan_bind_ctx(exon_hip_scan* scan, exon_hip_ctx* ctx);
/* (additive; the ABI stays 5)
 * One pushed-down comparison, evaluated by the scan itself: a row is emitted iff column `column` is valid AND value <cmp_op> literal
 * (EXON_HIP_GT .. EXON_HIP_NE), by K4's rule (Float32 widened to Float64 and compared in totalOrder; Int32 compared exactly).
 * ANDed with `region` when the scan has one.  Call after exon_hip_scan_open and before exon_hip_scan_bind_ctx / the first
 * exon_hip_scan_next / exon_hip_stream_consume_scan (later: EXON_HIP_ESTATE); a second call replaces the first.
 * `column` is a scan column as the plans use them; VCF: 2 = qual, 4 + k = typed INFO field k of `info_field`.  Float32 columns and
 * Int32 columns that are not dictionary ids (Number=1 Float / Integer keys) are accepted; pos (Int64), dictionary, Flag and list
 * columns are EXON_HIP_EUNSUPPORTED, a column outside the schema or a cmp_op outside 0 .. 5 EXON_HIP_EINVAL, any format but
 * EXON_HIP_FORMAT_VCF (plain, gzip or BGZF; with or without region / use_index) EXON_HIP_EUNSUPPORTED, and so is a region scan under
 * EXON_HIP_REFERENCE_QUIRKS=1 (that opener's unfiltered tail has no meaning for a second conjunct).
 * This is the reader's own filter, like `region`: dropped rows are not built and exon_hip_scan_rows counts the rows emitted.  A
 * fused plan over such a scan (exon_hip_stream_consume_scan) sees the kept rows only: K2 / K6 / K7 count them, K4 / K8 get a
 * second conjunct.  As with a region, a FILTER dictionary built on the device may hold values that only dropped rows carried:
 * they show up as groups with zero counts. */
int exon_hip_scan_set_predicate(exon_hip_scan* scan, int32_t column, int32_t cmp_op, double literal);
/* (additive; the ABI stays 5)
 * The flag / mapping-quality predicate of alignment scans, evaluated by the scan itself: a row is emitted iff
 *   (flag & flag_mask) == flag_value  AND  (mapq_min < 0  OR  (mapping_quality valid AND mapping_quality >= mapq_min))
 * -- the row predicate of EXON_HIP_PLAN_FLAG_MAPQ_GROUP_COUNT (K3), i.e. the flag tests of udfs/sam/samflags.rs:26-47 and
 * CAST(mapping_quality AS INT) >= q under FilterExec, where a NULL mapping_quality (255 in BAM and SAM) never passes.  The three
 * operands are plain int32 as K3 takes them: a flag_value with bits outside flag_mask, or a mapq_min above 255, keeps no row and is
 * no error.  DECISION: mapq_min < 0 means "no conjunct on mapping_quality" (`WHERE flag & 4 = 0` has none); K3's own plan field
 * keeps its meaning.
 * EXON_HIP_FORMAT_BAM and EXON_HIP_FORMAT_SAM (plain, gzip or BGZF) only, ANDed with `region`, with or without use_index; any other
 * format, CRAM included, is EXON_HIP_EUNSUPPORTED (BAM has no EXON_HIP_REFERENCE_QUIRKS region path to refuse).  Call order as
 * exon_hip_scan_set_predicate: after exon_hip_scan_open and before exon_hip_scan_bind_ctx / the first exon_hip_scan_next /
 * exon_hip_stream_consume_scan (later: EXON_HIP_ESTATE); a second call replaces the first.  exon_hip_scan_set_predicate on a BAM or
 * SAM scan stays EXON_HIP_EUNSUPPORTED.
 * Like `region` this is the reader's own filter: dropped rows are not built, exon_hip_scan_rows counts the rows emitted, and a SAM
 * FLAG / MAPQ field that is no number lets the record through to the builder.  Bound to a context, every slab is masked on the
 * device, the kept rows of every column -- name, cigar, sequence and the List<Int64> quality_score included -- are taken there and
 * only they are copied back (exon_hip_scan_export_stats).  A fused plan over such a scan sees the kept rows only: K3 gets a second
 * conjunct, K6 / K7 count kept rows. */
int exon_hip_scan_set_flag_predicate(exon_hip_scan* scan, int32_t flag_mask, int32_t flag_value, int32_t mapq_min);
/* (additive; the ABI stays 5)
 * BLOCKS MODE: the scan hands a plan every kept record as its ALIGNED BLOCKS instead of its span (exon_hip_cigar_blocks above states
 * the rule, cover_ops and the rows a record emits).  cover_ops = 0 turns it off; any bit outside 0x18D is EXON_HIP_EINVAL.
 * EXON_HIP_FORMAT_BAM and EXON_HIP_FORMAT_SAM only (plain, gzip, BGZF; with or without `region`, use_index or a flag predicate); any
 * other format is EXON_HIP_EUNSUPPORTED with the reason (CRAM: the decoder reconstructs the span only; GFF, GTF, BED and the rest
 * have no CIGAR), and so is a scan opened with a projection.  Call order and EXON_HIP_ESTATE as exon_hip_scan_set_flag_predicate; a
 * second call replaces the first.
 * The region and the flag predicate keep selecting RECORDS, by span as without the mode; every block of a kept record is emitted.
 * A blocks-mode scan serves FUSED PLANS OF KINDS 12, 13 AND 14 ONLY: exon_hip_stream_consume_scan under any other kind is
 * EXON_HIP_EUNSUPPORTED before anything is read (kind 11, K3 and K6 count records: a record would count once per block), and so are
 * exon_hip_scan_next and exon_hip_scan_bind_ctx (batches keep the reference's schema of one row per record).
 * THE PLANS' FOUR TOTALS COUNT BLOCK ROWS; `rows` of exon_hip_stream_consume_scan and exon_hip_scan_rows keep counting RECORDS, on
 * both decode paths.  The host readers emit the same block rows as the device stage (cigar_blocks.hip: a count pass, the offsets
 * scan, a fill pass per slab, the slab's total in one small copy), so gpu_parse = 0, EXON_HIP_GPU_PARSE=0 and every hand-over give
 * the same state word for word.  DECISIONS: a BAM record whose CIGAR is the two-op placeholder of a CG tag (<l_seq>S<n>N) is an
 * error that names the tag -- the device leaves it undecided, the host reader reports it -- never zero coverage; a SAM op longer
 * than 2^28 - 1, an op without a count and a letter outside MIDNSHP=X are `invalid CIGAR '...'` the same way. */
int exon_hip_scan_set_cover_ops(exon_hip_scan* scan, uint32_t cover_ops);
/* after the scan has ended: slabs exported by the GPU pipeline, how many of them went through the device take-rows step,
 * bytes copied device -> host for batches (mask / count words included). Any pointer may be NULL. */
int exon_hip_scan_export_stats(exon_hip_scan* scan, int64_t* slabs, int64_t* compacted_slabs, int64_t* d2h_bytes);
/* number of index chunks an indexed scan planned (-1 when the scan is not index-driven) */
int exon_hip_scan_index_chunks(exon_hip_scan* scan, int32_t* n_chunks);
/* Region -> BGZF chunks from a tabix (.tbi, is_bai = 0; `ref_name` resolved through the index' names) or BAI
 * (.bai, is_bai = 1; `ref_id` = BAM header order) index: get_byte_range_for_file
 * (exon-core/src/datasources/indexed_file/indexed_bgzf_file.rs:52-112).  Virtual positions are written to
 * starts/ends (up to `cap`); *n_chunks receives the full count. */
int exon_hip_index_query(const char* index_path, int32_t is_bai, const char* ref_name, int32_t ref_id, int64_t start,
                         int64_t end, uint64_t* starts, uint64_t* ends, int32_t cap, int32_t* n_chunks);
/* After exon_hip_stream_consume_scan: *decoded = 1 when every record was decoded on the GPU (0: the host decoder ran,
 * because gpu_parse was off or the device handed the file back); *inflated (optional) = 1 when the BGZF blocks were
 * inflated on the GPU as well. */
int exon_hip_scan_decoded_on_gpu(exon_hip_scan* scan, int32_t* decoded, int32_t* inflated);
int exon_hip_scan_close(exon_hip_scan* scan);
/* ---- (ABI 5) plain gzip on the GPU: RFC 1952 members that are NOT BGZF (no "BC" extra field, one DEFLATE stream per member) -------
 * The `else` arm of the reference's openers (exon-core/src/datasources/fastq/file_opener.rs:79-92: a gzip file that fails
 * is_bgzip_valid_header goes through file_compression_type.convert_stream).  The compressed bytes of a slab are cut into chunks, one
 * wavefront per chunk finds a block start by itself and decodes with the 32 KiB in front of it unknown (16-bit symbols: a byte, or
 * "byte k of the window"); the host proves the chain of chunks, the windows are resolved by composing the chunks' tail maps, a last
 * pass writes bytes; CRC-32 and ISIZE of every member are checked (exon_amd/csrc/gzip_stream.hip).
 * A stream is one file: create, decode slab after slab, destroy.  Any failure (EXON_HIP_EINVAL with a text) means: inflate this
 * file on the host -- nothing of the failing call has been committed to the stream's state except that it cannot be continued. */
typedef struct exon_hip_gzip_stream exon_hip_gzip_stream;
typedef struct exon_hip_gzip_stats {
  uint64_t calls, chunks, repairs, overflow_retries, members, comp_bytes, out_bytes;
} exon_hip_gzip_stats;
/* max_comp_bytes: the most compressed bytes one decode call is given; scratch_bytes: symbol scratch (2 bytes per output byte of a
 * call; 0 = 16 x max_comp_bytes, at least 64 MiB -- a call whose chunks overflow their share is repeated on a quarter of the slab) */
int exon_hip_gzip_stream_create(exon_hip_ctx* ctx, int64_t max_comp_bytes, int64_t scratch_bytes, exon_hip_gzip_stream** out);
/* d_comp: device memory (any alignment; the up to 3 bytes in front of it down to the 4-byte boundary must be readable), n_comp bytes
 * that start at the byte the previous call stopped in (the file's first byte for the first call) with 4096 readable bytes behind them; final_input: these are the file's last bytes.  Decodes whole DEFLATE blocks
 * while their output fits out_cap; *consumed = compressed bytes used up (pass the rest again in front of the next bytes; the bit
 * position inside the first byte is the stream's business), *produced = bytes written to d_out, *stream_end = 1 once the last
 * member's trailer has been checked at the end of the input.  Synchronises `stream`. */
int exon_hip_gzip_stream_decode(exon_hip_gzip_stream* s, void* stream, const uint8_t* d_comp, int64_t n_comp, int32_t final_input,
                                uint8_t* d_out, int64_t out_cap, int64_t* consumed, int64_t* produced, int32_t* stream_end);
int exon_hip_gzip_stream_get_stats(exon_hip_gzip_stream* s, exon_hip_gzip_stats* out);
int exon_hip_gzip_stream_destroy(exon_hip_gzip_stream* s);
/* ---- VCF record parsing on the GPU (raw text in HBM -> device-layout columns in HBM) ---------------------------
 * Same field rules as LazyVCFArrayBuilder::append (exon-vcf/src/array_builder/lazy_array_builder.rs:159-216) for the
 * device-layout columns.  A parser is bound to one header (contig dictionary) and one optional typed INFO field and
 * keeps the FILTER dictionary it discovers across slabs.  Rows the device cannot decide (float with > 19 significant
 * digits, contig missing from the header, malformed line) are counted in n_undecided: re-decode that slab on the host. */
#define EXON_HIP_MAX_INFO_FIELDS 16 /* typed INFO fields per scan / parser */
typedef struct exon_hip_vcf_parser exon_hip_vcf_parser;
typedef struct exon_hip_vcf_columns {
  int64_t n_rows;
  int64_t n_undecided;
  int32_t* chrom_id;   /* device pointers owned by the parser, overwritten by the next parse call */
  int64_t* pos;
  uint8_t* pos_valid;
  float* qual;
  uint8_t* qual_valid;
  int32_t* filter_id;
  float* info;         /* NULL without an INFO field; = infos[0] */
  uint8_t* info_valid;
  int64_t consumed_bytes; /* bytes up to and including the last newline; a trailing partial line is not parsed */
  /* all typed INFO fields of the parser, in the order given to *_parser_create (scan columns 4 ..), 4-byte values + validity:
   * info_kinds[k] = 'f' Float -> float values; 'i' Integer -> int32_t values (exact; schema_builder.rs:197-205); 'b' Flag ->
   * infos[k] == NULL, the column is the presence bitmap infos_valid[k] (true where set) */
  int32_t n_info;
  int32_t reserved;
  void* infos[EXON_HIP_MAX_INFO_FIELDS];
  uint8_t* infos_valid[EXON_HIP_MAX_INFO_FIELDS];
  char info_kinds[EXON_HIP_MAX_INFO_FIELDS];
  /* list-valued fields, info_kinds[k] = 'F' (List<f32>) / 'I' (List<i32>) -- any Number other than 0 / 1
   * (schema_builder.rs:235-249): Arrow List layout.  infos_valid[k] = validity of the LIST per row (NULL list: key absent,
   * `key=.`, INFO '.'), list_offsets[k] = int32 offsets [n_rows + 1] into the items, infos[k] = the items,
   * list_item_valid[k] = validity of the items (a '.' item is a NULL item: info_builder.rs:258-305).  NULL for scalar kinds. */
  int32_t* list_offsets[EXON_HIP_MAX_INFO_FIELDS];
  uint8_t* list_item_valid[EXON_HIP_MAX_INFO_FIELDS];
  /* (ABI 5) info_kinds[k] = 's' (Number=1 String / Character, VCF text only): infos[k] = int32 dictionary ids, infos_valid[k] =
   * validity; the dictionary is built on the device like the FILTER one: exon_hip_vcf_parser_info_values.  info_nulls[k] = rows
   * of this slab without a value (-1 for other kinds): a GROUP BY over the key has a NULL group unless this is 0. */
  int32_t info_nulls[EXON_HIP_MAX_INFO_FIELDS];
} exon_hip_vcf_columns;
/* info_field: NULL, or up to EXON_HIP_MAX_INFO_FIELDS comma-separated INFO keys "name[:kind]" -- kind f (default): Number=1
 * Float -> f32; kind i: Number=1 Integer -> i32; kind b: Flag -> presence bitmap; kinds F / I: list-valued Float / Integer
 * fields -> List<f32> / List<i32>.  (String INFO fields, scalar or list, are decoded by the host reader only.) */
int exon_hip_vcf_parser_create(exon_hip_ctx* ctx, const char* const* contig_names, int32_t n_contigs,
                               const char* info_field, int64_t max_slab_bytes, exon_hip_vcf_parser** out);
/* d_text: a slab of '\n'-terminated data lines in HBM, any alignment (a trailing partial line is left to the
 * caller: see consumed_bytes).  Synchronises `stream`. */
int exon_hip_vcf_parser_parse(exon_hip_vcf_parser* parser, void* stream, const uint8_t* d_text, int64_t n_bytes,
                              exon_hip_vcf_columns* cols);
/* FILTER dictionary discovered so far, '\0'-separated in id order ("" = the empty list) */
int exon_hip_vcf_parser_filters(exon_hip_vcf_parser* parser, char* buf, size_t cap, int32_t* n_filters);
/* values of the String / Character INFO key `key` (index in the parser's key list) seen so far, '\0'-separated, in id order */
int exon_hip_vcf_parser_info_values(exon_hip_vcf_parser* parser, int32_t key, char* buf, size_t cap, int32_t* n_values);
/* on != 0: rows WITHOUT a value of a String / Character key take the dictionary id of the EMPTY text (a value no row can carry:
 * "key=" is a missing value) and info_nulls stays 0 -- NULL becomes a group key of its own, which is what DataFusion's GROUP BY
 * does with a nullable key.  exon_hip_stream_consume_scan switches it on (a fused plan cannot skip rows by a key's bitmap);
 * batches (exon_hip_scan_next) keep NULL as NULL.  In a keyed stream's dictionary the NULL group is the key "". */
int exon_hip_vcf_parser_set_null_key(exon_hip_vcf_parser* parser, int32_t on);
/* (additive; the ABI stays 5) The `info` Utf8 column of the reference's default schema, built on the device: every record's INFO
 * entries printed again (see exon_hip_scan_options.projection).  set_key_types gives the parser the value types of the header's
 * ##INFO lines: packed_keys = n key names, each with its NUL, back to back; kinds[k] = i (Integer), f (Float), b (Flag),
 * c (Character) or s (String).  The first line of a key wins; the reserved keys of the specification keep their types unless the
 * header names them; any other key is a String.  n = 0: the reserved keys alone.
 * info_text, after a parse call without undecided rows and before the next one: offsets [n_rows + 1] and values [n_bytes] in
 * HBM, owned by the parser and valid until its next call.  n_undecided != 0: rows the host reader must print or refuse (no
 * buffers then).  Synchronises `stream`. */
typedef struct exon_hip_vcf_info_text {
  int64_t n_bytes;
  int64_t n_undecided;
  const int32_t* offsets;
  const uint8_t* values;
} exon_hip_vcf_info_text;
int exon_hip_vcf_parser_set_key_types(exon_hip_vcf_parser* parser, const char* packed_keys, const char* kinds, int32_t n);
int exon_hip_vcf_parser_info_text(exon_hip_vcf_parser* parser, void* stream, exon_hip_vcf_info_text* out);
/* (additive; the ABI stays 5) The `formats` Utf8 column, built on the device: FORMAT, a TAB, every sample printed again (see
 * exon_hip_scan_options.projection).  set_format_key_types: the value types of the header's ##FORMAT lines, packed like
 * set_key_types'; kinds i f c s (b is no FORMAT type: EXON_HIP_EINVAL).  GT is known by its name whatever the header says; the
 * reserved FORMAT keys of the specification keep their types unless the header names them; n = 0: the reserved keys alone.
 * formats_text follows info_text's contract and fills the same struct. */
int exon_hip_vcf_parser_set_format_key_types(exon_hip_vcf_parser* parser, const char* packed_keys, const char* kinds, int32_t n);
int exon_hip_vcf_parser_formats_text(exon_hip_vcf_parser* parser, void* stream, exon_hip_vcf_info_text* out);
int exon_hip_vcf_parser_destroy(exon_hip_vcf_parser* parser);

/* ---- BGZF inflate on the GPU (compressed blocks in HBM -> inflated bytes in HBM) ------------------------------------
 * Replaces noodles bgzf::AsyncReader around the byte stream (exon-core/src/datasources/vcf/file_opener/
 * unindex_file_opener.rs:62-70, fastq/file_opener.rs:69-75, streaming_bgzf.rs:56-64): RFC 1951 DEFLATE in RFC 1952
 * members carrying the BGZF "BC" extra field (SAM specification 4.1).  Blocks are independent: one wavefront each. */
typedef struct exon_hip_bgzf_block {
  uint32_t comp_offset; /* of the raw DEFLATE data inside the compressed buffer */
  uint32_t comp_size;
  uint32_t out_offset;  /* where the inflated bytes go inside the output buffer */
  uint32_t out_size;    /* ISIZE */
  uint32_t crc32;
  uint32_t reserved;
} exon_hip_bgzf_block;
/* Host: walk the block headers of `data[0..n)`.  Fills up to `cap` entries (blocks may be NULL to count only);
 * out_offset starts at `out_base` and advances by ISIZE.  *consumed = bytes of whole blocks walked (a trailing
 * partial block is left for the next call), *out_bytes = sum of ISIZE. */
int exon_hip_bgzf_scan(const uint8_t* data, size_t n, size_t out_base, exon_hip_bgzf_block* blocks, int32_t cap,
                       int32_t* n_blocks, size_t* consumed, size_t* out_bytes);
/* Device: inflate `n_blocks` blocks (table in host memory) from d_comp (4-byte aligned, with >= 4 KiB of readable
 * padding behind the last block) into d_out (4-byte aligned); verify_crc != 0 also checks every block's CRC-32.  Synchronises
 * `stream`.  A corrupt block -> EXON_HIP_EINVAL and *first_bad_block (else -1): inflate on the host instead. */
int exon_hip_bgzf_inflate(exon_hip_ctx* ctx, void* stream, const uint8_t* d_comp, const exon_hip_bgzf_block* blocks,
                          int32_t n_blocks, uint8_t* d_out, int32_t verify_crc, int32_t* first_bad_block);
/* The lane-parallel decoder keeps ~0.94 MiB of scratch per resident workgroup in a pool per (device, stream) -- up to ~1.4 GB
 * for a stream that inflated a 1536-member launch -- until the stream's owner lets go: streams the library owns do that
 * themselves; for a caller-owned `stream` passed to exon_hip_bgzf_inflate call this once the stream is idle. */
int exon_hip_bgzf_forget_stream(void* stream);
/* Diagnostics of the lane-parallel block decoder (HISTORY.md section 7e; used for launches of up to 1536 members unless
 * EXON_HIP_INFLATE_PAR says otherwise: 0 = never, 1 = always, 2 = side by side with the serial kernel): out32[0] = DEFLATE blocks
 * it decoded on the current device since the process started, out32[1..15] = blocks it handed back to the serial symbol loop, by
 * reason.  `stream` is ignored.  Synchronises the device. */
int exon_hip_bgzf_inflate_par_stats(void* stream, uint32_t* out32);

/* ---- FASTQ record splitting on the GPU (raw text in HBM -> per-read views into that text) ---------------------
 * Record rules of exon-fastq/src/batch_reader.rs:63-82 (noodles fastq: '@' definition line, sequence line, '+'
 * line, quality line; "\r\n" accepted).  The slab may end anywhere: consumed_bytes tells how many bytes form
 * whole records, the rest is carried into the next slab by the caller.  n_undecided != 0 (a record not starting
 * with '@', a missing '+' line, more lines than the parser was sized for, a partial record in the final slab):
 * decode that input on the host instead. */
typedef struct exon_hip_fastq_parser exon_hip_fastq_parser;
typedef struct exon_hip_fastq_views {
  int64_t n_reads;
  int64_t n_undecided;
  int64_t consumed_bytes;
  const int32_t* seq_start; /* device pointers owned by the parser, overwritten by the next parse call */
  const int32_t* seq_end;
  const int32_t* qual_start;
  const int32_t* qual_end;
  const uint8_t* text_base; /* what the views index: the 16-byte aligned address at or below d_text */
  const int32_t* head_start; /* (appended in round 6) the header line behind its '@' ... */
  const int32_t* head_end;   /* ... up to its end, CR dropped: name [space description] (exon-fastq/src/array_builder.rs:68-102) */
} exon_hip_fastq_views;
int exon_hip_fastq_parser_create(exon_hip_ctx* ctx, int64_t max_slab_bytes, exon_hip_fastq_parser** out);
/* d_text: any alignment, < 2 GiB.  final_slab != 0: the text ends the input (it must end with '\n').
 * Synchronises `stream`. */
int exon_hip_fastq_parser_parse(exon_hip_fastq_parser* parser, void* stream, const uint8_t* d_text, int64_t n_bytes,
                                int32_t final_slab, exon_hip_fastq_views* views);
int exon_hip_fastq_parser_destroy(exon_hip_fastq_parser* parser);

/* ---- (additive; the ABI stays 5) FASTA record splitting on the GPU (raw text in HBM -> definitions + compacted sequence layout) ----
 * The rules are the host reader's (FASTABatchReader + FASTAArrayBuilder, exon_amd/csrc/host/formats.h; exon-fasta/src/
 * batch_reader.rs:72-99, array_builder.rs:114-132), restated in gpu_parse.hip: lines end at '\n', one '\r' in front of it is dropped;
 * a line whose first byte is '>' starts a record and the rest of it is the definition; the sequence is every following line up to
 * the next '>' line, concatenated as it stands.  A record is a variable number of lines, so the parser describes the slab by LINE:
 * line l ends at line_end[l] (its '\n', an index into text_base), and the bytes it adds to the compacted sequence column lie at
 * [line_dst[l], line_dst[l + 1]) of that column (nothing for a definition line or an empty line).  Record r has the definition
 * [head_start[r], head_end[r]) -- behind '>', CR dropped -- and the sequence bytes [seq_offsets[r], seq_offsets[r + 1]): seq_offsets
 * is the Arrow int32 offsets buffer of the `sequence` column as it stands.
 * final_slab == 0: the slab's last record is never known to be complete: n_records = definition lines - 1 and consumed_bytes ends
 * directly in front of the last definition line (0 with fewer than two of them: the caller carries everything, or gives up).
 * final_slab != 0: every record is complete, consumed_bytes is the whole text (which must end with '\n').
 * n_undecided != 0 (the first line does not start with '>', more lines than the parser was sized for -- max_slab_bytes / 8 + 8, see
 * gpu_parse.hip): decode that input on the host instead.  The buffers are the parser's, overwritten by the next parse call. */
typedef struct exon_hip_fasta_parser exon_hip_fasta_parser;
typedef struct exon_hip_fasta_views {
  int64_t n_records;
  int64_t n_undecided;
  int64_t consumed_bytes;
  int64_t n_lines;               /* lines of the slab, the ones behind consumed_bytes included */
  int64_t seq_bytes;             /* = seq_offsets[n_records] */
  const uint8_t* text_base;      /* what the views index: the 16-byte aligned address at or below d_text */
  int64_t text_bytes;            /* bytes readable at text_base: n_bytes + first_line_start */
  int64_t first_line_start;      /* d_text - text_base (< 16): where line 0 starts */
  const int32_t* head_start;     /* [n_records] */
  const int32_t* head_end;       /* [n_records] */
  const int32_t* seq_offsets;    /* [n_records + 1] */
  const uint32_t* line_end;      /* [n_lines] */
  const uint32_t* line_dst;      /* [n_lines + 1] */
} exon_hip_fasta_views;
int exon_hip_fasta_parser_create(exon_hip_ctx* ctx, int64_t max_slab_bytes, exon_hip_fasta_parser** out);
/* d_text: any alignment, < 2 GiB.  Synchronises `stream`. */
int exon_hip_fasta_parser_parse(exon_hip_fasta_parser* parser, void* stream, const uint8_t* d_text, int64_t n_bytes,
                                int32_t final_slab, exon_hip_fasta_views* views);
int exon_hip_fasta_parser_destroy(exon_hip_fasta_parser* parser);

/* K10 (additive; the ABI stays 5).  Per-RECORD statistics of sequences (s = a record's sequence bytes as the reader returns them),
 *      integers only.  d_state holds 3 + 256 + (lmax + 2) + 32 + 102 int64 words (exon_hip_seq_stats_layout), and every word adds; a
 *      zeroed state is the empty state:
 *        totals       [3]         n_records, sum len(s), sum gc(s)
 *        composition  [256]       word b = number of sequence bytes equal to b, over all records
 *        length       [lmax + 2]  bin len(s) for len(s) <= lmax; bin lmax + 1 = every longer record (not an error: contigs are long)
 *        length_log2  [32]        bin 0 = empty sequence; bin k = 2^(k-1) <= len(s) < 2^k (int32 offsets keep k <= 31)
 *        gc_percent   [102]       bin floor(100 gc(s) / len(s)); bin 101 = empty sequence.  gc(s) = bytes equal to 'G' or 'C', upper
 *                                 case only (exon-core/src/udfs/sequence/gc_content.rs:52-71); the bin is the exact integer floor
 *                                 
 *      sum composition = sum len; composition['G'] + composition['C'] = sum gc; length, length_log2 and gc_percent each sum to
 *      n_records.  1 <= lmax <= 65536.  Validity is not read (as K5, K9); a negative offset difference counts as length 0; nothing in
 *      this plan is an input error.  The offsets must ascend, as Arrow requires: the kernel finds a tile's records by searching them,
 *      so offsets that do not ascend give counts without meaning (records missed or counted twice, G/C counts of several records
 *      in one) -- but never an access outside the payload or the state: every index is clamped.  No byte outside
 *      [offsets[0], offsets[n_records]) of `values` is loaded.  Accumulates.
 *      Any Utf8 column is an operand: through the host reader (pushes, a scan opened without gpu_parse) the plan counts whatever
 *      column `columns[0]` names -- `description` (1) of a FASTA scan included --, while the device path over FASTA text exists for
 *      column 2 alone and refuses any other index (EXON_HIP_EINVAL) instead of handing the scan to the host reader. */
int exon_hip_seq_stats_hist(exon_hip_ctx* ctx, void* stream, const exon_hip_column* sequence /*utf8*/, int64_t n_records, int32_t lmax,
                            int64_t* d_state);
/* K10 over the views of one FASTA slab resident in HBM (exon_hip_fasta_parser_parse; n_undecided must be 0): the n_records emitted
 * records, by the reader's rules (CR before LF dropped, definition lines and line ends are not sequence).  Nothing is compacted or
 * copied; no byte outside [first_line_start, first_line_start + consumed_bytes) of text_base is loaded. */
int exon_hip_seq_stats_hist_views(exon_hip_ctx* ctx, void* stream, const exon_hip_fasta_views* views, int32_t lmax, int64_t* d_state);
/* Host-only: out[0..4] = word offset of K10's totals / composition / length / length_log2 / gc_percent sections, out[5] = the
 * state's words.  EXON_HIP_EINVAL outside 1 <= lmax <= 65536.  Needs no device. */
int exon_hip_seq_stats_layout(int32_t lmax, int64_t* out /*[6]*/);

/* ---- BAM record splitting + field extraction on the GPU (inflated BAM bytes in HBM -> device-layout columns) ----
 * Column rules of BAMArrayBuilder::append (exon-bam/src/array_builder.rs:102-218) for flag, mapping_quality (NULL when
 * 255), reference id (NULL when -1), start = pos + 1 and end = start + reference length - 1 (NULL when pos < 0).
 * d_data must start at a record boundary; the chains of 64 KiB segments are walked in parallel from guessed record
 * starts and the guesses are proven by matching every chain's end with the next segment's start.  n_undecided != 0
 * (a proof failed, a record larger than a segment, a malformed record): decode on the host instead. */
typedef struct exon_hip_bam_parser exon_hip_bam_parser;
typedef struct exon_hip_bam_columns {
  int64_t n_rows;
  int64_t n_undecided;
  int64_t consumed_bytes; /* whole records; a record cut off by the end of the slab is left to the caller */
  int32_t* flag;          /* device pointers owned by the parser, overwritten by the next parse call */
  uint8_t* mapq;
  uint8_t* mapq_valid;
  int32_t* ref_id;
  uint8_t* ref_valid;
  int64_t* start;
  int64_t* end;
  uint8_t* pos_valid;     /* validity of start and end */
} exon_hip_bam_columns;
int exon_hip_bam_parser_create(exon_hip_ctx* ctx, int32_t n_references, int64_t max_slab_bytes, exon_hip_bam_parser** out);
/* Synchronises `stream`. */
int exon_hip_bam_parser_parse(exon_hip_bam_parser* parser, void* stream, const uint8_t* d_data, int64_t n_bytes,
                              exon_hip_bam_columns* cols);
/* (additive; the ABI stays 5) The aligned blocks of the slab of the LAST exon_hip_bam_parser_parse call of this parser -- d_data,
 * n_bytes and cols as that call had them -- for a caller that drives the parser itself: what a blocks-mode scan
 * (exon_hip_scan_set_cover_ops) runs per slab.  Rows, rule, cover_ops and the one shared validity bitmap are exon_hip_cigar_blocks';
 * d_row_mask (optional, one bit a row, LSB first): a row whose bit is 0 emits one invalid row.  out[0 .. 3) = ref_id (i32), start,
 * end (i64) of *n_blocks rows, in buffers that belong to the parser (16-byte aligned; overwritten by the next call, freed with the
 * parser).  Every load is checked against n_bytes again.  *n_undecided != 0: a record beyond the slab, or the CG-tag placeholder;
 * nothing was produced, decode on the host, whose reader reports what is wrong.  Synchronises `stream`. */
int exon_hip_bam_parser_cigar_blocks(exon_hip_bam_parser* parser, void* stream, const uint8_t* d_data, int64_t n_bytes, const exon_hip_bam_columns* cols,
                                     const uint8_t* d_row_mask, uint32_t cover_ops, exon_hip_column* out /*[3]*/, int64_t* n_blocks, int64_t* n_undecided);
int exon_hip_bam_parser_destroy(exon_hip_bam_parser* parser);

/* ---- SAM text parsing on the GPU (alignment lines in HBM -> the BAM device layout; `cols` is the BAM column struct) ----
 * Columns of exon-sam (schema_builder.rs:371-402, same as BAM): RNAME through the @SQ order ('*' / unknown -> NULL),
 * POS 0 -> NULL, MAPQ 255 -> NULL, end from the CIGAR.  d_text: '\n'-terminated alignment lines (no header), any
 * alignment; a trailing partial line is left to the caller (consumed_bytes). */
typedef struct exon_hip_sam_parser exon_hip_sam_parser;
int exon_hip_sam_parser_create(exon_hip_ctx* ctx, const char* const* reference_names, int32_t n_references,
                               int64_t max_slab_bytes, exon_hip_sam_parser** out);
int exon_hip_sam_parser_parse(exon_hip_sam_parser* parser, void* stream, const uint8_t* d_text, int64_t n_bytes,
                              exon_hip_bam_columns* cols);
int exon_hip_sam_parser_destroy(exon_hip_sam_parser* parser);

/* ---- GFF3 text parsing on the GPU (lines in HBM -> the GFF device layout) ----
 * Line rules of exon_amd/csrc/host/gff.h.  Lines that start with '#' are no rows.  seqname / source / type become ids into
 * dictionaries the parser builds across slabs (at most EXON_HIP_MAX_GROUPS values and 1 MiB of text each); `seed_seqnames`
 * are inserted before the first slab with ids 0 .. n_seed - 1, so that a region plan knows its contig's id up front.
 * n_undecided != 0 (a malformed field, more than 18 digits, a score the device leaves open, an empty line, a ##FASTA line, a
 * dictionary past its limits): decode the file on the host instead -- errors are the host reader's to report. */
typedef struct exon_hip_gff_parser exon_hip_gff_parser;
typedef struct exon_hip_gff_columns {
  int64_t n_rows, n_undecided, consumed_bytes; /* consumed: up to and including the last newline */
  const int32_t *seqname_id, *source_id, *type_id; /* device pointers owned by the parser, overwritten by the next parse call */
  const int64_t *start, *end;
  const float* score;
  const uint8_t* score_valid;
  const int32_t* strand_id; /* 0 "+", 1 "-" */
  const uint8_t* strand_valid;
  const int32_t* phase_id;  /* 0, 1, 2 */
  const uint8_t* phase_valid;
} exon_hip_gff_columns;
int exon_hip_gff_parser_create(exon_hip_ctx* ctx, const char* const* seed_seqnames, int32_t n_seed, int64_t max_slab_bytes,
                               exon_hip_gff_parser** out);
/* d_text: '\n'-terminated lines, any alignment; a trailing partial line is left to the caller.  Synchronises `stream`. */
int exon_hip_gff_parser_parse(exon_hip_gff_parser* parser, void* stream, const uint8_t* d_text, int64_t n_bytes,
                              exon_hip_gff_columns* cols);
/* the dictionary of column 0 (seqname), 1 (source) or 2 (type) discovered so far, '\0'-separated in id order */
int exon_hip_gff_parser_names(exon_hip_gff_parser* parser, int32_t column, char* buf, size_t cap, int32_t* n_names);
/* The `attributes` column of the slab of the last parse call (additive; the ABI stays 5), built on the device: the buffers of
 * Map<Utf8, List<Utf8>> -- rows -> entries (map_offsets), entries -> key bytes (key_offsets) and -> items (list_offsets),
 * items -> item bytes (item_offsets); bytes after percent-decoding.  Call exon_hip_gff_parser_want_attributes(parser, 1)
 * BEFORE the parse call (the line kernel then records where every row's ninth field lies; without it nothing new runs), and
 * exon_hip_gff_parser_attributes after it and before the next one.  n_undecided != 0 (a byte >= 0x80, raw or decoded; a piece
 * without '='; an empty piece other than the one behind a trailing ';'; more items than the scratch holds): nothing was
 * built, the host reader decides.  Device pointers owned by the parser, overwritten by the next call.  Synchronises `stream`. */
typedef struct exon_hip_gff_attributes {
  int64_t n_entries, n_items, n_key_bytes, n_item_bytes, n_undecided;
  const int32_t* map_offsets;  /* [n_rows + 1] */
  const int32_t* key_offsets;  /* [n_entries + 1] */
  const uint8_t* key_values;   /* [n_key_bytes] */
  const int32_t* list_offsets; /* [n_entries + 1] */
  const int32_t* item_offsets; /* [n_items + 1] */
  const uint8_t* item_values;  /* [n_item_bytes] */
} exon_hip_gff_attributes;
int exon_hip_gff_parser_want_attributes(exon_hip_gff_parser* parser, int32_t on);
int exon_hip_gff_parser_attributes(exon_hip_gff_parser* parser, void* stream, exon_hip_gff_attributes* out);
/* GTF on the same parser (additive; the ABI stays 5).  exon_hip_gff_parser_set_dialect(parser, EXON_HIP_FORMAT_GTF) before a
 * parse call: the line rules of exon_amd/csrc/host/gtf.h (a '?' strand makes the row undecided; the eighth column is the frame)
 * hold from then on; EXON_HIP_FORMAT_GFF switches back, any other value is EXON_HIP_EINVAL.
 * exon_hip_gff_parser_gtf_attributes builds the slab's `attributes` column, Map<Utf8, Utf8>, by gtf.h's ATTRIBUTE RULES -- rows ->
 * entries (map_offsets), entries -> key bytes (key_offsets) and -> value bytes (value_offsets); keys and values are spans of the
 * text, quotes dropped.  Same protocol as exon_hip_gff_parser_attributes (want_attributes, parse, then this); on a parser of
 * the GFF dialect it is EXON_HIP_ESTATE, as exon_hip_gff_parser_attributes is on one of the GTF dialect.  n_undecided != 0 (a
 * byte >= 0x80; a missing closing quote; a key without a value; an empty piece; bytes other than spaces behind a closing
 * quote): nothing was built, the host reader decides. */
typedef struct exon_hip_gtf_attributes {
  int64_t n_entries, n_key_bytes, n_value_bytes, n_undecided;
  const int32_t* map_offsets;   /* [n_rows + 1] */
  const int32_t* key_offsets;   /* [n_entries + 1] */
  const uint8_t* key_values;    /* [n_key_bytes] */
  const int32_t* value_offsets; /* [n_entries + 1] */
  const uint8_t* value_values;  /* [n_value_bytes] */
} exon_hip_gtf_attributes;
int exon_hip_gff_parser_set_dialect(exon_hip_gff_parser* parser, int32_t format);
int exon_hip_gff_parser_gtf_attributes(exon_hip_gff_parser* parser, void* stream, exon_hip_gtf_attributes* out);
int exon_hip_gff_parser_destroy(exon_hip_gff_parser* parser);

/* ---- BED text parsing on the GPU (lines in HBM -> the BED device layout; additive, the ABI stays 5) ----
 * Line rules of exon_amd/csrc/host/bed.h.  Lines that start with '#' are no rows.  reference_sequence_name becomes an id into a
 * dictionary the parser builds across slabs (limits and `seed_names` as for the GFF parser).  Every line is validated in full.
 * exon_hip_bed_parser_want(parser, projection) BEFORE a parse call: with any of EXON_HIP_PROJECT_BED_NAME / _SCORE / _STRAND the
 * line kernel also writes score, strand and where every row's name lies; with 0 (the default: a fused plan) it writes the three
 * operand columns and nothing else, and the other pointers of exon_hip_bed_columns are NULL.
 * n_undecided != 0 (anything the rules call an error, a byte >= 0x80 anywhere in a line -- UTF-8 is the host's to validate --, a
 * position of more than 18 digits, a ##FASTA line, a dictionary past its limits): decode the file on the host instead --
 * errors are the host reader's to report. */
typedef struct exon_hip_bed_parser exon_hip_bed_parser;
typedef struct exon_hip_bed_columns {
  int64_t n_rows, n_undecided, consumed_bytes; /* consumed: up to and including the last newline */
  const int32_t* chrom_id;                     /* device pointers owned by the parser, overwritten by the next parse call */
  const int64_t *start, *end;
  const int64_t* score;
  const uint8_t* score_valid;
  const int32_t* strand_id; /* 0 "+", 1 "-" */
  const uint8_t* strand_valid;
  const uint32_t *name_off, *name_len; /* the name's bytes in the (16-byte aligned) slab `text`; length 0 where NULL */
  const uint8_t* name_valid;
  const uint8_t* text;
} exon_hip_bed_columns;
int exon_hip_bed_parser_create(exon_hip_ctx* ctx, const char* const* seed_names, int32_t n_seed, int64_t max_slab_bytes,
                               exon_hip_bed_parser** out);
int exon_hip_bed_parser_want(exon_hip_bed_parser* parser, uint64_t projection);
/* d_text: '\n'-terminated lines, any alignment; a trailing partial line is left to the caller.  Synchronises `stream`. */
int exon_hip_bed_parser_parse(exon_hip_bed_parser* parser, void* stream, const uint8_t* d_text, int64_t n_bytes,
                              exon_hip_bed_columns* cols);
/* the reference_sequence_name dictionary discovered so far, '\0'-separated in id order */
int exon_hip_bed_parser_names(exon_hip_bed_parser* parser, char* buf, size_t cap, int32_t* n_names);
int exon_hip_bed_parser_destroy(exon_hip_bed_parser* parser);

/* ---- BCF2 record splitting + field extraction on the GPU (inflated BCF bytes in HBM -> the VCF device layout) ----
 * Same Arrow schema as VCF (exon-core/src/datasources/bcf/, exon-bcf); records are found like BAM's (parallel chain
 * walk, guessed starts proven by induction) and decoded one thread each: typed-value walk to FILTER (interned as a list
 * of header-string indexes) and one typed INFO key (dictionary index; Float or Integer value -> f32, missing -> NULL).
 * `cols` is the VCF column struct (pos_valid is NULL: POS is a fixed field). */
typedef struct exon_hip_bcf_parser exon_hip_bcf_parser;
int exon_hip_bcf_parser_create(exon_hip_ctx* ctx, int32_t n_contigs, int32_t n_header_strings, int32_t n_samples,
                               int32_t info_key /* header-string index of the INFO field, -1 = none */, int64_t max_slab_bytes,
                               exon_hip_bcf_parser** out);
/* several typed INFO fields instead of the single key of _create: header-string indexes + kinds ('f' Float -> f32, 'i' Integer
 * -> i32, 'b' Flag -> presence bitmap), up to EXON_HIP_MAX_INFO_FIELDS; call before the first parse */
int exon_hip_bcf_parser_set_info_keys(exon_hip_bcf_parser* parser, const int32_t* keys, const char* kinds, int32_t n);
int exon_hip_bcf_parser_parse(exon_hip_bcf_parser* parser, void* stream, const uint8_t* d_data, int64_t n_bytes,
                              exon_hip_vcf_columns* cols);
/* FILTER lists discovered so far, in id order: lists[8 * i .. 8 * i + counts[i]) are header-string indexes ([] = '.') */
int exon_hip_bcf_parser_filters(exon_hip_bcf_parser* parser, int32_t* lists, int32_t* counts, int32_t cap, int32_t* n_filters);
int exon_hip_bcf_parser_destroy(exon_hip_bcf_parser* parser);

/* GpuFilterAggExec::execute in one call: pull every batch of `scan` and push it through `stream`. */
int exon_hip_stream_consume_scan(exon_hip_stream* s, exon_hip_scan* scan, int64_t* rows);

#ifdef __cplusplus
}
#endif
#endif /* EXON_HIP_H */
