// internal.h -- shared between capi.cpp (ctx + operator launches) and stream.cpp (plan/stream layer).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/exon_hip.h"
#include "host/text_nodes.h"
#include "kernels.h"

struct exon_hip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;  // used when the caller passes stream == NULL
  exon::LaunchCfg cfg;
  std::mutex mu;
  std::map<hipStream_t, exon::Workspace> workspaces;
  std::string error;
  hipDeviceProp_t props;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // device buffers of the GPU-side parsers are recycled between scans (exon_pool_*): their sizes repeat exactly and
  // hipMalloc / hipFree of gigabytes costs tens of milliseconds per file
  std::multimap<size_t, void*> pool_free;
  std::map<void*, size_t> pool_live;
};

// records the message on the ctx (and the calling thread) and returns `code`
int fail(exon_hip_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
const std::string& exon_hip_tls_error();

#define HIP_TRY(ctx, expr)                                                                             \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(ctx, EXON_HIP_EDEVICE, "%s: %s", #expr, hipGetErrorString(e_));  \
  } while (0)

inline hipStream_t pick_stream(exon_hip_ctx* ctx, void* s) { return s ? (hipStream_t)s : ctx->stream; }

// Workspace of `words` 8-byte partial words for launches on stream `s` (grown on demand).
int get_workspace(exon_hip_ctx* ctx, hipStream_t s, size_t words, exon::Workspace* out);

// inflate.hip: enqueue the BGZF inflate (+ CRC-32) kernels over device-resident block tables
// a stream that is about to be destroyed: release the inflate scratch kept for it (the stream must be idle)
void exon_bgzf_forget_stream(hipStream_t s);
hipError_t exon_bgzf_inflate_launch(hipStream_t s, const uint8_t* d_comp, const exon_hip_bgzf_block* d_blocks, int n_blocks,
                                    uint8_t* d_out, int* d_status, bool verify_crc, bool text_like = true);
const char* exon_bgzf_status_name(int code);

// scan.cpp: slab buffers kept per ctx between scans
void exon_hip_release_ctx_caches(exon_hip_ctx* ctx);
const void* exon_hip_gpu_local_cpus(int device);  // scan.cpp: a cpu_set_t of the GPU's NUMA node (nullptr: nothing to choose), and ...
void exon_hip_run_on(const void* cpus);            // ... the calling thread's affinity set to it (host threads that feed the DMA engine)
void exon_hip_prewarm_ctx(exon_hip_ctx* ctx);  // scan.cpp: the file pipelines' side streams and events, made with the context

// text_columns.hip: the reference's string / list columns of a slab as Arrow buffers on the device (exon_hip_scan_options.projection).
// Every exon_text_* describes what it built as ExonTextColumns (host/text_nodes.h): one root per projected column, in schema order.
struct ExonTextScratch;
// the INFO key types of a VCF header on the device (text_columns.hip: exon_vcf_key_table_build, vcf_key_type): open addressing
// by the key's 64-bit hash (0: an empty slot), the key's text verified; type: i f b c s
struct ExonVcfKeyTable {
  const unsigned long long* hash;
  const uint32_t *off, *len;  // the key's text in `text`
  const uint8_t *type, *text;
  unsigned mask;              // slots - 1
};
class PoolBufs;
// which reserved keys of the specification seed the table behind the header's: INFO's (VcfKeyTypes::reserved_info) or FORMAT's
// (::reserved_format; kinds i f c s -- GT is known by its name, not by the table)
enum class ExonVcfKeySeed { Info, Format };
int exon_vcf_key_table_build(exon_hip_ctx* ctx, PoolBufs* bufs, const char* keys, const char* kinds, int32_t n, ExonVcfKeySeed seed, ExonVcfKeyTable* out);
// gpu_parse.hip: the table exon_hip_vcf_parser_set_key_types has made (hash == nullptr: none yet), and _set_format_key_types'
const ExonVcfKeyTable* exon_hip_vcf_parser_key_table(exon_hip_vcf_parser* p);
const ExonVcfKeyTable* exon_hip_vcf_parser_format_key_table(exon_hip_vcf_parser* p);
// n_undecided != 0 (every exon_text_* that has it): nothing was built, the slab is the host reader's -- a total beyond what the
// scratch buffers hold (IDs of many empty items, CIGARs of long ops; see scratch_for), or what the format's own note names
// (VCF `info`, with EXON_HIP_PROJECT_VCF_INFO and info_keys: the rows text_columns.hip lists next to k_vcf_info_measure)
// VCF: id List<Utf8>? (validity: the ID field is not '.'), ref Utf8, alt List<Utf8>? (validity: ALT is not '.'; no offsets, no items:
// see text_columns.hip), info Utf8 (the entries printed again; never NULL, "" for INFO '.'), formats Utf8 (FORMAT, a TAB, the samples
// printed again; never NULL; built only with EXON_HIP_PROJECT_VCF_FORMATS | _FORMATS_ON_DEVICE and format_keys -- undecided: the rows
// text_columns.hip lists next to k_fmt_rows)
int exon_text_vcf(exon_hip_ctx* ctx, void* stream, ExonTextScratch** scratch, const uint8_t* d_text, int64_t n_bytes, const unsigned* d_nl, int64_t n_rows, uint64_t projection,
                  const ExonVcfKeyTable* info_keys, const ExonVcfKeyTable* format_keys, ExonTextColumns* out, int64_t* n_undecided);
// BAM: name Utf8?, cigar Utf8, sequence Utf8, quality_scores List<Int64> over sequence's offsets (a record's qualities are as many as its bases)
int exon_text_bam(exon_hip_ctx* ctx, void* stream, ExonTextScratch** scratch, const uint8_t* d_data, int64_t n_bytes, const uint32_t* d_rec_of_row, int64_t n_rows, uint64_t projection,
                  ExonTextColumns* out, int64_t* n_undecided);
// SAM lines (the parser's newline index) -> the same columns, quality_scores over offsets of its own (QUAL may be '*' next to a SEQ);
// n_undecided != 0: a line the device does not print the way the reader would
int exon_text_sam(exon_hip_ctx* ctx, void* stream, ExonTextScratch** scratch, const uint8_t* d_text, int64_t n_bytes, const unsigned* d_nl, int64_t n_rows, uint64_t projection,
                  ExonTextColumns* out, int64_t* n_undecided);
// FASTQ: name, description? (validity: the header has something behind its first space), sequence, quality_scores, all Utf8
// (exon-fastq/src/config.rs:79-88), in that order
int exon_text_fastq(exon_hip_ctx* ctx, void* stream, ExonTextScratch** scratch, const exon_hip_fastq_views* views, int64_t n_bytes, ExonTextColumns* out);
// FASTA: id, description? (validity: something follows the blanks behind the id), sequence, all Utf8 (host/formats.h FASTABatchReader::schema),
// in that order; sequence's offsets are the parser's seq_offsets, its bytes every sequence line copied to its line_dst (one small
// group of lanes per LINE: k_fasta_seq_fill)
int exon_text_fasta(exon_hip_ctx* ctx, void* stream, ExonTextScratch** scratch, const exon_hip_fasta_views* views, ExonTextColumns* out);
// BCF id / ref / alt through the reference's EAGER builder (eager_array_builder.rs:112-134): both lists carry their items, neither is
// ever NULL (an empty list when the record has no id / no alternate bases)
int exon_text_bcf(exon_hip_ctx* ctx, void* stream, ExonTextScratch** scratch, const uint8_t* d_data, int64_t n_bytes, const uint32_t* d_rec_of_row, int64_t n_rows, uint64_t projection,
                  ExonTextColumns* out, int64_t* n_undecided);
// GFF `attributes` (Map<Utf8, List<Utf8>>, host/gff.h's ATTRIBUTE RULES): rows -> entries -> (key bytes | items -> item bytes),
// bytes after percent-decoding.  d_text is the ALIGNED slab the
// parser indexed; d_attr_off / d_attr_len every row's ninth field in it (k_parse_gff_lines<true>).  n_undecided != 0: a field with a
// byte >= 0x80 (raw or decoded: UTF-8 is the host's to validate), a piece without '=', an empty piece other than the one behind a
// trailing ';', or more items than the items' offsets hold
int exon_text_gff(exon_hip_ctx* ctx, void* stream, ExonTextScratch** scratch, const uint8_t* d_text, int64_t n_bytes, const uint32_t* d_attr_off, const uint32_t* d_attr_len,
                  int64_t n_rows, ExonTextColumns* out, int64_t* n_undecided);
// GTF `attributes` (Map<Utf8, Utf8>, host/gtf.h's ATTRIBUTE RULES): rows -> entries -> (key bytes | value bytes), keys and values
// spans of the text as they stand (quotes dropped).  d_text / d_attr_off / d_attr_len
// as for exon_text_gff (the line kernel of the GTF dialect recorded them).  n_undecided != 0: a field with a byte >= 0x80, a missing
// closing quote, a key without a value, an empty piece, or bytes other than spaces behind a closing quote
int exon_text_gtf(exon_hip_ctx* ctx, void* stream, ExonTextScratch** scratch, const uint8_t* d_text, int64_t n_bytes, const uint32_t* d_attr_off, const uint32_t* d_attr_len,
                  int64_t n_rows, ExonTextColumns* out, int64_t* n_undecided);
// BED `name` (Utf8?, host/bed.h: the field's bytes as they stand, NULL on 3- and 4-field lines): d_text is the ALIGNED slab the
// parser indexed; d_name_off / d_name_len every row's name in it (k_parse_bed_lines<true>; length 0 where NULL) and d_name_valid its
// bitmap, which the column takes as it is.  Nothing here is undecided: the line kernel has judged every byte of the line
int exon_text_bed(exon_hip_ctx* ctx, void* stream, ExonTextScratch** scratch, const uint8_t* d_text, int64_t n_bytes, const uint32_t* d_name_off, const uint32_t* d_name_len,
                  const uint8_t* d_name_valid, int64_t n_rows, ExonTextColumns* out);
void exon_text_scratch_destroy(ExonTextScratch* s);
// take_rows.hip: the rows a pushed-down predicate (VCF value, BAM / SAM flag / mapping quality) keeps, taken out of a slab's columns on the device (format-free: a fixed
// column is a width, a text column a tree of ExonTextNode kinds).  The scratch is made by the first exon_take_index and sized from
// the inputs of every call; what a call returns lives until the same call on the next slab.
struct ExonTakeScratch;
void exon_take_scratch_destroy(ExonTakeScratch* s);
// row mask (n_rows bits, bits behind them ignored) -> the kept rows' indices, ascending, and their count, both on the device; *K is
// the count read back (the one host wait of the step)
int exon_take_index(exon_hip_ctx* ctx, void* stream, ExonTakeScratch** scratch, const uint8_t* d_mask, int64_t n_rows, const uint32_t** d_rows, const unsigned** d_K, int64_t* K);
// one fixed-width column: values `width` bytes wide (0: none, a Flag's bitmap is its value) and / or a validity bitmap in, the kept
// rows' values and bits out (out_* are set by the call; nullptr where the input has none)
struct ExonTakeColumn {
  const void* values;
  const uint8_t* validity;
  int width;
  void* out_values;
  uint8_t* out_validity;
};
int exon_take_fixed(exon_hip_ctx* ctx, void* stream, ExonTakeScratch* scratch, ExonTakeColumn* cols, int n_cols);
// the kept rows of every root of `in` (UTF8 and LIST nodes, a LIST's INT64 item leaf; STRUCT2: EXON_HIP_EUNSUPPORTED) as columns of their own in `out`,
// lengths and totals filled in from one readback
int exon_text_take(exon_hip_ctx* ctx, void* stream, ExonTakeScratch* scratch, const ExonTextColumns& in, const uint32_t* d_rows, const unsigned* d_K, ExonTextColumns* out);
// the parsers' own indexes the text columns are built from (valid until the next parse call)
const unsigned* exon_hip_vcf_parser_newlines(exon_hip_vcf_parser* p);
// a device-built dictionary holds up to EXON_HIP_MAX_GROUPS names in a text pool of EXON_DICT_POOL bytes: its names, '\0'-separated,
// fit EXON_DICT_NAMES_CAP bytes.  The fetches behind the public exon_hip_*_parser_filters / _names / _info_values; so_far: they also
// answer after the table overflowed, with the names assigned before it (the exporter names a slab's batches after the next slab was
// parsed, which may have overflowed the table)
constexpr int EXON_DICT_POOL = 1 << 20;
constexpr size_t EXON_DICT_NAMES_CAP = (size_t)EXON_DICT_POOL + EXON_HIP_MAX_GROUPS;
int exon_vcf_parser_filter_names(exon_hip_vcf_parser* p, char* buf, size_t cap, int32_t* n_filters, bool so_far);
int exon_vcf_parser_info_value_names(exon_hip_vcf_parser* p, int32_t key, char* buf, size_t cap, int32_t* n_values, bool so_far);
int exon_gff_parser_column_names(exon_hip_gff_parser* p, int32_t column, char* buf, size_t cap, int32_t* n_names, bool so_far);
// gpu_parse.hip: the aligned slab of the last parse call and every row's ninth field in it (after exon_hip_gff_parser_want_attributes)
void exon_hip_gff_parser_attr_fields(exon_hip_gff_parser* p, const uint8_t** text, int64_t* n_bytes, const uint32_t** off, const uint32_t** len);
struct exon_hip_bed_parser;
int exon_bed_parser_reference_names(exon_hip_bed_parser* p, char* buf, size_t cap, int32_t* n_names, bool so_far);
// gpu_parse.hip: the aligned slab of the last parse call and every row's name in it (after exon_hip_bed_parser_want with a projection)
void exon_hip_bed_parser_name_fields(exon_hip_bed_parser* p, const uint8_t** text, int64_t* n_bytes, const uint32_t** off, const uint32_t** len, const uint8_t** valid);
int exon_bcf_parser_filter_lists(exon_hip_bcf_parser* p, int32_t* lists, int32_t* counts, int32_t cap, int32_t* n_filters, bool so_far);
const unsigned* exon_hip_sam_parser_newlines(exon_hip_sam_parser* p);      // gpu_parse.hip: the same for SAM lines      // gpu_parse.hip: byte offset of every line's '\n' in the aligned slab
const uint32_t* exon_hip_bam_parser_row_records(exon_hip_bam_parser* p);
const uint32_t* exon_hip_bcf_parser_row_records(exon_hip_bcf_parser* p);   // bcf_parse.hip: the same for BCF records   // bam_parse.hip: byte offset of every row's record

// cigar_blocks.hip: one slab's alignment rows -> their aligned blocks as rows (ref_id, start, end) with ONE validity bitmap, in buffers
// that belong to the scan (exon_hip_scan_set_cover_ops).  rec_of_row set: a BAM slab (`data` = the records); else a SAM slab (`data` =
// the text as the parser was given it, `newlines` = its line index).  *undecided: the host reader takes the file.
struct ExonBlockBufs;
struct ExonBlockSlab {
  const uint8_t* data;
  int64_t n_bytes;
  const uint32_t* rec_of_row;
  const unsigned* newlines;
  const int32_t* ref;
  const uint8_t* ref_valid;
  const int64_t* start;
  const uint8_t* pos_valid;
  const uint8_t* row_mask;  // NULL: every row is kept
  int64_t n_rows;
  uint32_t cover_ops;
};
int exon_cigar_blocks_slab(exon_hip_ctx* ctx, void* stream, ExonBlockBufs** bufs, const ExonBlockSlab& in, exon_hip_column* cols /*[3]*/, int64_t* n_blocks, int* undecided);
void exon_cigar_blocks_free(ExonBlockBufs* b);

// capi.cpp: size-keyed recycling of device buffers (released by exon_hip_ctx_destroy)
void* exon_pool_alloc(exon_hip_ctx* ctx, size_t bytes);
void exon_pool_free(exon_hip_ctx* ctx, void* p);

// The device buffers of one parser (or scratch) out of the ctx's pool, plus pinned host mirrors: each is freed exactly once, by
// release() or the destructor.  Failures are sticky: after the first one every take returns nullptr and status() keeps it.
class PoolBufs {
 public:
  explicit PoolBufs(exon_hip_ctx* ctx) : ctx_(ctx) {}
  ~PoolBufs() { release(); }
  PoolBufs(const PoolBufs&) = delete;
  PoolBufs& operator=(const PoolBufs&) = delete;
  // `bytes` of device memory; fill >= 0: every byte set to it
  template <class T>
  T* take(size_t bytes, int fill = -1) {
    if (err_ != hipSuccess) return nullptr;
    void* p = exon_pool_alloc(ctx_, bytes);
    if (!p) {
      err_ = hipErrorOutOfMemory;
      return nullptr;
    }
    dev_.push_back(p);
    // The fill runs on the NULL stream and a memset of device memory may return before it has run; the kernels that read the buffer
    // run on non-blocking streams, which the null stream does not order.  Without the wait a recycled buffer can still hold another
    // parser's words when the first kernel reads them (the line index: look-back words of the same generation), or be zeroed under it.
    if (fill >= 0 && ((err_ = hipMemset(p, fill, bytes)) != hipSuccess || (err_ = hipStreamSynchronize(nullptr)) != hipSuccess)) return nullptr;
    return static_cast<T*>(p);
  }
  template <class T>
  T* pinned(size_t bytes) {
    void* p = nullptr;
    if (err_ != hipSuccess || (err_ = hipHostMalloc(&p, bytes)) != hipSuccess) return nullptr;
    host_.push_back(p);
    return static_cast<T*>(p);
  }
  void upload(void* dst, const void* src, size_t bytes) {
    if (err_ == hipSuccess && bytes) err_ = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  }
  hipError_t status() const { return err_; }
  void release() {
    for (void* p : dev_) exon_pool_free(ctx_, p);
    for (void* p : host_) hipHostFree(p);
    dev_.clear();
    host_.clear();
    err_ = hipSuccess;
  }

 private:
  exon_hip_ctx* ctx_;
  std::vector<void*> dev_, host_;
  hipError_t err_ = hipSuccess;
};

// internal launch flags next to the public EXON_HIP_LAUNCH_* bits: K4's compared column / AVG argument is Int32
// (exon_hip_plan_desc.x_type / y_type)
#define EXON_LAUNCH_X_INT32 0x100
#define EXON_LAUNCH_Y_INT32 0x200

// capi.cpp: the operator launches with EXON_HIP_LAUNCH_* flags (the extern "C" operators are the ACCUMULATE forms)
int exon_op_region_count(exon_hip_ctx* ctx, void* stream, const exon_hip_column* chrom_id, const exon_hip_column* pos,
                         int64_t n, int32_t region_chrom_id, int64_t start, int64_t end, int64_t* d_count, int flags);
int exon_op_overlap_count(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id, const exon_hip_column* start,
                          const exon_hip_column* end, int64_t n, int32_t region_ref_id, int64_t region_start,
                          int64_t region_end, int64_t* d_count, int flags, bool strict);
int exon_op_flag_mapq_group_count(exon_hip_ctx* ctx, void* stream, const exon_hip_column* flag,
                                  const exon_hip_column* mapq, const exon_hip_column* ref_id, int64_t n,
                                  int32_t flag_mask, int32_t flag_value, int32_t mapq_min, int32_t n_refs,
                                  int64_t* d_counts, int flags);
int exon_op_cmp_avg_by_group(exon_hip_ctx* ctx, void* stream, const exon_hip_column* x, const exon_hip_column* y,
                             const exon_hip_column* group_id, int64_t n, double threshold, int32_t cmp_op,
                             int32_t n_groups, int64_t* d_counts, double* d_sums, int flags);
int exon_op_cmp_minmax_by_group(exon_hip_ctx* ctx, void* stream, const exon_hip_column* x, const exon_hip_column* y,
                                const exon_hip_column* group_id, int64_t n, double threshold, int32_t cmp_op,
                                int32_t n_groups, int64_t* d_state, int flags);
int exon_op_qual_pos_hist(exon_hip_ctx* ctx, void* stream, const exon_hip_column* q, int64_t n_reads, int32_t lmax,
                          int64_t* d_hist, int flags);
int exon_op_read_stats_hist(exon_hip_ctx* ctx, void* stream, const exon_hip_column* seq, const exon_hip_column* qual, int64_t n_reads,
                            int32_t lmax, int64_t* d_state, int flags);
int exon_op_seq_stats_hist(exon_hip_ctx* ctx, void* stream, const exon_hip_column* seq, int64_t n_records, int32_t lmax, int64_t* d_state,
                           int flags);
int exon_op_seq_stats_hist_views(exon_hip_ctx* ctx, void* stream, const exon_hip_fasta_views* views, int32_t lmax, int64_t* d_state, int flags);
int exon_op_region_set_overlap(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id, const exon_hip_column* start, const exon_hip_column* end,
                               int64_t n, const exon::RegionSetTables& tables, int64_t* d_state, int flags);
int exon_op_region_set_bases(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id, const exon_hip_column* start, const exon_hip_column* end,
                             int64_t n, const exon::RegionBasesTables& tables, int64_t* d_state, int flags);
int exon_op_window_bases(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id, const exon_hip_column* start, const exon_hip_column* end, int64_t n,
                         const exon::WindowBasesTables& tables, int64_t* d_state, int flags);
int exon_op_region_set_depth(exon_hip_ctx* ctx, void* stream, const exon_hip_column* ref_id, const exon_hip_column* start, const exon_hip_column* end, int64_t n,
                             const exon::RegionDepthTables& tables, int64_t* d_state, int flags);
int exon_op_region_depth_reduce(exon_hip_ctx* ctx, void* stream, const exon::RegionDepthReduce& r, const int64_t* d_state, int64_t* d_out);
// chunk c is q[c * stride]
int exon_op_qual_pos_hist_chunks(exon_hip_ctx* ctx, void* stream, const exon_hip_column* q, int stride, int32_t n_chunks,
                                 const int64_t* n_reads, int32_t lmax, int64_t* d_hist, int flags);
