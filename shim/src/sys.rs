//! Raw FFI of include/exon_hip.h (hand-written; bindgen would produce the same).  ABI version 4.
//! `tests/test_shim_layout.py` parses the `#[repr(C)]` structs below and checks field order, offsets and sizes against
//! `include/exon_hip.h` through a gcc-compiled `offsetof` dump, so this file cannot drift from the header unnoticed.
#![allow(non_camel_case_types)]
use arrow::ffi::{FFI_ArrowArray, FFI_ArrowSchema};
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct exon_hip_ctx { _p: [u8; 0] }
#[repr(C)]
pub struct exon_hip_plan { _p: [u8; 0] }
#[repr(C)]
pub struct exon_hip_stream { _p: [u8; 0] }
#[repr(C)]
pub struct exon_hip_scan { _p: [u8; 0] }
#[repr(C)]
pub struct exon_hip_vcf_parser { _p: [u8; 0] }
/// exon_hip_vcf_parser_info_text's and _formats_text's result (device pointers, owned by the parser): handled by pointer only
#[repr(C)]
pub struct exon_hip_vcf_info_text { _p: [u8; 0] }
/// exon_hip_fasta_parser_parse's result (device pointers, owned by the parser): handled by pointer only
#[repr(C)]
pub struct exon_hip_fasta_views { _p: [u8; 0] }

pub const EXON_HIP_ABI_VERSION: i32 = 5;
pub const EXON_HIP_PLAN_REGION_COUNT: i32 = 2;
pub const EXON_HIP_PLAN_FLAG_MAPQ_GROUP_COUNT: i32 = 3;
pub const EXON_HIP_PLAN_CMP_AVG_BY_GROUP: i32 = 4;
pub const EXON_HIP_PLAN_QUAL_POS_HIST: i32 = 5;
pub const EXON_HIP_PLAN_OVERLAP_COUNT: i32 = 6;
pub const EXON_HIP_PLAN_WITHIN_COUNT: i32 = 7;
pub const EXON_HIP_PLAN_CMP_MINMAX_BY_GROUP: i32 = 8; // K4's fields; state = 4 * n_groups int64 words (counts, then min / max words)
pub const EXON_HIP_PLAN_READ_STATS_HIST: i32 = 9; // lmax, columns (sequence, quality_scores); state = exon_hip_read_stats_layout words, all add
pub const EXON_HIP_PLAN_SEQ_STATS_HIST: i32 = 10; // lmax, column (sequence); state = exon_hip_seq_stats_layout words, all add
pub const EXON_HIP_PLAN_REGION_SET_OVERLAP: i32 = 11; // made by exon_hip_plan_create_region_set; state = 4 + 2 * (M + C) words, all add
pub const EXON_HIP_REGION_SET_MAX_REGIONS: i32 = 1048576;
pub const EXON_HIP_PLAN_REGION_SET_BASES: i32 = 12; // made by exon_hip_plan_create_region_set_bases; state = 4 + 4 * (P + C) words, all add modulo 2^64
pub const EXON_HIP_PLAN_WINDOW_BASES: i32 = 13; // made by exon_hip_plan_create_window_bases; state = 4 + 2 * B words, all add modulo 2^64
pub const EXON_HIP_WINDOW_MAX_BINS: i32 = 33554432;
pub const EXON_HIP_PLAN_REGION_SET_DEPTH: i32 = 14; // made by exon_hip_plan_create_region_set_depth; state = 4 + T + C words, all add modulo 2^64
pub const EXON_HIP_REGION_DEPTH_MAX_BINS: i32 = 67108864;
pub const EXON_HIP_REGION_DEPTH_MAX_THRESHOLDS: i32 = 8;
/// exon_hip_cigar_blocks' cover_ops: bit i = BAM op code i is covered (M = X; + D)
pub const EXON_HIP_COVER_ALIGNED: u32 = 0x181;
pub const EXON_HIP_COVER_ALIGNED_DEL: u32 = 0x185;
pub const EXON_HIP_GT: i32 = 0;
pub const EXON_HIP_GE: i32 = 1;
pub const EXON_HIP_LT: i32 = 2;
pub const EXON_HIP_LE: i32 = 3;
pub const EXON_HIP_ECAPACITY: i32 = -6; // more distinct group keys than the plan's n_groups; the stream is unchanged
pub const EXON_HIP_EQ: i32 = 4;
pub const EXON_HIP_NE: i32 = 5;
pub const EXON_HIP_FORMAT_VCF: i32 = 1;
pub const EXON_HIP_FORMAT_BAM: i32 = 2;
pub const EXON_HIP_FORMAT_FASTQ: i32 = 3;
pub const EXON_HIP_FORMAT_SAM: i32 = 5;
pub const EXON_HIP_FORMAT_BCF: i32 = 6;
pub const EXON_HIP_FORMAT_CRAM: i32 = 7;
pub const EXON_HIP_FORMAT_GFF: i32 = 8;
pub const EXON_HIP_FORMAT_GTF: i32 = 9;
pub const EXON_HIP_FORMAT_BED: i32 = 10;
// exon_hip_scan_options.projection of a BED scan: bit k = column k of the reference's schema (n_fields = k: bits 3 .. k - 1)
pub const EXON_HIP_PROJECT_BED_NAME: u64 = 1 << 3;
pub const EXON_HIP_PROJECT_BED_SCORE: u64 = 1 << 4;
pub const EXON_HIP_PROJECT_BED_STRAND: u64 = 1 << 5;
pub const EXON_HIP_PROJECT_BED_THICK_START: u64 = 1 << 6;
pub const EXON_HIP_PROJECT_BED_THICK_END: u64 = 1 << 7;
pub const EXON_HIP_PROJECT_BED_COLOR: u64 = 1 << 8;
pub const EXON_HIP_PROJECT_BED_BLOCK_COUNT: u64 = 1 << 9;
pub const EXON_HIP_PROJECT_BED_BLOCK_SIZES: u64 = 1 << 10;
pub const EXON_HIP_PROJECT_BED_BLOCK_STARTS: u64 = 1 << 11;
pub const EXON_HIP_PROJECT_GTF_ATTRIBUTES: u64 = 256; // exon_hip_scan_options.projection: GTF column 8, Map<Utf8, Utf8>
pub const EXON_HIP_PROJECT_GFF_ATTRIBUTES: u64 = 256; // exon_hip_scan_options.projection: GFF column 8, Map<Utf8, List<Utf8>>
// exon_hip_scan_options.projection of a VCF scan: the reference's unparsed Utf8 columns (the parsed entries printed again)
pub const EXON_HIP_PROJECT_VCF_INFO: u64 = 8; // from the host reader and, printed on the device, from the GPU pipeline
pub const EXON_HIP_PROJECT_VCF_FORMATS: u64 = 16; // host reader; the GPU pipeline only with the modifier below
pub const EXON_HIP_PROJECT_VCF_FORMATS_ON_DEVICE: u64 = 32; // a modifier, not a column: with bit 16, `formats` is printed on the device
pub const EXON_HIP_COMPRESSION_AUTO: i32 = 0;
pub const EXON_HIP_MAX_GROUPS: i32 = 4096;
pub const EXON_HIP_REGION_OPEN_END: i64 = i64::MAX;

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct exon_hip_plan_desc {
    pub kind: i32,
    pub n_groups: i32,
    pub region_chrom_id: i32,
    pub x_type: i32,
    pub region_start: i64,
    pub region_end: i64,
    pub flag_mask: i32,
    pub flag_value: i32,
    pub mapq_min: i32,
    pub cmp_op: i32,
    pub threshold: f64,
    pub lmax: i32,
    pub y_type: i32,
    pub columns: [i32; 4],
}

/// mirrors `exon_hip_scan_options`
#[repr(C)]
pub struct exon_hip_scan_options {
    pub format: i32,
    pub compression: i32,
    pub batch_size: i64,
    pub info_field: *const c_char,
    pub region: *const c_char,
    pub use_index: i32,
    pub gpu_parse: i32,
    pub projection: u64, // EXON_HIP_PROJECT_* (ABI 5): columns beyond the fused kernels' operands; 0 on the aggregate path
}

/// mirrors `exon_hip_column` (an Arrow array already resident in HBM)
#[repr(C)]
pub struct exon_hip_column {
    pub values: *const c_void,
    pub validity: *const u8,
    pub offsets: *const i32,
    pub length: i64,
}

/// mirrors `exon_hip_device_info`
#[repr(C)]
pub struct exon_hip_device_info {
    pub name: [c_char; 64],
    pub gcn_arch: [c_char; 32],
    pub compute_units: i32,
    pub wavefront_size: i32,
    pub hbm_bytes: i64,
    pub clock_khz: i32,
    pub reserved: i32,
}

extern "C" {
    pub fn exon_hip_abi_version() -> c_int;
    /// the `formats` Utf8 column printed on the device: the ##FORMAT lines' value types (kinds i f c s), then the column of the last parsed slab
    pub fn exon_hip_vcf_parser_set_format_key_types(parser: *mut exon_hip_vcf_parser, packed_keys: *const c_char, kinds: *const c_char, n: i32) -> c_int;
    pub fn exon_hip_vcf_parser_formats_text(parser: *mut exon_hip_vcf_parser, stream: *mut c_void, out: *mut exon_hip_vcf_info_text) -> c_int;
    pub fn exon_hip_ctx_create(device: c_int, out: *mut *mut exon_hip_ctx) -> c_int;
    pub fn exon_hip_ctx_destroy(ctx: *mut exon_hip_ctx) -> c_int;
    pub fn exon_hip_ctx_info(ctx: *mut exon_hip_ctx, out: *mut exon_hip_device_info) -> c_int;
    pub fn exon_hip_last_error(ctx: *const exon_hip_ctx) -> *const c_char;
    pub fn exon_hip_plan_create(ctx: *mut exon_hip_ctx, desc: *const exon_hip_plan_desc, out: *mut *mut exon_hip_plan) -> c_int;
    pub fn exon_hip_plan_destroy(plan: *mut exon_hip_plan) -> c_int;
    pub fn exon_hip_plan_state_size(plan: *const exon_hip_plan, n_i64: *mut i64, n_f64: *mut i64) -> c_int;
    /// K8 (bare operator, Float32 x / y): accumulates into d_state = [count_y[G]] [count_rows[G]] [minw[G]] [maxw[G]]
    pub fn exon_hip_cmp_minmax_by_group(ctx: *mut exon_hip_ctx, stream: *mut c_void, x: *const exon_hip_column, y: *const exon_hip_column, group_id: *const exon_hip_column, n: i64, threshold: f64, cmp_op: i32, n_groups: i32, d_state: *mut i64) -> c_int;
    /// host-only: words of K8's min (is_min != 0) or max plane -> 4-byte values + validity bytes (a word of 0 = no value)
    pub fn exon_hip_minmax_decode(words: *const i64, n: i64, is_min: i32, y_type: i32, out_values: *mut c_void, out_valid: *mut u8) -> c_int;
    /// K9 (bare operator): per-read length / GC percent / mean quality histograms + four totals over two Utf8 columns; accumulates
    pub fn exon_hip_read_stats_hist(ctx: *mut exon_hip_ctx, stream: *mut c_void, sequence: *const exon_hip_column, quality: *const exon_hip_column, n_reads: i64, lmax: i32, d_state: *mut i64) -> c_int;
    /// K9 over views of both lines into text resident in HBM
    pub fn exon_hip_read_stats_hist_views(ctx: *mut exon_hip_ctx, stream: *mut c_void, d_bytes: *const u8, seq_s: *const i32, seq_e: *const i32, qual_s: *const i32, qual_e: *const i32, n_reads: i64, lmax: i32, d_state: *mut i64) -> c_int;
    /// host-only: word offsets of K9's totals / length / gc_percent / mean_quality sections and the state's size
    pub fn exon_hip_read_stats_layout(lmax: i32, out: *mut i64) -> c_int;
    /// K10 (bare operator): per-record totals, byte composition, length / log2 length / GC percent histograms over one Utf8 column; accumulates
    pub fn exon_hip_seq_stats_hist(ctx: *mut exon_hip_ctx, stream: *mut c_void, sequence: *const exon_hip_column, n_records: i64, lmax: i32, d_state: *mut i64) -> c_int;
    /// K10 over the views of one FASTA slab resident in HBM (exon_hip_fasta_parser_parse)
    pub fn exon_hip_seq_stats_hist_views(ctx: *mut exon_hip_ctx, stream: *mut c_void, views: *const exon_hip_fasta_views, lmax: i32, d_state: *mut i64) -> c_int;
    /// host-only: word offsets of K10's totals / composition / length / length_log2 / gc_percent sections and the state's size
    pub fn exon_hip_seq_stats_layout(lmax: i32, out: *mut i64) -> c_int;
    /// K11: the plan of a whole region set (ids form: `packed_contig_names` null; names form: n_regions NUL-terminated names, resolved per consumed scan)
    pub fn exon_hip_plan_create_region_set(ctx: *mut exon_hip_ctx, columns: *const i32, packed_contig_names: *const c_char, packed_bytes: usize, ref_ids: *const i32, starts: *const i64, ends: *const i64, n_regions: i32, out: *mut *mut exon_hip_plan) -> c_int;
    /// host-only: word offsets of K11's totals / A / B sections and the state's size
    pub fn exon_hip_region_set_layout(plan: *const exon_hip_plan, out: *mut i64) -> c_int;
    /// host-only: K11's state words -> one count per region, in the caller's order; linear in the state
    pub fn exon_hip_region_set_decode(plan: *const exon_hip_plan, state: *const i64, out_counts: *mut i64) -> c_int;
    /// K11 (bare operator, ids form): overlap counts of every region of the plan's set over one batch; accumulates
    pub fn exon_hip_region_set_overlap(ctx: *mut exon_hip_ctx, stream: *mut c_void, ref_id: *const exon_hip_column, start: *const exon_hip_column, end: *const exon_hip_column, n: i64, plan: *const exon_hip_plan, d_state: *mut i64) -> c_int;
    /// K12: the plan of the covered bases of every region of a set; exon_hip_plan_create_region_set's arguments and rules
    pub fn exon_hip_plan_create_region_set_bases(ctx: *mut exon_hip_ctx, columns: *const i32, packed_contig_names: *const c_char, packed_bytes: usize, ref_ids: *const i32, starts: *const i64, ends: *const i64, n_regions: i32, out: *mut *mut exon_hip_plan) -> c_int;
    /// host-only: word offsets of K12's totals / Ns / Ss / Ne / Se sections and the state's size (out[6])
    pub fn exon_hip_region_bases_layout(plan: *const exon_hip_plan, out: *mut i64) -> c_int;
    /// host-only: K12's state words -> the covered bases of every region, in the caller's order; linear in the state modulo 2^64
    pub fn exon_hip_region_bases_decode(plan: *const exon_hip_plan, state: *const i64, out_bases: *mut i64) -> c_int;
    /// K12 (bare operator, ids form): covered bases of every region of the plan's set over one batch; accumulates
    pub fn exon_hip_region_set_bases(ctx: *mut exon_hip_ctx, stream: *mut c_void, ref_id: *const exon_hip_column, start: *const exon_hip_column, end: *const exon_hip_column, n: i64, plan: *const exon_hip_plan, d_state: *mut i64) -> c_int;
    /// K13: the plan of the bases per window of width `window` along each contig; contigs by id or by name as kind 11's, each once
    pub fn exon_hip_plan_create_window_bases(ctx: *mut exon_hip_ctx, columns: *const i32, packed_contig_names: *const c_char, packed_bytes: usize, ref_ids: *const i32, lengths: *const i64, n_contigs: i32, window: i64, out: *mut *mut exon_hip_plan) -> c_int;
    /// host-only: word offsets of K13's totals / E / D sections and the state's size (out[4])
    pub fn exon_hip_window_bases_layout(plan: *const exon_hip_plan, out: *mut i64) -> c_int;
    /// host-only: the windows in front of each contig, then their total B (woff[C + 1])
    pub fn exon_hip_window_bases_offsets(plan: *const exon_hip_plan, woff: *mut i64) -> c_int;
    /// host-only: K13's state words -> the bases of every window, contig by contig; linear in the state modulo 2^64
    pub fn exon_hip_window_bases_decode(plan: *const exon_hip_plan, state: *const i64, out_bases: *mut i64) -> c_int;
    /// K13 (bare operator, ids form): bases per window over one batch; accumulates
    pub fn exon_hip_window_bases(ctx: *mut exon_hip_ctx, stream: *mut c_void, ref_id: *const exon_hip_column, start: *const exon_hip_column, end: *const exon_hip_column, n: i64, plan: *const exon_hip_plan, d_state: *mut i64) -> c_int;
    /// K14: the plan of the per-base depth over a region set; regions as kind 11's with finite ends, up to 8 strictly increasing thresholds
    pub fn exon_hip_plan_create_region_set_depth(ctx: *mut exon_hip_ctx, columns: *const i32, packed_contig_names: *const c_char, packed_bytes: usize, ref_ids: *const i32, starts: *const i64, ends: *const i64, n_regions: i32, thresholds: *const i64, n_thresholds: i32, out: *mut *mut exon_hip_plan) -> c_int;
    /// host-only: word offsets of K14's totals and D and the state's size (out[3])
    pub fn exon_hip_region_depth_layout(plan: *const exon_hip_plan, out: *mut i64) -> c_int;
    /// host-only: the merged intervals in bin order (*n of them; any array may be NULL)
    pub fn exon_hip_region_depth_intervals(plan: *const exon_hip_plan, n: *mut i32, slot: *mut i32, start: *mut i64, end: *mut i64, bin: *mut i64) -> c_int;
    /// host-only: K14's state words -> the depth of every target base in bin order (out_depth[T])
    pub fn exon_hip_region_depth_per_base(plan: *const exon_hip_plan, state: *const i64, out_depth: *mut i64) -> c_int;
    /// host-only: K14's state words -> [M][1 + k] bases and threshold counts per region; not linear in the state
    pub fn exon_hip_region_depth_decode(plan: *const exon_hip_plan, state: *const i64, out: *mut i64) -> c_int;
    /// the same table made on the device on the caller's stream; d_state is only read
    pub fn exon_hip_region_depth_reduce(ctx: *mut exon_hip_ctx, stream: *mut c_void, plan: *const exon_hip_plan, d_state: *const i64, d_out: *mut i64) -> c_int;
    /// K14 (bare operator, ids form): per-base depth over the set's bases for one batch; accumulates
    pub fn exon_hip_region_set_depth(ctx: *mut exon_hip_ctx, stream: *mut c_void, ref_id: *const exon_hip_column, start: *const exon_hip_column, end: *const exon_hip_column, n: i64, plan: *const exon_hip_plan, d_state: *mut i64) -> c_int;
    /// alignment rows + a List<UInt32> of CIGAR ops on the device -> their aligned blocks as interval rows for kinds 12 - 14; synchronous
    pub fn exon_hip_cigar_blocks(ctx: *mut exon_hip_ctx, stream: *mut c_void, ref_id: *const exon_hip_column, start: *const exon_hip_column, d_cigar_offsets: *const i32, d_cigar_ops: *const u32, n: i64, cover_ops: u32, d_out_ref: *mut i32, d_out_start: *mut i64, d_out_end: *mut i64, d_out_valid: *mut u8, cap: i64, n_blocks: *mut i64) -> c_int;
    /// host-only: the aligned blocks of one record's ops (len << 4 | code)
    pub fn exon_hip_cigar_blocks_host(ops: *const u32, n_ops: i32, start: i64, cover_ops: u32, out_start: *mut i64, out_end: *mut i64, cap: i32, n_blocks: *mut i32) -> c_int;
    /// the reference lengths of a BAM / SAM / CRAM header in dictionary-id order: *n of them, the first min(*n, cap) into out
    pub fn exon_hip_scan_reference_lengths(scan: *mut exon_hip_scan, out: *mut i64, cap: i32, n: *mut i32) -> c_int;
    /// fold of `world` packed states by the plan's own layout (add; unsigned max for K8's extreme planes)
    pub fn exon_hip_plan_fold_states(plan: *const exon_hip_plan, stream: *mut c_void, d_gathered: *const c_void, world: i32, d_out: *mut c_void) -> c_int;
    pub fn exon_hip_stream_open(plan: *mut exon_hip_plan, partition: i32, out: *mut *mut exon_hip_stream) -> c_int;
    /// moves `batch` (the library calls batch.release exactly once, success or not)
    pub fn exon_hip_stream_push(s: *mut exon_hip_stream, batch: *mut FFI_ArrowArray) -> c_int;
    pub fn exon_hip_stream_reset(s: *mut exon_hip_stream) -> c_int;
    pub fn exon_hip_stream_state(s: *mut exon_hip_stream, d_i64: *mut *mut i64, d_f64: *mut *mut f64, hip_stream: *mut *mut c_void) -> c_int;
    /// AggregateExec(Final) across GPUs: one ncclAllGather of the packed state + a fold in rank order (comm: ncclComm_t)
    pub fn exon_hip_stream_all_reduce(s: *mut exon_hip_stream, rccl_comm: *mut c_void) -> c_int;
    // ---- group keys by VALUE (ABI 4): FILTER-list / reference ids are per file; the stream remembers the value behind every
    // state index, re-keys each further scan into its own order, and the ranks agree on one dictionary before the merge
    pub fn exon_hip_stream_keys(s: *mut exon_hip_stream, buf: *mut c_char, cap: usize, n_keys: *mut i32, bytes: *mut usize, agreed: *mut i32) -> c_int;
    pub fn exon_hip_stream_set_keys(s: *mut exon_hip_stream, packed_names: *const c_char, packed_bytes: usize, n_keys: i32) -> c_int;
    pub fn exon_hip_keys_union(packed: *const c_char, packed_bytes: usize, n_keys: *const i32, world: i32, out: *mut c_char, cap: usize, n_out: *mut i32, out_bytes: *mut usize, maps: *mut i32) -> c_int;
    /// collective over the communicator: two small ncclAllGathers move the dictionaries, every rank permutes its state into the union
    pub fn exon_hip_stream_reconcile_keys(s: *mut exon_hip_stream, rccl_comm: *mut c_void) -> c_int;
    /// region plans over files: the contig travels by name, each file resolves it in its own header order
    pub fn exon_hip_stream_set_region_contig(s: *mut exon_hip_stream, name: *const c_char) -> c_int;
    pub fn exon_hip_stream_finish_arrow(s: *mut exon_hip_stream, out: *mut FFI_ArrowArray, out_schema: *mut FFI_ArrowSchema) -> c_int;
    pub fn exon_hip_stream_close(s: *mut exon_hip_stream) -> c_int;
    pub fn exon_hip_rccl_unique_id(id128: *mut u8) -> c_int;
    pub fn exon_hip_rccl_comm_init(ctx: *mut exon_hip_ctx, id128: *const u8, world: i32, rank: i32, comm: *mut *mut c_void) -> c_int;
    pub fn exon_hip_rccl_comm_destroy(comm: *mut c_void) -> c_int;
    pub fn exon_hip_rccl_comm_count(comm: *mut c_void, world: *mut i32, rank: *mut i32) -> c_int;
    pub fn exon_hip_parse_region(region: *const c_char, name_out: *mut c_char, name_cap: usize, start: *mut i64, end: *mut i64) -> c_int;
    pub fn exon_hip_regroup_files_by_size(sizes: *const i64, n_files: i32, target_groups: i32, group_of: *mut i32) -> c_int;

    // ---- whole-partition path: the library opens the file itself (native decoders; with gpu_parse = 1 the file's bytes go
    // to HBM as they are -- BGZF blocks are inflated and VCF / BCF / BAM / SAM / FASTQ records decoded on the GPU) ----
    pub fn exon_hip_scan_open(path: *const c_char, options: *const exon_hip_scan_options, out: *mut *mut exon_hip_scan) -> c_int;
    pub fn exon_hip_scan_dictionary_size(scan: *mut exon_hip_scan, column: i32, size: *mut i32) -> c_int;
    pub fn exon_hip_scan_dictionary_intern(scan: *mut exon_hip_scan, column: i32, name: *const c_char, id: *mut i32) -> c_int;
    pub fn exon_hip_scan_dictionary_value(scan: *mut exon_hip_scan, column: i32, id: i32, name: *mut *const c_char) -> c_int;
    pub fn exon_hip_scan_decoded_on_gpu(scan: *mut exon_hip_scan, decoded: *mut i32, inflated: *mut i32) -> c_int;
    pub fn exon_hip_scan_rows(scan: *mut exon_hip_scan, rows_emitted: *mut i64) -> c_int;
    pub fn exon_hip_scan_bind_ctx(scan: *mut exon_hip_scan, ctx: *mut exon_hip_ctx) -> c_int;
    /// one pushed-down comparison on a Float32 / Int32 value column of a VCF scan (EXON_HIP_GT .. EXON_HIP_NE), evaluated by the scan
    /// itself and ANDed with its region; call right after exon_hip_scan_open
    pub fn exon_hip_scan_set_predicate(scan: *mut exon_hip_scan, column: i32, cmp_op: i32, literal: f64) -> c_int;
    /// the flag / mapping-quality predicate of a BAM or SAM scan, evaluated by the scan itself and ANDed with its region: a row is emitted
    /// iff (flag & flag_mask) == flag_value and (mapq_min < 0 or mapping_quality is valid and >= mapq_min); call right after exon_hip_scan_open
    pub fn exon_hip_scan_set_flag_predicate(scan: *mut exon_hip_scan, flag_mask: i32, flag_value: i32, mapq_min: i32) -> c_int;
    /// blocks mode of a BAM / SAM scan: kinds 12 - 14 get every kept record as its aligned blocks (0 turns it off); call right after exon_hip_scan_open
    pub fn exon_hip_scan_set_cover_ops(scan: *mut exon_hip_scan, cover_ops: u32) -> c_int;
    /// after the scan has ended: slabs the GPU pipeline exported, how many went through the device take-rows step, bytes copied back
    pub fn exon_hip_scan_export_stats(scan: *mut exon_hip_scan, slabs: *mut i64, compacted_slabs: *mut i64, d2h_bytes: *mut i64) -> c_int;
    pub fn exon_hip_scan_close(scan: *mut exon_hip_scan) -> c_int;
    /// GpuFilterAggExec::execute for one file in one call
    pub fn exon_hip_stream_consume_scan(s: *mut exon_hip_stream, scan: *mut exon_hip_scan, rows: *mut i64) -> c_int;
}
