// kernels.h -- launch interface of the gfx950 kernels (internal; the public surface is include/exon_hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace exon {

// Per-(ctx, stream) scratch: per-block partial words written by the main kernels and folded into the
// caller's state by finalize_partials in a fixed order (deterministic f64 sums, no atomics).
struct Workspace {
  unsigned long long* partials = nullptr;  // [blocks][words]
  size_t partial_capacity = 0;             // in 8-byte words
  int* status = nullptr;                   // device error word (K5: position >= lmax, bad group id)
  // K4 with more ids than registers + the LDS table hold (tier 3): two record buffers of `tail_capacity` 8-byte records
  // (compacted rows, then the same rows grouped by id range) and a block of counters; absent until such a plan runs
  uint2* tail_rec_a = nullptr;
  uint2* tail_rec_b = nullptr;
  size_t tail_capacity = 0;
  unsigned* tail_u32 = nullptr;
};

struct LaunchCfg {
  int compute_units = 256;
  int blocks_per_cu = 8;  // main-kernel grid = compute_units * blocks_per_cu (persistent, grid-stride)
  bool overwrite = false; // state := result of this launch (EXON_HIP_LAUNCH_OVERWRITE) instead of state += result
  bool x_is_int = false;  // K4: the compared column holds Int32 values (exon_hip_plan_desc.x_type), not Float32
  bool y_is_int = false;  // K4: AVG's argument holds Int32 values (exon_hip_plan_desc.y_type)
};

size_t k2_partial_words(const LaunchCfg&);
size_t k3_partial_words(const LaunchCfg&, int n_refs);
size_t k4_partial_words(const LaunchCfg&, int n_groups);
// 8-byte records of tier-3 scratch a K4 launch over n rows wants (0: no tier 3); per buffer
size_t k4_tail_records(int64_t n, int n_groups);
constexpr size_t K4_TAIL_U32_WORDS = 2048 + 3 * 2048 + 2 + (size_t)2048 * 2048;  // workgroup counts, range totals, offsets, slice starts, [workgroup][range] histogram
size_t k5_partial_words(const LaunchCfg&, int lmax);
size_t k8_partial_words(const LaunchCfg&, int n_groups);

hipError_t launch_region_count(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const int32_t* chrom,
                               const uint8_t* chrom_valid, const int64_t* pos, const uint8_t* pos_valid, int64_t n,
                               int32_t region_chrom, int64_t start, int64_t end, int64_t* d_count);

// K6: COUNT(*) of rows whose [start, end] interval on reference `region_ref` overlaps [region_start, region_end];
// strict: ... lies strictly inside (region_start, region_end) (start > a AND end < b: the BED / GFF form)
hipError_t launch_overlap_count(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const int32_t* ref,
                                const uint8_t* ref_valid, const int64_t* start, const uint8_t* start_valid,
                                const int64_t* end, const uint8_t* end_valid, int64_t n, int32_t region_ref,
                                int64_t region_start, int64_t region_end, int64_t* d_count, bool strict = false);

hipError_t launch_flag_mapq_group_count(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const int32_t* flag,
                                        const uint8_t* flag_valid, const uint8_t* mapq, const uint8_t* mapq_valid,
                                        const int32_t* ref_id, const uint8_t* ref_valid, int64_t n, int32_t flag_mask,
                                        int32_t flag_value, int32_t mapq_min, int32_t n_refs, int64_t* d_counts);

hipError_t launch_cmp_avg_by_group(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const float* x,
                                   const uint8_t* x_valid, const float* y, const uint8_t* y_valid, const int32_t* gid,
                                   int64_t n, double thr, int cmp_op, int n_groups, int64_t* d_counts, double* d_sums);

// K8: K4's predicate, MIN / MAX / COUNT(y) / COUNT(*) per group into the packed state [cnn[G]] [crow[G]] [minw[G]] [maxw[G]]
// (1 <= n_groups <= 4096; cfg.x_is_int / y_is_int as for K4)
hipError_t launch_cmp_minmax_by_group(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const float* x,
                                      const uint8_t* x_valid, const float* y, const uint8_t* y_valid, const int32_t* gid,
                                      int64_t n, double thr, int cmp_op, int n_groups, int64_t* d_state);

hipError_t launch_qual_pos_hist(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const int32_t* offsets,
                                const uint8_t* bytes, int64_t n_reads, int lmax, int64_t* d_hist);
// reads given as independent [starts[r], ends[r]) views into `bytes` (e.g. the quality lines of raw FASTQ text)
hipError_t launch_qual_pos_hist_views(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const int32_t* starts,
                                      const int32_t* ends, const uint8_t* bytes, int64_t n_reads, int lmax,
                                      int64_t* d_hist);

// a quality column held as several Arrow batches (chunks): ONE offsets scan, ONE main kernel (the workgroups' LDS
// histograms live across chunks), ONE finalize for up to K5_MAX_CHUNKS chunks.  Passed to the kernels by value.
constexpr int K5_MAX_CHUNKS = 64;
struct K5Chunks {
  const int32_t* off[K5_MAX_CHUNKS];
  const int32_t* ends[K5_MAX_CHUNKS];
  const uint8_t* bytes[K5_MAX_CHUNKS];
  int64_t n[K5_MAX_CHUNKS];
  int count;
};
// every chunk must have n > 0; 1 <= count <= K5_MAX_CHUNKS
hipError_t launch_qual_pos_hist_chunks(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const K5Chunks& ch, int lmax,
                                       int64_t* d_hist);

// K9: per-read length / GC percent / mean quality histograms + four totals over two sets of line views (an Arrow Utf8 column
// passes (offsets, offsets + 1)); state layout in include/exon_hip.h.  Length bins below K9_LEN_LDS are counted in LDS, the
// others by global atomics.  1 <= lmax <= 65536.  cfg.overwrite: state := this launch.  ws.status must be allocated.
constexpr int K9_LEN_LDS = 8192;
constexpr int64_t read_stats_words(int lmax) { return 4 + ((int64_t)lmax + 1) + 102 + 257; }
hipError_t launch_read_stats_hist(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const uint8_t* sbytes, const int32_t* ss,
                                  const int32_t* se, const uint8_t* qbytes, const int32_t* qs, const int32_t* qe, int64_t n_reads, int lmax,
                                  int64_t* d_state);

// K10 (seq_stats.hip): per-record FASTA statistics -- totals, byte composition, length, log2 length and GC percent histograms; state
// layout in include/exon_hip.h.  Work is divided by source bytes: tiles of SS_T bytes; workspace: one u32 per tile in ws.partials
// (seq_stats_partial_words() 8-byte words cover any int32-offset payload).  1 <= lmax <= 65536.  cfg.overwrite: state := this launch.
constexpr int SS_T = 16384;
constexpr int64_t SS_MAX_TILES = (((int64_t)1 << 31) + 16) / SS_T + 1;
constexpr int64_t seq_stats_words(int lmax) { return 3 + 256 + ((int64_t)lmax + 2) + 32 + 102; }
size_t seq_stats_partial_words();
// Arrow form: record r = values[offsets[r], offsets[r + 1]); no byte outside [offsets[0], offsets[n_records]) is loaded
hipError_t launch_seq_stats_hist(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const uint8_t* values, const int32_t* offsets,
                                 int64_t n_records, int lmax, int64_t* d_state);
// views form: the fields of an exon_hip_fasta_views; no byte outside [first_line_start, first_line_start + consumed_bytes) of
// text_base (16-byte aligned) is loaded
hipError_t launch_seq_stats_hist_views(hipStream_t s, const LaunchCfg& cfg, const Workspace& ws, const uint8_t* text_base, int64_t first_line_start,
                                       int64_t consumed_bytes, int64_t n_records, int64_t n_lines, int64_t seq_bytes, const int32_t* head_start,
                                       const int32_t* seq_offsets, const uint32_t* line_end, const uint32_t* line_dst, int lmax, int64_t* d_state);

// K11 (region_set.hip): K6's overlap count for every region of a set in one pass; state [counted, null_rows, elsewhere, inverted]
// [A: M + C] [B: M + C] (include/exon_hip.h, exon_hip_region_set_layout).  The tables live on the device: map[n_map] = contig slot of
// a reference id or -1, off[C + 1] = regions in front of each contig, ends / starts [M] sorted within each contig.  Sets with
// M + C <= REGION_SET_LDS_MAX keep the tables and a u32 histogram pair in LDS (24 bytes per word of the bound: 144 KiB of the CU's
// 160 at the bound); larger ones search through L2 and add to the state with global atomics.  The row walk is region_rows.h's (shared
// with K12): tiles of RS_TILE_BIG (1024 threads) once every CU gets one, else RS_TILE_SMALL (256 threads).  Column bases need their
// element's alignment only.  `ones`: 64 bytes of 0xFF on the device (Workspace::status + 8).  cfg.overwrite: state := this launch.
constexpr int RS_J = 2;
constexpr int RS_TILE_SMALL = 4 * 256 * RS_J, RS_TILE_BIG = 16 * 256 * RS_J;
constexpr int REGION_SET_LDS_MAX = 6144;
constexpr int REGION_SET_MAX_REGIONS = 1 << 20;
constexpr int64_t REGION_SET_LAUNCH_ROWS = (int64_t)1 << 31;  // rows per kernel launch: the LDS bins are u32
constexpr int64_t region_set_words(int64_t M, int64_t C) { return 4 + 2 * (M + C); }
constexpr size_t region_set_lds_bytes(int M, int C) { return (size_t)M * 16 + (size_t)(M + C) * 8; }
struct RegionSetTables {
  const int32_t* map;
  int32_t n_map;
  const int32_t* off;
  const int64_t* ends;
  const int64_t* starts;
  int32_t M, C;
};
hipError_t launch_region_set_overlap(hipStream_t s, const LaunchCfg& cfg, const uint8_t* ones, const int32_t* ref, const uint8_t* ref_valid,
                                     const int64_t* start, const uint8_t* start_valid, const int64_t* end, const uint8_t* end_valid, int64_t n,
                                     const RegionSetTables& t, int64_t* d_state);

// K12 (region_bases.hip): the bases of the rows that fall inside every region of a set, in one pass; state [counted, null_rows,
// elsewhere, inverted] [Ns: P + C] [Ss: P + C] [Ne: P + C] [Se: P + C], every word modulo 2^64 (include/exon_hip.h,
// exon_hip_region_bases_layout).  Device tables: map[n_map] as K11's, poff[C + 1] = points in front of each contig, points[P] sorted
// and unique within each contig.  The row walk (region_rows.h), the tiles (RS_TILE_SMALL / RS_TILE_BIG) and `ones` are K11's.
// REGION_BASES_LDS_MAX bounds P + C of the LDS tier.  One unit of P + C takes at most 8 B of point table (P <= P + C) and, per bin,
// u32 Ns + u32 Ne + u64 Ss + u64 Se = 24 B: 32 B, so 4096 units are 128 KiB of the CU's 160 KiB.  The largest power of two that
// fits (K11 likewise stops short of the 160 KiB a workgroup may ask for, at 144); a bound of 5119 (all of it, untried) would move the
// tier edge by a quarter only.  Larger sets search through L2 and add to the state with global 64-bit atomics.
constexpr int REGION_BASES_LDS_MAX = 4096;
constexpr int64_t region_bases_words(int64_t P, int64_t C) { return 4 + 4 * (P + C); }
constexpr size_t region_bases_lds_bytes(int P, int C) { return (size_t)P * 8 + (size_t)(P + C) * 24; }
struct RegionBasesTables {
  const int32_t* map;
  int32_t n_map;
  const int32_t* poff;
  const int64_t* points;
  int32_t P, C;
};
hipError_t launch_region_set_bases(hipStream_t s, const LaunchCfg& cfg, const uint8_t* ones, const int32_t* ref, const uint8_t* ref_valid,
                                   const int64_t* start, const uint8_t* start_valid, const int64_t* end, const uint8_t* end_valid, int64_t n,
                                   const RegionBasesTables& t, int64_t* d_state);

// K13 (window_bases.hip): the bases of the rows inside every fixed-width window along each contig, in one pass; state [counted,
// null_rows, elsewhere, inverted] [E: B] [D: B], every word modulo 2^64 (include/exon_hip.h, exon_hip_window_bases_layout).  Device
// tables: map[n_map] as K11's, woff[C + 1] = windows in front of each contig, len[C] = contig lengths.  The window of a clipped
// coordinate x is (x - 1) / W with x - 1 < 2^31: W (clamped to 2^31 - 1, which changes no quotient) travels with the reciprocal
// window_bases_reciprocal() makes, so the kernel multiplies and shifts.  Plans with B <= WINDOW_BASES_LDS_MAX keep E and D in LDS as
// u64, 16 B a bin: 128 KiB, the largest power of two under the 160 KiB a workgroup may take (K12's reasoning); D stays 64 bits wide
// there: a launch of 2^31 rows can leave a net of +2^31 or -2^31 in one bin, which 32 bits cannot tell apart.  Larger plans add to the
// state with global 64-bit atomics.  The row walk, the tiles and `ones` are K11's.  cfg.overwrite: state := this launch.
constexpr int WINDOW_BASES_LDS_MAX = 8192;
constexpr int64_t WINDOW_BASES_MAX_BINS = (int64_t)1 << 25;
constexpr int64_t window_bases_words(int64_t B) { return 4 + 2 * B; }
struct WindowBasesTables {
  const int32_t* map;
  int32_t n_map;
  const int32_t* woff;
  const int32_t* len;
  uint32_t W, mul, shift;  // floor(x / W) = (uint64_t)x * mul >> shift for every x < 2^31
  int32_t B, C;
};
// exact for 0 <= x < 2^31 and 1 <= W < 2^31 (Granlund & Montgomery 1994, N = 31): l = ceil(log2 W), mul = ceil(2^(31 + l) / W) < 2^32
inline void window_bases_reciprocal(uint32_t W, uint32_t* mul, uint32_t* shift) {
  uint32_t l = 0;
  while (((uint64_t)1 << l) < W) ++l;
  *shift = 31 + l;
  *mul = (uint32_t)((((uint64_t)1 << *shift) + W - 1) / W);
}
hipError_t launch_window_bases(hipStream_t s, const LaunchCfg& cfg, const uint8_t* ones, const int32_t* ref, const uint8_t* ref_valid,
                               const int64_t* start, const uint8_t* start_valid, const int64_t* end, const uint8_t* end_valid, int64_t n,
                               const WindowBasesTables& t, int64_t* d_state);

// K14 (region_depth.hip): the per-base depth over the bases a region set covers, in one pass; state [counted, null_rows, elsewhere,
// inverted] [D: T + C], every word modulo 2^64 (include/exon_hip.h, exon_hip_region_depth_layout).  Device tables: map[n_map] as K11's,
// ioff[C + 1] = merged intervals in front of each contig, doff[C] = first bin of each contig, ms[I] = interval starts ascending within
// a contig, cl[I] = { target bases of the contig in front of the interval, the interval's own }.  A counted row takes one
// count_below<true> per endpoint and adds +1 / -1 to two bins of D.  Plans with NB = T + C <= REGION_DEPTH_LDS_MAX keep the bins in
// LDS as u64 (64 KiB at the bound; 64 bits for K13's reason), and the interval table (16 B an interval) beside them when both fit
// REGION_DEPTH_LDS_MAX * 16 bytes = 128 KiB, K12's and K13's figure -- sets of one- and two-base targets have nearly an interval a
// bin and read the table through L2 instead.  Larger plans search through L2 and add to the state with global 64-bit atomics.  The
// row walk, the tiles and `ones` are K11's.  cfg.overwrite: state := this launch.
constexpr int REGION_DEPTH_LDS_MAX = 8192;
constexpr int64_t REGION_DEPTH_MAX_BINS = (int64_t)1 << 26;
constexpr int REGION_DEPTH_MAX_THRESHOLDS = 8;
constexpr int64_t region_depth_words(int64_t NB) { return 4 + NB; }
// 0: global atomics; 1: bins in LDS, table through L2; 2: bins and table in LDS
constexpr int region_depth_tier(int64_t NB, int64_t I) {
  return NB > REGION_DEPTH_LDS_MAX ? 0 : NB * 8 + I * 16 > (int64_t)REGION_DEPTH_LDS_MAX * 16 ? 1 : 2;
}
struct RegionDepthTables {
  const int32_t* map;
  int32_t n_map;
  const int32_t* ioff;
  const int32_t* doff;
  const int64_t* ms;
  const int2* cl;
  int32_t I, C, NB;
};
hipError_t launch_region_set_depth(hipStream_t s, const LaunchCfg& cfg, const uint8_t* ones, const int32_t* ref, const uint8_t* ref_valid,
                                   const int64_t* start, const uint8_t* start_valid, const int64_t* end, const uint8_t* end_valid, int64_t n,
                                   const RegionDepthTables& t, int64_t* d_state);
// K14's reduce: d_out[M][1 + k] = { bases_i, ge_t ... } from a state, word for word what host/region_depth.h's decode gives.  The
// running sum of D is taken over the whole section as one array, in tiles of REGION_DEPTH_REDUCE_TILE bins (a wave, 4 bins a lane):
// per-tile sums, one workgroup scans them, then one wave per piece (region x tile) rebuilds the tile's running sum from its offset and
// adds what the region's bins give to d_out.  pfx[M + 1] = pieces in front of each region (the plan's), lo / hi [M] = a region's bins.
// scratch: 2 * region_depth_reduce_tiles(NB) words.  d_state is only read.
constexpr int REGION_DEPTH_REDUCE_TILE = 256;
constexpr int64_t region_depth_reduce_tiles(int64_t NB) { return (NB + REGION_DEPTH_REDUCE_TILE - 1) / REGION_DEPTH_REDUCE_TILE; }
struct RegionDepthReduce {
  const int64_t* pfx;
  const int32_t* lo;
  const int32_t* hi;
  int64_t n_pieces;
  int32_t M, NB, k;
  int64_t thr[REGION_DEPTH_MAX_THRESHOLDS];
};
hipError_t launch_region_depth_reduce(hipStream_t s, const LaunchCfg& cfg, const RegionDepthReduce& r, const int64_t* d_state, unsigned long long* scratch,
                                      int64_t* d_out);

// pushed-down region filter as a row mask: out_valid = in_valid AND (row hits the region); *n_pass += rows kept.
// point form (VCF): id_col = chrom id, start = pos; range form (BAM): id_col = reference id, [start, end].
hipError_t launch_region_mask(hipStream_t s, bool range_form, const int32_t* id_col, const uint8_t* id_valid, const int64_t* start,
                              const int64_t* end, const uint8_t* pos_valid, const uint8_t* in_valid, int64_t n, int32_t id,
                              int64_t a, int64_t b, uint8_t* out_valid, unsigned long long* n_pass);

// pushed-down value predicate as a row mask: out_valid = in_valid AND region_mask AND (x valid AND x <cmp_op> literal, K4's rule;
// x_is_int: Int32 values compared exactly, else Float32 widened to Float64 in totalOrder); *n_pass += rows that pass the predicate
// and the region.  region_mask / in_valid may be null (all ones); region_mask may be out_valid.  hipErrorInvalidValue: cmp_op.
hipError_t launch_value_mask(hipStream_t s, const void* x, const uint8_t* x_valid, bool x_is_int, double literal, int cmp_op, const uint8_t* region_mask,
                             const uint8_t* in_valid, int64_t n, uint8_t* out_valid, unsigned long long* n_pass);

// pushed-down flag / mapping-quality predicate (BAM, SAM) as a row mask, launch_value_mask's contract: out_valid = in_valid AND
// region_mask AND (flag & flag_mask) == flag_value AND (mapq_min < 0 OR (mapq valid AND mapq >= mapq_min)); *n_pass += rows that pass
// the predicate and the region.  region_mask / in_valid / mapq_valid may be null (all ones); region_mask may be out_valid.
hipError_t launch_flag_mapq_mask(hipStream_t s, const int32_t* flag, const uint8_t* mapq, const uint8_t* mapq_valid, int32_t flag_mask, int32_t flag_value,
                                 int32_t mapq_min, const uint8_t* region_mask, const uint8_t* in_valid, int64_t n, uint8_t* out_valid, unsigned long long* n_pass);

// out[v] = sum over ranks (rank order) of gathered[rank][v]; words [0, n_i64) int64, then n_f64 float64; the last n_max of the
// int64 words fold by unsigned max instead (K8's extreme planes)
hipError_t launch_fold_states(hipStream_t s, const void* gathered, int world, int64_t n_i64, int64_t n_f64, void* out, int64_t n_max = 0);

// Re-keying of a packed partial state: dst[plane][map[g]] += src[plane][g] for every keyed plane (`planes_i64` int64 planes of G
// words, then `tail_i64` unkeyed int64 words that are added in place -- K3's NULL-reference group --, then `planes_f64` float64
// planes of G words; the last `planes_max` of the int64 planes are combined by unsigned max instead of add); map[g] < 0: key g
// carries nothing and is skipped.  Used when the dictionary ids of one scan / one rank
// are brought into the order of a shared key dictionary (merge by key VALUE, not by id).
hipError_t launch_permute_add_state(hipStream_t s, const void* src, void* dst, const int32_t* map, int n_map, int G, int planes_i64,
                                    int tail_i64, int planes_f64, int planes_max);

// bare streaming read of up to 4 buffers in lock-step, the access pattern and grid of K2-K6 (bench.py's per-box ceiling)
hipError_t launch_read_probe(hipStream_t s, const LaunchCfg& cfg, const void* const* buffers, int n_buffers, int64_t bytes_each,
                             unsigned* sink);

hipError_t launch_gen_c2(hipStream_t s, uint64_t seed, int64_t n_total, int64_t lo, int64_t hi, int32_t* chrom,
                         int64_t* pos);
hipError_t launch_gen_c3(hipStream_t s, uint64_t seed, int64_t lo, int64_t hi, int32_t* flag, uint8_t* mapq,
                         uint8_t* mapq_valid, int32_t* ref_id, uint8_t* ref_valid);
hipError_t launch_gen_c4(hipStream_t s, uint64_t seed, int64_t lo, int64_t hi, float* af, uint8_t* af_valid,
                         float* qual, uint8_t* qual_valid, int32_t* filter_id);
hipError_t launch_gen_c6(hipStream_t s, uint64_t seed, int64_t lo, int64_t hi, int32_t* ref_id, uint8_t* ref_valid,
                         int64_t* start, int64_t* end, uint8_t* pos_valid);
hipError_t launch_gen_c5(hipStream_t s, uint64_t seed, int64_t lo, int64_t hi, int32_t read_len, int32_t* offsets,
                         uint8_t* bytes);

}  // namespace exon
