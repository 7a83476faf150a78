// k4_route.h -- which way one launch of cmp_avg_by_group (K4) takes: launch shape, tiers, and the form of tier 3 (ids beyond
// the registers + the LDS table).  Plain host arithmetic without HIP types: kernels.hip (k4_one_launch, k4_tail_records) decides
// with it, tests/k4_route_harness.cpp prints it, tests/k4_route.py states it again in Python.  The constants the device code
// shares with this decision live here and nowhere else.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace exon {

// rows per workgroup and iteration of the three launch shapes (kernels.hip: ShapeOf<ShapeBig / ShapeBigJ2 / ShapeSmall>::TILE)
constexpr int K4_TILE_BIG_J4 = 16384;  // 1024 threads, J = 4: 1 .. 4 groups
constexpr int K4_TILE_BIG = 8192;      // 1024 threads, J = 2: 5 and more groups
constexpr int K4_TILE_SMALL = 2048;    // 256 threads, J = 2

constexpr int K4_SLOTS_MIN_G = 5;                  // from here on the register groups keep their sums in lane-private LDS slots (J = 2)
constexpr int K4_OVF_REGS = 4;                     // register groups of the > 8-group variant
constexpr int K4_LDS_GROUPS = K4_OVF_REGS + 4096;  // ids handled by registers + the LDS table
constexpr int K4_TAIL_MAX_RANGES = 2048;  // (2^24 - 4100) / 8192 ids
constexpr int K4_TAIL_MAX_GRID = 2048;    // workgroups of the main kernel the partitioned tier 3 has histogram rows for
constexpr int K4_TAIL_RANGE = 8192;  // ids per range of the partitioned tier 3 = entries of k4_tail_aggregate's LDS table (128 KiB)
constexpr int K4_CHUNK = 2048;        // records per chunk (16 KiB): two per thread of k4_tail_aggregate_chunks
constexpr int K4_POS_BITS = 13;       // position field of a cursor: K4_CHUNK + 1024 lanes' failed draws < 8192
constexpr int K4_DIRECT_MAX_RANGES = 128;
// rows per launch of the partitioned tier 3: its scratch is 2 x 8 bytes per row of a launch, so a longer table is cut
// into launches of this many rows (a multiple of every tile size and of 8: column and bitmap pointers stay aligned)
constexpr int64_t K4_TAIL_CHUNK_ROWS = int64_t(1) << 28;
constexpr int64_t K4_TAIL_SLACK = 2048 * 2048;  // grid x tile of the largest launch shape: rounding of the per-workgroup regions

constexpr int k4_nl(int n_groups) { return n_groups < K4_LDS_GROUPS ? n_groups : K4_LDS_GROUPS; }
// The main kernel counts its tier-3 records per id range in LDS.  With few ranges the 64 lanes of a wave instruction land on
// a handful of counters and same-address LDS atomics serialise, so every range gets 2^k counters picked by lane (summed when
// the workgroup stores its row of the histogram); k shrinks as the ranges grow: at most 3072 counters = 12 KiB behind the
// tier-2 table, which keeps two workgroups on a CU.
constexpr int k4_hist_copies_log2(int n_ranges) {
  return n_ranges <= 192 ? 4 : n_ranges <= 384 ? 3 : n_ranges <= 768 ? 2 : n_ranges <= 1536 ? 1 : 0;
}
constexpr int k4_stream_copies_log2(int n_ranges) {
  return n_ranges == 1 ? 2 : 0;  // measured (profiles/r6_groupby_direct.md): the main kernel slows down with the streams a wave store spreads over
}
// 8-byte records of tier-3 scratch a launch over n rows wants (0: no tier 3); per buffer
constexpr size_t k4_tail_records_for(int64_t n, int n_groups) {
  return n_groups <= K4_LDS_GROUPS ? 0 : (size_t)((n < K4_TAIL_CHUNK_ROWS ? n : K4_TAIL_CHUNK_ROWS) + K4_TAIL_SLACK);
}

enum K4Form {
  K4_FORM_NONE = 0,     // no tier 3: every id sits in the registers or the LDS table
  K4_FORM_ATOMIC = 1,   // global atomics straight into the caller's state
  K4_FORM_SCATTER = 2,  // per-workgroup regions + LDS histogram, then wg_scan -> offsets -> scatter -> aggregate
  K4_FORM_DIRECT = 3,   // per-stream chunks written by the main kernel, then offsets -> aggregate_chunks
};

struct K4RouteIn {
  int compute_units;
  int blocks_per_cu;
  int64_t n;             // rows of this launch (<= K4_TAIL_CHUNK_ROWS when the plan has a tier 3)
  int n_groups;
  size_t tail_capacity;  // records per buffer of the tier-3 scratch (0: none)
  bool one_allocation;   // the second record buffer starts where the first one ends
  bool has_u32;          // the block of u32 counters exists
};

struct K4Route {
  bool big;           // the 1024-thread shape
  int64_t tile_rows;  // rows per workgroup and iteration
  int nl;             // ids of tiers 1 + 2
  bool has_tail;      // n_groups > nl
  int n_ranges;       // id ranges of tier 3 (0 without one)
  size_t n_streams;   // cursors per workgroup of the direct form: n_ranges << copies_log2
  int copies_log2;
  int hist_copies_log2;
  size_t pool_chunks;  // chunks of all workgroups of the direct form, at most
  size_t cpw_max;      // chunks of one workgroup, at most
  K4Form form;         // of the tile loop; the rows behind the last whole tile always take the atomic form
};

inline K4Route k4_route(const K4RouteIn& in) {
  K4Route r{};
  const int64_t n = in.n, cu = in.compute_units;
  const int64_t max_grid = cu * (in.blocks_per_cu > 1 ? in.blocks_per_cu : 1);
  r.nl = k4_nl(in.n_groups);
  r.has_tail = in.n_groups > r.nl;
  // With register groups (1 .. 4 groups) K4 keeps the 16384-row tile whenever every CU gets one: measured on MI355X at 1e7 rows
  // J = 4 27.8 us, J = 2 31.5 us (its per-tile bookkeeping -- counter spills, 15-value reductions -- outweighs the better tile
  // balance that pays for K2).  With the sums in lane-private LDS slots (5 .. 8 groups) the choice was run again and J = 2 wins:
  // 5 groups, 1e9 rows 1.86 - 1.91 ms against 1.92 - 1.96 at J = 4, 125e6 rows 0.238 - 0.252 against 0.257, 1e7 rows
  // 29.5 - 30.5 us against 31.1 (profiles/k4_lane_slots.md); the threshold -- a 16384-row tile per CU -- stays.
  r.big = n / K4_TILE_BIG_J4 >= cu && n / K4_TILE_BIG >= (cu > 1 ? cu : 1);
  r.tile_rows = r.big ? (in.n_groups < K4_SLOTS_MIN_G ? K4_TILE_BIG_J4 : K4_TILE_BIG) : K4_TILE_SMALL;
  r.n_ranges = r.has_tail ? (in.n_groups - r.nl + K4_TAIL_RANGE - 1) / K4_TAIL_RANGE : 0;
  r.copies_log2 = k4_stream_copies_log2(r.n_ranges);
  r.hist_copies_log2 = k4_hist_copies_log2(r.n_ranges);
  r.n_streams = (size_t)r.n_ranges << r.copies_log2;
  // partitioned tier 3 when its scratch is there (sized with k4_tail_records_for)
  const bool partition = r.has_tail && in.tail_capacity > 0 && in.has_u32 && in.tail_capacity >= (size_t)(n + K4_TAIL_SLACK) &&
                         r.n_ranges <= K4_TAIL_MAX_RANGES && max_grid <= K4_TAIL_MAX_GRID;
  // the direct partition when the chunk pool + the chunk lists fit the two record buffers (one allocation);
  // chunks of all workgroups, at most: their rows (rounded up to tiles per workgroup) + one per stream and workgroup
  const int64_t grid_ub = r.big ? cu : (max_grid < n / r.tile_rows + 1 ? max_grid : n / r.tile_rows + 1);  // the grid's bounds
  r.pool_chunks = (size_t)(n + grid_ub * r.tile_rows) / K4_CHUNK + (size_t)grid_ub * r.n_streams;
  const int64_t tiles_all = n / r.tile_rows, g0 = tiles_all < cu ? tiles_all : cu, grid_min = g0 > 1 ? g0 : 1;
  r.cpw_max = (size_t)((tiles_all + grid_min - 1) / grid_min) * r.tile_rows / K4_CHUNK + r.n_streams;
  const bool direct = partition && r.n_ranges <= K4_DIRECT_MAX_RANGES && in.one_allocation &&
                      r.pool_chunks * K4_CHUNK + (size_t)r.n_ranges * r.pool_chunks <= 2 * in.tail_capacity &&
                      r.cpw_max < 65536;  // chunk numbers inside a workgroup are 16-bit
  r.form = !r.has_tail ? K4_FORM_NONE : direct ? K4_FORM_DIRECT : partition ? K4_FORM_SCATTER : K4_FORM_ATOMIC;
  return r;
}

}  // namespace exon
