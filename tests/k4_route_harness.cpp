// Stand-alone driver of exon_amd/csrc/host/k4_route.h for tests/test_k4_route.py: reads cases
//   compute_units blocks_per_cu n n_groups tail_capacity one_allocation has_u32
// one per line from the file named on the command line and prints, per case, the route k4_one_launch takes and the records
// k4_tail_records asks for.  The first line printed holds the constants.
#include <cinttypes>
#include <cstdio>

#include "host/k4_route.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  using namespace exon;
  printf("%d %d %d %d %d %d %d %d %d %" PRId64 " %" PRId64 "\n", K4_TILE_BIG_J4, K4_TILE_BIG, K4_TILE_SMALL, K4_SLOTS_MIN_G, K4_LDS_GROUPS,
         K4_TAIL_MAX_RANGES, K4_TAIL_MAX_GRID, K4_TAIL_RANGE, K4_CHUNK, (int64_t)K4_DIRECT_MAX_RANGES, K4_TAIL_CHUNK_ROWS);
  printf("%" PRId64 " %d\n", K4_TAIL_SLACK, 1 << K4_POS_BITS);
  int cu, bpc, G, one, u32;
  int64_t n;
  unsigned long long cap;
  while (fscanf(f, "%d %d %" SCNd64 " %d %llu %d %d", &cu, &bpc, &n, &G, &cap, &one, &u32) == 7) {
    const K4Route r = k4_route(K4RouteIn{cu, bpc, n, G, (size_t)cap, one != 0, u32 != 0});
    printf("%d %" PRId64 " %d %d %d %zu %d %d %zu %zu %d %zu\n", (int)r.big, r.tile_rows, r.nl, (int)r.has_tail, r.n_ranges, r.n_streams, r.copies_log2,
           r.hist_copies_log2, r.pool_chunks, r.cpw_max, (int)r.form, k4_tail_records_for(n, G));
  }
  fclose(f);
  return 0;
}
