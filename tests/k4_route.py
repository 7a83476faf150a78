"""The route one launch of cmp_avg_by_group (K4) takes, stated again in Python: exon_amd/csrc/host/k4_route.h word for word
(tests/test_k4_route.py holds the two against each other), plus the rule by which the tier-3 scratch of a stream's workspace
grows (capi.cpp, ensure_tail_scratch).  The GPU tests ask this mirror which form of tier 3 a case takes and assert it before
they launch."""
from collections import namedtuple

TILE_BIG_J4, TILE_BIG, TILE_SMALL = 16384, 8192, 2048
SLOTS_MIN_G = 5
LDS_GROUPS = 4 + 4096
TAIL_MAX_RANGES = 2048
TAIL_MAX_GRID = 2048
TAIL_RANGE = 8192
CHUNK = 2048
DIRECT_MAX_RANGES = 128
TAIL_CHUNK_ROWS = 1 << 28
TAIL_SLACK = 2048 * 2048
FORMS = ("none", "atomic", "scatter", "direct")

Route = namedtuple("Route", "big tile_rows nl has_tail n_ranges n_streams copies_log2 hist_copies_log2 pool_chunks cpw_max form")
FIELDS = Route._fields


def hist_copies_log2(n_ranges):
    return 4 if n_ranges <= 192 else 3 if n_ranges <= 384 else 2 if n_ranges <= 768 else 1 if n_ranges <= 1536 else 0


def stream_copies_log2(n_ranges):
    return 2 if n_ranges == 1 else 0


def n_ranges_of(n_groups):
    return -(-(n_groups - LDS_GROUPS) // TAIL_RANGE) if n_groups > LDS_GROUPS else 0


def groups_of(n_ranges, last=TAIL_RANGE):
    """n_groups with `n_ranges` id ranges whose last one holds `last` ids"""
    return LDS_GROUPS + TAIL_RANGE * (n_ranges - 1) + last


def tail_records(n, n_groups):
    return 0 if n_groups <= LDS_GROUPS else min(n, TAIL_CHUNK_ROWS) + TAIL_SLACK


def route(compute_units, blocks_per_cu, n, n_groups, tail_capacity, one_allocation=True, has_u32=True):
    cu = compute_units
    max_grid = cu * max(blocks_per_cu, 1)
    nl = min(n_groups, LDS_GROUPS)
    has_tail = n_groups > nl
    big = n // TILE_BIG_J4 >= cu and n // TILE_BIG >= max(cu, 1)
    tile_rows = (TILE_BIG_J4 if n_groups < SLOTS_MIN_G else TILE_BIG) if big else TILE_SMALL
    n_ranges = n_ranges_of(n_groups)
    ccl, hcl = stream_copies_log2(n_ranges), hist_copies_log2(n_ranges)
    n_streams = n_ranges << ccl
    partition = (has_tail and tail_capacity > 0 and has_u32 and tail_capacity >= n + TAIL_SLACK and n_ranges <= TAIL_MAX_RANGES
                 and max_grid <= TAIL_MAX_GRID)
    grid_ub = cu if big else min(max_grid, n // tile_rows + 1)
    pool_chunks = (n + grid_ub * tile_rows) // CHUNK + grid_ub * n_streams
    tiles_all = n // tile_rows
    grid_min = max(1, min(tiles_all, cu))
    cpw_max = -(-tiles_all // grid_min) * tile_rows // CHUNK + n_streams
    direct = (partition and n_ranges <= DIRECT_MAX_RANGES and one_allocation
              and pool_chunks * CHUNK + n_ranges * pool_chunks <= 2 * tail_capacity and cpw_max < 65536)
    form = "none" if not has_tail else "direct" if direct else "scatter" if partition else "atomic"
    return Route(big, tile_rows, nl, has_tail, n_ranges, n_streams, ccl, hcl, pool_chunks, cpw_max, form)


class Scratch:
    """The tier-3 scratch of one stream's workspace as ensure_tail_scratch keeps it: grown to what a launch asks for when it is
    smaller, never shrunk; one allocation; the u32 block comes with the first tier-3 launch.  (Allocation failure is not
    modelled: the tests stay far below the device's memory.)"""

    def __init__(self, compute_units, blocks_per_cu=8):
        self.cu, self.bpc = compute_units, blocks_per_cu
        self.capacity = 0
        self.has_u32 = False

    def peek(self, n, n_groups):
        """the route a launch of (n, n_groups) would take now (n <= TAIL_CHUNK_ROWS), without recording it"""
        want = tail_records(n, n_groups)
        cap = max(self.capacity, want) if n > 0 else self.capacity
        u32 = self.has_u32 or (want > 0 and n > 0)
        return route(self.cu, self.bpc, n, n_groups, cap, True, u32)

    def launch(self, n, n_groups):
        """record the launch (a launch of no rows never reaches the scratch) and return its route"""
        r = self.peek(n, n_groups)
        if n > 0 and n_groups > LDS_GROUPS:
            self.capacity = max(self.capacity, tail_records(n, n_groups))
            self.has_u32 = True
        return r


def tile_loop_form(r, n):
    """what the rows of (n, route) really meet: the rows behind the last whole tile take global atomics whatever the form, so a
    launch without a whole tile is atomic throughout"""
    return "atomic" if r.has_tail and n < r.tile_rows else r.form
