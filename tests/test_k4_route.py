"""CPU: the host's choice of K4's launch shape and tier-3 form (exon_amd/csrc/host/k4_route.h, what k4_one_launch and
k4_tail_records call) in a stand-alone program (tests/k4_route_harness.cpp, plain g++ with AddressSanitizer and
UndefinedBehaviorSanitizer) against its Python statement tests/k4_route.py, field by field over a grid of cases: the GPU tests
of tests/test_gpu_k4_tiers.py rely on the Python one to know which device code a case runs."""
import os
import shutil
import subprocess

import pytest

import k4_route as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CUS = [1, 64, 256, 304]
BPC = [1, 8, 9]
NS = [0, 1, 2047, 2048, 2049, 8191, 8192, 300_001, 700_001, 64 * 8192 - 1, 64 * 16384 - 1, 64 * 16384, 256 * 8192, 256 * 16384 - 1, 256 * 16384,
      256 * 16384 + 3 * 8192 + 777, 304 * 16384 - 1, 304 * 16384, 304 * 16384 + 3 * 8192 + 777, 4_200_000, 100_000_000, (1 << 28) - 1, 1 << 28,
      (1 << 28) + 1, 300_000_000]
RANGES = [1, 2, 3, 12, 13, 19, 20, 21, 28, 29, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256, 257, 303, 304, 305, 384, 385, 768, 769, 1536, 1537,
          2047, 2048]
GS = sorted({1, 4, 5, 8, 9, 64, 4099, 4100, 4101, 4102, 1 << 24}
            | {kr.groups_of(r, last) for r in RANGES for last in (1, 8191, 8192)} - {kr.groups_of(2048, 8192)})


def _capacities(n):
    """absent, fresh for this launch, one record short of it, grown by a 2^28-row launch, grown by a small one"""
    fresh = min(n, kr.TAIL_CHUNK_ROWS) + kr.TAIL_SLACK
    return sorted({0, fresh, fresh - 1, kr.TAIL_CHUNK_ROWS + kr.TAIL_SLACK, 300_001 + kr.TAIL_SLACK})


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("k4route")
    exe = str(d / "k4_route_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "exon_amd", "csrc"),
                    os.path.join(ROOT, "tests", "k4_route_harness.cpp"), "-o", exe], check=True)

    def run(cases):
        p = d / "cases.txt"
        p.write_text("".join("%d %d %d %d %d %d %d\n" % c for c in cases))
        r = subprocess.run([exe, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        lines = r.stdout.decode().split("\n")[:-1]
        assert len(lines) == len(cases) + 2
        return [[int(v) for v in ln.split()] for ln in lines]

    return run


def _check(cases, rows):
    seen = set()
    for c, row in zip(cases, rows):
        cu, bpc, n, G, cap, one, u32 = c
        want = kr.route(cu, bpc, n, G, cap, bool(one), bool(u32))
        got = kr.Route(bool(row[0]), row[1], row[2], bool(row[3]), row[4], row[5], row[6], row[7], row[8], row[9], kr.FORMS[row[10]])
        for f in kr.FIELDS:
            assert getattr(got, f) == getattr(want, f), (f, c, got, want)
        assert row[11] == kr.tail_records(n, G), c
        seen.add((got.form, got.big, got.n_ranges == 1))
    return seen


def test_constants(harness):
    a, b = harness([])
    assert a == [kr.TILE_BIG_J4, kr.TILE_BIG, kr.TILE_SMALL, kr.SLOTS_MIN_G, kr.LDS_GROUPS, kr.TAIL_MAX_RANGES, kr.TAIL_MAX_GRID, kr.TAIL_RANGE, kr.CHUNK,
                 kr.DIRECT_MAX_RANGES, kr.TAIL_CHUNK_ROWS]
    assert b == [kr.TAIL_SLACK, 8192]


def test_mirror_agrees_on_the_grid(harness):
    cases = [(cu, bpc, n, G, cap, 1, 1) for cu in CUS for bpc in BPC for n in NS for G in GS for cap in _capacities(n)]
    # two allocations and a missing u32 block: at the capacities where they decide
    cases += [(cu, 8, n, G, min(n, kr.TAIL_CHUNK_ROWS) + kr.TAIL_SLACK, one, u32) for cu in CUS for n in NS for G in GS for one, u32 in ((0, 1), (1, 0), (0, 0))]
    seen = _check(cases, harness(cases)[2:])
    # the grid reaches every form on both launch shapes, and the direct form with one range and with several
    for form in ("none", "atomic", "scatter", "direct"):
        for big in (False, True):
            assert any(s[0] == form and s[1] == big for s in seen), (form, big)
    assert ("direct", True, True) in seen and ("direct", True, False) in seen and ("direct", False, True) in seen and ("direct", False, False) in seen


def test_the_capacity_border_of_the_issue_table(harness):
    """256 CUs, a scratch sized by the launch itself: the first range count at which the chunk pool and its lists no longer fit
    (12 ranges = 102 404 groups at 700 001 rows, 20 at 4.2 M, 28 at 300 001); one id more than `ranges - 1` full ranges is enough."""
    for n, g_full, ranges in ((700_001, 102_404, 12), (4_200_000, 167_940, 20), (300_001, 233_476, 28)):
        cap = n + kr.TAIL_SLACK
        assert kr.groups_of(ranges) == g_full and kr.n_ranges_of(g_full) == ranges
        g_first = kr.groups_of(ranges, 1)
        assert kr.n_ranges_of(g_first) == ranges and kr.n_ranges_of(g_first - 1) == ranges - 1
        cases = [(256, 8, n, g_first - 1, cap, 1, 1), (256, 8, n, g_first, cap, 1, 1), (256, 8, n, g_first, kr.TAIL_CHUNK_ROWS + kr.TAIL_SLACK, 1, 1)]
        rows = harness(cases)[2:]
        _check(cases, rows)
        assert [kr.FORMS[r[10]] for r in rows] == ["direct", "scatter", "direct"]


def test_scratch_grows_and_never_shrinks():
    s = kr.Scratch(256)
    assert s.launch(700_001, 4100).form == "none" and s.capacity == 0 and not s.has_u32
    assert s.launch(0, 200_000).form in kr.FORMS and s.capacity == 0  # no rows: the scratch is not touched
    assert s.peek(700_001, 200_000).form == "scatter" and s.capacity == 0
    assert s.launch(700_001, 200_000).form == "scatter" and s.capacity == 700_001 + kr.TAIL_SLACK and s.has_u32
    assert s.launch(300_001, 4101).form == "direct" and s.capacity == 700_001 + kr.TAIL_SLACK
    s.launch(1 << 28, 4101)
    assert s.capacity == (1 << 28) + kr.TAIL_SLACK
    s.launch(1 << 28, 4101)
    assert s.capacity == (1 << 28) + kr.TAIL_SLACK
    assert s.launch(700_001, 200_000).form == "direct"
    assert s.launch(700_001, kr.groups_of(129)).form == "scatter"
    assert kr.Scratch(256, 9).launch(700_001, 5000).form == "atomic"
    r = kr.Scratch(256).launch(2047, 4101)
    assert r.form == "direct" and kr.tile_loop_form(r, 2047) == "atomic"  # no whole tile: every row is in the remainder loop
