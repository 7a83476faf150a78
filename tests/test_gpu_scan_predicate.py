"""GPU: a VCF scan with a pushed-down value predicate through the GPU pipeline: k_value_mask (kernels.hip) over every slab, the kept
rows taken out of every column on the device (take_rows.hip: k_mask_rows_fill, k_take_fixed, k_take_bits, exon_text_take) and sent
back as ONE run of views -- against tests/scan_predicate_expect.py, which never touches the library.

Every scan here is Scan(..., gpu_parse=True, where=...).bind_ctx(ctx) unless said otherwise, and every case asserts decoded_on_gpu()
unless said otherwise: a host fallback cannot pass for the device.  The sizes are the ones at which the kernels can go wrong: row
counts around a wave (64) and a workgroup (256), kept rows none / all / at either end / across a wave boundary / scattered."""
import os

import numpy as np
import pytest

import exon_amd
import scan_predicate_expect as E
from bgzf_index_writer import write_tabix
from test_scan_predicate import k2_count, k4_groups, k4_numpy, mixed, table, write

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "ref_fixtures")
PROJECT = ("id", "ref", "alt", "info")
WHERE = (2, ">=", 30.0)


def gpu_scan(ctx, path, where, project=PROJECT, gpu_parse=True, **kw):
    """-> (columns, batch lengths, Scan.rows(), decoded on the GPU?, export_stats())"""
    s = exon_amd.Scan(str(path), "vcf", info_field=E.INFO_FIELD, gpu_parse=gpu_parse, project=project, where=where, **kw)
    if gpu_parse:
        s.bind_ctx(ctx)
    cols, lens = table(s)
    out = cols, lens, s.rows(), s.decoded_on_gpu()[0], s.export_stats()
    s.close()
    return out


def check(got, lines, wants, kept, project=PROJECT, batch_size=8192, on_gpu=True):
    cols, lens, rows, on, _ = got
    assert on == on_gpu
    assert rows == len(kept) == sum(lens) and all(0 < n <= batch_size for n in lens)
    if kept:
        assert E.same(cols, E.columns(lines, wants, kept, project))
    else:
        assert cols == {}


def pattern_lines(n, kept, seed=0):
    """n lines whose qual passes `>= 30` exactly on the rows `kept`; the others fail it or are NULL"""
    keep = set(kept)
    made = [E.line(i, ("40", "30", "1e3")[i % 3] if i in keep else ("20", ".", "29.99")[i % 3]) for i in range(n)]
    return [m[0] for m in made], [m[1] for m in made]


def patterns(n):
    rng = np.random.default_rng(n)
    return {"none": [], "all": list(range(n)), "first": [0], "last": [n - 1], "every other": list(range(0, n, 2)),
            "60..70": [r for r in range(60, 71) if r < n], "p=0.05": np.flatnonzero(rng.random(n) < 0.05).tolist(),
            "p=0.5": np.flatnonzero(rng.random(n) < 0.5).tolist()}


# ---- row counts and kept patterns ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 2049])
def test_kept_patterns_around_a_wave_and_a_workgroup(ctx, tmp_path, n):
    for k, (name, kept) in enumerate(patterns(n).items()):
        lines, wants = pattern_lines(n, kept)
        assert E.keep(lines, "qual", *WHERE[1:]) == kept
        bs = (7, 64, 8192)[(k + n) % 3]
        got = gpu_scan(ctx, write(tmp_path, f"p{k}", lines), WHERE, batch_size=bs)
        check(got, lines, wants, kept, batch_size=bs)
        st = got[4]
        assert st["slabs"] == 1 and st["compacted_slabs"] == (1 if kept else 0), name


@pytest.mark.parametrize("pad", range(16))
def test_line_start_residues(ctx, tmp_path, pad):
    n = 257
    kept = patterns(n)["p=0.5"]
    lines, wants = pattern_lines(n, kept)
    check(gpu_scan(ctx, write(tmp_path, "pad", lines, pad=pad), WHERE, batch_size=64), lines, wants, kept, batch_size=64)


# ---- operators and types ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["qual", "AF", "DP"])
def test_operator_literal_and_null_table_on_the_device(ctx, tmp_path, what):
    """the host test's table.  The device parsers leave the nan / inf SPELLINGS to the host reader, so the table runs twice: without
    those rows (decoded on the device, NaN literal included) and with them (handed over: the same rows come out of the host reader)"""
    project = ("id", "ref", "alt")  # (no `info`: the table has `AF=.` rows, which that column refuses)
    for spelled_out in (False, True):
        lines = E.table_lines(what, spelled_out)
        path = write(tmp_path, f"t{spelled_out}", lines)
        handed_over = spelled_out and what != "DP"
        for op in E.OPS if not spelled_out else (">=", "!="):
            for lit in E.LITERALS[what]:
                kept = E.keep(lines, what, op, lit)
                check(gpu_scan(ctx, path, (E.COLUMN[what], op, lit), project), lines, None, kept, project, on_gpu=not handed_over)


# ---- several slabs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.05, 0.5])
def test_several_slabs_with_an_empty_one_between(ctx, tmp_path, monkeypatch, p):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    n = 64_000  # ~4 MB
    rng = np.random.default_rng(int(p * 100))
    mask = rng.random(n) < p
    mask[n // 5: 4 * n // 5] = False  # the rows of more than two slabs in the middle keep nothing: one slab at least lies inside
    kept = np.flatnonzero(mask).tolist()
    lines, wants = pattern_lines(n, kept)
    path = write(tmp_path, "slabs", lines)
    assert os.path.getsize(path) > (5 << 19)
    got = gpu_scan(ctx, path, WHERE)
    check(got, lines, wants, kept)
    st = got[4]
    assert st["slabs"] >= 3 and 2 <= st["compacted_slabs"] < st["slabs"]
    host = gpu_scan(ctx, path, WHERE, gpu_parse=False)
    assert not host[3] and E.same(host[0], got[0]) and host[2] == got[2]


# ---- compression and region --------------------------------------------------------------------------------------------------------------
def test_gzip_bgzf_and_region(ctx, tmp_path):
    lines, wants = mixed(3000, seed=11, pos0=False, chrom=lambda i: "1" if i < 2000 else "2")
    kept = E.keep(lines, "qual", ">=", 30.0)
    gz, bg = write(tmp_path, "c", lines, "gz"), write(tmp_path, "c", lines, "bgzf")
    for path in (gz, bg):
        check(gpu_scan(ctx, path, WHERE, batch_size=64), lines, wants, kept, batch_size=64)
    assert write_tabix(bg) == 3000
    for region, rg in (("1:500-1500", ("1", 500, 1500)), ("2:2001-2500", ("2", 2001, 2500)), ("1:5000-6000", ("1", 5000, 6000))):
        both = E.keep(lines, "qual", ">=", 30.0, rg)
        assert len(both) < len(kept)
        for use_index in (False, True):
            check(gpu_scan(ctx, bg, WHERE, region=region, use_index=use_index), lines, wants, both)
    both = E.keep(lines, "DP", ">", 90000.0, ("1", 1, 1000))
    check(gpu_scan(ctx, bg, (5, ">", 90000.0), region="1:1-1000", use_index=True), lines, wants, both)


# ---- only survivors cross PCIe -----------------------------------------------------------------------------------------------------------
def test_only_the_kept_rows_come_back(ctx, tmp_path):
    """65 536 rows, one of every 4096 kept: the kept rows are 1/4096 of the data, the rest of what comes back is the 64-byte alignment
    of the parts and the count words -- a pass that copied the slab back could not come near a tenth of the unfiltered scan's bytes"""
    n = 65_536
    kept = list(range(100, n, 4096))
    lines, wants = pattern_lines(n, kept)
    path = write(tmp_path, "pcie", lines)
    got = gpu_scan(ctx, path, WHERE)
    check(got, lines, wants, kept)
    st = got[4]
    assert st["compacted_slabs"] == st["slabs"] >= 1
    plain = gpu_scan(ctx, path, None)
    assert plain[3] and plain[2] == n and plain[4]["compacted_slabs"] == 0 and plain[4]["slabs"] == st["slabs"]
    assert 0 < st["d2h_bytes"] < plain[4]["d2h_bytes"] / 10
    assert plain[4]["d2h_bytes"] > n * 20  # (chrom, pos, qual, filter alone are 20 bytes a row)


# ---- hand-over ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dropped", [False, True])
def test_hand_over_behind_the_rows_emitted(ctx, tmp_path, dropped):
    """a Float value of more than 19 digits is the host reader's to print: with `info` projected the device leaves the row undecided
    and the host reader -- with the same predicate -- finishes the file"""
    n = 600
    kept = patterns(n)["p=0.5"]
    lines, wants = pattern_lines(n, kept)
    r = 300
    lines[r] = E.line(r, "20" if dropped else "40", info="XF=0.12345678901234567890")[0]
    wants[r] = "XF=0.12345679"
    kept = E.keep(lines, "qual", *WHERE[1:])
    assert (r in kept) != dropped
    check(gpu_scan(ctx, write(tmp_path, "ho", lines), WHERE, batch_size=64), lines, wants, kept, batch_size=64, on_gpu=False)


# ---- fused plans over such a scan, on the device ----------------------------------------------------------------------------------------
def test_k2_plan_counts_the_kept_rows_on_the_device(ctx, tmp_path):
    lines, _ = mixed(5000, seed=3)
    path = write(tmp_path, "k2", lines)
    kept = E.keep(lines, "qual", ">=", 30.0)
    in_region = [i for i in kept if int(lines[i].split("\t")[1]) >= 1]
    dev, host = k2_count(ctx, path, WHERE, True), k2_count(ctx, path, WHERE, False)
    assert dev == (len(kept), len(in_region), True) and host == (len(kept), len(in_region), False)
    # ... and with the region of the plan narrower than the file
    narrow = [i for i in kept if 1000 <= int(lines[i].split("\t")[1]) <= 3000]
    assert k2_count(ctx, path, WHERE, True, (1000, 3000)) == (len(kept), len(narrow), True)


def test_k4_plan_gets_a_second_conjunct_on_the_device(ctx, tmp_path):
    lines, _ = mixed(5000, seed=4)
    path = write(tmp_path, "k4", lines)
    where = (5, "<", 50000.0)
    kept = E.keep(lines, "DP", "<", 50000.0)
    want = k4_numpy(lines, kept)
    rows, got, on = k4_groups(ctx, path, where, True)
    hrows, host, hon = k4_groups(ctx, path, where, False)
    assert rows == hrows == len(kept) and on and not hon and got.keys() == host.keys() == want.keys()
    for k in want:
        assert got[k][:2] == want[k][:2] == host[k][:2]
        assert got[k][2] == pytest.approx(want[k][2], rel=1e-9) and got[k][2] == pytest.approx(host[k][2], rel=1e-9)
    # with a pushed-down region as the third conjunct
    scan_region = ("1", 1000, 4000)
    both = E.keep(lines, "DP", "<", 50000.0, scan_region)
    want = k4_numpy(lines, both)
    scan = exon_amd.Scan(path, "vcf", info_field="AF,DP", gpu_parse=True, where=where, region="1:1000-4000")
    plan = ctx.plan_cmp_avg_by_group(">", 0.01, 8, columns=(4, 2, 3))
    st = plan.open()
    rows = st.consume(scan)
    counts, sums = st.finish()
    names = scan.dictionary(3)
    got = {names[g]: (int(counts[g]), int(counts[8 + g]), float(sums[g])) for g in range(len(names)) if counts[8 + g]}
    assert scan.decoded_on_gpu()[0] and rows == len(both) and got.keys() == want.keys()
    st.close(); plan.close(); scan.close()
    for k in want:
        assert got[k][:2] == want[k][:2] and got[k][2] == pytest.approx(want[k][2], rel=1e-9)


# ---- the reference's fixture ------------------------------------------------------------------------------------------------------------
def test_the_reference_fixture(ctx):
    """index.vcf.gz, project id and info: the rows of oracle/decode.py's decode_vcf filtered in Python, info from decode.info_string.
    Every QUAL of the fixture is 0, so `qual >= 30` -- the query this is named after -- keeps nothing; `qual < 30` keeps all 621 rows
    and info.DP > 2 a part of them."""
    from oracle import decode
    path = os.path.join(FX, "vcf", "index.vcf.gz")
    v = decode.decode_vcf(path)
    n = len(v["chrom"])
    qual = [None if q is None else np.float32(q) for q in v["qual"]]
    dp = [E.info_value(raw, "DP") for raw in v["info_raw"]]
    dp = [None if d in (None, True) else int(d) for d in dp]
    cases = [(WHERE, None, [i for i in range(n) if E.passes(qual[i], ">=", 30.0)]), ((2, "<", 30.0), None, [i for i in range(n) if E.passes(qual[i], "<", 30.0)]),
             ((4, ">", 2.0), "DP", [i for i in range(n) if E.passes(dp[i], ">", 2.0)])]
    assert [len(c[2]) for c in cases][:2] == [0, 621] and 0 < len(cases[2][2]) < 621
    for where, info_field, keep in cases:
        s = exon_amd.Scan(path, "vcf", gpu_parse=True, info_field=info_field, project=("id", "info"), where=where).bind_ctx(ctx)
        cols, _ = table(s)
        assert s.decoded_on_gpu()[0] and s.rows() == len(keep)
        s.close()
        if not keep:
            assert cols == {}
            continue
        assert cols["info"] == [decode.info_string(v, i) for i in keep]
        assert cols["pos"] == [v["pos"][i] for i in keep]
        assert cols["id"] == [v["id"][i] if v["id"][i] else None for i in keep]
