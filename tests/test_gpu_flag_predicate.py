"""GPU: a BAM / SAM scan with a pushed-down flag / mapping-quality predicate through the GPU pipeline: k_flag_mapq_mask (kernels.hip)
over every slab, the kept rows taken out of every column on the device (take_rows.hip: exon_take_fixed for flag / mapping_quality /
reference / start / end, exon_text_take for name / cigar / sequence and -- k_take_item_spans -- the List<Int64> quality_score) and
sent back as ONE run of views, against tests/flag_predicate_expect.py, which works on the records' dicts alone.

Every scan here is Scan(..., gpu_parse=True, where_flags=...).bind_ctx(ctx) unless said otherwise and every case asserts
decoded_on_gpu() unless said otherwise: a host fallback cannot pass for the device.  The fused-plan cases run "with the device parser
on and off" as Scan(gpu_parse=True / False); the CLI case sets EXON_HIP_GPU_PARSE itself."""
import os

import numpy as np
import pytest

import exon_amd
import flag_predicate_expect as E
from test_flag_predicate import CLI, FX, check, cli_count, fixture_columns, mixed, numpy_keep, scan, write

pytestmark = pytest.mark.gpu
WHERE = (4, 0)


def gpu_scan(ctx, path, fmt, where_flags, project=E.PROJECT, **kw):
    """-> ((columns, batch lengths, Scan.rows()), decoded on the GPU?, export_stats())"""
    s = exon_amd.Scan(str(path), fmt[:3], gpu_parse=True, project=project, where_flags=where_flags, **kw).bind_ctx(ctx)
    cols, lens = E.table(s)
    out = (cols, lens, s.rows()), s.decoded_on_gpu()[0], s.export_stats()
    s.close()
    return out


def check_gpu(got, recs, sam, kept, project=E.PROJECT, batch_size=8192, on_gpu=True):
    assert got[1] == on_gpu
    check(got[0], E.columns(recs, sam, kept, project), len(kept), batch_size)


def pattern_records(n, kept, l_seq=None):
    """n records whose flag passes `flag & 4 = 0` exactly on the rows `kept`"""
    keep = set(kept)
    return [E.read(i, flag=(0, 16, 1024)[i % 3] if i in keep else (4, 20, 1284)[i % 3], mapq=(0, 60, 255)[i % 3], l_seq=l_seq, ref=i % 2) for i in range(n)]


def patterns(n):
    return {"none": [], "all": list(range(n)), "first": [0], "last": [n - 1], "alternating": list(range(0, n, 2)), "every 64th": list(range(0, n, 64))}


# ---- row counts and kept patterns ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bam", "sam"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_kept_patterns_around_a_wave_and_a_workgroup(ctx, tmp_path, n, fmt):
    for k, (name, kept) in enumerate(patterns(n).items()):
        recs = pattern_records(n, kept)
        assert E.keep(recs, *WHERE) == kept
        path = write(tmp_path, f"p{k}", recs, fmt)
        bs = (7, 64, 8192)[(k + n) % 3]
        got = gpu_scan(ctx, path, fmt, WHERE, batch_size=bs)
        check_gpu(got, recs, fmt == "sam", kept, batch_size=bs)  # (rows(), the mask's count, is K)
        assert got[2]["slabs"] == 1 and got[2]["compacted_slabs"] == (1 if kept else 0), name
        host = scan(path, fmt, WHERE, batch_size=bs)
        assert host[0] == got[0][0] and host[2] == got[0][2]


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_the_mapping_quality_conjunct_on_the_device(ctx, tmp_path, fmt):
    recs = mixed(700, seed=12)
    path = write(tmp_path, "q", recs, fmt)
    for where in ((0, 0, 0), (0, 0, 30), (1284, 0, 30), (16, 16, 255), (0, 0, 256), (4, 5), (0xFFFF, 83), (0, 0, -5)):
        check_gpu(gpu_scan(ctx, path, fmt, where), recs, fmt == "sam", E.keep(recs, *where))


# ---- the List<Int64> take ------------------------------------------------------------------------------------------------------------------
# (length, kept?): a kept read of length 0 between two long dropped ones; kept and dropped reads of different lengths side by side; every
# length around the 16-lane group (15, 16, 17, 31, 32, 33), 255 and 1000 kept at least once
SPANS = [(1000, False), (0, True), (255, False), (1, True), (15, False), (15, True), (16, True), (17, False), (17, True), (31, True), (32, False), (32, True),
         (33, True), (1, False), (255, True), (1000, True), (16, False), (33, False), (0, False), (31, True)]


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_the_list_int64_take(ctx, tmp_path, fmt):
    sam = fmt == "sam"
    recs = [E.read(i, flag=0 if keep else 4, l_seq=n, high=not sam) for i, (n, keep) in enumerate(SPANS)]
    if sam:  # QUAL '*' beside a SEQ: an empty list next to a sequence that is not
        for i in (6, 11, 15):
            recs[i]["qual_text"] = "*"
    kept = E.keep(recs, *WHERE)
    assert kept == [i for i, (_, keep) in enumerate(SPANS) if keep] and len(kept) % 4 and len(kept) % 16
    want = E.columns(recs, sam, kept)
    if sam:
        assert [len(q) for q in want["quality_score"]][:5] == [0, 1, 15, 0, 17] and want["sequence"][3] == recs[6]["seq"]
    else:
        assert min(min(q) for q in want["quality_score"] if q) < -100  # quality bytes above 127 are negative Int64 items
    path = write(tmp_path, "l", recs, fmt)
    for bs in (1, 5, 8192):
        got = gpu_scan(ctx, path, fmt, WHERE, batch_size=bs)
        check_gpu(got, recs, sam, kept, batch_size=bs)
        assert got[2]["compacted_slabs"] == 1
    # each text column on its own (the take's scratch is sized per projection) and none
    for project in (("quality_score",), ("name",), ("sequence", "quality_score"), ()):
        check_gpu(gpu_scan(ctx, path, fmt, WHERE, project=project), recs, sam, kept, project)


@pytest.mark.parametrize("l_seq", [31, 32, 33])
def test_sequence_rows_around_the_wide_copy(ctx, tmp_path, l_seq):
    """a string column whose rows are 32 bytes long on average is copied 16 lanes to a row, a shorter one a thread to a row: `sequence`
    just below, at and above that mean (name and cigar stay below it), and a mean of 32 made of rows of 0 and 1000 bases"""
    n = 301
    kept = list(range(0, n, 2)) + [n - 2]
    kept.sort()
    recs = pattern_records(n, kept, l_seq=l_seq)
    if l_seq == 32:
        for i, r in enumerate(recs):
            m = 1000 if i % 25 == 3 else 0
            r.update(E.read(i, flag=r["flag"], mapq=r["mapq"], l_seq=m, ref=r["ref"]))
        assert sum(len(r["seq"]) for r in recs) >= 32 * n
    for fmt in ("bam", "sam"):
        got = gpu_scan(ctx, write(tmp_path, f"w{fmt}", recs, fmt), fmt, WHERE, batch_size=64)
        check_gpu(got, recs, fmt == "sam", kept, batch_size=64)


# ---- several slabs ----------------------------------------------------------------------------------------------------------------------------
def test_several_slabs_with_an_empty_one_between(ctx, tmp_path, monkeypatch):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    n = 24_000  # ~6 MB of SAM text
    rng = np.random.default_rng(7)
    mask = rng.random(n) < 0.05
    mask[n // 5: 4 * n // 5] = False  # the rows of more than two slabs in the middle keep nothing: one slab at least lies inside
    kept = np.flatnonzero(mask).tolist()
    recs = pattern_records(n, kept, l_seq=100)
    path = write(tmp_path, "slabs", recs, "sam")
    assert os.path.getsize(path) > (5 << 20)
    got = gpu_scan(ctx, path, "sam", WHERE)
    check_gpu(got, recs, True, kept)
    st = got[2]
    assert st["slabs"] >= 3 and 2 <= st["compacted_slabs"] < st["slabs"]
    host = scan(path, "sam", WHERE)
    assert host[0] == got[0][0] and host[2] == got[0][2]


# ---- containers and region ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bam", "sam", "sam.gz", "sam.bgz"])
def test_containers_and_region(ctx, tmp_path, fmt):
    recs = mixed(3000, seed=11)
    path = write(tmp_path, "c", recs, fmt)
    sam = fmt != "bam"
    for where in ((4, 0), (1284, 0, 30)):
        check_gpu(gpu_scan(ctx, path, fmt, where, batch_size=64), recs, sam, E.keep(recs, *where), batch_size=64)
        for region, rg in (("r1:2000-6000", ("r1", 2000, 6000)), ("r2:1-3000", ("r2", 1, 3000)), ("r1:50000-60000", ("r1", 50000, 60000))):
            both = E.keep(recs, *where, region=rg)
            assert len(both) < len(E.keep(recs, *where)) and (both or rg[1] == 50000)
            check_gpu(gpu_scan(ctx, path, fmt, where, region=region), recs, sam, both)


def test_the_fixtures_on_the_device(ctx):
    bam = os.path.join(FX, "bam", "test.bam")
    whole = fixture_columns(bam, "bam", project=E.PROJECT)
    for where in ((64, 64, -1), (128, 128, -1), (512, 0, -1), (0, 0, 0)):
        kept = numpy_keep(whole, *where)
        got = gpu_scan(ctx, bam, "bam", where)
        assert got[1]
        check(got[0], E.take(whole, kept), len(kept))
        for use_index in (True, False):  # region AND predicate, through the .bai and without it
            rg = ("chr1", 12205000, 12212000)
            both = numpy_keep(whole, *where, region=rg)
            assert len(both) < len(numpy_keep(whole, 0, 0, region=rg))
            got = gpu_scan(ctx, bam, "bam", where, region="chr1:12205000-12212000", use_index=use_index)
            assert got[1]
            check(got[0], E.take(whole, both), len(both))
    sam = os.path.join(FX, "sam", "test.sam")
    whole = fixture_columns(sam, "sam", project=E.PROJECT)
    for where in ((64, 64, -1), (99, 99, 0), (4, 4, -1), (64, 64, 1)):
        kept = numpy_keep(whole, *where)
        got = gpu_scan(ctx, sam, "sam", where)
        assert got[1]
        check(got[0], E.take(whole, kept), len(kept))


# ---- only survivors cross PCIe -------------------------------------------------------------------------------------------------------------------
def test_only_the_kept_rows_come_back(ctx, tmp_path):
    """16 384 reads of 20 bases, one of every 1024 kept: the kept rows are 1/1024 of the data, the rest of what comes back is the
    alignment of the parts and the count words -- a pass that copied the slab back could not come near a tenth of the unfiltered
    scan's bytes, which are at least 25 bytes of fixed-width columns, 20 of sequence and 8 * 20 of quality items a row"""
    n, l_seq = 16_384, 20
    kept = list(range(100, n, 1024))
    recs = pattern_records(n, kept, l_seq=l_seq)
    path = write(tmp_path, "pcie", recs, "bam")
    got = gpu_scan(ctx, path, "bam", WHERE)
    check_gpu(got, recs, False, kept)
    st = got[2]
    assert st["compacted_slabs"] == st["slabs"] >= 1
    plain = gpu_scan(ctx, path, "bam", None)
    assert plain[1] and plain[0][2] == n and plain[2]["compacted_slabs"] == 0 and plain[2]["slabs"] == st["slabs"]
    assert 0 < st["d2h_bytes"] < plain[2]["d2h_bytes"] / 10
    assert plain[2]["d2h_bytes"] > n * (4 + 1 + 4 + 8 + 8 + l_seq + 8 * l_seq)
    assert st["d2h_bytes"] >= len(kept) * (4 + 1 + 4 + 8 + 8 + l_seq + 8 * l_seq)


# ---- hand-over ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dropped", [False, True])
def test_hand_over_behind_the_rows_emitted(ctx, tmp_path, dropped):
    """a CIGAR with a leading zero in an op count is the host reader's to print ("03M2I" comes out as "3M2I"): the device leaves the
    row undecided and the host reader -- with the same predicate -- finishes the file behind the rows emitted"""
    n = 600
    kept = list(range(0, n, 2))
    recs = pattern_records(n, kept)
    r = 301 if dropped else 300
    recs[r].update(cigar=[(3, 0), (2, 1)], cigar_text="03M2I", seq="ACGTA", qual=[10, 20, 30, 40, 50])
    assert E.keep(recs, *WHERE) == kept and (r in kept) != dropped
    path = write(tmp_path, "ho", recs, "sam")
    check_gpu(gpu_scan(ctx, path, "sam", WHERE, batch_size=64), recs, True, kept, batch_size=64, on_gpu=False)


# ---- fused plans over such a scan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gpu_parse", [True, False])
@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_k3_gets_a_second_conjunct(ctx, tmp_path, fmt, gpu_parse):
    recs = mixed(5000, seed=4)
    path = write(tmp_path, "k3", recs, fmt)
    p1, p2 = (4, 0, 10), (16, 16, 30)
    scan_ = exon_amd.Scan(path, fmt, gpu_parse=gpu_parse, where_flags=p1)
    plan = ctx.plan_flag_mapq_group_count(*p2, 2)
    st = plan.open()
    rows = st.consume(scan_)
    counts, _ = st.finish()
    on = scan_.decoded_on_gpu()[0]
    st.close(); plan.close(); scan_.close()
    kept = E.keep(recs, *p1)
    both = [i for i in kept if E.passes(recs[i]["flag"], recs[i]["mapq"], *p2)]
    want = [sum(1 for i in both if recs[i]["ref"] == g) for g in (0, 1)] + [sum(1 for i in both if recs[i]["ref"] is None)]
    assert on == gpu_parse and rows == len(kept) and 0 < len(both) < len(kept) and all(want)
    assert counts.tolist() == want


@pytest.mark.parametrize("gpu_parse", [True, False])
@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_k6_counts_the_kept_rows(ctx, tmp_path, fmt, gpu_parse):
    recs = mixed(5000, seed=9)
    path = write(tmp_path, "k6", recs, fmt)
    where, rg = (1284, 0, 30), ("r2", 3000, 9000)
    scan_ = exon_amd.Scan(path, fmt, gpu_parse=gpu_parse, where_flags=where)
    plan = ctx.plan_overlap_count(1, rg[1], rg[2])
    st = plan.open()
    rows = st.consume(scan_)
    counts, _ = st.finish()
    on = scan_.decoded_on_gpu()[0]
    st.close(); plan.close(); scan_.close()
    kept, both = E.keep(recs, *where), E.keep(recs, *where, region=rg)
    assert on == gpu_parse and rows == len(kept) and 0 < len(both) < len(E.keep(recs, 0, 0, region=rg))
    assert int(counts[0]) == len(both)


def test_cli_region_and_flags_on_the_device(tmp_path):
    """bam_region_filter(..) AND flag & M = V AND CAST(mapping_quality AS INT) >= q: K6 over a scan that carries the flag predicate, the
    records decoded on the device (EXON_HIP_GPU_PARSE_STRICT=1) and, EXON_HIP_GPU_PARSE=0, by the host reader"""
    assert os.path.exists(CLI)
    recs = mixed(2000, seed=6)
    both = E.keep(recs, 4, 0, 10, region=("r1", 300, 4000))
    assert 0 < len(both) < len(E.keep(recs, 0, 0, region=("r1", 300, 4000)))
    for fmt in ("bam", "sam"):
        src = f"{fmt}_scan('{write(tmp_path, 'c', recs, fmt)}')"
        sql = f"SELECT COUNT(*) FROM {src} WHERE bam_region_filter('r1:300-4000', reference, start, end) AND flag & 4 = 0 AND CAST(mapping_quality AS INT) >= 10"
        assert cli_count(sql, EXON_HIP_GPU_PARSE_STRICT="1") == len(both)
        assert cli_count(sql, EXON_HIP_GPU_PARSE="0") == len(both)
