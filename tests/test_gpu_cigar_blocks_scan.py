"""GPU: BAM and SAM scans in blocks mode (exon_hip_scan_set_cover_ops) under names-form plans of kinds 12, 13 and 14.  The files come
from tests/bam_sam_writer.py: records mixing M I D N S H P = X, unmapped and '*' records, read names of every length mod 4 so that
the slab's ops are unaligned.  The device-decoded state == the host reader's state == the expectation (the records' aligned blocks
from cigar_blocks_expect.py through each kind's own expect_state), word for word; decoded_on_gpu is asserted for every device run;
`rows` counts records; mask 0x18D gives span mode's state.  Then slab seams, the predicates, two @SQ orders, a spliced read over a
whole target, and the refusals."""
import os

import numpy as np
import pytest

import bam_sam_writer as bsw
import cigar_blocks_expect as E
import exon_amd
import flag_predicate_expect as FE
import region_bases_expect as E12
import region_depth_expect as E14
import window_bases_expect as E13
from test_flag_predicate import BGZIP, FX

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED, ESTATE = -1, -4, -5
COLS = (2, 3, 4)
REGIONS = [("r2", 300, 900), ("r1", 1, 4000), ("r2", 1, 99), ("r1", 7000, 7000), ("r3", 1, 500), ("r2", 3000, 9000), ("r1", 2500, 5200)]
CONTIGS = [("r2", 9000), ("r1", 12000)]
THR = [1, 2, 5]
MASKS = [E.ALIGNED, E.ALIGNED_DEL, E.LEGAL]
SHAPES = ["30M", "10M200N15M", "5S20M3D20M2I10M", "8=1X8=", "4H10M5P10M", "12M300N12M40N6M", "3I", "25N", "", "7M2D", "1M1N1M1N1M", "6S6M"]


def records(n, seed=1, l_seq=None):
    rng = np.random.default_rng(seed)
    flag = rng.choice([0, 4, 16, 83, 147, 256, 1024, 1040, 2048], n)
    mapq = rng.choice([0, 10, 29, 30, 60, 255], n)
    shape = rng.integers(0, len(SHAPES), n)
    out = []
    for i in range(n):
        k = 4 + i % 9 if l_seq is None else l_seq
        out.append(dict(name="*" if i % 11 == 5 else "q" * (i % 4) + str(i % 10), flag=int(flag[i]), ref=None if i % 17 == 3 else i % 2, pos=0 if i % 19 == 7 else 50 + 3 * i,
                        mapq=int(mapq[i]), cigar=E.cigar(SHAPES[shape[i]]), seq="".join("ACGT"[(i + j) % 4] for j in range(k)), qual=[10 + (i + j) % 60 for j in range(k)]))
    return out


def write(tmp, name, recs, fmt, refs=bsw.REFS):
    p = str(tmp / (name + "." + fmt))
    if fmt == "bam":
        bsw.write_bam(p, recs, BGZIP, refs=refs)
    else:
        bsw.write_sam(p, recs, refs=refs)
    return p


def plan_of(ctx, kind):
    if kind == 12:
        return ctx.plan_region_set_bases(REGIONS, columns=COLS)
    if kind == 13:
        return ctx.plan_window_bases(CONTIGS, 100, columns=COLS)
    return ctx.plan_region_set_depth(REGIONS, THR, columns=COLS)


def through(ctx, kind, paths, fmt, gpu_parse, cover, **kw):
    """-> (rows of every file, the state, decoded on the GPU? of every file) with ONE stream over all `paths`"""
    plan = plan_of(ctx, kind)
    st = plan.open()
    rows, on = [], []
    for p in paths:
        scan = exon_amd.Scan(str(p), fmt, gpu_parse=gpu_parse, cover_ops=cover, **kw)
        rows.append(st.consume(scan))
        assert scan.rows() == rows[-1]
        on.append(bool(scan.decoded_on_gpu()[0]))
        scan.close()
    state, _ = st.finish()
    st.close(); plan.close()
    return rows, state, on


def expect_state(kind, recs, mask, refs=bsw.REFS, kept=None):
    """the state of the kept records' block rows (mask None: their spans), contigs by NAME"""
    kept = range(len(recs)) if kept is None else kept
    names = [n for n, _ in refs]
    sel = [recs[i] for i in kept]
    rv = np.array([r["ref"] is not None for r in sel], bool)
    sv = np.array([r["pos"] >= 1 for r in sel], bool)
    order = {}
    for c, *_ in (REGIONS if kind != 13 else CONTIGS):
        order.setdefault(c, len(order))
    ref = np.array([order.get(names[r["ref"]], 99) if r["ref"] is not None else -1 for r in sel], np.int32)
    start = np.array([r["pos"] for r in sel], np.int64)
    cig = [r["cigar"] for r in sel]
    if mask is None:  # span mode: three bitmaps, end NULL with start
        end = start + np.array([sum(ln for ln, c in ops if c in E.REF_CODES) for ops in cig], np.int64) - 1
        rows = (ref, start, end, rv, sv, sv)
    else:
        r, s, e, v = E.expand(ref, start, cig, mask, rv, sv)
        rows = (r, s, e, v, v, v)
    if kind == 12:
        return E12.expect_state([(order[c], a, b) for c, a, b in REGIONS], *rows)
    if kind == 13:
        return E13.expect_state([(order[c], ln) for c, ln in CONTIGS], 100, *rows)
    return E14.expect_state([(order[c], a, b) for c, a, b in REGIONS], *rows)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("blocks")
    recs = records(3000)
    assert {len(r["name"]) % 4 for r in recs} == {0, 1, 2, 3}
    return recs, {fmt: write(tmp, "mix", recs, fmt) for fmt in ("bam", "sam")}


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("kind", [12, 13, 14])
@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_device_state_is_host_state_is_the_expectation(ctx, files, fmt, kind, mask):
    recs, paths = files
    g = through(ctx, kind, [paths[fmt]], fmt, True, mask)
    h = through(ctx, kind, [paths[fmt]], fmt, False, mask)
    assert g[2] == [True] and h[2] == [False], "silent host fallback"
    assert g[0] == h[0] == [len(recs)]  # rows = records, not block rows
    want = expect_state(kind, recs, mask)
    assert np.array_equal(g[1], want) and np.array_equal(h[1], want)
    if mask != E.LEGAL:
        assert g[1][:4].sum() > len(recs)  # the totals count block rows
    else:  # 0x18D: span mode's state, word for word
        span = through(ctx, kind, [paths[fmt]], fmt, True, None)
        assert span[2] == [True] and np.array_equal(span[1], g[1]) and np.array_equal(span[1], expect_state(kind, recs, None))
        assert g[1][:4].sum() == len(recs)


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_records_cross_slabs(ctx, tmp_path, monkeypatch, fmt):
    """a few MB under 1 MiB slabs: records (and SAM lines) straddle the slabs, the block buffers are reused and regrown"""
    recs = records(30000, seed=5, l_seq=90 if fmt == "bam" else 40)
    path = write(tmp_path, "big", recs, fmt)
    assert os.path.getsize(path + ".u" if fmt == "bam" else path) > 3 << 20
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    for kind in (12, 14):
        g = through(ctx, kind, [path], fmt, True, E.ALIGNED)
        assert g[2] == [True] and g[0] == [len(recs)]
        assert np.array_equal(g[1], expect_state(kind, recs, E.ALIGNED))
    monkeypatch.delenv("EXON_HIP_GPU_PARSE_SLAB_MB")
    h = through(ctx, 12, [path], fmt, False, E.ALIGNED)
    assert h[2] == [False] and np.array_equal(h[1], expect_state(12, recs, E.ALIGNED))


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_predicates_select_records_by_span(ctx, files, fmt):
    """a flag predicate and a region keep RECORDS; every block of a kept record is emitted, those outside the region included.  (As in
    span mode the device path masks the dropped records, which the plan sees as NULL rows, and the host reader never emits them:
    every word but null_rows agrees.)"""
    recs, paths = files
    for kw, kept in (({"where_flags": (1284, 0, 30)}, FE.keep(recs, 1284, 0, 30)), ({"region": "r2:400-700"}, FE.keep(recs, 0, 0, -1, ("r2", 400, 700)))):
        assert 0 < len(kept) < len(recs)
        want = expect_state(12, recs, E.ALIGNED, kept=kept)
        for gpu_parse in (True, False):
            rows, state, on = through(ctx, 12, [paths[fmt]], fmt, gpu_parse, E.ALIGNED, **kw)
            assert on == [gpu_parse] and rows == [len(kept)]
            assert state[0] == want[0] and np.array_equal(state[2:], want[2:])
            if not gpu_parse:
                assert np.array_equal(state, want)


def test_two_files_with_different_sq_orders_in_one_stream(ctx, tmp_path):
    a, b = records(2000, seed=31), records(1500, seed=32)
    flipped = [bsw.REFS[1], bsw.REFS[0]]  # in the second file id 0 is "r2"
    pa, pb = write(tmp_path, "a", a, "sam"), write(tmp_path, "b", b, "sam", refs=flipped)
    for kind in (12, 13):
        want = (expect_state(kind, a, E.ALIGNED).view(np.uint64) + expect_state(kind, b, E.ALIGNED, refs=flipped).view(np.uint64)).view(np.int64)
        for gpu_parse in (True, False):
            rows, state, on = through(ctx, kind, [pa, pb], "sam", gpu_parse, E.ALIGNED)
            assert on == [gpu_parse, gpu_parse] and rows == [2000, 1500]
            assert np.array_equal(state, want)


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_a_spliced_read_whose_intron_spans_a_whole_target(ctx, tmp_path, fmt):
    rec = dict(name="spliced", flag=0, ref=0, pos=1000, mapq=60, cigar=E.cigar("50M10000N50M"), seq="ACGT", qual=[30] * 4)
    path = write(tmp_path, "rna", [rec], fmt)
    for cover, bases in ((E.ALIGNED, 0), ("aligned", 0), ("aligned+del", 0), (None, 1000), (E.LEGAL, 1000)):
        for gpu_parse in (True, False):
            plan = ctx.plan_region_set_bases([("r1", 2000, 2999), ("r1", 1040, 1059)], columns=COLS)
            st = plan.open()
            scan = exon_amd.Scan(path, fmt, gpu_parse=gpu_parse, cover_ops=cover)
            assert st.consume(scan) == 1 and bool(scan.decoded_on_gpu()[0]) == gpu_parse
            state, _ = st.finish()
            assert plan.decode(state).tolist() == [bases, 10 if bases == 0 else 20]
            scan.close(); st.close(); plan.close()


def _consume_error(ctx, path, fmt, gpu_parse, cover=E.ALIGNED, kind=12):
    plan = plan_of(ctx, kind)
    st = plan.open()
    scan = exon_amd.Scan(path, fmt, gpu_parse=gpu_parse, cover_ops=cover)
    with pytest.raises(exon_amd.ExonHipError) as e:
        st.consume(scan)
    scan.close(); st.close(); plan.close()
    return e.value


def test_plans_that_count_records_and_batches_are_refused(ctx, files):
    recs, paths = files
    for fmt in ("bam", "sam"):
        for gpu_parse in (True, False):
            for plan in (ctx.plan_region_set_overlap(REGIONS, columns=COLS),                                      # kind 11
                         ctx.plan_flag_mapq_group_count(4, 0, 0, 2, columns=(0, 1, 2)),                           # K3
                         ctx.plan_overlap_count(0, 1, 5000, columns=COLS)):                                      # K6
                st = plan.open()
                scan = exon_amd.Scan(paths[fmt], fmt, gpu_parse=gpu_parse, cover_ops="aligned")
                with pytest.raises(exon_amd.ExonHipError) as e:
                    st.consume(scan)
                assert e.value.code == EUNSUPPORTED and "once per aligned block" in str(e.value)
                assert scan.rows() == 0  # before anything is read
                scan.close(); st.close(); plan.close()
        scan = exon_amd.Scan(paths[fmt], fmt, gpu_parse=False, cover_ops="aligned")
        with pytest.raises(exon_amd.ExonHipError) as e:
            next(iter(scan))
        assert e.value.code == EUNSUPPORTED and "one row per record" in str(e.value)
        scan.close()
        scan = exon_amd.Scan(paths[fmt], fmt, gpu_parse=True, cover_ops="aligned")
        with pytest.raises(exon_amd.ExonHipError) as e:
            scan.bind_ctx(ctx)
        assert e.value.code == EUNSUPPORTED and "one row per record" in str(e.value)
        scan.close()


def test_formats_without_a_cigar_late_calls_and_illegal_bits_are_refused(ctx, files):
    recs, paths = files
    for path, fmt, word in ((os.path.join(FX, "cram", "test_input_1_a.cram"), "cram", "span only"), (os.path.join(FX, "gff", "test.gff.gz"), "gff", "no CIGAR"),
                            (os.path.join(FX, "bed", "test.bed"), "bed", "no CIGAR")):
        with pytest.raises(exon_amd.ExonHipError) as e:
            exon_amd.Scan(path, fmt, cover_ops="aligned")
        assert e.value.code == EUNSUPPORTED and word in str(e.value)
    for mask in (0x2, 0x10, 0x200, 0x18D | 0x40, 0xFFFFFFFF):
        with pytest.raises(exon_amd.ExonHipError) as e:
            exon_amd.Scan(paths["bam"], "bam", cover_ops=mask)
        assert e.value.code == EINVAL and "0x18D" in str(e.value)
    exon_amd.Scan(os.path.join(FX, "gff", "test.gff.gz"), "gff", cover_ops=0).close()  # 0 is "off", like None: nothing to refuse
    with pytest.raises(exon_amd.ExonHipError) as e:
        exon_amd.Scan(paths["bam"], "bam", cover_ops="aligned", project=("cigar",))
    assert e.value.code == EUNSUPPORTED
    # a second call replaces the first, 0 turns the mode off; a call after the scan has been read from is out of order
    scan = exon_amd.Scan(paths["sam"], "sam", gpu_parse=True, cover_ops="aligned").set_cover_ops(E.ALIGNED_DEL).set_cover_ops(0)
    plan = plan_of(ctx, 12)
    st = plan.open()
    assert st.consume(scan) == len(recs)
    state, _ = st.finish()
    assert np.array_equal(state, expect_state(12, recs, None))
    with pytest.raises(exon_amd.ExonHipError) as e:
        scan.set_cover_ops("aligned")
    assert e.value.code == ESTATE
    scan.close(); st.close(); plan.close()


def test_the_cg_placeholder_is_an_error_that_names_the_tag(ctx, tmp_path):
    recs = records(400, seed=7)
    recs[250]["cigar"] = [(len(recs[250]["seq"]), 4), (5000, 3)]  # <l_seq>S<n>N: the real ops are in a CG tag
    recs[250]["ref"], recs[250]["pos"] = 0, 777
    path = write(tmp_path, "cg", recs, "bam")
    for gpu_parse in (True, False):
        err = _consume_error(ctx, path, "bam", gpu_parse)
        assert "CG" in str(err)
    # span mode reads the file as before
    plan = plan_of(ctx, 12)
    st = plan.open()
    assert st.consume(exon_amd.Scan(path, "bam", gpu_parse=True)) == 400
    st.close(); plan.close()


def test_a_sam_op_of_2_pow_28_and_an_unknown_letter_are_invalid(ctx, tmp_path):
    for text in ("268435456M", "10M5Q10M", "M", "10"):
        recs = records(300, seed=8)
        recs[123].update(cigar_text=text, ref=1, pos=500)
        path = write(tmp_path, "bad", recs, "sam")
        for gpu_parse in (True, False):
            err = _consume_error(ctx, path, "sam", gpu_parse)
            assert "invalid CIGAR '%s'" % text in str(err)
    recs = records(300, seed=8)
    recs[123].update(cigar_text="268435455M", cigar=[((1 << 28) - 1, 0)], ref=1, pos=500)  # the longest op BAM can hold is fine
    path = write(tmp_path, "top", recs, "sam")
    g = through(ctx, 12, [path], "sam", True, E.ALIGNED)
    assert g[2] == [True] and np.array_equal(g[1], expect_state(12, recs, E.ALIGNED))
