"""GPU: a names-form window plan (kind 13) fed by files.  The contigs and their lengths come from the file's own header
(Scan.reference_lengths() beside dictionary(2)) or from the caller; every consumed scan resolves the names in its own dictionary.  The
expected sums come from the HOST reader's batches of the same file (gpu_parse off) through numpy (window_bases_expect.py); the
device-decoded run and the host-decoded run must both give them."""
import os

import numpy as np
import pytest

import bam_sam_writer as bsw
import exon_amd
import flag_predicate_expect as FE
import window_bases_expect as E
from test_flag_predicate import BGZIP, FX, mixed, write

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -4
COLS = {"bam": (2, 3, 4), "sam": (2, 3, 4), "gff": (0, 3, 4)}
CONTIG = {"bam": "reference", "sam": "reference", "gff": "seqname"}


def header_contigs(path, fmt):
    scan = exon_amd.Scan(str(path), fmt, gpu_parse=False)
    out = list(zip(scan.dictionary(2), scan.reference_lengths()))
    scan.close()
    return out


def through_windows(ctx, paths, fmt, contigs, W, gpu_parse, where_flags=None):
    """-> (rows of every file, state, bases per window, decoded on the GPU? of every file) with ONE stream over all `paths`"""
    plan = ctx.plan_window_bases(contigs, W, columns=COLS[fmt])
    assert plan.by_name
    st = plan.open()
    rows, on = [], []
    for p in paths:
        kw = {} if where_flags is None else {"where_flags": where_flags}
        scan = exon_amd.Scan(str(p), fmt, gpu_parse=gpu_parse, **kw)
        rows.append(st.consume(scan))
        on.append(scan.decoded_on_gpu()[0])
        scan.close()
    state, _ = st.finish()
    bases = plan.decode(state)
    st.close(); plan.close()
    return rows, state, bases, on


def host_rows(path, fmt, contigs, where_flags=None):
    """the host reader's batches as expect()'s arguments: names -> the contig's slot (a name outside the plan: -2), None -> invalid"""
    kw = {} if where_flags is None else {"where_flags": where_flags}
    scan = exon_amd.Scan(str(path), fmt, gpu_parse=False, **kw)
    cols, _ = FE.table(scan)
    scan.close()
    slot = {name: i for i, (name, _) in enumerate(contigs)}
    names, starts, ends = cols[CONTIG[fmt]], cols["start"], cols["end"]
    ref = np.array([0 if c is None else slot.get(c, -2) for c in names], np.int32)
    val = lambda xs: np.array([0 if x is None else x for x in xs], np.int64)  # noqa: E731
    ok = lambda xs: np.array([x is not None for x in xs], bool)  # noqa: E731
    return ref, val(starts), val(ends), ok(names), ok(starts), ok(ends)


def by_slot(contigs):
    return [(i, ln) for i, (_, ln) in enumerate(contigs)]


def check_file(ctx, path, fmt, contigs, W, n_rows, pileup=True):
    g = through_windows(ctx, [path], fmt, contigs, W, True)
    h = through_windows(ctx, [path], fmt, contigs, W, False)
    assert g[3] == [True] and h[3] == [False], "silent host fallback"  # decoded_on_gpu == 1, and == 0 with the device parser off
    assert g[0] == h[0] == [n_rows]
    assert np.array_equal(g[1], h[1])
    rows = host_rows(path, fmt, contigs)
    assert len(rows[0]) == n_rows
    assert np.array_equal(g[1], E.expect_state(by_slot(contigs), W, *rows))
    totals, bases = (E.expect if pileup else E.expect_fast)(by_slot(contigs), W, *rows)
    assert g[1][:4].tolist() == totals.tolist() and totals.sum() == n_rows
    assert np.array_equal(g[2], bases) and np.array_equal(h[2], bases)
    return totals, bases


@pytest.mark.parametrize("W", [1000, 100_000])
def test_bam_reference_fixture(ctx, W):
    path = os.path.join(FX, "bam", "test.bam")
    contigs = header_contigs(path, "bam")
    assert len(contigs) == 195 and contigs[0] == ("chr1", 248956422)
    totals, bases = check_file(ctx, path, "bam", contigs, W, 61)
    assert totals[0] > 0 and bases.sum() > 0
    assert bases.size == sum((ln - 1) // W + 1 for _, ln in contigs)


@pytest.mark.parametrize("W", [7, 50])
def test_sam_reference_fixture(ctx, W):
    path = os.path.join(FX, "sam", "test.sam")
    contigs = header_contigs(path, "sam")
    assert contigs == [("ref1", 56)]
    totals, bases = check_file(ctx, path, "sam", contigs, W, 1)
    assert totals.tolist() == [1, 0, 0, 0] and bases.sum() > 0


def test_gff_fixture_with_caller_given_lengths(ctx):
    path = os.path.join(FX, "gff", "test.gff.gz")
    cols, _ = FE.table(exon_amd.Scan(path, "gff", gpu_parse=False))
    n = len(cols["start"])
    hi = {c: max(e for s, e in zip(cols["seqname"], cols["end"]) if s == c) for c in ("sq0", "sq1")}
    contigs = [("sq1", hi["sq1"] + 100), ("sq7", 500), ("sq0", hi["sq0"] - 5)]  # sq0's last rows are clipped; no row names sq7
    assert hi["sq0"] > 8  # (the fixture's features are a few bases long: windows of 3 cut them)
    totals, bases = check_file(ctx, path, "gff", contigs, 3, n, pileup=False)
    assert totals.tolist() == [n, 0, 0, 0]  # "sq7" was interned: no row is elsewhere, nothing is NULL
    span = sum(max(0, min(e, dict(contigs)[c]) - s + 1) for c, s, e in zip(cols["seqname"], cols["start"], cols["end"]))
    assert bases.sum() == span > 0
    woff = E.offsets(contigs, 3)
    assert bases[woff[1]:woff[2]].sum() == 0 and bases[:woff[1]].sum() > 0 and bases[woff[2]:].sum() > 0


CASES = [(1000, bsw.REFS), (50, bsw.REFS), (50, [("r1", 9000), ("r2", 1 << 20)])]  # (the short r1: the rows behind 9000 are clipped or outside)


@pytest.mark.parametrize("W,refs", CASES, ids=["1000", "50", "50-short-r1"])
@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_synthetic_records_and_the_flag_predicate(ctx, tmp_path, fmt, W, refs):
    recs = mixed(5000, seed=21)
    if refs is bsw.REFS:
        path = write(tmp_path, "wb", recs, fmt)
    elif fmt == "bam":
        path = str(tmp_path / "wb.bam")
        bsw.write_bam(path, recs, BGZIP, refs=refs)
    else:
        path = str(tmp_path / "wb.sam")
        bsw.write_sam(path, recs, refs=refs)
    contigs = header_contigs(path, fmt)
    assert contigs == [(n, ln) for n, ln in refs]
    totals, bases = check_file(ctx, path, fmt, contigs, W, len(recs))

    def from_records(kept):  # what the records' own dicts say: [pos, pos + reference-consuming cigar length - 1], clipped to the contig
        out = np.zeros_like(bases)
        woff = E.offsets(contigs, W)
        for i in kept:
            r = recs[i]
            if r["ref"] is None or r["pos"] < 1:
                continue
            end = min(r["pos"] + sum(n for n, op in r["cigar"] if op in bsw.REF_CONSUMING) - 1, refs[r["ref"]][1])
            for x in range(r["pos"], end + 1):
                out[woff[r["ref"]] + (x - 1) // W] += 1
        return out
    assert np.array_equal(bases, from_records(range(len(recs)))) and bases.sum() > 0
    # under a pushed-down flag / mapping-quality predicate only the kept rows are summed
    where = (1284, 0, 30)
    kept = FE.keep(recs, *where)
    rows = host_rows(path, fmt, contigs, where_flags=where)
    want_totals, want = E.expect(by_slot(contigs), W, *rows)
    assert np.array_equal(want, from_records(kept)) and 0 < want.sum() < bases.sum()
    for gpu_parse in (True, False):
        n, state, got, on = through_windows(ctx, [path], fmt, contigs, W, gpu_parse, where_flags=where)
        assert on == [gpu_parse] and n == [len(kept)] == [len(rows[0])]
        # (the device path masks the rows the predicate drops, which the plan then sees as NULL rows; the host reader never emits them:
        # `counted` and the sums agree, null_rows need not)
        assert state[0] == want_totals[0] and state[2:4].tolist() == want_totals[2:].tolist()
        assert np.array_equal(state[4:], E.expect_state(by_slot(contigs), W, *rows)[4:])
        assert np.array_equal(got, want)


def test_two_files_with_different_sq_orders_in_one_stream(ctx, tmp_path):
    a, b = mixed(3000, seed=31), mixed(2000, seed=32)
    flipped = [bsw.REFS[1], bsw.REFS[0]]  # in the second file id 0 is "r2"
    pa, pb = str(tmp_path / "a.sam"), str(tmp_path / "b.sam")
    bsw.write_sam(pa, a)
    bsw.write_sam(pb, b, refs=flipped)
    contigs, W = [("r2", 1 << 20), ("r1", 5000)], 1000
    one = [E.expect(by_slot(contigs), W, *host_rows(p, "sam", contigs)) for p in (pa, pb)]
    for gpu_parse in (True, False):
        rows, state, bases, on = through_windows(ctx, [pa, pb], "sam", contigs, W, gpu_parse)
        assert on == [gpu_parse, gpu_parse] and rows == [3000, 2000] and state[:4].sum() == 5000
        assert np.array_equal(bases, one[0][1] + one[1][1])
        assert state[:4].tolist() == (one[0][0] + one[1][0]).tolist()
    woff = E.offsets(contigs, W)
    assert one[1][1][:woff[1]].sum() > 0 and one[1][1][woff[1]:].sum() > 0
    # resolved by ids instead, the second file's rows would land on the other contig: the two files alone differ from each other
    alone = through_windows(ctx, [pb], "sam", contigs, W, True)[2]
    assert np.array_equal(alone, one[1][1]) and not np.array_equal(alone, one[0][1])


@pytest.mark.parametrize("fmt", ["bam", "sam"])
@pytest.mark.parametrize("gpu_parse", [True, False])
def test_reference_lengths_of_written_files(ctx, tmp_path, fmt, gpu_parse):
    path = write(tmp_path, "rl", mixed(50), fmt)
    scan = exon_amd.Scan(path, fmt, gpu_parse=gpu_parse)
    assert scan.reference_lengths() == [ln for _, ln in bsw.REFS] and scan.dictionary(2) == [n for n, _ in bsw.REFS]
    plan = ctx.plan_window_bases(list(zip(scan.dictionary(2), scan.reference_lengths())), 1 << 20, columns=COLS[fmt])
    st = plan.open()
    assert st.consume(scan) == 50
    assert scan.decoded_on_gpu()[0] == gpu_parse
    assert scan.reference_lengths() == [ln for _, ln in bsw.REFS]  # and behind the scan, whichever decoder took the records
    st.close(); plan.close(); scan.close()


def test_reference_lengths_of_other_sources(tmp_path):
    p = tmp_path / "no_ln.sam"
    p.write_text("@HD\tVN:1.6\n@SQ\tSN:a\tLN:77\n@SQ\tSN:b\n@SQ\tSN:c\tLN:5\n")
    scan = exon_amd.Scan(str(p), "sam", gpu_parse=False)
    assert scan.reference_lengths() == [77, 0, 5] and scan.dictionary(2) == ["a", "b", "c"]  # an @SQ without LN reports 0
    scan.close()
    cram = exon_amd.Scan(os.path.join(FX, "cram", "test_input_1_a.cram"), "cram", gpu_parse=False)
    assert len(cram.reference_lengths()) == len(cram.dictionary(2)) > 0 and min(cram.reference_lengths()) > 0
    cram.close()
    vcf = exon_amd.Scan(os.path.join(FX, "vcf", "index.vcf"), "vcf", gpu_parse=False)
    with pytest.raises(exon_amd.ExonHipError) as e:
        vcf.reference_lengths()
    assert e.value.code == EUNSUPPORTED
    vcf.close()
