"""CPU: a VCF scan with a pushed-down value predicate, Scan(..., where=(column, op, literal)) = exon_hip_scan_set_predicate, through the
HOST reader (host/formats.h: vcf_value_hit in the sequential, the indexed and the slab-parallel reader) against
tests/scan_predicate_expect.py, which splits the lines itself and compares on explicit totalOrder keys.

Two notes on the cases.  The operator / NULL table scans project id, ref, alt WITHOUT `info`: its rows include `AF=.`, and the
`info` text column refuses a key without a value for every row it builds (the reference's builder panics there), whatever the
predicate.  The two fused-plan cases run the host reader too (gpu_parse=False) but a plan lives on a device context, so they alone
carry the gpu mark."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import scan_predicate_expect as E
from bgzf_index_writer import write_tabix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "ref_fixtures")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
EINVAL, EUNSUPPORTED, ESTATE = -1, -4, -5
PROJECT = ("id", "ref", "alt", "info")


def table(scan):
    """every batch of a Scan -> (columns as lists, the batches' lengths)"""
    cols, lens = {}, []
    for b in scan:
        lens.append(len(b))
        for i in range(b.type.num_fields):
            cols.setdefault(b.type.field(i).name, []).extend(b.field(i).to_pylist())
    return cols, lens


def write(tmp_path, name, lines, comp="plain", pad=None):
    """the file in one of the three containers: plain text, one gzip member, BGZF"""
    text = E.header(pad) + "".join(ln + "\n" for ln in lines)
    p = tmp_path / (name + ".vcf")
    p.write_text(text)
    if comp == "gz":
        g = tmp_path / (name + ".plain.vcf.gz")
        with gzip.open(g, "wb") as f:
            f.write(text.encode())
        return str(g)
    if comp == "bgzf":
        g = tmp_path / (name + ".vcf.gz")
        subprocess.check_call([BGZIP, str(p), str(g), "6"])
        return str(g)
    return str(p)


def scan_where(path, where, project=PROJECT, **kw):
    s = exon_amd.Scan(path, "vcf", info_field=E.INFO_FIELD, project=project, where=where, **kw)
    cols, lens = table(s)
    rows = s.rows()
    s.close()
    return cols, lens, rows


def check(got, lines, wants, kept, project=PROJECT, batch_size=8192):
    cols, lens, rows = got
    assert rows == len(kept) == sum(lens) and all(0 < n <= batch_size for n in lens)
    if kept:
        assert E.same(cols, E.columns(lines, wants, kept, project))
    else:
        assert cols == {}


# ---- columns and operators: the table ----------------------------------------------------------------------------------------------
QUALS, AF_INFOS, DP_INFOS, LITERALS, table_lines = E.QUALS, E.AF_INFOS, E.DP_INFOS, E.LITERALS, E.table_lines


@pytest.mark.parametrize("comp", ["plain", "gz", "bgzf"])
@pytest.mark.parametrize("what", ["qual", "AF", "DP"])
def test_operator_literal_and_null_table(tmp_path, what, comp):
    lines = table_lines(what)
    path = write(tmp_path, "t", lines, comp)
    project = ("id", "ref", "alt")
    for op in E.OPS:
        for lit in LITERALS[what]:
            kept = E.keep(lines, what, op, lit)
            check(scan_where(path, (E.COLUMN[what], op, lit), project), lines, None, kept, project)


def test_the_table_pins_the_cases_the_rule_is_about():
    """the expectation itself, on the rows the issue names: f32(0.01) is below 0.01, 16777217 is exact on the Integer key and rounds on
    a Float column, -0.0 sorts below +0.0, NaN is above everything and equal to itself, NULL never passes"""
    q = table_lines("qual")
    assert QUALS.index("0.01") not in E.keep(q, "qual", ">=", 0.01) and QUALS.index("0.01") in E.keep(q, "qual", "<", 0.01)
    assert QUALS.index("16777217") in E.keep(q, "qual", "=", 16777216.0)
    assert QUALS.index("-0.0") in E.keep(q, "qual", "=", -0.0) and QUALS.index("0") not in E.keep(q, "qual", "=", -0.0)
    assert E.keep(q, "qual", "=", float("nan")) == [QUALS.index("nan")] and E.keep(q, "qual", ">", float("nan")) == []
    assert len(E.keep(q, "qual", "<", float("nan"))) == len(QUALS) - 2  # all but NULL and the NaN
    d = table_lines("DP")
    assert E.keep(d, "DP", "=", 16777217.0) == [0] and E.keep(d, "DP", ">", 16777217.0) == [2, 10]
    assert E.keep(d, "DP", "=", 5.0) == [DP_INFOS.index("DP=5;DP=50")]
    for op in E.OPS:  # NULL under every operator, != included
        assert not {DP_INFOS.index("DP=."), DP_INFOS.index("AF=0.5"), DP_INFOS.index(".")} & set(E.keep(d, "DP", op, 1.0))
        assert QUALS.index(".") not in E.keep(q, "qual", op, 1.0)


# ---- every column of the emitted rows, containers, batch sizes, row counts ------------------------------------------------------------
def mixed(n, seed=5, pos0=True, chrom=None):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 60, n)
    made = [E.line(i, "." if i % 13 == 4 else str(int(q[i])) + (".5" if i % 2 else ""), pos0=pos0, chrom=chrom(i) if chrom else "1") for i in range(n)]
    return [m[0] for m in made], [m[1] for m in made]


@pytest.mark.parametrize("batch_size", [1, 7, 8192])
@pytest.mark.parametrize("n", [0, 1, 2, 1000])
def test_every_column_of_the_emitted_rows(tmp_path, n, batch_size):
    lines, wants = mixed(n)
    for comp in ("plain", "gz", "bgzf") if n == 1000 or batch_size == 7 else ("plain",):
        path = write(tmp_path, f"m{comp}", lines, comp)
        for where, what in (((2, ">=", 30.0), "qual"), ((4, ">", 0.01), "AF"), ((5, "<=", 50000.0), "DP")):
            kept = E.keep(lines, what, where[1], where[2])
            check(scan_where(path, where, batch_size=batch_size), lines, wants, kept, batch_size=batch_size)
    if n == 1000:
        assert 300 < len(E.keep(lines, "qual", ">=", 30.0)) < 700


def test_the_slab_parallel_reader_applies_it_too(tmp_path):
    """a file of more than 8 MB without projected text columns goes through the reader's parse pipeline (parse_vcf_slab)"""
    n = 150_000
    lines, _ = mixed(n, seed=9)
    p = tmp_path / "big.vcf"
    p.write_text(E.header() + "".join(ln + "\n" for ln in lines))
    assert os.path.getsize(p) > (8 << 20)
    kept = E.keep(lines, "AF", ">", 0.01)
    s = exon_amd.Scan(str(p), "vcf", info_field="AF,DP", where=(4, ">", 0.01))
    cols, lens = table(s)
    assert s.rows() == len(kept) == sum(lens)
    s.close()
    want = E.columns(lines, None, kept, ())
    for k in ("pos", "qual", "filter", "info.AF", "info.DP"):
        assert cols[k] == want[k], k


# ---- region AND predicate --------------------------------------------------------------------------------------------------------------
def test_region_and_predicate_unindexed_and_indexed(tmp_path):
    lines, wants = mixed(3000, seed=11, pos0=False, chrom=lambda i: "1" if i < 2000 else "2")
    plain = write(tmp_path, "r", lines, "plain")
    bg = write(tmp_path, "r", lines, "bgzf")
    assert write_tabix(bg) == 3000
    for region, rg in (("1:500-1500", ("1", 500, 1500)), ("2:2001-2500", ("2", 2001, 2500)), ("2", ("2", 1, 1 << 62)), ("1:5000-6000", ("1", 5000, 6000))):
        kept = E.keep(lines, "qual", ">=", 30.0, rg)
        assert len(kept) < len(E.keep(lines, "qual", ">=", 30.0)) and (len(kept) > 100 or rg[1] == 5000)
        for path, use_index in ((plain, False), (bg, False), (bg, True)):
            check(scan_where(path, (2, ">=", 30.0), region=region, use_index=use_index, batch_size=64), lines, wants, kept, batch_size=64)
    kept = E.keep(lines, "DP", ">", 90000.0, ("1", 1, 1000))
    check(scan_where(bg, (5, ">", 90000.0), region="1:1-1000", use_index=True), lines, wants, kept)


# ---- a malformed value is the builder's error ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad, where", [(("1x", None), (2, ">=", 30.0)), (("50", "AF=0.5.5"), (4, ">", 0.01)), (("50", "DP=1e3"), (5, ">", 1.0))])
def test_a_malformed_operand_raises_the_readers_own_error(tmp_path, bad, where):
    lines = [E.line(i, "50", info="AF=0.5;DP=5")[0] for i in range(5)]
    lines[3] = E.line(3, bad[0], info=bad[1] or "AF=0.5;DP=5")[0]
    path = write(tmp_path, "bad", lines)
    texts = []
    for w in (None, where):
        s = exon_amd.Scan(path, "vcf", info_field=E.INFO_FIELD, where=w)
        with pytest.raises(exon_amd.ExonHipError) as e:
            table(s)
        texts.append((e.value.code, str(e.value)))
        s.close()
    assert texts[0] == texts[1] and texts[0][0] == EINVAL


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_status_code(tmp_path, monkeypatch):
    lines, _ = mixed(50, pos0=False)
    path = write(tmp_path, "x", lines)
    fields = "AF,DP,DB,XS,AL"  # columns 4 .. 8: Float, Integer, Flag, String (dictionary), list

    def refused(column, op, lit=1.0, **kw):
        s = exon_amd.Scan(path, "vcf", info_field=fields, **kw)
        with pytest.raises(exon_amd.ExonHipError) as e:
            s.set_predicate(column, op, lit)
        s.close()
        return e.value.code, str(e.value)

    for column, word in ((1, "Int64"), (0, "ictionary"), (3, "ictionary"), (6, "Flag"), (7, "ictionary"), (8, "ist")):
        code, text = refused(column, ">")
        assert code == EUNSUPPORTED and word in text, (column, text)
    for column in (-1, 9, 100):
        assert refused(column, ">")[0] == EINVAL
    for op in (-1, 6):
        assert refused(2, op)[0] == EINVAL
    with pytest.raises(KeyError):
        exon_amd.Scan(path, "vcf", where=(2, "=>", 1.0))
    bam = exon_amd.Scan(os.path.join(FX, "bam", "test.bam"), "bam")
    with pytest.raises(exon_amd.ExonHipError) as e:
        bam.set_predicate(1, ">", 1.0)
    assert e.value.code == EUNSUPPORTED
    bam.close()
    with pytest.raises(exon_amd.ExonHipError) as e:  # the constructor's form closes the scan and raises the same
        exon_amd.Scan(os.path.join(FX, "bam", "test.bam"), "bam", where=(1, ">", 1.0))
    assert e.value.code == EUNSUPPORTED
    # after the first batch
    s = exon_amd.Scan(path, "vcf", batch_size=8)
    assert s.next_raw() is not None
    with pytest.raises(exon_amd.ExonHipError) as e:
        s.set_predicate(2, ">", 1.0)
    assert e.value.code == ESTATE
    s.close()
    # the reference's unfiltered tail and a second conjunct
    monkeypatch.setenv("EXON_HIP_REFERENCE_QUIRKS", "1")
    code, _ = refused(2, ">", region="1:1-10")
    assert code == EUNSUPPORTED
    s = exon_amd.Scan(path, "vcf", where=(2, ">", 1.0))  # (without a region the switch changes nothing)
    s.close()


def test_a_second_call_replaces_the_first(tmp_path):
    lines, wants = mixed(200)
    path = write(tmp_path, "x", lines)
    s = exon_amd.Scan(path, "vcf", info_field=E.INFO_FIELD, project=PROJECT, where=(2, ">=", 30.0))
    s.set_predicate(5, "<", 1000.0)
    cols, lens = table(s)
    kept = E.keep(lines, "DP", "<", 1000.0)
    assert kept != E.keep(lines, "qual", ">=", 30.0)
    check((cols, lens, s.rows()), lines, wants, kept)
    s.close()


# ---- fused plans over such a scan, host reader ------------------------------------------------------------------------------------------
def k2_count(ctx, path, where, gpu_parse, region=(1, None)):
    scan = exon_amd.Scan(path, "vcf", info_field="AF,DP", gpu_parse=gpu_parse, where=where)
    plan = ctx.plan_region_count(scan.intern(0, "1"), region[0], region[1])
    st = plan.open()
    rows = st.consume(scan)
    counts, _ = st.finish()
    on = scan.decoded_on_gpu()[0]
    st.close(); plan.close(); scan.close()
    return rows, int(counts[0]), on


def k4_groups(ctx, path, where, gpu_parse):
    """WHERE info.AF > 0.01 [AND where] ... AVG(qual) GROUP BY filter -> {filter: (count(qual), count(*), sum(qual))} of the groups with rows"""
    scan = exon_amd.Scan(path, "vcf", info_field="AF,DP", gpu_parse=gpu_parse, where=where)
    plan = ctx.plan_cmp_avg_by_group(">", 0.01, 8, columns=(4, 2, 3))
    st = plan.open()
    rows = st.consume(scan)
    counts, sums = st.finish()
    names = scan.dictionary(3)
    res = {names[g]: (int(counts[g]), int(counts[8 + g]), float(sums[g])) for g in range(len(names)) if counts[8 + g]}
    on = scan.decoded_on_gpu()[0]
    st.close(); plan.close(); scan.close()
    return rows, res, on


def k4_numpy(lines, kept):
    """the same from the lines: rows `kept` (what the scan emits) that pass AF > 0.01"""
    res = {}
    for i in kept:
        f = lines[i].split("\t")
        if not E.passes(E.typed(f, "AF"), ">", 0.01):
            continue
        name = "" if f[6] == "." else f[6]
        cn, cr, s = res.get(name, (0, 0, 0.0))
        q = E.typed(f, "qual")
        res[name] = (cn + (q is not None), cr + 1, s + (float(np.float64(q)) if q is not None else 0.0))
    return res


@pytest.mark.gpu
def test_k2_plan_counts_the_kept_rows_host_reader(ctx, tmp_path):
    lines, _ = mixed(5000, seed=3)
    path = write(tmp_path, "k2", lines)
    kept = E.keep(lines, "qual", ">=", 30.0)
    in_region = [i for i in kept if int(lines[i].split("\t")[1]) >= 1]  # K2: chrom = '1' AND pos >= 1; POS 0 is NULL
    rows, count, on = k2_count(ctx, path, (2, ">=", 30.0), False)
    assert rows == len(kept) and count == len(in_region) and not on and 0 < len(in_region) < len(kept)


@pytest.mark.gpu
def test_k4_plan_gets_a_second_conjunct_host_reader(ctx, tmp_path):
    lines, _ = mixed(5000, seed=4)
    path = write(tmp_path, "k4", lines)
    kept = E.keep(lines, "DP", "<", 50000.0)
    want = k4_numpy(lines, kept)
    rows, got, on = k4_groups(ctx, path, (5, "<", 50000.0), False)
    assert rows == len(kept) and not on and got.keys() == want.keys() and len(want) == 4
    assert want != k4_numpy(lines, range(len(lines)))
    for k in want:
        assert got[k][:2] == want[k][:2] and got[k][2] == pytest.approx(want[k][2], rel=1e-9)
