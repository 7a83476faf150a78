"""CPU: a BAM / SAM scan with a pushed-down flag / mapping-quality predicate, Scan(..., where_flags=(mask, value[, mapq_min])) =
exon_hip_scan_set_flag_predicate, through the HOST readers (host/formats.h: bam_flag_hit on the raw record's fixed fields,
sam_flag_hit on fields 2 and 5 of the line) against tests/flag_predicate_expect.py, which works on the records' dicts alone, or
against the UNFILTERED scan's flag / mapping_quality columns filtered here with numpy.

Notes on the cases.  BAM and SAM have one host reader form each besides the indexed BAM reader (no slab-parallel parser as VCF
has; BAM inflates its BGZF blocks on several threads): the "large file" case runs a BAM of many BGZF blocks through that reader.
The SAM builder reads FLAG and MAPQ with C's atoi and so raises nothing for a field that is no number; the record is let through
and comes out as it does without a predicate, which is what the test pins -- a line of fewer than six fields (no MAPQ field at
all) is the malformed operand the builder does raise on, with the same text either way.  The fixture test.sam holds ONE record and
every mapping_quality of test.bam is NULL: the triples for test.bam keep a strict part of its 61 rows on the flag alone (and a
fourth, with a mapq_min, keeps none of them); on test.sam a count can only be 0 or 1, and both are pinned."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_sam_writer as bsw
import exon_amd
import flag_predicate_expect as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "ref_fixtures")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
EUNSUPPORTED, ESTATE = -4, -5

FLAGS = [0, 4, 16, 256, 1024, 1284, 0xFFFF]
MAPQS = [0, 29, 30, 254, 255]
MAPQ_MINS = [-1, 0, 30, 255, 256]
PAIRS = [(0, 0), (4, 0), (4, 4), (1284, 0), (4, 5)] + [(0xFFFF, f) for f in FLAGS]


def write(tmp, name, recs, fmt):
    """the records as a BAM (BGZF) or a SAM in one of its three containers: "sam", "sam.gz" (one gzip member), "sam.bgz" (BGZF)"""
    if fmt == "bam":
        p = str(tmp / (name + ".bam"))
        bsw.write_bam(p, recs, BGZIP)
        return p
    p = str(tmp / (name + ".sam"))
    bsw.write_sam(p, recs)
    if fmt == "sam.gz":
        g = str(tmp / (name + ".plain.sam.gz"))
        with gzip.open(g, "wb") as f:
            f.write(open(p, "rb").read())
        return g
    if fmt == "sam.bgz":
        g = str(tmp / (name + ".sam.gz"))
        subprocess.check_call([BGZIP, p, g, "6"], stdout=subprocess.DEVNULL)
        return g
    return p


def scan(path, fmt, where_flags=None, project=E.PROJECT, **kw):
    s = exon_amd.Scan(path, fmt[:3], project=project, where_flags=where_flags, **kw)
    cols, lens = E.table(s)
    rows = s.rows()
    s.close()
    return cols, lens, rows


def check(got, want, n_kept, batch_size=8192):
    cols, lens, rows = got
    assert rows == n_kept == sum(lens) and all(0 < n <= batch_size for n in lens)
    assert cols == (want if n_kept else {})


# ---- the truth table ----------------------------------------------------------------------------------------------------------------------
def table_records():
    return [E.read(i, flag=f, mapq=q) for i, (f, q) in enumerate((f, q) for f in FLAGS for q in MAPQS)]


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_truth_table(tmp_path, fmt):
    recs = table_records()
    path = write(tmp_path, "t", recs, fmt)
    seen = set()
    for mask, value in PAIRS:
        for mapq_min in MAPQ_MINS:
            kept = E.keep(recs, mask, value, mapq_min)
            seen.add(len(kept))
            check(scan(path, fmt, (mask, value, mapq_min)), E.columns(recs, fmt == "sam", kept), len(kept))
    assert 0 in seen and len(recs) in seen and len(seen) > 4


def test_the_table_pins_the_cases_the_rule_is_about():
    """the expectation itself: a value with bits outside the mask and a mapq_min above 255 keep nothing, a NULL mapping_quality passes
    no mapq_min >= 0 (not even 0, not 255) and any mapq_min < 0, mask 0 looks at no flag bit"""
    recs = table_records()
    n = len(recs)
    assert E.keep(recs, 4, 5) == [] and E.keep(recs, 0, 0, 256) == [] and E.keep(recs, 0, 0) == list(range(n))
    null = [i for i, r in enumerate(recs) if r["mapq"] == 255]
    assert len(null) == len(FLAGS) and E.keep(recs, 0, 0, 0) == [i for i in range(n) if i not in null] and E.keep(recs, 0, 0, 255) == []
    assert [recs[i]["mapq"] for i in E.keep(recs, 0xFFFF, 1284, 30)] == [30, 254]
    assert sorted({recs[i]["flag"] for i in E.keep(recs, 1284, 0)}) == [0, 16]
    assert E.keep(recs, 4, 0, -7) == E.keep(recs, 4, 0, -1) == E.keep(recs, 4, 0)


# ---- every column of the emitted rows --------------------------------------------------------------------------------------------------------
def mixed(n, seed=3, l_seq=None):
    rng = np.random.default_rng(seed)
    flag = rng.choice([0, 4, 16, 83, 147, 256, 1024, 1040, 2048], n)
    mapq = rng.choice([0, 10, 29, 30, 60, 255], n)
    return [E.read(i, flag=int(flag[i]), mapq=int(mapq[i]), l_seq=l_seq, ref=None if i % 17 == 3 else i % 2, pos=0 if i % 19 == 7 else 100 + 3 * i) for i in range(n)]


@pytest.mark.parametrize("batch_size", [1, 8192])
@pytest.mark.parametrize("fmt", ["bam", "sam", "sam.gz", "sam.bgz"])
def test_every_column_of_the_emitted_rows(tmp_path, fmt, batch_size):
    recs = mixed(300)
    path = write(tmp_path, "m", recs, fmt)
    whole, _, rows = scan(path, fmt, batch_size=batch_size)
    assert rows == len(recs) and whole == E.columns(recs, fmt != "bam", range(len(recs)))
    for where in ((4, 0), (1284, 0, 30), (16, 16, 0), (0, 0, 60)):
        kept = E.keep(recs, *where)
        assert 0 < len(kept) < len(recs)
        check(scan(path, fmt, where, batch_size=batch_size), E.take(whole, kept), len(kept), batch_size)


def test_a_bam_of_many_bgzf_blocks(tmp_path):
    """~1.6 MB of records, some 25 BGZF blocks: the reader's inflate threads run ahead of the record loop that filters"""
    recs = mixed(8000, seed=8, l_seq=100)
    path = write(tmp_path, "big", recs, "bam")
    assert os.path.getsize(path + ".u") > 20 * 65280
    whole, _, rows = scan(path, "bam", project=("name", "sequence"))
    assert rows == len(recs)
    kept = E.keep(recs, 1284, 0, 30)
    assert 1000 < len(kept) < 4000
    got = scan(path, "bam", (1284, 0, 30), project=("name", "sequence"))
    check(got, E.take(whole, kept), len(kept))
    assert got[0] == E.columns(recs, False, kept, ("name", "sequence"))


# ---- region AND predicate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bam", "sam", "sam.bgz"])
def test_region_and_predicate_unindexed(tmp_path, fmt):
    recs = mixed(400, seed=5)
    path = write(tmp_path, "r", recs, fmt)
    whole, _, _ = scan(path, fmt)
    for region, rg in (("r1:300-700", ("r1", 300, 700)), ("r2:1-500", ("r2", 1, 500)), ("r1:5000-6000", ("r1", 5000, 6000))):
        for where in ((4, 0), (1284, 0, 30)):
            both, alone = E.keep(recs, *where, region=rg), E.keep(recs, 0, 0, region=rg)
            assert len(both) < len(alone) or not alone
            check(scan(path, fmt, where, region=region), E.take(whole, both), len(both))
    assert E.keep(recs, 4, 0, region=("r1", 300, 700))


def fixture_columns(path, fmt, **kw):
    s = exon_amd.Scan(path, fmt, **kw)
    cols, _ = E.table(s)
    s.close()
    return cols


def numpy_keep(cols, mask, value, mapq_min=-1, region=None):
    """the kept rows from an unfiltered scan's columns"""
    flag = np.array(cols["flag"], np.int64)
    ok = (flag & mask) == value
    if mapq_min >= 0:
        ok &= np.array([q is not None and q >= mapq_min for q in cols["mapping_quality"]], bool)
    if region:
        name, a, b = region
        ok &= np.array([r == name and s is not None and s <= b and a <= e for r, s, e in zip(cols["reference"], cols["start"], cols["end"])], bool)
    return np.flatnonzero(ok).tolist()


def test_region_and_predicate_indexed_on_the_fixture():
    path = os.path.join(FX, "bam", "test.bam")
    whole = fixture_columns(path, "bam", project=E.PROJECT)
    for region, rg in (("chr1:12205000-12212000", ("chr1", 12205000, 12212000)), ("chr1", ("chr1", 1, 1 << 40))):
        for where in ((64, 64), (128, 128), (512, 0)):
            both, alone = numpy_keep(whole, *where, region=rg), numpy_keep(whole, 0, 0, region=rg)
            assert 0 < len(both) < len(alone)
            for use_index in (True, False):
                check(scan(path, "bam", where, region=region, use_index=use_index), E.take(whole, both), len(both))


# ---- errors and refusals ----------------------------------------------------------------------------------------------------------------------
def sam_with(tmp_path, name, lines):
    p = tmp_path / name
    p.write_text("@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in bsw.REFS) + "".join(ln + "\n" for ln in lines))
    return str(p)


@pytest.mark.parametrize("where", [(4, 4), (4, 0), (0, 0, 30)])
def test_a_malformed_operand_is_the_builders(tmp_path, where):
    recs = [E.read(i, flag=(0, 4)[i % 2], mapq=(10, 40)[i // 2 % 2]) for i in range(12)]
    lines = [bsw.sam_line(r) for r in recs]

    def outcome(path, where_flags):
        try:
            return scan(path, "sam", where_flags)
        except exon_amd.ExonHipError as e:
            return e.code, str(e)

    # a line that ends before its MAPQ field: the builder's error, with the predicate and without, word for word
    short = sam_with(tmp_path, "short.sam", lines[:5] + ["\t".join(lines[5].split("\t")[:4])] + lines[6:])
    plain, pushed = outcome(short, None), outcome(short, where)
    assert isinstance(plain[0], int) and plain[0] < 0 and "fewer than 6 fields" in plain[1] and pushed == plain
    # a FLAG / MAPQ that is no number: the record goes through to the builder and comes out as it does without a predicate
    for field, text in ((1, "4x"), (1, ""), (1, "-4"), (1, "65536"), (4, "q"), (4, "256"), (4, "3 ")):
        f = lines[5].split("\t")
        f[field] = text
        path = sam_with(tmp_path, f"bad{field}.sam", lines[:5] + ["\t".join(f)] + lines[6:])
        whole = outcome(path, None)
        assert whole[2] == len(recs)
        kept = sorted(set(E.keep(recs, *where)) | {5})
        check(outcome(path, where), E.take(whole[0], kept), len(kept))


@pytest.mark.parametrize("fmt,rel", [("vcf", "vcf/index.vcf"), ("vcf", "vcf/index.vcf.gz"), ("bcf", "bcf/index.bcf"), ("fastq", "fastq/test.fastq"),
                                     ("gff", "gff/ecoli.gff"), ("cram", "cram/0500_mapped.cram")])
def test_other_formats_are_refused(fmt, rel):
    s = exon_amd.Scan(os.path.join(FX, rel), fmt)
    with pytest.raises(exon_amd.ExonHipError) as e:
        s.set_flag_predicate(4, 0)
    assert e.value.code == EUNSUPPORTED
    s.close()
    with pytest.raises(exon_amd.ExonHipError) as e:  # the constructor form closes the scan it opened
        exon_amd.Scan(os.path.join(FX, rel), fmt, where_flags=(4, 0))
    assert e.value.code == EUNSUPPORTED


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_call_order_and_the_value_predicate_stays_refused(tmp_path, fmt):
    recs = mixed(50, seed=2)
    path = write(tmp_path, "o", recs, fmt)
    s = exon_amd.Scan(path, fmt, batch_size=8)
    with pytest.raises(exon_amd.ExonHipError) as e:  # exon_hip_scan_set_predicate is VCF's
        s.set_predicate(1, ">=", 30.0)
    assert e.value.code == EUNSUPPORTED
    assert s.next_raw() is not None
    with pytest.raises(exon_amd.ExonHipError) as e:
        s.set_flag_predicate(4, 0)
    assert e.value.code == ESTATE
    s.close()
    # a second call replaces the first
    s = exon_amd.Scan(path, fmt, where_flags=(4, 4))
    s.set_flag_predicate(16, 16, 30)
    cols, _ = E.table(s)
    kept = E.keep(recs, 16, 16, 30)
    assert kept and kept != E.keep(recs, 4, 4) and s.rows() == len(kept) and cols == E.columns(recs, fmt == "sam", kept, ())
    s.close()


# ---- the reference's fixtures -----------------------------------------------------------------------------------------------------------------
def test_the_fixtures():
    bam = os.path.join(FX, "bam", "test.bam")
    whole = fixture_columns(bam, "bam", project=E.PROJECT)
    n = len(whole["flag"])
    assert n == 61 and whole["mapping_quality"] == [None] * n
    for where in ((64, 64, -1), (128, 128, -1), (512, 0, -1), (16, 16, -1)):
        kept = numpy_keep(whole, *where)
        assert 0 < len(kept) < n
        check(scan(bam, "bam", where), E.take(whole, kept), len(kept))
    assert numpy_keep(whole, 0, 0, 0) == []  # every mapping_quality is NULL
    check(scan(bam, "bam", (0, 0, 0)), {}, 0)
    sam = os.path.join(FX, "sam", "test.sam")
    whole = fixture_columns(sam, "sam", project=E.PROJECT)
    assert whole["flag"] == [99] and whole["mapping_quality"] == [0]
    for where in ((64, 64, -1), (99, 99, 0), (4, 4, -1), (64, 64, 1)):
        kept = numpy_keep(whole, *where)
        check(scan(sam, "sam", where), E.take(whole, kept), len(kept))
    assert [len(numpy_keep(whole, *w)) for w in ((64, 64, -1), (99, 99, 0), (4, 4, -1), (64, 64, 1))] == [1, 1, 0, 0]


# ---- exon-hip-cli -----------------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(ROOT, "exon_amd", "bin", "exon-hip-cli")


def cli_count(sql, **env):
    r = subprocess.run([CLI, "-q", "-c", sql], capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
    assert r.returncode == 0, r.stderr
    return int([line for line in r.stdout.splitlines() if line.startswith("|")][-1].strip("| "))


def test_cli_puts_the_conjuncts_into_the_scan(tmp_path):
    """SELECT COUNT(*) ... WHERE flag & M = V [AND CAST(mapping_quality AS INT) >= q] without GROUP BY, alone and ANDed with
    bam_region_filter (EXON_HIP_GPU_PARSE=0: the host reader counts)"""
    recs = mixed(400, seed=6)
    for fmt in ("bam", "sam"):
        src = f"{fmt}_scan('{write(tmp_path, 'c', recs, fmt)}')"
        assert cli_count(f"SELECT COUNT(*) FROM {src} WHERE flag & 4 = 0", EXON_HIP_GPU_PARSE="0") == len(E.keep(recs, 4, 0))
        assert cli_count(f"SELECT COUNT(*) FROM {src} WHERE flag & 1284 = 0 AND CAST(mapping_quality AS INT) >= 30", EXON_HIP_GPU_PARSE="0") == len(E.keep(recs, 1284, 0, 30))
        assert cli_count(f"SELECT COUNT(*) FROM {src} WHERE CAST(mapping_quality AS INT) > 29 AND flag & 16 = 16", EXON_HIP_GPU_PARSE="0") == len(E.keep(recs, 16, 16, 30))
        both = E.keep(recs, 4, 0, 10, region=("r1", 300, 900))
        assert 0 < len(both) < len(E.keep(recs, 0, 0, region=("r1", 300, 900)))
        sql = f"SELECT COUNT(*) FROM {src} WHERE bam_region_filter('r1:300-900', reference, start, end) AND flag & 4 = 0 AND CAST(mapping_quality AS INT) >= 10"
        assert cli_count(sql, EXON_HIP_GPU_PARSE="0") == len(both)
        sql = f"SELECT COUNT(*) FROM {src} WHERE flag & 4 = 0 AND CAST(mapping_quality AS INT) >= 10 AND bam_region_filter('r1:300-900', reference, start, end) = true"
        assert cli_count(sql, EXON_HIP_GPU_PARSE="0") == len(both)
