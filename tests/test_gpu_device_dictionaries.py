"""The dictionaries the device parsers build (VCF FILTER lists and String INFO values: gpu_parse.hip k_parse_lines /
k_info_string_ids / k_assign_filters / k_remap_filters; BCF FILTER lists: bcf_parse.hip FilterLists) at their limits:
EXON_HIP_MAX_GROUPS (4096) ids, a 1 MiB text pool, the slab in which the table overflows, many rows inserting one new value
at once, values that differ in one byte, and two different texts with the same 64-bit FNV-1a hash.  The reference is the
text each test writes itself: every row's value must come back under its own name, in batches and in GROUP BY aggregates,
from the device up to capacity and from the host reader beyond it (a hand-over, never an error)."""
import math
import os

import numpy as np
import pytest

import exon_amd
import vcf_bcf_writer as vbw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
CAP = 4096  # EXON_HIP_MAX_GROUPS
POOL = 1 << 20  # the device dictionary's text pool

# Two distinct strings, legal as FILTER IDs and as INFO values, with the same fnv1a (| 1): found by a distinguished-point rho
# search over x -> fnv1a(hex16(x)).
COLLIDING = ("ec66b0c02bb97703", "77f933ec87d772e9")
COLLIDING_HASH = 0xCC889E799BBC46AB

HEAD = ('##fileformat=VCFv4.3\n##contig=<ID=1>\n##INFO=<ID=AF,Number=1,Type=Float,Description="x">\n'
        '##INFO=<ID=CSQ,Number=1,Type=String,Description="x">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n')


def fnv1a(b):
    """the device dictionaries' key: 64-bit FNV-1a with bit 0 set (0 marks an empty slot)"""
    h = 0xCBF29CE484222325
    for c in b:
        h = ((h ^ c) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h | 1


def test_colliding_pair_is_distinct_and_hashes_alike():
    a, b = (s.encode() for s in COLLIDING)
    assert a != b and len(a) == len(b) == 16
    assert fnv1a(a) == fnv1a(b) == COLLIDING_HASH
    assert all(c in b"0123456789abcdef" for c in a + b)  # no ';', '=', ',', whitespace: a FILTER ID and an INFO value alike


def _af(i):
    return "0.001" if i % 13 == 0 else "0.5"  # 0.001 does not pass "> 0.01"


def _qual(i):
    return None if i % 7 == 3 else (i % 1999) / 2  # halves: exact in f32


def write_case(tmp_path, mode, vals, name="t"):
    """vals: per row the FILTER list text ("" = '.') for modes "filter" / "bcf", the CSQ value (None = no value) for "string".
    Returns (path, format, info_field, column)."""
    if mode == "bcf":
        ids = sorted({f for v in vals if v for f in v.split(";")} - {"PASS"})
        rows = [dict(chrom="1", pos=i + 1, qual=_qual(i), filter=v.split(";") if v else [], info={"AF": float(_af(i))})
                for i, v in enumerate(vals)]
        path = tmp_path / f"{name}.bcf"
        vbw.write_bcf(path, rows, BGZIP, filters=ids)
        return path, "bcf", "AF", 3
    lines = [HEAD]
    for i, v in enumerate(vals):
        q = "." if _qual(i) is None else f"{_qual(i):.1f}"
        if mode == "string":
            filt, info = "PASS", f"AF={_af(i)}" + ("" if v is None else f";CSQ={v}")
        else:
            filt, info = v or ".", f"AF={_af(i)}"
        lines.append(f"1\t{i + 1}\t.\tA\tC\t{q}\t{filt}\t{info}\n")
    path = tmp_path / f"{name}.vcf"
    path.write_text("".join(lines))
    return path, "vcf", ("AF,CSQ" if mode == "string" else "AF"), (5 if mode == "string" else 3)


def check_batches(ctx, case, vals, on_gpu):
    """every row's dictionary[id] is the written value (NULL where none was written), in file order; no dictionary repeats a
    name; on the device path the dictionary is exactly the distinct values"""
    path, fmt, info_field, col = case
    s = exon_amd.Scan(str(path), fmt, info_field=info_field, gpu_parse=True).bind_ctx(ctx)
    got, last = [], []
    for b in s:
        a = b.field(col)
        d = a.dictionary.to_pylist()
        assert len(set(d)) == len(d), "a batch's dictionary repeats a name"
        got.extend(None if i is None else d[i] for i in a.indices.to_pylist())
        last = d
    flags = s.decoded_on_gpu()
    names = s.dictionary(col)
    s.close()
    assert len(got) == len(vals)
    bad = next((i for i, (g, w) in enumerate(zip(got, vals)) if g != w), None)
    assert bad is None, f"row {bad}: {got[bad]!r} instead of {vals[bad]!r}"
    assert flags[0] == on_gpu, f"decoded on the GPU: {flags[0]}, expected {on_gpu}"
    if on_gpu:
        distinct = {v for v in vals if v is not None}
        assert len(last) == len(distinct) and set(last) == distinct
        assert len(names) == len(distinct) and set(names) == distinct


def check_aggregate(ctx, case, vals, on_gpu):
    """COUNT(*), COUNT(qual), SUM(qual) WHERE AF > 0.01 GROUP BY the value (NULL = the key "") = the same sums over the written rows"""
    path, fmt, info_field, col = case
    want = {}
    for i, v in enumerate(vals):
        if _af(i) != "0.5":
            continue
        w = want.setdefault("" if v is None else v, [0, 0, []])
        w[0] += 1
        if _qual(i) is not None:
            w[1] += 1
            w[2].append(float(np.float32(_qual(i))))
    n_groups = max(64, len({v for v in vals}) + 8)  # beyond 4096: the global tier
    scan = exon_amd.Scan(str(path), fmt, info_field=info_field, gpu_parse=True)
    plan = ctx.plan_cmp_avg_by_group(">", 0.01, n_groups, columns=(4, 2, col))
    st = plan.open()
    rows = st.consume(scan)
    counts, sums = st.finish()
    names = scan.dictionary(col)
    flags = scan.decoded_on_gpu()
    st.close()
    plan.close()
    scan.close()
    assert rows == len(vals)
    assert len(names) <= n_groups and len(set(names)) == len(names), "the dictionary repeats a name"
    got = {names[g]: (int(counts[n_groups + g]), int(counts[g]), float(sums[g])) for g in range(len(names)) if counts[n_groups + g]}
    assert got.keys() == want.keys()
    for k, (n, nq, qs) in want.items():
        assert got[k][:2] == (n, nq), k
        assert got[k][2] == pytest.approx(math.fsum(qs), rel=1e-12), k
    assert flags[0] == on_gpu, f"decoded on the GPU: {flags[0]}, expected {on_gpu}"


def check_both(ctx, tmp_path, mode, vals, on_gpu, agg_on_gpu=None):
    case = write_case(tmp_path, mode, vals)
    check_batches(ctx, case, vals, on_gpu)
    check_aggregate(ctx, case, vals, on_gpu if agg_on_gpu is None else agg_on_gpu)


def distinct_values(mode, n):
    """n distinct values: FILTER kinds include the empty list and PASS"""
    if mode == "string":
        return [f"v{k}" for k in range(n)]
    return (["PASS", ""] + [f"f{k}" for k in range(2, n)])[:n]


MODES = ["filter", "string", "bcf"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, CAP - 1, CAP, CAP + 1])
def test_distinct_count_up_to_and_beyond_capacity(ctx, tmp_path, mode, n):
    vals0 = distinct_values(mode, n)
    vals = [vals0[(i * 7919) % n] for i in range(2 * n + 50)]  # every value at least twice, in a scattered order
    check_both(ctx, tmp_path, mode, vals, on_gpu=n <= CAP)


@pytest.mark.gpu
def test_string_key_capacity_with_null_rows(ctx, tmp_path):
    """4096 values and rows without one: batches keep NULL as NULL (4096 ids: the device); a GROUP BY spends one more id on the
    empty text for the NULL group (4097: the host reader)"""
    vals0 = distinct_values("string", CAP)
    vals = [None if i % 10 == 4 else vals0[i % CAP] for i in range(3 * CAP)]
    assert len({v for v in vals if v is not None}) == CAP
    check_both(ctx, tmp_path, "string", vals, on_gpu=True, agg_on_gpu=False)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("where", ["first_slab", "later_slab"])
def test_overflow_in_the_first_or_a_later_slab(ctx, tmp_path, monkeypatch, mode, where):
    """1 MiB slabs: the 4097th value in the first slab, or in a later one (about 100 values in slab 1, the rest arriving slab by
    slab): the scan hands over to the host reader; batches come out whole and in file order"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    vals0 = distinct_values(mode, CAP + 1)
    if where == "first_slab":
        order = list(range(CAP + 1)) + [i % 100 for i in range(60000)]
    else:
        order = [i % 100 for i in range(30000)]
        for k in range(100, CAP + 1):
            order += [k] + [(k + j) % 100 for j in range(10)]
    vals = [vals0[k] for k in order]
    check_both(ctx, tmp_path, mode, vals, on_gpu=False)


def pool_values(total_extra):
    """2048 distinct 512-byte values that differ in their LAST four bytes (exactly the 1 MiB pool), adjusted by total_extra bytes:
    -1 = the last value one byte shorter (just under), +1 = one more value of one byte (just over)"""
    vals = ["x" * 508 + f"{k:04d}" for k in range(2048)]
    if total_extra < 0:
        vals[-1] = vals[-1][1:]
    elif total_extra > 0:
        vals.append("z")
    assert sum(len(v) for v in vals) == POOL + total_extra
    return vals


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["filter", "string"])
@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_text_pool_just_under_exactly_and_just_over_one_mib(ctx, tmp_path, mode, extra):
    vals0 = pool_values(extra)
    vals = vals0 + vals0[::-1]
    check_both(ctx, tmp_path, mode, vals, on_gpu=extra <= 0)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_parser_filters_with_a_full_text_pool(ctx, extra):
    """exon_hip_vcf_parser_filters through VCFParser.filters(): 2048 names of 512 bytes fill the pool and must fit the name buffer
    (the pool plus one NUL per name); one byte more overflows the table: the slab is undecided and the names are refused"""
    vals = pool_values(extra)
    text = "".join(f"1\t{i + 1}\t.\tA\tC\t1\t{v}\tAF=0.5\n" for i, v in enumerate(vals + vals)).encode()
    p = exon_amd.VCFParser(ctx, ["1"], info_field="AF", max_slab_bytes=len(text) + 4096)
    try:
        res = p.parse_host(text)
        assert res["n_rows"] == 2 * len(vals)
        if extra <= 0:
            assert res["n_undecided"] == 0
            f = p.filters()
            assert len(f) == len(vals) and set(f) == set(vals)
            assert [f[i] for i in res["filter_id"]] == vals + vals
        else:
            assert res["n_undecided"] > 0
            with pytest.raises(exon_amd.ExonHipError):
                p.filters()
    finally:
        p.close()


NEAR = {"filter": ["", "PASS", "PAS", "PASSX", "PASS;q10", "q10;PASS", "q10", "q1", "q11", "q10;s50", "q10;s5", "q10;s51"],
        "string": ["abc", "abd", "ab", "abcd", "abcc", "bbc", "a", "aa", "A", "abc.", "abc_"]}
NEAR["bcf"] = NEAR["filter"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", ["all_rows_one_value", "every_other_row", "near_misses"])
def test_many_rows_inserting_and_values_one_byte_apart(ctx, tmp_path, mode, shape):
    """one launch where every row (or every other row) inserts the same new value; values that differ only in their last byte
    or only in length; the empty list ('.') is its own key, not PASS"""
    same = "q10;s50" if mode != "string" else "NEWVAL"
    n = 20000
    if shape == "all_rows_one_value":
        vals = [same] * n
    elif shape == "every_other_row":
        other = distinct_values(mode, 3000)
        vals = [same if i % 2 == 0 else other[(i // 2) % 3000] for i in range(n)]
    else:
        vals = [NEAR[mode][(i * 5) % len(NEAR[mode])] for i in range(n)]
    check_both(ctx, tmp_path, mode, vals, on_gpu=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["filter", "string"])
def test_two_values_with_the_same_hash_stay_two_groups(ctx, tmp_path, mode):
    """COLLIDING[0] and COLLIDING[1] hash alike: each must keep its own rows and name (here: the host reader's, after the device
    found that the texts differ), and a third value its own"""
    third = "PASS" if mode == "filter" else "third"
    vals = [(COLLIDING[0], COLLIDING[1], third)[i % 3] if i % 5 else COLLIDING[0] for i in range(3000)]
    assert vals.count(COLLIDING[0]) != vals.count(COLLIDING[1])  # two groups of different sizes, each keyed by its own name
    check_both(ctx, tmp_path, mode, vals, on_gpu=False)
