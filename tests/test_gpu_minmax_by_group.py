"""GPU: MIN / MAX by group (plan kind 8) -- the kernel's two tiers and launch shapes, the special values of the encoding,
accumulate / overwrite / chunks, the refusals, the stream (host batches, Arrow state, reset), the fold, re-keying by value
and the VCF file pipelines -- against tests/minmax_expect.py (plain numpy), bit-exact on every state word."""
import os
import subprocess

import numpy as np
import pytest

import exon_amd
from exon_amd import _lib, distributed

import minmax_expect as MX

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
EINVAL, EUNSUPPORTED = -1, -4
PAD = 64  # spare elements behind every device column


def pack(valid):
    return np.concatenate([np.packbits(np.asarray(valid, bool), bitorder="little"), np.zeros(PAD, np.uint8)])


class Table:
    """host columns x, y, gid (+ validity) and their device copies"""

    def __init__(self, ctx, x, xv, y, yv, gid):
        self.ctx, self.n = ctx, len(x)
        self.x, self.xv, self.y, self.yv, self.gid = x, np.asarray(xv, bool), y, np.asarray(yv, bool), np.asarray(gid, np.int32)
        pad = lambda a: np.concatenate([a, np.zeros(PAD, a.dtype)])  # noqa: E731
        self.d = [ctx.to_device(pad(x)), ctx.to_device(pack(self.xv)), ctx.to_device(pad(y)), ctx.to_device(pack(self.yv)),
                  ctx.to_device(pad(self.gid))]

    def cols(self, lo=0):
        """device columns from row `lo` on (a multiple of 8: validity bitmaps split on bytes; of 4: 16-byte values)"""
        assert lo % 8 == 0
        dx, dxv, dy, dyv, dg = self.d
        return [(dx.ptr + 4 * lo, dxv.ptr + lo // 8, None), (dy.ptr + 4 * lo, dyv.ptr + lo // 8, None), (dg.ptr + 4 * lo, None, None)]

    def expect(self, G, op, thr, lo=0, hi=None, **kw):
        s = slice(lo, self.n if hi is None else hi)
        return MX.expect(self.x[s], self.xv[s], self.y[s], self.yv[s], self.gid[s], G, op, thr, **kw)


def random_table(ctx, n, seed, max_gid=1 << 20):
    rng = np.random.default_rng(seed)
    x = (10 ** rng.uniform(-4, 0, n)).astype(np.float32)
    y = rng.normal(30, 400, n).astype(np.float32)
    return Table(ctx, x, rng.random(n) > 0.1, y, rng.random(n) > 0.1, rng.integers(0, max_gid, n))


@pytest.fixture(scope="module")
def base(ctx):
    """70 001 random rows with ~10 % NULLs in x and in y; group ids are drawn wide and reduced modulo G by each case"""
    return random_table(ctx, 70_001, 11)


def bare(ctx, t, n, G, op, thr, gid=None):
    """the bare operator over the first n rows of `t` into a zeroed state"""
    dg = t.d[4] if gid is None else ctx.to_device(np.concatenate([gid.astype(np.int32), np.zeros(PAD, np.int32)]))
    st = ctx.zeros(np.int64, 4 * G)
    ctx.cmp_minmax_by_group(t.d[0], t.d[1], t.d[2], t.d[3], dg, n, thr, op, G, st)
    ctx.sync()
    return st.to_host()


@pytest.mark.parametrize("op", [">", "<=", "!="])
@pytest.mark.parametrize("G", [1, 5, 8, 9, 64, 4096])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 70_001])
def test_bare_operator_bit_exact(ctx, base, n, G, op):
    thr = float(base.x[7]) if op == "!=" else 0.01
    gid = base.gid[:n] % G
    got = bare(ctx, base, n, G, op, thr, gid=gid)
    want = MX.expect(base.x[:n], base.xv[:n], base.y[:n], base.yv[:n], gid, G, op, thr)
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def big(ctx):
    """the smallest table that takes a big launch shape: every CU gets one 8192-row tile, plus a ragged tail"""
    n = ctx.info()["compute_units"] * 8192 + 4099
    return random_table(ctx, n, 12)


@pytest.mark.parametrize("G", [5, 300])
def test_big_launch_shape(ctx, big, G):
    gid = big.gid % G
    got = bare(ctx, big, big.n, G, ">", 0.01, gid=gid)
    assert np.array_equal(got, MX.expect(big.x, big.xv, big.y, big.yv, gid, G, ">", 0.01))


@pytest.fixture(scope="module")
def big4(ctx):
    """... and the smallest at which the register tier takes its 16384-row tile (every CU gets one of those): the shape
    large tables run.  The table tier stays at 8192-row tiles."""
    n = ctx.info()["compute_units"] * 16384 + 4099
    return random_table(ctx, n, 13)


@pytest.mark.parametrize("G", [5, 8])
def test_big_launch_shape_16384_row_tiles(ctx, big4, G):
    gid = big4.gid % G
    got = bare(ctx, big4, big4.n, G, ">", 0.01, gid=gid)
    assert np.array_equal(got, MX.expect(big4.x, big4.xv, big4.y, big4.yv, gid, G, ">", 0.01))


def plan_run(ctx, t, G, op, thr, x_type="f32", y_type="f32", overwrite=True, state=None, lo=0, hi=None):
    plan = ctx.plan_cmp_minmax_by_group(op, thr, G, x_type=x_type, y_type=y_type)
    assert (plan.n_i64, plan.n_f64) == (4 * G, 0)
    st = ctx.zeros(np.int64, 4 * G) if state is None else state
    plan.launch(t.cols(lo), (t.n if hi is None else hi) - lo, st, overwrite=overwrite)
    ctx.sync()
    plan.close()
    return st


@pytest.mark.parametrize("G", [7, 40])
def test_special_float_values_null_only_and_empty_groups(ctx, G):
    """y holds the ends of totalOrder (both NaN signs, all-ones payloads, infinities, signed zeros, denormals) among random
    values; group 1 passes rows but all its y are NULL, group 2 has no passing row"""
    rng = np.random.default_rng(5)
    n = 20_011
    y = rng.normal(0, 1e3, n).astype(np.float32)
    at = rng.random(n) < 0.02
    y[at] = rng.choice(MX.SPECIAL_F32_BITS, int(at.sum())).view(np.float32)
    gid = rng.integers(0, G, n)
    x = (10 ** rng.uniform(-4, 0, n)).astype(np.float32)
    xv, yv = rng.random(n) > 0.1, rng.random(n) > 0.1
    yv[gid == 1] = False
    xv[gid == 2] = False
    t = Table(ctx, x, xv, y, yv, gid)
    got = plan_run(ctx, t, G, ">", 0.01).to_host().reshape(4, G)
    want = t.expect(G, ">", 0.01).reshape(4, G)
    assert np.array_equal(got, want)
    assert got[1, 1] > 0 and got[0, 1] == 0 and got[2, 1] == 0 and got[3, 1] == 0
    assert not got[:, 2].any()
    # one group each for the two extremes of the order: the kernel's raw keys are 0xFFFFFFFF and 0 there
    y2 = np.array([0x7FFFFFFF, 0xFFFFFFFF] * 8, np.uint32).view(np.float32)
    t2 = Table(ctx, np.ones(16, np.float32), np.ones(16, bool), y2, np.ones(16, bool), np.arange(16) % 2)
    got = plan_run(ctx, t2, G, ">", 0.01).to_host().reshape(4, G)
    assert np.array_equal(got, t2.expect(G, ">", 0.01).reshape(4, G))
    assert got[2, 0] == 1 and got[3, 0] == 2**32 and got[2, 1] == 2**32 and got[3, 1] == 1


@pytest.mark.parametrize("G", [3, 33])
def test_int32_columns(ctx, G):
    """Int32 y at both extremes; Int32 x compared with 16777217 exactly (f32 cannot tell it from 16777216)"""
    rng = np.random.default_rng(6)
    n = 9_001
    x = rng.integers(16777215, 16777220, n).astype(np.int32)
    y = rng.integers(-2**31, 2**31, n).astype(np.int32)
    at = rng.random(n) < 0.05
    y[at] = rng.choice(MX.SPECIAL_I32, int(at.sum()))
    t = Table(ctx, x.view(np.float32), rng.random(n) > 0.1, y.view(np.float32), rng.random(n) > 0.1, rng.integers(0, G, n))
    got = plan_run(ctx, t, G, ">", 16777217, x_type="i32", y_type="i32").to_host()
    want = MX.expect(x, t.xv, y, t.yv, t.gid, G, ">", 16777217, x_is_int=True, y_is_int=True)
    assert np.array_equal(got, want)
    assert want[G:2 * G].sum() == int((t.xv & (x > 16777217)).sum()) > 0
    vals, valid = exon_amd.minmax_decode(got[2 * G:3 * G], True, "i32")
    assert valid.all() and vals.min() == -2**31


@pytest.mark.parametrize("G,key", [(64, "hot63"), (64, "sorted"), (4096, "sorted"), (5, "hot3")])
def test_hot_and_sorted_keys(ctx, base, G, key):
    n = base.n
    gid = {"hot63": np.full(n, 63), "hot3": np.full(n, 3), "sorted": np.arange(n) * G // n}[key]
    got = bare(ctx, base, n, G, ">", 0.01, gid=gid)
    assert np.array_equal(got, MX.expect(base.x, base.xv, base.y, base.yv, gid, G, ">", 0.01))


@pytest.mark.parametrize("G", [5, 100])
def test_accumulate_overwrite_and_chunks(ctx, G):
    t = random_table(ctx, 30_011, 21, max_gid=G)
    whole = t.expect(G, "<=", 0.02)
    half = 15_000 // 8 * 8
    st = plan_run(ctx, t, G, "<=", 0.02, hi=half)                                  # OVERWRITE of the first half ...
    assert np.array_equal(st.to_host(), t.expect(G, "<=", 0.02, hi=half))
    plan_run(ctx, t, G, "<=", 0.02, overwrite=False, state=st, lo=half)            # ... + ACCUMULATE of the second
    assert np.array_equal(st.to_host(), whole)
    dirty = ctx.to_device(np.full(4 * G, 2**40 + 12345, np.int64))                 # OVERWRITE ignores what was there
    assert np.array_equal(plan_run(ctx, t, G, "<=", 0.02, state=dirty).to_host(), whole)
    plan = ctx.plan_cmp_minmax_by_group("<=", 0.02, G)
    cuts = [0, 8, 10_000, t.n]                                                    # three ragged chunks (+ an empty one)
    chunks = [(t.cols(a), b - a) for a, b in zip(cuts, cuts[1:])] + [(t.cols(0), 0)]
    plan.launch_chunks(chunks, dirty, overwrite=True)
    ctx.sync()
    assert np.array_equal(dirty.to_host(), whole)
    plan.launch_chunks([(t.cols(0), 0)], dirty, overwrite=True)                    # an overwrite of nothing: the empty state
    ctx.sync()
    assert not dirty.to_host().any()
    plan.close()


def test_refusals(ctx, base):
    with pytest.raises(exon_amd.ExonHipError) as e:
        ctx.plan_cmp_minmax_by_group(">", 0.01, 4097)
    assert e.value.code == EUNSUPPORTED
    st = ctx.zeros(np.int64, 4 * 4097)
    with pytest.raises(exon_amd.ExonHipError) as e:
        ctx.cmp_minmax_by_group(base.d[0], base.d[1], base.d[2], base.d[3], base.d[4], 100, 0.01, ">", 4097, st)
    assert e.value.code == EUNSUPPORTED
    d = _lib.PlanDesc(kind=_lib.PLAN_CMP_MINMAX_BY_GROUP, n_groups=5, cmp_op=6, threshold=0.01)
    with pytest.raises(exon_amd.ExonHipError) as e:
        exon_amd.Plan(ctx, d, (0, 1, 2))
    assert e.value.code == EINVAL
    plan = ctx.plan_cmp_minmax_by_group(">", 0.01, 5)
    cols = base.cols()
    cols[2] = (cols[2][0], base.d[1].ptr, None)  # a validity bitmap on the group column
    with pytest.raises(exon_amd.ExonHipError) as e:
        plan.launch(cols, 100, st)
    assert e.value.code == EUNSUPPORTED and "nullable group" in str(e.value)
    for G in (5, 20):  # ids up to 2^20 in a plan for G groups: reported at the next sync, like K4
        ctx.cmp_minmax_by_group(base.d[0], base.d[1], base.d[2], base.d[3], base.d[4], base.n, 0.01, ">", G, st)
        with pytest.raises(exon_amd.ExonHipError, match="group id out of range"):
            ctx.sync()
    ctx.sync()  # the status word was taken
    plan.close()


@pytest.mark.parametrize("y_type", ["f32", "i32"])
def test_stream_batches_arrow_state_and_reset(ctx, y_type):
    import pyarrow as pa
    rng = np.random.default_rng(31)
    n, G = 8192 + 8192 + 777, 6
    x = (10 ** rng.uniform(-4, 0, n)).astype(np.float32)
    y = rng.integers(-1000, 1000, n).astype(np.int32) if y_type == "i32" else rng.normal(0, 50, n).astype(np.float32)
    xv, yv = rng.random(n) > 0.1, rng.random(n) > 0.1
    gid = rng.integers(0, 4, n).astype(np.int32)  # groups 4 and 5 never appear
    gid[gid == 3] = 5
    yv[gid == 2] = False                          # group 2: rows, but no value
    tbl = pa.record_batch({"x": pa.array(x, mask=~xv), "y": pa.array(y, mask=~yv), "g": pa.array(gid)})
    plan = ctx.plan_cmp_minmax_by_group(">", 0.01, G, y_type=y_type)
    st = plan.open()
    for lo in (0, 8192, 16384):
        st.push(tbl.slice(lo, 8192))
    want = MX.expect(x, xv, y, yv, gid, G, ">", 0.01, y_is_int=y_type == "i32")
    arr = st.finish_arrow()
    assert [f.name for f in arr.type] == ["group", "min[min]", "max[max]", "count[count]", "count(*)[count]"]
    vt = pa.int32() if y_type == "i32" else pa.float32()
    assert [f.type for f in arr.type] == [pa.int32(), vt, vt, pa.int64(), pa.int64()]
    rows = arr.to_pylist()
    assert [r["group"] for r in rows] == [0, 1, 2, 5]
    for r in rows:
        g = r["group"]
        assert r["count[count]"] == want[g] and r["count(*)[count]"] == want[G + g]
        if g == 2:
            assert r["min[min]"] is None and r["max[max]"] is None
        else:
            sel = y[(gid == g) & yv & MX.passes(x, xv, ">", 0.01)]
            assert r["min[min]"] == sel.min() and r["max[max]"] == sel.max()
    # a second query on the same stream gives its own answer (finish() returns the raw words)
    st.reset()
    st.push(tbl.slice(100, 5000))
    counts, sums = st.finish()
    s = slice(100, 5100)
    assert len(sums) == 0 and np.array_equal(counts, MX.expect(x[s], xv[s], y[s], yv[s], gid[s], G, ">", 0.01, y_is_int=y_type == "i32"))
    st.close()
    plan.close()


def test_plan_fold_states(ctx):
    G, world = 37, 3
    plan = ctx.plan_cmp_minmax_by_group(">", 0.01, G)
    states = []
    gathered = ctx.zeros(np.int64, world * 4 * G)
    for r in range(world):
        t = random_table(ctx, 5_000 + 77 * r, 40 + r, max_gid=G - 5 * r)
        plan.launch(t.cols(), t.n, gathered.ptr + r * 4 * G * 8, overwrite=True)
        ctx.sync()  # (the table's device buffers go away with `t`)
        states.append(t.expect(G, ">", 0.01))
    out = ctx.zeros(np.int64, 4 * G)
    plan.fold_states(gathered, world, out)
    ctx.sync()
    assert np.array_equal(gathered.to_host().reshape(world, -1), np.stack(states))
    assert np.array_equal(out.to_host(), MX.fold(states, G))
    plan.close()
    # a K4 plan: the same bits as exon_hip_fold_states
    k4 = ctx.plan_cmp_avg_by_group(">", 0.01, 5)
    words = k4.n_i64 + k4.n_f64
    g4 = ctx.zeros(np.int64, world * words)
    for r in range(world):
        af, av, q, qv, fid = ctx.gen_c4(4 + r, 0, 50_000)
        k4.launch([(af, av, None), (q, qv, None), (fid, None, None)], 50_000, g4.ptr + r * words * 8, overwrite=True)
        ctx.sync()
    a, b = ctx.zeros(np.int64, words), ctx.zeros(np.int64, words)
    k4.fold_states(g4, world, a)
    ctx._check(ctx.lib.exon_hip_fold_states(ctx.h, None, g4.ptr, world, k4.n_i64, k4.n_f64, b.ptr))
    ctx.sync()
    assert a.to_host().any() and np.array_equal(a.to_host(), b.to_host())
    k4.close()


def test_set_keys_moves_all_four_planes(ctx):
    import pyarrow as pa
    import torch
    rng = np.random.default_rng(50)
    n, G = 6_000, 9
    names = ["PASS", "", "q10", "s50"]
    x = (10 ** rng.uniform(-4, 0, n)).astype(np.float32)
    y = rng.normal(0, 50, n).astype(np.float32)
    xv, yv = rng.random(n) > 0.1, rng.random(n) > 0.1
    gid = rng.integers(0, len(names), n).astype(np.int32)
    plan = ctx.plan_cmp_minmax_by_group(">", 0.01, G)
    st = plan.open()
    st.set_keys(names)  # a declaration: what the pushed ids mean
    st.push(pa.record_batch({"x": pa.array(x, mask=~xv), "y": pa.array(y, mask=~yv), "g": pa.array(gid)}))
    before, _ = st.snapshot()
    assert np.array_equal(before, MX.expect(x, xv, y, yv, gid, G, ">", 0.01))
    new = ["zz", "s50", "never", "q10", "PASS", "", "more"]
    st.set_keys(new)
    after, _ = st.finish()
    layout = distributed.state_layout_ex(_lib.PLAN_CMP_MINMAX_BY_GROUP, G)
    want = distributed.permute_state(torch.from_numpy(before), layout, [new.index(k) for k in names]).numpy()
    assert np.array_equal(after, want) and after.reshape(4, G)[1].sum() == before.reshape(4, G)[1].sum() > 0
    assert not after.reshape(4, G)[:, [0, 2, 6, 7, 8]].any()
    st.close()
    plan.close()


# ------------------------------------------------------------------------------------------------ files

VCF_HEAD = ('##fileformat=VCFv4.3\n##contig=<ID=1>\n##contig=<ID=2>\n'
            '##FILTER=<ID=q10,Description="x">\n##FILTER=<ID=s50,Description="x">\n'
            '##INFO=<ID=AF,Number=1,Type=Float,Description="x">\n##INFO=<ID=DP,Number=1,Type=Integer,Description="x">\n'
            '#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n')
FILTERS = ["PASS", ".", "q10", "q10;s50", "s50"]


def write_vcf(path, n, seed, first_filters, dp_type="Integer"):
    """n rows; the first rows carry `first_filters` in that order (they decide the file's dictionary ids).  AF straddles 0.01,
    QUAL is in eighths and DP an integer (both exact in text); some '.' QUALs, some rows without AF / DP / any INFO.
    Returns the rows as (filter, af, qual, dp) with None for a missing value."""
    rng = np.random.default_rng(seed)
    lines, rows = [], []
    for i in range(n):
        f = first_filters[i] if i < len(first_filters) else FILTERS[int(rng.integers(0, 5))]
        af = None if rng.random() < 0.05 else float("%.4g" % (10 ** rng.uniform(-4, 0)))
        q = None if rng.random() < 0.05 else int(rng.integers(0, 8000)) / 8
        dp = None if rng.random() < 0.05 else int(rng.integers(0, 100000))
        info = ";".join(([f"AF={af:.4g}"] if af is not None else []) + ([f"DP={dp}"] if dp is not None else [])) or "."
        lines.append(f"{1 + i % 2}\t{i + 1}\t.\tA\tC\t{'.' if q is None else q}\t{f}\t{info}\n")
        rows.append(("" if f == "." else f, af, q, dp))
    with open(path, "w") as fh:
        fh.write(VCF_HEAD.replace("ID=DP,Number=1,Type=Integer", "ID=DP,Number=1,Type=" + dp_type) + "".join(lines))
    return rows


def expect_by_value(rows, y_col):
    """{filter value: (count_y, count_rows, min, max)} over rows with AF > 0.01 (AF as the f32 the column holds)"""
    out = {}
    for r in rows:
        if r[1] is None or not float(np.float32(r[1])) > 0.01:
            continue
        c = out.setdefault(r[0], [0, 0, None, None])
        c[1] += 1
        y = r[y_col]
        if y is not None:
            c[0] += 1
            c[2] = y if c[2] is None else min(c[2], y)
            c[3] = y if c[3] is None else max(c[3], y)
    return {k: tuple(v) for k, v in out.items()}


def state_by_value(keys, counts, G, is_int):
    c = counts.reshape(4, G)
    lo, lov = MX.decode(c[2], True, is_int)
    hi, hiv = MX.decode(c[3], False, is_int)
    assert np.array_equal(lov, c[0] > 0) and np.array_equal(hiv, c[0] > 0)
    assert not c[:, len(keys):].any()
    return {k: (int(c[0, g]), int(c[1, g]), lo[g].item() if lov[g] else None, hi[g].item() if hiv[g] else None)
            for g, k in enumerate(keys) if c[1, g]}


@pytest.fixture(scope="module")
def vcf_pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("minmax_vcf")
    paths = [str(d / "a.vcf"), str(d / "b.vcf")]
    rows = write_vcf(paths[0], 3000, 1, ["PASS", ".", "q10"]) + write_vcf(paths[1], 3100, 2, ["s50", "q10;s50", "q10", ".", "PASS"])
    gz = []
    if os.path.exists(BGZIP):
        for p in paths:
            subprocess.check_call([BGZIP, p, p + ".gz"])
            gz.append(p + ".gz")
    return paths, gz, rows


@pytest.mark.parametrize("form", ["text", "bgzf"])
@pytest.mark.parametrize("gpu_parse", [True, False])
@pytest.mark.parametrize("y", ["qual", "DP"])
def test_vcf_files_by_key_value(ctx, vcf_pair, y, gpu_parse, form):
    paths, gz, rows = vcf_pair
    if form == "bgzf":
        assert gz, "tools/bin/bgzip is built by the test session"
        paths = gz
    G = 16
    plan = ctx.plan_cmp_minmax_by_group(">", 0.01, G, columns=(4, 2, 3) if y == "qual" else (4, 5, 3))
    st = plan.open()
    n = 0
    for p in paths:
        s = exon_amd.Scan(p, "vcf", info_field="AF,DP", gpu_parse=gpu_parse)
        n += st.consume(s)
        if gpu_parse:
            assert s.decoded_on_gpu()[0]
        s.close()
    assert n == len(rows)
    keys, _ = st.keys()
    counts, _ = st.finish()
    assert state_by_value(keys, counts, G, y == "DP") == expect_by_value(rows, 2 if y == "qual" else 3)
    assert sorted(keys) == sorted(["PASS", "", "q10", "q10;s50", "s50"])
    st.close()
    plan.close()


@pytest.mark.parametrize("gpu_parse", [True, False])
def test_one_stream_takes_one_type_of_the_argument(ctx, tmp_path, gpu_parse):
    """DP is Type=Integer in one file and Type=Float in the other: the state's words are keys of the TYPE, so the second file
    is refused and the stream keeps the first file's answer; MIN / MAX(qual) over the same two files is fine"""
    a, b = str(tmp_path / "a.vcf"), str(tmp_path / "b.vcf")
    rows_a = write_vcf(a, 500, 3, ["PASS", "q10"])
    rows_b = write_vcf(b, 500, 4, ["q10", "PASS"], dp_type="Float")
    G = 8
    plan = ctx.plan_cmp_minmax_by_group(">", 0.01, G, columns=(4, 5, 3))
    st = plan.open()
    s = exon_amd.Scan(a, "vcf", info_field="AF,DP", gpu_parse=gpu_parse)
    st.consume(s)
    s.close()
    s = exon_amd.Scan(b, "vcf", info_field="AF,DP", gpu_parse=gpu_parse)
    with pytest.raises(exon_amd.ExonHipError) as e:
        st.consume(s)
    assert e.value.code == -5 and "Int32" in str(e.value) and "Float32" in str(e.value)  # EXON_HIP_ESTATE
    s.close()
    keys, _ = st.keys()
    counts, _ = st.snapshot()
    assert state_by_value(keys, counts, G, True) == expect_by_value(rows_a, 3)
    st.reset()  # a new query takes the other type
    s = exon_amd.Scan(b, "vcf", info_field="AF,DP", gpu_parse=gpu_parse)
    st.consume(s)
    s.close()
    keys, _ = st.keys()
    arr = st.finish_arrow()
    import pyarrow as pa
    assert arr.type[1].type == pa.float32()
    got = {keys[r["group"]]: (r["count[count]"], r["count(*)[count]"], r["min[min]"], r["max[max]"]) for r in arr.to_pylist()}
    assert got == expect_by_value(rows_b, 3)
    st.close()
    plan.close()
    plan = ctx.plan_cmp_minmax_by_group(">", 0.01, G, columns=(4, 2, 3))
    st = plan.open()
    for p in (a, b):
        s = exon_amd.Scan(p, "vcf", info_field="AF,DP", gpu_parse=gpu_parse)
        st.consume(s)
        s.close()
    keys, _ = st.keys()
    counts, _ = st.finish()
    assert state_by_value(keys, counts, G, False) == expect_by_value(rows_a + rows_b, 2)
    st.close()
    plan.close()
