"""GPU: several partitions of ONE context at the same time -- what no other test does: every other GPU test drives one stream or one
scan to completion on one host thread.  What is looked for is one partition corrupting another: a partial record, a ticket or a
status word read by the wrong stream, a recycled buffer that is still in use, a pinned export block freed under a live batch.

Every case asserts exact equality (==) with an expectation computed without the library -- tests/stream_batches_expect.py,
seq_stats_expect.py, read_stats_expect.py, scan_predicate_expect.py, flag_predicate_expect.py and the Python rows the files were
written from -- AND with the same work done one partition after another.  f64 sums are kept order-free: pushed y values are
multiples of 1/8, QUAL in the files a multiple of 1/8 (halves), so the LDS and tier-3 paths compare with == too.

  1  interleaved on one host thread: 28 streams of 14 plans fed round-robin, workspace growth under load, status words, close / reopen
  2  one host thread per partition, host Arrow batches (held and copied by the shared staging threads)
  3  one host thread per partition, files through Stream.consume (slab buffers, inflate scratch, re-keying)
  4  one host thread per scan, batch export (pinned export blocks that outlive their scans)
  5  the error text of two threads failing at once

Guards: workers catch their exceptions and the main thread re-raises the first; joins carry a limit of max(60 s, 20 x the sequential
pass timed in the same test); a worker still alive at the limit is a hang: the session ends there (pytest.exit), nothing else starts
on the GPU.  No sleeps, no loops "until it fails"."""
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import exon_amd
import fasta_expect
import flag_predicate_expect as FE
import gff_expect
import read_stats_expect as RE
import scan_predicate_expect as VE
import seq_stats_expect as QE
import stream_batches_expect as S
from test_flag_predicate import mixed as bam_mixed, write as write_bam_sam
from test_gpu_stream_batch_limits import U8
from test_key_reconcile import write_vcf as write_keyed_vcf
from test_scan_predicate import k4_numpy, mixed as vcf_mixed, write as write_vcf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tools", "bin", "gen_text")
EINVAL, EUNSUPPORTED = -1, -4


# ---- guards ---------------------------------------------------------------------------------------------------------------------------
def run_threads(what, workers, seq_seconds):
    """workers: {name: zero-argument callable}, each on its own thread, released together by a barrier.  -> seconds"""
    limit = max(60.0, 20.0 * seq_seconds)
    barrier = threading.Barrier(len(workers))
    errors = []

    def body(name, fn):
        try:
            barrier.wait(timeout=limit)
            fn()
        except BaseException as e:  # noqa: BLE001 (the main thread re-raises it)
            errors.append((name, e))

    threads = [threading.Thread(target=body, args=(n, f), name=n, daemon=True) for n, f in workers.items()]
    t0 = time.perf_counter()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, t0 + limit - time.perf_counter()))
    took = time.perf_counter() - t0
    hung = [t.name for t in threads if t.is_alive()]
    if hung:
        pytest.exit(f"{what}: worker(s) {hung} still running after {took:.0f} s (limit {limit:.0f} s = max(60, 20 x the sequential "
                    f"pass of {seq_seconds:.2f} s)): a hang; nothing else is started on the GPU", returncode=3)
    print(f"[concurrent partitions] {what}: sequential pass {seq_seconds:.2f} s, join limit {limit:.0f} s, threads {took:.2f} s")
    if errors:
        raise errors[0][1]
    return took


def same(got, want, what=None):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64, what
    assert np.array_equal(got[0], want[0]), (what, np.flatnonzero(got[0] != want[0])[:8])
    assert np.array_equal(got[1], want[1]), what


# ---- 1. pushed rows: the plans of the issue's list ----------------------------------------------------------------------------------
ROUND = [2049, 8193, 1, 40_000, 257]  # rows per push, round by round
STARTS = np.concatenate([[0], np.cumsum(ROUND)]).tolist()
N_ROWS = STARTS[-1]
X_VALUES = np.array([0.0, 0.01, 0.25, 0.5, 1.0, -1.0], np.float32)
FLAGS = np.array([0, 4, 16, 99, 147, 256, 1024, 1028, 1284, 2048], np.int32)


def _gen_k2(rng, n):
    return [rng.integers(0, 4, n).astype(np.int32), rng.integers(1, 1000, n).astype(np.int64)]


def _gen_k6(rng, n):
    start = rng.integers(1, 5000, n).astype(np.int64)
    return [rng.integers(0, 3, n).astype(np.int32), start, start + rng.integers(0, 300, n)]


def _gen_k3(R):
    return lambda rng, n: [rng.choice(FLAGS, n), rng.integers(0, 61, n).astype(np.uint8), rng.integers(0, R, n).astype(np.int32)]


def _gen_k4(G, lo=0):  # y from eighths: the f64 sums are exact in any order
    return lambda rng, n: [rng.choice(X_VALUES, n), (rng.integers(lo, 8000, n) / 8.0).astype(np.float32), rng.integers(0, G, n).astype(np.int32)]


class Entry:
    """one plan of the list: kind / params as tests/stream_batches_expect.py takes them ("k10": seq_stats_expect)"""

    def __init__(self, name, kind, params, plan, gen, nullable):
        self.name, self.kind, self.params, self.make_plan, self.gen, self.nullable = name, kind, params, plan, gen, nullable


ENTRIES = [
    Entry("k2", "k2", (2, 100, 600), lambda c: c.plan_region_count(2, 100, 600), _gen_k2, [True, True]),
    Entry("k6", "k6", (1, 1000, 3000), lambda c: c.plan_overlap_count(1, 1000, 3000, columns=(0, 1, 2)), _gen_k6, [True] * 3),
    Entry("k3 R=25", "k3", (1284, 0, 30, 25), lambda c: c.plan_flag_mapq_group_count(1284, 0, 30, 25), _gen_k3(25), [True] * 3),  # 26 words: fused fold
    Entry("k3 R=300", "k3", (1284, 0, 30, 300), lambda c: c.plan_flag_mapq_group_count(1284, 0, 30, 300), _gen_k3(300), [True] * 3),  # 301 > FUSE_MAX_V
    Entry("k8 G=5", "k8", ("<=", 0.25, 5, False, False), lambda c: c.plan_cmp_minmax_by_group("<=", 0.25, 5), _gen_k4(5, -8000), [True, True, False]),
    Entry("k8 G=64", "k8", ("<=", 0.25, 64, False, False), lambda c: c.plan_cmp_minmax_by_group("<=", 0.25, 64), _gen_k4(64, -8000), [True, True, False]),
    Entry("k5 lmax=100", "k5", (100,), lambda c: c.plan_qual_pos_hist(100), lambda rng, n: [U8.random(rng, n, 0, 100)], [False]),
    Entry("k9", "k9", (40,), lambda c: c.plan_read_stats_hist(40), lambda rng, n: [U8.random(rng, n, 0, 40, b"ACGTNacgt"), U8.random(rng, n, 0, 17)], [False, False]),
    Entry("k10", "k10", (151,), lambda c: c.plan_seq_stats_hist(151), lambda rng, n: [U8.random(rng, n, 0, 150, b"ACGTNacgtn")], [False]),
]
# K4: lane slots, the LDS table, 3G = 255 / 258 words either side of FUSE_MAX_V = 256, tier 3 (every stream its own tail scratch)
for _G in (5, 64, 85, 86, 5000):
    ENTRIES.append(Entry(f"k4 G={_G}", "k4", (">", 0.01, _G, False, False), (lambda G: lambda c: c.plan_cmp_avg_by_group(">", 0.01, G))(_G), _gen_k4(_G),
                         [True, True, False]))
BY_NAME = {e.name: e for e in ENTRIES}


class Rows:
    """N_ROWS rows of one stream: values and boolean validity per column"""

    def __init__(self, entry, seed, n=N_ROWS):
        rng = np.random.default_rng(seed)
        self.entry, self.n = entry, n
        self.values = entry.gen(rng, n)
        self.valid = [(rng.random(n) < 0.7) if nb else np.ones(n, bool) for nb in entry.nullable]
        self._text = {}

    def text(self, c):
        if c not in self._text:
            self._text[c] = self.values[c].rows(range(self.n))
        return self._text[c]

    def want(self, spans):
        """the state of the rows [a, b) of `spans` (a span may repeat: everything adds, extremes are idempotent)"""
        idx = np.concatenate([np.arange(a, b) for a, b in spans] + [np.zeros(0, np.int64)]).astype(np.int64)
        cols = []
        for c, (v, ok) in enumerate(zip(self.values, self.valid)):
            cols.append(([self.text(c)[i] for i in idx], ok[idx]) if isinstance(v, U8) else (v[idx], ok[idx]))
        if self.entry.kind == "k10":
            return QE.expect_fast(cols[0][0], self.entry.params[0]), S.NO_SUMS
        return S.expect(self.entry.kind, self.entry.params, cols)

    def upload(self, ctx, lo, n, values=None):
        """rows [lo, lo + n) as device columns [(values, validity | None, offsets | None)] of their own allocations"""
        cols = []
        for c, v in enumerate(self.values if values is None else values):
            bm = None
            if self.entry.nullable[c]:
                bm = ctx.to_device(np.concatenate([np.packbits(self.valid[c][lo:lo + n], bitorder="little"), np.zeros(64, np.uint8)]))
            if isinstance(v, U8):
                a, b = int(v.off[lo]), int(v.off[lo + n])
                off = ctx.to_device((v.off[lo:lo + n + 1] - a).astype(np.int32))
                cols.append((ctx.to_device(np.concatenate([v.data[a:b], np.full(64, 73, np.uint8)])), bm, off))
            else:
                cols.append((ctx.to_device(np.concatenate([v[lo:lo + n], np.zeros(64, v.dtype)])), bm, None))
        return cols


class Pushed:
    """per entry: its plan, two streams' rows (j = 0, 1), their five device batches and the state of all their rows"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.plan, self.rows, self.dev, self.all = {}, {}, {}, {}
        for k, e in enumerate(ENTRIES):
            self.plan[e.name] = e.make_plan(ctx)
            for j in (0, 1):
                r = Rows(e, [7, k, j])
                self.rows[e.name, j] = r
                self.dev[e.name, j] = [r.upload(ctx, STARTS[b], ROUND[b]) for b in range(len(ROUND))]
                self.all[e.name, j] = r.want([(0, N_ROWS)])
        ctx.sync()

    def push(self, st, name, j, b):
        st.push_device(self.dev[name, j][b], ROUND[b])

    def close(self):
        for p in self.plan.values():
            p.close()


@pytest.fixture(scope="module")
def pushed(ctx):
    p = Pushed(ctx)
    yield p
    p.close()


def test_28_streams_of_14_plans_fed_round_robin(ctx, pushed):
    """every plan of the list open at once, two streams each (so two streams share every plan), one push per stream and round, no
    stream sync between the rounds; then the same pushes stream by stream"""
    keys = [(e.name, j) for e in ENTRIES for j in (0, 1)]
    streams = {k: pushed.plan[k[0]].open(k[1]) for k in keys}
    assert len({st.state()[2] for st in streams.values()}) == len(keys)  # 28 different hipStream_t
    for b in range(len(ROUND)):
        for k in keys:
            pushed.push(streams[k], k[0], k[1], b)
    got = {k: streams[k].finish() for k in keys}
    for st in streams.values():
        st.close()
    for k in keys:
        same(got[k], pushed.all[k], k)
    for k in keys:  # one partition after another
        st = pushed.plan[k[0]].open(k[1])
        for b in range(len(ROUND)):
            pushed.push(st, k[0], k[1], b)
        alone = st.finish()
        st.close()
        same(alone, pushed.all[k], k)
        same(got[k], alone, k)


def test_workspace_growth_under_load(ctx, pushed):
    """bare K3 on a stream's own hipStream_t with R = 25 and then R = 4095: the partials of that stream's workspace are freed and
    allocated again (behind a sync of THAT stream) while two other streams have launches queued"""
    n = 40_000
    rng = np.random.default_rng(5)
    flag, mapq = rng.choice(FLAGS, n), rng.integers(0, 61, n).astype(np.uint8)
    ref = {R: rng.integers(0, R, n).astype(np.int32) for R in (25, 4095)}
    mok, rok = rng.random(n) < 0.7, rng.random(n) < 0.7
    pad = np.zeros(64, np.uint8)
    d_flag, d_mapq = ctx.to_device(np.concatenate([flag, np.zeros(64, np.int32)])), ctx.to_device(np.concatenate([mapq, pad]))
    d_ref = {R: ctx.to_device(np.concatenate([ref[R], np.zeros(64, np.int32)])) for R in ref}
    d_mok = ctx.to_device(np.concatenate([np.packbits(mok, bitorder="little"), pad]))
    d_rok = ctx.to_device(np.concatenate([np.packbits(rok, bitorder="little"), pad]))
    d_out = {R: ctx.zeros(np.int64, R + 1) for R in ref}
    ctx.sync()
    names = ["k3 R=25", "k4 G=5000", "k5 lmax=100"]
    st = {nm: pushed.plan[nm].open() for nm in names}
    hs = st["k3 R=25"].state()[2]

    def bare(R):
        ctx.flag_mapq_group_count(d_flag, d_mapq, d_mok, d_ref[R], d_rok, n, 1284, 0, 30, R, d_out[R], stream=hs)

    for b in (0, 3):
        for nm in names:
            pushed.push(st[nm], nm, 0, b)
    bare(25)
    for nm in names[1:]:
        pushed.push(st[nm], nm, 0, 1)
    bare(4095)  # 2048 workgroups x 4096 words: far beyond the 65536 words the workspace starts with
    for nm in names:
        pushed.push(st[nm], nm, 0, 4)
    bare(25)  # ... and into the new partials
    spans = {nm: [(STARTS[b], STARTS[b + 1]) for b in ((0, 3, 4) if nm == "k3 R=25" else (0, 3, 1, 4))] for nm in names}
    for nm in names:
        same(st[nm].finish(), pushed.rows[nm, 0].want(spans[nm]), nm)
    ctx.sync(hs)
    for R in ref:
        want = S.k3([(flag, np.ones(n, bool)), (mapq, mok), (ref[R], rok)], 1284, 0, 30, R)[0]
        assert np.array_equal(d_out[R].to_host(), want * (2 if R == 25 else 1)), R
    for s in st.values():
        s.close()


def _poisoned(ctx, pushed, name, j, b):
    """device batch b of stream j with ONE row the kernel must report: a group id equal to G on a passing row with a valid y (K4),
    a read one byte longer than lmax (K5)"""
    r = pushed.rows[name, j]
    lo, n = STARTS[b], ROUND[b]
    if r.entry.kind == "k4":
        G = r.entry.params[2]
        keep = (r.values[0][lo:lo + n].astype(np.float64) > 0.01) & r.valid[0][lo:lo + n] & r.valid[1][lo:lo + n]
        gid = r.values[2].copy()
        gid[lo + int(np.flatnonzero(keep)[len(np.flatnonzero(keep)) // 2])] = G
        return r.upload(ctx, lo, n, [r.values[0], r.values[1], gid])
    lens = np.diff(r.values[0].off[lo:lo + n + 1]).astype(np.int64)
    lens[n // 2] = r.entry.params[0] + 1
    return Rows(r.entry, 1, n).upload(ctx, 0, n, [U8(lens, np.full(int(lens.sum()), 70, np.uint8))])


@pytest.mark.parametrize("name,message", [("k4 G=5", "group id out of range"), ("k5 lmax=100", "read longer than lmax")])
def test_status_words_stay_with_their_stream(ctx, pushed, name, message):
    """two streams of one plan, interleaved; one gets a batch with a row the device reports.  Its finish() says so -- as
    tests/test_gpu_k4_lane_slots.py expects of a single stream --, the other one finishes clean with exact numbers, and so does a
    stream opened after the first was closed (which may get its handle value, and must get a fresh status word)"""
    bad_batch = _poisoned(ctx, pushed, name, 0, 1)
    ctx.sync()
    bad, good = pushed.plan[name].open(0), pushed.plan[name].open(1)
    for b in range(len(ROUND)):
        if b == 1:
            bad.push_device(bad_batch, ROUND[b])
        else:
            pushed.push(bad, name, 0, b)
        pushed.push(good, name, 1, b)
    with pytest.raises(exon_amd.ExonHipError, match=message) as e:
        bad.finish()
    assert e.value.code == EINVAL
    same(good.finish(), pushed.all[name, 1], name)
    bad.close()
    again = pushed.plan[name].open(0)
    for b in range(len(ROUND)):
        pushed.push(again, name, 0, b)
    same(again.finish(), pushed.all[name, 0], name)
    again.close()
    good.close()


def test_20_rounds_of_open_push_finish_close_beside_a_long_lived_stream(ctx, pushed):
    """a new stream may get the hipStream_t of a closed one: it must start from a fresh workspace (partials, status word, fold ticket,
    tail scratch), whatever plan the closed one ran"""
    cycle = ["k4 G=5", "k3 R=300", "k4 G=5000", "k5 lmax=100", "k4 G=86", "k9", "k3 R=25", "k8 G=64", "k10", "k4 G=85"]
    short_spans = [(STARTS[0], STARTS[1]), (STARTS[4], STARTS[5])]
    want_short = {nm: pushed.rows[nm, 1].want(short_spans) for nm in cycle}
    long_name = "k4 G=64"
    long = pushed.plan[long_name].open()
    long_spans, handles = [], set()
    for r in range(20):
        nm = cycle[r % len(cycle)]
        st = pushed.plan[nm].open()
        handles.add(st.state()[2])
        pushed.push(st, nm, 1, 0)
        pushed.push(long, long_name, 0, r % len(ROUND))
        long_spans.append((STARTS[r % len(ROUND)], STARTS[r % len(ROUND) + 1]))
        pushed.push(st, nm, 1, 4)
        same(st.finish(), want_short[nm], (r, nm))
        st.close()
    same(long.finish(), pushed.rows[long_name, 0].want(long_spans), long_name)
    long.close()
    print(f"[concurrent partitions] close / reopen: 20 short streams used {len(handles)} different hipStream_t values")


# ---- 2. one host thread per partition, rows from memory -----------------------------------------------------------------------------
P_PUSH = 8
HOST_BATCHES = [8192] * 12 + [200_000]  # the last one is above the 131 072-row hold limit


def _host_partition(entry, w):
    """partition w: its rows, and its 13 pyarrow batches -- slices of one parent whose first row is w (mod 8): the validity bitmaps of
    every partition but the first start in the middle of a byte"""
    import pyarrow as pa
    n = sum(HOST_BATCHES)
    rows = Rows(entry, [11, w, len(entry.name)], n + 8)
    arrays = [pa.array(v, mask=~ok) if nb else pa.array(v) for v, ok, nb in zip(rows.values, rows.valid, entry.nullable)]
    batches, lo = [], w % 8
    first = lo
    for m in HOST_BATCHES:
        batches.append(pa.RecordBatch.from_arrays([a.slice(lo, m) for a in arrays], [f"c{c}" for c in range(len(arrays))]))
        lo += m
    if w % 8:
        assert batches[0].column(0).offset % 8 and batches[0].column(0).null_count  # (mid-byte, and a bitmap is there)
    return rows, batches, (first, lo)


def _packed(state):
    return np.concatenate([state[0], state[1].view(np.int64)])


@pytest.mark.parametrize("name", ["k4 G=8", "k3 R=25"])
def test_8_threads_push_host_batches_into_streams_of_one_plan(ctx, name):
    entry = BY_NAME.get(name) or Entry(name, "k4", (">", 0.01, 8, False, False), lambda c: c.plan_cmp_avg_by_group(">", 0.01, 8), _gen_k4(8), [True, True, False])
    plan = entry.make_plan(ctx)
    parts = [_host_partition(entry, w) for w in range(P_PUSH)]
    want = [rows.want([span]) for rows, _, span in parts]

    def partition(w, reps, out):
        for _ in range(reps):
            st = plan.open(w)
            for b in parts[w][1]:
                st.push(b)
            out.append(st.finish())
            st.close()

    alone = [[] for _ in range(P_PUSH)]
    t0 = time.perf_counter()
    for w in range(P_PUSH):
        partition(w, 1, alone[w])
    seq = time.perf_counter() - t0
    got = [[] for _ in range(P_PUSH)]
    run_threads(f"push {name}", {f"partition {w}": (lambda w=w: partition(w, 3, got[w])) for w in range(P_PUSH)}, seq)
    for w in range(P_PUSH):
        same(alone[w][0], want[w], w)
        assert len(got[w]) == 3
        for state in got[w]:
            same(state, want[w], w)
    # the P states folded on the device = one stream over all rows = the numpy statement's fold
    d_all = ctx.to_device(np.concatenate([_packed(got[w][2]) for w in range(P_PUSH)]))
    d_out = ctx.zeros(np.int64, plan.n_i64 + plan.n_f64)
    ctx.sync()
    plan.fold_states(d_all, P_PUSH, d_out)
    ctx.sync()
    folded = d_out.to_host()
    one = plan.open()
    for _, batches, _ in parts:
        for b in batches:
            one.push(b)
    whole = one.finish()
    one.close()
    plan.close()
    assert np.array_equal(folded, _packed(whole))
    same(whole, S.fold(entry.kind, entry.params, want), name)


# ---- 3. one host thread per partition, files through consume -------------------------------------------------------------------------
BGZF_SLAB_TEXT = 96 * 65536  # what a BGZF slab of EXON_HIP_GPU_PARSE_SLAB_MB=1 holds at the most: 96 members


def _k4_by_value(names, counts, sums, G):
    return {names[g]: (int(counts[g]), int(counts[G + g]), float(sums[g])) for g in range(len(names)) if counts[G + g]}


class Files:
    """the files of sections 3 and 4, written once, with what their rows say"""

    def __init__(self, tmp):
        self.tmp = tmp
        rng = np.random.default_rng(99)
        # VCF: QUAL in halves; ~75 bytes a line
        self.vcf_lines, self.vcf_wants = vcf_mixed(120_000, seed=21)
        self.vcf_bgzf = write_vcf(tmp, "big", self.vcf_lines, "bgzf")
        assert os.path.getsize(str(tmp / "big.vcf")) > BGZF_SLAB_TEXT  # two BGZF slabs
        self.want_vcf = k4_numpy(self.vcf_lines, range(len(self.vcf_lines)))
        self.gz_lines = self.vcf_lines[:50_000]
        self.vcf_gz = write_vcf(tmp, "part", self.gz_lines, "gz")
        assert os.path.getsize(str(tmp / "part.vcf")) > (5 << 19)  # three plain-gzip slabs of 1 MiB of text
        self.want_gz = k4_numpy(self.gz_lines, range(len(self.gz_lines)))
        # BAM and SAM from the same records: ~270 bytes a BAM record, ~380 a SAM line
        self.recs = bam_mixed(30_000, seed=8, l_seq=150)
        self.bam = write_bam_sam(tmp, "reads", self.recs, "bam")
        assert os.path.getsize(self.bam + ".u") > BGZF_SLAB_TEXT
        self.sam = write_bam_sam(tmp, "reads", self.recs, "sam")
        keep = [r for r in self.recs if FE.passes(r["flag"], r["mapq"], 1284, 0, 30)]
        self.k3 = np.bincount([2 if r["ref"] is None else r["ref"] for r in keep], minlength=3).tolist()
        self.k6_region = ("r1", 20_000, 60_000)
        self.k6 = sum(FE.hits(r, self.k6_region) for r in self.recs)
        assert min(self.k3) > 0 and 0 < self.k6 < len(self.recs)
        # FASTQ: ~190 bytes a read
        n = 20_000
        lens = rng.integers(1, 180, n)
        o = np.concatenate([[0], np.cumsum(lens)])
        sb = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, int(o[-1]))].tobytes()
        qb = rng.integers(33, 74, int(o[-1]), dtype=np.uint8).tobytes()
        self.fq_seqs, self.fq_quals = [sb[o[i]:o[i + 1]] for i in range(n)], [qb[o[i]:o[i + 1]] for i in range(n)]
        self.fq_heads = [b"r%d" % i + (b"", b" lane:%d x y" % (i % 7))[i % 2] for i in range(n)]
        self.fastq = str(tmp / "reads.fastq")
        with open(self.fastq, "wb") as f:
            f.write(b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in zip(self.fq_heads, self.fq_seqs, self.fq_quals)))
        assert os.path.getsize(self.fastq) > (5 << 19)
        self.k9 = RE.expect_fast(self.fq_seqs, self.fq_quals, 256).tolist()
        # FASTA: ragged records, wrapped at 60 columns or not
        lens = rng.integers(0, 300, n)
        o = np.concatenate([[0], np.cumsum(lens)])
        sb = np.frombuffer(b"ACGTNacgtRYKM", np.uint8)[rng.integers(0, 13, int(o[-1]))].tobytes()
        self.fa_seqs, out = [sb[o[i]:o[i + 1]] for i in range(n)], []
        for i, s in enumerate(self.fa_seqs):
            out.append(b">s%d some text\n" % i if i % 3 else b">s%d\n" % i)
            width = 60 if i % 2 else 1 << 20
            out.extend(s[k:k + width] + b"\n" for k in range(0, len(s), width))
        self.fasta_text = b"".join(out)
        self.fasta = str(tmp / "seqs.fasta")
        with open(self.fasta, "wb") as f:
            f.write(self.fasta_text)
        assert len(self.fasta_text) > (5 << 19)
        self.k10 = QE.expect_fast(self.fa_seqs, 256).tolist()
        # GFF: the generator's file, read back in Python
        self.gff = str(tmp / "genes.gff")
        subprocess.check_call([GEN, "gff", "60000", self.gff])
        names, ids, start, end = gff_expect.interval_columns(open(self.gff, "rb").read())
        assert os.path.getsize(self.gff) > (5 << 19)
        self.gff_rows = len(ids)
        a, b = int(np.percentile(start, 25)), int(np.percentile(start, 75))
        self.k2_region = (names[0], a, b)
        self.k2 = int(((ids == 0) & (start >= a) & (start <= b)).sum())
        assert 0 < self.k2 < len(ids)
        # three files per re-keying worker whose FILTER values appear in different orders
        orders = [[["PASS", ".", "q10"], ["s50", "q10;s50", "q10", ".", "PASS"], ["q10;s50", "PASS"]],
                  [["q10;s50", "s50"], ["PASS"], [".", "q10", "PASS", "s50"]]]
        self.keyed = []
        for w, firsts in enumerate(orders):
            paths, lines = [], []
            for k, first in enumerate(firsts):
                paths.append(str(tmp / f"keyed{w}{k}.vcf"))
                lines += [ln.rstrip("\n") for ln in write_keyed_vcf(paths[-1], 5000 + 1000 * k, 40 + 3 * w + k, first)]
            self.keyed.append((paths, k4_numpy(lines, range(len(lines))), len(lines)))

    # every job: (rows, result) of one partition, computed by the calling thread; asserts that the DEVICE decoded the file
    def vcf_k4(self, ctx, path):
        scan = exon_amd.Scan(path, "vcf", info_field="AF,DP", gpu_parse=True)
        plan = ctx.plan_cmp_avg_by_group(">", 0.01, 8, columns=(4, 2, 3))
        st = plan.open()
        try:
            rows = st.consume(scan)
            counts, sums = st.finish()
            assert scan.decoded_on_gpu()[0], path
            return rows, _k4_by_value(scan.dictionary(3), counts, sums, 8)
        finally:
            st.close(); plan.close(); scan.close()

    def plain(self, ctx, path, fmt, make_plan, contig=None):
        scan = exon_amd.Scan(path, fmt, gpu_parse=True)
        plan = make_plan(scan)
        st = plan.open()
        try:
            if contig:
                st.set_region_contig(contig)
            rows = st.consume(scan)
            counts, _ = st.finish()
            assert scan.decoded_on_gpu()[0], path
            return rows, counts.tolist()
        finally:
            st.close(); plan.close(); scan.close()

    def rekey(self, ctx, w):
        paths, _, _ = self.keyed[w]
        plan = ctx.plan_cmp_avg_by_group(">", 0.01, 64, columns=(4, 2, 3))
        st = plan.open()
        try:
            rows = 0
            for p in paths:
                scan = exon_amd.Scan(p, "vcf", info_field="AF", gpu_parse=True)
                rows += st.consume(scan)
                assert scan.decoded_on_gpu()[0], p
                scan.close()
            keys, _ = st.keys()
            counts, sums = st.finish()
            return rows, _k4_by_value(keys, counts, sums, 64)
        finally:
            st.close(); plan.close()

    def jobs(self, ctx):
        """name -> (callable, what it must return)"""
        return {
            "bgzf vcf -> k4": (lambda: self.vcf_k4(ctx, self.vcf_bgzf), (len(self.vcf_lines), self.want_vcf)),
            "gzip vcf -> k4": (lambda: self.vcf_k4(ctx, self.vcf_gz), (len(self.gz_lines), self.want_gz)),
            "bam -> k3": (lambda: self.plain(ctx, self.bam, "bam", lambda s: ctx.plan_flag_mapq_group_count(1284, 0, 30, 2)), (len(self.recs), self.k3)),
            "fastq -> k9": (lambda: self.plain(ctx, self.fastq, "fastq", lambda s: ctx.plan_read_stats_hist(256, columns=(2, 3))), (len(self.fq_seqs), self.k9)),
            "fasta -> k10": (lambda: self.plain(ctx, self.fasta, "fasta", lambda s: ctx.plan_seq_stats_hist(256, columns=(2,))), (len(self.fa_seqs), self.k10)),
            "sam -> k6": (lambda: self.plain(ctx, self.sam, "sam", lambda s: ctx.plan_overlap_count(s.dictionary(2).index("r1"), *self.k6_region[1:])), (len(self.recs), [self.k6])),
            "gff -> k2": (lambda: self.plain(ctx, self.gff, "gff", lambda s: ctx.plan_region_count(0, *self.k2_region[1:], columns=(0, 3)), contig=self.k2_region[0]), (self.gff_rows, [self.k2])),
            "rekey 0": (lambda: self.rekey(ctx, 0), (self.keyed[0][2], self.keyed[0][1])),
            "rekey 1": (lambda: self.rekey(ctx, 1), (self.keyed[1][2], self.keyed[1][1])),
        }


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return Files(tmp_path_factory.mktemp("partitions"))


@pytest.fixture
def small_slabs(monkeypatch):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    monkeypatch.setenv("EXON_HIP_GZ_SLAB_MB", "1")


def _consume_at_once(what, jobs, workers):
    """workers: {worker name: job name}.  Every job alone first (timed: the expectation's second half), then all workers at once, each
    doing its job three times"""
    alone = {}
    t0 = time.perf_counter()
    for job in dict.fromkeys(workers.values()):
        alone[job] = jobs[job][0]()
    seq = time.perf_counter() - t0
    got = {w: [] for w in workers}

    def body(w):
        for _ in range(3):
            got[w].append(jobs[workers[w]][0]())

    run_threads(what, {w: (lambda w=w: body(w)) for w in workers}, seq)
    for w, job in workers.items():
        want = jobs[job][1]
        assert alone[job] == want, job
        assert len(got[w]) == 3
        for res in got[w]:
            assert res == want, (w, job)
            assert res == alone[job], (w, job)


def test_mixed_formats_consumed_at_once(ctx, files, small_slabs):
    """BGZF VCF, plain-gzip VCF, BAM and FASTQ partitions at once, beside two streams that each re-key three files"""
    jobs = files.jobs(ctx)
    _consume_at_once("consume: 4 formats + 2 re-keying streams", jobs, {j: j for j in ("bgzf vcf -> k4", "gzip vcf -> k4", "bam -> k3", "fastq -> k9", "rekey 0", "rekey 1")})


def test_fasta_sam_and_gff_beside_two_of_the_others(ctx, files, small_slabs):
    jobs = files.jobs(ctx)
    _consume_at_once("consume: fasta, sam, gff + 2", jobs, {j: j for j in ("fasta -> k10", "sam -> k6", "gff -> k2", "bgzf vcf -> k4", "fastq -> k9")})


def test_9_bgzf_scans_at_once_one_more_than_the_inflate_pools(ctx, files, small_slabs):
    """a device gets at most 8 scratch pools for the parallel inflate: the ninth scan takes the serial inflate path"""
    jobs = files.jobs(ctx)
    _consume_at_once("consume: 9 BGZF VCF scans", jobs, {f"scan {k}": "bgzf vcf -> k4" for k in range(9)})


# ---- 4. one host thread per scan, batch export ------------------------------------------------------------------------------------------
def _columns(batches):
    cols = {}
    for b in batches:
        for i in range(b.type.num_fields):
            cols.setdefault(b.type.field(i).name, []).extend(b.field(i).to_pylist())
    return cols


def test_six_scans_export_batches_at_once_and_the_batches_outlive_them(ctx, files, small_slabs):
    tmp = files.tmp
    n_vcf = 30_000
    lines, wants = vcf_mixed(n_vcf, seed=31, pos0=False, chrom=lambda i: "1" if i < 20_000 else "2")
    vcf = write_vcf(tmp, "export", lines)
    vcf_bgzf = write_vcf(tmp, "export", lines, "bgzf")
    project = ("id", "ref", "alt", "info")
    kept = VE.keep(lines, "qual", ">=", 30.0)
    region = [i for i, ln in enumerate(lines) if ln.startswith("1\t") and 5000 <= int(ln.split("\t")[1]) <= 15_000]
    assert 0 < len(kept) < n_vcf and len(region) == 10_001
    recs = bam_mixed(6000, seed=14)
    bam = write_bam_sam(tmp, "export", recs, "bam")
    bam_kept = FE.keep(recs, 4, 0)
    assert 0 < len(bam_kept) < len(recs)
    nq, na = 10_000, 8000
    fq = {"name": [h.split(b" ", 1)[0].decode() for h in files.fq_heads[:nq]],
          "description": [h.split(b" ", 1)[1].decode() if b" " in h else None for h in files.fq_heads[:nq]],
          "sequence": [s.decode() for s in files.fq_seqs[:nq]], "quality_scores": [q.decode() for q in files.fq_quals[:nq]]}
    fastq = str(tmp / "export.fastq")
    with open(fastq, "wb") as f:
        f.write(b"".join(b"@" + h + b"\n" + s + b"\n+\n" + q + b"\n" for h, s, q in zip(files.fq_heads[:nq], files.fq_seqs[:nq], files.fq_quals[:nq])))
    fa_text = files.fasta_text[:files.fasta_text.index(b">s%d" % na)]
    fasta = str(tmp / "export.fasta")
    with open(fasta, "wb") as f:
        f.write(fa_text)

    def vcf_scan(path, bs, **kw):
        return exon_amd.Scan(path, "vcf", info_field=VE.INFO_FIELD, gpu_parse=True, project=project, batch_size=bs, **kw)

    # name -> (open, batch size, expected columns)
    cases = {
        "vcf where": (lambda: vcf_scan(vcf, 64, where=(2, ">=", 30.0)), 64, VE.columns(lines, wants, kept, project)),
        "vcf": (lambda: vcf_scan(vcf, 1000), 1000, VE.columns(lines, wants, range(n_vcf), project)),
        "vcf region": (lambda: vcf_scan(vcf_bgzf, 8192, region="1:5000-15000"), 8192, VE.columns(lines, wants, region, project)),
        "bam flags": (lambda: exon_amd.Scan(bam, "bam", gpu_parse=True, project=FE.PROJECT, where_flags=(4, 0), batch_size=64), 64, FE.columns(recs, False, bam_kept)),
        "fastq": (lambda: exon_amd.Scan(fastq, "fastq", gpu_parse=True, batch_size=1000), 1000, fq),
        "fasta": (lambda: exon_amd.Scan(fasta, "fasta", gpu_parse=True, batch_size=8192), 8192, fasta_expect.columns(fa_text)),
    }

    def equal(name, cols):
        want = cases[name][2]
        return VE.same(cols, want) if name.startswith("vcf") else cols == want

    def drain(name, scan, out):
        out.extend(scan)
        assert scan.decoded_on_gpu()[0], name
        assert all(0 < len(b) <= cases[name][1] for b in out) and scan.rows() == sum(len(b) for b in out), name

    t0 = time.perf_counter()
    for name in cases:  # one scan after another: the second half of the expectation
        scan, out = cases[name][0]().bind_ctx(ctx), []
        drain(name, scan, out)
        scan.close()
        assert equal(name, _columns(out)), name
        del out
    seq = time.perf_counter() - t0
    scans = {name: cases[name][0]().bind_ctx(ctx) for name in cases}
    batches = {name: [] for name in cases}
    run_threads("export: 6 scans", {name: (lambda name=name: drain(name, scans[name], batches[name])) for name in cases}, seq)
    for name in cases:
        assert equal(name, _columns(batches[name])), name
    for scan in scans.values():
        scan.close()
    for name in cases:  # the pinned blocks the batches view must still hold their bytes
        for b in batches[name]:
            b.validate(full=True)
        assert equal(name, _columns(batches[name])), (name, "after every scan was closed")
    batches.clear()


# ---- 5. two threads failing at once ------------------------------------------------------------------------------------------------------
def test_two_threads_failing_at_once_get_their_own_code_and_message(ctx):
    """a plan with lmax = 0 and a K8 plan above EXON_HIP_MAX_GROUPS: Context._check reads the calling thread's text first, so neither
    thread can be handed the other's"""
    seen = {"lmax": set(), "groups": set()}

    def fails(key, make, code, text, other):
        for _ in range(300):
            with pytest.raises(exon_amd.ExonHipError) as e:
                make()
            seen[key].add((e.value.code, str(e.value)))
            assert e.value.code == code and text in str(e.value) and other not in str(e.value)

    t0 = time.perf_counter()
    fails("lmax", lambda: ctx.plan_qual_pos_hist(0), EINVAL, "lmax 0 out of range", "n_groups")
    fails("groups", lambda: ctx.plan_cmp_minmax_by_group(">", 0.0, 4097), EUNSUPPORTED, "n_groups 4097 outside", "lmax")
    seq = time.perf_counter() - t0
    run_threads("errors", {"lmax": lambda: fails("lmax", lambda: ctx.plan_qual_pos_hist(0), EINVAL, "lmax 0 out of range", "n_groups"),
                           "groups": lambda: fails("groups", lambda: ctx.plan_cmp_minmax_by_group(">", 0.0, 4097), EUNSUPPORTED, "n_groups 4097 outside", "lmax")}, seq)
    assert len(seen["lmax"]) == 1 and len(seen["groups"]) == 1
