"""K5 (per-position quality histogram, exon_hip_qual_pos_hist*) at its limits, against tests/k5_expect.py.

K5 picks its algorithm on the device (k5_scan_offsets -> k5_pick_path -> path A / B / G inside k5_main), so what a test reaches
depends on the read lengths, the address of the first byte, lmax and the form of the call.  The groups below walk those:
  1. every length class at every alignment, both k5_main instantiations, both path-G layouts, the pt cap
  2. every byte value on every path (bytes >= 128 bypass LDS)
  3. long reads (the q2 loop, positions >= 310 by global atomics), lmax up to 65536, the argument checks
  4. the views form: contiguous uniform views (paths A / B behind the non-CONTIG offsets scan), gaps, order, overlap
  5. chunk lists across the 64-chunk launches of the ABI, direct and through a plan / a stream
  6. accumulation from launch to launch, across paths
  7. a read longer than lmax, seen by each detector alone; nothing written outside the histogram; the next launch is clean
  8. long reads through a FASTQ file
Every comparison is `==` against k5_expect.hist, every histogram sits between 64 guard words on each side, and every launch is
followed by ctx.sync() so that a status word surfaces in the case that raised it.  The library does not say which path ran: the
length classes of k5_expect only choose the shapes and label the failures.

NOT covered: the u32 range of a workgroup's LDS counters (the reads_cap = CUs << 30 split of exon_op_qual_pos_hist_chunks needs
more than 2^30 reads in one launch); reads outside their buffer and negative view lengths (the header promises nothing).
"""
import collections

import numpy as np
import pytest

import exon_amd
import k5_expect as E

pytestmark = pytest.mark.gpu

GUARD, MARK = 64, 0x5A5A5A5A5A5A5A5A
LAUNCHES = collections.Counter()  # ABI calls per group, printed at the end of the module (pytest -s)


@pytest.fixture(scope="module", autouse=True)
def _launch_counts():
    yield
    print("\nK5 limits, ABI calls per group:", dict(sorted(LAUNCHES.items())))


class Hist:
    """an int64 [lmax, 256] histogram in HBM between GUARD words of MARK on each side"""

    def __init__(self, ctx, lmax, fill=0):
        self.lmax = lmax
        h = np.full(lmax * 256 + 2 * GUARD, MARK, np.int64)
        h[GUARD:-GUARD] = fill
        self.buf = ctx.to_device(h)
        self.ptr = self.buf.ptr + 8 * GUARD

    def read(self, label=None):
        h = self.buf.to_host()
        assert (h[:GUARD] == MARK).all() and (h[-GUARD:] == MARK).all(), ("guard words", label)
        return h[GUARD:-GUARD].reshape(self.lmax, 256)


def qual(rng, total):
    """Phred+33 bytes with about one byte in a hundred drawn from all 256 values"""
    d = rng.integers(33, 75, total, dtype=np.uint8)
    if total:
        k = total // 100 + 1
        d[rng.integers(0, total, k)] = rng.integers(0, 256, k)
    return d


def arrow(ctx, group, off, data, lmax, label):
    d_off, d_data = ctx.to_device(off), ctx.to_device(data)
    h = Hist(ctx, lmax)
    ctx.qual_pos_hist(d_off, d_data, len(off) - 1, lmax, h)
    LAUNCHES[group] += 1
    ctx.sync()
    assert np.array_equal(h.read(label), E.hist_column(off, data, lmax)), label


def views(ctx, group, starts, ends, text, lmax, label):
    starts, ends = np.asarray(starts, np.int32), np.asarray(ends, np.int32)
    d_text, d_s, d_e = ctx.to_device(text), ctx.to_device(starts), ctx.to_device(ends)
    h = Hist(ctx, lmax)
    ctx.qual_pos_hist_views(d_text, d_s, d_e, len(starts), lmax, h)
    LAUNCHES[group] += 1
    ctx.sync()
    assert np.array_equal(h.read(label), E.hist(starts, ends, text, lmax)), label


# ---- 1. every length class at every alignment ----------------------------------------------------------------------------------
LENGTHS = (E.B_LENGTHS + [9, 11, 15] + [18, 30, 32, 60] + [17, 31, 34, 62, 64, 124]
           + [33, 63, 65, 66, 100, 101, 127, 128, 129, 150, 151, 250, 251, 255, 256, 257, 301, 309, 310] + [311, 312, 400])
SHIFTS = [0, 1, 2, 3, 4, 8, 15, 16, 17]
NS = [1, 2, 3, 4, 5, 63, 64, 65, 257, 1025]


def test_the_length_list_covers_every_class():
    assert {E.length_class(L) for L in LENGTHS} == {"B", "A4", "A2", "A1", "G"} and len(set(LENGTHS)) == len(LENGTHS) == 50


@pytest.mark.parametrize("cls", ["B", "A4", "A2", "A1", "G"])
def test_every_length_at_every_residue_and_read_count(ctx, cls):
    """one chunk, Arrow form: every length with every first-byte residue and with every small read count, lmax = L and L + 1
    (a B-class length off a 16-byte boundary silently becomes path G and must still be exact)"""
    for L in [L for L in LENGTHS if E.length_class(L) == cls]:
        rng = np.random.default_rng(L)
        combos = [(s, int(rng.choice(NS))) for s in SHIFTS] + [(int(rng.choice(SHIFTS)), n) for n in NS]
        flip = int(rng.integers(0, 2))
        for i, (shift, n) in enumerate(combos):
            lmax = L + ((i + flip) & 1)
            off, data = E.column(np.full(n, L), shift, payload=lambda t: qual(rng, t))
            arrow(ctx, 1, off, data, lmax, dict(L=L, cls=cls, lmax=lmax, shift=shift, n=n))


@pytest.mark.parametrize("L", [100, 7])
def test_lmax_around_the_template_the_layout_and_the_pt_switch(ctx, L):
    """lmax 128 | 129: k5_main<128> | <256>; 256 | 257: path G byte-major | [p][129]; 310 | 311: all positions in LDS | capped"""
    rng = np.random.default_rng(1000 + L)
    for lmax in (127, 128, 129, 255, 256, 257, 309, 310, 311):
        for shift in SHIFTS:
            n = int(rng.choice(NS))
            off, data = E.column(np.full(n, L), shift, payload=lambda t: qual(rng, t))
            arrow(ctx, 1, off, data, lmax, dict(L=L, cls=E.length_class(L), lmax=lmax, shift=shift, n=n))
        # the same lmax with ragged reads up to it (path G whatever the alignment)
        lens = rng.integers(0, lmax + 1, 65)
        lens[:2] = (lmax, 0)
        off, data = E.column(lens, int(rng.choice(SHIFTS)), payload=lambda t: qual(rng, t))
        arrow(ctx, 1, off, data, lmax, dict(ragged=True, lmax=lmax))


@pytest.mark.parametrize("L,shift", [(7, 0), (36, 3), (101, 1), (310, 17)])
def test_a_payload_that_gives_every_wave_several_rows(ctx, L, shift):
    """~6 MiB: 16 waves x every CU x 256-byte rows x a few, so path A's rolling window and path B's grid-stride loop both run"""
    rng = np.random.default_rng(2000 + L)
    n = (6 << 20) // L
    off, data = E.column(np.full(n, L), shift, payload=lambda t: qual(rng, t))
    arrow(ctx, 1, off, data, L, dict(L=L, cls=E.length_class(L), lmax=L, shift=shift, n=n))


# ---- 2. every byte value on every path -------------------------------------------------------------------------------------------
def _representative(name, rng):
    if name == "A":
        return np.full(3000, 101), 101
    if name == "B":
        return np.full(4000, 16), 16
    lmax = 200 if name == "G byte-major" else 700
    lens = rng.integers(0, lmax + 1, 3000 if lmax == 200 else 2000)
    lens[:3] = (lmax, 0, lmax - 1)
    return lens, lmax


PAYLOADS = {
    "uniform over 0..255": lambda rng, t: rng.integers(0, 256, t, dtype=np.uint8),
    "all 0xFF": lambda rng, t: np.full(t, 0xFF, np.uint8),
    "0x7F / 0x80 alternating": lambda rng, t: np.where(np.arange(t) % 2 == 0, 0x7F, 0x80).astype(np.uint8),
}


@pytest.mark.parametrize("name", ["A", "B", "G byte-major", "G position-major"])
def test_every_byte_value_on_every_path(ctx, name):
    rng = np.random.default_rng(len(name))
    lens, lmax = _representative(name, rng)
    assert name != "G position-major" or (lens > 310).sum() > 100
    for pname, fn in PAYLOADS.items():
        off, data = E.column(lens, 0, payload=lambda t: fn(rng, t))
        arrow(ctx, 2, off, data, lmax, (name, pname))


# ---- 3. long reads ---------------------------------------------------------------------------------------------------------------
LONG_LENGTHS = [0, 1, 2, 3, 4, 5] + [m + d for m in range(128, 1025, 128) for d in (-1, 0, 1)] + [309, 310, 311]


@pytest.mark.parametrize("lmax,seeds", [(311, 3), (1000, 3), (5000, 2), (65536, 1)])
def test_ragged_long_reads(ctx, lmax, seeds):
    for seed in range(seeds):
        rng = np.random.default_rng(lmax + seed)
        pool = [k for k in LONG_LENGTHS if k <= lmax]
        lens = rng.choice(pool, 300)
        lens[:3] = (lmax, 0, lmax - 1)
        rng.shuffle(lens)
        off, data = E.column(lens, (0, 5, 2)[seed], payload=lambda t: qual(rng, t))
        arrow(ctx, 3, off, data, lmax, dict(lmax=lmax, seed=seed))


@pytest.mark.parametrize("L", [311, 1000, 5000])
def test_uniform_long_reads(ctx, L):
    rng = np.random.default_rng(L)
    for shift in (0, 5):
        off, data = E.column(np.full(70, L), shift, payload=lambda t: qual(rng, t))
        arrow(ctx, 3, off, data, L, dict(L=L, cls=E.length_class(L), lmax=L, shift=shift, n=70))


def test_lmax_out_of_range_is_refused(ctx):
    off, data = E.column([4, 4])
    d_off, d_data = ctx.to_device(off), ctx.to_device(data)
    d_s, d_e = ctx.to_device(off[:-1]), ctx.to_device(off[1:])
    d = ctx.zeros(np.int64, 16)  # never written: the calls are refused before anything is launched
    for lmax in (0, (1 << 20) + 1):
        for call in (lambda: ctx.qual_pos_hist(d_off, d_data, 2, lmax, d),
                     lambda: ctx.qual_pos_hist_chunks([(d_off, d_data, 2)], lmax, d),
                     lambda: ctx.qual_pos_hist_views(d_data, d_s, d_e, 2, lmax, d)):
            with pytest.raises(exon_amd.ExonHipError, match="lmax") as e:
                call()
            assert e.value.code == -1  # EXON_HIP_EINVAL
    with pytest.raises(exon_amd.ExonHipError, match="lmax") as e:
        ctx.plan_qual_pos_hist(65537)
    assert e.value.code == -1
    ctx.sync()
    assert not d.to_host().any()


# ---- 4. the views form -----------------------------------------------------------------------------------------------------------
NS_V = [1, 3, 4, 5, 7, 8, 9, 1027]


def _text(rng, shift, span):
    """`shift` junk bytes, `span` bytes the views may index (all of them random: a byte counted from a gap changes the answer),
    320 junk bytes"""
    return np.concatenate([np.full(shift, E.JUNK_FRONT, np.uint8), qual(rng, span), np.full(E.BACK_BYTES, E.JUNK_BACK, np.uint8)])


@pytest.mark.parametrize("L", [16, 36, 101, 310])
def test_uniform_views_contiguous_and_with_gaps(ctx, L):
    """contiguous uniform views take paths A / B behind the non-CONTIG offsets scan; one gap anywhere must send them to path G"""
    rng = np.random.default_rng(4000 + L)
    for shift in (0, 3):
        for n in NS_V:
            base = shift + L * np.arange(n, dtype=np.int64)
            shapes = {"contiguous": base, "newline after every read": base + np.arange(n)}
            if n >= 2:
                g = base.copy()
                g[-1] += 1
                shapes["gap between the last two reads"] = g
            for k in [k for k in (1, 2, 200) if 4 * k < n]:
                g = base.copy()
                g[4 * k:] += 1
                shapes["gap at read %d" % (4 * k)] = g
            for shape, starts in shapes.items():
                text = _text(rng, shift, int(starts[-1]) + L - shift)
                views(ctx, 4, starts, starts + L, text, L + (n & 1), dict(L=L, cls=E.length_class(L), shift=shift, n=n, shape=shape))


@pytest.mark.parametrize("n", NS_V)
def test_views_in_any_order_overlapping_repeated_ragged(ctx, n):
    rng = np.random.default_rng(4500 + n)
    for L, shift in ((16, 0), (101, 3)):
        label = dict(L=L, shift=shift, n=n)
        text = _text(rng, shift, (L + 1) * n)
        asc = shift + (L + 1) * np.arange(n, dtype=np.int64)
        views(ctx, 4, asc[::-1], asc[::-1] + L, text, L, dict(label, shape="descending, newline gaps"))
        asc = shift + L * np.arange(n, dtype=np.int64)
        views(ctx, 4, asc[::-1], asc[::-1] + L, text, L, dict(label, shape="descending, back to back"))
        over = shift + 7 * np.arange(n, dtype=np.int64) % (L * n)
        views(ctx, 4, over, over + L, text, L, dict(label, shape="overlapping"))
        one = np.full(n, shift + min(5, n - 1), np.int64)
        views(ctx, 4, one, one + L, text, L, dict(label, shape="one view repeated"))
        lmax = 3 * L
        lens = rng.integers(0, min(lmax, (L + 1) * n) + 1, n)
        lens[rng.integers(0, n, 1 + n // 3)] = 0
        starts = shift + np.array([rng.integers(0, (L + 1) * n - k + 1) for k in lens], np.int64)
        views(ctx, 4, starts, starts + lens, text, lmax, dict(label, shape="ragged with empty views", lmax=lmax))


# ---- 5. chunks ---------------------------------------------------------------------------------------------------------------------
COUNTS = [1, 2, 63, 64, 65, 128, 129]


def _chunks(ctx, specs, rng, lmax):
    """specs: [(lens, shift)] -> (device chunk list for qual_pos_hist_chunks, the reference of their sum)"""
    want = np.zeros((lmax, 256), np.int64)
    dev = []
    for lens, shift in specs:
        off, data = E.column(lens, shift, payload=lambda t: qual(rng, t))
        dev.append((ctx.to_device(off), ctx.to_device(data), len(lens)))
        want += E.hist_column(off, data, lmax)
    return dev, want


def _direct(ctx, dev, want, lmax, label, fill=0):
    h = Hist(ctx, lmax, fill)
    ctx.qual_pos_hist_chunks(dev, lmax, h)
    LAUNCHES[5] += 1
    ctx.sync()
    assert np.array_equal(h.read(label), want + fill), label


def _chunk_lists(count, rng):
    """name -> (specs, lmax): the chunk lists of group 5 for one chunk count"""
    sizes = lambda: rng.integers(1, 51, count)  # noqa: E731
    out = {}
    for L, good, bad in ((101, 3, 6), (16, 0, 5)):
        out["uniform L=%d" % L] = ([(np.full(m, L), good) for m in sizes()], L)
        for where, at in (("first", 0), ("middle", count // 2), ("last", count - 1)):
            out["uniform L=%d, %s chunk misaligned" % (L, where)] = ([(np.full(m, L), bad if c == at else good) for c, m in enumerate(sizes())], L)
    out["lengths differ from chunk to chunk"] = ([(np.full(m, (101, 16, 36, 7, 100)[c % 5]), 0) for c, m in enumerate(sizes())], 101)
    first = np.full(int(rng.integers(2, 51)), 101)
    first[0] = 64
    out["the first read alone differs"] = ([(first, 0)] + [(np.full(m, 101), 0) for m in sizes()[1:]], 101)
    empty = {0, count - 1} | set(rng.integers(0, count, 1 + count // 4).tolist())
    out["empty chunks among the others"] = ([(np.full(0 if c in empty else m, 101), 4) for c, m in enumerate(sizes())], 101)
    return out


@pytest.mark.parametrize("count", COUNTS)
def test_chunk_lists_across_the_64_chunk_launches(ctx, count):
    """the ABI runs 64 chunks per launch: the first launch takes the caller's flags, the later ones accumulate"""
    rng = np.random.default_rng(5000 + count)
    for name, (specs, lmax) in _chunk_lists(count, rng).items():
        dev, want = _chunks(ctx, specs, rng, lmax)
        _direct(ctx, dev, want, lmax, (count, name), fill=3)
    # all chunks empty: an accumulating call leaves the histogram as it was
    dev, want = _chunks(ctx, [(np.zeros(0, np.int64), 0)] * count, rng, 40)
    assert not want.any()
    _direct(ctx, dev, want, 40, (count, "all chunks empty"), fill=7)


@pytest.mark.parametrize("count", [1, 64, 65, 129])
def test_chunk_lists_through_a_plan(ctx, count):
    """exon_hip_plan_launch_chunks in overwrite mode over a state full of garbage: the first fused launch overwrites, the later
    ones must add"""
    rng = np.random.default_rng(5500 + count)
    for name, (specs, lmax) in _chunk_lists(count, rng).items():
        dev, want = _chunks(ctx, specs, rng, lmax)
        plan = ctx.plan_qual_pos_hist(lmax)
        h = Hist(ctx, lmax, fill=0x1234567)
        plan.launch_chunks([([(d_data, None, d_off)], n) for d_off, d_data, n in dev], h.ptr, overwrite=True)
        LAUNCHES[5] += 1
        ctx.sync()
        assert np.array_equal(h.read((count, name)), want), (count, name)
        plan.close()


@pytest.mark.parametrize("count", [65, 129])
def test_batches_through_a_stream_and_a_second_cycle(ctx, count):
    """a stream opens in overwrite mode: `count` pushed batches end with exactly the reference, and after reset() the same
    batches give the same numbers again"""
    rng = np.random.default_rng(5800 + count)
    specs, lmax = _chunk_lists(count, rng)["lengths differ from chunk to chunk"]
    dev, want = _chunks(ctx, specs, rng, lmax)
    plan = ctx.plan_qual_pos_hist(lmax)
    st = plan.open()
    for cycle in range(2):
        for d_off, d_data, n in dev:
            st.push_device([(d_data, None, d_off)], n)
            LAUNCHES[5] += 1
        counts, _ = st.finish()
        assert np.array_equal(np.asarray(counts).reshape(lmax, 256), want), (count, cycle)
        st.reset()
    st.close()
    plan.close()


# ---- 6. accumulation ---------------------------------------------------------------------------------------------------------------
def _class_column(cls, rng, lmax):
    if cls == "A":
        return E.column(np.full(500, 101), 3, payload=lambda t: qual(rng, t))
    if cls == "B":
        return E.column(np.full(700, 16), 0, payload=lambda t: qual(rng, t))
    lens = rng.integers(0, lmax + 1, 400)
    lens[:2] = (lmax, 0)
    return E.column(lens, 1, payload=lambda t: qual(rng, t))


@pytest.mark.parametrize("x,y", [("A", "A"), ("B", "B"), ("G", "G"), ("A", "G"), ("G", "B"), ("B", "A")])
def test_launches_accumulate_into_one_histogram(ctx, x, y):
    """x == y: the same column twice gives twice the reference; otherwise column X then column Y of another class into one
    lmax-sized histogram: flags[0] left by one launch does not leak into the next launch's answer"""
    rng = np.random.default_rng(ord(x) * 256 + ord(y))
    lmax = 128
    X = _class_column(x, rng, lmax)
    Y = X if x == y else _class_column(y, rng, lmax)
    h = Hist(ctx, lmax)
    for off, data in (X, Y):
        ctx.qual_pos_hist(ctx.to_device(off), ctx.to_device(data), len(off) - 1, lmax, h)
        LAUNCHES[6] += 1
    ctx.sync()
    assert np.array_equal(h.read((x, y)), E.hist_column(*X, lmax) + E.hist_column(*Y, lmax)), (x, y)


# ---- 7. a read longer than lmax ------------------------------------------------------------------------------------------------------
def _refused_then_clean(ctx, form, lens, lmax, label):
    rng = np.random.default_rng(len(lens))
    off, data = E.column(lens, 0, payload=lambda t: qual(rng, t))
    with pytest.raises(ValueError, match="longer than lmax"):
        E.hist_column(off, data, lmax)
    ok_off, ok_data = E.column(np.minimum(lens, lmax), 2, payload=lambda t: qual(rng, t))
    keep = [ctx.to_device(a) for a in (off, data, off[:-1], off[1:], ok_off, ok_data, ok_off[:-1], ok_off[1:])]

    def launch(h, k):
        if form == "arrow":
            ctx.qual_pos_hist(keep[k], keep[k + 1], len(lens), lmax, h)
        else:
            ctx.qual_pos_hist_views(keep[k + 1], keep[k + 2], keep[k + 3], len(lens), lmax, h)
        LAUNCHES[7] += 1

    h = Hist(ctx, lmax)
    launch(h, 0)
    with pytest.raises(exon_amd.ExonHipError, match="read longer than lmax"):
        ctx.sync()
    h.read(label)  # the guard words; the histogram's contents after the error are undefined
    h = Hist(ctx, lmax)
    launch(h, 4)
    ctx.sync()  # clean
    assert np.array_equal(h.read(label), E.hist_column(ok_off, ok_data, lmax)), label


LMAX7 = 100
PLACEMENTS = [("main loop, read 0", 1030, 0), ("main loop, read 300 (lane 11 of wave 1)", 1030, 300), ("main loop, read 1023 (lane 63)", 1030, 1023),
              ("tail, n = 5", 5, 4), ("tail, n = 6", 6, 5), ("tail, n = 7", 7, 6), ("tail, n = 1", 1, 0)]


@pytest.mark.parametrize("form", ["arrow", "views"])
@pytest.mark.parametrize("where,n,at", PLACEMENTS)
def test_one_read_longer_than_lmax(ctx, form, where, n, at):
    lens = np.full(n, 50)
    lens[at] = LMAX7 + 1
    _refused_then_clean(ctx, form, lens, LMAX7, (form, where))


@pytest.mark.parametrize("form", ["arrow", "views"])
@pytest.mark.parametrize("n", [5, 64])
def test_every_read_longer_than_lmax(ctx, form, n):
    _refused_then_clean(ctx, form, np.full(n, LMAX7 + 1), LMAX7, (form, "uniform", n))


# ---- 8. through a file -----------------------------------------------------------------------------------------------------------------
def test_long_reads_through_a_fastq_file(ctx, tmp_path):
    """~40 ragged reads of up to 20 000 bases and a few of 1-5, parsed on the device, lmax = 32768"""
    rng = np.random.default_rng(8)
    lens = np.concatenate([rng.integers(6, 20001, 38), [20000, 19999], [1, 2, 3, 4, 5]])
    rng.shuffle(lens)
    quals = [rng.integers(33, 75, int(k), dtype=np.uint8) for k in lens]
    path = tmp_path / "long.fastq"
    with open(path, "wb") as f:
        for i, q in enumerate(quals):
            f.write(b"@r%d\n" % i + bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), q.size)) + b"\n+\n" + q.tobytes() + b"\n")
    lmax = 32768
    off, data = E.column(lens, 0, payload=np.concatenate(quals))
    want = E.hist_column(off, data, lmax)
    got = {}
    for gpu_parse in (True, False):
        scan = exon_amd.Scan(str(path), "fastq", gpu_parse=gpu_parse)
        plan = ctx.plan_qual_pos_hist(lmax, columns=(3,))
        st = plan.open()
        rows = st.consume(scan)
        LAUNCHES[8] += 1
        counts, _ = st.finish()
        st.close()
        plan.close()
        assert scan.decoded_on_gpu()[0] == gpu_parse, "silent host fallback"
        scan.close()
        assert rows == len(lens)
        got[gpu_parse] = np.asarray(counts).reshape(lmax, 256)
        assert np.array_equal(got[gpu_parse], want), gpu_parse
    assert np.array_equal(got[True], got[False])
