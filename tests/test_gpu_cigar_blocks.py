"""GPU: exon_hip_cigar_blocks against the Python statement of the rule (cigar_blocks_expect.py), element for element: row counts around
the wave and the scan workgroup, rows without ops, with uncounted ops only, with one op, with one-base blocks, one record of 65 535
ops, many-block rows across the scan workgroup's seam, NULL rows, a list that does not start at offset 0, a capacity that fits
exactly and one that is one short (nothing is written then, and a guard pattern behind every buffer stays intact in both), the mask
that gives the span back, and the block rows fed to the operators of kinds 12, 13 and 14."""
import ctypes

import numpy as np
import pytest

import bam_sam_writer as bsw
import exon_amd

import cigar_blocks_expect as E
import region_bases_expect as E12
import region_depth_expect as E14
import window_bases_expect as E13
from region_set_expect import pack_bits

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY = -1, -6
GUARD = 64
PAT32, PAT64, PAT8 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A, 0x5A


class Blocks:
    """one call: inputs on the device, outputs with GUARD elements of a pattern behind `cap`, everything copied back"""

    def __init__(self, ctx, ref, start, cigars, mask, rv=None, sv=None, first=0, cap=None):
        ref, start = np.asarray(ref, np.int32), np.asarray(start, np.int64)
        n = len(cigars)
        self.want = E.expand(ref, start, cigars, mask, rv, sv)
        self.total = len(self.want[0])
        self.cap = cap = self.total if cap is None else cap
        offsets, ops = E.list_columns(cigars, first)
        self.d_in = [ctx.to_device(np.concatenate([ref, np.zeros(8, np.int32)])), ctx.to_device(np.concatenate([start, np.zeros(8, np.int64)])),
                     ctx.to_device(offsets), ctx.to_device(np.concatenate([ops, np.zeros(4, np.uint32)]))]
        self.d_v = [None if v is None else ctx.to_device(np.concatenate([pack_bits(np.asarray(v, bool)), np.zeros(64, np.uint8)])) for v in (rv, sv)]
        self.vbytes = (cap + 31) // 32 * 4
        self.d_out = [ctx.to_device(np.full(cap + GUARD, PAT32, np.int32)), ctx.to_device(np.full(cap + GUARD, PAT64, np.int64)),
                      ctx.to_device(np.full(cap + GUARD, PAT64, np.int64)), ctx.to_device(np.full(self.vbytes + GUARD, PAT8, np.uint8))]
        self.error = None
        try:
            self.got = ctx.cigar_blocks(self.d_in[0], self.d_v[0], self.d_in[1], self.d_v[1], self.d_in[2], self.d_in[3], n, mask, *self.d_out, cap)
        except exon_amd.ExonHipError as e:
            self.error = e
        self.out = [d.to_host() for d in self.d_out]

    def check(self):
        """the rows == the expectation; behind them, and behind the capacity, the pattern"""
        assert self.error is None, self.error
        t = self.total
        assert self.got == t
        for o, w, pat in zip(self.out[:3], self.want[:3], (PAT32, PAT64, PAT64)):
            assert np.array_equal(o[:t], w)
            assert (o[t:] == pat).all()
        bits = np.unpackbits(self.out[3][:(t + 31) // 32 * 4], bitorder="little")
        assert np.array_equal(bits[:t].astype(bool), self.want[3]) and bits[t:].all()
        assert (self.out[3][(t + 31) // 32 * 4:] == PAT8).all()
        return self

    def untouched(self):
        for o, pat in zip(self.out, (PAT32, PAT64, PAT64, PAT8)):
            assert (o == pat).all()


def mixed_rows(rng, n, null=0.1):
    """rows without ops, with uncounted ops only, with one op, with one-base blocks, spliced, and random ones"""
    kinds = [[], E.cigar("5S3I2H4P"), E.cigar("1M1N" * 7), E.cigar("50M1000N50M"), E.cigar("10M5I10M"), E.cigar("5M3D5M"), E.cigar("4N"), E.cigar("0M")]
    cigars = []
    for i in range(n):
        r = int(rng.integers(0, 12))
        if r < len(kinds):
            cigars.append(kinds[r])
        elif r == 8:
            cigars.append([(int(rng.integers(0, 200)), int(rng.integers(0, 16)))])
        else:
            k = int(rng.integers(1, 10))
            cigars.append([(int(ln), int(c)) for ln, c in zip(rng.choice([0, 1, 2, 30, 151], k), rng.choice([0, 0, 1, 2, 3, 4, 7, 8, 11], k))])
    ref = rng.integers(-1, 5, n).astype(np.int32)
    start = rng.integers(1, 3000, n)
    return ref, start, cigars, rng.random(n) >= null, rng.random(n) >= null


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("mask", [E.ALIGNED, E.ALIGNED_DEL])
def test_row_counts(ctx, n, mask):
    rng = np.random.default_rng(1000 + n)
    ref, start, cig, rv, sv = mixed_rows(rng, n)
    b = Blocks(ctx, ref, start, cig, mask, rv, sv).check()
    if n == 0:
        b.untouched()
    elif n >= 63:
        assert b.total > n and not b.want[3].all()


def test_rows_of_each_kind(ctx):
    cig = [[], E.cigar("5S3I"), E.cigar("7M"), E.cigar("1M1N" * 50), E.cigar("0M"), E.cigar("3N"), [(5, 12), (4, 0)]]
    b = Blocks(ctx, [3] * len(cig), [10 * (i + 1) for i in range(len(cig))], cig, E.ALIGNED).check()
    r, s, e, v = b.want
    assert v.all() and (r == 3).all()
    assert list(zip(s.tolist(), e.tolist())) == [(10, 9), (20, 19), (30, 36)] + [(40 + 2 * j, 40 + 2 * j) for j in range(50)] + [(50, 49), (60, 59), (70, 73)]


def test_one_record_of_65535_ops_between_one_op_neighbours(ctx):
    long = [(1, 0), (1, 3)] * 32767 + [(1, 0)]
    for mask, k in ((E.ALIGNED, 32768), (E.LEGAL, 1)):
        b = Blocks(ctx, [0, 1, 2], [5, 100, 7], [E.cigar("9M"), long, E.cigar("4M")], mask).check()
        assert b.total == k + 2


def test_many_block_rows_across_the_scan_workgroup_seam(ctx):
    n = 600
    cig = [E.cigar("20M")] * n
    cig[255], cig[256], cig[511] = E.cigar("1M1N" * 300), E.cigar("2M3D" * 257), E.cigar("1M1N" * 70)
    b = Blocks(ctx, np.arange(n) % 4, 1 + 3 * np.arange(n), cig, E.ALIGNED).check()
    assert b.total == n - 3 + 300 + 257 + 70


@pytest.mark.parametrize("which", [0, 1])
def test_null_reference_and_null_position_rows(ctx, which):
    rng = np.random.default_rng(5 + which)
    ref, start, cig, _, _ = mixed_rows(rng, 500)
    v = [None, None]
    v[which] = rng.random(500) < 0.5
    b = Blocks(ctx, ref, start, cig, E.ALIGNED, *v).check()
    # an invalid row is one invalid row of zeros, whatever its ops
    assert (~b.want[3]).sum() == (~v[which]).sum() > 0 and not b.want[0][~b.want[3]].any() and not b.want[1][~b.want[3]].any()


def test_a_list_that_does_not_start_at_offset_0(ctx):
    rng = np.random.default_rng(9)
    ref, start, cig, rv, sv = mixed_rows(rng, 300)
    Blocks(ctx, ref, start, cig, E.ALIGNED_DEL, rv, sv, first=5).check()  # (the five words in front are ops of 2^28 - 1 M)


@pytest.mark.parametrize("n", [1, 257, 1000])
def test_capacity_exact_and_one_short(ctx, n):
    rng = np.random.default_rng(40 + n)
    ref, start, cig, rv, sv = mixed_rows(rng, n)
    cig[0] = E.cigar("3M2N3M")  # (more rows than records even for n = 1)
    rv[0] = sv[0] = True
    ok = Blocks(ctx, ref, start, cig, E.ALIGNED, rv, sv).check()
    short = Blocks(ctx, ref, start, cig, E.ALIGNED, rv, sv, cap=ok.total - 1)
    assert short.error is not None and short.error.code == ECAPACITY and short.error.need == ok.total
    short.untouched()
    none = Blocks(ctx, ref, start, cig, E.ALIGNED, rv, sv, cap=0)
    assert none.error.code == ECAPACITY and none.error.need == ok.total
    none.untouched()
    Blocks(ctx, ref, start, cig, E.ALIGNED, rv, sv, cap=ok.total + 37).check()


def test_the_span_mask_gives_one_row_per_record_equal_to_the_span(ctx):
    rng = np.random.default_rng(50)
    ref, start, cig, rv, sv = mixed_rows(rng, 1000)
    b = Blocks(ctx, ref, start, cig, E.LEGAL, rv, sv).check()
    assert b.total == 1000
    valid = rv & sv
    span = np.array([sum(ln for ln, c in ops if c in E.REF_CODES) for ops in cig])
    assert np.array_equal(b.out[0][:1000][valid], ref[valid]) and np.array_equal(b.out[1][:1000][valid], start[valid])
    assert np.array_equal(b.out[2][:1000][valid], (start + span - 1)[valid])  # `end` as the readers compute it
    assert np.array_equal(np.unpackbits(b.out[3][:125], bitorder="little").astype(bool), valid)


REGIONS = [(0, 100, 180), (0, 181, 260), (1, 500, 1999), (1, 700, 2100), (2, 1, 50), (3, 1200, 1300), (0, 1000, 2500)]


def test_block_rows_feed_kinds_12_13_and_14(ctx):
    rng = np.random.default_rng(60)
    ref, start, cig, rv, sv = mixed_rows(rng, 3000)
    for mask in (E.ALIGNED, E.ALIGNED_DEL, E.LEGAL):
        b = Blocks(ctx, ref, start, cig, mask, rv, sv).check()
        r, s, e, v = b.want
        cols = (b.d_out[0], b.d_out[3], b.d_out[1], b.d_out[3], b.d_out[2], b.d_out[3], b.total)  # ONE bitmap for the three columns

        p12 = ctx.plan_region_set_bases(REGIONS, columns=(0, 1, 2))
        d = ctx.zeros(np.int64, p12.n_i64)
        ctx.region_set_bases(*cols, p12, d)
        ctx.sync()
        st = d.to_host()
        assert np.array_equal(st, E12.expect_state(REGIONS, r, s, e, v, v, v))
        assert st[0] > 0 and st[1] == (~v).sum() and st[3] > 0  # block rows counted; a record without a block lands in `inverted`

        contigs = [(0, 3000), (1, 2500), (3, 1250)]
        p13 = ctx.plan_window_bases(contigs, 100, columns=(0, 1, 2))
        d = ctx.zeros(np.int64, p13.n_i64)
        ctx.window_bases(*cols, p13, d)
        ctx.sync()
        assert np.array_equal(d.to_host(), E13.expect_state(contigs, 100, r, s, e, v, v, v))

        p14 = ctx.plan_region_set_depth(REGIONS, [1, 2, 5], columns=(0, 1, 2))
        d = ctx.zeros(np.int64, p14.n_i64)
        ctx.region_set_depth(*cols, p14, d)
        ctx.sync()
        st = d.to_host()
        assert np.array_equal(st, E14.expect_state(REGIONS, r, s, e, v, v, v))
        # ... and the per-base depth is the pile-up of the blocks
        pile = E.pileup(5, 4000, r, s, e, v)
        order, _ = E14.slots(REGIONS)
        assert np.array_equal(p14.per_base(st), np.concatenate([pile[c, E14.positions(iv)] for c, iv in zip(order, E14.merged(REGIONS))]))
        for p in (p12, p13, p14):
            p.close()


def test_a_spliced_read_leaves_its_intron_uncovered(ctx):
    regions = [(0, 2000, 2999)]  # inside the intron of 50M10000N50M at 1000
    for mask, bases in ((E.ALIGNED, 0), (E.LEGAL, 1000)):
        b = Blocks(ctx, [0], [1000], [E.cigar("50M10000N50M")], mask).check()
        p = ctx.plan_region_set_bases(regions, columns=(0, 1, 2))
        d = ctx.zeros(np.int64, p.n_i64)
        ctx.region_set_bases(b.d_out[0], b.d_out[3], b.d_out[1], b.d_out[3], b.d_out[2], b.d_out[3], b.total, p, d)
        ctx.sync()
        assert p.decode(d.to_host()).tolist() == [bases]
        p.close()


def test_refusals(ctx):
    for mask in (0, 0x2, 0x200, 0x18D | 0x10, 0xFFFFFFFF):
        b = Blocks(ctx, [0], [1], [E.cigar("5M")], E.ALIGNED)
        with pytest.raises(exon_amd.ExonHipError) as e:
            ctx.cigar_blocks(b.d_in[0], None, b.d_in[1], None, b.d_in[2], b.d_in[3], 1, mask, *b.d_out, 1)
        assert e.value.code == EINVAL and "0x18D" in str(e.value)
    b = Blocks(ctx, [0], [1], [E.cigar("5M")], E.ALIGNED)
    for n, cap in ((-1, 1), (1, -1)):
        with pytest.raises(exon_amd.ExonHipError) as e:
            ctx.cigar_blocks(b.d_in[0], None, b.d_in[1], None, b.d_in[2], b.d_in[3], n, E.ALIGNED, *b.d_out, cap)
        assert e.value.code == EINVAL
    with pytest.raises(exon_amd.ExonHipError) as e:
        ctx.cigar_blocks(b.d_in[0], None, b.d_in[1], None, None, b.d_in[3], 1, E.ALIGNED, *b.d_out, 1)
    assert e.value.code == EINVAL
    # offsets out of order, or beyond their own last entry: refused by the count pass, no op is loaded for such a row, nothing is written
    ops = ctx.to_device(E.encode(E.cigar("1M1N1M1N1M1N1M1N")))
    ref, start = ctx.to_device(np.zeros(8, np.int32)), ctx.to_device(np.ones(8, np.int64))
    for offs in ([0, 5, 3, 8], [0, 4, 100, 8], [2, 1, 4, 8], [-1, 2, 4, 8]):
        out = Blocks(ctx, [0], [1], [[]], E.ALIGNED, cap=16)
        with pytest.raises(exon_amd.ExonHipError) as e:
            ctx.cigar_blocks(ref, None, start, None, ctx.to_device(np.array(offs, np.int32)), ops, 3, E.ALIGNED, *out.d_out, 16)
        assert e.value.code == EINVAL and "offsets" in str(e.value)
        assert all((d.to_host()[1:] == pat).all() for d, pat in zip(out.d_out[:3], (PAT32, PAT64, PAT64)))  # (row 0 is `out`'s own call)


def _fetch(ctx, ptr, dtype, n):
    out = np.empty(n, dtype)
    if n:
        ctx._check(ctx.lib.exon_hip_memcpy_d2h(ctx.h, out.ctypes.data_as(ctypes.c_void_p), ptr, out.nbytes, None))
    return out


def test_the_bam_slab_form_through_the_parser(ctx):
    """exon_hip_bam_parser_cigar_blocks, what a blocks-mode scan runs per slab: records written by bam_sam_writer (names of every length
    mod 4: unaligned ops; op codes beyond 8; unmapped and position-less records), split by the parser, with and without a row mask"""
    rng = np.random.default_rng(77)
    shapes = ["30M", "10M200N15M", "5S20M3D20M2I10M", "8=1X8=", "", "25N", "1M1N1M1N1M", "3I"]
    recs = []
    for i in range(700):
        cig = E.cigar(shapes[int(rng.integers(0, len(shapes)))]) + ([(3, 12)] if i % 13 == 0 else [])
        recs.append(dict(name="q" * (i % 4) + "x", flag=0, ref=None if i % 17 == 3 else i % 2, pos=0 if i % 19 == 7 else 10 + 5 * i, mapq=60, cigar=cig, seq="ACGTA", qual=[30] * 5))
    data = np.frombuffer(b"".join(bsw.bam_record(r) for r in recs), np.uint8)
    d = ctx.to_device(np.concatenate([data, np.zeros(64, np.uint8)]))
    parser = exon_amd.BAMParser(ctx, 2, len(data) + 64)
    cols = parser.parse(d, len(data))
    assert cols.n_rows == len(recs) and cols.n_undecided == 0
    ref = np.array([-1 if r["ref"] is None else r["ref"] for r in recs], np.int32)
    start = np.array([r["pos"] for r in recs], np.int64)
    rv, sv = ref >= 0, start >= 1
    keep = rng.random(len(recs)) < 0.7
    d_mask = ctx.to_device(np.concatenate([pack_bits(keep), np.zeros(64, np.uint8)]))
    for mask in (E.ALIGNED, E.ALIGNED_DEL, E.LEGAL):
        for row_mask, kept in ((None, rv), (d_mask, rv & keep)):
            n, und, out = parser.cigar_blocks(d, len(data), cols, mask, row_mask=row_mask)
            w_ref, w_s, w_e, w_v = E.expand(ref, start, [r["cigar"] for r in recs], mask, kept, sv)
            assert und == 0 and n == len(w_ref) and out[0].validity == out[1].validity == out[2].validity and out[0].values % 16 == 0
            assert np.array_equal(_fetch(ctx, out[0].values, np.int32, n), w_ref)
            assert np.array_equal(_fetch(ctx, out[1].values, np.int64, n), w_s) and np.array_equal(_fetch(ctx, out[2].values, np.int64, n), w_e)
            bits = np.unpackbits(_fetch(ctx, out[0].validity, np.uint8, (n + 7) // 8), bitorder="little")[:n].astype(bool)
            assert np.array_equal(bits, w_v)
    for bad in (0, 0x2, 0x200):
        with pytest.raises(exon_amd.ExonHipError) as e:
            parser.cigar_blocks(d, len(data), cols, bad)
        assert e.value.code == EINVAL and "0x18D" in str(e.value)
    other = exon_amd.BAMParser(ctx, 2, len(data) + 64)
    with pytest.raises(exon_amd.ExonHipError) as e:  # columns of another parser
        other.cigar_blocks(d, len(data), cols, E.ALIGNED)
    assert e.value.code == EINVAL
    other.close()
    # the CG-tag placeholder among valid records: undecided, nothing produced
    recs[300].update(cigar=[(5, 4), (900, 3)], ref=0, pos=40)
    data = np.frombuffer(b"".join(bsw.bam_record(r) for r in recs), np.uint8)
    d = ctx.to_device(np.concatenate([data, np.zeros(64, np.uint8)]))
    cols = parser.parse(d, len(data))
    n, und, _ = parser.cigar_blocks(d, len(data), cols, E.ALIGNED)
    assert (n, und) == (0, 1)
    parser.close()
