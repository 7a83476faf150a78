"""The device's record splitting (chain_walk.h: guessed starts, proven by induction) for BAM and BCF, and the BCF typed walk of
k_bcf_extract, at their limits -- against the plain statement of the two formats in record_expect.py.

The contract, for every slab: if n_undecided == 0, the rows, their order, every column, every validity bit and consumed_bytes
equal the statement exactly; if the statement refuses a record that lies wholly inside the slab, n_undecided > 0.  Every case
carries a label written down with it: MUST (decide: n_undecided == 0 is asserted) or MAY (hand back: the contract alone on the
parser, and the same bytes as a file through Scan(gpu_parse=True) give the host reader's rows).

Filler inside payloads is the byte 0x21: read as a length it is 0x21212121, more than any length the product follows, so no
offset inside filler can look like a record start and MUST is a property of how a slab is built.  Small records keep their own
fields away from what could be read as a chain of three headers: BAM positions lie above 2^25, bins at 4680, mates at -1."""
import struct

import numpy as np
import pytest

import bcf_typed_walk_cases as T
import exon_amd
import record_expect as X

pytestmark = pytest.mark.gpu
SEG = 65536
MUST, MAY = "must decide", "may hand back"
N_REF = 25
FILL = bytes([X.FILL])
FMTS = ["bam", "bcf"]


# ---- records of both formats behind one interface ------------------------------------------------------------------------------
class Bam:
    name, small_size, min_size = "bam", 61, 37

    @staticmethod
    def small(i, **kw):
        """61 bytes; mapq 255, ref -1 and pos -1 mixed"""
        f = dict(ref=-1 if i % 7 == 3 else 1 + i % 23, pos=-1 if i % 3 == 1 else (1 << 25) + 5 * i, name=b"r%04d\0" % (i % 10000),
                 mapq=255 if i % 5 == 2 else i % 60, cigar=[((10 + i % 90) << 4) | (0, 2, 4, 7)[i % 4]], flag=(i * 37) % 4096,
                 seq=FILL * 5, qual=FILL * 10)
        f.update(kw)
        return X.bam_record(**f)

    @classmethod
    def stretched(cls, i, total):
        """a small record with filler behind it (where the optional fields are), `total` bytes long"""
        return cls.small(i, aux=FILL * (total - cls.small_size))

    @staticmethod
    def tiny(i):
        """the smallest record: block_size 33 -- a one-byte name, no CIGAR, no sequence"""
        return X.bam_record(ref=-1 if i % 7 == 3 else i % N_REF, pos=-1 if i % 3 == 1 else (1 << 25) + i, name=b"\0",
                            mapq=255 if i % 5 == 2 else i % 60, flag=(i * 37) % 4096)

    @classmethod
    def carrier(cls, i, payload, via=0):
        """a record whose payload bytes are the last bytes of the record: via 0 a 'B' aux array of bytes, via 1 the qualities"""
        if via == 0:
            return cls.small(i, aux=b"XBBC" + struct.pack("<i", len(payload)) + payload)
        return cls.small(i, seq=FILL * ((len(payload) + 1) // 2), qual=payload)

    carrier_tail = 0  # bytes of the carrier behind its payload

    @staticmethod
    def row(rec):
        r = X.bam_row(rec, N_REF)
        return r if isinstance(r, X.Reject) else (r["flag"], r["mapq"], r["ref"], r["start"], r["end"])

    @staticmethod
    def parser(ctx, max_bytes):
        return exon_amd.BAMParser(ctx, N_REF, max_slab_bytes=max_bytes)

    @staticmethod
    def device_rows(res):
        n = res["n_rows"]
        mv, rv, pv = (bits(res[k], n) for k in ("mapq_valid", "ref_valid", "pos_valid"))
        return list(zip(res["flag"].tolist(), masked(res["mapq"], mv), masked(res["ref_id"], rv), masked(res["start"], pv), masked(res["end"], pv)))

    @staticmethod
    def file(body):
        return X.bam_file(body, N_REF)

    scan_kw = {}


class Bcf:
    name, small_size, min_size = "bcf", 58, 35

    @staticmethod
    def small(i, **kw):
        """58 bytes; QUAL missing and pos0 = -1 mixed"""
        f = dict(chrom=i % 2, pos0=-1 if i % 3 == 1 else i, qual_bits=X.FLOAT_MISSING if i % 5 == 2 else T.F1 + i,
                 id_=X.typed_str(b"s%04d" % (i % 10000)), alleles=(X.typed_str(b"A"), X.typed_str(b"C")), filter_=X.typed_ints([i % 3]),
                 info=[(T.key(T.AF), X.typed_floats([T.F2 + i])), (T.key(T.DP), X.typed_ints([i], width=3))])
        f.update(kw)
        return X.bcf_record(**f)

    @classmethod
    def stretched(cls, i, total):
        """a small record whose REF is filler (and up to six filler bytes behind the INFO pairs, where the descriptor's own length
        leaves a gap), `total` bytes long"""
        k = max(0, total - cls.small_size - 6)
        rec = cls.small(i, alleles=(X.typed_str(b"A" + FILL * k), X.typed_str(b"C")))
        return cls.small(i, alleles=(X.typed_str(b"A" + FILL * k), X.typed_str(b"C")), tail=FILL * (total - len(rec)))

    @staticmethod
    def tiny(i):
        """the smallest record: ID 0x07, one empty allele, FILTER 0x00"""
        return X.bcf_record(chrom=i % 2, pos0=-1 if i % 3 == 1 else i, qual_bits=X.FLOAT_MISSING if i % 5 == 2 else T.F1 + i,
                            alleles=(b"\x07",))

    @classmethod
    def carrier(cls, i, payload, via=0):
        """a record whose payload is an allele string: via 0 the last ALT of a record that ends one byte (FILTER 0x00) behind it,
        via 1 the REF of a small record"""
        if via == 0:
            return X.bcf_record(chrom=i % 2, pos0=i, id_=X.typed_str(b"c%04d" % i), alleles=(X.typed_str(b"A"), X.typed_str(payload)))
        rec = cls.small(i, alleles=(X.typed_str(payload), X.typed_str(b"C")))
        return rec

    carrier_tail = 1

    @staticmethod
    def row(rec):
        r = X.bcf_row(rec, T.N_CONTIGS, T.N_STRINGS, T.KEYS)
        if isinstance(r, X.Reject):
            return r
        return (r["chrom"], r["pos"], r["qual"], r["filter"]) + tuple(tuple(v) if isinstance(v, list) else v for v in r["info"])

    @staticmethod
    def parser(ctx, max_bytes):
        return exon_amd.BCFParser(ctx, T.N_CONTIGS, T.N_STRINGS, 0, [k for k, _ in T.KEYS], "".join(k for _, k in T.KEYS), max_slab_bytes=max_bytes)

    @staticmethod
    def device_rows(res):
        n = res["n_rows"]
        cols = [res["chrom_id"].tolist(), masked(res["pos"], bits(res["pos_valid"], n)), masked(res["qual"].view(np.uint32), bits(res["qual_valid"], n)),
                [res["filters"][f] for f in res["filter_id"].tolist()]]
        for k in res["infos"]:
            valid = bits(k["valid"], n)
            if k["kind"] == "b":
                cols.append([True if v else None for v in valid])
            elif k["kind"] in "FI":
                off = k["offsets"].tolist() if n else [0]
                vals = masked(k["values"].view(np.int32 if k["kind"] == "I" else np.uint32), bits(k["item_valid"], off[-1]))
                cols.append([tuple(vals[off[r]:off[r + 1]]) if valid[r] else None for r in range(n)])
                assert all(valid[r] or off[r] == off[r + 1] for r in range(n))  # a NULL list holds no items
            else:
                cols.append(masked(k["values"].view(np.int32 if k["kind"] == "i" else np.uint32), valid))
        return list(zip(*cols)) if n else []

    @staticmethod
    def file(body):
        return X.bcf_file(body)

    scan_kw = {"info_field": "AF,DP,DB"}  # (batches with list-valued keys come from the host reader whatever the scan is asked for)


F = {"bam": Bam, "bcf": Bcf}


def bits(bm, n):
    b = np.unpackbits(bm, bitorder="little")
    assert not b[n:].any()  # nothing set behind the last row
    return b[:n].astype(bool).tolist()


def masked(values, valid):
    return [v if ok else None for v, ok in zip(values.tolist(), valid)]


_rows = {}


def statement(fmt, data):
    """(rows -- a tuple, or a Reject, for every whole record --, consumed, the chain's Reject or None) by the plain statement"""
    offs, consumed, rej = X.split(data, fmt.name)
    rows = []
    for a, b in zip(offs, offs[1:] + [consumed]):
        rec = data[a:b]
        if rec not in _rows:
            _rows[rec] = fmt.row(rec)
        rows.append(_rows[rec])
    return rows, consumed, rej


def check(fmt, p, data, label, what=""):
    """the contract on one slab; -> the parser's result"""
    rows, consumed, rej = statement(fmt, data)
    res = p.parse_host(data)
    refused = rej is not None or any(isinstance(r, X.Reject) for r in rows)
    if label == MUST:
        assert len(data) > SEG, what  # a must-decide slab has more than one segment
        assert not refused, what      # (a slab the statement refuses cannot carry this label)
        assert res["n_undecided"] == 0, what
    if refused:
        assert res["n_undecided"] > 0, what
    if res["n_undecided"] == 0:
        assert res["n_rows"] == len(rows) and res["consumed_bytes"] == consumed, (what, res["n_rows"], len(rows), res["consumed_bytes"], consumed)
        got = fmt.device_rows(res)
        if got != rows:
            bad = next(i for i, (g, w) in enumerate(zip(got, rows)) if g != w)
            raise AssertionError(f"{what}: row {bad}: device {got[bad]}, statement {rows[bad]}")
    return res


class Refused:
    """a scan that ended in an error: equal to any other"""

    def __init__(self, msg):
        self.msg = msg

    def __eq__(self, other):
        return isinstance(other, Refused)

    def __repr__(self):
        return f"Refused({self.msg!r})"


def scan_rows(fmt, path, ctx=None):
    s = exon_amd.Scan(str(path), fmt.name, gpu_parse=ctx is not None, **fmt.scan_kw)
    try:
        if ctx is not None:
            s.bind_ctx(ctx)
        return [r for b in s for r in b.to_pylist()]
    except exon_amd.ExonHipError as e:
        return Refused(str(e))
    finally:
        s.close()


def check_file(fmt, ctx, tmp_path, data, what=""):
    """the same bytes as a file: the GPU pipeline gives the host reader's rows (or its error), whoever decoded them"""
    path = tmp_path / ("m." + fmt.name)
    path.write_bytes(fmt.file(data))
    host, gpu = scan_rows(fmt, path), scan_rows(fmt, path, ctx)
    assert gpu == host, what
    return host


def run_to(fmt, cur, target, i):
    """records (small ones, one of them stretched with filler) that fill the bytes cur .. target exactly"""
    n_small = (target - cur - fmt.small_size - 8) // fmt.small_size
    assert n_small >= 0, (cur, target)
    smalls = [fmt.small(i + j) for j in range(n_small)]
    mid = fmt.stretched(i + n_small, target - cur - n_small * fmt.small_size)
    out = smalls[:n_small // 2] + [mid] + smalls[n_small // 2:]
    assert sum(map(len, out)) == target - cur
    return out


def smalls(fmt, n, i=0):
    return [fmt.small(i + j) for j in range(n)]


# ---- sweeps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_record_starts_around_a_segment_edge(ctx, fmt):
    """A record starts at k * 65536 + d for every d in -40 .. 40: the header and the length field straddle the edge at every
    byte, a start exactly on the edge, one byte behind it.  Rows per segment are no multiple of 32."""
    fmt = F[fmt]
    p = fmt.parser(ctx, 6 * SEG)
    for k, d in [(1, d) for d in range(-40, 41)] + [(2, -5), (2, 0), (2, 1)]:
        recs = run_to(fmt, 0, k * SEG + d, 3 * d + 200)
        recs += smalls(fmt, ((k + 2) * SEG + 777 - (k * SEG + d)) // fmt.small_size, 11 * d + 500)
        data = b"".join(recs)
        res = check(fmt, p, data, MUST, f"k={k} d={d}")
        assert res["consumed_bytes"] == len(data) and res["n_rows"] == len(recs)
        starts = np.cumsum([0] + [len(r) for r in recs[:-1]])
        assert k * SEG + d in starts
        assert all(np.count_nonzero(starts // SEG == s) % 32 for s in range(k + 2))
    p.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_slab_cut_inside_its_last_record(ctx, fmt):
    """The last record starts at 2 * 65536 + d and the slab is cut j bytes into it: the rows in front of it, consumed_bytes = its
    start -- whether the cut falls into the length field, the header or the body, and whether the record starts in the last
    segment, on its edge or in the one before (which then ends the slab).  And a slab of whole segments that ends with a record."""
    fmt = F[fmt]
    p = fmt.parser(ctx, 6 * SEG)
    for d in (-40, -9, -8, -4, -1, 0, 1, 30):
        t = 2 * SEG + d
        recs = run_to(fmt, 0, t, 7 * d + 300)
        last = fmt.small(4242)
        full = b"".join(recs) + last
        for j in list(range(0, 41)) + [len(last) - 1]:
            res = check(fmt, p, full[:t + j], MUST, f"d={d} j={j}")
            assert res["consumed_bytes"] == t and res["n_rows"] == len(recs)
    data = b"".join(run_to(fmt, 0, 3 * SEG, 900))
    res = check(fmt, p, data, MUST, "whole segments")
    assert res["consumed_bytes"] == 3 * SEG
    p.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_densest_slabs(ctx, fmt):
    """The smallest records the formats allow, five segments of them: more record starts per segment than a workgroup has
    threads (the extract kernels' k += 256 loop), validity words published at every shift."""
    fmt = F[fmt]
    p = fmt.parser(ctx, 6 * SEG)
    for shift in (0, 1):
        recs = smalls(fmt, shift, 77) + [fmt.tiny(i) for i in range((5 * SEG + 1234) // fmt.min_size)]
        assert all(len(r) == fmt.min_size for r in recs[shift:])
        data = b"".join(recs)
        starts = np.cumsum([0] + [len(r) for r in recs[:-1]])
        per_seg = [np.count_nonzero(starts // SEG == s) for s in range(5)]
        assert min(per_seg) >= (1771 if fmt is Bam else 1872), per_seg
        res = check(fmt, p, data, MUST, f"shift {shift}")
        assert res["n_rows"] == len(recs)
        check(fmt, p, data[:-3], MUST, f"shift {shift}, cut")
    p.close()


# ---- records longer than a segment: the serial proof --------------------------------------------------------------------------
def long_record(fmt, i, total):
    return fmt.stretched(i, total)


@pytest.mark.parametrize("fmt", FMTS)
def test_records_longer_than_a_segment(ctx, fmt):
    fmt = F[fmt]
    p = fmt.parser(ctx, 12 * SEG)
    s = fmt.small_size
    # 90 000 and 300 000 bytes of REF (BAM: of optional fields) between small records
    recs = smalls(fmt, 20) + [long_record(fmt, 1, 90_000 + s)] + smalls(fmt, 30, 40) + [long_record(fmt, 2, 300_000 + s)] + smalls(fmt, 1500, 80)
    res = check(fmt, p, b"".join(recs), MUST, "90 000 and 300 000")
    assert res["n_rows"] == len(recs)
    for d in (-1, 0, 1):  # a long record that ends at a segment edge, one byte before it, one byte behind it
        head = smalls(fmt, 7, d + 5)
        at = sum(map(len, head))
        recs = head + [long_record(fmt, 3, 3 * SEG + d - at)] + smalls(fmt, 2500, 90)
        res = check(fmt, p, b"".join(recs), MUST, f"long record ends at 3 segments {d:+d}")
        assert res["n_rows"] == len(recs) and res["consumed_bytes"] == sum(map(len, recs))
    recs = smalls(fmt, 3) + [long_record(fmt, 4, 100_001), long_record(fmt, 5, 2 * SEG + 17)] + smalls(fmt, 1300, 9)
    check(fmt, p, b"".join(recs), MUST, "two long records back to back")
    recs = smalls(fmt, 1200) + [long_record(fmt, 6, 200_000)]
    data = b"".join(recs)
    res = check(fmt, p, data[:-70_000], MUST, "a long record, last and cut off")
    assert res["n_rows"] == 1200 and res["consumed_bytes"] == 1200 * s
    recs = [long_record(fmt, 7, 150_000)] + smalls(fmt, 1100, 3)
    res = check(fmt, p, b"".join(recs), MUST, "a long record first in the slab")
    assert res["n_rows"] == 1101
    res = check(fmt, p, b"".join(recs)[:140_000], MUST, "nothing but a cut-off long record")
    assert res["n_rows"] == 0 and res["consumed_bytes"] == 0
    p.close()


# ---- decoys: payloads that hold byte-exact copies of whole records ------------------------------------------------------------
def decoy_slab(fmt, k_decoys, where, via=0):
    """where: 'front' -- the copies lie in the tail of the record that spans the edge of segment 1, filler and then the true first
    start of the segment behind them; 'behind' -- in a record that starts behind the segment's true first start; 'landing' -- at
    the very end of the spanning record: their chain lands on the true first start; 'jumped' -- inside a segment that a long
    record covers from end to end; 'cut' -- one copy in a last record that the slab cuts off just behind the copy; 'last' -- one
    copy at the very end of the spanning record, in front of a small record that is the slab's last."""
    copies = b"".join(fmt.small(6000 + j) for j in range(k_decoys))
    tail = fmt.carrier_tail if via == 0 else None
    if where in ("landing", "last"):
        assert via == 0
        if tail:  # the carrier's own last byte(s) are the last byte(s) of the last copy
            assert copies[-tail:] == fmt.carrier(0, b"")[-tail:]
            copies = copies[:-tail]
    head = smalls(fmt, (SEG - 3000) // fmt.small_size, 10)
    at = sum(map(len, head))
    if where == "front":
        payload = FILL * (SEG + 200 - at - 80) + copies + FILL * 200
        recs = head + [fmt.carrier(1, payload, via)] + smalls(fmt, 2600, 50)
    elif where == "behind":
        recs = run_to(fmt, 0, SEG + 9, 10) + smalls(fmt, 5, 30) + [fmt.carrier(1, FILL * 300 + copies + FILL * 200, via)] + smalls(fmt, 2600, 50)
    elif where == "landing":
        recs = head + [fmt.carrier(1, FILL * (SEG + 100 - at - 80) + copies)] + smalls(fmt, 2600, 50)
    elif where == "jumped":
        recs = head + [fmt.carrier(1, FILL * (2 * SEG + 50 - at - 80) + copies + FILL * (SEG + 5000), via)] + smalls(fmt, 1500, 50)
    elif where == "cut":
        recs = head + [fmt.carrier(1, FILL * (SEG + 120 - at - 80) + copies + FILL * 5000, via)]
    elif where == "last":
        recs = head + [fmt.carrier(1, FILL * (SEG + 100 - at - 80) + copies), fmt.small(99)]
    data = b"".join(recs)
    c0 = data.index(copies[:fmt.min_size])  # the first copy (nothing in front of it holds these bytes: its ID / name is its own)
    if where == "cut":
        data = data[:c0 + len(copies) + 10]
    return data, c0


DECOYS = [  # (copies, where, payload kind, label)
    (1, "front", 0, MUST), (2, "front", 0, MUST), (1, "front", 1, MUST), (2, "front", 1, MUST),  # the guess wants three headers
    (3, "front", 0, MAY), (5, "front", 0, MAY),
    (3, "behind", 0, MUST), (5, "behind", 1, MUST),    # the smallest offset wins
    (3, "landing", 0, MAY),                            # ... and must never yield the copies as rows
    (3, "jumped", 0, MUST),                            # the proof ignores a segment that the chain jumps over
    (1, "cut", 0, MUST),                               # accepted with fewer than three records, in a segment behind the slab's end
    (1, "last", 0, MAY),
]


@pytest.mark.parametrize("fmt", FMTS)
def test_payloads_that_hold_copies_of_whole_records(ctx, tmp_path, fmt):
    fmt = F[fmt]
    assert len(DECOYS) == 12 and sum(label == MAY for _, _, _, label in DECOYS) <= 4
    p = fmt.parser(ctx, 8 * SEG)
    for k, where, via, label in DECOYS:
        what = f"{k} copies, {where}, payload kind {via}"
        data, c0 = decoy_slab(fmt, k, where, via)
        offs, consumed, _ = X.split(data, fmt.name)
        assert c0 not in offs and c0 // SEG >= 1, what  # the copies are payload: no record of the chain starts there
        first_of_seg = min([o for o in offs + [consumed] if o // SEG == c0 // SEG], default=None)
        if where in ("front", "landing", "last"):
            assert c0 < first_of_seg, what
        if where in ("landing", "last"):
            assert c0 + k * fmt.small_size == first_of_seg, what  # the copies' chain lands on the true start
        if where == "behind":
            assert first_of_seg < c0, what
        if where == "jumped":
            assert not any(o // SEG == c0 // SEG for o in offs), what
        if where == "cut":
            assert consumed // SEG < c0 // SEG and len(data) - (c0 + fmt.small_size) < 32, what
        check(fmt, p, data, label, what)
        if label == MAY:
            host = check_file(fmt, ctx, tmp_path, data, what)
            assert len(host) == len(offs), what
    p.close()


# ---- true records that the start guess cannot recognise ------------------------------------------------------------------------
def odd_records(fmt):
    if fmt is Bam:
        return {"ref >= n_ref": Bam.small(1, ref=N_REF), "pos < -1": Bam.small(2, pos=-2),
                "l_read_name = 0": Bam.small(3, name=b""), "a name without its NUL": Bam.small(4, name=b"r0004x"),
                "l_seq beyond block_size": Bam.small(5, l_seq=1_000_000), "mate reference out of range": Bam.small(6, mref=N_REF + 5)}
    return {"rlen < 0": Bcf.small(1, rlen=-1), "missing ID written as 0x00": Bcf.small(2, id_=b"\x00"),
            "n_allele = 0": Bcf.small(3, alleles=()), "a sample count that is not the header's": Bcf.small(4, n_sample=3, n_fmt=1, indiv=FILL * 12)}


@pytest.mark.parametrize("fmt", FMTS)
def test_true_records_that_no_start_guess_recognises(ctx, tmp_path, fmt):
    """The walk trusts the length field alone, so such a record inside a chain is a row like any other; as the first record of a
    segment it leaves the segment's guess on a later record, which the proof notices: the slab goes back to the host reader.
    (A BAM reference id beyond the header's was such a row too, and a dictionary index outside the dictionary in the host reader's
    batches: the first run of this test found that.  Both readers refuse it now.)"""
    fmt = F[fmt]
    p = fmt.parser(ctx, 6 * SEG)
    for what, rec in odd_records(fmt).items():
        refused = isinstance(fmt.row(rec), X.Reject)
        assert refused == (what == "ref >= n_ref"), what  # (that one has no name to be a row with: both readers refuse it, wherever it lies)
        first = b"".join(run_to(fmt, 0, SEG + 10, 20) + [rec] + smalls(fmt, 2500, 60))
        check(fmt, p, first, MAY, what + ", first of its segment")
        host = check_file(fmt, ctx, tmp_path, first, what)
        assert isinstance(host, Refused) if refused else len(host) == len(X.split(first, fmt.name)[0]), what
        inside = b"".join(run_to(fmt, 0, SEG + 10, 20) + smalls(fmt, 40, 7) + [rec] + smalls(fmt, 2500, 60))
        check(fmt, p, inside, MAY, what + ", inside its segment")
    p.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_lengths_the_walk_refuses(ctx, fmt):
    fmt = F[fmt]
    p = fmt.parser(ctx, 6 * SEG)
    bad = ([struct.pack("<I", 31), struct.pack("<I", (1 << 28) + 1)] if fmt is Bam else
           [struct.pack("<II", 23, 0), struct.pack("<II", (1 << 28) + 1, 0), struct.pack("<II", 40, (1 << 28) + 1)])
    for lens in bad:
        rec = fmt.small(5)
        data = b"".join(smalls(fmt, 1700) + [lens + rec[len(lens):]] + smalls(fmt, 1700, 9))
        rows, consumed, rej = statement(fmt, data)
        assert rej is not None and len(rows) == 1700
        res = check(fmt, p, data, MAY, lens.hex())
        assert res["n_undecided"] > 0
    p.close()


def test_bam_record_between_the_plausibility_cap_and_the_walks_cap(ctx, tmp_path):
    """block_size of 18 MB: above 2^24, beyond which no start guess believes a header, and below 2^28, up to which the walk
    follows a length.  First in its slab nobody has to guess it; in the middle of a file the host reader's rows come out."""
    big = Bam.stretched(1, 18_000_000)
    assert (1 << 24) < struct.unpack_from("<I", big, 0)[0] < (1 << 28)
    data = big + b"".join(smalls(Bam, 1500, 3))
    p = Bam.parser(ctx, len(data) + 4096)
    res = check(Bam, p, data, MUST, "first in its slab")
    assert res["n_rows"] == 1501
    p.close()
    host = check_file(Bam, ctx, tmp_path, b"".join(smalls(Bam, 1500, 8)) + data, "in the middle of a file")
    assert len(host) == 3001


# ---- the BCF typed walk ------------------------------------------------------------------------------------------------------
def test_bcf_typed_walk_table(ctx):
    """Every case of bcf_typed_walk_cases.py between good records in the middle of a segment.  DECIDED: a row equal to the
    statement's; REJECT and LIMIT: undecided -- among them the counts whose byte size wraps 32 bits (2^30 four-byte items: 0)."""
    p = Bcf.parser(ctx, 4 * SEG)
    head, tail = b"".join(smalls(Bcf, 1600, 1)), b"".join(smalls(Bcf, 1700, 5))
    for n, (name, rec, label) in enumerate(T.cases()):
        data = head + T.good(n + 1) + rec + T.good(n + 2) + tail
        row = Bcf.row(rec)
        assert isinstance(row, X.Reject) == (label != T.DECIDED), name  # the label, written down with the case, and the statement agree
        res = check(Bcf, p, data, MUST if label == T.DECIDED else MAY, name)
        assert (res["n_undecided"] == 0) == (label == T.DECIDED), name
    p.close()
