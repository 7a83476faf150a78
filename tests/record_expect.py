"""Test infrastructure: what a slab of BAM or BCF records must split and decode to, restated in plain Python, and raw record
builders that take every field as a parameter.

Written from the formats (SAM specification 4.2, VCF 4.x specification 6) and from the rules the header comments of
exon_amd/csrc/bam_parse.hip, bcf_parse.hip and host/bcf.h state -- not from the C++, and without the device's rule for
guessing a record start: records are found by walking the chain of length fields from byte 0, nothing else.  All arithmetic
is in unbounded Python integers, so nothing here can wrap.  Not product code: only tests import it.

Lengths the product refuses (the chain cannot be followed): BAM block_size < 32 or > 2^28; BCF l_shared < 24 or > 2^28,
l_indiv > 2^28.

A BAM row (the device layout: flag, mapping_quality, reference, start, end) needs the fixed fields and the CIGAR; a CIGAR that
does not fit in block_size is refused, and so is a reference id beyond the header's (it has no name).  Nothing else of the
record is looked at: a read name without its NUL, an l_seq the record cannot hold, a reference below -1 (NULL like -1), a mate
reference beyond the header's are decoded as they stand.

A BCF row (chrom, pos, qual, FILTER index list, watched INFO keys) walks the typed values of the shared block: ID, n_allele
alleles, FILTER, n_info (key, value) pairs.  A typed value is a descriptor byte (type in the low nibble: 0 missing, 1 / 2 / 3
int8 / int16 / int32, 5 float, 7 character; count in the high nibble), 15 meaning that the count follows as a typed integer:
one more descriptor byte, of which the type alone counts and must be 1, 2 or 3, and the integer.  Refused: any byte needed at
or past l_shared, a negative count, a FILTER entry that is no integer or lies outside the header's strings, a CHROM outside
the contigs and -- a limit of the device layout, not of the format -- more than 8 FILTER entries.
"""
import struct
import zlib

import numpy as np

import vcf_bcf_writer as W

FILL = 0x21  # filler of payloads: as a length field 0x21212121, beyond every length the product follows
MAX_LEN = 1 << 28
FLOAT_MISSING, FLOAT_EOV = 0x7F800001, 0x7F800002
INT_MISSING = {1: -128, 2: -32768, 3: -(1 << 31)}
TYPE_SIZE = {1: 1, 2: 2, 3: 4, 5: 4, 7: 1}


class Reject:
    """why a record, or a length field, is refused"""

    def __init__(self, reason, device_limit=False):
        self.reason, self.device_limit = reason, device_limit

    def __repr__(self):
        return f"Reject({self.reason!r})"


def _i32(b, o):
    return struct.unpack_from("<i", b, o)[0]


def _u32(b, o):
    return struct.unpack_from("<I", b, o)[0]


# ---- the chain ------------------------------------------------------------------------------------------------------------
def record_bytes(data, o, fmt):
    """total size of the record whose length field starts at o (the field lies inside data), or a Reject"""
    if fmt == "bam":
        bs = _u32(data, o)
        if bs < 32 or bs > MAX_LEN:
            return Reject(f"block_size {bs}")
        return 4 + bs
    ls, li = _u32(data, o), _u32(data, o + 4)
    if ls < 24 or ls > MAX_LEN or li > MAX_LEN:
        return Reject(f"l_shared {ls}, l_indiv {li}")
    return 8 + ls + li


def split(data, fmt):
    """-> (offsets of the records that lie wholly inside data, consumed, reject): consumed = where the first record that the slab
    cuts off starts (len(data) when the chain lands on the end; a cut inside the length field counts), reject = a Reject when
    the chain met a length the product refuses (consumed is then where that record starts), else None."""
    n, o, offs = len(data), 0, []
    len_bytes = 4 if fmt == "bam" else 8
    while o + len_bytes <= n:
        size = record_bytes(data, o, fmt)
        if isinstance(size, Reject):
            return offs, o, size
        if o + size > n:
            break
        offs.append(o)
        o += size
    return offs, o, None


def records(data, fmt):
    """the whole records of data, as bytes"""
    offs, consumed, _ = split(data, fmt)
    return [data[a:b] for a, b in zip(offs, offs[1:] + [consumed])]


# ---- rows -----------------------------------------------------------------------------------------------------------------
REF_CONSUMING = (0, 2, 3, 7, 8)  # M D N = X


def bam_row(rec, n_ref):
    """rec: one record, block_size field included -> dict(flag, mapq, ref, start, end), None = NULL; or a Reject"""
    bs = _u32(rec, 0)
    assert 4 + bs == len(rec) and bs >= 32
    ref, pos = _i32(rec, 4), _i32(rec, 8)
    l_name, mapq = rec[12], rec[13]
    n_cigar, flag = struct.unpack_from("<HH", rec, 16)
    co = 32 + l_name
    if ref >= n_ref:
        return Reject(f"reference {ref} of {n_ref}")
    if co + 4 * n_cigar > bs:
        return Reject("CIGAR beyond block_size")
    span = 0
    for k in range(n_cigar):
        op = _u32(rec, 4 + co + 4 * k)
        if op & 0xF in REF_CONSUMING:
            span += op >> 4
    return dict(flag=flag, mapq=None if mapq == 255 else mapq, ref=None if ref < 0 else ref,
                start=pos + 1 if pos >= 0 else None, end=pos + span if pos >= 0 else None)


class _Cursor:
    def __init__(self, rec, o, end):
        self.rec, self.o, self.end = rec, o, end

    def need(self, k, what):
        if self.o + k > self.end:
            raise _Refused(f"{what} beyond l_shared")

    def byte(self, what):
        self.need(1, what)
        self.o += 1
        return self.rec[self.o - 1]

    def int(self, t, what):
        if t not in (1, 2, 3):
            raise _Refused(f"{what}: type {t} is no integer")
        self.need(TYPE_SIZE[t], what)
        v = int.from_bytes(self.rec[self.o:self.o + TYPE_SIZE[t]], "little", signed=True)
        self.o += TYPE_SIZE[t]
        return v

    def header(self, what):
        d = self.byte(what + " descriptor")
        t, c = d & 0xF, d >> 4
        if c == 15:
            ct = self.byte(what + " count descriptor") & 0xF
            c = self.int(ct, what + " count")
            if c < 0:
                raise _Refused(f"{what}: negative count {c}")
        return t, c

    def skip(self, t, c, what):
        self.need(c * TYPE_SIZE.get(t, 0), what)
        self.o += c * TYPE_SIZE.get(t, 0)


class _Refused(Exception):
    pass


def f32_bits_of_int(v):
    return int(np.float32(v).view(np.uint32))


def bcf_row(rec, n_contigs, n_strings, keys, max_filters=8):
    """rec: one record, l_shared / l_indiv included; keys: [(header-string index, kind)], kind 'f' Float, 'i' Integer, 'b' Flag,
    'F' / 'I' lists.  -> dict(chrom, pos, qual, filter, info): pos None when pos0 < 0, qual the float's bit pattern or None,
    filter a tuple of string indexes, info one entry per key: 'f' float bits, 'i' int, 'b' True, lists of float bits / ints with
    None items, None = NULL.  Or a Reject.  max_filters=None lifts the device layout's limit (the host reader has none)."""
    ls = _u32(rec, 0)
    assert ls >= 24 and 8 + ls <= len(rec)
    chrom, pos0 = _i32(rec, 8), _i32(rec, 12)
    qbits, nia = _u32(rec, 20), _u32(rec, 24)
    n_info, n_allele = nia & 0xFFFF, nia >> 16
    c = _Cursor(rec, 32, 8 + ls)
    try:
        c.skip(*c.header("ID"), "ID")
        for a in range(n_allele):
            c.skip(*c.header(f"allele {a}"), f"allele {a}")
        ft, fc = c.header("FILTER")
        if max_filters is not None and fc > max_filters:
            return Reject(f"{fc} FILTER entries", device_limit=True)
        filt = []
        for i in range(fc):
            v = c.int(ft, "FILTER entry")
            if v < 0 or v >= n_strings:
                return Reject(f"FILTER index {v}")
            filt.append(v)
        info = [None] * len(keys)
        have = [False] * len(keys)
        for q in range(n_info):
            kt, kc = c.header("INFO key")
            key = c.int(kt, "INFO key") if kc else -1
            vt, vc = c.header("INFO value")
            c.need(vc * TYPE_SIZE.get(vt, 0), "INFO value")
            o = c.o

            def item(e):
                if vt == 5:
                    return _u32(rec, o + 4 * e)
                return int.from_bytes(rec[o + TYPE_SIZE[vt] * e:o + TYPE_SIZE[vt] * (e + 1)], "little", signed=True)

            for w, (k, kind) in enumerate(keys):
                if k != key or have[w]:
                    continue  # the first occurrence of a key wins
                ints = vt in (1, 2, 3)
                missing, eov = (FLOAT_MISSING, FLOAT_EOV) if vt == 5 else (INT_MISSING.get(vt), INT_MISSING.get(vt, 0) + 1)
                if kind == "b":
                    info[w], have[w] = True, True
                elif kind in "fi":
                    if vc >= 1 and (ints or (vt == 5 and kind == "f")) and item(0) not in (missing, eov):
                        info[w] = item(0) if kind == "i" or vt == 5 else f32_bits_of_int(item(0))
                        have[w] = True
                elif vc >= 1 and (ints or (vt == 5 and kind == "F")):
                    items = []
                    for e in range(vc):
                        v = item(e)
                        if v == eov:
                            break
                        items.append(None if v == missing else v if kind == "I" or vt == 5 else f32_bits_of_int(v))
                    if items and items != [None]:  # one missing item is `key=.`: the whole value is missing
                        info[w], have[w] = items, True
            c.o = o + vc * TYPE_SIZE.get(vt, 0)
    except _Refused as e:
        return Reject(str(e))
    if chrom < 0 or chrom >= n_contigs:
        return Reject(f"CHROM {chrom}")
    return dict(chrom=chrom, pos=pos0 + 1 if pos0 >= 0 else None, qual=None if qbits == FLOAT_MISSING else qbits,
                filter=tuple(filt), info=info)


# ---- raw record builders: every field is a parameter, nothing is validated --------------------------------------------------
def bam_record(ref=1, pos=1 << 25, name=b"r\0", mapq=30, bin_=4680, cigar=(), flag=0, seq=b"", qual=b"", mref=-1, mpos=-1,
               tlen=0, aux=b"", l_read_name=None, n_cigar=None, l_seq=None, block_size=None):
    """cigar: raw 32-bit ops (length << 4 | code); seq / qual / aux: raw bytes; l_read_name, n_cigar, l_seq (default: the number
    of quality bytes) and block_size say what the fields hold when they should differ from what is written"""
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) if l_read_name is None else l_read_name, mapq, bin_,
                       len(cigar) if n_cigar is None else n_cigar, flag, len(qual) if l_seq is None else l_seq, mref, mpos, tlen)
    body += name + b"".join(struct.pack("<I", c) for c in cigar) + seq + qual + aux
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def bcf_record(chrom=0, pos0=0, rlen=1, qual_bits=FLOAT_MISSING, id_=b"\x07", alleles=(b"\x17A",), filter_=b"\x00", info=(),
               n_info=None, n_allele=None, n_fmt=0, n_sample=0, indiv=b"", tail=b"", l_shared=None, l_indiv=None):
    """id_, alleles, filter_: typed values as raw bytes (typed / typed_ints / typed_str below); info: (key bytes, value bytes)
    pairs; tail: bytes of the shared block behind the last pair; n_info, n_allele, l_shared, l_indiv as with bam_record"""
    shared = struct.pack("<iiiIII", chrom, pos0, rlen, qual_bits,
                         (len(info) if n_info is None else n_info) | ((len(alleles) if n_allele is None else n_allele) << 16),
                         (n_fmt << 24) | n_sample)
    shared += id_ + b"".join(alleles) + filter_ + b"".join(k + v for k, v in info) + tail
    return struct.pack("<II", len(shared) if l_shared is None else l_shared, len(indiv) if l_indiv is None else l_indiv) + shared + indiv


def typed(count, t, payload=b"", count_width=None, count_bytes=None):
    """a typed value: the descriptor of `count` items of type t (vcf_bcf_writer._desc and its knobs) and whatever payload is given"""
    return W._desc(count, t, count_width, count_bytes) + payload


def typed_str(s, count_width=None):
    return typed(len(s), 7, s, count_width)


def typed_ints(vals, width=None, pad=0, count_width=None):
    return W._typed_ints(vals, width, pad, count_width)


def typed_floats(bits, count_width=None):
    return typed(len(bits), 5, b"".join(struct.pack("<I", b) for b in bits), count_width)


# ---- files ----------------------------------------------------------------------------------------------------------------
def bgzf(data, block=0xFF00):
    out = []
    for i in list(range(0, len(data), block)) + [None]:  # a trailing empty block: the EOF marker
        chunk = b"" if i is None else data[i:i + block]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = c.compress(chunk) + c.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(comp) + 25) + comp +
                   struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out)


def bam_file(body, n_ref):
    text = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:c%d\tLN:%d\n" % (i, 1 << 29) for i in range(n_ref))
    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_ref)
    for i in range(n_ref):
        name = b"c%d\0" % i
        head += struct.pack("<i", len(name)) + name + struct.pack("<i", 1 << 29)
    return bgzf(head + body)


def bcf_file(body, filters=()):
    text = W.header_text(True, list(filters)).encode() + b"\0"
    return bgzf(b"BCF\x02\x02" + struct.pack("<I", len(text)) + text + body)


def f32(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def bcf_scan_row(row, contigs, strings, keys, names):
    """a bcf_row as exon_amd.Scan(..., info_field=names) prints it (to_pylist): names and floats in place of indexes and bits"""
    out = {"chrom": contigs[row["chrom"]], "pos": row["pos"], "qual": None if row["qual"] is None else f32(row["qual"]),
           "filter": ";".join(strings[i] for i in row["filter"])}
    for (_, kind), name, v in zip(keys, names, row["info"]):
        if v is not None and kind == "f":
            v = f32(v)
        elif v is not None and kind == "F":
            v = [None if e is None else f32(e) for e in v]
        out["info." + name] = v
    return out
