"""Test-side writer of a VCF text file and its BCF 2.2 twin with typed INFO fields of every kind the reference builds
(exon-core/src/datasources/vcf/schema_builder.rs:197-249): Float / Integer scalars, a Flag, a String scalar, and lists
(Number=A Integer, Number=. Float, Number=. String).  Independent of the product's decoders and of the oracle: rows are
python dicts, the BCF side encodes typed values the way htslib does (smallest integer type that holds every item)."""
import functools
import struct
import subprocess

import numpy as np

INFO_HEADER = [("AF", "1", "Float"), ("DP", "1", "Integer"), ("DB", "0", "Flag"), ("CSQ", "1", "String"),
               ("AC", "A", "Integer"), ("MQS", ".", "Float"), ("TAGS", ".", "String")]
FILTERS = ["q10", "s50"]


def header_text(bcf, filters=FILTERS):
    """filters: the FILTER IDs the header declares besides PASS (IDX 1 .. in BCF)"""
    idx = 0
    lines = ["##fileformat=VCFv4.3", '##FILTER=<ID=PASS,Description="All filters passed"' + (",IDX=0>" if bcf else ">"),
             "##contig=<ID=1" + (",IDX=0>" if bcf else ">"), "##contig=<ID=2" + (",IDX=1>" if bcf else ">")]
    for f in filters:
        idx += 1
        lines.append(f'##FILTER=<ID={f},Description="x"' + (f",IDX={idx}>" if bcf else ">"))
    for name, number, typ in INFO_HEADER:
        idx += 1
        lines.append(f'##INFO=<ID={name},Number={number},Type={typ},Description="x"' + (f",IDX={idx}>" if bcf else ">"))
    lines.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO")
    return "\n".join(lines) + "\n"


def string_index(filters=FILTERS):
    names = ["PASS"] + list(filters) + [n for n, _, _ in INFO_HEADER]
    return {n: i for i, n in enumerate(names)}


def make_rows(n, seed=7):
    """rows: dict(chrom, pos, qual (float | None), filter (list[str]), info (dict | None)).  info values: float, int, True,
    str, or lists with None items; a key mapped to None means `key=.`.  Optional keys (row_id_ref_alt): id (the ID field's text,
    "" = an empty field), ref (text), alt (list of alleles; None or [] = none: '.' in VCF, REF alone in BCF; BCF alleles may be
    empty strings), alleles (BCF only: every allele, REF first; [] = n_allele 0)"""
    rng = np.random.default_rng(seed)
    edge_dp = [16777215, 16777216, 16777217, 16777218, 16777219, 2**31 - 1, -(2**31) + 8, -5, 0, 127, 128, -120, 32767, 32768, 100000]
    rows = []
    for i in range(n):
        info = {}
        if rng.random() < 0.9:
            info["AF"] = float(np.float32(rng.choice([0.001, 0.01, 0.0100000001, 0.25, 0.5, 1e-5, 3.0e-2])))
        if rng.random() < 0.85:
            info["DP"] = int(edge_dp[i % len(edge_dp)]) if rng.random() < 0.5 else int(rng.integers(0, 200))
        elif rng.random() < 0.3:
            info["DP"] = None  # DP=.
        if rng.random() < 0.3:
            info["DB"] = True
        if rng.random() < 0.4:
            info["CSQ"] = str(rng.choice(["missense", "stop", "syn"]))
        if rng.random() < 0.6:
            k = int(rng.integers(1, 4))
            info["AC"] = [None if rng.random() < 0.15 else int(rng.choice([1, 2, 300, 70000, -3])) for _ in range(k)]
        if rng.random() < 0.4:
            k = int(rng.integers(1, 5))
            info["MQS"] = [None if rng.random() < 0.1 else float(np.float32(rng.choice([60.0, 37.5, 0.125, 1e-3]))) for _ in range(k)]
        if rng.random() < 0.3:
            k = int(rng.integers(1, 3))
            info["TAGS"] = [None if rng.random() < 0.1 else str(rng.choice(["a", "bb", "ccc"])) for _ in range(k)]
        for k in ("AC", "MQS", "TAGS"):  # a one-item list whose item is missing IS `key=.`: the whole value is missing (NULL list)
            if info.get(k) == [None]:
                info[k] = None
        filt = [[], ["PASS"], ["q10"], ["q10", "s50"], ["s50"]][int(rng.integers(0, 5))]
        qual = None if rng.random() < 0.05 else float(np.float32(int(rng.integers(0, 10000)) / 10))
        rows.append(dict(chrom=str(1 + (i >= n // 2)), pos=i + 1, qual=qual, filter=filt, info=(info if info and rng.random() < 0.97 else None)))
    return rows


def _info_text(info):
    if info is None:
        return "."
    parts = []
    for k, v in info.items():
        if v is True:
            parts.append(k)
        elif v is None:
            parts.append(f"{k}=.")
        elif isinstance(v, list):
            parts.append(k + "=" + ",".join("." if e is None else (np.format_float_positional(np.float32(e), unique=True, trim="0")
                                                                    if isinstance(e, float) else str(e)) for e in v))
        elif isinstance(v, float):
            parts.append(f"{k}={np.format_float_positional(np.float32(v), unique=True, trim='0')}")
        else:
            parts.append(f"{k}={v}")
    return ";".join(parts)


def row_id_ref_alt(r):
    """(id text, ref, alt alleles) of a row: today's '.', 'A', ['C'] unless the row says otherwise"""
    alt = r.get("alt", ["C"])
    return r.get("id", "."), r.get("ref", "A"), [] if alt is None else list(alt)


def write_vcf(path, rows, filters=FILTERS, eol=lambda i: "\n"):
    """eol(i): the line end of row i ("\r\n"; "" for a last line without LF)"""
    with open(path, "w", newline="") as f:
        f.write(header_text(False, filters))
        for i, r in enumerate(rows):
            q = "." if r["qual"] is None else np.format_float_positional(np.float32(r["qual"]), unique=True, trim="0")
            rid, ref, alt = row_id_ref_alt(r)
            f.write(f"{r['chrom']}\t{r['pos']}\t{rid}\t{ref}\t{','.join(alt) or '.'}\t{q}\t{';'.join(r['filter']) or '.'}\t{_info_text(r['info'])}{eol(i)}")


INT_TYPES = {1: ("b", -128), 2: ("h", -32768), 3: ("i", -2147483648)}  # BCF type code -> (struct format, 'missing'; + 1 = end of vector)
FLOAT_MISSING, FLOAT_EOV = 0x7F800001, 0x7F800002


class Ints:
    """Opt-in control over how an INFO value is written to BCF (write_bcf only): an integer vector -- under an Integer key or, as
    htslib never does but the format allows, a Float key -- in a forced width (1 / 2 / 3 = int8 / int16 / int32; None: the
    narrowest), followed by `pad` end-of-vector values (they count in the vector's length), its length written as an extended
    count in the integer width `count_width` (None: inline below 15 items).  vals: int, or None = the width's missing value."""

    def __init__(self, vals, width=None, pad=0, count_width=None):
        self.vals, self.width, self.pad, self.count_width = list(vals), width, pad, count_width

    def encode(self):
        return _typed_ints(self.vals, self.width, self.pad, self.count_width)


class Floats:
    """... a float vector given as raw bit patterns (None = missing, 0x7F800001), `pad` end-of-vector values behind it"""

    def __init__(self, bits, pad=0, count_width=None):
        self.bits, self.pad, self.count_width = list(bits), pad, count_width

    def encode(self):
        words = [FLOAT_MISSING if b is None else b for b in self.bits] + [FLOAT_EOV] * self.pad
        return _desc(len(words), 5, self.count_width) + b"".join(struct.pack("<I", w) for w in words)


def _typed_ints(vals, width=None, pad=0, count_width=None):
    """typed integer vector (None = missing) in the smallest type that holds every item (reserving the 8 lowest values), or in
    the forced `width`; `pad` end-of-vector values behind the items"""
    present = [v for v in vals if v is not None]
    lo, hi = (min(present), max(present)) if present else (0, 0)
    if width is not None:
        t = width
    elif -120 <= lo and hi <= 127:
        t = 1
    elif -32760 <= lo and hi <= 32767:
        t = 2
    else:
        t = 3
    fmt, miss = INT_TYPES[t]
    return _desc(len(vals) + pad, t, count_width) + b"".join(struct.pack("<" + fmt, miss if v is None else v) for v in vals) + struct.pack("<" + fmt, miss + 1) * pad


def _desc(n, t, count_width=None, count_bytes=None):
    """descriptor byte(s) of a typed vector of n items of type t.  Opt-in: `count_width` forces the extended form with the count
    in that integer width (n may then be anything the width holds, negative included); `count_bytes` are written behind the
    0xF? byte as they are, in place of the typed count (a count whose own descriptor is no integer's, a cut-off count)."""
    if count_bytes is not None:
        return bytes([0xF0 | t]) + count_bytes
    if 0 <= n < 15 and count_width is None:
        return bytes([(n << 4) | t])
    return bytes([0xF0 | t]) + _typed_ints([n], count_width)


def _typed_floats(vals):
    return _desc(len(vals), 5) + b"".join(struct.pack("<I", 0x7F800001) if v is None else struct.pack("<f", np.float32(v)) for v in vals)


@functools.lru_cache(maxsize=4096)
def _typed_str(s):
    b = s.encode()
    return _desc(len(b), 7) + b


def write_bcf(path, rows, bgzip, filters=FILTERS):
    """uncompressed BCF stream -> `bgzip` (tools/bin/bgzip) -> path; a row's FILTER IDs are PASS or among `filters`.
    Opt-in row keys: "qual_bits" (QUAL as a raw bit pattern), "pos0" (the 0-based POS field as it is), "key_width" (the integer
    width of every INFO key index of the row); an INFO value may be an `Ints` or a `Floats`."""
    sidx = string_index(filters)
    types = {n: (num, typ) for n, num, typ in INFO_HEADER}
    text = header_text(True, filters).encode() + b"\0"
    out = [b"BCF\x02\x02", struct.pack("<I", len(text)), text]
    for r in rows:
        info = r["info"] or {}
        rid, ref, alt = row_id_ref_alt(r)
        alleles = r["alleles"] if "alleles" in r else [ref] + alt
        qbits = r["qual_bits"] if "qual_bits" in r else (0x7F800001 if r["qual"] is None else struct.unpack("<I", struct.pack("<f", np.float32(r["qual"])))[0])
        shared = struct.pack("<iiiIII", int(r["chrom"]) - 1, r["pos0"] if "pos0" in r else r["pos"] - 1, 1, qbits, len(info) | (len(alleles) << 16), 0)
        shared += (_typed_str(r["id"]) if "id" in r else b"\x07") + b"".join(_typed_str(a) for a in alleles)
        shared += _typed_ints([sidx[f] for f in r["filter"]]) if r["filter"] else b"\x00"
        for k, v in info.items():
            shared += _typed_ints([sidx[k]], r.get("key_width"))
            num, typ = types[k]
            if isinstance(v, (Ints, Floats)):
                shared += v.encode()
            elif typ == "Flag":
                shared += b"\x00"
            elif v is None:
                shared += (_typed_floats([None]) if typ == "Float" else _typed_ints([None]) if typ == "Integer" else _typed_str("."))
            elif typ == "Integer":
                shared += _typed_ints(v if isinstance(v, list) else [v])
            elif typ == "Float":
                shared += _typed_floats(v if isinstance(v, list) else [v])
            else:
                shared += _typed_str(",".join("." if e is None else e for e in v) if isinstance(v, list) else v)
        out.append(struct.pack("<II", len(shared), 0) + shared)
    raw = str(path) + ".u"
    with open(raw, "wb") as f:
        f.write(b"".join(out))
    subprocess.check_call([bgzip, raw, str(path), "6"])


def expected_column(rows, key):
    """what info.<key> must decode to (python values; floats f32-rounded), straight from the rows"""
    num, typ = {n: (a, b) for n, a, b in INFO_HEADER}[key]
    out = []
    for r in rows:
        v = None if r["info"] is None else r["info"].get(key)
        if typ == "Flag":
            out.append(True if v else None)
        elif isinstance(v, list):
            out.append([None if e is None else (float(np.float32(e)) if typ == "Float" else e) for e in v])
        elif isinstance(v, float):
            out.append(float(np.float32(v)))
        else:
            out.append(v)
    return out
