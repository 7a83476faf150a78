"""Plain Python / numpy statement of a VCF scan with a pushed-down value predicate (Scan(..., where=(column, op, literal))) for
tests/test_scan_predicate.py and tests/test_gpu_scan_predicate.py.  Uses neither the library nor oracle/: the lines are split here,
the FIRST matching INFO key decides, values go through np.float32 / int, and the comparison is made on explicit IEEE totalOrder
keys -- the f32 widened to f64, or the int itself as an f64 (every int32 is exact there), against the f64 literal's key.  NULL
(qual '.', INFO '.', key absent, value '.') never passes.

The files are made here too (line(), header()), with the strings the `info` column prints for them spelled out next to the
spellings that go into the file (AF_SPELLINGS): `info` is the parsed entries printed again, not a copy of field 8."""
import struct

import numpy as np

OPS = (">", ">=", "<", "<=", "=", "!=")
CONTIGS = ("1", "2")
COLS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
# (what the file says, what `info` prints for it)
AF_SPELLINGS = (("0.01", "0.01"), ("0.5", "0.5"), ("0.25", "0.25"), ("1e-3", "0.001"), ("0.010", "0.01"), ("0.75", "0.75"), ("2", "2"))
FILTERS = (".", "PASS", "q10;s50", "q10")
INFO_FIELD = "AF,DP,DB,XS"  # Float, Integer, Flag, String: scan columns 4, 5, 6, 7
COLUMN = {"qual": 2, "AF": 4, "DP": 5}


def header(pad=None):
    h = "##fileformat=VCFv4.2\n" + "".join(f"##contig=<ID={c}>\n" for c in CONTIGS)
    if pad is not None:  # moves the data lines by as many bytes
        h += "##pad=" + "x" * pad + "\n"
    h += '##INFO=<ID=AF,Number=1,Type=Float,Description="f">\n##INFO=<ID=DP,Number=1,Type=Integer,Description="i">\n'
    h += '##INFO=<ID=DB,Number=0,Type=Flag,Description="b">\n##INFO=<ID=XS,Number=1,Type=String,Description="s">\n'
    h += '##INFO=<ID=XF,Number=1,Type=Float,Description="f">\n##INFO=<ID=AL,Number=A,Type=Float,Description="list">\n'
    h += '##FILTER=<ID=q10,Description="q">\n##FILTER=<ID=s50,Description="s">\n'
    return h + COLS


def line(i, qual, chrom="1", pos0=True, info=None):
    """data line i (no terminator) and what its `info` column prints.  Varied by i: id NULL / one item / three items, alt NULL or
    not (an empty list then), POS 0 (NULL) on some rows, every typed key absent on some rows, info 0 .. ~70 bytes."""
    rid = (".", f"rs{i}", f"a{i};b{i};c{i}")[i % 3]
    alt = (".", "C", "C,T")[(i // 3) % 3]
    pos = 0 if pos0 and i % 17 == 5 else i + 1
    want = None
    if info is None:
        raw, printed = [], []
        if i % 5:
            a, b = AF_SPELLINGS[i % len(AF_SPELLINGS)]
            raw.append("AF=" + a)
            printed.append("AF=" + b)
        if i % 7:
            dp = str((i * 37) % 100000)
            raw.append("DP=" + dp)
            printed.append("DP=" + dp)
        if i % 3 == 0:
            raw.append("DB")
            printed.append("DB=true")
        if i % 4:
            xs = "s" + "x" * (i % 41)
            raw.append("XS=" + xs)
            printed.append("XS=" + xs)
        info, want = (";".join(raw), ";".join(printed)) if raw else (".", "")
    return f"{chrom}\t{pos}\t{rid}\tA{'C' * (i % 4)}\t{alt}\t{qual}\t{FILTERS[i % 4]}\t{info}", want


# ---- the operator / literal / NULL table -------------------------------------------------------------------------------------------
# every row's operand spelling by column; NULL forms: qual '.', INFO '.', key absent, `=.`; a repeated key is decided by its FIRST piece
QUALS = [".", "0.01", "0.5", "-0.0", "0", "nan", "30", "29.999", "16777217", "1e10", "-5", "0.010", "inf", "-inf"]
AF_INFOS = ["AF=0.01", "AF=.", "DP=3", ".", "AF=nan", "AF=-0.0", "AF=0", "AF=0.5;AF=0.001", "AF=0.001;AF=0.5", "DP=1;AF=30", "AF=16777217", "AF=-5;DB", "XS=AF;AF=0.010"]
DP_INFOS = ["DP=16777217", "DP=16777216", "DP=16777218", "DP=0", "DP=-3", "DP=.", "AF=0.5", ".", "DP=5;DP=50", "DP=50;DP=5", "DB;DP=2147483647", "DP=-2147483648", "XS=DP;DP=1"]
LITERALS = {"qual": [0.01, -0.0, float("nan"), 30.0, 16777216.0], "AF": [0.01, -0.0, float("nan"), 0.5], "DP": [16777217.0, -0.0, 0.5, 5.0, float("nan")]}


def table_lines(what, spelled_out=True):
    """the table's data lines for the column `what`; spelled_out=False: without the nan / inf spellings (the device parsers hand
    those to the host reader)"""
    words = ("nan", "inf")
    if what == "qual":
        return [line(i, q, pos0=False, info="DP=7")[0] for i, q in enumerate(QUALS) if spelled_out or not any(w in q for w in words)]
    return [line(i, "50", pos0=False, info=x)[0] for i, x in enumerate(AF_INFOS if what == "AF" else DP_INFOS) if spelled_out or not any(w in x for w in words)]


def info_value(info, key):
    """the value text of the FIRST piece whose key is `key`; None: INFO '.', key absent, a bare key, a value of '.' or none.
    A Flag: True when present."""
    if info == "." or info == "":
        return None
    for piece in info.split(";"):
        k, eq, v = piece.partition("=")
        if k == key:
            if not eq:
                return True  # bare: a Flag that is there (a valued key's bare form is NULL: callers ask `is True`)
            return None if v in ("", ".") else v
    return None


def f64_key(x):
    """IEEE totalOrder key of a float64"""
    b = struct.unpack("<q", struct.pack("<d", float(x)))[0]
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)


def passes(value, op, literal):
    """value: None (NULL), an np.float32 or an int; the predicate as FilterExec sees it, in totalOrder"""
    if value is None:
        return False
    a = f64_key(np.float64(value)) if isinstance(value, np.float32) else f64_key(float(int(value)))
    b = f64_key(literal)
    return {">": a > b, ">=": a >= b, "<": a < b, "<=": a <= b, "=": a == b, "!=": a != b}[op]


def typed(fields, what):
    """the predicate's operand of one split line: `what` is "qual" or an INFO key; Float -> np.float32, Integer -> int"""
    if what == "qual":
        return None if fields[5] == "." else np.float32(fields[5])
    v = info_value(fields[7], what)
    if v is None or v is True:
        return None
    return int(v) if what == "DP" else np.float32(v)


def keep(text_lines, what, op, literal, region=None):
    """indexes of the lines the scan emits; region: (contig, first, last), the point form (POS inside, POS 0 never)"""
    out = []
    for i, ln in enumerate(text_lines):
        f = ln.split("\t")
        if region is not None and not (f[0] == region[0] and int(f[1]) >= 1 and region[1] <= int(f[1]) <= region[2]):
            continue
        if passes(typed(f, what), op, literal):
            out.append(i)
    return out


def columns(text_lines, wants, rows, project=("id", "ref", "alt", "info")):
    """the batches' columns (as lists, pyarrow's to_pylist forms) of the lines `rows`; wants[i]: what line i's `info` prints"""
    c = {k: [] for k in ("chrom", "pos", "qual", "filter", "info.AF", "info.DP", "info.DB", "info.XS") + tuple(project)}
    for i in rows:
        f = text_lines[i].split("\t")
        c["chrom"].append(f[0])
        c["pos"].append(int(f[1]) if int(f[1]) > 0 else None)
        c["qual"].append(None if f[5] == "." else float(np.float32(f[5])))
        c["filter"].append("" if f[6] == "." else f[6])
        af, dp, xs = info_value(f[7], "AF"), info_value(f[7], "DP"), info_value(f[7], "XS")
        c["info.AF"].append(None if af in (None, True) else float(np.float32(af)))
        c["info.DP"].append(None if dp in (None, True) else int(dp))
        c["info.DB"].append(True if info_value(f[7], "DB") is not None else None)
        c["info.XS"].append(None if xs in (None, True) else xs)
        if "id" in project:
            c["id"].append(None if f[2] == "." else f[2].split(";"))
        if "ref" in project:
            c["ref"].append(f[3])
        if "alt" in project:
            c["alt"].append(None if f[4] == "." else [])  # the reference appends the list without its values
        if "info" in project:
            c["info"].append(wants[i])
    return c


def same(a, b):
    """two column dicts, NaN equal to NaN"""
    if a.keys() != b.keys():
        return False
    for k in a:
        if len(a[k]) != len(b[k]):
            return False
        for x, y in zip(a[k], b[k]):
            if isinstance(x, float) and isinstance(y, float) and x != x and y != y:
                continue
            if x != y:
                return False
    return True


def table(scan):
    """every batch of a Scan -> (columns as lists, the batches' lengths)"""
    cols, lens = {}, []
    for b in scan:
        lens.append(len(b))
        for i in range(b.type.num_fields):
            cols.setdefault(b.type.field(i).name, []).extend(b.field(i).to_pylist())
    return cols, lens


def empty(project=("id", "ref", "alt", "info")):
    return columns([], [], [], project)
