"""Test infrastructure: what a GTF scan must return, restated in plain Python.

Written from the rules (exon_amd/csrc/host/gtf.h's header comment), not from the C++.
Lines: a line ends at '\\n', one '\\r' in front of it dropped; a last line without '\\n' is read whole; a line starting with '#' is
no row (no ##FASTA case); an empty line is an error; every other line is a record of eight TAB-separated fields and a ninth that
is whatever follows the eighth TAB; fewer than eight TABs is an error.
Fields: start / end decimal, one leading '+', >= 1 (up to 18 digits here); score '.' or Rust's f32::from_str; strand + - or '.'
(NULL), '?' is an error; frame '.' (NULL) or 0 1 2.
Attributes: "" is no entry; else a run of entries `key`, spaces, `value`, optional spaces, then ';' or the end.  Spaces in front
of a key are skipped and a trailing ';' (and spaces) ends the field.  The key runs to the first space and is not empty.  A value
that starts with '"' runs to the next '"' (quotes dropped, no escapes, ';' and spaces inside are the value's); any other value
runs to the next ';' or the end, trailing spaces dropped.  Errors: a missing closing quote, a key with no value, an empty piece,
bytes other than spaces behind a closing quote.  Duplicate keys stay, nothing is percent-decoded, keys and values are UTF-8.
The float parser, the line splitter and the region filter are gff_expect's (test code too).  Not product code: only tests import it.
"""
import numpy as np

import gff_expect
from gff_expect import OPEN_END, f32_from_str, hit, lines_of, parse_region  # noqa: F401

STRANDS = ["+", "-"]
FRAMES = ["0", "1", "2"]


class GtfError(ValueError):
    pass


def _position(x):
    m = gff_expect._POS.match(x)
    if not m or int(m.group(1)) < 1:
        raise GtfError(f"invalid position {x!r}")
    return int(m.group(1))


def parse_record(line):
    """-> (seqname, source, type, start, end, score | None, strand id | None, frame id | None); GtfError when malformed"""
    f = line.split(b"\t", 8)
    if len(f) < 9:
        raise GtfError(f"fewer than eight TABs: {line[:80]!r}")
    start, end = _position(f[3]), _position(f[4])
    try:
        score = None if f[5] == b"." else f32_from_str(f[5])
    except gff_expect.GffError as e:
        raise GtfError(str(e))
    if f[6] not in (b"+", b"-", b"."):
        raise GtfError(f"invalid strand {f[6]!r}")
    if f[7] not in (b".", b"0", b"1", b"2"):
        raise GtfError(f"invalid frame {f[7]!r}")
    return f[0], f[1], f[2], start, end, score, {b"+": 0, b"-": 1}.get(f[6]), (None if f[7] == b"." else int(f[7]))


def record_lines(text):
    """The record lines of `text` in file order; GtfError for an empty line."""
    out = []
    for line in lines_of(text):
        if not line:
            raise GtfError("empty line")
        if line[:1] != b"#":
            out.append(line)
    return out


def _utf8(raw, what, field):
    try:
        return raw.decode("utf-8")
    except UnicodeDecodeError:
        raise GtfError(f"attribute {what} is not UTF-8 in {field[:60]!r}")


def attributes(field):
    """field 9 (bytes) -> [(key, value), ...] in file order; GtfError when it breaks a rule"""
    out, pos, n = [], 0, len(field)
    while True:
        while pos < n and field[pos:pos + 1] == b" ":
            pos += 1
        if pos == n:
            return out
        if field[pos:pos + 1] == b";":
            raise GtfError(f"empty piece in {field[:60]!r}")
        sp = field.find(b" ", pos)
        semi = field.find(b";", pos)
        if sp < 0 or 0 <= semi < sp:
            raise GtfError(f"key without a value in {field[:60]!r}")
        key = field[pos:sp]
        pos = sp
        while pos < n and field[pos:pos + 1] == b" ":
            pos += 1
        if pos == n or field[pos:pos + 1] == b";":
            raise GtfError(f"key without a value in {field[:60]!r}")
        if field[pos:pos + 1] == b'"':
            close = field.find(b'"', pos + 1)
            if close < 0:
                raise GtfError(f"missing closing quote in {field[:60]!r}")
            value = field[pos + 1:close]
            pos = close + 1
            while pos < n and field[pos:pos + 1] == b" ":
                pos += 1
            if pos < n and field[pos:pos + 1] != b";":
                raise GtfError(f"bytes behind a closing quote in {field[:60]!r}")
            pos += 1
        else:
            semi = field.find(b";", pos)
            stop = n if semi < 0 else semi
            value = field[pos:stop].rstrip(b" ")
            pos = stop + 1
        out.append((_utf8(key, "key", field), _utf8(value, "value", field)))
        if pos >= n:
            return out


def columns(recs):
    """numpy columns of parsed records, named as the parser's (the eighth: frame_id / frame_valid, and as phase_* too)."""
    out = gff_expect.columns(recs)
    out["frame_id"], out["frame_valid"] = out["phase_id"], out["phase_valid"]
    return out


def expect(text, region=None, attrs=False, well_formed=False):
    """The columns a scan of `text` returns (with a region: the records the filter keeps; every record is validated either way).
    attrs: out["maps"] = the rows' [(key, value), ...] too, every record's ninth field validated.  well_formed (no region): the eight
    columns are taken on trust and only "maps" and "n_rows" are returned -- the generator's files, too long for parse_record."""
    rg = parse_region(region) if isinstance(region, str) else region
    recs, maps = [], []
    for line in record_lines(text):
        if well_formed and rg is None:
            rec, keep = None, True
            f9 = line.split(b"\t", 8)[8]
        else:
            rec = parse_record(line)
            keep = rg is None or hit(rec, rg)
            f9 = line.split(b"\t", 8)[8]
        if attrs:
            m = attributes(f9)
            if keep:
                maps.append(m)
        if keep:
            recs.append(rec)
    out = {"n_rows": len(recs)} if well_formed and rg is None else columns(recs)
    if attrs:
        out["maps"] = maps
    return out


def buffers(maps):
    """The five Arrow buffers of a run of rows' maps: offsets rows -> entries, entries -> key bytes, entries -> value bytes, and
    the two byte pools; and the three totals."""
    map_off, key_off, val_off = [0], [0], [0]
    keys, values = bytearray(), bytearray()
    for m in maps:
        for k, v in m:
            keys += k.encode()
            key_off.append(len(keys))
            values += v.encode()
            val_off.append(len(values))
        map_off.append(len(key_off) - 1)
    return {"map_offsets": np.array(map_off, np.int32), "key_offsets": np.array(key_off, np.int32), "key_values": np.frombuffer(bytes(keys), np.uint8),
            "value_offsets": np.array(val_off, np.int32), "value_values": np.frombuffer(bytes(values), np.uint8),
            "n_entries": len(key_off) - 1, "n_key_bytes": len(keys), "n_value_bytes": len(values)}
