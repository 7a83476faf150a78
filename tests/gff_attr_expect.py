"""Test infrastructure: what the GFF `attributes` column (Map<Utf8, List<Utf8>>) must hold, restated in plain Python.

Written from the ATTRIBUTE RULES as exon_amd/csrc/host/gff.h's header comment and DESIGN.md section 9 state them, not from the
C++: field 9 is everything behind the eighth TAB; "" and "." are a map of no entries; entries are split at every ';', exactly one
empty piece at the very end is ignored and any other empty piece is an error; a piece is split at its first '=' (none: an error;
an empty key is fine; an empty value is one empty item); a value with ',' is one item per piece, empty ones included; after the
splitting the key and every item are percent-decoded ('%' + two hex digits of either case -> that byte, any other '%' stays) and
must then be valid UTF-8; nothing is trimmed, duplicate keys stay, in file order.  Not product code: only tests import it.
"""
import re

import numpy as np

import gff_expect
from gff_expect import GffError

_ESC = re.compile(rb"%([0-9A-Fa-f]{2})")


def decode(raw):
    """percent-decoded and as str; GffError when the bytes are no UTF-8"""
    out = _ESC.sub(lambda m: bytes([int(m.group(1), 16)]), raw) if b"%" in raw else raw
    try:
        return out.decode("utf-8")
    except UnicodeDecodeError:
        raise GffError(f"invalid UTF-8 in attribute text {raw[:40]!r}")


def attributes(field):
    """field 9 (bytes) -> [(key, [item, ...]), ...] in file order"""
    if field in (b"", b"."):
        return []
    pieces = field.split(b";")
    if len(pieces) > 1 and pieces[-1] == b"":
        pieces.pop()
    out = []
    for p in pieces:
        if p == b"":
            raise GffError(f"empty attribute in {field[:60]!r}")
        key, eq, value = p.partition(b"=")
        if not eq:
            raise GffError(f"attribute without '=': {p[:60]!r}")
        out.append((decode(key), [decode(v) for v in value.split(b",")]))
    return out


def field9(line):
    f = line.split(b"\t", 8)
    if len(f) < 9:
        raise GffError(f"fewer than nine fields: {line[:80]!r}")
    return f[8]


def rows(text, region=None, well_formed=False):
    """The attributes of every record of `text` that a scan returns, as lists of (key, items) -- what pyarrow's to_pylist() gives
    for a map column.  Every record is validated (all nine columns), kept by the region filter or not.  well_formed (no region): the
    first eight columns are taken on trust -- the generator's files, too long for gff_expect.parse_record."""
    rg = gff_expect.parse_region(region) if isinstance(region, str) else region
    out = []
    for line in gff_expect.lines_of(text):
        if not line:
            raise GffError("empty line")
        if line[:1] == b"#":
            if line[:7] == b"##FASTA":
                raise gff_expect.GffUnsupported("##FASTA section")
            continue
        rec = None if well_formed and rg is None else gff_expect.parse_record(line)
        a = attributes(field9(line))
        if rg is None or gff_expect.hit(rec, rg):
            out.append(a)
    return out


def buffers(maps):
    """The six Arrow buffers of a run of rows' maps: offsets rows -> entries, entries -> key bytes, entries -> items, items ->
    item bytes, and the two byte pools."""
    map_off, key_off, list_off, item_off = [0], [0], [0], [0]
    keys, items = bytearray(), bytearray()
    for m in maps:
        for k, vs in m:
            keys += k.encode()
            key_off.append(len(keys))
            for v in vs:
                items += v.encode()
                item_off.append(len(items))
            list_off.append(len(item_off) - 1)
        map_off.append(len(key_off) - 1)
    return {"map_offsets": np.array(map_off, np.int32), "key_offsets": np.array(key_off, np.int32), "key_values": np.frombuffer(bytes(keys), np.uint8),
            "list_offsets": np.array(list_off, np.int32), "item_offsets": np.array(item_off, np.int32), "item_values": np.frombuffer(bytes(items), np.uint8),
            "n_entries": len(key_off) - 1, "n_items": len(item_off) - 1, "n_key_bytes": len(keys), "n_item_bytes": len(items)}
