"""Test infrastructure: what a GFF3 scan must return, restated in plain Python, and a tabix writer for GFF files.

Written from the rules (exon_amd/csrc/host/gff.h's header comment), not from the C++: lines end at '\\n'
(one '\\r' in front of it dropped); a line starting with '#' is no row; every other line is a record of nine TAB-separated
fields (the ninth = whatever follows the eighth TAB) validated against all eight columns; start / end are Rust's
usize::from_str (one leading '+', up to 18 digits here) and >= 1; score is '.' or Rust's f32::from_str, correctly rounded;
strand is one of + - . ?; phase one of . 0 1 2; an empty line or a short record is an error; a "##FASTA" line is refused.
A region keeps a record when seqname == name and start lies in [a, b] (the start alone).  Not product code: only tests import it.
"""
import bisect
import fractions
import functools
import gzip
import re
import struct

import numpy as np

from bgzf_index_writer import RefIndex, VirtualOffsets, bgzf_blocks

STRANDS = ["+", "-"]
PHASES = ["0", "1", "2"]
OPEN_END = 2**63 - 1


class GffError(ValueError):
    pass


class GffUnsupported(GffError):
    pass


_POS = re.compile(rb"\+?([0-9]{1,18})\Z")
_F32 = re.compile(rb"[+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)\Z")
_F32_WORD = re.compile(rb"([+-]?)(inf|infinity|nan)\Z", re.I)


@functools.lru_cache(maxsize=1 << 16)
def f32_from_str(s):
    """Rust's str::parse::<f32>: the float nearest to the decimal's exact value, ties to even."""
    m = _F32_WORD.match(s)
    if m:
        v = np.float32(np.nan if m.group(2).lower() == b"nan" else np.inf)
        return -v if m.group(1) == b"-" else v
    if not _F32.match(s):
        raise GffError(f"invalid score {s!r}")
    t = s.decode().lower()
    mant, _, exp = t.partition("e")
    exact = fractions.Fraction(mant if mant[-1] != "." else mant + "0") * fractions.Fraction(10) ** int(exp or 0)
    with np.errstate(over="ignore"):
        guess = np.float32(float(exact)) if abs(exact) < fractions.Fraction(10) ** 60 else np.float32(np.inf if exact > 0 else -np.inf)
    best = None
    for c in (np.nextafter(guess, np.float32(-np.inf)), guess, np.nextafter(guess, np.float32(np.inf))):
        if not np.isfinite(c):
            continue
        err = abs(fractions.Fraction(float(c)) - exact)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[1]):
            best = (err, even, c)
    fmax = fractions.Fraction(float(np.finfo(np.float32).max))
    if abs(exact) >= fmax + fractions.Fraction(2) ** 103:  # beyond the midpoint to 2^128: infinity
        return np.float32(np.inf if exact > 0 else -np.inf)
    v = np.float32(best[2])
    if v == 0 and t.lstrip("+").startswith("-"):
        v = np.float32(-0.0)
    return v


def lines_of(text):
    """The lines of `text` (bytes): terminator dropped, and one CR in front of a '\\n'."""
    out, u = [], 0
    while u < len(text):
        e = text.find(b"\n", u)
        if e < 0:
            out.append(text[u:])
            break
        out.append(text[u:e - 1] if e > u and text[e - 1:e] == b"\r" else text[u:e])
        u = e + 1
    return out


@functools.lru_cache(maxsize=1 << 18)
def parse_record(line):
    """-> (seqname, source, type, start, end, score | None, strand id | None, phase id | None); GffError when malformed"""
    f = line.split(b"\t", 8)
    if len(f) < 9:
        raise GffError(f"fewer than nine fields: {line[:80]!r}")
    pos = []
    for x in f[3:5]:
        m = _POS.match(x)
        if not m or int(m.group(1)) < 1:
            raise GffError(f"invalid position {x!r}")
        pos.append(int(m.group(1)))
    score = None if f[5] == b"." else f32_from_str(f[5])
    if f[6] not in (b"+", b"-", b".", b"?"):
        raise GffError(f"invalid strand {f[6]!r}")
    if f[7] not in (b".", b"0", b"1", b"2"):
        raise GffError(f"invalid phase {f[7]!r}")
    strand = {b"+": 0, b"-": 1}.get(f[6])
    phase = None if f[7] == b"." else int(f[7])
    return f[0], f[1], f[2], pos[0], pos[1], score, strand, phase


def records(text):
    """Every record of `text` in file order (all of them validated)."""
    out = []
    for line in lines_of(text):
        if not line:
            raise GffError("empty line")
        if line[:1] == b"#":
            if line[:7] == b"##FASTA":
                raise GffUnsupported("##FASTA section")
            continue
        out.append(parse_record(line))
    return out


def parse_region(region):
    """'chr1', 'chr1:5' (from 5 on), 'chr1:5-9' -> (name, a, b)"""
    name, _, iv = region.partition(":")
    if not iv:
        return name, 1, OPEN_END
    a, _, b = iv.partition("-")
    return name, int(a), (int(b) if b else OPEN_END)


def hit(rec, region):
    name, a, b = region
    return rec[0] == name.encode() and a <= rec[3] <= b


def columns(recs):
    """numpy columns of `recs`: dictionary ids in order of first appearance + the names, values, byte-per-row validity."""
    out = {"n_rows": len(recs)}
    for k, col in enumerate(("seqname", "source", "type")):
        names, ids = [], {}
        out[col + "_id"] = np.array([ids.setdefault(r[k], len(ids)) for r in recs], np.int32)
        names = [None] * len(ids)
        for nm, i in ids.items():
            names[i] = nm.decode(errors="replace")
        out[col + "_names"] = names
        out[col] = np.array([r[k].decode(errors="replace") for r in recs], object)
    out["start"] = np.array([r[3] for r in recs], np.int64)
    out["end"] = np.array([r[4] for r in recs], np.int64)
    out["score"] = np.array([np.float32(0) if r[5] is None else r[5] for r in recs], np.float32)
    out["score_valid"] = np.array([r[5] is not None for r in recs], bool)
    out["strand_id"] = np.array([r[6] or 0 for r in recs], np.int32)
    out["strand_valid"] = np.array([r[6] is not None for r in recs], bool)
    out["phase_id"] = np.array([r[7] or 0 for r in recs], np.int32)
    out["phase_valid"] = np.array([r[7] is not None for r in recs], bool)
    return out


def expect(text, region=None):
    """The columns a scan of `text` returns (with a region: the records the reader's filter keeps)."""
    recs = records(text)
    if region is not None:
        rg = parse_region(region) if isinstance(region, str) else region
        recs = [r for r in recs if hit(r, rg)]
    return columns(recs)


def interval_columns(text):
    """(seqname names in order of first appearance, ids int32, start int64, end int64) of a WELL-FORMED file (the generator's):
    only what the region, overlap and within predicates read, for files too long for records()."""
    names, ids, seq, start, end = [], {}, [], [], []
    for line in text.split(b"\n"):
        if not line or line[:1] == b"#":
            continue
        f = line.split(b"\t", 5)
        seq.append(ids.setdefault(f[0], len(ids)))
        start.append(int(f[3]))
        end.append(int(f[4]))
    names = [None] * len(ids)
    for nm, i in ids.items():
        names[i] = nm.decode()
    return names, np.array(seq, np.int32), np.array(start, np.int64), np.array(end, np.int64)


# ---- tabix for GFF -------------------------------------------------------------------------------------------------

def write_gff_tabix(gff_gz):
    """<gff_gz>.tbi for a BGZF-compressed GFF sorted by (seqname, start): the generic preset with sequence column 1, begin
    column 4, end column 5, comment character '#'.  Returns the number of records indexed."""
    raw = open(gff_gz, "rb").read()
    blocks = bgzf_blocks(raw)
    vo = VirtualOffsets(blocks)
    text = b"".join(d for _, _, d in blocks)
    names, refs, n, u = [], {}, 0, 0
    while u < len(text):
        e = text.find(b"\n", u)
        e = len(text) if e < 0 else e + 1
        line = text[u:e]
        if line[:1] != b"#" and line.strip():
            f = line.split(b"\t", 5)
            name, beg, end = f[0].decode(), int(f[3]), int(f[4])
            if name not in refs:
                names.append(name)
                refs[name] = RefIndex()
            refs[name].add(beg - 1, max(beg, end), vo.at(u), vo.at(e))
            n += 1
        u = e
    nm = b"".join(x.encode() + b"\0" for x in names)
    body = b"TBI\1" + struct.pack("<8i", len(names), 0, 1, 4, 5, ord("#"), 0, len(nm)) + nm
    body += b"".join(refs[x].pack() for x in names)
    with gzip.open(str(gff_gz) + ".tbi", "wb") as fh:
        fh.write(body)
    return n


@functools.lru_cache(maxsize=4)
def read_tabix(path):
    """-> (header ints {format, col_seq, col_beg, col_end, meta, skip}, names, [(bins {bin: [(v0, v1)]}, linear)])"""
    raw = gzip.open(path, "rb").read()
    assert raw[:4] == b"TBI\1"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", raw, 4)
    o = 36
    names = [x.decode() for x in raw[o:o + l_nm].split(b"\0")[:-1]]
    o += l_nm
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", raw, o)[0]
        o += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", raw, o)
            o += 8
            chunks = [struct.unpack_from("<QQ", raw, o + 16 * k) for k in range(n_chunk)]
            o += 16 * n_chunk
            if b != 37450:
                bins[b] = chunks
        n_intv = struct.unpack_from("<i", raw, o)[0]
        o += 4
        linear = list(struct.unpack_from(f"<{n_intv}Q", raw, o))
        o += 8 * n_intv
        refs.append((bins, linear))
    return dict(format=fmt, col_seq=col_seq, col_beg=col_beg, col_end=col_end, meta=meta, skip=skip), names, refs


def query_chunks(tbi, region):
    """The merged chunks a tabix query of `region` reads (UCSC binning, the linear index' lower bound, overlapping chunks merged)."""
    _hdr, names, refs = read_tabix(tbi)
    name, a, b = region
    if name not in names:
        return []
    bins, linear = refs[names.index(name)]
    b = min(b, (1 << 29) - 1)
    a = max(a, 1)
    if a > b:
        return []
    beg, end = a - 1, b - 1
    want, offset, shift = [0], 1, 26
    for level in range(1, 6):
        want += [offset + k for k in range(beg >> shift, (end >> shift) + 1)]
        offset += 1 << (3 * level)
        shift -= 3
    chunks = [c for w in want for c in bins.get(w, [])]
    win = beg >> 14
    lo = linear[win] if win < len(linear) else 0
    chunks = sorted(c for c in chunks if c[1] > lo)
    merged = []
    for v0, v1 in chunks:
        if merged and v0 <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], v1)
        else:
            merged.append([v0, v1])
    return [tuple(c) for c in merged]


@functools.lru_cache(maxsize=2)
def _block_table(gff_gz):
    blocks = bgzf_blocks(open(gff_gz, "rb").read())
    return blocks, [c for c, _, _ in blocks]


def indexed_records(gff_gz, region, reference_quirk=False):
    """The records an indexed scan of `region` returns.  Default: every record that starts inside a chunk and that the filter
    keeps.  reference_quirk: the reference's opener reads the COMPRESSED range [chunk.start.compressed, chunk.end.compressed)
    -- the whole rest of the file when both lie in one block -- from the chunk start's offset in its first block; the block that
    holds the chunk's end is never read, and a last line that has no '\\n' inside the range is dropped."""
    rg = parse_region(region) if isinstance(region, str) else region
    blocks, coffs = _block_table(str(gff_gz))
    out = []
    for v0, v1 in query_chunks(str(gff_gz) + ".tbi", rg):
        i0 = bisect.bisect_left(coffs, v0 >> 16)
        if reference_quirk:
            hi = len(blocks) if (v1 >> 16) == (v0 >> 16) else bisect.bisect_left(coffs, v1 >> 16)
            data = b"".join(d for _, _, d in blocks[i0:hi])[v0 & 0xFFFF:]
            data = data[:data.rfind(b"\n") + 1]
        else:
            # everything from the chunk's start; a record belongs to the chunk when it STARTS in front of the chunk's end
            i1 = bisect.bisect_right(coffs, v1 >> 16)
            data = b"".join(d for _, _, d in blocks[i0:])[v0 & 0xFFFF:]
            limit = sum(len(d) for _, _, d in blocks[i0:i1 - 1]) + (v1 & 0xFFFF) - (v0 & 0xFFFF) if i1 > i0 else 0
            cut, u = 0, 0
            while u < len(data) and u < limit:
                e = data.find(b"\n", u)
                u = len(data) if e < 0 else e + 1
                cut = u
            data = data[:cut]
        out += [r for r in records(data) if hit(r, rg)]
    return out
