"""Test infrastructure: what the shared line index and the per-format framing on top of it must report for a slab of text, stated in
plain numpy (no import of the package, the library or the oracle), and builders of slabs whose newlines sit exactly where a test wants
them.

The statement
  newlines(buf)           the positions of the bytes of value 10, in order
  lines(buf)              per terminated line: begin, end (its newline) and end without one CR
  consumed(buf)           the last newline's position + 1, 0 without one: the bytes a caller may discard
  fastq_views(buf, final) lines in fours: header, sequence and quality spans with one CR dropped, the bytes the whole records take
                          and the records the splitter cannot decide -- a first byte that is not '@', a third line that does not
                          start with '+', and, in the input's last slab, a line count that is no multiple of 4
FASTA comes from fasta_expect, the tabular columns from the format's own *_expect module.

The geometry of the index kernel the builders are used around: a load group of 16 bytes, 64 bytes a thread, 4096 a wave, 65536 a
tile (one workgroup), 64 tiles a look-back round."""
import numpy as np

GROUP, THREAD, WAVE, TILE, ROUND = 16, 64, 4096, 65536, 64
EDGES = (GROUP, THREAD, WAVE, TILE, 2 * TILE)
FORMATS = ("fasta", "fastq", "vcf", "sam", "gff", "bed")
BASES = b"ACGTN"
# the header the VCF rows of with_newlines_at are read under
VCF_HEADER = (b"##fileformat=VCFv4.2\n##INFO=<ID=A,Number=1,Type=String,Description=\"padding\">\n"
              b"##INFO=<ID=FL,Number=0,Type=Flag,Description=\"two bytes of padding\">\n##contig=<ID=1>\n"
              b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")


def _arr(buf):
    return buf if isinstance(buf, np.ndarray) else np.frombuffer(bytes(buf), np.uint8)


def newlines(buf):
    return np.flatnonzero(_arr(buf) == 10)


def lines(buf):
    """(begin, end, end_without_cr) of every terminated line: line i is buf[begin[i]:end[i]], buf[end[i]] its newline; one CR in
    front of the newline is dropped when the line has a byte at all"""
    a = _arr(buf)
    end = newlines(a)
    begin = np.concatenate([[0], end[:-1] + 1]).astype(np.int64) if len(end) else np.zeros(0, np.int64)
    cr = np.zeros(len(end), bool)
    some = end > begin
    cr[some] = a[end[some] - 1] == 13
    return begin, end.astype(np.int64), end.astype(np.int64) - cr


def consumed(buf):
    nl = newlines(buf)
    return int(nl[-1]) + 1 if len(nl) else 0


def fastq_views(buf, final):
    """Record r is lines 4r .. 4r + 3.  head: the first line behind its first byte; seq / qual: the second and fourth line; each
    without one CR, which is dropped only where the span has a byte in front of it.  consumed: the bytes of the whole records.
    n_undecided: one per record whose first byte is not '@' or whose third line does not start with '+', one more for a final
    slab whose line count is no multiple of 4."""
    a = _arr(buf)
    begin, end, _ = lines(a)
    n_lines = len(end)
    n = n_lines // 4
    b, e = begin[:4 * n].reshape(n, 4), end[:4 * n].reshape(n, 4)

    def span(start, stop):
        stop = stop.copy()
        some = stop > start
        drop = np.zeros(n, bool)
        drop[some] = a[stop[some] - 1] == 13
        return start, stop - drop

    head = span(b[:, 0] + 1, e[:, 0])
    seq = span(b[:, 1], e[:, 1])
    qual = span(b[:, 3], e[:, 3])
    bad = (a[b[:, 0]] != ord("@")) | (a[b[:, 2]] != ord("+")) if n else np.zeros(0, bool)
    return {"n_lines": n_lines, "n_reads": n, "consumed": int(e[-1, 3]) + 1 if n else 0,
            "n_undecided": int(bad.sum()) + (1 if final and n_lines % 4 else 0),
            "head_start": head[0], "head_end": head[1], "seq_start": seq[0], "seq_end": seq[1],
            "qual_start": qual[0], "qual_end": qual[1]}


# ---- slabs with their newlines where a test wants them ------------------------------------------------------------------------------
NOISE = None  # see noise()


def noise(seed=20240607, n=1 << 20):
    """Letters without a period, for the padding of slabs that go through a compressor: periodic text deflates into blocks of
    several MB of output, more than a small slab of a gzip scan holds.  with_newlines_at(..., noisy=True) pads from it."""
    global NOISE
    if NOISE is None:
        NOISE = np.random.RandomState(seed).choice(np.frombuffer(b"ACGTNacgtnRYKMxyz", np.uint8), n).tobytes()
    return NOISE


def _fill(pattern, n, shift=0, noisy=False):
    if noisy and 0 < n < len(noise()) // 2:
        at = (shift * 7919 + n * 104729) % (len(NOISE) - n)
        return NOISE[at:at + n]
    reps = (n + shift) // len(pattern) + 1
    return (pattern * reps)[shift:shift + n]


def _tab_row(fmt, i, length, noisy=False):
    """row i of a tabular format in exactly `length` bytes (without its newline): the row number + 1 is the row's POS / start, the
    free-text last field takes the padding"""
    p = i + 1
    if fmt == "vcf":  # INFO: '.', a Flag key, or A=<text>
        head = b"1\t%d\t.\tA\tC\t.\t.\t" % p
        k = length - len(head)
        tail = b"." if k == 1 else b"FL" if k == 2 else b"A=" + _fill(b"xyz", k - 2, i, noisy) if k > 2 else None
    elif fmt == "sam":  # one optional field XX:Z:<text>; the few lengths it cannot give go into the read name
        k = length - len(b"r\t0\t*\t%d\t0\t*\t*\t0\t0\t*\t*" % p)
        if k < 0:
            raise ValueError("a SAM row of %d bytes" % length)
        name = b"r" + (_fill(b"n", k) if 0 < k < 7 else b"")
        head, tail = name + b"\t0\t*\t%d\t0\t*\t*\t0\t0\t*\t*" % p, (b"\tXX:Z:" + _fill(b"xyz", k - 6, i, noisy) if k >= 7 else b"")
    elif fmt == "gff":
        head = b"s\t.\tt\t%d\t%d\t.\t.\t.\t" % (p, p + 9)
        k = length - len(head)
        tail = b"a=" + _fill(b"xyz", k - 2, i, noisy) if k > 2 else None
    elif fmt == "bed":  # five fields: the readers give a name only next to a score
        head = b"c\t%d\t%d\t" % (p, p + 9)
        k = length - len(head) - 2
        tail = _fill(b"nam", k, i, noisy) + b"\t7" if k > 0 else None
    else:
        raise ValueError(fmt)
    if tail is None:
        raise ValueError("a %s row of %d bytes" % (fmt, length))
    return head + tail


def min_row(fmt, i):
    """the shortest row _tab_row writes as row i"""
    k = 1
    while True:
        try:
            _tab_row(fmt, i, k)
            return k
        except ValueError:
            k += 1


def _line(fmt, i, length, strict, crlf, defs=None, noisy=False):
    """line i of a slab in `length` bytes; crlf: its last byte is a CR"""
    n = length - (1 if crlf else 0)
    cr = b"\r" if crlf else b""
    if n < 0:
        raise ValueError("a CRLF line of %d bytes" % length)
    if fmt == "fasta":  # a definition first, then one every seventh line where it fits
        if (i == 0 or (i % 7 == 0 if defs is None else i in defs)) and n >= 2:
            return b">d" + _fill(b"%d " % i, n - 2) + cr if n > 2 else b">d" + cr
        if i == 0:
            raise ValueError("a slab starts with a definition line of two bytes or more")
        return _fill(BASES, n, i, noisy) + cr
    if fmt == "fastq":
        kind = i % 4
        if kind == 1:
            return _fill(BASES, n, i, noisy) + cr
        if kind == 3:
            return _fill(b"IHGFEDCB", n, i, noisy) + cr
        if n == 0:
            if strict:
                raise ValueError("an empty FASTQ header or '+' line")
            return cr
        return (b"@" + _fill(b"r%d " % i, n - 1) if kind == 0 else b"+" + _fill(b"p", n - 1)) + cr
    return _tab_row(fmt, i, n, noisy) + cr


def with_newlines_at(n_bytes, positions, fmt, strict=True, crlf=(), tail=None, defs=None, noisy=False):
    """A slab of n_bytes bytes whose newlines sit exactly at `positions` (ascending) and whose lines are valid for `fmt`: FASTA
    definition (`>d...`) and sequence lines of any length, FASTQ records of four lines, VCF / SAM / GFF / BED rows with the row
    number + 1 in POS / start and the padding in the free-text last field.  crlf: the lines (by number) that end in CR LF.
    noisy: the padding comes out of noise() instead of a short period.
    defs (FASTA): the lines that are definition lines, every seventh without it (a line of less than two bytes is a sequence line).
    Bytes behind the last newline are an unterminated line of the same kind (`tail`: those bytes as given).
    strict=False (FASTQ): a header or '+' line that the positions leave no byte is written empty -- fastq_views says what a
    splitter makes of it."""
    positions = [int(p) for p in positions]
    assert positions == sorted(set(positions)) and (not positions or (0 <= positions[0] and positions[-1] < n_bytes))
    out, at = [], 0
    crlf = set(crlf)
    for i, p in enumerate(positions):
        out.append(_line(fmt, i, p - at, strict, i in crlf, defs, noisy))
        out.append(b"\n")
        at = p + 1
    rest = n_bytes - at
    if tail is not None:
        assert len(tail) == rest and b"\n" not in tail
        out.append(tail)
    elif rest:
        try:
            out.append(_line(fmt, len(positions), rest, False if fmt == "fastq" else strict, False, defs, noisy))
        except ValueError:
            out.append(_fill(b"x", rest))
    text = b"".join(out)
    assert len(text) == n_bytes
    return text


def dense(first_line_bytes, n_empty, fmt="fasta"):
    """One line of first_line_bytes bytes (its newline included) and a run of n_empty empty lines behind it: the run starts at byte
    first_line_bytes"""
    first = _line(fmt, 0, first_line_bytes - 1, True, False)
    return first + b"\n" + b"\n" * n_empty


def edge_positions(n_bytes, deltas=(-1, 0, 1), first=None):
    """newlines at e + d for every edge e of the index kernel below n_bytes and every d, one in the first load group (`first`,
    default 3) and one as the slab's last byte"""
    ps = {e + d for e in EDGES for d in deltas if 0 <= e + d < n_bytes}
    ps.add(3 if first is None else first)
    ps.add(n_bytes - 1)
    return sorted(ps)
