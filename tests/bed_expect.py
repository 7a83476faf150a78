"""Test infrastructure: what a BED scan must return, restated in plain Python with unbounded integers.

Written from the rules (exon_amd/csrc/host/bed.h's header comment), not from the C++: lines end at '\\n' (one
'\\r' in front of it dropped, a last line without '\\n' read whole); a line starting with '#' is no row; every other line is split
at every TAB and decoded by its own field count -- 3: name of the sequence, start, end; 4: the same (the name is dropped: NULL);
5: plus name and score; 6 and 12: plus strand -- and any other count (an empty line is one field) is an error.  start / end are
Rust's usize::from_str (digits, one leading '+') with 0 allowed and nothing above i64::MAX; score is u16::from_str (0 .. 65535,
no '.'); strand is '+', '-' or '.' (NULL); name is the field's bytes as they stand; the whole line must be valid UTF-8.  Columns
6 .. 11 are NULL on every row.  Not product code: only tests import it."""
import re

import numpy as np

from gff_expect import lines_of

STRANDS = ["+", "-"]
COLUMNS = ["reference_sequence_name", "start", "end", "name", "score", "strand", "thick_start", "thick_end", "color", "block_count",
           "block_sizes", "block_starts"]
UTF8_COLUMNS = {"name", "color", "block_sizes", "block_starts"}
I64_MAX = 2**63 - 1
U16_MAX = 65535
_UINT = re.compile(rb"\+?([0-9]+)\Z")


class BedError(ValueError):
    pass


def mask_of(n_fields):
    """the projection mask of the reference's n_fields = k (3 .. 12): bits 3 .. k - 1"""
    assert 3 <= n_fields <= 12
    return sum(1 << b for b in range(3, n_fields))


def _uint(x, most, what):
    m = _UINT.match(x)
    if not m or int(m.group(1)) > most:
        raise BedError(f"invalid {what} {x!r}")
    return int(m.group(1))


def parse_record(line):
    """-> (reference_sequence_name, start, end, name | None, score | None, strand id | None); BedError when malformed"""
    f = line.split(b"\t")
    if len(f) not in (3, 4, 5, 6, 12):
        raise BedError(f"invalid number of fields: {len(f)}: {line[:80]!r}")
    try:
        line.decode("utf-8")
    except UnicodeDecodeError:
        raise BedError(f"not UTF-8: {line[:80]!r}")
    start, end = _uint(f[1], I64_MAX, "start"), _uint(f[2], I64_MAX, "end")
    name = score = strand = None
    if len(f) >= 5:
        name, score = f[3], _uint(f[4], U16_MAX, "score")
    if len(f) >= 6:
        if f[5] not in (b"+", b"-", b"."):
            raise BedError(f"invalid strand {f[5]!r}")
        strand = {b"+": 0, b"-": 1}.get(f[5])
    return f[0], start, end, name, score, strand


def records(text):
    """Every record of `text` in file order (all of them validated)."""
    return [parse_record(line) for line in lines_of(text) if line[:1] != b"#"]


def expect(text):
    """The columns of a scan of `text`: n_rows, chrom (bytes a row), start / end (int64), names (bytes | None a row), score /
    score_valid, strand_id / strand_valid."""
    recs = records(text)
    n = len(recs)
    return {"n_rows": n, "chrom": [r[0] for r in recs], "start": np.array([r[1] for r in recs], np.int64).reshape(n),
            "end": np.array([r[2] for r in recs], np.int64).reshape(n), "names": [r[3] for r in recs],
            "score_valid": np.array([r[4] is not None for r in recs], bool).reshape(n),
            "score": np.array([r[4] or 0 for r in recs], np.int64).reshape(n),
            "strand_valid": np.array([r[5] is not None for r in recs], bool).reshape(n),
            "strand_id": np.array([r[5] or 0 for r in recs], np.int32).reshape(n)}
