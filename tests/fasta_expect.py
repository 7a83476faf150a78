"""What a FASTA reader must return for a text, written from the rules alone (no import of the package, the library or the oracle):

  * lines end at '\\n'; one '\\r' in front of it is dropped, on definition lines and on sequence lines;
  * a line whose first byte is '>' starts a record, the definition is the rest of that line;
  * id = the definition up to the first ' ' or '\\t' (it may be empty); description = what follows the run of ' ' / '\\t' behind the id,
    None when nothing follows;
  * sequence = every following line up to the next '>' line or the end of the input, concatenated as it stands (inner blanks kept, empty
    lines add nothing, "" without sequence lines);
  * text in front of the first '>' line is skipped.

Everything is bytes -> str through latin-1 so that any byte survives; the tests write ASCII."""


def lines_of(text):
    """the lines of `text` (bytes) without their terminators; a last line without '\\n' counts, an empty rest does not"""
    parts = text.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    return [p[:-1] if p.endswith(b"\r") else p for p in parts]


def split_definition(d):
    """definition bytes -> (id, description or None)"""
    ws = 0
    while ws < len(d) and d[ws] not in b" \t":
        ws += 1
    k = ws
    while k < len(d) and d[k] in b" \t":
        k += 1
    return d[:ws].decode("latin-1"), (d[k:].decode("latin-1") if k < len(d) else None)


def records(text):
    """[(id, description, sequence)] of a whole input"""
    out, cur = [], None
    for ln in lines_of(text):
        if ln[:1] == b">":
            if cur is not None:
                out.append(cur)
            cur = [ln[1:], []]
        elif cur is not None:
            cur[1].append(ln)
    if cur is not None:
        out.append(cur)
    return [split_definition(d) + (b"".join(seq).decode("latin-1"),) for d, seq in out]


def columns(text):
    r = records(text)
    return {"id": [x[0] for x in r], "description": [x[1] for x in r], "sequence": [x[2] for x in r]}


def slab(text, final):
    """What the device parser must report for one slab that starts with a '>' line: the definitions (bytes behind '>', CR dropped) and
    sequence lengths of the records it emits, and how many bytes they take.  A slab that is not the input's last never emits its last
    record and ends its consumed bytes directly in front of that record's definition line; the final slab (which ends with '\\n')
    emits everything and consumes everything."""
    starts, pos = [], 0
    for raw in text.split(b"\n")[:-1]:  # (what follows the last '\n' is no line yet)
        if raw[:1] == b">":
            starts.append(pos)
        pos += len(raw) + 1
    whole = text[:pos]
    if final:
        n, consumed = len(starts), len(whole)
    else:
        n = max(len(starts) - 1, 0)
        consumed = starts[-1] if len(starts) >= 2 else 0
    defs, lens = [], []
    for k in range(n):
        end = starts[k + 1] if k + 1 < len(starts) else len(whole)
        ls = lines_of(whole[starts[k]:end])
        defs.append(ls[0][1:])
        lens.append(sum(len(x) for x in ls[1:]))
    return {"n_records": n, "consumed": consumed, "definitions": defs, "seq_len": lens}


def write_text(rows, newline=b"\n", final_newline=True):
    """rows: (definition bytes, [sequence line bytes, ...]) -> the file's bytes"""
    out = []
    for d, seq in rows:
        out.append(b">" + d)
        out.extend(seq)
    t = newline.join(out)
    return t + newline if final_newline and out else t
