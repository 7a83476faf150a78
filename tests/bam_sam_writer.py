"""Test-side writer of a BAM file (SAM specification 4.2) and its SAM twin from python dicts, independent of the product's
decoders and of the oracle.  A record: dict(name (str; "" = l_read_name 1, "*" = the missing name), flag, ref (index into
`refs` or None), pos (1-based, 0 = none), mapq, cigar [(length, op code 0..15)], seq (text over "=ACMGRSVTWYHKDBN"),
qual (one int 0..255 per base)).  Nothing is validated: op codes 9-15, op lengths 0 and 2^28 - 1, an odd or zero l_seq and
quality bytes beyond 93 are written as given.  `expected` says what the name / cigar / sequence / quality_score columns of
such records must hold (exon-bam/src/array_builder.rs:105-201), from the dicts alone."""
import struct
import subprocess

BASES = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"
REFS = [("r1", 1 << 29), ("r2", 1 << 29)]


def bam_record(r):
    name = r["name"].encode() + b"\0"
    seq, qual = r["seq"], r["qual"]
    assert len(qual) == len(seq) and len(name) <= 255
    codes = [BASES.index(c) for c in seq] + [0]
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(seq), 2))
    cigar = b"".join(struct.pack("<I", (n << 4) | op) for n, op in r["cigar"])
    ref = -1 if r["ref"] is None else r["ref"]
    body = struct.pack("<iiBBHHHiiii", ref, r["pos"] - 1, len(name), r["mapq"], 4680, len(r["cigar"]), r["flag"], len(seq), -1, -1, 0)
    body += name + cigar + packed + bytes(qual)
    return struct.pack("<i", len(body)) + body


def write_bam(path, recs, bgzip, refs=REFS):
    """uncompressed BAM stream -> `bgzip` (tools/bin/bgzip) -> path"""
    text = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    out = [b"BAM\1", struct.pack("<i", len(text)), text.encode(), struct.pack("<i", len(refs))]
    for n, ln in refs:
        out.append(struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln))
    out.extend(bam_record(r) for r in recs)
    raw = str(path) + ".u"
    with open(raw, "wb") as f:
        f.write(b"".join(out))
    subprocess.check_call([bgzip, raw, str(path), "6"], stdout=subprocess.DEVNULL)


def sam_line(r, refs=REFS):
    """the record as a SAM line (no line end).  Keys `cigar_text` / `qual_text` / `extra` (further fields) replace what the
    writer would print: lines the readers refuse or print differently are written through them."""
    cigar = r.get("cigar_text")
    if cigar is None:
        cigar = "".join(f"{n}{OPS[op]}" for n, op in r["cigar"]) or "*"
    qual = r.get("qual_text")
    if qual is None:
        qual = "".join(chr(q + 33) for q in r["qual"]) or "*"
    f = [r["name"], str(r["flag"]), "*" if r["ref"] is None else refs[r["ref"]][0], str(r["pos"]), str(r["mapq"]), cigar, "*", "0", "0",
         r["seq"] or "*", qual] + list(r.get("extra", []))
    return "\t".join(f)


def write_sam(path, recs, refs=REFS, eol=lambda i: "\n"):
    with open(path, "w", newline="") as f:
        f.write("@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs))
        for i, r in enumerate(recs):
            f.write(sam_line(r, refs) + eol(i))


REF_CONSUMING = (0, 2, 3, 7, 8)


def expected(recs, sam, refs=REFS):
    """the columns both readers must give.  BAM: an op code beyond 8 prints as '?'; quality bytes are i8 widened to i64.
    SAM: the fields' text ('*' = none); Phred = character - 33; QUAL may be '*' beside a SEQ (`qual_text`)."""
    out = dict(name=[], cigar=[], sequence=[], quality_score=[], flag=[], start=[], end=[], reference=[])
    for r in recs:
        out["name"].append(None if r["name"] == "*" else r["name"])
        out["sequence"].append(r["seq"])
        out["flag"].append(r["flag"])
        out["reference"].append(None if r["ref"] is None else refs[r["ref"]][0])
        out["start"].append(r["pos"] if r["pos"] >= 1 else None)
        span = sum(n for n, op in r["cigar"] if op in REF_CONSUMING)
        out["end"].append(r["pos"] + span - 1 if r["pos"] >= 1 else None)
        if sam:
            out["cigar"].append("".join(f"{n}{OPS[op]}" for n, op in r["cigar"]))
            qt = r.get("qual_text") or "".join(chr(q + 33) for q in r["qual"])  # (one base of Phred 9 prints as '*': no qualities)
            out["quality_score"].append([] if qt == "*" else [ord(c) - 33 for c in qt])
        else:
            out["cigar"].append("".join(f"{n}{OPS[op] if op < 9 else '?'}" for n, op in r["cigar"]))
            out["quality_score"].append([q - 256 if q > 127 else q for q in r["qual"]])
    return out
