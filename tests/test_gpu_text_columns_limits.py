"""The Arrow string and list columns text_columns.hip builds on the device (VCF / BCF id, ref, alt; BAM / SAM name, cigar,
sequence, quality_score; the four FASTQ columns) and scan.cpp's export of them (views, batch cuts, the row-by-row gather) at
their limits: row counts on the kernels' borders, cell values on the edges of every field, totals on either side of the
scratch capacities, batch and slab cuts, and the gather.

Every expectation is computed here from the python rows the test wrote (vcf_bcf_writer, bam_sam_writer, the FASTQ lines
below), never from a product path.  Each file is read three ways: the host reader and oracle/decode.py (CPU tests, no
marker) and the GPU pipeline (-m gpu), all against that expectation."""
import os
import subprocess

import pytest

import bam_sam_writer as bsw
import exon_amd
import vcf_bcf_writer as vbw
from oracle import decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")

FORMATS = ["vcf", "vcf.gz", "bcf", "bam", "sam", "fastq"]
VCF_KEYS = ("chrom", "pos", "id", "ref", "alt")
BAM_KEYS = ("flag", "reference", "start", "name", "cigar", "sequence", "quality_score")
FASTQ_KEYS = ("name", "description", "sequence", "quality_scores")
KEYS = {"vcf": VCF_KEYS, "bcf": VCF_KEYS, "bam": BAM_KEYS, "sam": BAM_KEYS, "fastq": FASTQ_KEYS}
PROJECT = {"vcf": ("id", "ref", "alt"), "bcf": ("id", "ref", "alt"), "bam": ("name", "cigar", "sequence", "quality_score"),
           "sam": ("name", "cigar", "sequence", "quality_score"), "fastq": None}


# ---- the rows ------------------------------------------------------------------------------------------------------------------
def is_null(i, mode="some"):
    """the NULL rhythm: the first and the last row of every 32-row group, and every 7th row from 3 on -- not periodic in 32"""
    return {"all": True, "none": False}.get(mode, i % 32 in (0, 31) or i % 7 == 3)


IDS = ["a", "bc", "a;b", "rs1234", "x;yz;w"]  # 1-6 bytes; period 5 (coprime to 32)
REFS = ["A", "AC", "ACG", "ACGT", "ACGTA", "G", "TT"]  # period 7
ALTS = [["C"], ["C", "GT"], ["T", "A", "CCC"]]


def variant(i, chrom="1", nulls="some", **kw):
    r = dict(chrom=chrom, pos=i + 1, qual=None, filter=[], info=None, ref=REFS[i % 7])
    r["id"] = "." if is_null(i, nulls) else IDS[i % 5]
    r["alt"] = None if is_null(i + 5, nulls) else ALTS[i % 3]
    r.update(kw)
    return r


def variant_expected(rows, fmt):
    """VCF text goes through the reference's lazy builder: id NULL for '.' or an empty field, else its ';'-separated items
    (empty ones kept); alt NULL for '.', else a list WITHOUT items.  BCF through the eager builder: lists with their items,
    never NULL; n_allele 0 = an empty ref."""
    out = {k: [] for k in VCF_KEYS}
    for r in rows:
        rid, ref, alt = vbw.row_id_ref_alt(r)
        out["chrom"].append(r["chrom"])
        out["pos"].append(r["pos"])
        if fmt == "bcf":
            alleles = r["alleles"] if "alleles" in r else [ref] + alt
            rid = r.get("id", "")
            out["id"].append([] if rid in ("", ".") else rid.split(";"))
            out["ref"].append(alleles[0] if alleles else "")
            out["alt"].append(list(alleles[1:]))
        else:
            out["id"].append(None if rid in ("", ".") else rid.split(";"))
            out["ref"].append(ref)
            out["alt"].append([] if alt else None)
    return out


SEQ = "ACGTNACGGTCA"


def read(i, ref=0, nulls="some", **kw):
    """a short alignment: 0-5 bases (period 7), a name of 1-6 bytes (period 5) or '*'"""
    n = (i * 3) % 7 % 6
    r = dict(name="*" if is_null(i, nulls) else "nmabcd"[:1 + i % 5] + "z"[:i % 2], flag=(i * 37) % 4096, ref=ref, pos=i + 1, mapq=i % 61,
             cigar=[(n, 0)] if n else [], seq=SEQ[i % 5:i % 5 + n], qual=[(i + 11 * j) % 94 for j in range(n)])
    r.update(kw)
    return r


def fastq_read(i, nulls="some"):
    """(name, what follows it on the header line, sequence, quality): a NULL description = no space, or a space and nothing"""
    n = (i * 3) % 7 % 6
    if is_null(i, nulls):
        tail = "" if i % 2 else " "
    else:
        tail = " " + ["d", "lane:1 x", "q  r"][i % 3]
    return ("rd" + "abcd"[:i % 5], tail, SEQ[i % 5:i % 5 + n], "".join(chr(33 + (i + 7 * j) % 94) for j in range(n)))


def fastq_expected(reads):
    out = {k: [] for k in FASTQ_KEYS}
    for name, tail, seq, qual in reads:
        out["name"].append(name)
        out["description"].append(tail[1:] if len(tail) > 1 else None)
        out["sequence"].append(seq)
        out["quality_scores"].append(qual)
    return out


# ---- writing a file of one format and reading it the three ways -----------------------------------------------------------------
class Case:
    def __init__(self, path, fmt, expected):
        self.path, self.fmt, self.expected = str(path), fmt, expected
        self.n = len(expected[KEYS[fmt][0]])


def write_case(d, name, kind, rows, eol=lambda i: "\n"):
    """kind: one of FORMATS; rows: variants (vcf, vcf.gz, bcf), reads (bam, sam) or fastq reads"""
    fmt = "vcf" if kind == "vcf.gz" else kind
    path = os.path.join(str(d), f"{name}.{kind}")
    if fmt == "vcf":
        plain = path + ".u" if kind == "vcf.gz" else path  # (the text of a BGZF file: <file>.u, as the BCF and BAM writers name it)
        vbw.write_vcf(plain, rows, filters=[], eol=eol)
        if kind == "vcf.gz":
            subprocess.check_call([BGZIP, plain, path, "6"], stdout=subprocess.DEVNULL)
        return Case(path, fmt, variant_expected(rows, fmt))
    if fmt == "bcf":
        vbw.write_bcf(path, rows, BGZIP, filters=[])
        return Case(path, fmt, variant_expected(rows, fmt))
    if fmt == "bam":
        bsw.write_bam(path, rows, BGZIP)
        return Case(path, fmt, bsw.expected(rows, sam=False))
    if fmt == "sam":
        bsw.write_sam(path, rows, eol=eol)
        return Case(path, fmt, bsw.expected(rows, sam=True))
    with open(path, "w", newline="") as f:
        for i, (name_, tail, seq, qual) in enumerate(rows):
            e = eol(i)
            f.write(f"@{name_}{tail}{e}{seq}{e}+{e}{qual}{e}")
    return Case(path, fmt, fastq_expected(rows))


def rows_of(kind, n, nulls="some"):
    if kind in ("vcf", "vcf.gz", "bcf"):
        return [variant(i, nulls=nulls) for i in range(n)]
    if kind in ("bam", "sam"):
        return [read(i, nulls=nulls) for i in range(n)]
    return [fastq_read(i, nulls=nulls) for i in range(n)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """files shared between the tests of one run: get(name, kind, make_rows) writes a case once"""
    d = tmp_path_factory.mktemp("text_limits")
    cache = {}

    def get(name, kind, make_rows, **kw):
        if (name, kind) not in cache:
            cache[name, kind] = write_case(d, name, kind, make_rows(), **kw)
        return cache[name, kind]
    return get


def read_scan(scan, keys):
    cols, sizes = {k: [] for k in keys}, []
    for b in scan:
        sizes.append(len(b))
        for i in range(b.type.num_fields):
            k = b.type.field(i).name
            if k in cols:
                cols[k].extend(b.field(i).to_pylist())
    return cols, sizes


def open_scan(case, **kw):
    if PROJECT[case.fmt]:
        kw["project"] = PROJECT[case.fmt]
    return exon_amd.Scan(case.path, case.fmt, **kw)


def assert_columns(got, want, keys, what):
    for k in keys:
        assert len(got[k]) == len(want[k]), f"{what}: {k}: {len(got[k])} rows instead of {len(want[k])}"
        if got[k] != want[k]:
            i = next(i for i, (g, w) in enumerate(zip(got[k], want[k])) if g != w)
            raise AssertionError(f"{what}: {k}, row {i}: {got[k][i]!r} instead of {want[k][i]!r}")


def oracle_columns(case):
    if case.fmt in ("vcf", "bcf"):
        v = (decode.decode_vcf if case.fmt == "vcf" else decode.decode_bcf)(case.path)
        return {k: v[k] for k in VCF_KEYS}
    if case.fmt == "fastq":
        recs = decode.decode_fastq(case.path)
        return {k: [r[k] for r in recs] for k in FASTQ_KEYS}
    refs, recs = (decode.decode_bam if case.fmt == "bam" else decode.decode_sam)(case.path)
    out = dict(flag=[r["flag"] for r in recs], start=[r["start"] for r in recs], cigar=[r["cigar"] for r in recs], sequence=[r["sequence"] for r in recs],
               reference=[None if r["ref_id"] is None else refs[r["ref_id"]][0] for r in recs])
    if case.fmt == "bam":
        out["name"] = [None if r["name"] == "*" else r["name"] for r in recs]
        out["quality_score"] = [[q - 256 if q > 127 else q for q in r["quality_score"]] for r in recs]
    else:
        out["name"] = [r["name_opt"] for r in recs]
        out["quality_score"] = [r["quality_score"] for r in recs]
    return out


def check_cpu(case, **kw):
    """host reader == expected, oracle/decode.py == expected"""
    keys = KEYS[case.fmt]
    s = open_scan(case, **kw)
    got, sizes = read_scan(s, keys)
    s.close()
    assert_columns(got, case.expected, keys, "host reader")
    assert_columns(oracle_columns(case), case.expected, keys, "oracle")
    return sizes


def check_gpu(ctx, case, on_gpu=True, expected=None, **kw):
    """GPU pipeline == expected; decoded_on_gpu()[0] as the case says"""
    keys = KEYS[case.fmt]
    s = open_scan(case, gpu_parse=True, **kw).bind_ctx(ctx)
    got, sizes = read_scan(s, keys)
    flag = s.decoded_on_gpu()[0]
    s.close()
    assert_columns(got, case.expected if expected is None else expected, keys, "GPU pipeline")
    assert bool(flag) == on_gpu, f"decoded on the GPU: {flag}, expected {on_gpu}"
    return sizes


# ---- 1. row counts on the kernels' borders ----------------------------------------------------------------------------------------
# 32, 64: the two ballot words a wave writes in k_*_measure; 256: LIST_TPB and list_first_item's cross-wave sum; 65 537 and 131 073:
# the first row counts at which k_list_scan_blocks adds 2 and 3 block sums per thread
ROW_COUNTS = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 65536, 65537, 131073]
BORDER_CASES = [(n, "some") for n in ROW_COUNTS] + [(65, "all"), (65, "none")]


def border_case(files, kind, n, nulls):
    return files(f"rows{n}{nulls}", kind, lambda: rows_of(kind, n, nulls))


@pytest.mark.parametrize("kind", FORMATS)
@pytest.mark.parametrize("n,nulls", BORDER_CASES)
def test_cpu_row_counts_on_the_borders(files, kind, n, nulls):
    case = border_case(files, kind, n, nulls)
    assert case.n == n
    check_cpu(case)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FORMATS)
@pytest.mark.parametrize("n,nulls", BORDER_CASES)
def test_gpu_row_counts_on_the_borders(ctx, files, kind, n, nulls):
    check_gpu(ctx, border_case(files, kind, n, nulls))


# ---- 2. cell values on the edges ------------------------------------------------------------------------------------------------
ID_EDGES = [".", "", "a", "a;b", ";", "a;", ";a", ";;;", "i" * 299 + ";"]
REF_EDGES = ["A", "ACGT" * 75]
ALT_EDGES = [None, ["C"], ["C", "G", "T", "AC", "GTT"]]
# BCF only: alleles of 0, 14, 15, 16 bytes (15 = the first count that takes the long descriptor) and 300 (a 2-byte count)
BCF_ALT_EDGES = ALT_EDGES + [[""], ["", ""], ["A" * 14], ["C" * 15], ["G" * 16, "", "T" * 300], ["N" * 300]]
N_EDGE = 317  # (a prime: every edge meets every other and many row positions)


def variant_edges(kind):
    rows = []
    for i in range(N_EDGE):
        alts = BCF_ALT_EDGES if kind == "bcf" else ALT_EDGES
        r = variant(i, chrom="1" if (i // 5) % 2 == 0 else "2", id=ID_EDGES[i % 9], ref=REF_EDGES[(i // 3) % 2], alt=alts[i % len(alts)])
        if kind == "bcf":
            if i % 9 == 0 and i % 2:
                del r["id"]  # the ID as an empty typed string instead of "."
            if i % 13 == 4:
                r["alleles"] = []  # n_allele 0
            if i % 13 == 9:
                r["alleles"] = [r["ref"]]  # n_allele 1
        rows.append(r)
    return rows


def vcf_edge_eol(i):
    return "" if i == N_EDGE - 1 else "\r\n" if i % 5 == 2 else "\n"  # a CR before the LF; the last line without LF


CIGAR_EDGES = [[], [(0, 0)], [(9, 1)], [(10, 2)], [(99999999, 3)], [(100000000, 4)], [(268435455, 5)], [(1, 6), (12, 7), (123, 8)],
               [(5, 9)], [(6, 10), (7, 11), (8, 12)], [(99, 13), (100, 14), (999999, 15)], [(1000, 0), (0, 8), (268435455, 8), (10000000, 1)]]
NAME_EDGES = ["", "*", "a", "abcdefg", "abcdefgh", "abcdefghi", "n" * 254, "**"]
SEQ_EDGES = ["", "A", bsw.BASES, bsw.BASES[:15], bsw.BASES[::-1], bsw.BASES[3:] + bsw.BASES[:4], "NN=", "ACGTACG", "ACGTACGT", "ACGTACGTA"]
QUAL_BYTES = [0x00, 0x7F, 0x80, 0xFF, 0x21, 0x5D, 0x01, 0xFE]


def bam_edges():
    recs = []
    for i in range(N_EDGE):
        seq = SEQ_EDGES[i % 10]
        recs.append(read(i, ref=(i // 5) % 2, name=NAME_EDGES[i % 8], cigar=CIGAR_EDGES[i % 12], seq=seq,
                         qual=[QUAL_BYTES[(i + j) % 8] for j in range(len(seq))]))
    return recs


SAM_CIGARS = [[], [(1, 0)], [(10, 0), (2, 1), (3, 2)], [(10, 0), (2, 1), (30, 2)], [(10, 0), (20, 1), (30, 2)], [(268435455, 3), (1, 8)],
              [(1, 4), (2, 5), (3, 6), (4, 7), (5, 8)]]  # "10M2I3D", "10M2I30D", "10M20I30D": 7, 8 and 9 bytes (copy_run moves 8 at a time)
SAM_NAMES = ["*", "a", "abcdefg", "abcdefgh", "abcdefghi", "**"]
SAM_SEQS = ["", "A", "ACGTACG", "ACGTACGT", "ACGTACGTA", "acgtnACGTN=.", "NNNNNNNNNNNNNNNNN"]


def sam_edges():
    recs = []
    for i in range(N_EDGE):
        seq = SAM_SEQS[i % 7]
        r = read(i, ref=(i // 5) % 2, name=SAM_NAMES[i % 6], cigar=SAM_CIGARS[i % 5 + (i % 3 == 0) * 2], seq=seq,
                 qual=[(0, 93, 1, 92, 40)[(i + j) % 5] for j in range(len(seq))])
        if seq and i % 4 == 1:
            r["qual_text"] = "*"  # QUAL '*' beside a SEQ
        elif seq and i % 4 == 2:
            r["qual_text"] = ("!" if i % 8 == 2 else "~") * len(seq)
        recs.append(r)
    return recs


def fastq_edges():
    reads = []
    names = ["", "r", "read7ab", "read8abc", "read9abcd"]
    tails = ["", " ", "  ", " d", "  two", " a b  c ", " 1234567", " 12345678"]  # no space; a space and nothing; two spaces; ...
    lens = [0, 7, 8, 9, 1, 17]
    for i in range(N_EDGE):
        n = lens[i % 6]
        reads.append((names[i % 5], tails[i % 8], (SEQ * 2)[i % 3:i % 3 + n], "".join(chr(33 + (i * 5 + 31 * j) % 94) for j in range(n))))
    return reads


def edge_case(files, kind):
    if kind in ("vcf", "vcf.gz"):
        return files("edges", kind, lambda: variant_edges(kind), eol=vcf_edge_eol)
    if kind == "bcf":
        return files("edges", kind, lambda: variant_edges(kind))
    if kind == "bam":
        return files("edges", kind, bam_edges)
    if kind == "sam":
        return files("edges", kind, sam_edges, eol=lambda i: "\r\n" if i % 5 == 2 else "\n")
    return files("edges", kind, fastq_edges, eol=lambda i: "\r\n" if i % 5 == 2 else "\n")


@pytest.mark.parametrize("kind", FORMATS)
def test_cpu_cell_values_on_the_edges(files, kind):
    check_cpu(edge_case(files, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FORMATS)
def test_gpu_cell_values_on_the_edges(ctx, files, kind):
    check_gpu(ctx, edge_case(files, kind), batch_size=100)


def test_the_edge_files_hold_every_edge(files):
    """the writers put on disk what the cases name (a check of the inputs, independent of every reader)"""
    raw = decode.read_bytes(edge_case(files, "bcf").path)
    for count in (14, 15, 16):
        desc = bytes([(count << 4) | 7]) if count < 15 else b"\xf7\x11" + bytes([count])
        assert desc + (b"A" * 14 if count == 14 else b"C" * 15 if count == 15 else b"G" * 16) in raw
    assert b"\xf7\x12\x2c\x01" + b"N" * 300 in raw  # 300 characters: the count as an int16
    raw = decode.read_bytes(edge_case(files, "bam").path)
    assert b"\xf5\xff\xff\xff" in raw  # 2^28 - 1 of op 5, low byte first
    assert b"\x59\x00\x00\x00" in raw and b"\xff\x23\xf4\x00" in raw  # 5 of op 9; 999 999 of op 15
    text = open(edge_case(files, "vcf").path, newline="").read()
    assert "\t\tA\t" in text and "\r\n" in text and not text.endswith("\n")


SAM_HANDED_OVER = {  # a line the device must hand over -> what the host reader answers (None: its error)
    "leading_zero_op_count": (dict(cigar_text="03M2I"), dict(cigar="3M2I")),
    "op_of_length_zero": (dict(cigar_text="0M3M"), dict(cigar="0M3M")),  # (printed as it is; the device takes any leading 0 for one the printer drops)
    "unknown_op_letter": (dict(cigar_text="3Q"), None),
    "trailing_digits": (dict(cigar_text="3M2"), None),
    "qual_byte_32": (dict(qual_text="!! "), None),
    "qual_byte_127": (dict(qual_text="!!\x7f"), None),
    "ten_fields": (dict(drop_qual=True), None),
}


def sam_handed_over_case(tmp_path, which):
    change, answer = SAM_HANDED_OVER[which]
    recs = [read(i, name=f"n{i}", cigar=[(3, 0)], seq="ACG", qual=[0, 1, 93]) for i in range(40)]
    want = bsw.expected(recs, sam=True)
    lines = [bsw.sam_line(r) for r in recs]
    k = 33  # (in the second 32-row word)
    if change.get("drop_qual"):
        lines[k] = lines[k].rsplit("\t", 1)[0]
    else:
        lines[k] = bsw.sam_line(dict(recs[k], **change))
    if answer:
        for key, v in answer.items():
            want[key][k] = v
    path = tmp_path / f"{which}.sam"
    path.write_text("@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in bsw.REFS) + "\n".join(lines) + "\n")
    return Case(path, "sam", want), answer is not None


@pytest.mark.parametrize("which", list(SAM_HANDED_OVER))
def test_cpu_sam_rows_the_device_hands_over(tmp_path, which):
    case, answers = sam_handed_over_case(tmp_path, which)
    if answers:
        s = open_scan(case)
        got, _ = read_scan(s, BAM_KEYS)
        s.close()
        assert_columns(got, case.expected, BAM_KEYS, "host reader")
    else:
        with pytest.raises(exon_amd.ExonHipError):
            read_scan(open_scan(case), BAM_KEYS)


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(SAM_HANDED_OVER))
def test_gpu_sam_rows_the_device_hands_over(ctx, tmp_path, which):
    case, answers = sam_handed_over_case(tmp_path, which)
    s = open_scan(case, gpu_parse=True).bind_ctx(ctx)
    if answers:
        got, _ = read_scan(s, BAM_KEYS)
        assert_columns(got, case.expected, BAM_KEYS, "GPU pipeline")
    else:
        with pytest.raises(exon_amd.ExonHipError):
            read_scan(s, BAM_KEYS)
    assert not s.decoded_on_gpu()[0]
    s.close()


# ---- 3. the scratch capacities ----------------------------------------------------------------------------------------------------
# A slab of up to 1 MiB and 65 536 rows gets item-offset buffers of 2^20 / 2 + 65 536 + 64 + 2 = 589 890 entries (an entry per
# item and one that closes the last) and value buffers of 1 MiB (BAM: 2 * n_bytes, so the same up to 512 KiB of records).  The
# fix chosen compares the totals with these capacities on the host before the fill kernel is launched: a slab that fits is
# built on the device (decoded_on_gpu), one that does not goes to the host reader (not decoded_on_gpu) -- at every size the
# answer is the expectation.
ITEM_CAP = (1 << 19) + (1 << 16) + 64 + 2
VALUE_CAP = 1 << 20


def rows_with_items(total, per_row):
    """how many rows of per_row items, and the items of one last row, that make `total` items"""
    full, rest = divmod(total, per_row)
    return [per_row] * full + ([rest] if rest else [])


def capacity_rows(what, total):
    if what in ("vcf_id", "bcf_id"):  # an ID of k semicolons is k + 1 items in k bytes
        return [variant(i, id=";" * (k - 1)) for i, k in enumerate(rows_with_items(total, 1001))]
    if what == "bcf_alt":  # an empty allele is the single byte 0x07
        return [variant(i, alleles=["A"] + [""] * k) for i, k in enumerate(rows_with_items(total, 60000))]
    # bam_cigar: an op of length 100 000 000 prints as ten characters; the last record tops up with "1M" (two) and "10M" (three)
    recs = []
    for i, chars in enumerate(rows_with_items(total, 600000)):
        ops = [(100000000, 0)] * (chars // 10)
        rest = chars % 10
        if rest == 1:  # (no op prints as one character: take a long op back)
            ops.pop()
            rest = 11
        ops += [(10, 0)] * (rest % 2) + [(1, 0)] * ((rest - 3 * (rest % 2)) // 2)
        recs.append(read(i, name=f"c{i}", cigar=ops, seq="", qual=[]))
        assert sum(len(f"{n}M") for n, _ in ops) == chars
    return recs


# item-offset entries (the items and the closing one): ITEM_CAP + at, at 0 = the most that fits, 1 = the first that does not; CIGAR
# bytes: VALUE_CAP + at, 65 = the first total that was written past the old allocation of max_bytes + 64, 66 = just above it
CAPACITY = [(what, at) for what in ("vcf_id", "bcf_id", "bcf_alt") for at in (0, 1, 2)] + [("bam_cigar", at) for at in (0, 1, 65, 66)]


def capacity_case(files, what, at):
    kind = {"vcf_id": "vcf", "bcf_id": "bcf", "bcf_alt": "bcf", "bam_cigar": "bam"}[what]
    total = VALUE_CAP + at if what == "bam_cigar" else ITEM_CAP + at
    case = files(f"cap_{what}_{at}", kind, lambda: capacity_rows(what, total if what == "bam_cigar" else total - 1))
    assert os.path.getsize(case.path + ".u" if kind != "vcf" else case.path) < (1 << 19 if kind == "bam" else 1 << 20)
    if what == "bam_cigar":
        assert sum(len(c) for c in case.expected["cigar"]) == total
    else:
        col = "alt" if what == "bcf_alt" else "id"
        assert sum(len(v) for v in case.expected[col] if v) + 1 == total  # the entries the item offsets take
    fits = total <= (VALUE_CAP if what == "bam_cigar" else ITEM_CAP)
    return case, fits


@pytest.mark.parametrize("what,at", CAPACITY)
def test_cpu_totals_around_the_scratch_capacities(files, what, at):
    check_cpu(capacity_case(files, what, at)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("what,at", CAPACITY)
def test_gpu_totals_around_the_scratch_capacities(ctx, files, what, at):
    case, fits = capacity_case(files, what, at)
    check_gpu(ctx, case, on_gpu=fits)


# With EXON_HIP_GPU_PARSE_SLAB_MB=1 the first BGZF slab is 64 blocks of 65 280 bytes, 4.18 MB of text, and the later ones 64 to 96
# blocks (plain text cannot show this case: its first slab carries what the host reader had buffered in front of the first MiB,
# its later slabs are 1 MiB, and the scratch of the larger first slab -- kept for the scan -- holds any total 1 MiB can produce).
# The scratch after the first slab holds 4.18e6 / 2 + 65 602 = 2.15 M item entries and 2 * 4.18e6 = 8.4 M CIGAR characters; the rows
# behind it, 2.7 and 3.8 MB that fit one slab of either size, make 2.6 M items (VCF ids of 1000 ';' each) and 9.5 M characters (BAM
# CIGARs of 1000 ten-character ops).
def later_slab_rows(kind):
    """normal rows for a little more than the first slab, then rows the second slab's buffers do not hold"""
    if kind == "vcf.gz":
        return [variant(i, info={"CSQ": "x" * 600}) for i in range(6800)] + [variant(6800 + i, id=";" * 1000) for i in range(2600)]
    return ([read(i, name="n" * 60, cigar=[(1, 0)] * 1000, seq="ACGT", qual=[30] * 4) for i in range(1050)]
            + [read(1050 + i, cigar=[(100000000, 0)] * 1000, seq="", qual=[]) for i in range(950)])


LATER_SLAB_KINDS = ["vcf.gz", "bam"]


@pytest.mark.parametrize("kind", LATER_SLAB_KINDS)
def test_cpu_totals_beyond_the_capacities_in_a_later_slab(files, kind):
    case = files("later_slab", kind, lambda: later_slab_rows(kind))
    check_cpu(case)
    text = case.path + ".u"
    assert 4.25e6 + (2.6e6 if kind == "vcf.gz" else 3.8e6) < os.path.getsize(text) < 8 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LATER_SLAB_KINDS)
def test_gpu_totals_beyond_the_capacities_in_a_later_slab(ctx, files, monkeypatch, kind):
    """the first slab is built on the device and sent, the second holds more items (VCF) or CIGAR text (BAM) than the scratch:
    the host reader continues behind the rows already sent -- none lost, none doubled -- and the scan says so"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    case = files("later_slab", kind, lambda: later_slab_rows(kind))
    sizes = check_gpu(ctx, case, on_gpu=False, batch_size=1 << 20)
    assert len(sizes) >= 2 and sizes[0] < case.n  # (batches end with their slab: the first came from the device)


# ---- 4. batch cuts --------------------------------------------------------------------------------------------------------------
# 37 starts batches at every bit of a validity byte; 65 000 | 65 001: K_ZERO_ROWS, the static or the slab-wide zero offsets of VCF alt
BATCH_SIZES = [1, 7, 37, 64, 65000, 65001]


def batch_case(files, kind, bs):
    n = 300 if bs == 1 else 70000  # (one row a batch: 300 rows, to stay within time)
    return files(f"rows{n}some", kind, lambda: rows_of(kind, n))


@pytest.mark.parametrize("kind", FORMATS)
def test_cpu_batch_cuts(files, kind):
    for bs in (1, 65000):
        case = batch_case(files, kind, bs)
        sizes = check_cpu(case, batch_size=bs)
        assert sum(sizes) == case.n and max(sizes) <= bs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FORMATS)
@pytest.mark.parametrize("bs", BATCH_SIZES)
def test_gpu_batch_cuts(ctx, files, kind, bs):
    case = batch_case(files, kind, bs)
    h = open_scan(case, batch_size=bs)
    want_sizes = [len(b) for b in h]
    h.close()
    sizes = check_gpu(ctx, case, batch_size=bs)
    assert sizes == want_sizes


# ---- 5. slab cuts and scratch reuse ---------------------------------------------------------------------------------------------
FIRST_BGZF_SLAB = 64 * 65280  # the text of the first BGZF slab: 64 blocks of tools/bin/bgzip (later slabs: up to 96)


def irregular_rows(kind):
    """rows whose lengths follow no period a slab end could lock on: about 3 MB of text (1 MiB slabs), about 5 MB behind BGZF
    (the first slab ends at FIRST_BGZF_SLAB).  One BAM read in 40 carries a CIGAR of 2000 ops: the fill kernel of such a slab is
    still running when the host goes on to the next slabs, whose inflate must not land in the text it reads"""
    def ln(i, m):
        return (i * i * 31 + i * 7) % m
    if kind in ("vcf", "vcf.gz"):
        return [variant(i, id="." if is_null(i) else ";".join("r" * (1 + ln(i + k, 23)) for k in range(1 + i % 3)), ref="ACGT" * ln(i, 41) + "A",
                        alt=None if is_null(i + 5) else ["G" * (1 + ln(i, 29))]) for i in range(22000 if kind == "vcf" else 38000)]
    if kind == "bcf":
        return [variant(i, id="." if is_null(i) else ";".join("r" * (1 + ln(i + k, 23)) for k in range(1 + i % 3)), ref="ACGT" * ln(i, 41) + "A",
                        alt=[c * ln(i + k, 37) for k, c in enumerate("GTC"[:i % 4])]) for i in range(31000)]
    if kind in ("bam", "sam"):
        recs = []
        for i in range(13000):
            n = ln(i, 211)
            cigar = [(n, 0), (1 + ln(i, 5000), 3), (7, 4)] if n else []
            if kind == "bam" and i % 40 == 7:
                cigar = [(1 + (i + k) % 9, k % 9) for k in range(2000)]
            recs.append(read(i, name="*" if is_null(i) else "q" * (1 + ln(i, 47)), cigar=cigar,
                             seq=(SEQ * 18)[i % 7:i % 7 + n], qual=[(i + 3 * j) % 94 for j in range(n)]))
        return recs
    return [("f" * (1 + ln(i, 19)), "" if is_null(i) else " " + "d" * ln(i, 31), (SEQ * 20)[i % 5:i % 5 + ln(i, 173)],
             "".join(chr(33 + (i + j) % 94) for j in range(ln(i, 173)))) for i in range(16000)]


def id_in_one_half_rows(kind, first):
    """40 000 rows of about 150 bytes.  ids_first: the first 20 000 carry ids (BCF: and alt items), the rest none -- every slab
    behind the first (2 MiB of VCF text, FIRST_BGZF_SLAB of BCF) has none.  ids_last: the first 31 500 rows, more than the first
    slab of either kind, have none, the rest carry them"""
    def row(i, full):
        if kind == "bcf":
            return variant(i, id="a;b;c" if full else ".", alt=["C", "GG"] if full else None, info={"CSQ": "y" * 100})
        return variant(i, id="a;b;c" if full else ".", info={"CSQ": "y" * 100})
    return [row(i, i < 20000 if first else i >= 31500) for i in range(40000)]


SLAB_CASES = [(kind, "irregular") for kind in FORMATS] + [(kind, which) for kind in ("vcf", "bcf") for which in ("ids_first", "ids_last")]


def slab_case(files, kind, which):
    if which == "irregular":
        return files("irregular", kind, lambda: irregular_rows(kind))
    return files(which, kind, lambda: id_in_one_half_rows(kind, which == "ids_first"))


@pytest.mark.parametrize("kind,which", SLAB_CASES)
def test_cpu_slab_cut_files(files, kind, which):
    case = slab_case(files, kind, which)
    check_cpu(case)
    raw = case.path + ".u" if kind in ("vcf.gz", "bcf", "bam") else case.path
    least = FIRST_BGZF_SLAB + (400 << 10) if kind in ("vcf.gz", "bcf", "bam") else 2 << 20
    assert least < os.path.getsize(raw) < 8 << 20
    if which == "ids_last":  # the rows without ids reach beyond the first slab
        head = vbw.header_text(kind == "bcf", [])
        first = FIRST_BGZF_SLAB if kind == "bcf" else 2 << 20  # (the rows with ids are the longer ones: an underestimate)
        assert 31500 * (os.path.getsize(raw) - len(head)) // 40000 > first + (100 << 10)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,which", SLAB_CASES)
def test_gpu_slab_cuts_and_scratch_reuse(ctx, files, monkeypatch, kind, which):
    """slabs end anywhere in rows of irregular length; a slab without any id (alt item) behind one full of them, and the reverse:
    item_off[0] of the item-less slab is cleared although the slab before left data there.  Batches end with their slab: a
    batch size beyond the row count shows that the file came in several slabs"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    case = slab_case(files, kind, which)
    sizes = check_gpu(ctx, case, batch_size=1 << 20)
    assert len(sizes) >= 2 and sum(sizes) == case.n, sizes


# ---- 6. the gather ----------------------------------------------------------------------------------------------------------------
def region_filter(case, region_name):
    """the rows a region over a whole contig / reference keeps.  VCF / BCF: those of the contig.  BAM / SAM (SemiLazyRecord::
    intersects): a mapped read of the reference that ends at or behind position 1"""
    e = case.expected
    if case.fmt in ("vcf", "bcf"):
        keep = [c == region_name for c in e["chrom"]]
    else:
        keep = [r == region_name and s is not None and en >= 1 for r, s, en in zip(e["reference"], e["start"], e["end"])]
    return {k: [v for v, kp in zip(e[k], keep) if kp] for k in KEYS[case.fmt]}


def alternating_rows(kind, n=600):
    """rows alternate in and out of the region: about n / 2 kept runs of one row, more than MAX_RUNS (256)"""
    if kind in ("vcf", "vcf.gz", "bcf"):
        return [variant(i, chrom="1" if i % 2 == 0 else "2") for i in range(n)]
    return [read(i, ref=i % 2, cigar=[(1 + i % 5, 0)], seq=SEQ[:1 + i % 5], qual=[(i + j) % 94 for j in range(1 + i % 5)]) for i in range(n)]


def blocks_rows(kind, n=257):
    """a border file of case 1 whose rows change contig / reference every 5 rows: some fifty kept runs"""
    if kind in ("vcf", "vcf.gz", "bcf"):
        return [variant(i, chrom="1" if (i // 5) % 2 == 0 else "2") for i in range(n)]
    return [read(i, ref=(i // 5) % 2, cigar=[(2, 0)], seq="AC", qual=[i % 94, 3]) for i in range(n)]


REGION = {"vcf": "1", "vcf.gz": "1", "bcf": "1", "bam": "r1", "sam": "r1"}
GATHER_KINDS = ["vcf", "vcf.gz", "bcf", "bam", "sam"]


def gather_case(files, kind, which):
    if which == "edges":
        return edge_case(files, kind)
    return files(which, kind, lambda: (alternating_rows if which == "alternating" else blocks_rows)(kind))


@pytest.mark.parametrize("kind", GATHER_KINDS)
@pytest.mark.parametrize("which", ["edges", "blocks", "alternating"])
def test_cpu_region_files(files, kind, which):
    """the host reader under the region == the expectation filtered here (the files themselves: cases 1 and 2, and below)"""
    case = gather_case(files, kind, which)
    if which != "edges":
        check_cpu(case)
    want = region_filter(case, REGION[kind])
    s = open_scan(case, region=REGION[kind])
    got, _ = read_scan(s, KEYS[case.fmt])
    s.close()
    assert_columns(got, want, KEYS[case.fmt], "host reader under a region")
    assert 0 < len(want[KEYS[case.fmt][0]]) < case.n


@pytest.mark.gpu
@pytest.mark.parametrize("kind", GATHER_KINDS)
@pytest.mark.parametrize("which", ["edges", "blocks"])
@pytest.mark.parametrize("forced", ["0", "1"])
def test_gpu_region_as_views_and_through_the_forced_gather(ctx, files, monkeypatch, kind, which, forced):
    """EXON_HIP_EXPORT_GATHER is read for every slab's export: 0 = the kept runs as views, 1 = the row-by-row gather"""
    monkeypatch.setenv("EXON_HIP_EXPORT_GATHER", forced)
    case = gather_case(files, kind, which)
    check_gpu(ctx, case, expected=region_filter(case, REGION[kind]), region=REGION[kind], batch_size=16)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", GATHER_KINDS)
def test_gpu_region_with_more_kept_runs_than_views_take(ctx, files, monkeypatch, kind):
    """no switch: 300 kept runs in one slab are more than MAX_RUNS, the export gathers row by row on its own"""
    monkeypatch.delenv("EXON_HIP_EXPORT_GATHER", raising=False)
    case = gather_case(files, kind, "alternating")
    want = region_filter(case, REGION[kind])
    assert len(want[KEYS[case.fmt][0]]) == 300
    check_gpu(ctx, case, expected=want, region=REGION[kind], batch_size=64)
