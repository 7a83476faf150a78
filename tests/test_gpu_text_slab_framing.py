"""GPU: how scan.cpp's GpuTextSource frames a text file for the device parsers -- slabs cut at a fixed byte count, the unconsumed tail
carried in front of the next slab, the missing terminator of the last line appended -- with the cut put on a chosen byte of a record
and the input ended in every way it can end.  Slabs are 1 MiB (EXON_HIP_GPU_PARSE_SLAB_MB=1, EXON_HIP_GZ_SLAB_MB=1).

Every case compares all projected columns of Scan(..., gpu_parse=True).bind_ctx(ctx) with the host reader's and with what the rows
were written to hold (tests/line_index_expect.py numbers them in POS / start), requires decoded_on_gpu()[0], and -- on plain text --
three slabs or more.

WHERE THE CUTS ARE (plain text; read from the code and observed on the device).  A slab takes 1 MiB of fresh bytes behind what is
carried.  The host reader that opens a VCF, SAM or FASTA file has buffered its first MiB (the header, the first line, the '>'), and
that buffer goes in front of the first slab: their first slab ends at byte 2 MiB of the FILE, the next at 3 MiB.  FASTQ, GFF and BED
readers have read nothing: 1, 2, 3 MiB.  So byte 2 MiB is a cut for every format (not "k * 2^20 shifted by the header": the header is
part of the buffered MiB), and the files here are 3.2 MiB, not 2.2, so that VCF, SAM and FASTA have three slabs too.  With one
batch a slab (batch_size beyond any slab) the batch sizes say where each slab ended, and every case asserts them against the rows
that end in front of 2 MiB and 3 MiB: a case whose cut is not where it was meant to be fails.

WHAT THE CASES FOUND.  An input whose last byte is a CR without its LF: the slab reader appended the missing '\n' behind it, the
parsers then dropped the CR as part of a "\r\n", and the last field came out one byte shorter than the host reader's (which, like
the reference, takes only '\n' and "\r\n" for terminators).  GpuTextSource now hands such an input to the host reader (plain, gzip
and BGZF alike); test_the_end_of_the_input pins the hand-over and the byte.
A row longer than a slab is not the host reader's by its length alone: it is handed over when no slab holds a whole record (the row
starts within the last bytes of a slab), and decoded on the device when the carried tail and the fresh MiB hold it together --
test_vcf_a_line_longer_than_a_slab pins both.

BGZF slabs are cut by member count (64 members at the least) and plain-gzip slabs by what the DEFLATE blocks allow, so the compressed
twins of the end-of-input cases do not control their cuts; they are here for the terminator each of those paths appends itself."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import fasta_expect
import line_index_expect as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
MIB = 1 << 20
CUT = 2 * MIB
W = 160  # lines are W .. 2 W bytes
FIRST_CUT = {"vcf": 2, "sam": 2, "fasta": 2, "fastq": 1, "gff": 1, "bed": 1}  # MiB of the file in the first slab
PROJECT = {"vcf": ("id", "ref", "alt", "info"), "sam": ("name", "cigar", "sequence", "quality_score"), "gff": ("attributes",),
           "bed": ("name", "score"), "fasta": (), "fastq": ()}
EXT = {"vcf": "vcf", "sam": "sam", "gff": "gff", "bed": "bed", "fasta": "fasta", "fastq": "fastq"}
ONE_BATCH = 1 << 24


@pytest.fixture(autouse=True)
def small_slabs(monkeypatch):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    monkeypatch.setenv("EXON_HIP_GZ_SLAB_MB", "1")


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def head_of(fmt):
    return E.VCF_HEADER if fmt == "vcf" else b""


def positions(n_text, line_start, group=1):
    """newline positions of lines of W .. 2 W bytes in a text of about n_text bytes, one of the lines starting at line_start (its
    number comes back too); the number of lines is a multiple of `group`"""
    pos, at = [], 0
    while at + 2 * W <= line_start:
        pos.append(at + W - 1)
        at += W
    if at < line_start:
        pos.append(line_start - 1)
    at = line_start
    k = len(pos)
    while at + W <= n_text:
        pos.append(at + W - 1)
        at += W
    while len(pos) % group:
        pos.pop()
    return pos, k


def write_file(tmp_path, fmt, line_start_in_file, n_file=3 * MIB + MIB // 5, crlf_before=False):
    """A file of about n_file bytes one of whose lines starts at byte line_start_in_file; crlf_before: the line in front of it ends
    in CR LF.  -> path, text, newline positions in the file, the line's number"""
    head = head_of(fmt)
    pos, k = positions(n_file - len(head), line_start_in_file - len(head))
    text = E.with_newlines_at(pos[-1] + 1, pos, fmt, crlf=(k - 1,) if crlf_before else ())
    path = tmp_path / ("t." + EXT[fmt])
    path.write_bytes(head + text)
    return path, text, np.asarray(pos) + len(head), k


def compressed(tmp_path, path, kind):
    if kind == "gzip":
        q = tmp_path / (path.name + ".gz")
        q.write_bytes(gzip.compress(path.read_bytes(), 6))
        return q
    if kind == "bgzf":
        q = tmp_path / ("bgzf." + path.name + ".gz")
        subprocess.check_call([BGZIP, str(path), str(q), "6"], stdout=subprocess.DEVNULL)
        return q
    return path


# ---- scans ----------------------------------------------------------------------------------------------------------------------------
def read(scan):
    """(columns by name, batch sizes, decoded_on_gpu(), export_stats()) of a scan, which is closed"""
    try:
        names = [f.name for f in scan.schema()]
        batches = list(scan)
        for b in batches:
            b.validate(full=True)
        cols = {name: [v for b in batches for v in b.field(k).to_pylist()] for k, name in enumerate(names)}
        return cols, [len(b) for b in batches], scan.decoded_on_gpu(), scan.export_stats()
    finally:
        scan.close()


def both(ctx, path, fmt):
    """the GPU pipeline's columns (one batch a slab) after they were found equal to the host reader's"""
    got, sizes, flags, stats = read(exon_amd.Scan(str(path), fmt, gpu_parse=True, batch_size=ONE_BATCH, project=PROJECT[fmt]).bind_ctx(ctx))
    want = read(exon_amd.Scan(str(path), fmt, batch_size=ONE_BATCH, project=PROJECT[fmt]))[0]
    assert got.keys() == want.keys()
    for name in got:
        assert got[name] == want[name], name
    return got, sizes, flags, stats


def raw_lines(text):
    begin, end, end_nocr = E.lines(text)
    return [text[b:e] for b, e in zip(begin.tolist(), end_nocr.tolist())]


def check_columns(fmt, got, text, last_cr=False):
    """the columns against what the rows were written to hold.  last_cr (VCF, FASTQ): the input ends in a CR without its LF, which
    is a byte of the last field -- `text` is that input with the LF"""
    raw = raw_lines(text)
    n = len(raw)
    cr = lambda values: values[:-1] + [values[-1] + "\r"] if last_cr else values
    if fmt == "fasta":
        assert got == fasta_expect.columns(text)
        return len(got["id"])
    if fmt == "fastq":
        v = E.fastq_views(text, True)
        assert v["n_undecided"] == 0 and v["consumed"] == E.consumed(text)
        cut = lambda a, b: [text[x:y].decode() for x, y in zip(v[a].tolist(), v[b].tolist())]
        heads = cut("head_start", "head_end")
        assert got["name"] == [h.split(" ", 1)[0] for h in heads]
        assert got["description"] == [h.split(" ", 1)[1] if " " in h and h.split(" ", 1)[1] else None for h in heads]
        assert got["sequence"] == cut("seq_start", "seq_end") and got["quality_scores"] == cr(cut("qual_start", "qual_end"))
        return v["n_reads"]
    col = {"vcf": "pos", "sam": "start", "gff": "start", "bed": "start"}[fmt]
    assert got[col] == list(range(1, n + 1))
    last = [r.rsplit(b"\t", 1)[1].decode() for r in raw]
    if fmt == "vcf":
        assert got["info"] == cr([{".": "", "FL": "FL=true"}.get(x, x) for x in last])
        assert got["ref"] == ["A"] * n and got["chrom"] == ["1"] * n
    elif fmt == "sam":
        assert got["name"] == [r.split(b"\t", 1)[0].decode() for r in raw] and got["flag"] == [0] * n
    elif fmt == "gff":
        assert got["attributes"] == [[("a", [x[2:]])] for x in last] and got["end"] == list(range(10, n + 10))
    else:
        assert got["name"] == [r.split(b"\t")[3].decode() for r in raw] and got["end"] == list(range(10, n + 10))
    return n


def slab_sizes(fmt, nl_file, text, n_file):
    """the rows every slab emits when the slabs end at FIRST_CUT, FIRST_CUT + 1, ... MiB of the file"""
    cuts = [c * MIB for c in range(FIRST_CUT[fmt], n_file // MIB + 1) if c * MIB < n_file]
    if fmt == "fasta":  # a slab that is not the last keeps its last record back, whole or not
        a = np.frombuffer(text, np.uint8)
        begin = E.lines(text)[0]
        def_nl = nl_file[a[begin] == ord(">")]
        done = [int((def_nl < c).sum()) - 1 for c in cuts] + [len(def_nl)]
    else:
        per = 4 if fmt == "fastq" else 1
        whole = nl_file[per - 1::per]  # the newline that ends a record
        done = [int((whole < c).sum()) for c in cuts] + [len(whole)]
    return np.diff([0] + done).tolist()


def run_case(ctx, tmp_path, fmt, line_start, **kw):
    path, text, nl_file, k = write_file(tmp_path, fmt, line_start, **kw)
    n_file = os.path.getsize(path)
    assert n_file > 3 * MIB and path.read_bytes()[line_start - 1:line_start] == b"\n"  # the line starts where the case wants it
    got, sizes, flags, stats = both(ctx, path, fmt)
    assert flags == (True, False), "a hand-over to the host reader: the device path is not tested by this run"
    n = check_columns(fmt, got, text)
    assert sum(sizes) == n
    assert stats["slabs"] >= 3
    assert sizes == slab_sizes(fmt, nl_file, text, n_file), "the slabs were not cut where this case puts its record"
    return path, text, nl_file, k


# ---- a cut at a chosen byte of a record --------------------------------------------------------------------------------------------------
D = [-17, -16, -15, -2, -1, 0, 1, 2, 15, 16, 17]
CASES = [(d, False) for d in D] + [(-2, True), (-1, True), (0, True)]  # (-1, True): the cut between a CR and its LF


@pytest.mark.parametrize("d,crlf", CASES)
@pytest.mark.parametrize("fmt", ["vcf", "sam", "bed", "gff"])
def test_the_cut_d_bytes_from_a_line_start(ctx, tmp_path, fmt, d, crlf):
    """d > 0: the first slab ends d bytes into a row; d < 0: -d bytes in front of the row's end -- -1 directly in front of the
    newline, 0 directly behind it"""
    run_case(ctx, tmp_path, fmt, CUT - d, crlf_before=crlf)


@pytest.mark.parametrize("inside", [True, False])
@pytest.mark.parametrize("j", [0, 1, 2, 3])
def test_fastq_the_cut_in_every_line_and_behind_every_newline(ctx, tmp_path, j, inside):
    """inside: 5 bytes into line j of a record; else directly behind line j's newline.  Beside the batches, the quality histogram
    through the fused plan (the views go to K5 without a copy)."""
    # lines of W bytes up to line k - 1, which is as long as it takes to start line k, the chosen line of its record, on the cut
    k = (CUT // W - 8) // 4 * 4 + (j if inside else j + 1)
    line_start = CUT - 5 if inside else CUT
    head_lines = k - 1  # lines of W bytes, then one line up to line_start
    assert W <= line_start - head_lines * W < 16 * W
    pos = [W * (i + 1) - 1 for i in range(head_lines)] + [line_start - 1]
    at = line_start
    while at + W <= 3 * MIB + MIB // 5:
        pos.append(at + W - 1)
        at += W
    while len(pos) % 4:
        pos.pop()
    text = E.with_newlines_at(pos[-1] + 1, pos, "fastq")
    assert text[line_start - 1:line_start] == b"\n"
    assert len(E.newlines(text[:line_start])) % 4 == (j if inside else (j + 1) % 4)
    path = tmp_path / "t.fastq"
    path.write_bytes(text)
    got, sizes, flags, stats = both(ctx, path, "fastq")
    assert flags == (True, False) and stats["slabs"] >= 3
    n = check_columns("fastq", got, text)
    assert sum(sizes) == n and sizes == slab_sizes("fastq", np.asarray(pos), text, len(text))
    hists = []
    for gpu_parse in (True, False):
        scan = exon_amd.Scan(str(path), "fastq", gpu_parse=gpu_parse)
        plan = ctx.plan_qual_pos_hist(16 * W, columns=(3,))
        st = plan.open()
        try:
            rows = st.consume(scan)
            counts, _ = st.finish()
            assert scan.decoded_on_gpu()[0] == gpu_parse and rows == n
            hists.append(np.array(counts))
        finally:
            st.close(); plan.close(); scan.close()
    assert np.array_equal(hists[0], hists[1])
    quals = "".join(got["quality_scores"])
    assert hists[0].sum() == len(quals) and hists[0].reshape(-1, 256)[:, ord("I")].sum() == quals.count("I")


FASTA_CUTS = {"inside a definition line": (0, 5), "inside a sequence line": (2, 5), "directly in front of a '>'": (0, 0),
              "in front of the newline that ends a record": (0, -1), "directly behind a definition line": (1, 0)}


@pytest.mark.parametrize("what", list(FASTA_CUTS))
def test_fasta_the_cut_in_a_record(ctx, tmp_path, what):
    j, d = FASTA_CUTS[what]  # the line of its record (of four lines) that starts at CUT - d
    line_start = CUT - d
    k = (CUT // W - 8) // 4 * 4 + j
    pos = [W * (i + 1) - 1 for i in range(k - 1)] + [line_start - 1]
    at = line_start
    while at + W <= 3 * MIB + MIB // 5:
        pos.append(at + W - 1)
        at += W
    text = E.with_newlines_at(pos[-1] + 1, pos, "fasta", defs=set(range(0, len(pos), 4)), crlf=(k - 1, k + 7))
    assert text[line_start - 1:line_start] == b"\n" and (text[line_start:line_start + 1] == b">") == (j == 0)
    path = tmp_path / "t.fasta"
    path.write_bytes(text)
    got, sizes, flags, stats = both(ctx, path, "fasta")
    assert flags == (True, False) and stats["slabs"] >= 3
    n = check_columns("fasta", got, text)
    assert sum(sizes) == n and sizes == slab_sizes("fasta", np.asarray(pos), text, len(text)), what


# ---- the end of the input -------------------------------------------------------------------------------------------------------------------
def ending(fmt, how):
    """a file of three slabs and something whose end is `how` (tail only, on the slab edge: of three slabs to the byte);
    -> (bytes of the file, the same text properly ended)"""
    group = 4 if fmt == "fastq" else 1
    head = head_of(fmt)
    edge = (FIRST_CUT[fmt] + 2) * MIB
    n_file = edge if how in ("tail only", "on the slab edge") else edge + MIB // 5
    pos, _ = positions(n_file - len(head) - 2 * W, 5 * W, group)
    # the last line is made to end exactly where the file has to
    end = n_file - len(head) - 1 + (1 if how == "tail only" else 0)
    while (len(pos) + 1) % group or end - pos[-1] > 2 * W:
        pos.append(pos[-1] + W)
    assert W // 2 < end - pos[-1] < 3 * W
    pos.append(end)
    whole = E.with_newlines_at(end + 1, pos, fmt, crlf=(len(pos) - 1,) if how == "cr, no newline" else (), noisy=True)
    cutoff = {"no newline": 1, "cr, no newline": 1, "tail only": 1, "on the slab edge": 0}[how]
    data = head + whole[:len(whole) - cutoff]
    if how in ("tail only", "on the slab edge"):
        assert len(data) == edge
    return data, whole


@pytest.mark.parametrize("kind", ["plain", "bgzf", "gzip"])
@pytest.mark.parametrize("how", ["no newline", "cr, no newline", "tail only", "on the slab edge"])
@pytest.mark.parametrize("fmt", ["vcf", "fastq"])
def test_the_end_of_the_input(ctx, tmp_path, fmt, how, kind):
    """no newline: the last line (FASTQ: the last record's quality line) lacks its terminator; cr, no newline: it ends in a CR;
    tail only: the file ends on a slab edge to the byte and lacks the terminator, so the last slab is the carried tail and no fresh
    byte; on the slab edge: the same size, the last byte the newline, so the last slab is empty.  All rows come out, the last one
    whole, decoded on the device -- but for the CR: only "\\r\\n" is a terminator, a CR that ends the input belongs to the last field
    (host/io.h read_line), and behind the '\\n' the slab reader appends the parsers would drop it.  Before this test the pipeline did
    just that (the device rows lacked the byte the host reader returns); now such an input is handed to the host reader, and the
    case pins the hand-over and the byte."""
    data, whole = ending(fmt, how)
    assert (data[-1:] == b"\n") == (how == "on the slab edge") and (how != "cr, no newline" or data[-1:] == b"\r")
    path = tmp_path / ("t." + EXT[fmt])
    path.write_bytes(data)
    path = compressed(tmp_path, path, kind)
    got, sizes, flags, stats = both(ctx, path, fmt)
    n = check_columns(fmt, got, whole, last_cr=how == "cr, no newline")
    assert sum(sizes) == n
    if how == "cr, no newline":
        assert not flags[0], "the hand-over must be reported"
        return
    assert flags == (True, kind != "plain"), "a hand-over to the host reader: the device path is not tested by this run"
    if kind == "plain":
        assert stats["slabs"] >= 3
        nl_file = E.newlines(whole) + len(head_of(fmt))
        want = slab_sizes(fmt, nl_file, whole, len(data) + 1)
        assert sizes == [s for s in want if s], "the slabs were not cut where this case puts the end of the file"


def test_fastq_a_last_record_short_of_a_line_is_the_host_readers(ctx, tmp_path):
    """three lines of a record at the end of the input: the device splitter counts the slab undecided, the pipeline hands over, and the
    scan gives what the host reader gives -- its error"""
    data, whole = ending("fastq", "no newline")
    short = whole[:E.newlines(whole)[-2] + 1]  # without the last record's quality line
    assert len(E.newlines(short)) % 4 == 3
    path = tmp_path / "short.fastq"
    path.write_bytes(short)
    errors = []
    for gpu_parse in (False, True):
        scan = exon_amd.Scan(str(path), "fastq", gpu_parse=gpu_parse, batch_size=ONE_BATCH)
        if gpu_parse:
            scan.bind_ctx(ctx)
        with pytest.raises(exon_amd.ExonHipError) as e:
            list(scan)
        errors.append(str(e.value))
        if gpu_parse:
            assert scan.decoded_on_gpu()[0] is False
        scan.close()
    assert errors[0] == errors[1] and "truncated FASTQ record" in errors[0]


@pytest.mark.parametrize("where", ["at the end of a slab", "in the middle of a slab"])
def test_vcf_a_line_longer_than_a_slab(ctx, tmp_path, where):
    """A row of 1 MiB + 100 bytes.  What becomes of it depends on where it starts, not on its length alone (a slab is the carried
    tail, up to 1 MiB, and 1 MiB of fresh bytes).  Starting 50 bytes in front of a cut, the next slab is those 50 bytes and 1 MiB
    without a newline: not one whole record in a slab, the file is the host reader's -- the same rows, and the scan says so.
    Starting in the middle of a slab, half a MiB of it is carried, the next slab holds it whole, and the device decodes the file."""
    start = CUT - 50 if where == "at the end of a slab" else CUT - MIB // 2
    pos, k = positions(start + W, start - len(E.VCF_HEADER))
    pos = pos[:k]
    long_end = start - len(E.VCF_HEADER) + MIB + 100 - 1
    pos += [long_end] + [long_end + W * (i + 1) for i in range(4000)]
    text = E.with_newlines_at(pos[-1] + 1, pos, "vcf")
    assert max(np.diff(pos)) == MIB + 100 and (E.VCF_HEADER + text)[start - 1:start] == b"\n"
    path = tmp_path / "long.vcf"
    path.write_bytes(E.VCF_HEADER + text)
    got, sizes, flags, stats = both(ctx, path, "vcf")
    assert flags == (where == "in the middle of a slab", False), "the hand-over must be reported, and only where there is one"
    assert check_columns("vcf", got, text) == len(pos) == sum(sizes)
    assert len(got["info"][k]) == MIB + 100 - len(b"1\t%d\t.\tA\tC\t.\t.\t\n" % (k + 1))
