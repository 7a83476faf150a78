"""CPU: tests/line_index_expect.py checked against itself and the host readers before the GPU tests lean on it -- the statement
(newlines, lines, consumed, fastq_views) against bytes.split and against what Scan(..., gpu_parse=False) reads from small files, and
every builder's output for its newlines: exactly where they were asked for, with rows the host readers number 1, 2, 3, ..."""
import numpy as np
import pytest

import exon_amd
import fasta_expect
import line_index_expect as E


def random_text(rng, n, p_nl, p_cr=0.05):
    a = rng.integers(32, 127, n).astype(np.uint8)
    a[rng.random(n) < p_cr] = 13
    a[rng.random(n) < p_nl] = 10
    return a.tobytes()


@pytest.mark.parametrize("p_nl", [0.0, 0.01, 0.3, 1.0])
@pytest.mark.parametrize("n", [0, 1, 17, 5000])
def test_the_statement_against_bytes_split(n, p_nl):
    rng = np.random.default_rng(n + int(100 * p_nl))
    for _ in range(5):
        text = random_text(rng, n, p_nl)
        parts = text.split(b"\n")
        whole, rest = parts[:-1], parts[-1]
        begin, end, end_nocr = E.lines(text)
        assert len(E.newlines(text)) == len(whole) == text.count(b"\n")
        assert [text[b:e] for b, e in zip(begin, end)] == whole
        assert [text[b:e] for b, e in zip(begin, end_nocr)] == [ln[:-1] if ln.endswith(b"\r") else ln for ln in whole]
        assert E.consumed(text) == len(text) - len(rest) if whole else E.consumed(text) == 0
        assert all(text[p] == 10 for p in E.newlines(text))


def fastq_by_hand(text, final):
    parts = text.split(b"\n")[:-1]
    n = len(parts) // 4
    out, at, bad = [], 0, 0
    strip = lambda s: s[:-1] if s.endswith(b"\r") else s
    for r in range(n):
        h, s, p, q = parts[4 * r:4 * r + 4]
        bad += h[:1] != b"@" or p[:1] != b"+"
        out.append((strip(h[1:]), strip(s), strip(q)))
        at += len(h) + len(s) + len(p) + len(q) + 4
    return out, at, bad + (1 if final and len(parts) % 4 else 0)


@pytest.mark.parametrize("final", [True, False])
def test_fastq_views_against_a_loop_over_split_lines(final):
    rng = np.random.default_rng(7)
    good = b"".join(b"@r%d x\r\n%s\n+\r\n%s\r\n" % (i, b"ACGT" * (i % 5), b"IIII" * (i % 5)) for i in range(40))
    texts = [good, good + b"@tail\nAC", good + b"@tail\nAC\n", b"", b"\n", b"\r\n\r\n\r\n\r\n", b"@\n\n+\n\n", b"x\nAC\n+\nII\n", b"@a\nAC\n-\nII\n"]
    texts += [random_text(rng, 3000, 0.1, 0.1) for _ in range(5)]
    for text in texts:
        v = E.fastq_views(text, final)
        want, at, bad = fastq_by_hand(text, final)
        assert v["n_reads"] == len(want) and v["consumed"] == at and v["n_undecided"] == bad
        for r, (h, s, q) in enumerate(want):
            # (a header line without a byte has no span: its end lies in front of its start)
            assert text[v["head_start"][r]:v["head_end"][r]] == h
            assert text[v["seq_start"][r]:v["seq_end"][r]] == s and text[v["qual_start"][r]:v["qual_end"][r]] == q
    assert E.fastq_views(good, final)["n_undecided"] == 0


def spread(rng, fmt, n_lines, lo=0):
    """ascending positions with line lengths from the format's shortest row up"""
    at, out = -1, []
    for i in range(n_lines):
        least = E.min_row(fmt, i) if fmt in ("vcf", "sam", "gff", "bed") else 2 if (fmt == "fasta" and i == 0) or (fmt == "fastq" and i % 2 == 0) else 0
        at += 1 + max(least, lo) + int(rng.integers(0, 60))
        out.append(at)
    return out


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_every_builder_puts_its_newlines_where_asked(fmt):
    rng = np.random.default_rng(3)
    for n_lines, extra in ((1, 0), (8, 0), (8, 33), (200, 1)):
        pos = spread(rng, fmt, n_lines)
        text = E.with_newlines_at(pos[-1] + 1 + extra, pos, fmt, crlf=(2, 5) if n_lines > 5 else ())
        assert len(text) == pos[-1] + 1 + extra and E.newlines(text).tolist() == pos
        assert E.consumed(text) == pos[-1] + 1
    assert E.newlines(E.with_newlines_at(100, [], fmt)).tolist() == []


def test_the_edge_positions_and_the_dense_builder():
    n = 3 * E.TILE + 1000
    pos = E.edge_positions(n)
    for e in E.EDGES:
        assert {e - 1, e, e + 1} <= set(pos)
    assert pos[0] < 16 and pos[-1] == n - 1 and len(pos) == 17
    assert E.newlines(E.with_newlines_at(n, pos, "fasta")).tolist() == pos
    assert E.newlines(E.with_newlines_at(n, pos, "fastq", strict=False)).tolist() == pos
    with pytest.raises(ValueError):
        E.with_newlines_at(n, pos, "fastq")  # (adjacent newlines: an empty header or '+' line)
    with pytest.raises(ValueError):
        E.with_newlines_at(n, pos, "vcf")
    for d in (-1, 0, 1):
        one = E.edge_positions(n, deltas=(d,), first=16 + d)
        for fmt in ("fastq", "vcf", "bed"):
            assert E.newlines(E.with_newlines_at(n, one, fmt)).tolist() == one
        for fmt in ("sam", "gff"):  # (their shortest rows are longer than the first load group)
            assert E.newlines(E.with_newlines_at(n, one[1:], fmt)).tolist() == one[1:]
    run = E.TILE + E.WAVE + E.THREAD + 1
    text = E.dense(E.TILE, run)
    assert text[:2] == b">d" and E.newlines(text).tolist() == list(range(E.TILE - 1, E.TILE + run))
    assert fasta_expect.slab(text, True)["n_records"] == 1


def read_all(path, fmt, **kw):
    s = exon_amd.Scan(str(path), fmt, **kw)
    try:
        names = [f.name for f in s.schema()]
        batches = list(s)
        return {name: [v for b in batches for v in b.field(k).to_pylist()] for k, name in enumerate(names)}
    finally:
        s.close()


PROJECT = {"vcf": ("id", "ref", "alt", "info"), "sam": ("name",), "gff": ("attributes",), "bed": ("name",), "fasta": (), "fastq": ()}


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_the_host_readers_read_what_the_builders_write(tmp_path, fmt):
    rng = np.random.default_rng(11)
    pos = spread(rng, fmt, 96 if fmt == "fastq" else 97)  # (the host reader refuses a FASTQ record that is not whole)
    text = E.with_newlines_at(pos[-1] + 1, pos, fmt, crlf=(3, 4, 5, 6, 40))
    path = tmp_path / ("t." + fmt)
    path.write_bytes((E.VCF_HEADER if fmt == "vcf" else b"") + text)
    got = read_all(path, fmt, project=PROJECT[fmt])
    begin, end, end_nocr = E.lines(text)
    raw = [text[b:e] for b, e in zip(begin, end_nocr)]
    if fmt == "fasta":
        assert got == fasta_expect.columns(text) and len(got["id"]) > 10
    elif fmt == "fastq":
        v = E.fastq_views(text, True)
        assert v["n_reads"] == 24 and len(got["name"]) == 24 and v["n_undecided"] == 0
        heads = [text[a:b].decode() for a, b in zip(v["head_start"], v["head_end"])]
        assert [h.split(" ", 1)[0] for h in heads] == got["name"]
        assert [text[a:b].decode() for a, b in zip(v["seq_start"], v["seq_end"])] == got["sequence"]
        assert [text[a:b].decode() for a, b in zip(v["qual_start"], v["qual_end"])] == got["quality_scores"]
    else:
        col = {"vcf": "pos", "sam": "start", "gff": "start", "bed": "start"}[fmt]
        assert got[col] == list(range(1, 98))
        last = {"vcf": "info", "sam": None, "gff": "attributes", "bed": "name"}[fmt]
        if fmt == "vcf":
            want = [r.rsplit(b"\t", 1)[1].decode() for r in raw]  # ('.' reads as no entry, a Flag key prints with its value)
            assert got["info"] == [{".": "", "FL": "FL=true"}.get(x, x) for x in want]
        elif fmt == "bed":
            assert got["name"] == [r.split(b"\t")[3].decode() for r in raw]
        elif fmt == "gff":
            assert got["attributes"] == [[("a", [r.rsplit(b"\t", 1)[1][2:].decode()])] for r in raw]
        assert last is None or len(got[last]) == 97
