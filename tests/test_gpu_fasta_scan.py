"""GPU: FASTA batches out of the GPU pipeline (Scan(..., "fasta", gpu_parse=True).bind_ctx(ctx)): id, description and sequence built on
the device (gpu_parse.hip: the FASTA parser; text_columns.hip: exon_text_fasta, the line-parallel k_fasta_seq_fill) must equal
tests/fasta_expect.py -- computed from the rows the test wrote -- and the host reader, on plain text, plain gzip and BGZF, across slab
cuts and batch cuts.  Every case but the hand-over requires decoded_on_gpu()[0]: a hand-over to the host reader must not be able to
hide a wrong kernel."""
import gc
import gzip
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import fasta_expect
from oracle import decode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "fasta")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")
EUNSUPPORTED, ESTATE = -4, -5
NAMES = ["id", "description", "sequence"]
BASES = b"ACGTNacgtnRYKM"
# sequence bytes come out of a pseudo-random pool: periodic text deflates into blocks of several MB of output, and a plain-gzip slab
# of 1 MB cannot hold one (the pipeline would hand such a file over whatever the FASTA kernels do)
POOL = np.random.RandomState(20240607).choice(np.frombuffer(BASES, np.uint8), 1 << 20).tobytes()


def bases(seed, n):
    at = (seed * 7919) % (len(POOL) - 128)
    return POOL[at:at + n]


def is_null(i):
    """the NULL rhythm of tests/test_gpu_text_columns_limits.py: not periodic in 32"""
    return i % 32 in (0, 31) or i % 7 == 3


def read(scan):
    """(columns by name, batch sizes, (decoded, inflated), rows) of a scan, which is closed"""
    try:
        fields = [f.name for f in scan.schema()]
        batches = list(scan)
        for b in batches:
            b.validate(full=True)
        cols = {name: [v for b in batches for v in b.field(k).to_pylist()] for k, name in enumerate(fields)}
        return cols, [len(b) for b in batches], scan.decoded_on_gpu(), scan.rows(), fields
    finally:
        scan.close()


def gpu(ctx, path, **kw):
    return read(exon_amd.Scan(str(path), "fasta", gpu_parse=True, **kw).bind_ctx(ctx))


def host(path, **kw):
    return read(exon_amd.Scan(str(path), "fasta", **kw))[0]


def compressed(tmp_path, text, kind):
    p = tmp_path / "t.fasta"
    p.write_bytes(text)
    if kind == "gzip":
        q = tmp_path / "t.fasta.gz"
        q.write_bytes(gzip.compress(text, 6))
        return q
    if kind == "bgzf":
        q = tmp_path / "t.bgzf.fasta.gz"
        subprocess.check_call([BGZIP, str(p), str(q), "6"], stdout=subprocess.DEVNULL)
        return q
    return p


def synthetic(n_records, big_at=None, big_bytes=0):
    """ragged records: 0 .. 9 lines of 0 .. 84 bytes (so every source and destination alignment of the 8-byte copies occurs), inner
    blanks, CRLF here and there, NULL descriptions in the rhythm of is_null; `big_at`: that record's sequence is big_bytes long"""
    out = []
    for i in range(n_records):
        d = b"s%d" % i + (b"|x" * (i % 4))
        if is_null(i):
            d += (b"", b" ", b"\t \t")[i % 3]
        else:
            d += (b" ", b"\t", b"  \t ")[i % 3] + b"desc %d of\tit " % i
        eol = b"\r\n" if i % 11 == 5 else b"\n"
        out.append(b">" + d + eol)
        n_lines = (i * 7 + i // 3) % 10
        for j in range(n_lines):
            w = (i * 13 + j * 29) % 85
            if i == big_at:
                w = 70
            ln = bases(i * 10 + j, w)
            if w > 20 and (i + j) % 17 == 0:
                ln = ln[:9] + b" " + ln[10:]
            out.append(ln + (b"\r\n" if (i + j) % 13 == 2 else b"\n"))
        if i == big_at:
            out.extend(bases(k, 70) + b"\n" for k in range(big_bytes // 70))
    return b"".join(out)


@pytest.fixture(scope="module")
def ragged():
    text = synthetic(16000)
    assert 3 << 20 < len(text) < 6 << 20  # four slabs of 1 MB at the least
    return text, fasta_expect.columns(text)


@pytest.mark.parametrize("name", ["test.fasta", "test.fasta.gz", "bgzf"])
def test_reference_fixtures(ctx, tmp_path, name):
    text = open(os.path.join(FIX, "test.fasta"), "rb").read()
    assert gzip.open(os.path.join(FIX, "test.fasta.gz")).read() == text
    path = compressed(tmp_path, text, "bgzf") if name == "bgzf" else os.path.join(FIX, name)
    got, sizes, flags, rows, fields = gpu(ctx, path)
    assert fields == NAMES and flags[0], "the batches did not come from the GPU pipeline"
    assert flags[1] == (name != "test.fasta")
    want = fasta_expect.columns(text)
    assert got == want and rows == len(want["id"]) == sum(sizes) > 0
    assert got == host(path)
    ref = decode.decode_fasta(os.path.join(FIX, "test.fasta"))
    assert got == {k: [r[k] for r in ref] for k in NAMES}


@pytest.mark.parametrize("batch_size", [1, 7, 8192])
@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
def test_ragged_records_across_slab_and_batch_cuts(ctx, tmp_path, monkeypatch, ragged, kind, batch_size):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    monkeypatch.setenv("EXON_HIP_GZ_SLAB_MB", "1")  # (plain-gzip slabs are cut by output bytes, by a switch of their own)
    text, want = ragged
    path = compressed(tmp_path, text, kind)
    got, sizes, flags, rows, _ = gpu(ctx, path, batch_size=batch_size)
    assert flags[0], "a hand-over to the host reader: the device path is not tested by this run"
    assert flags[1] == (kind != "plain")
    assert rows == len(want["id"]) == sum(sizes) and all(0 < k <= batch_size for k in sizes)
    for name in NAMES:
        assert got[name] == want[name], name
    if batch_size == 8192:
        assert got == host(path, batch_size=batch_size)


def test_no_final_newline(ctx, tmp_path, monkeypatch):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    for text in (synthetic(300) + b">last one\nACGT\nAC", synthetic(300) + b">last one"):
        for kind in ("plain", "bgzf", "gzip"):
            got, _, flags, _, _ = gpu(ctx, compressed(tmp_path, text, kind))
            assert flags[0] and got == fasta_expect.columns(text), kind


def test_a_record_beyond_the_carry_limit_goes_to_the_host_reader(ctx, tmp_path, monkeypatch):
    """one 3 MB record in the middle, 1 MB slabs: no slab holds two of its neighbours' definition lines around it, the pipeline hands
    over behind the rows it has emitted -- every record once, in order, and the scan says so"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    text = synthetic(9000, big_at=4500, big_bytes=3 << 20)
    want = fasta_expect.columns(text)
    assert len(want["sequence"][4500]) > (3 << 20) - 70
    got, sizes, flags, rows, _ = gpu(ctx, compressed(tmp_path, text, "plain"), batch_size=1000)
    assert not flags[0], "the hand-over must be reported"
    assert rows == 9000 == sum(sizes)
    for name in NAMES:
        assert got[name] == want[name], name


def test_bind_ctx_refusals(ctx, tmp_path):
    empty = tmp_path / "empty.fasta"
    empty.write_bytes(b"")
    blank = tmp_path / "blank.fasta"
    blank.write_bytes(b"\n>a\nAC\n")
    for path, word in ((empty, "empty"), (blank, "does not start with a '>'")):
        s = exon_amd.Scan(str(path), "fasta", gpu_parse=True)
        with pytest.raises(exon_amd.ExonHipError) as e:
            s.bind_ctx(ctx)
        assert e.value.code == EUNSUPPORTED and word in str(e.value), str(e.value)
        # the scan is still the host reader's
        assert read(s)[0] == fasta_expect.columns(path.read_bytes())
    # opened without gpu_parse: as for the other formats
    good = tmp_path / "good.fasta"
    good.write_bytes(b">a\nAC\n")
    s = exon_amd.Scan(str(good), "fasta")
    with pytest.raises(exon_amd.ExonHipError) as e:
        s.bind_ctx(ctx)
    assert e.value.code == EUNSUPPORTED and "host reader" in str(e.value)
    s.close()
    gz_blank = tmp_path / "blank.fasta.gz"
    gz_blank.write_bytes(gzip.compress(b" \n>a\nAC\n"))
    s = exon_amd.Scan(str(gz_blank), "fasta", gpu_parse=True)
    with pytest.raises(exon_amd.ExonHipError) as e:
        s.bind_ctx(ctx)
    assert e.value.code == EUNSUPPORTED
    s.close()


def test_bind_ctx_after_the_first_host_batch_is_estate(ctx, tmp_path):
    p = tmp_path / "t.fasta"
    p.write_bytes(synthetic(50))
    s = exon_amd.Scan(str(p), "fasta", gpu_parse=True, batch_size=10)
    first = next(iter(s))
    assert len(first) == 10
    with pytest.raises(exon_amd.ExonHipError) as e:
        s.bind_ctx(ctx)
    assert e.value.code == ESTATE
    s.close()


def test_unbound_scan_next_yields_the_host_readers_rows(tmp_path):
    text = synthetic(400)
    p = tmp_path / "t.fasta"
    p.write_bytes(text)
    cols, sizes, flags, rows, _ = read(exon_amd.Scan(str(p), "fasta", gpu_parse=True, batch_size=64))
    assert cols == fasta_expect.columns(text) and rows == 400 and sizes == [64] * 6 + [16]
    assert not flags[0]


def test_batches_outlive_the_scan(ctx, tmp_path, ragged, monkeypatch):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    text, want = ragged
    p = tmp_path / "t.fasta"
    p.write_bytes(text)
    s = exon_amd.Scan(str(p), "fasta", gpu_parse=True, batch_size=500).bind_ctx(ctx)
    held = list(s)
    assert s.decoded_on_gpu()[0]
    s.close()
    del s
    first = [0]
    for b in held:  # (a slab's last batch is short: the batches' first rows come from their sizes)
        first.append(first[-1] + len(b))
    assert first[-1] == len(want["id"]) and len(held) >= 18
    seq_even = [b.field(2) for b in held[::2]]  # single columns kept, their batches dropped
    odd = list(range(1, len(held), 2))
    held = held[1::2]
    gc.collect()
    for k, name in enumerate(NAMES):
        got = [v for b in held for v in b.field(k).to_pylist()]
        assert got == [v for j in odd for v in want[name][first[j]:first[j + 1]]], name
    assert [v for c in seq_even for v in c.to_pylist()] == [v for j in range(0, len(first) - 1, 2) for v in want["sequence"][first[j]:first[j + 1]]]
