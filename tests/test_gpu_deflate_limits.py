"""Both device inflate decoders (exon_hip_bgzf_inflate: exon_amd/csrc/inflate.hip; exon_hip_gzip_stream_*: gzip_stream.hip) on DEFLATE
streams zlib's encoder never writes: the table of tests/deflate_expect.py, whose every case tests/test_deflate_expect.py has checked
against zlib, against a plain inflater and against its own label on the CPU.

The contract: where zlib accepts, the device gives zlib's bytes; where zlib refuses, the device refuses and names the member
(first_bad_block for BGZF, the failed call for a gzip stream); a refusal never changes a byte outside the refused member's own
[out_offset, out_offset + out_size).  The reference reads BGZF through libdeflate and plain gzip through miniz_oxide; where they, zlib
and RFC 1951 differ, zlib decides: it is what the host readers that take over use."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import exon_amd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_expect as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
SLACK = 66 << 10


def inflate_raw(ctx, data, verify_crc=True):
    """exon_hip_bgzf_inflate over a sentinel-filled output buffer with 66 KiB of slack behind the last member:
    (return code, first_bad_block, message, the whole buffer, block table, bytes of output the table claims)"""
    blocks, n, consumed, out_bytes = exon_amd.bgzf_scan(data)
    assert consumed == len(data)
    comp = np.frombuffer(data, np.uint8)
    d_comp = ctx.to_device(np.concatenate([comp, np.zeros(4096 + (-len(comp)) % 4, np.uint8)]))
    d_out = ctx.to_device(np.full(out_bytes + SLACK + (-out_bytes) % 4, SENTINEL, np.uint8))
    bad = C.c_int32(-7)
    rc = ctx.lib.exon_hip_bgzf_inflate(ctx.h, None, d_comp.ptr, blocks, n, d_out.ptr, 1 if verify_crc else 0, C.byref(bad))
    msg = ctx.lib.exon_hip_last_error(ctx.h).decode(errors="replace") if rc else ""
    buf = d_out.to_host()
    d_comp.free()
    d_out.free()
    return rc, bad.value, msg, buf, blocks, out_bytes


def zlib_member(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return D.bgzf_member(co.compress(data) + co.flush(), D.crc32(data), len(data))


def text(n, seed):
    r = np.random.default_rng(seed)
    rows = "".join("%d\t%d\trs%d\t%s\tq%d\n" % (1 + i % 22, 1000 + i * 37, r.integers(1, 10**7), "ACGT"[i % 4], r.integers(0, 99)) for i in range(n // 20 + 2))
    return rows.encode()[:n]


@pytest.fixture
def small_chunks(monkeypatch):
    monkeypatch.setenv("EXON_HIP_GZ_CHUNK_KB", "4")  # read at stream creation


def accepted_members():
    """[(label, member, expected bytes)]: every accepted case bare and in its filler, a zlib-made neighbour behind each"""
    out = []
    for k, c in enumerate(D.CASES):
        if c.refused or not c.bgzf:
            continue
        for form in c.forms():
            deflate, expect = c.stream(form)
            out.append(("%s [%s]" % (c.label, form), D.bgzf_member(deflate, *c.crc_isize(expect)), expect))
            t = text(37 * k % 3000, k)
            out.append(("zlib-made neighbour %d" % k, zlib_member(t), t))
    return out


@pytest.fixture(scope="module")
def table():
    return accepted_members()


def test_accepted_members_one_launch(ctx, table):
    """more than 256 members: the serial kernel (wide_run) in auto mode; EXON_HIP_INFLATE_PAR=1 takes them through the lane-parallel
    decoder and its hand-back loop (test_every_symbol_loop_in_a_fresh_process)"""
    assert len(table) > 256
    rc, bad, msg, buf, blocks, out_bytes = inflate_raw(ctx, b"".join(m for _, m, _ in table))
    assert rc == 0 and bad == -1, (bad, msg, table[bad][0] if 0 <= bad < len(table) else None)
    for (label, _, expect), b in zip(table, blocks):
        assert b.out_size == len(expect), label
        got = buf[b.out_offset:b.out_offset + b.out_size].tobytes()
        if got != expect:
            at = next(i for i in range(len(expect)) if got[i] != expect[i])
            raise AssertionError("%s: first difference at byte %d of %d" % (label, at, len(expect)))
    assert (buf[out_bytes:] == SENTINEL).all()


def test_accepted_members_few_per_launch(ctx, table):
    """the same members eight to a launch: small launches take the lane-parallel kernel in auto mode (members below its 6144-bit
    floor and every block it hands back run symbol_run_v)"""
    for i in range(0, len(table), 8):
        part = table[i:i + 8]
        rc, bad, msg, buf, blocks, out_bytes = inflate_raw(ctx, b"".join(m for _, m, _ in part))
        assert rc == 0, (msg, part[bad][0])
        for (label, _, expect), b in zip(part, blocks):
            assert buf[b.out_offset:b.out_offset + b.out_size].tobytes() == expect, label
        assert (buf[out_bytes:] == SENTINEL).all()


GZIP_CLASSES = sorted({c.cls for c in D.CASES if c.gzip and not c.refused})


@pytest.mark.parametrize("cls", GZIP_CLASSES)
def test_accepted_streams_gzip_decoder(ctx, small_chunks, cls):
    """the same streams as one-member gzip files through the chunked decoder, 4 KiB chunks (streams above 4 KiB span several: their
    chunks behind the first begin with the window unknown)"""
    for c in D.CASES:
        if c.cls != cls or not c.gzip or c.refused:
            continue
        deflate, expect = c.stream()
        got = ctx.gzip_inflate(D.gzip_member(deflate, D.crc32(expect), len(expect)))
        assert got == expect, c.label


def test_gzip_files_for_the_chunked_decoder(ctx, small_chunks):
    """distances 32768 and 32767 from the first symbol of a chunk (the marker of window byte 0: 256 + WIN + idx with idx = -32768) and
    from a few symbols in; a chain of such copies over 76 chunks, each copying the copy of the chunk 8 in front (markers until the
    maps are composed: two groups of 64); members that reach their own first byte (accepted) and one byte beyond (refused), from the
    member's first chunk and from three chunks on, whole files and 8 KiB slabs."""
    for label, raw, expect, _ in D.gzip_files():
        for slab in (None, 8 << 10) if "three chunks on" in label else (None,):
            if expect is None:
                with pytest.raises(exon_amd.ExonHipError, match="invalid distance too far back"):
                    ctx.gzip_inflate(raw, slab_bytes=slab)
                continue
            got, st = ctx.gzip_inflate(raw, slab_bytes=slab, return_stats=True)
            assert got == expect, label
            if label.startswith("a chain"):
                assert st["calls"] == 1 and st["chunks"] >= 85 and st["members"] == 1, st


def neighbours():
    g = [text(3000, 1), np.random.default_rng(2).integers(0, 256, 40000, dtype=np.uint8).tobytes(), text(5000, 3), b"0123456789"]
    return g, [zlib_member(x) for x in g]


REFUSED_CLASSES = sorted({c.cls for c in D.CASES if c.refused})


@pytest.mark.parametrize("verify_crc", [True, False])
@pytest.mark.parametrize("cls", REFUSED_CLASSES)
def test_refused_member_between_good_ones(ctx, cls, verify_crc):
    """One refused member per launch, third of five: the call fails and names member 2; the four neighbours hold zlib's bytes and
    the 66 KiB behind the last one the sentinel, byte for byte.  A distance beyond the member's first byte would copy the 40000
    random bytes of the member in front; the trailer is the one those bytes would satisfy, so with verify_crc=False nothing but the
    distance check can refuse (and with ISIZE wrong, nothing but the size check)."""
    good, members = neighbours()
    for c in D.CASES:
        if c.cls != cls or not c.bgzf:
            continue
        for form in c.forms():
            deflate, unchecked = c.stream(form, history=good[1])
            crc, isize = c.crc_isize(unchecked)
            bad_member = D.bgzf_member(deflate, crc, min(isize, 65536))
            rc, bad, msg, buf, blocks, out_bytes = inflate_raw(ctx, b"".join(members[:2] + [bad_member] + members[2:]), verify_crc)
            where = (c.label, form, verify_crc, msg)
            if c.label == "a wrong CRC-32" and not verify_crc:  # nothing is wrong with its bytes
                assert rc == 0 and bad == -1, where
                assert buf[blocks[2].out_offset:blocks[2].out_offset + blocks[2].out_size].tobytes() == unchecked, where
            else:
                assert rc != 0 and bad == 2 and "block 2" in msg, where
            for k, g in ((0, good[0]), (1, good[1]), (3, good[2]), (4, good[3])):
                assert buf[blocks[k].out_offset:blocks[k].out_offset + blocks[k].out_size].tobytes() == g, (where, "neighbour", k)
            assert (buf[out_bytes:] == SENTINEL).all(), where


@pytest.mark.parametrize("cls", [x for x in REFUSED_CLASSES if x != "refused/distance"])
def test_refused_streams_gzip_decoder(ctx, small_chunks, cls):
    """the same refusals from the chunked decoder, as the second member of a two-member file (the distance class has files of its
    own: test_gzip_files_for_the_chunked_decoder)"""
    first = text(2000, 5)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    head = co.compress(first) + co.flush()
    for c in D.CASES:
        if c.cls != cls or not c.gzip:
            continue
        deflate, unchecked = c.stream()
        crc, isize = c.crc_isize(unchecked)
        raw = head + D.gzip_member(deflate, crc, isize)
        with pytest.raises(exon_amd.ExonHipError):
            ctx.gzip_inflate(raw)
    assert ctx.gzip_inflate(head) == first


def par_child():
    """run under EXON_HIP_INFLATE_PAR=1 in a process of its own: the filler forms through the lane-parallel decoder, which must have
    decoded blocks itself (out32[0]) -- every member made "around" its case carries two filler blocks of more than 8000 bits of
    fixed-code symbols each, inside all of its caps -- rather than handing all of them back to the serial loop"""
    ctx = exon_amd.Context(0)
    members = [(c.label, D.bgzf_member(d, *c.crc_isize(e)), e, c.filler) for c in D.CASES if not c.refused and c.bgzf and c.filler for d, e in [c.stream("filler")]]
    rc, bad, msg, buf, blocks, out_bytes = inflate_raw(ctx, b"".join(m for _, m, _, _ in members))
    assert rc == 0, msg
    for (label, _, expect, _), b in zip(members, blocks):
        assert buf[b.out_offset:b.out_offset + b.out_size].tobytes() == expect, label
    st = (C.c_uint32 * 32)()
    assert ctx.lib.exon_hip_bgzf_inflate_par_stats(None, st) == 0
    print("par stats", list(st)[:16])
    print(st[0], sum(1 for m in members if m[3] == "around"))


@pytest.mark.parametrize("mode", ["0", "1"])
def test_every_symbol_loop_in_a_fresh_process(mode):
    """EXON_HIP_INFLATE_PAR is read once per process: this module again under =0 (the serial kernel's wide loop for every launch) and
    under =1 (the lane-parallel decoder and its hand-back loop symbol_run_v for every launch)."""
    env = dict(os.environ, EXON_HIP_INFLATE_PAR=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "--timeout", "300", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "not fresh_process"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (mode, r.stdout[-3000:] + r.stderr[-2000:])


def test_lane_parallel_decoder_at_work_in_a_fresh_process():
    """a short child under EXON_HIP_INFLATE_PAR=1 that must find the lane-parallel decoder decoding blocks of the filler forms itself
    (a decoder that handed every block back to the serial loop would prove nothing about itself)"""
    env = dict(os.environ, EXON_HIP_INFLATE_PAR="1")
    code = "import sys; sys.path.insert(0, %r); import test_gpu_deflate_limits as t; t.par_child()" % os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    decoded, around = (int(x) for x in r.stdout.strip().splitlines()[-1].split())
    assert decoded >= around, r.stdout[-500:]
