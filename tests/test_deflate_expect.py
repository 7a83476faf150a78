"""The statement the device inflate tests rest on (tests/deflate_expect.py), itself under test, on the CPU: for every case of its
table zlib's raw inflate and `inflate_plain` give the bytes the case's author expects by construction, or both refuse with the
message the case names; the trace shows that the case is what its label says; the host readers' block inflater
(exon_amd/csrc/host/bgzf_block.h, compiled into a small harness) agrees on every member.  A GPU test can then only pass on streams
that hit their target."""
import os
import shutil
import struct
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_expect as D  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFLATE_CASES = [c for c in D.CASES if c.member_refusal is None]


def forms(c):
    return c.forms()


def holds(want, got):
    return want(got) if callable(want) else got == want


def test_the_table_has_what_the_issue_lists():
    n = D.class_counts()
    assert n == {"distance/bgzf/all-so-far": 11, "distance/bgzf/later": 10, "distance/top": 8, "distance/gzip-near-ring": 6, "length": 40,
                 "codes": 7, "header": 9, "stored": 5, "member": 3, "refused/distance": 10, "refused/symbols": 5, "refused/tables": 17,
                 "refused/input": 6, "refused/output": 4}
    assert len(D.gzip_files()) == 14
    # every BGZF accepted case exists bare and, unless it fills a member by itself, in >= 2 KiB of filler symbols
    for c in D.CASES:
        if not c.refused and c.filler:
            assert len(c.stream("filler")[0]) >= len(c.stream("bare")[0]) + 2048, c.label


@pytest.mark.parametrize("cls", sorted({c.cls for c in DEFLATE_CASES}))
def test_zlib_and_inflate_plain_agree_with_the_author(cls):
    for c in DEFLATE_CASES:
        if c.cls != cls:
            continue
        for form in forms(c):
            deflate, expect = c.stream(form)
            z, zmsg = D.zlib_verdict(deflate)
            r = D.inflate_plain(deflate)
            if c.refusal:
                assert z is None and zmsg == c.refusal, (c.label, form, zmsg)
                assert r.out is None and r.refusal == c.refusal, (c.label, form, r.refusal)
            else:
                assert z == expect, (c.label, form, zmsg)
                assert r.out == expect, (c.label, form, r.refusal)
            if form == "bare":  # the label's claim, on the stream as its author wrote it
                for name, want in c.claims.items():
                    assert holds(want, r.trace[name]), (c.label, name, r.trace[name])


def test_every_case_claims_something():
    for c in D.CASES:
        assert c.claims, c.label


def test_members_whose_trailer_lies():
    """the stream is good, ISIZE or the CRC-32 is not: inflate_plain gives the bytes, a gzip reader (zlib, wbits 31) refuses"""
    for c in D.CASES:
        if c.member_refusal is None:
            continue
        deflate, expect = c.stream()
        assert D.inflate_plain(deflate).out == expect and D.zlib_verdict(deflate)[0] == expect
        crc, isize = c.crc_isize(expect)
        with pytest.raises(zlib.error, match=c.member_refusal):
            zlib.decompressobj(31).decompress(D.gzip_member(deflate, crc, isize))
        assert D.inflate_gzip_plain(D.gzip_member(deflate, crc, isize))[0] is None


def test_gzip_files_for_the_chunked_decoder():
    for label, raw, expect, claims in D.gzip_files():
        got, refusal, traces = D.inflate_gzip_plain(raw)
        try:
            z, rest = b"", raw
            while rest:
                d = zlib.decompressobj(31)
                z += d.decompress(rest)
                assert d.eof
                rest = d.unused_data
        except zlib.error as e:
            z = None
            assert "invalid distance too far back" in str(e), label
        if expect is None:
            assert z is None and got is None and refusal == "invalid distance too far back", label
        else:
            assert z == expect and got == expect, (label, refusal)
            for name, want in claims.items():
                assert holds(want, traces[-1][name]), (label, name)
            # every dynamic block of the chunk files begins at a 4 KiB border of the FILE, and every chunk inflates to 4 KiB
            if label.startswith(("dist=", "a chain")):
                assert (len(raw) - 8 - 2) % D.CHUNK == 0 and len(expect) == 36849 + (len(raw) - 10 - 36864) // D.CHUNK * D.CHUNK


def test_inflate_plain_against_zlib_made_streams():
    """the statement itself under test: streams of zlib's encoder, every strategy, as tests/test_gpu_inflate.py makes them"""
    import random
    r = random.Random(5)
    text = b"".join(b"%d\t%d\trs%d\tACGT\t%f\n" % (1 + i % 22, 1000 + i * 37, r.randrange(1, 10**7), r.random()) for i in range(1500))
    runs = b"".join(bytes([65 + i % 26]) * (i % 7) for i in range(400)) + b"".join(r.randbytes(d) * (700 // d + 1) for d in range(1, 40))
    for data in (text, runs, r.randbytes(20000), bytes(30000), b""):
        for level, strategy in ((6, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY),
                                (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)):
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            deflate = co.compress(data[:len(data) // 2]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(data[len(data) // 2:]) + co.flush()
            res = D.inflate_plain(deflate)
            assert res.out == data, (len(data), level, strategy, res.refusal)
            assert res.trace["max_distance"] <= 32506  # (what the issue says of zlib's encoder: window - MIN_LOOKAHEAD)
            for cut in (len(deflate) - 1, len(deflate) // 2):
                if cut > 0:
                    assert D.inflate_plain(deflate[:cut]).refusal == "truncated" and D.zlib_verdict(deflate[:cut])[1] == "truncated"
    far = r.randbytes(32768)
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    assert D.inflate_plain(co.compress(far + far + far) + co.flush()).trace["max_distance"] == 0  # (zlib cannot reach 32768 back at all)


def test_build_code_rule_before_and_after():
    """inflate.hip's build_code_impl let an incomplete code through whenever it had ONE symbol; zlib (inflate_table) takes one code
    only at length 1, and never for the code-length code.  The rule before, the rule now and zlib's, side by side, over every
    single-code set and over the table's own sets: the old rule accepts what zlib refuses exactly for one code of length 2..15."""
    for which, size in (("lit", 286), ("dist", 30), ("cl", 19)):
        for length in range(1, 16 if which != "cl" else 8):
            lens = [0] * size
            lens[size // 2] = length
            assert D.accepts_parent_build_code(lens, which)                                  # before: always
            assert D.accepts_zlib(lens, which) == (length == 1 and which != "cl")
            assert D.accepts_build_code(lens, which) == D.accepts_zlib(lens, which)          # now: zlib's verdict
    sets = [([2], "dist"), ([0, 0, 0, 15], "dist"), ([2, 2], "dist"), ([1, 1, 1], "dist"), ([1], "dist"), ([0] * 30, "dist"), ([1, 1], "dist"),
            ([0, 0, 1], "cl"), ([1, 2], "cl"), ([1, 1], "cl"), (D.FIXED_LIT, "lit"), (D.FIXED_DIST, "dist"), ([1, 2, 3, 3], "lit"), ([3] * 7, "lit")]
    for lens, which in sets:
        assert D.accepts_build_code(lens, which) == D.accepts_zlib(lens, which), (lens, which)
    # the two cases of the issue: served by the BGZF device path before, refused now, as zlib and the gzip device path do
    for lens in ([2], [0, 0, 0, 15]):
        assert D.accepts_parent_build_code(lens, "dist") and not D.accepts_build_code(lens, "dist") and not D.accepts_zlib(lens, "dist")


@pytest.fixture(scope="module")
def host_inflater(tmp_path_factory):
    """host/bgzf_block.h compiled from the header the library is built from (no GPU needed)"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("bgzf") / "bgzf_block_harness")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "exon_amd", "csrc"), os.path.join(ROOT, "tests", "bgzf_block_harness.cpp"),
                    "-o", exe, "-lz"], check=True)

    def run(members):
        inp = b"".join(struct.pack("<I", len(m)) + m for m in members)
        r = subprocess.run([exe], input=inp, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-500:]
        out, o, res = r.stdout, 0, []
        for _ in members:
            ok, n = out[o], struct.unpack_from("<I", out, o + 1)[0]
            res.append((bool(ok), out[o + 5:o + 5 + n]))
            o += 5 + n
        assert o == len(out)
        return res
    return run


def test_host_block_inflater_agrees_on_every_member(host_inflater):
    """it is zlib: the bytes where zlib accepts, a refusal where it refuses.  (The table found one exception, since mended: a member
    whose ISIZE is 0 was not inflated at all, so an empty member was accepted whatever its DEFLATE data held, where the device
    refuses it.)"""
    todo = []
    for c in D.CASES:
        if not c.bgzf:
            continue
        for form in forms(c):
            deflate, expect = c.stream(form, history=b"\xAA" * 70000 if c.cls == "refused/distance" else b"")
            crc, isize = c.crc_isize(expect)
            todo.append((c, form, D.bgzf_member(deflate, crc, min(isize, 65536)), expect))
    res = host_inflater([m for _, _, m, _ in todo])
    for (c, form, _, expect), (ok, got) in zip(todo, res):
        if c.refused:
            assert not ok, (c.label, form)
            assert got.startswith(b"BGZF inflate error") or (c.member_refusal and c.trailer(expect)[1] == len(expect) and got.startswith(b"BGZF CRC-32 mismatch")), (c.label, got)
        else:
            assert ok and got == expect, (c.label, form, got[:80])
    # ISIZE = 0: the end-of-file marker and the empty cases above are taken, DEFLATE data zlib refuses (or that has output) is not
    eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    bad = next(c for c in D.CASES if c.label == "block type 3")
    some = next(c for c in D.CASES if c.label == "len=3 dist=1")
    res = host_inflater([eof, D.bgzf_member(bad.stream()[0], 0, 0), D.bgzf_member(some.stream()[0], 0, 0)])
    assert res[0] == (True, b"") and not res[1][0] and not res[2][0], res
