"""GPU-side BED parsing (exon_hip_bed_parser_*, k_parse_bed_lines) through exon_amd.BEDParser against tests/bed_expect.py, the
plain-Python restatement of host/bed.h's rules, at the sizes where the kernel can go wrong: row counts around a wave and a
workgroup, every misalignment on the identity and the ranked path, mixed field counts in neighbouring lanes, TABs on the edges of
the 16-byte groups, name lengths up to 70 000 bytes, a shorter slab behind a longer one, and every kind of undecided row."""
import numpy as np
import pytest

import exon_amd
import bed_expect

pytestmark = pytest.mark.gpu
TPB = 256
SLAB = 1 << 20  # the parsers' slab size here: every text of this file fits
PROJ = exon_amd._lib.PROJECT_BED["name"] | exon_amd._lib.PROJECT_BED["score"] | exon_amd._lib.PROJECT_BED["strand"]


def bits(bitmap, n):
    return np.unpackbits(bitmap, bitorder="little")[:n].astype(bool)


def device_columns(res, parser):
    """parse_host's result in bed_expect.expect's form: ids through the parser's names"""
    n = res["n_rows"]
    names = parser.names()
    assert (res["chrom_id"] >= 0).all() and (res["chrom_id"] < len(names)).all()
    out = {"n_rows": n, "chrom": [names[i].encode() for i in res["chrom_id"]], "start": res["start"], "end": res["end"]}
    if res["projected"]:
        out["names"] = res["names"]
        for name in ("score", "strand"):
            out[name + "_valid"] = bits(res[name + "_valid"], n)
        out["score"], out["strand_id"] = res["score"], res["strand_id"]
        # NULL slots hold defined values: 0
        assert (res["score"][~out["score_valid"]] == 0).all() and (res["strand_id"][~out["strand_valid"]] == 0).all()
        assert (res["name_len"][[v is None for v in res["names"]]] == 0).all()
    return out


def assert_same(got, want, what=""):
    assert got["n_rows"] == want["n_rows"], what
    assert got["chrom"] == want["chrom"], (what, "reference_sequence_name")
    for name in ("start", "end"):
        assert np.array_equal(got[name], want[name]), (what, name)
    if "names" in got:
        assert got["names"] == want["names"], (what, "name")
        for name in ("score_valid", "score", "strand_valid", "strand_id"):
            assert np.array_equal(got[name], want[name]), (what, name)


def check(ctx, text, misalign=0, parser=None, want=None, projection=PROJ):
    own = parser is None
    parser = parser or exon_amd.BEDParser(ctx, max_slab_bytes=SLAB)
    res = parser.parse_host(text, misalign=misalign, projection=projection)
    assert res["n_undecided"] == 0, (misalign, res)
    last = text.rfind(b"\n") + 1
    assert res["consumed_bytes"] == last
    assert res["projected"] == bool(projection)
    assert_same(device_columns(res, parser), want or bed_expect.expect(text[:last]), f"misalign {misalign}")
    if own:
        parser.close()
    return res


def row(i, nf):
    """row i with nf fields: names of every length class, scores over the whole of u16, the three strands"""
    name = (b"", b".", b"n", b"exon_%d" % i, b"NR_%06d_exon_%d_f" % (i * 7919 % 1000000, i % 40))[i % 5]
    f = [b"chr%d" % (i % 5 + 1), b"%d" % (i * 37 % 100000), b"%d" % (i * 37 % 100000 + i % 4000), name, b"%d" % ((i * 131) % 65536), b"+-."[i % 3:i % 3 + 1],
         b"%d" % i, b"%d" % (i + 5), b"0,0,255", b"2", b"10,20", b"0,30"]
    return b"\t".join(f[:nf])


def mixed(n, first=0):
    counts = (3, 4, 5, 6, 12)
    return b"".join(row(i, counts[(i * 7 + i // 5) % 5]) + b"\n" for i in range(first, first + n))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2 * TPB + 1])
def test_row_counts(ctx, n):
    text = mixed(n)
    check(ctx, text)
    check(ctx, text, projection=0)                     # PROJ = false: the three operand columns alone
    check(ctx, b"# head\n" + text, misalign=3)        # ranked: rows are ranks among the lines that are rows


def test_every_misalignment_identity_and_ranked(ctx):
    lines = mixed(300).split(b"\n")[:-1]
    plain = b"\n".join(lines) + b"\n"                                                         # no '#' line: row = line, validity by ballot
    ranked = b"#first\n" + b"".join(ln + b"\n#between %d\n" % i for i, ln in enumerate(lines[:150])) + b"#last\n"  # '#' first, last, between every pair
    assert b"#" not in plain and ranked.count(b"\n#") == 151
    for slab in (plain, ranked):
        want = bed_expect.expect(slab)
        parser = exon_amd.BEDParser(ctx, max_slab_bytes=SLAB)
        for misalign in range(16):
            check(ctx, slab, misalign=misalign, parser=parser, want=want)
        parser.close()


def test_neighbouring_lanes_of_every_field_count(ctx):
    text = b"".join(row(i, nf) + b"\n" for i in range(40) for nf in (3, 4, 5, 6, 12))
    res = check(ctx, text)
    assert res["n_rows"] == 200 and {len(ln.split(b"\t")) for ln in text.split(b"\n")[:-1]} == {3, 4, 5, 6, 12}
    valid = bits(res["name_valid"], 200).reshape(40, 5)
    assert not valid[:, :2].any() and valid[:, 2:].all()  # NULL on 3- and 4-field lines
    check(ctx, text.replace(b"\n", b"\r\n"))                # one CR in front of every LF


def test_tabs_on_group_edges(ctx):
    """a TAB as the last byte of a 16-byte group and as the first of the next, for every field's TAB; a line that ends exactly on
    a group edge; and the slab's last group read byte by byte (the slab ends 1 .. 15 bytes into it)"""
    parser = exon_amd.BEDParser(ctx, max_slab_bytes=SLAB)
    for pad in range(0, 34):
        chrom = b"c" * (1 + pad)  # shifts every TAB of the line across the group edges
        text = chrom + b"\t10\t20\tname\t5\t-\t1\t2\t0\t1\t2\t3\n" + chrom + b"\t1\t2\n" + b"x\t3\t4\tn\t65535\n"
        for misalign in (0, 1, 15):
            check(ctx, text, misalign=misalign, parser=parser)
    for n in range(16, 33):
        line = b"chr1\t1\t2\t" + b"n" * (n - 12) + b"\t7\n"  # n bytes, the newline included: the line ends on a group edge at n = 16, 32
        assert len(line) == n
        check(ctx, line * 3, parser=parser)
    parser.close()


@pytest.mark.parametrize("misalign", [0, 7])
def test_name_lengths_and_null_rows(ctx, misalign):
    lengths = [0, 1, 7, 8, 9, 255, 256, 70000]
    text = b"".join(b"chr1\t%d\t%d\t%s\t%d\t+\n" % (k, k + 1, bytes(97 + (j % 26) for j in range(n)), k) for k, n in enumerate(lengths))
    res = check(ctx, text, misalign=misalign)
    assert [len(v) for v in res["names"]] == lengths
    # NULL names at rows 0, 7, 8, 63, 64 of 130 (the bitmap's byte and wave edges), on both paths
    null_rows = {0, 7, 8, 63, 64}
    text = b"".join(row(i, 3 if i in null_rows else 6) + b"\n" for i in range(130))
    for slab in (text, b"#c\n" + text):
        res = check(ctx, slab, misalign=misalign)
        assert {i for i, v in enumerate(res["names"]) if v is None} == null_rows


def test_a_shorter_slab_behind_a_longer_one(ctx):
    parser = exon_amd.BEDParser(ctx, max_slab_bytes=SLAB)
    check(ctx, mixed(700), parser=parser)
    check(ctx, b"#c\n" + mixed(700, first=1000), parser=parser, misalign=5)
    check(ctx, mixed(70, first=5000), parser=parser)              # no stale offsets, values or validity behind row 69
    check(ctx, b"#c\n" + mixed(9, first=9000), parser=parser)
    res = check(ctx, b"chrZ\t0\t0\n", parser=parser)
    assert sorted(parser.names()[:5]) == ["chr1", "chr2", "chr3", "chr4", "chr5"] and parser.names()[5:] == ["chrZ"] and res["names"] == [None]
    check(ctx, b"chrZ\t1\t2\tn\t3\t-\n", parser=parser, projection=0)  # ... and back to the operand columns alone
    parser.close()


# rows the host reader reads although the device leaves them to it (valid UTF-8 beyond ASCII, more digits than the device takes)
HOSTS_TO_READ = {b"chr\xc3\xa9\t1\t2", b"chr1\t1\t2\tn\xc3\xa9\t1", b"chr1\t1\t2\t\xc3\xa9", b"chr1\t1\t2\tn\t1\t+\t1\t2\t0\t1\t4\tcaf\xc3\xa9",
                 b"chr1\t1\t2\tn\t000001", b"chr1\t1234567890123456789\t2"}
# rows the rules call an error, or whose decision is the host's: each makes exactly one undecided row
UNDECIDED = [
    b"chr\xc3\xa9\t1\t2",                                  # a byte >= 0x80 in each field (valid UTF-8 or not: the host's to say)
    b"chr1\t1\xff\t2", b"chr1\t1\t2\xff", b"chr1\t1\t2\tn\xc3\xa9\t1", b"chr1\t1\t2\tn\t1\x80", b"chr1\t1\t2\tn\t1\t\xff",
    b"chr1\t1\t2\t\xc3\xa9",                               # ... in the dropped fourth field of four
    b"chr1\t1\t2\tn\t1\t+\t1\t2\t0\t1\t4\tcaf\xc3\xa9",    # ... in an ignored field of twelve
    b"chr1\t1",                                            # 2 fields
    b"chr1",                                               # 1
    b"chr1\t1\t2\tn\t1\t+\t5",                             # 7
    b"chr1\t1\t2\tn\t1\t+\t1\t2\t0\t1\t4",                 # 11
    b"chr1\t1\t2\tn\t1\t+\t1\t2\t0\t1\t4\t0\tx",           # 13
    b"chr1\t1\t2\tn\t1\t+\t1\t2\t0\t1\t4\t0\tx\ty\tz\tw",  # 16
    b"chr1\t1\t2\tn\t65536", b"chr1\t1\t2\tn\t.", b"chr1\t1\t2\tn\t", b"chr1\t1\t2\tn\t-1", b"chr1\t1\t2\tn\t+",
    b"chr1\t1\t2\tn\t000001",                              # (six digits: the host's to read)
    b"chr1\t1\t2\tn\t1\t?", b"chr1\t1\t2\tn\t1\t", b"chr1\t1\t2\tn\t1\t+-",
    b"chr1\t1234567890123456789\t2",                       # a 19-digit position
    b"chr1\t1\t9223372036854775808",
    b"chr1\t\t2", b"chr1\t1\tx", b"chr1\t-1\t2", b"chr1\t1 \t2",
    b"",                                                   # an empty line
    b"chr1\t1\t2\r\r",                                     # (one CR is dropped, the second belongs to the end)
]


@pytest.mark.parametrize("k", range(len(UNDECIDED)))
def test_undecided_rows_between_good_rows(ctx, k):
    bad = UNDECIDED[k]
    good = [row(i, (3, 4, 5, 6, 12)[i % 5]) for i in range(70)]
    for at in (0, 33, 70):
        lines = good[:at] + [bad] + good[at:]
        for head in (b"", b"#c\n"):
            text = head + b"\n".join(lines) + b"\n"
            parser = exon_amd.BEDParser(ctx, max_slab_bytes=SLAB)
            res = parser.parse_host(text, projection=PROJ, all_rows=True, misalign=at % 16)
            assert res["n_undecided"] == 1 and res["n_rows"] == 71, (bad, at, res["n_undecided"])
            # the good rows' values are intact around it (dictionary ids are provisional in an undecided slab: not compared)
            want = bed_expect.expect(b"\n".join(good) + b"\n")
            keep = np.arange(71) != at
            assert np.array_equal(res["start"][keep], want["start"]) and np.array_equal(res["end"][keep], want["end"])
            assert [v for i, v in enumerate(res["names"]) if i != at] == want["names"]
            assert np.array_equal(bits(res["score_valid"], 71)[keep], want["score_valid"]) and np.array_equal(res["score"][keep], want["score"])
            assert np.array_equal(bits(res["strand_valid"], 71)[keep], want["strand_valid"]) and np.array_equal(res["strand_id"][keep], want["strand_id"])
            # without all_rows an undecided slab hands nothing back
            assert len(parser.parse_host(text, projection=PROJ)["start"]) == 0
            parser.close()
    if bad in HOSTS_TO_READ:
        assert bed_expect.expect(bad + b"\n")["n_rows"] == 1
    else:
        with pytest.raises(bed_expect.BedError):
            bed_expect.expect(bad + b"\n")


def test_limits_of_the_decided_values(ctx):
    text = (b"chr1\t0\t0\n" b"chr1\t+0\t+999999999999999999\n" b"chr1\t999999999999999999\t0\tn\t65535\n" b"chr1\t000000000000000018\t9\tn\t+0\t.\n"
            b"chr1\t9\t3\tn\t00042\t-\n" b"\t1\t2\n")
    res = check(ctx, text)
    assert list(res["start"]) == [0, 0, 999999999999999999, 18, 9, 1] and list(res["score"][2:5]) == [65535, 0, 42]


def test_dictionary_overflow_hands_back(ctx):
    parser = exon_amd.BEDParser(ctx, max_slab_bytes=SLAB)
    text = b"".join(b"contig_%d\t1\t2\n" % i for i in range(4097))
    assert parser.parse_host(text)["n_undecided"] >= 1  # more names than a device-built dictionary holds: the host reader's
    parser.close()
    parser = exon_amd.BEDParser(ctx, seed_names=["chrM", "contig_7"], max_slab_bytes=SLAB)
    text = b"".join(b"contig_%d\t1\t2\n" % i for i in range(4094))
    res = check(ctx, text, parser=parser, projection=0)
    assert parser.names()[:2] == ["chrM", "contig_7"] and len(parser.names()) == 4095 and res["chrom_id"][7] == 1
    parser.close()


def test_slab_cut_inside_a_line(ctx):
    text = mixed(50)
    for cut in (len(text), len(text) - 1, len(text) - 7):
        res = check(ctx, text[:cut])
        assert text[res["consumed_bytes"] - 1:res["consumed_bytes"]] == b"\n"
    p = exon_amd.BEDParser(ctx, max_slab_bytes=SLAB)
    res = p.parse_host(b"chr1\t1\t2")  # not one whole line
    assert (res["n_rows"], res["n_undecided"], res["consumed_bytes"]) == (0, 0, 0)
    p.close()
