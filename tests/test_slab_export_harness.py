"""CPU: exon_amd/csrc/host/slab_export.h -- the plan, the views, the gather and the runs scan every fixed-width column of an
exported batch goes through -- in a stand-alone program (tests/slab_export_harness.cpp) built with AddressSanitizer and
UndefinedBehaviorSanitizer.  The program holds 19 hand-made rows of every layout in exact-size heap buffers and prints every row of
the views and gathers below; what the exporter has always made of such rows is worked out here from the columns' literals and
compared.  Nothing sanitized is loaded into Python.

The expectations restate the exporter's rules, not the header's code: a view has the batch's length, the offset of its first row
behind the copied span's first row (a multiple of 8), null_count -1 where the column came with a bitmap and 0 elsewhere; a Flag's
values are its bitmap; a gathered array has offset 0, its exact null count and a bitmap only where a gathered row is NULL; an
all-NULL column has null_count = length; a BED batch is in the schema's order (name in front of score and strand, NULL columns
last).  (The layouts are built by hand in the program: scan.cpp's own per-format layouts are what the GPU scan tests check.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 19
V1 = [1, 1, 0, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0]
V2 = [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1]
FLAGV = [1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1]
NAME = ["a", "bc", "", "d", "efg", "h", "ij", "k", "lmn", "", "o", "pq", "x", "r", "stu", "v", "w", "xyz", "end"]
CUTS = [(0, 19), (0, 8), (8, 8), (16, 3), (5, 9), (18, 1)]
ROW_LISTS = [("all", list(range(N))), ("last", [18]), ("edges", [0, 7, 8, 15, 16, 18]), ("hollow", [2, 7, 9])]  # hollow: NULL in every V1 column and the Flag
WIDTH = {"c": 1, "i": 4, "f": 4, "I": 8, "b": 0}


def fixed(t, c, valid=None, names=None):
    """column c of type t (c u8, i i32, f f32, I i64, b Flag): (type, has a bitmap, dictionary, the 19 rows as printed)"""
    def shown(r):
        if valid is not None and not valid[r]:
            return "NULL"
        if t == "b":
            return "true"
        if t == "c":
            return str((r * 13 + c) % 256)
        if t == "i":
            return str(r % len(names) if names else 10 * r - 50 + c)
        if t == "f":
            return "%g" % (r * 0.5 - 2.0 + c)
        return str((r + 1) * 4294967296 + r + c)
    return (t, valid is not None, names, [shown(r) for r in range(N)])


TEXT = ("T", True, None, ['"%s"' % NAME[r] if V2[r] else "NULL" for r in range(N)])
NULL_I64 = ("n", True, None, ["NULL"] * N)
NULL_UTF8 = ("u", True, None, ["NULL"] * N)


def bed(name, score, strand, nulls):
    cols = [fixed("i", 0, None, ["chr1", "chr2"]), fixed("I", 1), fixed("I", 2)]
    c = 3
    kids = list(cols)
    if name:
        kids.append(TEXT)
    if score:
        kids.append(fixed("I", c, V1))
        c += 1
    if strand:
        kids.append(fixed("i", c, V2, ["+", "-"]))
    return kids + ([NULL_I64, NULL_UTF8] if nulls else [])


CASES = {  # name -> the children of its batches, in order
    "vcf": [fixed("i", 0, None, ["chr1", "chr2", "chrX"]), fixed("I", 1, V2), fixed("f", 2, V1), fixed("i", 3, None, ["PASS", "q10", "q10;s50"]),
            fixed("i", 4, V1), fixed("f", 5, V2), fixed("b", 6, FLAGV)],
    "bam": [fixed("i", 0), fixed("c", 1, V1), fixed("i", 2, V2, ["ref0", "ref1"]), fixed("I", 3, V2), fixed("I", 4, V2), TEXT],
    "gff": [fixed("i", 0, None, ["s1", "s2"]), fixed("i", 1, None, ["src"]), fixed("i", 2, None, ["gene", "exon", "CDS", "mRNA"]), fixed("I", 3), fixed("I", 4),
            fixed("f", 5, V1), fixed("i", 6, V1, ["+", "-"]), fixed("i", 7, V2, ["0", "1", "2"])],
    "bed_": bed(False, False, False, False),
    "bed_n": bed(True, False, False, False),
    "bed_st": bed(False, True, True, False),
    "bed_t": bed(False, False, True, False),
    "bed_nstz": bed(True, True, True, True),
}


def pad(b):
    return (b + 63) & ~63


def plan_line(name, kids, span, lo, hi):
    c_lo = lo & ~7
    c_n = hi - c_lo
    widths = [WIDTH[t] for t, _, _, _ in kids if t in WIDTH]
    n_nulls = sum(t in "nu" for t, _, _, _ in kids)
    zbytes = pad((c_n + 1) * 8) if n_nulls else 0
    total = sum(pad(c_n * w) + pad((c_n + 7) // 8) for w in widths) + pad((c_n + 7) // 8) + zbytes  # per column values + bitmap, the row mask, the zeros
    return "P %s %d c_lo=%d c_n=%d bytes=%d zbytes=%d" % (name, span, c_lo, c_n, total, zbytes)


def dict_shown(names):
    return "[" + "|".join('"%s"' % s for s in names) + "]" if names else ""


def expected():
    out = []
    for name, kids in CASES.items():
        for span, (lo, hi), cuts in ((0, (0, N), CUTS), (1, (11, 18), [(11, 7)])):
            out.append(plan_line(name, kids, span, lo, hi))
            for b0, n in cuts:
                head = "V %s %d %d" % (name, b0, n)
                sigs = []
                for t, bitmap, names, _ in kids:
                    if t in "nu":
                        sigs.append("%s(%d,0,%d,1)" % (t, n, n))
                    elif t == "T":  # (the harness's own stand-in for a text root: the slab's buffers, cut by the offset)
                        sigs.append("T(%d,%d,-1,1)" % (n, b0))
                    else:
                        sigs.append("%s(%d,%d,%d,%d)%s" % (t, n, b0 - (lo & ~7), -1 if bitmap else 0, bitmap, dict_shown(names)))
                out.append(head + " sig " + " ".join(sigs))
                out += [head + " %d\t" % i + "\t".join(rows[b0 + i] for _, _, _, rows in kids) for i in range(n)]
        for lname, idx in ROW_LISTS:
            head = "G %s %s" % (name, lname)
            sigs = []
            for t, _, names, rows in kids:
                nulls = sum(rows[r] == "NULL" for r in idx)
                sigs.append("%s(%d,0,%d,%d)%s" % (t, len(idx), nulls, nulls > 0, dict_shown(names)))
            out.append(head + " sig " + " ".join(sigs))
            out += [head + " %d\t" % i + "\t".join(rows[r] for _, _, _, rows in kids) for i, r in enumerate(idx)]

    def runs(name, runs_):
        rows = [r for a, b in runs_ for r in range(a, b)]
        return "R %s too_many=0 kept=%d runs=%s rows=%s" % (name, len(rows), "".join("(%d,%d)" % r for r in runs_), "".join("%d," % r for r in rows))
    out.append(runs("ones", [(0, 19)]))
    out.append(runs("zeros", []))
    out.append(runs("one", [(5, 17)]))
    out.append(runs("three", [(1, 3), (6, 10), (17, 19)]))
    out.append("R many too_many=1")  # 257 single-row runs: more than the 256 a slab goes out as views with
    out.append(runs("most", [(r, r + 1) for r in range(0, 512, 2)]))
    return out


def test_views_gathers_plan_and_runs_of_every_layout(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "slab_export_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "exon_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "slab_export_harness.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]  # (a sanitizer report ends the program with a status)
    got = r.stdout.decode().split("\n")[:-1]
    want = expected()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
    # what the whole-slab plan of the widest case comes to, by hand, in 64-byte units: 19 rows of 4 bytes are 76 -> 128, of 8 bytes 152 -> 192,
    # a bitmap 3 -> 64.  BED with score, strand and two NULL columns: values 128 + 192 + 192 + 192 + 128, five bitmaps, the row mask,
    # and (19 + 1) * 8 = 160 -> 192 bytes of zeros
    assert "P bed_nstz 0 c_lo=0 c_n=19 bytes=%d zbytes=192" % (2 * 128 + 3 * 192 + 5 * 64 + 64 + 192) in got
