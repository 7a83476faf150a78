"""CPU: exon_amd/csrc/host/text_export.h -- the plan, the views and the gather every device-built text column goes through -- in a
stand-alone program (tests/text_export_harness.cpp) built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program holds
19 hand-made rows of every column shape in exact-size heap buffers and prints every row of the views and gathers below; the rows
are repeated here as literals and compared.  Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 19

UTF8N = ["a", "bc", "", None, "defg", "h", "ij", "k", "lmn", "", "o", "pq", None, "r", "stu", "v", "w", "xyz", "end"]
LISTN = [["a"], ["b", "c"], ["", "d"], None, ["e"], [], ["f", "g", "h"], ["i"], ["j", ""], [], ["k"], ["l"], None, ["m", "n"], ["o"], ["p"], ["q", "r"], [""], ["s", "t"]]
NOLIST = [[], [], None, None, [], [], None, [], [], [], None, [], None, [], [], None, [], [], []]
SEQ = ["ACGT", "A", "", "", "GG", "TTT", "C", "AC", "GTA", "", "N", "ACGTN", "", "T", "CA", "G", "TT", "ACG", "TA"]
QUAL = [[100 * i + j for j in range(len(s))] for i, s in enumerate(SEQ)]
MAP_UU = [[("a", "1")], [("b", "2"), ("c", "3")], [], [], [("d", "")], [("e", "5")], [("f", "6"), ("g", "7"), ("h", "8")], [("i", "9")], [("j", "10")], [],
          [("k", "11")], [("l", "12")], [], [("m", "13")], [("n", "14")], [("o", "15")], [("p", "16")], [("q", "17")], [("r", "18"), ("s", "19")]]
MAP_UL = [[("a", ["1"])], [("b", ["2", "3"]), ("c", [])], [], [], [("d", [""])], [("e", ["5"])], [("f", ["6", "7"]), ("g", ["8"])], [("h", [])], [("i", ["9"])], [],
          [("j", ["10"])], [("k", ["11", "12"])], [], [("l", ["13"])], [("m", [])], [("n", ["14"])], [("o", ["15"])], [("p", ["16"])], [("q", ["17"]), ("r", ["18", "19"])]]

# a column's type: ("U", nullable) Utf8, ("I",) Int64, ("L", nullable, item) List, ("S", first, second) Struct
U, UN, I = ("U", False), ("U", True), ("I",)
CASES = {  # name -> its root columns as (type, rows)
    "utf8n": [(UN, UTF8N)],
    "listn": [(("L", True, U), LISTN)],
    "nolist": [(("L", True, U), NOLIST)],
    "nolist_slab": [(("L", True, U), NOLIST)],
    "shared": [(U, SEQ), (("L", False, I), QUAL)],
    "map_uu": [(("L", False, ("S", U, U)), MAP_UU)],
    "map_ul": [(("L", False, ("S", U, ("L", False, U))), MAP_UL)],
}
CUTS = [(0, 19), (0, 8), (8, 8), (16, 3), (5, 9), (18, 1)]
ROW_LISTS = [("all", list(range(N))), ("last", [18]), ("edges", [0, 7, 8, 15, 16, 18]), ("hollow", [3, 9, 12])]  # hollow: NULL / empty rows only


def shown(v):
    if v is None:
        return "NULL"
    if isinstance(v, str):
        return '"%s"' % v
    if isinstance(v, int):
        return str(v)
    if isinstance(v, tuple):
        return shown(v[0]) + ":" + shown(v[1])
    return "[" + ",".join(shown(x) for x in v) + "]"


def sig(t, vals, view, length=None):
    """kind(length,null_count,has validity)[children] of the array of `vals`.  A view: the null count is left to the consumer (-1)
    wherever there is a bitmap, and the children are the slab's whole (vals: all rows; length: the cut's).  A gather: exact counts,
    a bitmap only where a row is NULL."""
    nullable = t[0] in "UL" and t[1]
    nulls = sum(v is None for v in vals)
    head = "%s(%d,%d,%d)" % (t[0], len(vals) if length is None else length, (-1 if nullable else 0) if view else nulls, nullable if view else nulls > 0)
    if t[0] == "L":
        return head + "[" + sig(t[2], [x for v in vals if v is not None for x in v], view) + "]"
    if t[0] == "S":
        return head + "[" + sig(t[1], [v[0] for v in vals], view) + "," + sig(t[2], [v[1] for v in vals], view) + "]"
    return head


def pad(b):
    return (b + 63) & ~63


def expected():
    out = []
    for name, cols in CASES.items():
        if name == "shared":  # offsets once (two nodes share them), the bases, the qualities: a copy fewer than buffers
            parts = [(N + 1) * 4, sum(map(len, SEQ)), 8 * sum(map(len, SEQ))]
            out.append("P shared copies=3 buffers=4 bytes=%d total=%d" % (sum(parts), 64 + sum(map(pad, parts))))
        for r0, n in CUTS:
            head = "V %s %d %d" % (name, r0, n)
            out.append(head + " sig " + " ".join(sig(t, rows, True, n) for t, rows in cols))
            out += [head + " %d\t" % i + "\t".join(shown(rows[r0 + i]) for _, rows in cols) for i in range(n)]
        for lname, idx in ROW_LISTS:
            head = "G %s %s" % (name, lname)
            out.append(head + " sig " + " ".join(sig(t, [rows[r] for r in idx], False) for t, rows in cols))
            out += [head + " %d\t" % i + "\t".join(shown(rows[r]) for _, rows in cols) for i, r in enumerate(idx)]
    return out


def test_views_gathers_and_plan_of_every_shape(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "text_export_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "exon_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "text_export_harness.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]  # (a sanitizer report ends the program with a status)
    got = r.stdout.decode().split("\n")[:-1]
    plans = [line for line in got if line.startswith("P ")]
    assert len(plans) == len(CASES)
    want = expected()
    assert [line for line in got if not line.startswith("P ") or line.startswith("P shared ")] == want
    # the item-less list: no offsets come back (a bitmap alone); a scan of large batches gets its zeros in the block instead
    assert "P nolist copies=1 buffers=1 bytes=3 total=128" in plans
    assert "P nolist_slab copies=2 buffers=1 bytes=%d total=%d" % (3 + (N + 1) * 4, 64 + 64 + pad((N + 1) * 4)) in plans
