"""GPU: exon-hip-cli runs `SELECT filter, MIN(c), MAX(c), COUNT(*) ... WHERE info."AF" <op> lit GROUP BY filter` through the
fused MIN / MAX plan (kind 8), over two VCF files whose FILTER dictionaries differ, against an expectation parsed from the text."""
import os
import subprocess

import pytest

from test_gpu_minmax_by_group import expect_by_value, write_vcf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "exon_amd", "bin", "exon-hip-cli")


def table(out):
    return [[c.strip() for c in line.strip("|").split("|")] for line in out.splitlines() if line.startswith("|")]


@pytest.mark.parametrize("arg,col", [("qual", 2), ('info."DP"', 3)])
def test_cli_min_max_by_filter(tmp_path, arg, col):
    d = tmp_path / "vcfs"
    d.mkdir()
    rows = write_vcf(str(d / "a.vcf"), 3000, 1, ["PASS", ".", "q10"]) + write_vcf(str(d / "b.vcf"), 3100, 2, ["s50", "q10;s50", "q10", ".", "PASS"])
    sql = ["SET exon.vcf_parse_info = true;" f"CREATE EXTERNAL TABLE v STORED AS VCF LOCATION '{d}';"
           f'SELECT filter, MIN({arg}), MAX({arg}), COUNT(*) FROM v WHERE info."AF" > 0.01 GROUP BY filter']
    r = subprocess.run([CLI, "-q", "-c", *sql], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    t = table(r.stdout)
    name = arg.replace('"', "")
    assert t[0] == ["filter", f"min({name})", f"max({name})", "count(*)"]
    num = int if col == 3 else float
    got = {row[0]: (num(row[1]), num(row[2]), int(row[3])) for row in t[1:]}
    want = {("[" + ", ".join(k.split(";")) + "]" if k else "[]"): (v[2], v[3], v[1]) for k, v in expect_by_value(rows, col).items()}
    assert got == want and len(got) == 5


def test_cli_min_max_null_and_refusal(tmp_path):
    p = tmp_path / "n.vcf"
    p.write_text('##fileformat=VCFv4.3\n##contig=<ID=1>\n##INFO=<ID=AF,Number=1,Type=Float,Description="x">\n'
                 "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
                 "1\t1\t.\tA\tC\t.\tPASS\tAF=0.5\n1\t2\t.\tA\tC\t.\tPASS\tAF=0.5\n1\t3\t.\tA\tC\t7.5\tq10\tAF=0.5\n")
    pre = "SET exon.vcf_parse_info = true;" f"CREATE EXTERNAL TABLE v STORED AS VCF LOCATION '{p}';"
    r = subprocess.run([CLI, "-q", "-c", pre + 'SELECT filter, MIN(qual), MAX(qual), COUNT(*) FROM v WHERE info."AF" > 0.01 GROUP BY filter'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert sorted(table(r.stdout)[1:]) == [["[PASS]", "NULL", "NULL", "2"], ["[q10]", "7.5", "7.5", "1"]]
    # a table whose files type the argument differently has no single answer column: an error, not a wrong number
    d = tmp_path / "mixed"
    d.mkdir()
    write_vcf(str(d / "a.vcf"), 200, 1, ["PASS"])
    write_vcf(str(d / "b.vcf"), 200, 2, ["PASS"], dp_type="Float")
    r = subprocess.run([CLI, "-q", "-c", "SET exon.vcf_parse_info = true;" f"CREATE EXTERNAL TABLE m STORED AS VCF LOCATION '{d}';"
                        'SELECT filter, MIN(info."DP"), MAX(info."DP"), COUNT(*) FROM m WHERE info."AF" > 0.01 GROUP BY filter'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "one stream takes one type" in r.stderr
    r = subprocess.run([CLI, "-q", "-c", pre + 'SELECT filter, MIN(qual), AVG(qual) FROM v WHERE info."AF" > 0.01 GROUP BY filter'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "MIN / MAX" in r.stderr
