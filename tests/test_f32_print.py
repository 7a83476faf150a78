"""host/f32_print.h (Rust's `{}` of an f32, usable on the device: the printer of the VCF `info` column's Float values) against
exon::rust_f32_display (host/vcf_text.h, std::to_chars) through tools/check_f32_print.cpp: every exponent with the mantissas at
its ends, the subnormals 2^k and 2^k +- 1, the neighbours of every power of ten, and every 64th of the 2^32 bit patterns --
67 112 578 values, about 12 s on one core.  The same bytes, the same length from the length-only mode, nothing written behind it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_f32_print_equals_rust_f32_display(tmp_path):
    exe = tmp_path / "check_f32_print"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "check_f32_print.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    m = re.search(r"checked (\d+), longest (\d+), mismatches (\d+)", r.stdout)
    assert r.returncode == 0 and m, r.stdout + r.stderr
    assert int(m.group(1)) == 67_112_578 and int(m.group(3)) == 0
    assert int(m.group(2)) == 48  # kF32PrintMax, reached ("-0." + 45 places)


def test_f32_print_table_is_what_its_script_prints():
    out = subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_f32_print_table.py")], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "exon_amd", "csrc", "host", "f32_print.h")).read()
    assert out.count("\n") == 77 and out in header
