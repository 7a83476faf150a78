"""CPU: EXON_HIP_PROJECT_VCF_FORMATS_ON_DEVICE (32), the modifier that lets a gpu_parse scan print the VCF `formats` column on the
device: what the open accepts, that it adds no column, and that the new entry points are declared, exported and bound."""
import ctypes as C
import os
import re

import pytest

import exon_amd
from exon_amd import _lib as L
from test_scan_projection import FX, table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCF = os.path.join(FX, "vcf", "index.vcf")


def open_rc(fmt, path, projection, gpu_parse=0):
    lib = L.load()
    opt = L.ScanOptions(L.FORMATS[fmt], 0, 0, None, None, 0, gpu_parse, projection)
    h = C.c_void_p()
    rc = lib.exon_hip_scan_open(path.encode(), C.byref(opt), C.byref(h))
    if rc == 0:
        lib.exon_hip_scan_close(h)
    return rc


def test_the_modifier_needs_the_formats_bit_and_is_no_bit_of_other_formats():
    assert open_rc("vcf", VCF, 32) == -1 and open_rc("vcf", VCF, 32 | 8) == -1 and open_rc("vcf", VCF, 32, gpu_parse=1) == -1  # EXON_HIP_EINVAL
    assert "EXON_HIP_PROJECT_VCF_FORMATS" in L.load().exon_hip_last_error(None).decode()
    assert open_rc("vcf", VCF, 48) == 0 and open_rc("vcf", VCF, 63) == 0 and open_rc("vcf", VCF, 48, gpu_parse=1) == 0
    assert open_rc("vcf", VCF, 64) == -1 and open_rc("vcf", VCF, 64 | 48) == -1
    assert open_rc("bcf", os.path.join(FX, "bcf", "index.bcf"), 32) == -1 and open_rc("bcf", os.path.join(FX, "bcf", "index.bcf"), 48) == -1
    assert open_rc("bam", os.path.join(FX, "bam", "test.bam"), 32) == -1 and open_rc("sam", os.path.join(FX, "sam", "test.sam"), 32) == -1
    assert open_rc("fastq", os.path.join(FX, "fastq", "test.fastq"), 32) == -4


def test_scan_takes_the_option_only_next_to_formats():
    with pytest.raises(exon_amd.ExonHipError):
        exon_amd.Scan(VCF, "vcf", project=("info",), formats_on_device=True)
    with pytest.raises(exon_amd.ExonHipError):
        exon_amd.Scan(VCF, "vcf", formats_on_device=True)
    with pytest.raises(ValueError):
        exon_amd.Scan(os.path.join(FX, "bam", "test.bam"), "bam", project=("name",), formats_on_device=True)
    assert "formats_on_device" not in exon_amd.Scan.PROJECT["vcf"] and 32 not in exon_amd.Scan.PROJECT["vcf"].values()  # a modifier, not a column
    exon_amd.Scan(VCF, "vcf", project=("formats",), formats_on_device=True).close()


@pytest.mark.parametrize("project", [("formats",), ("id", "ref", "alt", "info", "formats")])
def test_a_host_reader_scan_with_the_modifier_serves_what_one_without_it_serves(project):
    """the host reader knows the five column bits alone: same schema, same batches"""
    gpu_parse = False  # (a gpu_parse scan with the modifier stays one: it serves batches once a context is bound, like `info`)
    for path in (VCF, VCF + ".gz"):
        a = exon_amd.Scan(path, "vcf", batch_size=100, gpu_parse=gpu_parse, project=project)
        b = exon_amd.Scan(path, "vcf", batch_size=100, gpu_parse=gpu_parse, project=project, formats_on_device=True)
        sa, sb = a.schema(), b.schema()
        names = [sa.field(i).name for i in range(sa.num_fields)]
        assert names == [sb.field(i).name for i in range(sb.num_fields)] and names[-len(project):] == list(project)
        assert [str(sa.field(i).type) for i in range(sa.num_fields)] == [str(sb.field(i).type) for i in range(sb.num_fields)]
        ba, bb = list(a), list(b)
        assert [len(x) for x in ba] == [len(x) for x in bb] and sum(len(x) for x in ba) == 621
        for x, y in zip(ba, bb):
            assert x.equals(y)
        a.close()
        b.close()
    c = table(exon_amd.Scan(VCF, "vcf", project=("formats",), formats_on_device=True))
    assert c["formats"][0] == "GT:PL:PG\t0/0:0,3,26:0"


def test_the_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "exon_hip.h")).read()
    assert re.search(r"#define EXON_HIP_PROJECT_VCF_FORMATS_ON_DEVICE 32ull", header)
    lib = L.load()
    for name in ("exon_hip_vcf_parser_set_format_key_types", "exon_hip_vcf_parser_formats_text"):
        assert re.search(r"\bint " + name + r"\(exon_hip_vcf_parser\*", header), name
        assert getattr(lib, name).argtypes  # exported by the library, typed by _lib.py
        assert name in open(os.path.join(ROOT, "exon_amd", "_lib.py")).read()
        assert f"pub fn {name}(" in open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    assert L.PROJECT_VCF_FORMATS_ON_DEVICE == 32 and lib.exon_hip_abi_version() == 5
    import inspect
    assert "formats_on_device" in inspect.signature(exon_amd.Scan.__init__).parameters
    assert "format_key_types" in inspect.signature(exon_amd.VCFParser.__init__).parameters
    assert "formats_text" in inspect.signature(exon_amd.VCFParser.parse_host).parameters
