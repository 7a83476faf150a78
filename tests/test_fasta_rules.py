"""CPU: the FASTA rules.  The host reader (exon_amd/csrc/host/formats.h: FASTABatchReader + FASTAArrayBuilder) is the yardstick the
GPU pipeline is held to; here it is held to tests/fasta_expect.py, the plain-Python restatement of the rules, a case per rule.  And
the public surface names the device parser: header, ctypes prototypes, exon_amd.FASTAParser."""
import gzip
import os
import re

import pytest

import exon_amd
import fasta_expect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ref_fixtures", "fasta")


def host_columns(path, **kw):
    s = exon_amd.Scan(str(path), "fasta", **kw)
    try:
        fields = [f.name for f in s.schema()]
        batches = list(s)
    finally:
        s.close()
    assert fields == ["id", "description", "sequence"]
    for b in batches:
        b.validate(full=True)
    return {name: [v for b in batches for v in b.field(k).to_pylist()] for k, name in enumerate(fields)}


CASES = {
    "plain": b">a one\nACGT\nAC\n>b\nGG\n",
    "empty id": b"> only a description\nAC\n>\nGT\n",
    "tab after the id": b">id1\tdesc with\ttabs\nACGT\n",
    "run of blanks": b">id1 \t  \t desc  tail \nAC GT\n",
    "trailing blank, NULL description": b">id1 \nAC\n>id2\t\t\nGT\n>id3   \n",
    "CRLF": b">id1 d\r\nACGT\r\nAC\r\n>id2\r\n\r\nGG\r\n",
    "a lone CR line": b">id1\nAC\n\r\nGT\n",
    "empty lines inside a record": b">id1\n\nAC\n\n\nGT\n\n>id2\n\n",
    "a record without sequence lines": b">id1\n>id2 d\n>id3\nAC\n>id4\n",
    "no final newline": b">id1 d\nACGT\n>id2\nGG",
    "no final newline on a definition": b">id1 d\nACGT\n>id2 last",
    "text in front of the first record": b"; a comment\n\nACGT\n>id1\nAC\n",
    "'>' inside a sequence line": b">id1\nAC>GT\n >id2 is no definition\n>id3\nA>\n",
    "inner blanks are kept": b">id1\n AC GT \n\tAC\n",
    "nothing at all": b"",
    "no record": b"ACGT\nAC\n",
}


@pytest.mark.parametrize("name", list(CASES))
def test_host_reader_follows_the_rules(tmp_path, name):
    text = CASES[name]
    p = tmp_path / "t.fasta"
    p.write_bytes(text)
    want = fasta_expect.columns(text)
    assert host_columns(p) == want, name
    assert host_columns(p, batch_size=1) == want, name
    gz = tmp_path / "t.fasta.gz"
    gz.write_bytes(gzip.compress(text))
    assert host_columns(gz) == want, name


def test_expectation_states_the_rules():
    """the restatement itself, on values written out by hand"""
    assert fasta_expect.records(b">id1 \t d e \r\nAC\r\n\r\n G T\r\n>\n>x\tq\nA>C") == [("id1", "d e ", "AC G T"), ("", None, ""), ("x", "q", "A>C")]
    assert fasta_expect.records(b"junk\n>a\n") == [("a", None, "")]
    s = fasta_expect.slab(b">a d\r\nAC\r\nG\n>b\nTT\n>c", final=False)  # (">c" is no line yet: ">b" is the last definition line)
    assert s == {"n_records": 1, "consumed": 12, "definitions": [b"a d"], "seq_len": [3]}
    s = fasta_expect.slab(b">a d\r\nAC\r\nG\n>b\nTT\n>c\nA", final=False)
    assert s == {"n_records": 2, "consumed": 18, "definitions": [b"a d", b"b"], "seq_len": [3, 2]}
    s = fasta_expect.slab(b">a\nAC\n>b\n", final=True)
    assert s == {"n_records": 2, "consumed": 9, "definitions": [b"a", b"b"], "seq_len": [2, 0]}
    assert fasta_expect.slab(b">a\nAC\nGT\n", final=False)["consumed"] == 0


@pytest.mark.parametrize("name", ["test.fasta", "test.fasta.gz"])
def test_host_reader_on_the_reference_fixtures(name):
    p = os.path.join(FIX, name)
    text = gzip.open(p).read() if name.endswith(".gz") else open(p, "rb").read()
    got = host_columns(p)
    assert got == fasta_expect.columns(text) and len(got["id"]) > 0


def test_public_surface_names_the_device_parser():
    hdr = open(os.path.join(ROOT, "include", "exon_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = exon_amd._lib.SIGNATURES
    lib = exon_amd.load()
    for fn in ("exon_hip_fasta_parser_create", "exon_hip_fasta_parser_parse", "exon_hip_fasta_parser_destroy"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(", code), fn + " is not declared in include/exon_hip.h"
        assert hasattr(lib, fn), fn + " is not exported by the library"
        assert fn in protos and getattr(lib, fn).argtypes, fn + " has no ctypes prototype in exon_amd/_lib.py"
    assert "typedef struct exon_hip_fasta_views" in code
    # the struct of _lib.py has the header's fields, in the header's order
    body = re.search(r"typedef struct exon_hip_fasta_views\s*\{(.*?)\}\s*exon_hip_fasta_views;", code, re.S).group(1)
    c_fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert [f for f, _ in exon_amd._lib.FASTAViews._fields_] == c_fields
    assert exon_amd.FASTAParser is exon_amd.engine.FASTAParser and hasattr(exon_amd.FASTAParser, "parse_host")
    assert "FASTA 0 id 1 description? 2 sequence" in hdr and "#define EXON_HIP_FORMAT_FASTA 4" in hdr
    assert lib.exon_hip_abi_version() == 5
