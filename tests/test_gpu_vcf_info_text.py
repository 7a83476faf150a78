"""The VCF `info` Utf8 column out of the GPU pipeline (text_columns.hip: k_vcf_info_measure / k_vcf_info_fill, the device printer
of host/f32_print.h, the key-type table) -- the reference's unparsed `info`, which is the parsed entries PRINTED AGAIN
(exon-vcf/src/array_builder/lazy_array_builder.rs:216-297).

Expectations come from oracle/decode.py (info_string, rust_f32_display), from numpy's format_float_positional(unique=True) and
from strings spelled out here; the host reader is compared against only where the test is about the batches being the same.
File-level tests go through Scan(..., gpu_parse=True, project=(... "info" ...)).bind_ctx(ctx), parser-level ones through
VCFParser.parse_host(..., info_text=True)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import exon_amd
from oracle import decode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "ref_fixtures")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")

KEY_TYPES = {"XF": "f", "XL": "f", "XI": "i", "XJ": "i", "XB": "b", "XC": "c", "XD": "c", "XS": "s"}
TYPE_NAMES = {"f": "Float", "i": "Integer", "b": "Flag", "c": "Character", "s": "String"}
COLS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def head(key_types=KEY_TYPES, pad=None):
    """a header that types `key_types`; pad: a ##pad line of that many x, which moves the data lines by as many bytes"""
    h = "##fileformat=VCFv4.2\n##contig=<ID=1>\n"
    if pad is not None:
        h += "##pad=" + "x" * pad + "\n"
    for k, t in key_types.items():
        h += f"##INFO=<ID={k},Number={'0' if t == 'b' else '.'},Type={TYPE_NAMES[t]},Description=\"{t}\">\n"
    return h + COLS


def line(i, info, rid=".", ref="A", alt="C"):
    return f"1\t{i + 1}\t{rid}\t{ref}\t{alt}\t.\t.\t{info}\n"


def write_vcf(path, infos, **kw):
    with open(path, "w") as f:
        f.write(head(**kw) + "".join(line(i, x) for i, x in enumerate(infos)))
    return str(path)


def table(scan):
    cols = {}
    for b in scan:
        for i in range(b.type.num_fields):
            cols.setdefault(b.type.field(i).name, []).extend(b.field(i).to_pylist())
    return cols


def oracle_info(path):
    v = decode.decode_vcf(str(path))
    return [decode.info_string(v, i) for i in range(len(v["chrom"]))]


def gpu_scan(ctx, path, project=("info",), **kw):
    """-> (columns, decoded on the GPU?)"""
    s = exon_amd.Scan(str(path), "vcf", gpu_parse=True, project=project, **kw).bind_ctx(ctx)
    c = table(s)
    on = s.decoded_on_gpu()[0]
    s.close()
    return c, on


def parser_info(ctx, infos, misalign=0, key_types=KEY_TYPES, par=None):
    """-> (the column's strings or None, n_undecided of the info column) through the parser-level entry points"""
    text = "".join(line(i, x) for i, x in enumerate(infos)).encode()
    own = par is None
    if own:
        par = exon_amd.VCFParser(ctx, ["1"], max_slab_bytes=len(text) + 4096, key_types=key_types)
    res = par.parse_host(text, misalign=misalign, info_text=True)
    if own:
        par.close()
    assert res["n_rows"] == len(infos) and res["n_undecided"] == 0
    it = res["info_text"]
    if it["n_undecided"]:
        return None, it["n_undecided"]
    off, val = it["offsets"], it["values"].tobytes()
    assert off[0] == 0 and off[-1] == it["n_bytes"] == len(val)
    return [val[off[i]:off[i + 1]].decode() for i in range(len(infos))], 0


# rows that touch every branch of the walk, lengths 0 .. ~70; period 11 (coprime to 64 and to 16)
MIX = ["XF=0.50;XB", ".", "XL=1e-5,.,1.0;XI=007", "XS=a,b,.;XC=q", "XD=a,.,b;XJ=+5,.,-3", "", "DB;AF=0.010;ZZ=0.50", "XB;XB;XB=7",
       "XF=16777217;XI=-2147483648;;", "XL=3.4028235e38,-0,1e-45;XS=x", "XI=0"]
MIX_WANT = ["XF=0.5;XB=true", "", "XL=0.00001,.,1;XI=7", "XS=a,b,.;XC=q", "XD=a,b;XJ=5,.,-3", "", "DB=true;AF=0.01;ZZ=0.50", "XB=true;XB=true;XB=true",
            "XF=16777216;XI=-2147483648", "XL=340282350000000000000000000000000000000,-0,0.000000000000000000000000000000000000000000001;XS=x", "XI=0"]


def mix(n):
    return [MIX[i % 11] for i in range(n)], [MIX_WANT[i % 11] for i in range(n)]


# ---- fixtures and spelled-out rows ---------------------------------------------------------------------------------------------
def test_gpu_info_text_of_the_reference_fixture(ctx, tmp_path):
    """index.vcf, index.vcf.gz and a BGZF copy of index.vcf: 621 rows = decode.info_string; the first rows = slt/vcf-select-tests.slt:6-16
    (the strings test_scan_projection.py quotes).  (Before the device printer existed bind_ctx refused this scan.)"""
    p = os.path.join(FX, "vcf", "index.vcf")
    bg = tmp_path / "copy.vcf.gz"
    subprocess.check_call([BGZIP, p, str(bg), "6"])
    for path in (p, p + ".gz", str(bg)):
        c, on = gpu_scan(ctx, path, batch_size=64)
        assert on
        assert c["info"][:2] == ["DP=1;I16=1,0,0,0,26,676,0,0,60,3600,0,0,0,0,0,0;QS=1,0;MQ0F=0",
                                 "DP=1;I16=1,0,0,0,34,1156,0,0,60,3600,0,0,1,1,0,0;QS=1,0;MQ0F=0"]
        assert len(c["info"]) == 621 and c["info"] == oracle_info(path)


def test_gpu_info_text_is_printed_again_not_copied(ctx, tmp_path):
    """the INFO part of test_host_vcf_info_and_formats_text_are_printed_again_not_copied, same exact strings"""
    infos = ["XF=0.50;XL=1e-5,.,1.0,-0,123456790528,3.4028235e38;XI=007;XJ=+5,.,-3;XB;XC=q;XD=a,.,b;XS=a,b,.;AF=0.010;DB;ZZ=0.50",
             ".", "XF=16777217;XI=-2147483648", "XF=nan;XL=inf,-inf", "XS=only"]
    want = ["XF=0.5;XL=0.00001,.,1,-0,123456790000,340282350000000000000000000000000000000;XI=7;XJ=5,.,-3;XB=true;XC=q;"
            "XD=a,b;XS=a,b,.;AF=0.01;DB=true;ZZ=0.50", "", "XF=16777216;XI=-2147483648", "XF=NaN;XL=inf,-inf", "XS=only"]
    p = write_vcf(tmp_path / "text.vcf", infos)
    c, on = gpu_scan(ctx, p)
    assert on and c["info"] == want == oracle_info(p)
    got, und = parser_info(ctx, ["XL=NAN,+Inf,-INFINITY,infinity,-nan"])
    assert und == 0 and got == ["XL=NaN,inf,-inf,inf,NaN"]


# ---- row counts and alignment --------------------------------------------------------------------------------------------------
def test_gpu_info_text_row_counts_and_misalignment_parser_level(ctx):
    par = exon_amd.VCFParser(ctx, ["1"], max_slab_bytes=1 << 20, key_types=KEY_TYPES)
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        infos, want = mix(n)
        for k in range(16):
            got, und = parser_info(ctx, infos, misalign=k, par=par)
            assert und == 0 and got == want, (n, k)
    par.close()


@pytest.mark.parametrize("pad", range(16))
def test_gpu_info_text_row_counts_and_line_start_residues_file_level(ctx, tmp_path, pad):
    n = (1, 63, 64, 65, 255, 256, 257, 513)[pad % 8]
    infos, want = mix(n)
    p = write_vcf(tmp_path / "rows.vcf", infos, pad=pad)
    c, on = gpu_scan(ctx, p, batch_size=100)
    assert on and c["info"] == want and c["pos"] == list(range(1, n + 1))


# ---- the printer on the device -------------------------------------------------------------------------------------------------
def printer_bits():
    rng = np.random.default_rng(7)
    b = []
    for e in range(255):  # every finite exponent, the mantissas at its ends and in the middle
        for m in (0, 1, 2, 1 << 22, (1 << 23) - 2, (1 << 23) - 1):
            b += [e << 23 | m, 1 << 31 | e << 23 | m]
    for k in range(23):  # subnormals 2^k, 2^k +- 1
        b += [x for x in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 < x < 1 << 23]
    for k in range(-45, 39):  # the neighbours of every power of ten
        c = int(np.array([float(f"1e{k}")], np.float32).view(np.uint32)[0])
        b += [c - 1, c, c + 1]
    b = np.array(b, np.uint64).astype(np.uint32)
    rnd = rng.integers(0, 2**32, 20_000, dtype=np.uint64).astype(np.uint32)
    f = np.concatenate([b, rnd]).view(np.float32)
    f = f[np.isfinite(f)]
    # values whose shortest form has nd = 1 .. 9 digits.  Up to 7: nd random digits (no trailing zero) times a power of ten inside
    # the normals, kept when that IS the shortest form; 8 and 9 (few decimals of that length are the shortest form of their f32):
    # picked from random bit patterns
    def n_digits(x):
        return len(np.format_float_scientific(x, unique=True).split("e")[0].replace(".", "").replace("-", "").rstrip("0") or "0")

    short = []
    for nd in range(1, 8):
        d = rng.integers(10 ** (nd - 1), 10 ** nd, 4000)
        d = d[d % 10 != 0]
        e = rng.integers(-30, 30 - nd, len(d))
        keep = [x for x in np.array([float(f"{a}e{x}") for a, x in zip(d, e)], np.float32) if n_digits(x) == nd]
        assert len(keep) > 1000, nd
        short += keep
    pool = rng.integers(0, 2**32, 300_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    pool = pool[np.isfinite(pool)]
    for nd in (8, 9):
        keep = [x for x in pool if n_digits(x) == nd][:3000]
        assert len(keep) == 3000, nd
        short += keep
    return np.concatenate([f, np.array(short, np.float32)])


def test_gpu_info_text_float_printer_against_numpy_and_the_oracle(ctx):
    f = printer_bits()
    assert 50_000 < len(f) < 70_000
    spelled = [np.format_float_scientific(x, unique=True) for x in f]
    infos = ["XL=" + ",".join(spelled[i:i + 64]) for i in range(0, len(f), 64)]
    got, und = parser_info(ctx, infos)
    assert und == 0  # (all inside dec::parse_f32's domain: at most 9 digits, exponents -45 .. 38)
    items = [x for row in got for x in row[3:].split(",")]
    assert all(row.startswith("XL=") for row in got) and len(items) == len(f)
    assert items == [decode.rust_f32_display(x) for x in f]
    assert items == [np.format_float_positional(x, unique=True, trim="-") for x in f]
    assert max(len(x) for x in items) == 48  # "-0." + 45 places: the bound host/f32_print.h states


# ---- integers ------------------------------------------------------------------------------------------------------------------
def test_gpu_info_text_integers_at_the_i32_borders(ctx, tmp_path):
    infos = ["XI=2147483647", "XI=-2147483648", "XI=+2147483647", "XI=007", "XI=+5", "XI=-0", "XI=-007", "XJ=0000000000002147483647,.,-00", "XJ=1,2,3"]
    want = ["XI=2147483647", "XI=-2147483648", "XI=2147483647", "XI=7", "XI=5", "XI=0", "XI=-7", "XJ=2147483647,.,0", "XJ=1,2,3"]
    p = write_vcf(tmp_path / "ints.vcf", infos)
    c, on = gpu_scan(ctx, p)
    assert on and c["info"] == want == oracle_info(p)


@pytest.mark.parametrize("bad", ["XI=2147483648", "XI=+2147483648", "XI=-2147483649", "XI=1x", "XI=-", "XJ=1,,2", "XI=99999999999999999999"])
def test_gpu_info_text_integers_the_device_hands_over_and_the_host_refuses(ctx, tmp_path, bad):
    infos = ["XI=1"] * 70 + [bad] + ["XI=2"] * 70
    got, und = parser_info(ctx, infos)
    assert got is None and und == 1
    p = write_vcf(tmp_path / "bad.vcf", infos)
    with pytest.raises(exon_amd.ExonHipError):
        gpu_scan(ctx, p)
    with pytest.raises(ValueError):
        oracle_info(p)


# ---- types and keys ------------------------------------------------------------------------------------------------------------
def test_gpu_info_text_types_and_keys(ctx, tmp_path):
    long_key = "K" * 300
    types = dict(KEY_TYPES, Q="i", **{long_key: "f"})
    rows = [
        ("XB;XB=1;XB=.", "XB=true;XB=true;XB=true"),                       # a Flag prints key=true whatever follows it
        ("XD=a,.,b,.;XD=.,.;XC=x;XC=,", "XD=a,b;XD=;XC=x;XC=,"),            # Character lists drop '.' items
        ("XS=a,b,.,0.50;XS=...;XS=1e5", "XS=a,b,.,0.50;XS=...;XS=1e5"),     # String values are copied
        ("AF=0.50,1e-3;DP=007;DB;END=0100", "AF=0.5,0.001;DP=7;DB=true;END=100"),  # reserved keys the header does not declare
        ("ZZ=0.50;NOVEL;MQ=1e1;MQ0=01", "ZZ=0.50;NOVEL=true;MQ=10;MQ0=1"),  # an unknown key is a String
        ("A=1.0;AF=1.0;AF2=1.0;AFF=1.0", "A=1.0;AF=1;AF2=1.0;AFF=1.0"),     # keys that are prefixes of each other
        ("Q=01;" + long_key + "=0.50", "Q=1;" + long_key + "=0.5"),        # key lengths 1 and 300
        ("XI=1;;XB;", "XI=1;XB=true"), (";;XI=2", "XI=2"), ("XI=3;", "XI=3"),
        (".", ""), ("", ""), ("=5;XI=4", "=5;XI=4"),
        ("XL=1,.,2.50;XJ=.,.", "XL=1,.,2.5;XJ=.,."),
    ]
    infos, want = [r[0] for r in rows], [r[1] for r in rows]
    p = write_vcf(tmp_path / "types.vcf", infos, key_types=types)
    c, on = gpu_scan(ctx, p)
    assert on and c["info"] == want == oracle_info(p)
    got, und = parser_info(ctx, infos, key_types=types)
    assert und == 0 and got == want
    # a header that types a reserved key itself: DP a String, AF an Integer, DB a String
    retyped = dict(KEY_TYPES, DP="s", AF="i", DB="s")
    infos = ["DP=007;AF=010;DB=x;END=01", "DP=1.50"]
    want = ["DP=007;AF=10;DB=x;END=1", "DP=1.50"]
    p = write_vcf(tmp_path / "retyped.vcf", infos, key_types=retyped)
    c, on = gpu_scan(ctx, p)
    assert on and c["info"] == want == oracle_info(p)
    # no ##INFO line at all: the reserved keys alone
    got, und = parser_info(ctx, ["DP=007;XI=007;DB"], key_types={})
    assert und == 0 and got == ["DP=7;XI=007;DB=true"]


@pytest.mark.parametrize("bad", ["XF=.", "XI", "XI=", "XS=.", "XS", "XF=1;ZZ", "XF=0.1234567890123456789012345", "XF=1e", "XF=0x10", "XS=é"])
def test_gpu_info_text_rows_the_device_leaves_to_the_host_reader(ctx, bad):
    got, und = parser_info(ctx, ["XB"] * 65 + [bad])
    assert got is None and und == 1


# ---- expansion -----------------------------------------------------------------------------------------------------------------
LONG = "XL=" + ",".join(["1e38"] * 50) + ";XB;DB"
LONG_WANT = "XL=" + ",".join(["1" + "0" * 38] * 50) + ";XB=true;DB=true"


@pytest.mark.parametrize("n_long,n_short", [(300, 0), (5000, 60000)])
def test_gpu_info_text_longer_than_the_slab(ctx, tmp_path, monkeypatch, n_long, n_short):
    """printed `info` of more than 4x the text, below the values buffer's first size (1 MiB) and, with 1 MiB slabs, far beyond it;
    then shorter slabs behind the long ones"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    infos = [LONG] * n_long + ["XI=07"] * n_short
    want = [LONG_WANT] * n_long + ["XI=7"] * n_short
    p = write_vcf(tmp_path / "long.vcf", infos)
    printed_long, text_long = n_long * len(LONG_WANT), n_long * len(line(0, LONG))
    assert printed_long > 4 * text_long and (printed_long < 1 << 20) == (n_short == 0)
    assert (os.path.getsize(p) > 2 << 20) == (n_short != 0)
    c, on = gpu_scan(ctx, p, batch_size=4096)
    assert on and c["info"] == want


# ---- batches -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch_file(tmp_path_factory):
    """30 000 rows, about 1.3 MB: two slabs of 1 MiB; ids / refs / alts / infos of their own rhythms"""
    p = tmp_path_factory.mktemp("info_batches") / "b.vcf"
    ids, refs, alts = [".", "rs1", "a;b;c"], ["A", "ACGT", "GG", "T", "CCCCCCC"], [".", "C", "C,GT"]
    with open(p, "w") as f:
        f.write(head(KEY_TYPES))
        for i in range(30000):
            f.write(line(i, MIX[i % 11] if i % 11 != 5 else "XI=%d" % i, ids[i % 3], refs[i % 5], alts[(i // 2) % 3]))
    host = {}
    for r in range(1, 5):
        for proj in itertools.combinations(("id", "ref", "alt", "info"), r):
            s = exon_amd.Scan(str(p), "vcf", project=proj)
            names = [s.schema().field(i).name for i in range(s.schema().num_fields)]
            host[proj] = (names, table(s))
            s.close()
    return str(p), host


@pytest.mark.parametrize("batch_size", [777, 8192])
def test_gpu_info_text_batches_equal_the_host_readers_for_every_projection(ctx, batch_file, monkeypatch, batch_size):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    path, host = batch_file
    want_info = oracle_info(path)
    for proj, (names, cols) in host.items():
        s = exon_amd.Scan(path, "vcf", gpu_parse=True, project=proj, batch_size=batch_size).bind_ctx(ctx)
        assert [s.schema().field(i).name for i in range(s.schema().num_fields)] == names
        sizes, got = [], {}
        for b in s:
            sizes.append(len(b))
            assert [b.type.field(i).name for i in range(b.type.num_fields)] == names  # the host reader's column order
            for i, k in enumerate(names):
                got.setdefault(k, []).extend(b.field(i).to_pylist())
        assert s.decoded_on_gpu()[0], proj
        s.close()
        assert sum(sizes) == 30000 and max(sizes) <= batch_size and len(sizes) > 30000 // batch_size
        for k in names:
            assert got[k] == cols[k], (proj, k)
        if "info" in proj:
            assert got["info"] == want_info


def test_gpu_info_text_next_to_typed_info_fields(ctx, tmp_path, monkeypatch):
    """typed INFO columns (Number=1 Float / Integer, a Flag: the kinds the device decodes) and the `info` text of the same field"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    p = tmp_path / "typed.vcf"
    with open(p, "w") as f:
        f.write(head(KEY_TYPES).replace("ID=XF,Number=.", "ID=XF,Number=1").replace("ID=XI,Number=.", "ID=XI,Number=1"))
        for i in range(40000):
            f.write(line(i, MIX[i % 11] if i % 11 != 5 else "XI=%d;XF=%d.50" % (i, i)))
    assert os.path.getsize(p) > (1 << 20) and "ID=XF,Number=1,Type=Float" in open(p).read(600)
    c, on = gpu_scan(ctx, p, project=("ref", "info"), info_field="XF,XI,XB", batch_size=5000)
    h = table(exon_amd.Scan(str(p), "vcf", project=("ref", "info"), info_field="XF,XI,XB"))
    assert on and list(c) == list(h) and c["info"] == oracle_info(p)
    assert c["info"][5] == "XI=5;XF=5.5" and c["info"][16] == "XI=16;XF=16.5"
    for k in h:
        assert c[k] == h[k], k


# ---- a pushed-down region ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_gpu_info_text_under_a_pushed_down_region(ctx, tmp_path, monkeypatch, order):
    """a sorted file keeps one run of rows per slab (views), a shuffled one rows here and there (the gather)"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    n = 40000
    pos = np.arange(1, n + 1)
    if order == "shuffled":
        pos = np.random.default_rng(3).permutation(pos)
    p = tmp_path / "region.vcf"
    with open(p, "w") as f:
        f.write(head(KEY_TYPES))
        for i, q in enumerate(pos):
            f.write(f"1\t{q}\t.\tA\tC\t.\t.\tXI={q:05d}" + (";" + MIX[i % 11] if MIX[i % 11] not in (".", "") else "") + "\n")
    lo, hi = 9000, 31000
    c, on = gpu_scan(ctx, p, region=f"1:{lo}-{hi}", batch_size=3000)
    keep = [i for i, q in enumerate(pos) if lo <= q <= hi]
    want = [f"XI={pos[i]}" + (";" + MIX_WANT[i % 11] if MIX_WANT[i % 11] else "") for i in keep]
    assert on and c["pos"] == [int(pos[i]) for i in keep] and c["info"] == want and len(want) == hi - lo + 1


# ---- hand-over -----------------------------------------------------------------------------------------------------------------
def handover_file(tmp_path, odd):
    infos = [MIX[i % 11] if i % 11 != 5 else "XI=%d" % i for i in range(60000)]  # about 2 MB: the odd row lies in the second slab
    infos[45001] = odd
    return write_vcf(tmp_path / "handover.vcf", infos), infos


def test_gpu_info_text_a_float_of_25_digits_hands_the_file_over(ctx, tmp_path, monkeypatch):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    p, infos = handover_file(tmp_path, "XF=0.1234567890123456789012345")
    c, on = gpu_scan(ctx, p, project=("ref", "info"), batch_size=1000)
    h = table(exon_amd.Scan(p, "vcf", project=("ref", "info"), batch_size=1000))
    assert not on
    assert c["pos"] == list(range(1, 60001))  # nothing lost, nothing doubled
    for k in h:
        assert c[k] == h[k], k
    assert c["info"][45001] == "XF=0.12345679" and c["info"][45000] == MIX_WANT[45000 % 11] and c["info"][45002] == MIX_WANT[45002 % 11]


def test_gpu_info_text_a_missing_value_raises_on_both_paths(ctx, tmp_path, monkeypatch):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    p, _ = handover_file(tmp_path, "XF=.")
    with pytest.raises(exon_amd.ExonHipError):
        gpu_scan(ctx, p)
    with pytest.raises(exon_amd.ExonHipError):
        table(exon_amd.Scan(p, "vcf", project=("info",)))


# ---- formats stays host-only ---------------------------------------------------------------------------------------------------
def test_gpu_scan_with_formats_still_decodes_on_the_host(ctx):
    p = os.path.join(FX, "vcf", "index.vcf.gz")
    s = exon_amd.Scan(p, "vcf", batch_size=100, gpu_parse=True, project=("info", "formats"))
    with pytest.raises(exon_amd.ExonHipError):
        s.bind_ctx(ctx)
    c = table(s)
    assert not s.decoded_on_gpu()[0]
    s.close()
    v = decode.decode_vcf(p)
    assert c["info"] == [decode.info_string(v, i) for i in range(621)]
    assert c["formats"] == [decode.formats_string(v, i) for i in range(621)]
