"""The VCF `formats` Utf8 column out of the GPU pipeline (text_columns.hip: the tab index, k_fmt_rows, k_fmt_sample_measure,
k_fmt_head_fill / k_fmt_sample_fill -- a thread a SAMPLE; host/vcf_sample_walk.h) -- the reference's unparsed `formats`, which is
FORMAT, a TAB and the samples PRINTED AGAIN (exon-vcf/src/array_builder/lazy_array_builder.rs:310-423).  The column is opt-in:
Scan(..., project=(..., "formats"), formats_on_device=True).

Expectations come from oracle/decode.py (formats_string) and from strings spelled out here; the host reader is compared against
only where the test is about both paths serving the same batches.  File-level tests go through
Scan(..., gpu_parse=True, formats_on_device=True).bind_ctx(ctx), parser-level ones through VCFParser.parse_host(..., formats_text=True)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import exon_amd
import vcf_formats_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "ref_fixtures")
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")


def table(scan):
    cols = {}
    for b in scan:
        for i in range(b.type.num_fields):
            cols.setdefault(b.type.field(i).name, []).extend(b.field(i).to_pylist())
    return cols


def gpu_scan(ctx, path, project=("formats",), **kw):
    """-> (columns, decoded on the GPU?)"""
    s = exon_amd.Scan(str(path), "vcf", gpu_parse=True, project=project, formats_on_device=True, **kw).bind_ctx(ctx)
    c = table(s)
    on = s.decoded_on_gpu()[0]
    s.close()
    return c, on


# ---- the 300-row mix: every branch of the walk, 0 - 70 samples a row; printed once by the oracle, shared -----------------------------
def sample_of(r, k, floats):
    gt = ("0/1", "1|1", "0|0", "./.", "1/2", "00|01")[(r + k) % 6]
    return f"{gt}:{(r * 7 + k) % 100:02d}:{k % 50},0{r % 10},{(r + k) % 300}" + (f":0.{(r + k) % 10}0" if floats else "")


def mix_rows(n=300):
    counts = [0, 1, 2, 3, 0, 5, 1, 0, 17, 2, 70, 1, 3]
    rows = []
    for r in range(n):
        c = counts[r % 13]
        if r % 13 == 4:
            rows.append((".", ["0/1:1:2"] * 2))          # FORMAT '.': "\t", whatever follows
        elif c == 0:
            rows.append((None, []))                      # no FORMAT field
        elif r % 13 == 11:
            rows.append(K.LIMITS[(r // 13) % 10][:2])    # genotypes at their limits
        else:
            floats = r % 2 == 0
            rows.append(("GT:DP:XP:XQ" if floats else "GT:DP:XP", [sample_of(r, k, floats) for k in range(c)]))
    return rows


@pytest.fixture(scope="module")
def mix(tmp_path_factory):
    """-> (rows, the oracle's strings)"""
    rows = mix_rows()
    want = K.oracle_formats(K.write_vcf(tmp_path_factory.mktemp("fmt_mix") / "mix.vcf", rows))
    assert None not in want and want[0] == "\t" and want[4] == "\t" and want[1] == "GT:DP:XP\t1|1:7:0,1,1"
    return rows, want


def cycle_file(path, mix, n, infos=None, ids=None):
    rows, want = mix
    with open(path, "w") as f:
        f.write(K.HEAD)
        for i in range(n):
            fmt, samples = rows[i % len(rows)]
            line = K.data_line(i, fmt, samples, infos[i % len(infos)] if infos else ".")
            if ids:
                c = line.split("\t")
                c[2], c[3], c[4] = ids[i % 3], ("A", "ACGT", "GG", "T", "CCCCCCC")[i % 5], (".", "C", "C,GT")[(i // 2) % 3]
                line = "\t".join(c)
            f.write(line + "\n")
    return str(path), [want[i % len(rows)] for i in range(n)]


# ---- fixtures and spelled-out rows ---------------------------------------------------------------------------------------------
def test_gpu_formats_text_of_the_reference_fixture(ctx, tmp_path):
    """index.vcf, index.vcf.gz and a BGZF copy of index.vcf: 621 rows = decode.formats_string, decoded on the GPU.  (Without the
    device column bind_ctx refuses a scan that projects `formats`.)"""
    p = os.path.join(FX, "vcf", "index.vcf")
    bg = tmp_path / "copy.vcf.gz"
    subprocess.check_call([BGZIP, p, str(bg), "6"])
    for path in (p, p + ".gz", str(bg)):
        c, on = gpu_scan(ctx, path, batch_size=64)
        assert on
        if path != p + ".gz":  # (the .gz fixture is another file: its first record has FORMAT "PL")
            assert c["formats"][0] == "GT:PL:PG\t0/0:0,3,26:0"
        assert len(c["formats"]) == 621 and c["formats"] == K.oracle_formats(path)


def test_gpu_formats_text_is_printed_again_not_copied(ctx, tmp_path):
    """the FORMAT part of test_host_vcf_info_and_formats_text_are_printed_again_not_copied with its exact strings, then the rows at
    the walk's limits (all but the one of 17 keys, which is handed over)"""
    p = K.write_vcf(tmp_path / "text.vcf", [(f, s) for f, s, _ in K.SPELLED])
    c, on = gpu_scan(ctx, p)
    assert on and c["formats"] == [t for _, _, t in K.SPELLED] == K.oracle_formats(p)
    rows = [r for r in K.LIMITS if r[0] is None or r[0].count(":") < 16]
    assert len(rows) == len(K.LIMITS) - 1
    p = K.write_vcf(tmp_path / "limits.vcf", rows)
    c, on = gpu_scan(ctx, p)
    want = K.oracle_formats(p)
    assert on and c["formats"] == want
    by = {(f, tuple(s)): w for (f, s), w in zip(rows, c["formats"])}
    assert by[("GT", ("1/02|3/004",))] == "GT\t1/2/3|4" and by[("GT", ("123456789012|000000000000|1|.",))] == "GT\t123456789012|0|1|."
    assert by[("GT:XQ", ("0/1:0.5:extra:values", "1|1:1.0:9"))] == "GT:XQ\t0/1:0.5\t1|1:1" and by[("GT::DP", ("0/1:x:07", "1/1:y:+3"))] == "GT::DP\t0/1:x:7\t1/1:y:3"
    assert by[(":".join(K.KEYS16), (":".join(K.VALS16), ":".join(K.VALS16[:5])))].endswith("\t0|1:0.5:7:t:5:0.00001,.:q:a:b:c:d:e:f:g:h:0\t0|1:0.5:7:t:5")


# ---- sample counts: item indices cross wave and workgroup boundaries at every phase -------------------------------------------------
COUNTS = [None, ".", 1, 2, 63, 64, 65, 255, 256, 257, 2504]


@pytest.fixture(scope="module")
def count_rows(tmp_path_factory):
    """198 rows cycling through COUNTS (None: no FORMAT; '.': FORMAT '.'), printed once by the oracle"""
    rows = []
    for r in range(198):
        c = COUNTS[r % 11]
        if c is None:
            rows.append((None, []))
        elif c == ".":
            rows.append((".", ["0/1"] * (r % 5)))
        else:
            floats = c <= 65
            rows.append(("GT:DP:XP:XQ" if floats else "GT:DP:XP", [sample_of(r, k, floats) for k in range(c)]))
    d = tmp_path_factory.mktemp("fmt_counts")
    want = K.oracle_formats(K.write_vcf(d / "counts.vcf", rows))
    assert None not in want
    return d, rows, want


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_gpu_formats_text_sample_counts(ctx, count_rows, order):
    d, rows, want = count_rows
    if order == "reversed":
        rows, want = rows[::-1], want[::-1]
    p = K.write_vcf(d / f"{order}.vcf", rows)
    c, on = gpu_scan(ctx, p, batch_size=50)
    assert on and c["pos"] == list(range(1, 199))
    assert [len(x) for x in c["formats"]] == [len(x) for x in want]
    assert c["formats"] == want
    assert max(x.count("\t") for x in want) == 2504 and sum(x == "\t" for x in want) == 36


# ---- parser level -------------------------------------------------------------------------------------------------------------------
def test_gpu_formats_text_offsets_and_misalignment_parser_level(ctx, mix):
    rows, want = mix
    text = "".join(K.data_line(i, f, s) + "\n" for i, (f, s) in enumerate(rows)).encode()
    par = exon_amd.VCFParser(ctx, ["1"], max_slab_bytes=len(text) + 4096, format_key_types=K.FORMAT_TYPES)
    for k in range(16):
        res = par.parse_host(text, misalign=k, formats_text=True)
        assert res["n_rows"] == len(rows) and res["n_undecided"] == 0
        ft = res["formats_text"]
        assert ft["n_undecided"] == 0
        off, val = ft["offsets"], ft["values"].tobytes()
        assert off[0] == 0 and off[-1] == ft["n_bytes"] == len(val) and np.all(np.diff(off) >= 1)
        assert [val[off[i]:off[i + 1]].decode() for i in range(len(rows))] == want, k
    # the reserved FORMAT keys alone; and a Flag is no FORMAT type
    par.set_format_key_types({})
    res = par.parse_host(b"1\t1\t.\tA\tC\t.\t.\t.\tGT:DP:GL:XQ:XP\t0|1:007:1e-5,0.50:0.50:007\n", formats_text=True)
    ft = res["formats_text"]
    assert ft["values"].tobytes().decode() == "GT:DP:GL:XQ:XP\t0|1:7:0.00001,0.5:0.50:007"
    with pytest.raises(exon_amd.ExonHipError):
        par.set_format_key_types({"XB": "b"})
    par.close()


@pytest.mark.parametrize("fmt,samples", K.HANDED_OVER + [(":".join(K.KEYS16 + ["XT"]), [":".join(K.VALS16 + ["z"])]), ("XT", ["é"]), ("XT:Gé", ["a:b"])])
def test_gpu_formats_text_rows_the_device_leaves_to_the_host_reader(ctx, fmt, samples):
    text = ("".join(K.data_line(i, "GT", ["0/1"] * 3) + "\n" for i in range(65)) + K.data_line(65, fmt, samples) + "\n").encode()
    par = exon_amd.VCFParser(ctx, ["1"], max_slab_bytes=len(text) + 4096, format_key_types=K.FORMAT_TYPES)
    res = par.parse_host(text, formats_text=True)
    par.close()
    assert res["n_rows"] == 66 and res["n_undecided"] == 0
    assert res["formats_text"]["n_undecided"] == 1 and "values" not in res["formats_text"]


# ---- CRLF -------------------------------------------------------------------------------------------------------------------------
def test_gpu_formats_text_of_crlf_lines(ctx, tmp_path, mix):
    """the CR in front of the LF is no part of the last sample, of FORMAT (a line that ends there) or of INFO (a line without FORMAT)"""
    rows, want = mix
    p = K.write_vcf(tmp_path / "crlf.vcf", rows, eol="\r\n")
    assert open(p, "rb").read().count(b"\r\n") == len(rows) + K.HEAD.count("\n")
    c, on = gpu_scan(ctx, p, batch_size=100)
    assert on and c["formats"] == want == K.oracle_formats(p)


# ---- slabs ------------------------------------------------------------------------------------------------------------------------
def test_gpu_formats_text_over_slabs_of_short_rows(ctx, tmp_path, monkeypatch, mix):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    rows, want = mix
    short = ([r for r in rows if len(r[1]) <= 3], [w for r, w in zip(rows, want) if len(r[1]) <= 3])
    p, want = cycle_file(tmp_path / "short.vcf", short, 30000)
    assert os.path.getsize(p) > (1 << 20)
    c, on = gpu_scan(ctx, p, batch_size=4096)
    assert on and c["pos"] == list(range(1, 30001)) and c["formats"] == want


def test_gpu_formats_text_over_slabs_of_2504_sample_rows(ctx, tmp_path, monkeypatch):
    """120 rows of 2 504 samples, about 30 KB each: some 30 rows a slab of 1 MiB, rows straddle the slab's end and are carried"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    rows = [("GT:DP:XP", [sample_of(r, k, False) for k in range(2504)]) for r in range(12)]
    want = K.oracle_formats(K.write_vcf(tmp_path / "wide12.vcf", rows))
    p = K.write_vcf(tmp_path / "wide.vcf", rows * 10)
    assert os.path.getsize(p) > (3 << 20) and 20 < (1 << 20) / (os.path.getsize(p) / 120) < 40
    c, on = gpu_scan(ctx, p, batch_size=16)
    assert on and c["pos"] == list(range(1, 121)) and c["formats"] == want * 10


def test_gpu_formats_text_longer_than_the_slab(ctx, tmp_path, monkeypatch):
    """Float items spelled 1e38 print 39 digits: the printed column is several times the text and far beyond the values buffer's first
    size (1 MiB), which grows; shorter slabs follow and reuse the buffers"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    long_s, long_w = ",".join(["1e38"] * 25), ",".join(["1" + "0" * 38] * 25)
    rows = [("GL", [long_s, long_s])] * 6000 + [("GT:DP", ["0|1:07"])] * 40000
    want = ["GL\t" + long_w + "\t" + long_w] * 6000 + ["GT:DP\t0|1:7"] * 40000
    p = K.write_vcf(tmp_path / "long.vcf", rows)
    assert 6000 * len(want[0]) > 4 * 6000 * len(K.data_line(0, *rows[0])) > (1 << 20) and os.path.getsize(p) > (2 << 20)
    c, on = gpu_scan(ctx, p, batch_size=4096)
    assert on and c["formats"] == want


def test_gpu_formats_text_of_a_tab_dense_slab(ctx, tmp_path):
    """5 000 one-character samples a row, 40 rows: 200 000 tabs, three times the tab buffer's first capacity (65 536).  The index is
    counted before its buffer is sized, so the slab is neither re-run nor handed over: it decodes on the GPU at the first go."""
    rows = [("XT", [("a", "b", "c")[(r + k) % 3] for k in range(5000)]) for r in range(40)]
    p = K.write_vcf(tmp_path / "dense.vcf", rows)
    c, on = gpu_scan(ctx, p)
    assert on
    assert c["formats"] == ["XT\t" + "\t".join(s) for _, s in rows]


# ---- hand-over --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,samples,raises", [("GT:XQ", ["0/1:."], True), ("GT", ["0/x", "0/1"], True), (":".join(K.KEYS16 + ["XT"]), [":".join(K.VALS16 + ["z"])], False),
                                                ("XT", ["café"], False), ("GT", [], True)])
def test_gpu_formats_text_one_row_in_the_second_slab_hands_the_file_over(ctx, tmp_path, monkeypatch, mix, fmt, samples, raises):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    rows, _ = mix
    short = [r for r in rows if len(r[1]) <= 5]
    all_rows = [short[i % len(short)] for i in range(40000)]
    all_rows[33001] = (fmt, samples)
    p = K.write_vcf(tmp_path / "handover.vcf", all_rows)
    assert sum(len(K.data_line(i, *r)) + 1 for i, r in enumerate(all_rows[:33001])) > (1 << 20)  # the odd row lies in the second slab
    if raises:
        with pytest.raises(exon_amd.ExonHipError):
            gpu_scan(ctx, p, batch_size=1000)
        with pytest.raises(exon_amd.ExonHipError):
            table(exon_amd.Scan(p, "vcf", project=("formats",), batch_size=1000))
        return
    c, on = gpu_scan(ctx, p, project=("ref", "formats"), batch_size=1000)
    h = table(exon_amd.Scan(p, "vcf", project=("ref", "formats"), batch_size=1000))
    assert not on
    assert c["pos"] == list(range(1, 40001))  # nothing lost, the first slab's rows not served twice
    for k in h:
        assert c[k] == h[k], k
    assert c["formats"][33001].startswith(fmt + "\t")


# ---- other columns ----------------------------------------------------------------------------------------------------------------
INFOS = ["XF=0.50;XB", ".", "XL=1e-5,.,1.0;XI=007", "XS=a,b,.;XC=q", "XD=a,.,b;XJ=+5,.,-3", "DB;AF=0.010;ZZ=0.50", "XI=0"]
PROJECTIONS = [p + ("formats",) for r in range(5) for p in itertools.combinations(("id", "ref", "alt", "info"), r)]


@pytest.fixture(scope="module")
def batch_files(tmp_path_factory, mix):
    """600 rows (batches of 1) and 20 000 rows (two slabs of 1 MiB) with ids / refs / alts / infos of their own rhythms, and the
    host reader's columns for every projection that has `formats`"""
    d = tmp_path_factory.mktemp("fmt_batches")
    out = {}
    for n in (600, 20000):
        p, want = cycle_file(d / f"b{n}.vcf", mix, n, infos=INFOS, ids=[".", "rs1", "a;b;c"])
        host = {}
        for proj in PROJECTIONS:
            s = exon_amd.Scan(p, "vcf", project=proj)
            names = [s.schema().field(i).name for i in range(s.schema().num_fields)]
            host[proj] = (names, table(s))
            s.close()
        out[n] = (p, want, host)
    assert len(PROJECTIONS) == 16 and os.path.getsize(out[20000][0]) > (1 << 20)
    return out


@pytest.mark.parametrize("batch_size", [1, 64, 8192])
def test_gpu_formats_text_batches_equal_the_host_readers_for_every_projection(ctx, batch_files, monkeypatch, batch_size):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    n = 600 if batch_size == 1 else 20000
    path, want, host = batch_files[n]
    for proj, (names, cols) in host.items():
        s = exon_amd.Scan(path, "vcf", gpu_parse=True, project=proj, formats_on_device=True, batch_size=batch_size).bind_ctx(ctx)
        assert [s.schema().field(i).name for i in range(s.schema().num_fields)] == names
        sizes, got = [], {}
        for b in s:
            sizes.append(len(b))
            assert [b.type.field(i).name for i in range(b.type.num_fields)] == names  # the host reader's column order
            for i, k in enumerate(names):
                got.setdefault(k, []).extend(b.field(i).to_pylist())
        assert s.decoded_on_gpu()[0], proj
        s.close()
        assert sum(sizes) == n and max(sizes) <= batch_size and len(sizes) >= n // batch_size
        for k in names:
            assert got[k] == cols[k], (proj, k)
        assert got["formats"] == want


def test_gpu_formats_text_next_to_typed_info_fields(ctx, batch_files, monkeypatch):
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    path, want, _ = batch_files[20000]
    c, on = gpu_scan(ctx, path, project=("ref", "info", "formats"), info_field="XF,XI,XB", batch_size=5000)
    h = table(exon_amd.Scan(path, "vcf", project=("ref", "info", "formats"), info_field="XF,XI,XB"))
    assert on and list(c) == list(h) and c["formats"] == want
    for k in h:
        assert c[k] == h[k], k


# ---- a pushed-down predicate and region -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_gpu_formats_text_under_a_pushed_down_predicate_and_region(ctx, tmp_path, monkeypatch, mix, order):
    """the kept rows' column: taken on the device under the predicate (the generic Utf8 take), views or the gather under a region"""
    monkeypatch.setenv("EXON_HIP_GPU_PARSE_SLAB_MB", "1")
    rows, want = mix
    n = 20000
    pos = np.arange(1, n + 1)
    if order == "shuffled":
        pos = np.random.default_rng(5).permutation(pos)
    qual = [(int(q) * 7) % 100 for q in pos]
    p = tmp_path / "kept.vcf"
    with open(p, "w") as f:
        f.write(K.HEAD)
        for i, q in enumerate(pos):
            fmt, samples = rows[i % len(rows)]
            f.write("\t".join(["1", str(q), ".", "A", "C", str(qual[i]), ".", "."]) + K.tail(fmt, samples) + "\n")
    assert os.path.getsize(p) > (1 << 20)
    lo, hi = 4000, 15000
    full = exon_amd.Scan(str(p), "vcf", gpu_parse=True, project=("formats",), formats_on_device=True, batch_size=3000).bind_ctx(ctx)
    c = table(full)
    assert full.decoded_on_gpu()[0] and c["formats"] == [want[i % len(rows)] for i in range(n)]
    full_d2h = full.export_stats()["d2h_bytes"]
    full.close()
    for where, region in (((2, ">", 49.5), None), (None, f"1:{lo}-{hi}"), ((2, ">", 49.5), f"1:{lo}-{hi}")):
        s = exon_amd.Scan(str(p), "vcf", gpu_parse=True, project=("formats",), formats_on_device=True, batch_size=3000, where=where, region=region).bind_ctx(ctx)
        c = table(s)
        keep = [i for i, q in enumerate(pos) if (where is None or qual[i] > 49.5) and (region is None or lo <= q <= hi)]
        assert s.decoded_on_gpu()[0] and len(keep) > 2000
        assert c["pos"] == [int(pos[i]) for i in keep] and c["formats"] == [want[i % len(rows)] for i in keep], (where, region)
        if order == "sorted":
            assert s.export_stats()["d2h_bytes"] < full_d2h, (where, region)
        s.close()


# ---- fuzz -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_samples,seed", [(2000, 3, 41), (300, 300, 43)])
def test_gpu_formats_text_fuzz_against_the_oracle(ctx, tmp_path, n, max_samples, seed):
    """the host fuzz generator: no key list beyond 16, no byte >= 0x80, no missing value -- no undecided row, so the file decodes on the GPU"""
    rows = K.fuzz_rows(n, seed, max_samples)
    p = K.write_vcf(tmp_path / "fuzz.vcf", rows)
    want = K.oracle_formats(p)
    assert None not in want
    c, on = gpu_scan(ctx, p, project=("info", "formats"), batch_size=500)
    assert on
    for i in range(n):
        assert c["formats"][i] == want[i], (i, rows[i])


# ---- opt-out ----------------------------------------------------------------------------------------------------------------------
def test_gpu_scan_with_formats_and_without_the_option_decodes_on_the_host_as_before(ctx):
    p = os.path.join(FX, "vcf", "index.vcf")
    s = exon_amd.Scan(p, "vcf", batch_size=100, gpu_parse=True, project=("formats",))
    with pytest.raises(exon_amd.ExonHipError):
        s.bind_ctx(ctx)
    c = table(s)
    assert not s.decoded_on_gpu()[0] and c["formats"] == K.oracle_formats(p)
    s.close()
