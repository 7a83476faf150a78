#!/usr/bin/env python3
"""K10 (per-record FASTA statistics, `exon_hip_seq_stats_hist[_views]`) on resident data and end to end.

  time_seq_stats.py [e2e_text_bytes=1e9] [slab_bytes=80e6] [out.md | -] [bound]

Resident: one slab of FASTA text of ~slab_bytes per case -- (a) 2 kb records at 60 columns, (b) one-line 150-base records, (c) unwrapped
8 MB records, (d) a 20-letter protein alphabet at 60 columns, (e) all-'G' at 60 columns -- is split by the device parser (timed with
device events: what every path over the slab pays first); K10 over the slab's views and K10 over the same sequences as an Arrow Utf8
column are timed with device events (median of 7 after a warm-up).  Bytes read = what the algorithm needs: views -- the consumed text
+ 8 B per line (line_end, line_dst) + 8 B per record (head_start, seq_offsets); Arrow -- the payload + 4 B of offsets per record.
The ceiling is `exon_hip_read_probe` over the same slab, in the same run.  Beside them K9's views time on FASTQ text of the same byte
count.  (`k_fasta_seq_fill`, what the batch path pays after the parser, has no entry point of its own: run this script under
`rocprofv3 --kernel-trace --stats` with `bound` as a fourth argument and read it from the kernel statistics of the bound passes.)
End to end: a BGZF FASTA file of ~e2e_text_bytes of text (case (a)'s records) through exon_hip_stream_consume_scan with kind 10,
gpu_parse on against off, alternating in one process; then the same text as plain gzip."""
import os, statistics, subprocess, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exon_amd
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
e2e_bytes = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
slab = int(float(sys.argv[2])) if len(sys.argv) > 2 else 80_000_000
out = open(sys.argv[3], "w") if len(sys.argv) > 3 and sys.argv[3] != "-" else None
bound_passes = len(sys.argv) > 4 and sys.argv[4] == "bound"
ctx = exon_amd.Context(0)
LMAX = 65536
DNA, PROTEIN = b"ACGT", b"ACDEFGHIKLMNPQRSTVWY"
HDR = np.frombuffer(b">record0000000 sample=7 len=x\n", np.uint8)


def say(line=""):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed(fn, reps=7):
    fn(); ctx.sync()
    ms = []
    for _ in range(reps):
        ctx.timer_start(); fn(); ms.append(ctx.timer_stop_ms()); ctx.sync()
    return statistics.median(ms), min(ms), max(ms)


def make(total, rec_len, width, alphabet, seed=1):
    """(text, sequence payload, record length, records): records of rec_len letters of `alphabet`, wrapped at `width` (None: one line)"""
    width = width or rec_len
    full, rest = divmod(rec_len, width)
    per = len(HDR) + full * (width + 1) + (rest + 1 if rest else 0)
    n = max(1, total // per)
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), (n, rec_len), dtype=np.uint8)]
    parts = [np.broadcast_to(HDR, (n, len(HDR)))]
    if full:
        body = np.full((n, full, width + 1), 10, np.uint8)
        body[:, :, :width] = seq[:, :full * width].reshape(n, full, width)
        parts.append(body.reshape(n, -1))
    if rest:
        tail = np.full((n, rest + 1), 10, np.uint8)
        tail[:, :rest] = seq[:, full * width:]
        parts.append(tail)
    return np.concatenate(parts, axis=1).reshape(-1), seq.reshape(-1), rec_len, n


CASES = [("(a) 2 kb records, 60 columns", 2000, 60, DNA), ("(b) 150-base records, one line", 150, None, DNA),
         ("(c) 8 MB records, one line", 8_000_000, None, DNA), ("(d) protein, 400 letters, 60 columns", 400, 60, PROTEIN),
         ("(e) all G, 2 kb records, 60 columns", 2000, 60, b"G")]

say(f"device: {ctx.info()['name']}, {ctx.info()['compute_units']} CUs; slab {slab / 1e6:.0f} MB")
say()
say("| case | form | records | lines | K10 ms (min .. max) | bytes | GB/s | of ceiling | parser ms | ceiling GB/s |")
say("|---|---|---|---|---|---|---|---|---|---|")
words = exon_amd.seq_stats_layout(LMAX)[5]
for name, rec_len, width, alphabet in CASES:
    text, payload, L, n = make(slab, rec_len, width, alphabet)
    nb = len(text)
    d = ctx.to_device(np.concatenate([text, np.zeros(64, np.uint8)]))
    gbps, _ = ctx.read_probe([d.ptr], (nb // 65536) * 65536)
    p = exon_amd.FASTAParser(ctx, max_slab_bytes=nb + 64)
    box = {}
    tp = timed(lambda: box.__setitem__("v", p.parse_device(d, nb, final=True)))
    v = box["v"]
    assert v.n_records == n and v.n_undecided == 0 and v.seq_bytes == len(payload)
    st = ctx.zeros(np.int64, words)
    kv = timed(lambda: ctx.seq_stats_hist_views(v, LMAX, st))
    h = st.to_host()
    assert h[0] == 8 * n and h[1] == 8 * len(payload), "K10's state does not match the slab"
    bv = nb + 8 * v.n_lines + 8 * n
    say(f"| {name} | views | {n} | {v.n_lines} | {kv[0]:.3f} ({kv[1]:.3f} .. {kv[2]:.3f}) | {bv / 1e6:.1f} MB | {bv / kv[0] / 1e6:.0f} | {bv / kv[0] / 1e6 / gbps:.2f} | "
        f"{tp[0]:.3f} ({tp[1]:.3f} .. {tp[2]:.3f}) | {gbps:.0f} |")
    p.close()
    del d, v
    off = ctx.to_device(np.arange(n + 1, dtype=np.int64) * L, np.int32)
    val = ctx.to_device(payload)
    st.zero()
    ka = timed(lambda: ctx.seq_stats_hist(off, val, n, LMAX, st))
    assert np.array_equal(st.to_host(), h), "the two forms disagree"
    ba = len(payload) + 4 * (n + 1)
    say(f"| {name} | Arrow | {n} | | {ka[0]:.3f} ({ka[1]:.3f} .. {ka[2]:.3f}) | {ba / 1e6:.1f} MB | {ba / ka[0] / 1e6:.0f} | {ba / ka[0] / 1e6 / gbps:.2f} | | {gbps:.0f} |")
    del off, val, text, payload

# K9 over the views of FASTQ text of the same byte count
path = "/tmp/k10_k9.fastq"
subprocess.check_call([os.path.join(BIN, "gen_text"), "fastq", str(slab // (2 * 150 + 28)), path, "150", "0"])
raw = np.fromfile(path, np.uint8)
os.remove(path)
d = ctx.to_device(np.concatenate([raw, np.zeros(64, np.uint8)]))
gbps, _ = ctx.read_probe([d.ptr], (len(raw) // 65536) * 65536)
p = exon_amd.FASTQParser(ctx, max_slab_bytes=len(raw) + 64)
v = p.parse_device(d, len(raw), final=True)
ctx.sync()
d9 = ctx.zeros(np.int64, exon_amd.read_stats_layout(256)[4])
k9 = timed(lambda: ctx.read_stats_hist_views(v.text_base, v.seq_start, v.seq_end, v.qual_start, v.qual_end, v.n_reads, 256, d9))
say()
say(f"K9 over the views of {len(raw) / 1e6:.1f} MB of FASTQ text ({v.n_reads} reads of 150): {k9[0]:.3f} ms ({k9[1]:.3f} .. {k9[2]:.3f}), "
    f"{len(raw) / k9[0] / 1e6:.0f} GB/s of text, ceiling {gbps:.0f} GB/s")
p.close()
del d, v, raw

if e2e_bytes > 0:
    plain, bgz, gz = "/tmp/k10_e2e.fasta", "/tmp/k10_e2e.bgzf.fasta.gz", "/tmp/k10_e2e.fasta.gz"
    block, _, _, n_block = make(min(e2e_bytes, 100_000_000), 2000, 60, DNA, seed=9)
    reps = max(1, e2e_bytes // len(block))
    with open(plain, "wb") as f:
        for _ in range(reps):
            f.write(block.tobytes())
    n_rec, tsize = n_block * reps, os.path.getsize(plain)
    subprocess.check_call([os.path.join(BIN, "bgzip"), plain, bgz, "1"], stdout=subprocess.DEVNULL)
    with open(gz, "wb") as f:
        subprocess.check_call(["gzip", "-1", "-c", plain], stdout=f)
    os.remove(plain)

    def run(path, gpu_parse):
        scan = exon_amd.Scan(path, "fasta", gpu_parse=gpu_parse)
        plan = ctx.plan_seq_stats_hist(LMAX, columns=(2,))
        st = plan.open()
        t = time.perf_counter()
        rows = st.consume(scan)
        counts, _ = st.finish()
        dt = time.perf_counter() - t
        assert scan.decoded_on_gpu()[0] == gpu_parse and rows == n_rec and counts[1] == n_rec * 2000
        st.close(); plan.close(); scan.close()
        return dt

    say()
    for label, path in (("BGZF", bgz), ("plain gzip", gz)):
        open(path, "rb").read()
        run(path, True); run(path, False)
        on, off_ = [], []
        for _ in range(3):
            on.append(run(path, True)); off_.append(run(path, False))
        say(f"end to end, {label}: {n_rec} records, {tsize / 1e9:.2f} GB of text in a {os.path.getsize(path) / 1e9:.2f} GB file (page cache), 3 alternating runs each:")
        for what, t in (("gpu_parse on ", on), ("gpu_parse off", off_)):
            say(f"- {what}: median {statistics.median(t):.3f} s ({min(t):.3f} .. {max(t):.3f}) = {tsize / statistics.median(t) / 1e9:.2f} GB/s of text")
        if bound_passes and label == "BGZF":  # the batch path over the same file, for a kernel trace (k_fasta_seq_fill)
            scan = exon_amd.Scan(path, "fasta", gpu_parse=True).bind_ctx(ctx)
            rows = sum(len(b) for b in scan)
            assert rows == n_rec
            scan.close()
        os.remove(path)
