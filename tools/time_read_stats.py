#!/usr/bin/env python3
"""K9 (per-read length / GC percent / mean quality, `exon_hip_read_stats_hist[_views]`) on resident data and end to end, beside K5.

  time_read_stats.py [e2e_reads=20e6] [resident_bytes=1.9e9] [out.md]

Resident: for L = 100, 151, 250 and a ragged file, a slab of FASTQ text of ~resident_bytes (a slab's views are int32, so 20 M reads
do not fit one slab: the reads per slab are printed) is split by the device parser; K9 over the views of both lines and K5's ragged
path over the quality views of the same text are timed with device events (median of 7 after a warm-up), and the Arrow form of K9 over
generated columns.  Bytes read = what the algorithm needs: K9 both lines + 16 B of views per read (8 B of offsets in the Arrow form),
K5 the quality line + 8 B.  The ceiling is `exon_hip_read_probe` over the same slab.
End to end: a BGZF .fastq.gz of e2e_reads reads through exon_hip_stream_consume_scan with kind 9 and with kind 5, alternating."""
import os, statistics, subprocess, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exon_amd
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
e2e_reads = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20_000_000
resident = int(float(sys.argv[2])) if len(sys.argv) > 2 else int(1.9e9)
out = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
ctx = exon_amd.Context(0)
LMAX = 256


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


say(f"device: {ctx.info()['name']}, {ctx.info()['compute_units']} CUs")
say()
say("| reads | form | reads per launch | K9 ms (min .. max) | K9 bytes | K9 GB/s | of ceiling | K5 path G ms | K5 bytes | K5 GB/s | of ceiling | ceiling GB/s |")
say("|---|---|---|---|---|---|---|---|---|---|---|---|")
for L, rag in ((100, 0), (151, 0), (250, 0), (151, 1)):
    path = "/tmp/k9_slab.fastq"
    n_file = resident // (2 * L + 28)  # a record: '@read<i> sample=<k>', two lines of <= L bytes, '+', four line ends
    subprocess.check_call([os.path.join(BIN, "gen_text"), "fastq", str(n_file), path, str(L), str(rag)])
    raw = np.fromfile(path, np.uint8, min(os.path.getsize(path), resident))
    cut = int(np.flatnonzero(raw[-4096:] == 10)[-1]) + 1 + len(raw) - 4096
    d = ctx.to_device(np.concatenate([raw[:cut], np.zeros(64, np.uint8)]))
    del raw
    gbps, _ = ctx.read_probe([d.ptr], (cut // 65536) * 65536)
    p = exon_amd.FASTQParser(ctx, max_slab_bytes=cut + 64)
    v = p.parse_device(d, cut, final=False)
    ctx.sync()
    n = v.n_reads
    lens = np.empty(n, np.int32), np.empty(n, np.int32)
    for a, (s, e) in zip(lens, ((v.seq_start, v.seq_end), (v.qual_start, v.qual_end))):
        hs, he = np.empty(n, np.int32), np.empty(n, np.int32)
        ctx._check(ctx.lib.exon_hip_memcpy_d2h(ctx.h, hs.ctypes.data, s, hs.nbytes, None))
        ctx._check(ctx.lib.exon_hip_memcpy_d2h(ctx.h, he.ctypes.data, e, he.nbytes, None))
        a[:] = he - hs
    sbytes, qbytes = int(lens[0].sum()), int(lens[1].sum())
    d9 = ctx.zeros(np.int64, exon_amd.read_stats_layout(LMAX)[4])
    d5 = ctx.zeros(np.int64, LMAX * 256)
    k9 = timed(lambda: ctx.read_stats_hist_views(v.text_base, v.seq_start, v.seq_end, v.qual_start, v.qual_end, n, LMAX, d9))
    k5 = timed(lambda: ctx.qual_pos_hist_views(v.text_base, v.qual_start, v.qual_end, n, LMAX, d5))
    st = d9.to_host()
    assert st[0] == 8 * n and st[1] == 8 * sbytes and st[3] > 0, "K9 state does not match the slab"
    b9, b5 = sbytes + qbytes + 16 * n, qbytes + 8 * n
    name = f"L = {L}" if not rag else f"ragged {L - L // 4} .. {L}"
    say(f"| {name} | views | {n} | {k9[0]:.3f} ({k9[1]:.3f} .. {k9[2]:.3f}) | {b9 / 1e9:.3f} GB | {b9 / k9[0] / 1e6:.0f} | {b9 / k9[0] / 1e6 / gbps:.2f} | "
        f"{k5[0]:.3f} | {b5 / 1e9:.3f} GB | {b5 / k5[0] / 1e6:.0f} | {b5 / k5[0] / 1e6 / gbps:.2f} | {gbps:.0f} |")
    p.close()
    del d, v
    if not rag:  # the Arrow form: two generated Utf8 columns (the bytes are quality-like; the kernel's work does not depend on them)
        m = min(20_000_000, int(1.9e9) // L)
        so, sd = ctx.gen_c5(5, 0, m, L)
        qo, qd = ctx.gen_c5(6, 0, m, L)
        d9.zero()
        ka = timed(lambda: ctx.read_stats_hist(so, sd, qo, qd, m, LMAX, d9))
        ba = 2 * m * L + 8 * m
        say(f"| {name} | Arrow | {m} | {ka[0]:.3f} ({ka[1]:.3f} .. {ka[2]:.3f}) | {ba / 1e9:.3f} GB | {ba / ka[0] / 1e6:.0f} | {ba / ka[0] / 1e6 / gbps:.2f} | | | | | {gbps:.0f} |")
        del so, sd, qo, qd

if e2e_reads > 0:
    plain, gz = "/tmp/k9_e2e.fastq", "/tmp/k9_e2e.fastq.gz"
    subprocess.check_call([os.path.join(BIN, "gen_text"), "fastq", str(e2e_reads), plain, "150", "0"])
    subprocess.check_call([os.path.join(BIN, "bgzip"), plain, gz, "6"])
    tsize, csize = os.path.getsize(plain), os.path.getsize(gz)
    os.remove(plain)
    open(gz, "rb").read()

    def run(kind):
        scan = exon_amd.Scan(gz, "fastq", gpu_parse=True)
        plan = ctx.plan_read_stats_hist(LMAX, columns=(2, 3)) if kind == 9 else ctx.plan_qual_pos_hist(LMAX, columns=(3,))
        st = plan.open()
        t = time.perf_counter()
        rows = st.consume(scan)
        st.finish()
        dt = time.perf_counter() - t
        assert scan.decoded_on_gpu() == (True, True) and rows == e2e_reads
        st.close(); plan.close(); scan.close()
        return dt
    run(9); run(5)
    t9, t5 = [], []
    for _ in range(4):
        t9.append(run(9)); t5.append(run(5))
    say()
    say(f"end to end, {e2e_reads} reads of 150 bases, {tsize / 1e9:.2f} GB of text in a {csize / 1e9:.2f} GB BGZF file (page cache), inflate + split + kernel on the device, 4 alternating runs each:")
    say(f"- kind 9: median {statistics.median(t9):.3f} s ({min(t9):.3f} .. {max(t9):.3f}) = {tsize / statistics.median(t9) / 1e9:.2f} GB/s of text")
    say(f"- kind 5: median {statistics.median(t5):.3f} s ({min(t5):.3f} .. {max(t5):.3f}) = {tsize / statistics.median(t5) / 1e9:.2f} GB/s of text")
    say(f"- difference of the medians: {(statistics.median(t9) - statistics.median(t5)) * 1e3:+.1f} ms")
    os.remove(gz)
