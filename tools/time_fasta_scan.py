#!/usr/bin/env python3
"""FASTA batches: the GPU pipeline (Scan(..., "fasta", gpu_parse=True).bind_ctx) beside the host reader, on generated files.

  time_fasta_scan.py gen  <dir> [proteins=2e6] [reads=3e6]   protein.fasta (60-column lines, lengths around 350), its BGZF copy
                                                              protein.fasta.gz (level 1) and reads.fasta (one 150-base line a record)
  time_fasta_scan.py time <dir> [passes=3] [out.md]          per file: `passes` alternating passes of the bound scan and of the host
                                                              reader (batches are counted, not converted), medians and spread
  time_fasta_scan.py one  <file>                             one bound pass and what it moved (for rocprofv3 --kernel-trace --stats:
                                                              the fill's bytes are 2 x sequence bytes + 8 bytes of index a line),
                                                              with the context's read_probe ceiling"""
import os, statistics, subprocess, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exon_amd
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGZIP = os.path.join(ROOT, "tools", "bin", "bgzip")


def gen(d, n_protein, n_reads):
    rs = np.random.RandomState(11)
    aa = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    rows = rs.choice(aa, (1 << 14, 61))
    rows[:, 60] = 10
    wrapped, flat = rows.tobytes(), rs.choice(aa, 1 << 14).tobytes()
    lens = np.clip(rs.gamma(2.2, 160, n_protein).astype(np.int64), 20, 5000)
    with open(os.path.join(d, "protein.fasta"), "wb") as f:
        for i, L in enumerate(lens.tolist()):
            at = (i * 37) % ((1 << 14) - 90)
            f.write(b">sp|P%07d|PROT%d_GEN Generated protein %d OS=Synthetic organism OX=%d GN=g%d PE=1 SV=1\n" % (i, i, i, i % 9973, i % 20011))
            f.write(wrapped[at * 61:(at + L // 60) * 61])
            if L % 60:
                f.write(flat[at:at + L % 60] + b"\n")
    subprocess.check_call([BGZIP, os.path.join(d, "protein.fasta"), os.path.join(d, "protein.fasta.gz"), "1"], stdout=subprocess.DEVNULL)
    nt = rs.choice(np.frombuffer(b"ACGT", np.uint8), 1 << 20).tobytes()
    with open(os.path.join(d, "reads.fasta"), "wb") as f:
        for i in range(n_reads):
            at = (i * 7919) % ((1 << 20) - 160)
            f.write(b">read%d\n" % i + nt[at:at + 150] + b"\n")


def one_pass(ctx, path, bound):
    s = exon_amd.Scan(path, "fasta", gpu_parse=bound)
    if bound:
        s.bind_ctx(ctx)
    t = time.perf_counter()
    rows = 0
    for b in s:
        rows += len(b)
    dt = time.perf_counter() - t
    flags = s.decoded_on_gpu() if bound else (False, False)
    s.close()
    return dt, rows, flags


def main():
    mode, where = sys.argv[1], sys.argv[2]
    if mode == "gen":
        os.makedirs(where, exist_ok=True)
        gen(where, int(float(sys.argv[3])) if len(sys.argv) > 3 else 2_000_000, int(float(sys.argv[4])) if len(sys.argv) > 4 else 3_000_000)
        for f in sorted(os.listdir(where)):
            print(f, os.path.getsize(os.path.join(where, f)), flush=True)
        return
    ctx = exon_amd.Context(0)
    if mode == "one":
        open(where, "rb").read()
        d = ctx.zeros(np.uint8, 1 << 30)
        gbps, _ = ctx.read_probe([d.ptr], 1 << 30)
        del d
        dt, rows, flags = one_pass(ctx, where, True)
        print(f"{where}: {rows} records in {dt:.3f} s, decoded on the GPU {flags}; read_probe ceiling {gbps:.0f} GB/s", flush=True)
        if not where.endswith(".gz"):  # (generated text: no CR)
            a = np.fromfile(where, np.uint8)
            ends = np.flatnonzero(a == 10)
            starts = np.concatenate([[0], ends[:-1] + 1])
            is_def = a[starts] == 62
            seq_bytes = int((ends - starts)[~is_def].sum())
            print(f"{len(a)} bytes of text, {len(ends)} lines, {int(is_def.sum())} definition lines, {seq_bytes} sequence bytes", flush=True)
        return
    passes = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    out = open(sys.argv[4], "w") if len(sys.argv) > 4 else None

    def say(line=""):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    say(f"device: {ctx.info()['name']}; {passes} alternating passes each, page cache warm; seconds, median (min .. max)")
    say()
    say("| file | bytes | records | GPU pipeline | host reader | GPU / host | decoded, inflated on the GPU |")
    say("|---|---|---|---|---|---|---|")
    for name in ("protein.fasta", "protein.fasta.gz", "reads.fasta"):
        path = os.path.join(where, name)
        open(path, "rb").read()
        one_pass(ctx, path, True)  # warm-up: the context's slab buffers and pinned blocks
        g, h, rows, flags = [], [], 0, None
        for _ in range(passes):
            dt, rows, flags = one_pass(ctx, path, True)
            g.append(dt)
            dt, rows_h, _ = one_pass(ctx, path, False)
            h.append(dt)
            assert rows == rows_h
        mg, mh = statistics.median(g), statistics.median(h)
        say(f"| {name} | {os.path.getsize(path)} | {rows} | {mg:.3f} ({min(g):.3f} .. {max(g):.3f}) | {mh:.3f} ({min(h):.3f} .. {max(h):.3f}) | {mg / mh:.2f} | {flags} |")
    ctx.close()


if __name__ == "__main__":
    main()
