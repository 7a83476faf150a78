"""Python host side above the C ABI (test harness / bench driver; the product is the HIP library).

`Context` owns a device; `DeviceBuffer` is a typed HBM allocation; `Plan` / `Stream` mirror the
ExecutionPlan-shaped surface of include/exon_hip.h (plan_create / stream_open / push / finish).
Every compute call goes through libexon_hip.so -- there is no numpy or oracle fallback.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import CMP, Column, ExonHipError


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class DeviceBuffer:
    """A typed allocation in HBM (hipMalloc through the C ABI)."""

    def __init__(self, ctx, dtype, n):
        self.ctx = ctx
        self.dtype = np.dtype(dtype)
        self.n = int(n)
        self.nbytes = self.n * self.dtype.itemsize
        p = C.c_void_p()
        ctx._check(ctx.lib.exon_hip_malloc(ctx.h, max(self.nbytes, 16), C.byref(p)))
        self.ptr = p.value

    def copy_from(self, host, stream=None):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.size <= self.n
        self.ctx._check(self.ctx.lib.exon_hip_memcpy_h2d(self.ctx.h, self.ptr, _np_ptr(host), host.nbytes, stream))
        self.ctx.sync(stream)
        return self

    def to_host(self, n=None, stream=None):
        n = self.n if n is None else n
        out = np.empty(n, self.dtype)
        self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(out), self.ptr, out.nbytes, stream))
        return out

    def zero(self, stream=None):
        self.ctx._check(self.ctx.lib.exon_hip_memset(self.ctx.h, self.ptr, 0, self.nbytes, stream))
        return self

    def free(self):
        if self.ptr:
            self.ctx.lib.exon_hip_free(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _col(values=None, validity=None, offsets=None, length=0):
    def p(x):
        if x is None:
            return None
        return x.ptr if isinstance(x, DeviceBuffer) else int(x)
    return Column(p(values), p(validity), p(offsets), int(length))


class Context:
    def __init__(self, device=0):
        self.lib = L.load()
        h = C.c_void_p()
        rc = self.lib.exon_hip_ctx_create(device, C.byref(h))
        if rc:
            raise ExonHipError(rc, self.lib.exon_hip_last_error(None).decode(errors="replace"))
        self.h = h
        self.device = device

    # -- plumbing ---------------------------------------------------------------------------
    def _last_error(self):
        """the calling thread's own text first (another thread of this ctx may have failed since), then the ctx's"""
        return self.lib.exon_hip_last_error(None).decode(errors="replace") or self.lib.exon_hip_last_error(self.h).decode(errors="replace")

    def _check(self, rc):
        if rc < 0:
            raise ExonHipError(rc, self._last_error())
        return rc

    def info(self):
        d = L.DeviceInfo()
        self._check(self.lib.exon_hip_ctx_info(self.h, C.byref(d)))
        return {"name": d.name.decode(), "gcn_arch": d.gcn_arch.decode(), "compute_units": d.compute_units,
                "wavefront_size": d.wavefront_size, "hbm_bytes": d.hbm_bytes, "clock_khz": d.clock_khz}

    def empty(self, dtype, n):
        return DeviceBuffer(self, dtype, n)

    def zeros(self, dtype, n):
        return DeviceBuffer(self, dtype, n).zero()

    def to_device(self, host, dtype=None):
        host = np.ascontiguousarray(host, dtype=dtype)
        return DeviceBuffer(self, host.dtype, host.size).copy_from(host)

    def sync(self, stream=None):
        self._check(self.lib.exon_hip_sync(self.h, stream))

    def read_probe(self, ptrs, bytes_each, reps=20, stream=None):
        """exon_hip_read_probe: (GB/s, ms per pass) of a bare streaming read over 1..4 device buffers in lock-step."""
        arr = (C.c_void_p * len(ptrs))(*[int(p) for p in ptrs])
        ms, nbytes = C.c_double(), C.c_int64()
        self._check(self.lib.exon_hip_read_probe(self.h, stream, arr, len(ptrs), int(bytes_each), int(reps), C.byref(ms), C.byref(nbytes)))
        return nbytes.value / (ms.value * 1e-3) / 1e9, ms.value

    def gzip_inflate(self, raw, slab_bytes=None, out_cap=None, scratch_bytes=0, return_stats=False):
        """A whole plain-gzip file through exon_hip_gzip_stream_*, `slab_bytes` of compressed input per call (the unused tail of
        a slab is passed again in front of the next bytes, as a file pipeline does): (bytes, stats)."""
        raw = bytes(raw)
        slab = int(slab_bytes or max(len(raw), 1))
        cap = int(out_cap or max(4 << 20, 40 * slab))
        h = C.c_void_p()
        self._check(self.lib.exon_hip_gzip_stream_create(self.h, slab, int(scratch_bytes), C.byref(h)))
        d_comp = DeviceBuffer(self, np.uint8, slab + 8192)
        d_out = DeviceBuffer(self, np.uint8, cap)
        out = []
        try:
            pos, ended = 0, False
            while not ended:
                n = min(slab, len(raw) - pos)
                final = pos + n == len(raw)
                buf = np.zeros(n + 4096, np.uint8)
                buf[:n] = np.frombuffer(raw, np.uint8, n, pos)
                d_comp.copy_from(buf)
                consumed, produced, end = C.c_int64(), C.c_int64(), C.c_int32()
                self._check(self.lib.exon_hip_gzip_stream_decode(h, None, d_comp.ptr, n, int(final), d_out.ptr, cap, C.byref(consumed),
                                                                 C.byref(produced), C.byref(end)))
                if produced.value:
                    out.append(d_out.to_host(produced.value).tobytes())
                ended = bool(end.value)
                if not ended and consumed.value == 0 and produced.value == 0:
                    raise ExonHipError(-1, "gzip_inflate: no progress")
                pos += consumed.value
                if final and not ended and consumed.value == 0:
                    raise ExonHipError(-1, "gzip_inflate: input ended without the stream's end")
            st = L.GzipStats()
            self._check(self.lib.exon_hip_gzip_stream_get_stats(h, C.byref(st)))
        finally:
            self.lib.exon_hip_gzip_stream_destroy(h)
            d_comp.free()
            d_out.free()
        data = b"".join(out)
        return (data, {n: getattr(st, n) for n, _ in L.GzipStats._fields_}) if return_stats else data

    def timer_start(self, stream=None):
        self._check(self.lib.exon_hip_timer_start(self.h, stream))

    def timer_stop_ms(self, stream=None):
        ms = C.c_float()
        self._check(self.lib.exon_hip_timer_stop_ms(self.h, stream, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.lib.exon_hip_ctx_destroy(self.h)
            self.h = None

    # -- operators (asynchronous; accumulate into device state) ---------------------------------
    def region_count(self, chrom_id, pos, n, region_chrom_id, start, end, d_count, chrom_valid=None,
                     pos_valid=None, stream=None):
        end = L.REGION_OPEN_END if end is None else end
        c0, c1 = _col(chrom_id, chrom_valid, None, n), _col(pos, pos_valid, None, n)
        self._check(self.lib.exon_hip_region_count(self.h, stream, C.byref(c0), C.byref(c1), n, region_chrom_id,
                                                   start, end, d_count.ptr))

    def flag_mapq_group_count(self, flag, mapq, mapq_valid, ref_id, ref_valid, n, flag_mask, flag_value, mapq_min,
                              n_refs, d_counts, flag_valid=None, stream=None):
        c0, c1, c2 = _col(flag, flag_valid, None, n), _col(mapq, mapq_valid, None, n), _col(ref_id, ref_valid, None, n)
        self._check(self.lib.exon_hip_flag_mapq_group_count(self.h, stream, C.byref(c0), C.byref(c1), C.byref(c2), n,
                                                            flag_mask, flag_value, mapq_min, n_refs, d_counts.ptr))

    def cmp_avg_by_group(self, x, x_valid, y, y_valid, group_id, n, threshold, op, n_groups, d_counts, d_sums,
                         stream=None):
        c0, c1, c2 = _col(x, x_valid, None, n), _col(y, y_valid, None, n), _col(group_id, None, None, n)
        self._check(self.lib.exon_hip_cmp_avg_by_group(self.h, stream, C.byref(c0), C.byref(c1), C.byref(c2), n,
                                                       float(threshold), CMP[op], n_groups, d_counts.ptr, d_sums.ptr))

    def cmp_minmax_by_group(self, x, x_valid, y, y_valid, group_id, n, threshold, op, n_groups, d_state, stream=None):
        """K8 (Float32 x, y): K4's predicate, then MIN / MAX / COUNT(y) / COUNT(*) per group accumulated into `d_state` =
        [count_y[G]] [count_rows[G]] [minw[G]] [maxw[G]] int64 words (minmax_decode turns the last two planes into values)."""
        c0, c1, c2 = _col(x, x_valid, None, n), _col(y, y_valid, None, n), _col(group_id, None, None, n)
        self._check(self.lib.exon_hip_cmp_minmax_by_group(self.h, stream, C.byref(c0), C.byref(c1), C.byref(c2), n,
                                                          float(threshold), CMP[op], n_groups, d_state.ptr))

    def overlap_count(self, ref_id, ref_valid, start, start_valid, end, end_valid, n, region_ref_id, region_start, region_end,
                      d_count, stream=None):
        """K6: rows whose [start, end] on reference `region_ref_id` overlaps [region_start, region_end] (all three valid)."""
        c0, c1, c2 = _col(ref_id, ref_valid, None, n), _col(start, start_valid, None, n), _col(end, end_valid, None, n)
        end_v = L.REGION_OPEN_END if region_end is None else region_end
        self._check(self.lib.exon_hip_overlap_count(self.h, stream, C.byref(c0), C.byref(c1), C.byref(c2), n, region_ref_id,
                                                    region_start, end_v, d_count.ptr))

    def within_count(self, ref_id, ref_valid, start, start_valid, end, end_valid, n, region_ref_id, after, before, d_count,
                     stream=None):
        """K6 strict form: rows with start > after AND end < before on reference `region_ref_id` (BED / GFF predicate)."""
        c0, c1, c2 = _col(ref_id, ref_valid, None, n), _col(start, start_valid, None, n), _col(end, end_valid, None, n)
        self._check(self.lib.exon_hip_within_count(self.h, stream, C.byref(c0), C.byref(c1), C.byref(c2), n, region_ref_id,
                                                   after, L.REGION_OPEN_END if before is None else before, d_count.ptr))

    def qual_pos_hist(self, offsets, data, n_reads, lmax, d_hist, stream=None):
        c0 = _col(data, None, offsets, n_reads)
        self._check(self.lib.exon_hip_qual_pos_hist(self.h, stream, C.byref(c0), n_reads, lmax, d_hist.ptr))

    def qual_pos_hist_chunks(self, chunks, lmax, d_hist, stream=None):
        """chunks = [(offsets, data, n_reads)]: one Utf8 batch each; fused launches of up to 64 chunks."""
        arr = (Column * max(1, len(chunks)))(*[_col(d, None, o, n) for (o, d, n) in chunks])
        ns = (C.c_int64 * max(1, len(chunks)))(*[n for _, _, n in chunks])
        self._check(self.lib.exon_hip_qual_pos_hist_chunks(self.h, stream, arr, len(chunks), ns, lmax, d_hist.ptr))

    def qual_pos_hist_views(self, d_text, starts, ends, n_reads, lmax, d_hist, stream=None):
        """K5 over [starts[r], ends[r]) views into `d_text` (device pointers / DeviceBuffers)."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        self._check(self.lib.exon_hip_qual_pos_hist_views(self.h, stream, ptr(d_text), ptr(starts), ptr(ends), n_reads, lmax,
                                                          d_hist.ptr))

    def read_stats_hist(self, seq_offsets, seq_data, qual_offsets, qual_data, n_reads, lmax, d_state, stream=None):
        """K9 over two Utf8 columns (sequence, quality_scores): per-read length / GC percent / mean quality histograms and
        four totals accumulated into `d_state` (read_stats_layout(lmax) int64 words)."""
        c0, c1 = _col(seq_data, None, seq_offsets, n_reads), _col(qual_data, None, qual_offsets, n_reads)
        self._check(self.lib.exon_hip_read_stats_hist(self.h, stream, C.byref(c0), C.byref(c1), n_reads, lmax,
                                                      d_state.ptr if isinstance(d_state, DeviceBuffer) else d_state))

    def read_stats_hist_views(self, d_text, seq_start, seq_end, qual_start, qual_end, n_reads, lmax, d_state, stream=None):
        """K9 over [start[r], end[r]) views of both lines into `d_text` (device pointers / DeviceBuffers)."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        self._check(self.lib.exon_hip_read_stats_hist_views(self.h, stream, ptr(d_text), ptr(seq_start), ptr(seq_end), ptr(qual_start),
                                                            ptr(qual_end), n_reads, lmax, ptr(d_state)))

    def seq_stats_hist(self, seq_offsets, seq_data, n_records, lmax, d_state, stream=None):
        """K10 over one Utf8 column (sequence): totals, byte composition and the length / log2 length / GC percent histograms
        of the records, accumulated into `d_state` (seq_stats_layout(lmax)[5] int64 words)."""
        c0 = _col(seq_data, None, seq_offsets, n_records)
        self._check(self.lib.exon_hip_seq_stats_hist(self.h, stream, C.byref(c0), n_records, lmax,
                                                     d_state.ptr if isinstance(d_state, DeviceBuffer) else d_state))

    def seq_stats_hist_views(self, views, lmax, d_state, stream=None):
        """K10 over the views of one FASTA slab in HBM (FASTAParser.parse_device): nothing is compacted or copied."""
        self._check(self.lib.exon_hip_seq_stats_hist_views(self.h, stream, C.byref(views), lmax,
                                                           d_state.ptr if isinstance(d_state, DeviceBuffer) else d_state))

    def bgzf_inflate(self, data, verify_crc=True, stream=None):
        """Test / tool helper: BGZF bytes -> inflated bytes through the GPU (exon_hip_bgzf_inflate).  Returns
        (inflated uint8 array, seconds spent in the device call)."""
        import time
        blocks, n, consumed, out_bytes = bgzf_scan(data)
        comp = np.frombuffer(data, np.uint8)[:consumed]
        d_comp = self.to_device(np.concatenate([comp, np.zeros(4096 + (-len(comp)) % 4, np.uint8)]))
        d_out = self.empty(np.uint8, out_bytes + 64)
        bad = C.c_int32(-1)
        t = time.perf_counter()
        self._check(self.lib.exon_hip_bgzf_inflate(self.h, stream, d_comp.ptr, blocks, n, d_out.ptr, 1 if verify_crc else 0,
                                                   C.byref(bad)))
        dt = time.perf_counter() - t
        return d_out.to_host()[:out_bytes], dt

    # -- synthetic inputs in HBM ------------------------------------------------------------------
    def gen_c2(self, seed, n_total, lo=0, hi=None, stream=None):
        hi = n_total if hi is None else hi
        n = hi - lo
        chrom, pos = self.empty(np.int32, n), self.empty(np.int64, n)
        self._check(self.lib.exon_hip_gen_c2(self.h, stream, seed, n_total, lo, hi, chrom.ptr, pos.ptr))
        return chrom, pos

    def gen_c6(self, seed, lo, hi, stream=None):
        n = hi - lo
        nb = (n + 7) // 8 + 64
        ref, rv = self.empty(np.int32, n), self.zeros(np.uint8, nb)
        start, end, pv = self.empty(np.int64, n), self.empty(np.int64, n), self.zeros(np.uint8, nb)
        self._check(self.lib.exon_hip_gen_c6(self.h, stream, seed, lo, hi, ref.ptr, rv.ptr, start.ptr, end.ptr, pv.ptr))
        return ref, rv, start, end, pv

    def gen_c3(self, seed, lo, hi, stream=None):
        n = hi - lo
        nb = (n + 7) // 8 + 64
        flag, mapq, mv = self.empty(np.int32, n), self.empty(np.uint8, n + 64), self.zeros(np.uint8, nb)
        ref, rv = self.empty(np.int32, n), self.zeros(np.uint8, nb)
        self._check(self.lib.exon_hip_gen_c3(self.h, stream, seed, lo, hi, flag.ptr, mapq.ptr, mv.ptr, ref.ptr, rv.ptr))
        return flag, mapq, mv, ref, rv

    def gen_c4(self, seed, lo, hi, stream=None):
        n = hi - lo
        nb = (n + 7) // 8 + 64
        af, av = self.empty(np.float32, n), self.zeros(np.uint8, nb)
        q, qv = self.empty(np.float32, n), self.zeros(np.uint8, nb)
        fid = self.empty(np.int32, n)
        self._check(self.lib.exon_hip_gen_c4(self.h, stream, seed, lo, hi, af.ptr, av.ptr, q.ptr, qv.ptr, fid.ptr))
        return af, av, q, qv, fid

    def gen_c5(self, seed, lo, hi, read_len, stream=None):
        n = hi - lo
        off, data = self.empty(np.int32, n + 1), self.empty(np.uint8, n * read_len + 64)
        self._check(self.lib.exon_hip_gen_c5(self.h, stream, seed, lo, hi, read_len, off.ptr, data.ptr))
        return off, data

    # -- plans ------------------------------------------------------------------------------------
    def plan_region_count(self, region_chrom_id, start=1, end=None, columns=(0, 1)):
        d = L.PlanDesc(kind=L.PLAN_REGION_COUNT, region_chrom_id=region_chrom_id, region_start=start,
                       region_end=L.REGION_OPEN_END if end is None else end)
        return Plan(self, d, columns)

    def plan_overlap_count(self, region_ref_id, start=1, end=None, columns=(2, 3, 4)):
        """COUNT(*) of BAM-layout rows overlapping a region (scan columns 2 reference, 3 start, 4 end)."""
        d = L.PlanDesc(kind=L.PLAN_OVERLAP_COUNT, region_chrom_id=region_ref_id, region_start=start,
                       region_end=L.REGION_OPEN_END if end is None else end)
        return Plan(self, d, columns)

    def plan_within_count(self, region_ref_id, after=0, before=None, columns=(2, 3, 4)):
        """COUNT(*) of rows with reference = id AND start > after AND end < before (StartEndIntervalPhysicalExpr)."""
        d = L.PlanDesc(kind=L.PLAN_WITHIN_COUNT, region_chrom_id=region_ref_id, region_start=after,
                       region_end=L.REGION_OPEN_END if before is None else before)
        return Plan(self, d, columns)

    def plan_flag_mapq_group_count(self, flag_mask, flag_value, mapq_min, n_refs, columns=(0, 1, 2)):
        d = L.PlanDesc(kind=L.PLAN_FLAG_MAPQ_GROUP_COUNT, n_groups=n_refs, flag_mask=flag_mask,
                       flag_value=flag_value, mapq_min=mapq_min)
        return Plan(self, d, columns)

    def plan_cmp_avg_by_group(self, op, threshold, n_groups, columns=(0, 1, 2), x_type="f32", y_type="f32"):
        """x_type / y_type "i32": the compared column / AVG's argument holds Int32 values (an INFO field of Type=Integer);
        a plan fed by Stream.consume(scan) takes both from the file's header instead."""
        d = L.PlanDesc(kind=L.PLAN_CMP_AVG_BY_GROUP, n_groups=n_groups, cmp_op=CMP[op], threshold=threshold,
                       x_type=1 if x_type == "i32" else 0, y_type=1 if y_type == "i32" else 0)
        return Plan(self, d, columns)

    def plan_cmp_minmax_by_group(self, op, threshold, n_groups, columns=(0, 1, 2), x_type="f32", y_type="f32"):
        """MIN(y), MAX(y), COUNT(y), COUNT(*) GROUP BY g behind K4's predicate; the arguments are plan_cmp_avg_by_group's.
        State: 4 * n_groups int64 words, n_groups <= 4096."""
        d = L.PlanDesc(kind=L.PLAN_CMP_MINMAX_BY_GROUP, n_groups=n_groups, cmp_op=CMP[op], threshold=threshold,
                       x_type=1 if x_type == "i32" else 0, y_type=1 if y_type == "i32" else 0)
        return Plan(self, d, columns)

    def plan_qual_pos_hist(self, lmax, columns=(0,)):
        d = L.PlanDesc(kind=L.PLAN_QUAL_POS_HIST, lmax=lmax)
        return Plan(self, d, columns)

    def plan_read_stats_hist(self, lmax, columns=(0, 1)):
        """Per-read length / GC percent / mean quality histograms over (sequence, quality_scores): columns (2, 3) of a FASTQ
        scan.  State: read_stats_layout(lmax)[4] int64 words, all of which add."""
        d = L.PlanDesc(kind=L.PLAN_READ_STATS_HIST, lmax=lmax)
        return Plan(self, d, columns)

    def plan_seq_stats_hist(self, lmax, columns=(0,)):
        """Per-record totals, byte composition and length / log2 length / GC percent histograms over one Utf8 column (sequence):
        column 2 of a FASTA scan and of a FASTQ scan.  State: seq_stats_layout(lmax)[5] int64 words, all of which add."""
        d = L.PlanDesc(kind=L.PLAN_SEQ_STATS_HIST, lmax=lmax)
        return Plan(self, d, columns)

    def plan_region_set_overlap(self, regions, columns=(2, 3, 4)):
        """K6's overlap count for every region of a set in one pass over the rows (plan kind 11).  `regions`: (contig, start, end)
        triples, 1-based inclusive, end None = open; contig an int (reference ids, the caller's or the file's own) in all of them
        or a str (names, resolved by every consumed scan in its own header order) in all of them.  State: 4 + 2 * (M + C) int64
        words, all of which add; RegionSetPlan.decode turns them into one count per region, finish_arrow into a table."""
        return RegionSetPlan(self, regions, columns)

    def region_set_overlap(self, ref_id, ref_valid, start, start_valid, end, end_valid, n, plan, d_state, stream=None):
        """K11 (bare operator, ids form): accumulates the batch into `d_state` (plan.n_i64 int64 words)."""
        c0, c1, c2 = _col(ref_id, ref_valid, None, n), _col(start, start_valid, None, n), _col(end, end_valid, None, n)
        self._check(self.lib.exon_hip_region_set_overlap(self.h, stream, C.byref(c0), C.byref(c1), C.byref(c2), n, plan.h,
                                                         d_state.ptr if isinstance(d_state, DeviceBuffer) else d_state))

    def plan_region_set_bases(self, regions, columns=(2, 3, 4)):
        """The bases of the rows that fall inside every region of a set, in one pass over the rows (plan kind 12): for region i the
        sum over the counted rows [s, e] of max(0, min(e, end_i) - max(s, start_i) + 1).  `regions` as plan_region_set_overlap's.
        State: 4 + 4 * (P + C) int64 words, all of which add modulo 2^64; RegionBasesPlan.decode turns them into one sum per region,
        finish_arrow into a table."""
        return RegionBasesPlan(self, regions, columns)

    def region_set_bases(self, ref_id, ref_valid, start, start_valid, end, end_valid, n, plan, d_state, stream=None):
        """K12 (bare operator, ids form): accumulates the batch into `d_state` (plan.n_i64 int64 words)."""
        c0, c1, c2 = _col(ref_id, ref_valid, None, n), _col(start, start_valid, None, n), _col(end, end_valid, None, n)
        self._check(self.lib.exon_hip_region_set_bases(self.h, stream, C.byref(c0), C.byref(c1), C.byref(c2), n, plan.h,
                                                       d_state.ptr if isinstance(d_state, DeviceBuffer) else d_state))

    def plan_window_bases(self, contigs, window, columns=(2, 3, 4)):
        """The bases of the rows inside every window of width `window` along each contig, in one pass over the rows (plan kind 13).
        `contigs`: (contig, length) pairs, contig an int (reference ids) in all of them or a str (names, resolved by every consumed
        scan in its own header order) in all of them.  Window j of a contig is [j * window + 1, min((j + 1) * window, length)]; rows
        are clipped to [1, length].  State: 4 + 2 * B int64 words, all of which add modulo 2^64; WindowBasesPlan.decode turns them
        into one sum per window, finish_arrow into a table."""
        return WindowBasesPlan(self, contigs, window, columns)

    def plan_region_set_depth(self, regions, thresholds, columns=(2, 3, 4)):
        """The per-base depth over the bases a region set covers, in one pass over the rows (plan kind 14), and per region its bases
        and how many of them are covered at least thresholds[t] times.  `regions` as plan_region_set_overlap's, with finite ends;
        `thresholds`: up to 8 strictly increasing depths >= 1.  State: 4 + T + C int64 words, all of which add modulo 2^64; the decode
        is not linear: add partial states first.  RegionDepthPlan.decode / .reduce make the table, finish_arrow serves it."""
        return RegionDepthPlan(self, regions, thresholds, columns)

    def region_set_depth(self, ref_id, ref_valid, start, start_valid, end, end_valid, n, plan, d_state, stream=None):
        """K14 (bare operator, ids form): accumulates the batch into `d_state` (plan.n_i64 int64 words)."""
        c0, c1, c2 = _col(ref_id, ref_valid, None, n), _col(start, start_valid, None, n), _col(end, end_valid, None, n)
        self._check(self.lib.exon_hip_region_set_depth(self.h, stream, C.byref(c0), C.byref(c1), C.byref(c2), n, plan.h,
                                                       d_state.ptr if isinstance(d_state, DeviceBuffer) else d_state))

    def window_bases(self, ref_id, ref_valid, start, start_valid, end, end_valid, n, plan, d_state, stream=None):
        """K13 (bare operator, ids form): accumulates the batch into `d_state` (plan.n_i64 int64 words)."""
        c0, c1, c2 = _col(ref_id, ref_valid, None, n), _col(start, start_valid, None, n), _col(end, end_valid, None, n)
        self._check(self.lib.exon_hip_window_bases(self.h, stream, C.byref(c0), C.byref(c1), C.byref(c2), n, plan.h,
                                                   d_state.ptr if isinstance(d_state, DeviceBuffer) else d_state))

    def cigar_blocks(self, ref_id, ref_valid, start, start_valid, cigar_offsets, cigar_ops, n, cover_ops, out_ref, out_start, out_end, out_valid,
                     cap, stream=None):
        """exon_hip_cigar_blocks: n alignment rows and their CIGAR ops (an Arrow List<UInt32> on the device, `len << 4 | code`) -> the
        aligned block rows kinds 12 - 14 take in place of the spans.  Returns the rows emitted.  Synchronous.  A `cap` too small
        raises ExonHipError(ECAPACITY) with the need in its `.need`; nothing has been written then."""
        def p(x):
            return None if x is None else x.ptr if isinstance(x, DeviceBuffer) else int(x)
        c0, c1 = _col(ref_id, ref_valid, None, n), _col(start, start_valid, None, n)
        need = C.c_int64()
        rc = self.lib.exon_hip_cigar_blocks(self.h, stream, C.byref(c0), C.byref(c1), p(cigar_offsets), p(cigar_ops), n, cover_ops_mask(cover_ops),
                                            p(out_ref), p(out_start), p(out_end), p(out_valid), int(cap), C.byref(need))
        if rc < 0:
            e = ExonHipError(rc, self._last_error())
            e.need = need.value
            raise e
        return need.value


def cover_ops_mask(cover_ops):
    """'aligned' (M = X: `samtools depth`, `bedcov -j`), 'aligned+del' (+ D: `samtools depth -J`) or the mask itself"""
    if isinstance(cover_ops, str):
        try:
            return {"aligned": L.COVER_ALIGNED, "aligned+del": L.COVER_ALIGNED_DEL}[cover_ops]
        except KeyError:
            raise ValueError(f"cover_ops {cover_ops!r}: 'aligned', 'aligned+del' or a mask of BAM op codes") from None
    return int(cover_ops)


def cigar_blocks_host(ops, start, cover_ops, cap=None):
    """exon_hip_cigar_blocks_host (host-only): the aligned blocks [(first, last)] of one record whose ops are `len << 4 | code`.
    `cap`: room for that many blocks (default: all of them); fewer than the record has raises ExonHipError(ECAPACITY), `.need` = k."""
    lib = L.load()
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    cap = len(ops) if cap is None else int(cap)
    s, e = np.empty(max(cap, 1), np.int64), np.empty(max(cap, 1), np.int64)
    k = C.c_int32()
    rc = lib.exon_hip_cigar_blocks_host(ops.ctypes.data if len(ops) else None, len(ops), int(start), cover_ops_mask(cover_ops), s.ctypes.data, e.ctypes.data, cap, C.byref(k))
    if rc < 0:
        err = ExonHipError(rc, lib.exon_hip_last_error(None).decode(errors="replace"))
        err.need = k.value
        raise err
    return list(zip(s[:k.value].tolist(), e[:k.value].tolist()))


def region_bases_layout(plan):
    """exon_hip_region_bases_layout (host-only): word offsets of the totals / Ns / Ss / Ne / Se sections of a kind-12 plan's state,
    and its size in words."""
    return plan.layout()


def region_bases_decode(plan, state):
    """exon_hip_region_bases_decode (host-only): the state's words -> the covered bases of every region, in the order the regions
    were given.  Linear modulo 2^64: the decoded states of partitions add up to the decoded merged state."""
    return plan.decode(state)


def region_set_layout(plan):
    """exon_hip_region_set_layout (host-only): word offsets of the totals / A / B sections of a region-set plan's state, and its
    size in words."""
    return plan.layout()


def region_set_decode(plan, state):
    """exon_hip_region_set_decode (host-only): the state's words -> one count per region, in the order the regions were given.
    Linear: the decoded states of partitions add up to the decoded merged state."""
    return plan.decode(state)


def seq_stats_layout(lmax):
    """exon_hip_seq_stats_layout (host-only): word offsets of the totals / composition / length / length_log2 / gc_percent
    sections of a per-record sequence statistics state, and its size in words."""
    lib = L.load()
    out = (C.c_int64 * 6)()
    rc = lib.exon_hip_seq_stats_layout(lmax, out)
    if rc:
        raise ExonHipError(rc, lib.exon_hip_last_error(None).decode(errors="replace"))
    return tuple(out)


def read_stats_layout(lmax):
    """exon_hip_read_stats_layout (host-only): word offsets of the totals / length / gc_percent / mean_quality sections of a
    per-read statistics state, and its size in words."""
    lib = L.load()
    out = (C.c_int64 * 5)()
    rc = lib.exon_hip_read_stats_layout(lmax, out)
    if rc:
        raise ExonHipError(rc, lib.exon_hip_last_error(None).decode(errors="replace"))
    return tuple(out)


def minmax_decode(words, is_min, y_type="f32"):
    """exon_hip_minmax_decode (host-only): state words of a MIN / MAX plan's min plane (is_min) or max plane ->
    (values float32 / int32 array, valid bool array); a word of 0 is "no value"."""
    lib = L.load()
    w = np.ascontiguousarray(words, np.int64)
    vals = np.zeros(len(w), np.int32 if y_type == "i32" else np.float32)
    valid = np.zeros(len(w), np.uint8)
    rc = lib.exon_hip_minmax_decode(w.ctypes.data if len(w) else None, len(w), 1 if is_min else 0, 1 if y_type == "i32" else 0,
                                    vals.ctypes.data if len(w) else None, valid.ctypes.data if len(w) else None)
    if rc:
        raise ExonHipError(rc, lib.exon_hip_last_error(None).decode(errors="replace"))
    return vals, valid.astype(bool)


def bgzf_scan(data, out_base=0):
    """Walk the BGZF block headers of `data` (bytes / uint8 array) -> (ctypes BgzfBlock array, n, consumed, out_bytes).
    Host-only helper of the C ABI (exon_hip_bgzf_scan)."""
    lib = L.load()
    buf = np.frombuffer(data, np.uint8)
    n, consumed, out_bytes = C.c_int32(), C.c_size_t(), C.c_size_t()
    ptr = buf.ctypes.data if len(buf) else None
    rc = lib.exon_hip_bgzf_scan(ptr, len(buf), out_base, None, 1 << 30, C.byref(n), C.byref(consumed), C.byref(out_bytes))
    if rc:
        raise ExonHipError(rc, lib.exon_hip_last_error(None).decode(errors="replace"))
    blocks = (L.BgzfBlock * max(n.value, 1))()
    rc = lib.exon_hip_bgzf_scan(ptr, len(buf), out_base, blocks, n.value, C.byref(n), C.byref(consumed), C.byref(out_bytes))
    if rc:
        raise ExonHipError(rc, lib.exon_hip_last_error(None).decode(errors="replace"))
    return blocks, n.value, consumed.value, out_bytes.value


def parse_region(region):
    """`name[:start[-end]]` -> (name, start, end|None)   (host helper of the C ABI)."""
    lib = L.load()
    name = C.create_string_buffer(512)
    a, b = C.c_int64(), C.c_int64()
    rc = lib.exon_hip_parse_region(region.encode(), name, 512, C.byref(a), C.byref(b))
    if rc:
        raise ExonHipError(rc, lib.exon_hip_last_error(None).decode(errors="replace"))
    return name.value.decode(), a.value, (None if b.value == L.REGION_OPEN_END else b.value)


def index_query(index_path, region=None, ref_id=None, start=1, end=None, is_bai=False):
    """Region -> list of (start, end) BGZF virtual-position chunks from a .tbi / .bai index."""
    lib = L.load()
    name = None
    if region is not None:
        name, start, end = parse_region(region)
    cap = 4096
    st, en = (C.c_uint64 * cap)(), (C.c_uint64 * cap)()
    n = C.c_int32()
    rc = lib.exon_hip_index_query(str(index_path).encode(), 1 if is_bai else 0, name.encode() if name else None,
                                  -1 if ref_id is None else ref_id, start, L.REGION_OPEN_END if end is None else end,
                                  st, en, cap, C.byref(n))
    if rc:
        raise ExonHipError(rc, lib.exon_hip_last_error(None).decode(errors="replace"))
    return [(st[i], en[i]) for i in range(min(n.value, cap))]


def pack_names(names):
    """'\\0'-terminated names back to back (the wire form of a key dictionary in the C ABI)."""
    return b"".join((n if isinstance(n, bytes) else n.encode()) + b"\0" for n in names)


def unpack_names(packed, n):
    parts = packed.split(b"\0")[:n]
    return [p.decode(errors="replace") for p in parts]


def keys_union(dicts):
    """exon_hip_keys_union (host-only C): the union of the ranks' dictionaries in rank order, first appearance first.
    Returns (union names, [per-rank list: union id of every local id])."""
    lib = L.load()
    packed = b"".join(pack_names(d) for d in dicts)
    n_keys = (C.c_int32 * len(dicts))(*[len(d) for d in dicts])
    n_out, nb = C.c_int32(), C.c_size_t()
    maps = (C.c_int32 * max(1, sum(len(d) for d in dicts)))()
    rc = lib.exon_hip_keys_union(packed, len(packed), n_keys, len(dicts), None, 0, C.byref(n_out), C.byref(nb), maps)
    if rc:
        raise ExonHipError(rc, lib.exon_hip_last_error(None).decode(errors="replace"))
    buf = C.create_string_buffer(max(nb.value, 1))
    rc = lib.exon_hip_keys_union(packed, len(packed), n_keys, len(dicts), buf, nb.value, C.byref(n_out), C.byref(nb), maps)
    if rc:
        raise ExonHipError(rc, lib.exon_hip_last_error(None).decode(errors="replace"))
    out, o = [], 0
    for d in dicts:
        out.append(list(maps[o:o + len(d)]))
        o += len(d)
    return unpack_names(buf.raw[:nb.value], n_out.value), out


def regroup_files_by_size(sizes, target_groups):
    """Whole-file round-robin repartition; returns a list of groups of ORIGINAL file indexes."""
    lib = L.load()
    n = len(sizes)
    s = (C.c_int64 * max(n, 1))(*sizes)
    g = (C.c_int32 * max(n, 1))()
    ng = lib.exon_hip_regroup_files_by_size(s, n, target_groups, g)
    if ng < 0:
        raise ExonHipError(ng, lib.exon_hip_last_error(None).decode(errors="replace"))
    groups = [[] for _ in range(ng)]
    for i in sorted(range(n), key=lambda i: (sizes[i], i)):
        groups[g[i]].append(i)
    return groups


class Scan:
    """Native decoder + device-layout array builder over one file (FileOpener::open + read_batch analogue).
    CPU-only: usable without a GPU."""

    PROJECT = {"vcf": {"id": 1, "ref": 2, "alt": 4, "info": 8, "formats": 16}, "bam": {"name": 1, "cigar": 2, "sequence": 4, "quality_score": 8},
               "bcf": {"id": 1, "ref": 2, "alt": 4}, "sam": {"name": 1, "cigar": 2, "sequence": 4, "quality_score": 8},
               "gff": {"attributes": 256}, "gtf": {"attributes": 256}, "bed": L.PROJECT_BED}

    def __init__(self, path, fmt, compression=None, batch_size=0, info_field=None, region=None, use_index=False,
                 gpu_parse=False, project=(), where=None, where_flags=None, formats_on_device=False, cover_ops=None):
        """cover_ops: "aligned" (M = X: `samtools depth`, `bedcov -j`), "aligned+del" (+ D: `samtools depth -J`) or a mask of BAM op
        codes inside 0x18D (exon_hip_scan_set_cover_ops; BAM, SAM): BLOCKS MODE -- plans of kinds 12, 13 and 14 get every kept record
        as its aligned blocks instead of its span; nothing else may read the scan.
        formats_on_device: VCF, next to "formats" in `project`: the modifier EXON_HIP_PROJECT_VCF_FORMATS_ON_DEVICE -- a gpu_parse scan
        then prints the column on the device instead of decoding on the host (no column of its own; the open refuses it without "formats").
        where_flags: (mask, value[, mapq_min]), the flag / mapping-quality predicate a BAM or SAM scan evaluates itself
        (exon_hip_scan_set_flag_predicate): rows with (flag & mask) != value, or -- for a mapq_min >= 0 -- a NULL or smaller
        mapping_quality, are not emitted (ANDed with `region`).
        where: (column, op, literal), one comparison the scan evaluates itself (exon_hip_scan_set_predicate): `column` a scan column
        (VCF: 2 = qual, 4 + k = typed INFO field k of info_field; Float32, or Int32 values), `op` one of ">" ">=" "<" "<=" "=" "!=";
        rows whose column is NULL or fails are not emitted (ANDed with `region`).
        project: names of the reference's columns beyond the fused kernels' operands (EXON_HIP_PROJECT_*): VCF "id", "ref", "alt",
        "info", "formats" (the last two as the reference's unparsed Utf8 columns; info from the GPU pipeline too, formats only with formats_on_device);
        BAM "name", "cigar", "sequence", "quality_score" -- appended behind the default columns in that order; GFF "attributes"
        (the reference's Map<Utf8, List<Utf8>>, column 8); GTF "attributes" (the reference's Map<Utf8, Utf8>, column 8); BED "name",
        "score", "strand", "thick_start", "thick_end", "color", "block_count", "block_sizes", "block_starts" (bits 3 .. 11: the
        reference's n_fields = k is the first k - 3 of them), appended behind reference_sequence_name / start / end in that order."""
        self.lib = L.load()
        self.fmt = fmt
        mask = 0
        for name in project:
            mask |= self.PROJECT[fmt][name]
        if formats_on_device:  # (a modifier, not a name of PROJECT: it adds no column)
            if fmt != "vcf":
                raise ValueError("formats_on_device is an option of VCF scans")
            mask |= L.PROJECT_VCF_FORMATS_ON_DEVICE
        opt = L.ScanOptions(L.FORMATS[fmt], L.COMPRESSION[compression], batch_size,
                            info_field.encode() if info_field else None, region.encode() if region else None,
                            1 if use_index else 0, 1 if gpu_parse else 0, mask)
        h = C.c_void_p()
        rc = self.lib.exon_hip_scan_open(str(path).encode(), C.byref(opt), C.byref(h))
        if rc:
            raise ExonHipError(rc, self.lib.exon_hip_last_error(None).decode(errors="replace"))
        self.h = h
        if where is not None:
            try:
                self.set_predicate(*where)
            except Exception:
                self.close()
                raise
        if where_flags is not None:
            try:
                self.set_flag_predicate(*where_flags)
            except Exception:
                self.close()
                raise
        if cover_ops is not None and cover_ops != 0:  # (0 is "off", like None: no call, so no refusal on a format without a CIGAR)
            try:
                self.set_cover_ops(cover_ops)
            except Exception:
                self.close()
                raise

    WHERE_OPS = {">": 0, ">=": 1, "<": 2, "<=": 3, "=": 4, "!=": 5}

    def set_predicate(self, column, op, literal):
        """exon_hip_scan_set_predicate: before bind_ctx / the first batch / Stream.consume; a second call replaces the first.  `op` may
        be the C ABI's integer too."""
        self._check(self.lib.exon_hip_scan_set_predicate(self.h, column, self.WHERE_OPS[op] if isinstance(op, str) else op, float(literal)))
        return self

    def set_flag_predicate(self, mask, value, mapq_min=-1):
        """exon_hip_scan_set_flag_predicate (BAM, SAM): before bind_ctx / the first batch / Stream.consume; a second call replaces the
        first.  mapq_min < 0: no conjunct on mapping_quality."""
        self._check(self.lib.exon_hip_scan_set_flag_predicate(self.h, int(mask), int(value), int(mapq_min)))
        return self

    def set_cover_ops(self, cover_ops):
        """exon_hip_scan_set_cover_ops (BAM, SAM): before the first Stream.consume; a second call replaces the first, 0 turns blocks mode
        off.  `cover_ops`: "aligned", "aligned+del" or the mask."""
        self._check(self.lib.exon_hip_scan_set_cover_ops(self.h, cover_ops_mask(cover_ops)))
        return self

    def export_stats(self):
        """After the scan has ended: {"slabs", "compacted_slabs", "d2h_bytes"} of the GPU pipeline's batch export (exon_hip_scan_export_stats)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.exon_hip_scan_export_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"slabs": a.value, "compacted_slabs": b.value, "d2h_bytes": c.value}

    def _check(self, rc):
        if rc < 0:
            raise ExonHipError(rc, self.lib.exon_hip_last_error(None).decode(errors="replace"))
        return rc

    def schema(self):
        import pyarrow as pa
        sch = L.ArrowSchema()
        self._check(self.lib.exon_hip_scan_schema(self.h, C.byref(sch)))
        return pa.DataType._import_from_c(C.addressof(sch))

    def next_raw(self):
        """-> ctypes ArrowArray (caller must release or move it) or None at end of stream."""
        arr = L.ArrowArray()
        rc = self._check(self.lib.exon_hip_scan_next(self.h, C.byref(arr)))
        return None if rc == 1 else arr

    def __iter__(self):
        """Batches as pyarrow StructArrays (imports = moves each batch)."""
        import pyarrow as pa
        while True:
            arr = self.next_raw()
            if arr is None:
                return
            sch = L.ArrowSchema()
            self._check(self.lib.exon_hip_scan_schema(self.h, C.byref(sch)))
            yield pa.Array._import_from_c(C.addressof(arr), C.addressof(sch))

    def bind_ctx(self, ctx):
        """Batches of a scan opened with gpu_parse=True come out of the GPU decode pipeline on `ctx` (exon_hip_scan_bind_ctx): iterate
        the scan as usual afterwards."""
        self._check(self.lib.exon_hip_scan_bind_ctx(self.h, ctx.h))
        return self

    def decoded_on_gpu(self):
        """(decoded, inflated) of the last Stream.consume: were the records decoded / the BGZF blocks inflated on the GPU?"""
        d, i = C.c_int32(), C.c_int32()
        self._check(self.lib.exon_hip_scan_decoded_on_gpu(self.h, C.byref(d), C.byref(i)))
        return bool(d.value), bool(i.value)

    def dictionary_size(self, column):
        n = C.c_int32()
        self._check(self.lib.exon_hip_scan_dictionary_size(self.h, column, C.byref(n)))
        return n.value

    def dictionary(self, column):
        out = []
        for i in range(self.dictionary_size(column)):
            p = C.c_char_p()
            self._check(self.lib.exon_hip_scan_dictionary_value(self.h, column, i, C.byref(p)))
            out.append(p.value.decode(errors="replace"))
        return out

    def intern(self, column, name):
        i = C.c_int32()
        self._check(self.lib.exon_hip_scan_dictionary_intern(self.h, column, name.encode(), C.byref(i)))
        return i.value

    def rows(self):
        n = C.c_int64()
        self._check(self.lib.exon_hip_scan_rows(self.h, C.byref(n)))
        return n.value

    def reference_lengths(self):
        """The header's reference lengths in dictionary-id order (BAM, SAM, CRAM; a SAM @SQ without LN gives 0), as dictionary(2)
        gives the names (exon_hip_scan_reference_lengths)."""
        n = C.c_int32()
        self._check(self.lib.exon_hip_scan_reference_lengths(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int64)
        self._check(self.lib.exon_hip_scan_reference_lengths(self.h, out.ctypes.data, n.value, C.byref(n)))
        return [int(x) for x in out[:n.value]]

    def index_chunks(self):
        n = C.c_int32()
        self._check(self.lib.exon_hip_scan_index_chunks(self.h, C.byref(n)))
        return n.value

    def close(self):
        if self.h:
            self.lib.exon_hip_scan_close(self.h)
            self.h = None


class VCFParser:
    """VCF record parsing on the GPU (exon_hip_vcf_parser_*): text slab in HBM -> device-layout columns in HBM."""

    def __init__(self, ctx, contigs, info_field=None, max_slab_bytes=64 << 20, key_types=None, format_key_types=None):
        """key_types: {INFO key: "i" | "f" | "b" | "c" | "s"} as the header's ##INFO lines type them, for the `info` text column
        (parse_host(..., info_text=True)); {} = the reserved keys of the specification alone.
        format_key_types: {FORMAT key: "i" | "f" | "c" | "s"} as the ##FORMAT lines type them, for the `formats` text column
        (parse_host(..., formats_text=True)); {} = the reserved FORMAT keys alone (GT is known by its name)."""
        self.ctx = ctx
        names = (C.c_char_p * max(len(contigs), 1))(*[c.encode() for c in contigs])
        h = C.c_void_p()
        ctx._check(ctx.lib.exon_hip_vcf_parser_create(ctx.h, names, len(contigs), info_field.encode() if info_field else None,
                                                      max_slab_bytes, C.byref(h)))
        self.h = h
        if key_types is not None:
            self.set_key_types(key_types)
        if format_key_types is not None:
            self.set_format_key_types(format_key_types)
        self.has_info = bool(info_field)
        self.cap_items = max_slab_bytes // 2 + 1  # items a list key's buffers hold (exon_hip_vcf_parser_create)

    def parse_device(self, d_text, n_bytes, stream=None):
        cols = L.VCFColumns()
        ptr = d_text.ptr if isinstance(d_text, DeviceBuffer) else int(d_text)
        self.ctx._check(self.ctx.lib.exon_hip_vcf_parser_parse(self.h, stream, ptr, n_bytes, C.byref(cols)))
        return cols

    def set_key_types(self, key_types):
        """The value types of the header's INFO keys (exon_hip_vcf_parser_set_key_types)."""
        packed = b"".join(k.encode() + b"\0" for k in key_types)
        kinds = "".join(key_types.values()).encode()
        self.ctx._check(self.ctx.lib.exon_hip_vcf_parser_set_key_types(self.h, packed, kinds, len(key_types)))

    def set_format_key_types(self, key_types):
        """The value types of the header's FORMAT keys (exon_hip_vcf_parser_set_format_key_types)."""
        packed = b"".join(k.encode() + b"\0" for k in key_types)
        kinds = "".join(key_types.values()).encode()
        self.ctx._check(self.ctx.lib.exon_hip_vcf_parser_set_format_key_types(self.h, packed, kinds, len(key_types)))

    def parse_host(self, text, misalign=0, info_text=False, formats_text=False):
        """Test helper: copy `text` (bytes of complete lines) to HBM (`misalign` bytes past a 16-byte boundary), parse,
        bring the columns back as numpy arrays.  info_text: the `info` Utf8 column too, printed on the device
        (exon_hip_vcf_parser_info_text): res["info_text"] = {"n_bytes", "n_undecided"} + "offsets" / "values" when 0 rows are
        undecided (nothing when the parse itself left rows undecided).  formats_text: the same for the `formats` column
        (exon_hip_vcf_parser_formats_text): res["formats_text"]."""
        buf = np.frombuffer(text, np.uint8)
        d = self.ctx.to_device(np.concatenate([np.full(misalign, 10, np.uint8), buf, np.zeros(64, np.uint8)]))
        cols = self.parse_device(d.ptr + misalign, len(buf))
        n = cols.n_rows
        nb = (n + 7) // 8

        def get(ptr, dtype, count):
            out = np.empty(count, dtype)
            if count:
                self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(out), ptr, out.nbytes, None))
            return out

        res = {"n_rows": n, "n_undecided": cols.n_undecided, "consumed_bytes": cols.consumed_bytes,
               "chrom_id": get(cols.chrom_id, np.int32, n), "pos": get(cols.pos, np.int64, n),
               "pos_valid": get(cols.pos_valid, np.uint8, nb), "qual": get(cols.qual, np.float32, n),
               "qual_valid": get(cols.qual_valid, np.uint8, nb), "filter_id": get(cols.filter_id, np.int32, n)}
        if self.has_info:
            res["info"] = get(cols.info, np.float32, n)
            res["info_valid"] = get(cols.info_valid, np.uint8, nb)
            # every key: {"kind", "valid"} + "values" (scalar kinds: one 4-byte slot per row) or, for the list kinds 'F' / 'I',
            # "offsets" (n + 1), "values" (the items) and "item_valid" (their bitmap); nothing but the validity for a Flag
            res["infos"] = []
            for q in range(cols.n_info):
                kind = cols.info_kinds[q:q + 1].decode()
                k = {"kind": kind, "valid": get(cols.infos_valid[q], np.uint8, nb)}
                if kind in "FI":
                    k["offsets"] = get(cols.list_offsets[q], np.int32, n + 1 if n else 0)
                    items = min(int(k["offsets"][-1]) if n else 0, self.cap_items)  # (more items than the buffers hold: an undecided slab)
                    k["values"] = get(cols.infos[q], np.float32, items)
                    k["item_valid"] = get(cols.list_item_valid[q], np.uint8, (items + 7) // 8)
                elif kind != "b":
                    k["values"] = get(cols.infos[q], np.float32, n)
                res["infos"].append(k)
        if info_text and cols.n_undecided == 0 and n:
            t = L.VCFInfoText()
            self.ctx._check(self.ctx.lib.exon_hip_vcf_parser_info_text(self.h, None, C.byref(t)))
            it = {"n_bytes": t.n_bytes, "n_undecided": t.n_undecided}
            if t.n_undecided == 0:
                it["offsets"] = get(t.offsets, np.int32, n + 1)
                it["values"] = get(t.values, np.uint8, t.n_bytes)
            res["info_text"] = it
        if formats_text and cols.n_undecided == 0 and n:
            t = L.VCFInfoText()
            self.ctx._check(self.ctx.lib.exon_hip_vcf_parser_formats_text(self.h, None, C.byref(t)))
            ft = {"n_bytes": t.n_bytes, "n_undecided": t.n_undecided}
            if t.n_undecided == 0:
                ft["offsets"] = get(t.offsets, np.int32, n + 1)
                ft["values"] = get(t.values, np.uint8, t.n_bytes)
            res["formats_text"] = ft
        return res

    def filters(self):
        n = C.c_int32()
        buf = C.create_string_buffer((1 << 20) + 4096)  # the dictionary's text pool plus one NUL per name (EXON_HIP_MAX_GROUPS)
        self.ctx._check(self.ctx.lib.exon_hip_vcf_parser_filters(self.h, buf, len(buf), C.byref(n)))
        names, o = [], 0
        raw = buf.raw
        for _ in range(n.value):
            e = raw.index(b"\0", o)
            names.append(raw[o:e].decode(errors="replace"))
            o = e + 1
        return names

    def close(self):
        if self.h:
            self.ctx.lib.exon_hip_vcf_parser_destroy(self.h)
            self.h = None


class GFFParser:
    """GFF3 record parsing on the GPU (exon_hip_gff_parser_*): text slab in HBM -> the GFF device layout in HBM.  The seqname, source
    and type dictionaries grow across slabs; `seed_seqnames` take the ids 0 .. len - 1 before the first slab.
    dialect="gtf": the same parser under the GTF rules (exon_hip_gff_parser_set_dialect) -- a '?' strand is undecided, and the
    attributes column is Map<Utf8, Utf8> (exon_hip_gff_parser_gtf_attributes)."""

    def __init__(self, ctx, seed_seqnames=(), max_slab_bytes=64 << 20, dialect="gff"):
        self.ctx = ctx
        self.dialect = dialect
        names = (C.c_char_p * max(len(seed_seqnames), 1))(*[c.encode() for c in seed_seqnames])
        h = C.c_void_p()
        ctx._check(ctx.lib.exon_hip_gff_parser_create(ctx.h, names, len(seed_seqnames), max_slab_bytes, C.byref(h)))
        self.h = h
        if dialect != "gff":
            ctx._check(ctx.lib.exon_hip_gff_parser_set_dialect(h, L.FORMATS[dialect]))

    def parse_device(self, d_text, n_bytes, stream=None):
        cols = L.GFFColumns()
        ptr = d_text.ptr if isinstance(d_text, DeviceBuffer) else int(d_text)
        self.ctx._check(self.ctx.lib.exon_hip_gff_parser_parse(self.h, stream, ptr, n_bytes, C.byref(cols)))
        return cols

    def parse_host(self, text, misalign=0, attributes=False, all_rows=False):
        """Test helper: copy `text` to HBM (`misalign` bytes past a 16-byte boundary), parse, bring the columns back as numpy arrays
        (none of them when the device left a row undecided).  attributes: the `attributes` column too, built on the device
        (exon_hip_gff_parser_attributes): res["attributes"] = its six buffers, four totals and n_undecided (buffers only when 0);
        for the GTF dialect (exon_hip_gff_parser_gtf_attributes) its five buffers, three totals and n_undecided.
        all_rows: the columns of an undecided slab too (its decided rows hold their values; dictionary ids are provisional)."""
        buf = np.frombuffer(text, np.uint8)
        d = self.ctx.to_device(np.concatenate([np.full(misalign, 10, np.uint8), buf, np.zeros(64, np.uint8)]))
        self.ctx._check(self.ctx.lib.exon_hip_gff_parser_want_attributes(self.h, 1 if attributes else 0))
        cols = self.parse_device(d.ptr + misalign, len(buf))
        n = cols.n_rows if cols.n_undecided == 0 or all_rows else 0
        nb = (n + 7) // 8

        def get(ptr, dtype, count):
            out = np.empty(count, dtype)
            if count:
                self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(out), ptr, out.nbytes, None))
            return out

        res = {"n_rows": cols.n_rows, "n_undecided": cols.n_undecided, "consumed_bytes": cols.consumed_bytes}
        for name in ("seqname_id", "source_id", "type_id", "strand_id", "phase_id"):
            res[name] = get(getattr(cols, name), np.int32, n)
        for name in ("start", "end"):
            res[name] = get(getattr(cols, name), np.int64, n)
        res["score"] = get(cols.score, np.float32, n)
        for name in ("score_valid", "strand_valid", "phase_valid"):
            res[name] = get(getattr(cols, name), np.uint8, nb)
        if attributes and cols.n_undecided == 0 and self.dialect == "gtf":
            a = L.GTFAttributes()
            self.ctx._check(self.ctx.lib.exon_hip_gff_parser_gtf_attributes(self.h, None, C.byref(a)))
            at = {k: getattr(a, k) for k in ("n_entries", "n_key_bytes", "n_value_bytes", "n_undecided")}
            if a.n_undecided == 0 and n:
                at["map_offsets"] = get(a.map_offsets, np.int32, n + 1)
                at["key_offsets"] = get(a.key_offsets, np.int32, a.n_entries + 1)
                at["key_values"] = get(a.key_values, np.uint8, a.n_key_bytes)
                at["value_offsets"] = get(a.value_offsets, np.int32, a.n_entries + 1)
                at["value_values"] = get(a.value_values, np.uint8, a.n_value_bytes)
            res["attributes"] = at
        elif attributes and cols.n_undecided == 0:
            a = L.GFFAttributes()
            self.ctx._check(self.ctx.lib.exon_hip_gff_parser_attributes(self.h, None, C.byref(a)))
            at = {k: getattr(a, k) for k in ("n_entries", "n_items", "n_key_bytes", "n_item_bytes", "n_undecided")}
            if a.n_undecided == 0 and n:
                at["map_offsets"] = get(a.map_offsets, np.int32, n + 1)
                at["key_offsets"] = get(a.key_offsets, np.int32, a.n_entries + 1)
                at["key_values"] = get(a.key_values, np.uint8, a.n_key_bytes)
                at["list_offsets"] = get(a.list_offsets, np.int32, a.n_entries + 1)
                at["item_offsets"] = get(a.item_offsets, np.int32, a.n_items + 1)
                at["item_values"] = get(a.item_values, np.uint8, a.n_item_bytes)
            res["attributes"] = at
        return res

    def names(self, column):
        """The dictionary of column 0 (seqname), 1 (source) or 2 (type) discovered so far, in id order."""
        n = C.c_int32()
        buf = C.create_string_buffer((1 << 20) + 4096)
        self.ctx._check(self.ctx.lib.exon_hip_gff_parser_names(self.h, column, buf, len(buf), C.byref(n)))
        names, o = [], 0
        raw = buf.raw
        for _ in range(n.value):
            e = raw.index(b"\0", o)
            names.append(raw[o:e].decode(errors="replace"))
            o = e + 1
        return names

    def close(self):
        if self.h:
            self.ctx.lib.exon_hip_gff_parser_destroy(self.h)
            self.h = None


class BEDParser:
    """BED record parsing on the GPU (exon_hip_bed_parser_*): text slab in HBM -> the BED device layout in HBM.  The
    reference_sequence_name dictionary grows across slabs; `seed_names` take the ids 0 .. len - 1 before the first slab."""

    def __init__(self, ctx, seed_names=(), max_slab_bytes=64 << 20):
        self.ctx = ctx
        names = (C.c_char_p * max(len(seed_names), 1))(*[c.encode() for c in seed_names])
        h = C.c_void_p()
        ctx._check(ctx.lib.exon_hip_bed_parser_create(ctx.h, names, len(seed_names), max_slab_bytes, C.byref(h)))
        self.h = h

    def parse_device(self, d_text, n_bytes, stream=None):
        cols = L.BEDColumns()
        ptr = d_text.ptr if isinstance(d_text, DeviceBuffer) else int(d_text)
        self.ctx._check(self.ctx.lib.exon_hip_bed_parser_parse(self.h, stream, ptr, n_bytes, C.byref(cols)))
        return cols

    def parse_host(self, text, misalign=0, projection=0, all_rows=False):
        """Test helper: copy `text` to HBM (`misalign` bytes past a 16-byte boundary), parse, bring the columns back as numpy arrays
        (none of them when the device left a row undecided).  projection: EXON_HIP_PROJECT_BED_* bits (exon_hip_bed_parser_want);
        with name, score or strand among them also score / strand / their validity and res["names"], the rows' names (None where
        NULL) cut from the slab by the device's (offset, length, validity).  0: the three operand columns alone.
        all_rows: the columns of an undecided slab too (its decided rows hold their values; dictionary ids are provisional)."""
        buf = np.frombuffer(text, np.uint8)
        d = self.ctx.to_device(np.concatenate([np.full(misalign, 10, np.uint8), buf, np.zeros(64, np.uint8)]))
        self.ctx._check(self.ctx.lib.exon_hip_bed_parser_want(self.h, projection))
        cols = self.parse_device(d.ptr + misalign, len(buf))
        n = cols.n_rows if cols.n_undecided == 0 or all_rows else 0
        nb = (n + 7) // 8

        def get(ptr, dtype, count):
            out = np.empty(count, dtype)
            if count:
                self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(out), ptr, out.nbytes, None))
            return out

        res = {"n_rows": cols.n_rows, "n_undecided": cols.n_undecided, "consumed_bytes": cols.consumed_bytes, "projected": bool(cols.score)}
        res["chrom_id"] = get(cols.chrom_id, np.int32, n)
        for name in ("start", "end"):
            res[name] = get(getattr(cols, name), np.int64, n)
        if cols.score:
            res["score"] = get(cols.score, np.int64, n)
            res["strand_id"] = get(cols.strand_id, np.int32, n)
            for name in ("score_valid", "strand_valid", "name_valid"):
                res[name] = get(getattr(cols, name), np.uint8, nb)
            off, ln = get(cols.name_off, np.uint32, n), get(cols.name_len, np.uint32, n)
            skip = misalign % 16  # the offsets count from the aligned address at or below the slab
            valid = np.unpackbits(res["name_valid"], bitorder="little")[:n].astype(bool)
            raw = buf.tobytes()
            res["name_len"] = ln
            res["names"] = [raw[int(o) - skip:int(o) - skip + int(k)] if v else None for o, k, v in zip(off, ln, valid)]
        return res

    def names(self):
        """The reference_sequence_name dictionary discovered so far, in id order."""
        n = C.c_int32()
        buf = C.create_string_buffer((1 << 20) + 4096)
        self.ctx._check(self.ctx.lib.exon_hip_bed_parser_names(self.h, buf, len(buf), C.byref(n)))
        names, o = [], 0
        raw = buf.raw
        for _ in range(n.value):
            e = raw.index(b"\0", o)
            names.append(raw[o:e].decode(errors="replace"))
            o = e + 1
        return names

    def close(self):
        if self.h:
            self.ctx.lib.exon_hip_bed_parser_destroy(self.h)
            self.h = None


class SAMParser:
    """SAM text parsing on the GPU (exon_hip_sam_parser_*): alignment lines in HBM -> the BAM device layout (flag, mapq, reference id,
    start, end) in HBM.  `references`: the header's @SQ names in order (their ids)."""

    def __init__(self, ctx, references, max_slab_bytes=64 << 20):
        self.ctx = ctx
        names = (C.c_char_p * max(len(references), 1))(*[r.encode() for r in references])
        h = C.c_void_p()
        ctx._check(ctx.lib.exon_hip_sam_parser_create(ctx.h, names, len(references), max_slab_bytes, C.byref(h)))
        self.h = h
        self.max_rows = max_slab_bytes // 12 + 1  # rows the column buffers hold (exon_hip_sam_parser_create)

    def parse_device(self, d_text, n_bytes, stream=None):
        cols = L.BAMColumns()
        ptr = d_text.ptr if isinstance(d_text, DeviceBuffer) else int(d_text)
        self.ctx._check(self.ctx.lib.exon_hip_sam_parser_parse(self.h, stream, ptr, n_bytes, C.byref(cols)))
        return cols

    def parse_host(self, text, misalign=0):
        """Test helper: copy `text` (complete alignment lines) to HBM (`misalign` bytes past a 16-byte boundary), parse, bring the
        columns back as numpy arrays -- of every row, undecided ones included (their slots hold whatever was there); of a slab
        with more lines than the row buffers hold (n_rows says how many, n_undecided is not 0) the rows that fit."""
        buf = np.frombuffer(text, np.uint8)
        d = self.ctx.to_device(np.concatenate([np.full(misalign, 10, np.uint8), buf, np.zeros(64, np.uint8)]))
        cols = self.parse_device(d.ptr + misalign, len(buf))
        n = min(cols.n_rows, self.max_rows)
        nb = (n + 7) // 8

        def get(ptr, dtype, count):
            out = np.empty(count, dtype)
            if count:
                self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(out), ptr, out.nbytes, None))
            return out

        return {"n_rows": cols.n_rows, "n_undecided": cols.n_undecided, "consumed_bytes": cols.consumed_bytes,
                "flag": get(cols.flag, np.int32, n), "mapq": get(cols.mapq, np.uint8, n),
                "mapq_valid": get(cols.mapq_valid, np.uint8, nb), "ref_id": get(cols.ref_id, np.int32, n),
                "ref_valid": get(cols.ref_valid, np.uint8, nb), "start": get(cols.start, np.int64, n),
                "end": get(cols.end, np.int64, n), "pos_valid": get(cols.pos_valid, np.uint8, nb)}

    def close(self):
        if self.h:
            self.ctx.lib.exon_hip_sam_parser_destroy(self.h)
            self.h = None


class BAMParser:
    """BAM record splitting + field extraction on the GPU (exon_hip_bam_parser_*): inflated bytes in HBM -> columns."""

    def __init__(self, ctx, n_references, max_slab_bytes=64 << 20):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.exon_hip_bam_parser_create(ctx.h, n_references, max_slab_bytes, C.byref(h)))
        self.h = h

    def parse_host(self, data):
        """Test helper: copy `data` (record bytes, starting at a record boundary) to HBM, split + extract, bring the
        columns back as numpy arrays."""
        buf = np.frombuffer(data, np.uint8)
        d = self.ctx.to_device(np.concatenate([buf, np.zeros(64, np.uint8)]))
        cols = L.BAMColumns()
        self.ctx._check(self.ctx.lib.exon_hip_bam_parser_parse(self.h, None, d.ptr, len(buf), C.byref(cols)))
        n = cols.n_rows if cols.n_undecided == 0 else 0
        nb = (n + 7) // 8

        def get(ptr, dtype, count):
            out = np.empty(count, dtype)
            if count:
                self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(out), ptr, out.nbytes, None))
            return out

        return {"n_rows": cols.n_rows, "n_undecided": cols.n_undecided, "consumed_bytes": cols.consumed_bytes,
                "flag": get(cols.flag, np.int32, n), "mapq": get(cols.mapq, np.uint8, n),
                "mapq_valid": get(cols.mapq_valid, np.uint8, nb), "ref_id": get(cols.ref_id, np.int32, n),
                "ref_valid": get(cols.ref_valid, np.uint8, nb), "start": get(cols.start, np.int64, n),
                "end": get(cols.end, np.int64, n), "pos_valid": get(cols.pos_valid, np.uint8, nb)}

    def parse(self, d_data, n_bytes, stream=None):
        """exon_hip_bam_parser_parse over record bytes resident in HBM: the columns struct (device pointers into the parser's buffers)"""
        cols = L.BAMColumns()
        self.ctx._check(self.ctx.lib.exon_hip_bam_parser_parse(self.h, stream, d_data.ptr if isinstance(d_data, DeviceBuffer) else d_data, int(n_bytes), C.byref(cols)))
        return cols

    def cigar_blocks(self, d_data, n_bytes, cols, cover_ops, row_mask=None, stream=None):
        """exon_hip_bam_parser_cigar_blocks: the aligned blocks of the slab `parse` has just split -> (n_blocks, n_undecided, [ref, start,
        end] as L.Column: device pointers into the parser's buffers, one validity bitmap).  What a blocks-mode scan runs per slab."""
        out = (L.Column * 3)()
        n, u = C.c_int64(), C.c_int64()
        p = lambda x: None if x is None else x.ptr if isinstance(x, DeviceBuffer) else int(x)
        self.ctx._check(self.ctx.lib.exon_hip_bam_parser_cigar_blocks(self.h, stream, p(d_data), int(n_bytes), C.byref(cols), p(row_mask), cover_ops_mask(cover_ops), out,
                                                                    C.byref(n), C.byref(u)))
        return n.value, u.value, out

    def close(self):
        if self.h:
            self.ctx.lib.exon_hip_bam_parser_destroy(self.h)
            self.h = None


class BCFParser:
    """BCF record splitting + typed-value walk on the GPU (exon_hip_bcf_parser_*): inflated bytes in HBM -> the VCF device layout.
    info_keys: header-string indexes of the INFO fields to extract, info_kinds: one letter each ('f', 'i', 'b', 'F', 'I')."""

    def __init__(self, ctx, n_contigs, n_strings, n_samples=0, info_keys=(), info_kinds="", max_slab_bytes=64 << 20):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.exon_hip_bcf_parser_create(ctx.h, n_contigs, n_strings, n_samples, -1, max_slab_bytes, C.byref(h)))
        self.h = h
        if info_keys:
            ctx._check(ctx.lib.exon_hip_bcf_parser_set_info_keys(self.h, (C.c_int32 * len(info_keys))(*info_keys),
                                                                 info_kinds.encode(), len(info_keys)))
        self.cap_items = max_slab_bytes + 1  # items a list key's buffers hold (exon_hip_bcf_parser_set_info_keys)

    def parse_host(self, data):
        """Test helper: copy `data` (record bytes, starting at a record boundary) to HBM, split + extract, bring the columns back
        as numpy arrays (no rows of an undecided slab).  "filters": the FILTER index list behind every filter id; "infos": as
        VCFParser.parse_host gives them."""
        buf = np.frombuffer(data, np.uint8)
        d = self.ctx.to_device(np.concatenate([buf, np.zeros(64, np.uint8)]))
        cols = L.VCFColumns()
        self.ctx._check(self.ctx.lib.exon_hip_bcf_parser_parse(self.h, None, d.ptr, len(buf), C.byref(cols)))
        n = cols.n_rows if cols.n_undecided == 0 else 0
        nb = (n + 7) // 8

        def get(ptr, dtype, count):
            out = np.empty(count, dtype)
            if count:
                self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(out), ptr, out.nbytes, None))
            return out

        res = {"n_rows": cols.n_rows, "n_undecided": cols.n_undecided, "consumed_bytes": cols.consumed_bytes,
               "chrom_id": get(cols.chrom_id, np.int32, n), "pos": get(cols.pos, np.int64, n),
               "pos_valid": get(cols.pos_valid, np.uint8, nb), "qual": get(cols.qual, np.float32, n),
               "qual_valid": get(cols.qual_valid, np.uint8, nb), "filter_id": get(cols.filter_id, np.int32, n),
               "filters": [], "infos": []}
        if cols.n_undecided == 0:
            res["filters"] = self.filters()
        for q in range(cols.n_info):
            kind = cols.info_kinds[q:q + 1].decode()
            k = {"kind": kind, "valid": get(cols.infos_valid[q], np.uint8, nb)}
            if kind in "FI":
                k["offsets"] = get(cols.list_offsets[q], np.int32, n + 1 if n else 0)
                items = min(int(k["offsets"][-1]) if n else 0, self.cap_items)
                k["values"] = get(cols.infos[q], np.float32, items)
                k["item_valid"] = get(cols.list_item_valid[q], np.uint8, (items + 7) // 8)
            elif kind != "b":
                k["values"] = get(cols.infos[q], np.float32, n)
            res["infos"].append(k)
        return res

    def filters(self):
        """the FILTER lists seen so far, in id order: tuples of header-string indexes"""
        n = C.c_int32()
        self.ctx._check(self.ctx.lib.exon_hip_bcf_parser_filters(self.h, None, None, 0, C.byref(n)))
        lists, counts = (C.c_int32 * (8 * max(n.value, 1)))(), (C.c_int32 * max(n.value, 1))()
        self.ctx._check(self.ctx.lib.exon_hip_bcf_parser_filters(self.h, lists, counts, n.value, C.byref(n)))
        return [tuple(lists[8 * i:8 * i + counts[i]]) for i in range(n.value)]

    def close(self):
        if self.h:
            self.ctx.lib.exon_hip_bcf_parser_destroy(self.h)
            self.h = None


class FASTQParser:
    """FASTQ record splitting on the GPU (exon_hip_fastq_parser_*): text slab in HBM -> per-read views into it."""

    def __init__(self, ctx, max_slab_bytes=64 << 20):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.exon_hip_fastq_parser_create(ctx.h, max_slab_bytes, C.byref(h)))
        self.h = h

    def parse_device(self, d_text, n_bytes, final=True, stream=None):
        v = L.FASTQViews()
        ptr = d_text.ptr if isinstance(d_text, DeviceBuffer) else int(d_text)
        self.ctx._check(self.ctx.lib.exon_hip_fastq_parser_parse(self.h, stream, ptr, n_bytes, 1 if final else 0, C.byref(v)))
        return v

    def parse_host(self, text, final=True, misalign=0):
        """Test helper: copy `text` to HBM (`misalign` bytes past a 16-byte boundary), split it, bring the views back as
        numpy arrays relative to the start of the text (on the device they index views.text_base, which
        exon_hip_qual_pos_hist_views takes)."""
        buf = np.frombuffer(text, np.uint8)
        d = self.ctx.to_device(np.concatenate([np.full(misalign, 10, np.uint8), buf, np.zeros(64, np.uint8)]))
        v = self.parse_device(d.ptr + misalign, len(buf), final)
        n = v.n_reads

        def get(ptr):
            out = np.empty(n, np.int32)
            if n:
                self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(out), ptr, out.nbytes, None))
            return out

        shift = (d.ptr + misalign) - (v.text_base or (d.ptr + misalign))
        return {"n_reads": n, "n_undecided": v.n_undecided, "consumed_bytes": v.consumed_bytes, "views": v, "d_text": v.text_base,
                "keepalive": d, "seq_start": get(v.seq_start) - shift, "seq_end": get(v.seq_end) - shift,
                "qual_start": get(v.qual_start) - shift, "qual_end": get(v.qual_end) - shift,
                "head_start": get(v.head_start) - shift, "head_end": get(v.head_end) - shift}

    def close(self):
        if self.h:
            self.ctx.lib.exon_hip_fastq_parser_destroy(self.h)
            self.h = None


class FASTAParser:
    """FASTA record splitting on the GPU (exon_hip_fasta_parser_*): text slab in HBM -> per record the definition and the
    Arrow offsets of the sequence column, per line where its bytes go in that column."""

    def __init__(self, ctx, max_slab_bytes=64 << 20):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.exon_hip_fasta_parser_create(ctx.h, max_slab_bytes, C.byref(h)))
        self.h = h

    def parse_device(self, d_text, n_bytes, final=True, stream=None):
        v = L.FASTAViews()
        ptr = d_text.ptr if isinstance(d_text, DeviceBuffer) else int(d_text)
        self.ctx._check(self.ctx.lib.exon_hip_fasta_parser_parse(self.h, stream, ptr, n_bytes, 1 if final else 0, C.byref(v)))
        return v

    def parse_host(self, text, final=True, misalign=0):
        """Test helper: copy `text` to HBM (`misalign` bytes past a 16-byte boundary), split it and bring back, per record, the
        definition bytes (behind '>', CR dropped) and the sequence length, plus n_records, n_undecided and consumed; line_dst
        (where every line's bytes go in the sequence column, n_lines + 1 entries) and line_end relative to the start of the
        text come along."""
        buf = np.frombuffer(text, np.uint8)
        d = self.ctx.to_device(np.concatenate([np.full(misalign, 10, np.uint8), buf, np.zeros(64, np.uint8)]))
        v = self.parse_device(d.ptr + misalign, len(buf), final)
        n = v.n_records

        def get(ptr, count, dtype=np.int32):
            out = np.empty(count, dtype)
            if count:
                self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(out), ptr, out.nbytes, None))
            return out

        out = {"n_records": n, "n_undecided": v.n_undecided, "consumed": v.consumed_bytes, "n_lines": v.n_lines,
               "seq_bytes": v.seq_bytes, "views": v, "keepalive": d, "definitions": [], "seq_len": []}
        if n:
            shift = v.first_line_start
            hs, he = get(v.head_start, n) - shift, get(v.head_end, n) - shift
            off = get(v.seq_offsets, n + 1)
            out["definitions"] = [bytes(buf[a:b]) for a, b in zip(hs.tolist(), he.tolist())]
            out["seq_len"] = np.diff(off).tolist()
            out["seq_offsets"] = off
        if v.n_lines:
            out["line_dst"] = get(v.line_dst, v.n_lines + 1, np.uint32)
            out["line_end"] = get(v.line_end, v.n_lines, np.uint32) - np.uint32(v.first_line_start)
        return out

    def close(self):
        if self.h:
            self.ctx.lib.exon_hip_fasta_parser_destroy(self.h)
            self.h = None


class Plan:
    def __init__(self, ctx, desc, columns):
        self.ctx = ctx
        for i, c in enumerate(columns):
            desc.columns[i] = c
        self.desc = desc
        self.n_cols = len(columns)
        h = C.c_void_p()
        ctx._check(ctx.lib.exon_hip_plan_create(ctx.h, C.byref(desc), C.byref(h)))
        self.h = h
        a, b = C.c_int64(), C.c_int64()
        ctx._check(ctx.lib.exon_hip_plan_state_size(h, C.byref(a), C.byref(b)))
        self.n_i64, self.n_f64 = a.value, b.value

    def open(self, partition=0):
        return Stream(self, partition)

    def launch(self, columns, n, d_state, overwrite=False, stream=None):
        """exon_hip_plan_launch: the plan's fused kernel over HBM-resident columns (operator argument order; each a
        (values, validity, offsets) triple of DeviceBuffers / raw device pointers) into the packed state `d_state`
        ([n_i64 int64][n_f64 float64], DeviceBuffer or raw pointer).  overwrite: state := this batch (no zeroing)."""
        cols = (Column * len(columns))(*[_col(v, b, o, n) for (v, b, o) in columns])
        ptr = d_state.ptr if isinstance(d_state, DeviceBuffer) else int(d_state)
        self.ctx._check(self.ctx.lib.exon_hip_plan_launch(self.h, stream, cols, len(columns), n,
                                                          L.LAUNCH_OVERWRITE if overwrite else L.LAUNCH_ACCUMULATE, ptr))

    def prepared(self, columns, n, d_state, overwrite=False, stream=None):
        """launch() with the argument marshalling done once: returns a zero-argument callable that enqueues the same
        launch again (a resident table queried repeatedly; a 10 M-row step is ~20 us of GPU time, so per-call ctypes
        struct building would be what gets measured)."""
        cols = (Column * len(columns))(*[_col(v, b, o, n) for (v, b, o) in columns])
        ptr = C.c_void_p(d_state.ptr if isinstance(d_state, DeviceBuffer) else int(d_state))
        fn, check, h = self.ctx.lib.exon_hip_plan_launch, self.ctx._check, self.h
        ncol, nn = C.c_int32(len(columns)), C.c_int64(n)
        flags = C.c_int32(L.LAUNCH_OVERWRITE if overwrite else L.LAUNCH_ACCUMULATE)
        st = C.c_void_p(stream)

        def go():
            rc = fn(h, st, cols, ncol, nn, flags, ptr)
            if rc:
                check(rc)
        go.keepalive = cols
        return go

    def launch_chunks(self, chunks, d_state, overwrite=False, stream=None):
        """exon_hip_plan_launch_chunks: `chunks` = [(columns, n)], columns as in launch().  A quality-histogram plan
        runs up to 64 chunks per kernel launch; the other kinds launch per chunk."""
        ncol = len(chunks[0][0]) if chunks else self.n_cols
        flat = [_col(v, b, o, n) for (cols, n) in chunks for (v, b, o) in cols]
        arr = (Column * max(1, len(flat)))(*flat)
        ns = (C.c_int64 * max(1, len(chunks)))(*[n for _, n in chunks])
        ptr = d_state.ptr if isinstance(d_state, DeviceBuffer) else int(d_state)
        self.ctx._check(self.ctx.lib.exon_hip_plan_launch_chunks(self.h, stream, arr, ncol, len(chunks), ns,
                                                                 L.LAUNCH_OVERWRITE if overwrite else L.LAUNCH_ACCUMULATE, ptr))

    def fold_states(self, d_gathered, world, d_out, stream=None):
        """exon_hip_plan_fold_states: `world` packed states of this plan (rank-major device memory) folded in rank order by
        the plan's own layout -- add for counts and sums, unsigned max for the extreme planes of a MIN / MAX plan."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else int(x)  # noqa: E731
        self.ctx._check(self.ctx.lib.exon_hip_plan_fold_states(self.h, stream, ptr(d_gathered), world, ptr(d_out)))

    def close(self):
        if self.h:
            self.ctx.lib.exon_hip_plan_destroy(self.h)
            self.h = None


class RegionSetPlan(Plan):
    """Plan kind 11 (exon_hip_plan_create_region_set).  ctx None: a host-only plan that serves layout() and decode() and cannot be
    launched."""

    _CREATE, _LAYOUT, _LAYOUT_WORDS, _DECODE = "exon_hip_plan_create_region_set", "exon_hip_region_set_layout", 4, "exon_hip_region_set_decode"

    def __init__(self, ctx, regions, columns=(2, 3, 4)):
        self.ctx = ctx
        self.lib = ctx.lib if ctx is not None else L.load()
        regions = [(c, int(s), L.REGION_OPEN_END if e is None else int(e)) for (c, s, e) in regions]
        by_name = [isinstance(c, (str, bytes)) for c, _, _ in regions]
        if any(by_name) and not all(by_name):
            raise ValueError("a region set names its contigs either all by name or all by reference id")
        self.by_name = bool(regions) and by_name[0]
        self.regions = regions
        self.n_cols = 3
        m = len(regions)
        starts = np.array([r[1] for r in regions], np.int64)
        ends = np.array([r[2] for r in regions], np.int64)
        cols = (C.c_int32 * 3)(*columns)
        packed, ids = None, None
        if self.by_name:
            packed = b"".join((c if isinstance(c, bytes) else c.encode()) + b"\0" for c, _, _ in regions)
        else:
            ids = np.array([r[0] for r in regions], np.int32)
        h = C.c_void_p()
        self._check(getattr(self.lib, self._CREATE)(ctx.h if ctx is not None else None, cols, packed, len(packed) if packed else 0,
                                                    ids.ctypes.data if ids is not None and m else None,
                                                    starts.ctypes.data if m else None, ends.ctypes.data if m else None, m, *self._create_extra(), C.byref(h)))
        self.h = h
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.exon_hip_plan_state_size(h, C.byref(a), C.byref(b)))
        self.n_i64, self.n_f64 = a.value, b.value

    def _create_extra(self):
        """What the kind's constructor takes between n_regions and the plan."""
        return ()

    def _check(self, rc):
        if rc < 0:
            raise ExonHipError(rc, self.lib.exon_hip_last_error(None).decode(errors="replace"))
        return rc

    def layout(self):
        out = (C.c_int64 * self._LAYOUT_WORDS)()
        self._check(getattr(self.lib, self._LAYOUT)(self.h, out))
        return tuple(out)

    def decode(self, state):
        state = np.ascontiguousarray(state, np.int64)
        if state.size != self.n_i64:
            raise ValueError("the state of this plan has %d words, %d given" % (self.n_i64, state.size))
        out = np.zeros(len(self.regions), np.int64)
        self._check(getattr(self.lib, self._DECODE)(self.h, state.ctypes.data, out.ctypes.data))
        return out

    def close(self):
        if self.h:
            self.lib.exon_hip_plan_destroy(self.h)
            self.h = None


class RegionBasesPlan(RegionSetPlan):
    """Plan kind 12 (exon_hip_plan_create_region_set_bases): RegionSetPlan's arguments; layout() gives the word offsets of the
    totals / Ns / Ss / Ne / Se sections and the word count, decode() the covered bases of every region."""

    _CREATE, _LAYOUT, _LAYOUT_WORDS, _DECODE = "exon_hip_plan_create_region_set_bases", "exon_hip_region_bases_layout", 6, "exon_hip_region_bases_decode"


class WindowBasesPlan(RegionSetPlan):
    """Plan kind 13 (exon_hip_plan_create_window_bases).  ctx None: a host-only plan that serves layout(), offsets() and decode() and
    cannot be launched.  layout() gives the word offsets of the totals / E / D sections and the word count, offsets() the windows in
    front of each contig and their total B, decode() the bases of every window, contig by contig."""

    _LAYOUT, _LAYOUT_WORDS, _DECODE = "exon_hip_window_bases_layout", 4, "exon_hip_window_bases_decode"

    def __init__(self, ctx, contigs, window, columns=(2, 3, 4)):
        self.ctx = ctx
        self.lib = ctx.lib if ctx is not None else L.load()
        contigs = [(c, int(n)) for (c, n) in contigs]
        by_name = [isinstance(c, (str, bytes)) for c, _ in contigs]
        if any(by_name) and not all(by_name):
            raise ValueError("a window plan names its contigs either all by name or all by reference id")
        self.by_name = bool(contigs) and by_name[0]
        self.contigs, self.window = contigs, int(window)
        self.n_cols = 3
        m = len(contigs)
        lengths = np.array([n for _, n in contigs], np.int64)
        packed, ids = None, None
        if self.by_name:
            packed = b"".join((c if isinstance(c, bytes) else c.encode()) + b"\0" for c, _ in contigs)
        else:
            ids = np.array([c for c, _ in contigs], np.int32)
        h = C.c_void_p()
        self._check(self.lib.exon_hip_plan_create_window_bases(ctx.h if ctx is not None else None, (C.c_int32 * 3)(*columns), packed, len(packed) if packed else 0,
                                                               ids.ctypes.data if ids is not None and m else None, lengths.ctypes.data if m else None, m,
                                                               self.window, C.byref(h)))
        self.h = h
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.exon_hip_plan_state_size(h, C.byref(a), C.byref(b)))
        self.n_i64, self.n_f64 = a.value, b.value

    def offsets(self):
        out = np.zeros(len(self.contigs) + 1, np.int64)
        self._check(self.lib.exon_hip_window_bases_offsets(self.h, out.ctypes.data))
        return out

    def decode(self, state):
        state = np.ascontiguousarray(state, np.int64)
        if state.size != self.n_i64:
            raise ValueError("the state of this plan has %d words, %d given" % (self.n_i64, state.size))
        out = np.zeros((self.n_i64 - 4) // 2, np.int64)
        self._check(self.lib.exon_hip_window_bases_decode(self.h, state.ctypes.data, out.ctypes.data))
        return out


class RegionDepthPlan(RegionSetPlan):
    """Plan kind 14 (exon_hip_plan_create_region_set_depth): RegionSetPlan's regions (finite ends) and up to 8 strictly increasing
    depth thresholds.  ctx None: a host-only plan that serves layout(), intervals(), per_base() and decode() and cannot be launched.
    layout(): the word offsets of the totals and of D and the word count; intervals(): the merged intervals in bin order as (slot,
    start, end, bin) arrays; per_base(state): the depth of every target base in bin order; decode(state): (bases[M], ge[M, k]) per
    region in the caller's order; reduce(d_state): the same table, [M, 1 + k] int64 words, made on the device."""

    _CREATE, _LAYOUT, _LAYOUT_WORDS = "exon_hip_plan_create_region_set_depth", "exon_hip_region_depth_layout", 3

    def __init__(self, ctx, regions, thresholds, columns=(2, 3, 4)):
        self.thresholds = [int(t) for t in thresholds]
        self._thr = np.array(self.thresholds, np.int64)
        super().__init__(ctx, regions, columns)

    def _create_extra(self):
        return (self._thr.ctypes.data if self._thr.size else None, int(self._thr.size))

    def _state(self, state):
        state = np.ascontiguousarray(state, np.int64)
        if state.size != self.n_i64:
            raise ValueError("the state of this plan has %d words, %d given" % (self.n_i64, state.size))
        return state

    def intervals(self):
        n = C.c_int32()
        self._check(self.lib.exon_hip_region_depth_intervals(self.h, C.byref(n), None, None, None, None))
        slot = np.zeros(n.value, np.int32)
        start, end, bins = (np.zeros(n.value, np.int64) for _ in range(3))
        self._check(self.lib.exon_hip_region_depth_intervals(self.h, C.byref(n), slot.ctypes.data, start.ctypes.data, end.ctypes.data, bins.ctypes.data))
        return slot, start, end, bins

    def per_base(self, state):
        state = self._state(state)
        n_contigs = len(set(c for c, _, _ in self.regions))
        out = np.zeros(self.n_i64 - 4 - n_contigs, np.int64)
        self._check(self.lib.exon_hip_region_depth_per_base(self.h, state.ctypes.data, out.ctypes.data))
        return out

    def decode(self, state):
        state = self._state(state)
        k = len(self.thresholds)
        out = np.zeros((len(self.regions), 1 + k), np.int64)
        self._check(self.lib.exon_hip_region_depth_decode(self.h, state.ctypes.data, out.ctypes.data))
        return out[:, 0].copy(), out[:, 1:].copy()

    def reduce(self, d_state, stream=None):
        """exon_hip_region_depth_reduce: a DeviceBuffer of [M, 1 + k] int64 words (bases, ge_t ...); `d_state` is only read."""
        out = self.ctx.empty(np.int64, len(self.regions) * (1 + len(self.thresholds)))
        self._check(self.lib.exon_hip_region_depth_reduce(self.ctx.h, stream, self.h, d_state.ptr if isinstance(d_state, DeviceBuffer) else d_state, out.ptr))
        return out


class Stream:
    """One partition's execution (ExecutionPlan::execute analogue)."""

    def __init__(self, plan, partition):
        self.plan, self.ctx = plan, plan.ctx
        h = C.c_void_p()
        self.ctx._check(self.ctx.lib.exon_hip_stream_open(plan.h, partition, C.byref(h)))
        self.h = h

    def push(self, batch):
        """Push a pyarrow.RecordBatch (host memory) through the Arrow C Data Interface (moved)."""
        arr = L.ArrowArray()
        sch = L.ArrowSchema()
        batch._export_to_c(C.addressof(arr), C.addressof(sch))
        try:
            self.ctx._check(self.ctx.lib.exon_hip_stream_push(self.h, C.byref(arr)))
        finally:
            if arr.release:  # (the library moves the batch whatever it returns; only a call it could not even look at leaves it here)
                C.CFUNCTYPE(None, C.POINTER(L.ArrowArray))(arr.release)(C.byref(arr))
            if sch.release:
                C.CFUNCTYPE(None, C.POINTER(L.ArrowSchema))(sch.release)(C.byref(sch))

    def push_device(self, columns, n_rows):
        """columns: list of (values DeviceBuffer, validity DeviceBuffer|None, offsets DeviceBuffer|None) already
        in HBM, in batch-child order; wrapped as an ArrowDeviceArray (ARROW_DEVICE_ROCM)."""
        keep = []
        kids = (C.POINTER(L.ArrowArray) * len(columns))()
        for i, (values, validity, offsets) in enumerate(columns):
            a = L.ArrowArray()
            if offsets is not None:
                bufs = (C.c_void_p * 3)(validity.ptr if validity else None, offsets.ptr, values.ptr)
                a.n_buffers = 3
            else:
                bufs = (C.c_void_p * 2)(validity.ptr if validity else None, values.ptr)
                a.n_buffers = 2
            a.length = n_rows
            a.null_count = -1 if validity else 0
            a.buffers = C.cast(bufs, C.POINTER(C.c_void_p))
            keep += [a, bufs]
            kids[i] = C.pointer(a)
        top = L.ArrowDeviceArray()
        tb = (C.c_void_p * 1)(None)
        top.array.length = n_rows
        top.array.n_buffers = 1
        top.array.buffers = C.cast(tb, C.POINTER(C.c_void_p))
        top.array.n_children = len(columns)
        top.array.children = C.cast(kids, C.POINTER(C.POINTER(L.ArrowArray)))
        top.device_id = self.ctx.device
        top.device_type = L.ARROW_DEVICE_ROCM
        # no sync_event travels with the batch, which by the Arrow C Device interface means "the data is ready": whatever this
        # harness queued on the context's stream to produce the columns (gen_c4 ...) has to be finished first (the plan runs on
        # its own stream; found by a test that only failed beside three other workers on the same GPU)
        self.ctx.sync()
        self.ctx._check(self.ctx.lib.exon_hip_stream_push_device(self.h, C.byref(top)))
        self._keep = keep + [kids, tb, top]

    def consume(self, scan):
        """Pull every batch of a Scan through this stream (GpuFilterAggExec::execute in native code)."""
        n = C.c_int64()
        rc = self.ctx.lib.exon_hip_stream_consume_scan(self.h, scan.h, C.byref(n))
        if rc < 0:
            raise ExonHipError(rc, self.ctx._last_error())
        return n.value

    def state(self):
        a, b, s = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ctx._check(self.ctx.lib.exon_hip_stream_state(self.h, C.byref(a), C.byref(b), C.byref(s)))
        return a.value, b.value, s.value

    def all_reduce(self, rccl_comm):
        """Merge of the partial state over the ranks of `rccl_comm` (an ncclComm_t as an integer) on the stream: one
        ncclAllGather + fixed-order fold; afterwards every rank's state is the sum over all ranks."""
        self.ctx._check(self.ctx.lib.exon_hip_stream_all_reduce(self.h, C.c_void_p(rccl_comm)))

    # ---- group keys by value (ABI 4): what the state's indexes stand for when the rows came from files
    def keys(self):
        """(names in state-index order, agreed) -- the dictionary exon_hip_stream_consume_scan built up; `agreed` is True once
        set_keys / reconcile_keys ran and no scan was consumed since."""
        n, b, a = C.c_int32(), C.c_size_t(), C.c_int32()
        self.ctx._check(self.ctx.lib.exon_hip_stream_keys(self.h, None, 0, C.byref(n), C.byref(b), C.byref(a)))
        buf = C.create_string_buffer(max(b.value, 1))
        self.ctx._check(self.ctx.lib.exon_hip_stream_keys(self.h, buf, b.value, C.byref(n), C.byref(b), C.byref(a)))
        return unpack_names(buf.raw[:b.value], n.value), bool(a.value)

    def set_keys(self, names):
        """Adopt `names` as the dictionary (every key held must be among them): the device state is permuted into that order."""
        packed = pack_names(names)
        self.ctx._check(self.ctx.lib.exon_hip_stream_set_keys(self.h, packed, len(packed), len(names)))

    def reconcile_keys(self, rccl_comm):
        """Collective: the ranks of `rccl_comm` (an ncclComm_t as an integer) agree on the union dictionary, natively."""
        self.ctx._check(self.ctx.lib.exon_hip_stream_reconcile_keys(self.h, C.c_void_p(rccl_comm)))

    def set_region_contig(self, name):
        """Region plans over files: the contig by name; every consumed file resolves it in its own header order."""
        self.ctx._check(self.ctx.lib.exon_hip_stream_set_region_contig(self.h, name.encode()))

    def snapshot(self):
        """(counts, sums) of the state as it stands, without finishing the stream."""
        a, b, s = self.state()
        self.ctx._check(self.ctx.lib.exon_hip_sync(self.ctx.h, C.c_void_p(s)))
        counts = np.zeros(self.plan.n_i64, np.int64)
        sums = np.zeros(self.plan.n_f64, np.float64)
        if counts.size:
            self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(counts), C.c_void_p(a), counts.nbytes, None))
        if sums.size:
            self.ctx._check(self.ctx.lib.exon_hip_memcpy_d2h(self.ctx.h, _np_ptr(sums), C.c_void_p(b), sums.nbytes, None))
        self.ctx.sync()
        return counts, sums

    def reset(self):
        """New query on this stream: the next launch defines the state (overwrite mode, no zeroing kernel)."""
        self.ctx._check(self.ctx.lib.exon_hip_stream_reset(self.h))

    def sync(self):
        self.ctx._check(self.ctx.lib.exon_hip_stream_sync(self.h))

    def finish(self):
        counts = np.zeros(self.plan.n_i64, np.int64)
        sums = np.zeros(self.plan.n_f64, np.float64)
        self.ctx._check(self.ctx.lib.exon_hip_stream_finish(self.h, _np_ptr(counts), _np_ptr(sums)))
        return counts, sums

    def finish_arrow(self):
        import pyarrow as pa
        arr, sch = L.ArrowArray(), L.ArrowSchema()
        self.ctx._check(self.ctx.lib.exon_hip_stream_finish_arrow(self.h, C.byref(arr), C.byref(sch)))
        return pa.Array._import_from_c(C.addressof(arr), C.addressof(sch))

    def close(self):
        if self.h:
            self.ctx.lib.exon_hip_stream_close(self.h)
            self.h = None
