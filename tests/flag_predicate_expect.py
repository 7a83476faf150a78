"""What a BAM / SAM scan with a pushed-down flag / mapping-quality predicate (exon_hip_scan_set_flag_predicate) must emit, from the
records' python dicts alone (tests/bam_sam_writer.py writes the files from the same dicts): no product code is touched here.
  passes   (flag & mask) == value AND (mapq_min < 0 OR (mapq != 255 AND mapq >= mapq_min)) -- 255 is the NULL mapping_quality
  hits     bam_region_filter's interval test: reference = name AND start <= b AND a <= end, NULL reference / start never
  keep     the indices of the records that pass both
  columns  every column of the kept records: the five fixed-width ones and name / cigar / sequence / quality_score"""
import bam_sam_writer as bsw

PROJECT = ("name", "cigar", "sequence", "quality_score")
FIXED = ("flag", "mapping_quality", "reference", "start", "end")


def read(i, flag=0, mapq=60, l_seq=None, ref=0, pos=None, high=False):
    """record i.  high: quality bytes above 127 (BAM only: negative Int64 items)"""
    n = 5 + i % 7 if l_seq is None else l_seq
    seq = "".join("ACGTN"[(i + k) % 5] for k in range(n))
    qual = [128 + (i * 7 + k * 3) % 128 if high else 10 + (i * 7 + k * 3) % 84 for k in range(n)]  # (SAM: Phred 10..93, never the lone '*')
    return dict(name="*" if i % 11 == 5 else f"read{i}", flag=flag, ref=ref, pos=100 + 10 * i if pos is None else pos, mapq=mapq,
                cigar=[(n, 0)] if n else [], seq=seq, qual=qual)


def passes(flag, mapq, mask, value, mapq_min=-1):
    return (flag & mask) == value and (mapq_min < 0 or (mapq != 255 and mapq >= mapq_min))


def hits(r, region, refs=bsw.REFS):
    name, a, b = region
    if r["ref"] is None or r["pos"] < 1 or refs[r["ref"]][0] != name:
        return False
    end = r["pos"] + sum(n for n, op in r["cigar"] if op in bsw.REF_CONSUMING) - 1
    return r["pos"] <= b and a <= end


def keep(recs, mask, value, mapq_min=-1, region=None):
    return [i for i, r in enumerate(recs) if passes(r["flag"], r["mapq"], mask, value, mapq_min) and (region is None or hits(r, region))]


def columns(recs, sam, kept, project=PROJECT):
    e = bsw.expected(recs, sam)
    e["mapping_quality"] = [None if r["mapq"] == 255 else r["mapq"] for r in recs]
    return {k: [e[k][i] for i in kept] for k in FIXED + tuple(project)}


def table(scan):
    """every batch of a Scan -> (columns as lists, the batches' lengths)"""
    cols, lens = {}, []
    for b in scan:
        lens.append(len(b))
        for i in range(b.type.num_fields):
            cols.setdefault(b.type.field(i).name, []).extend(b.field(i).to_pylist())
    return cols, lens


def take(cols, kept):
    """the rows `kept` of a table() result"""
    return {k: [v[i] for i in kept] for k, v in cols.items()}
