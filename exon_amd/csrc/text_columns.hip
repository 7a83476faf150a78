// text_columns.hip -- the reference's STRING / LIST columns out of the GPU decode pipeline: Arrow Utf8 / List<Utf8> / List<Int64>
// buffers (offsets + compact values) built on the device from the slab the parsers have just indexed.
//
// Reference columns rebuilt here (the ones outside the fused kernels' operands, selected by exon_hip_scan_options.projection):
//   VCF  id         List<Utf8>, NULL when the ID field is '.'       exon-vcf/src/array_builder/lazy_array_builder.rs:169-180
//        ref        Utf8                                             :181-190
//        alt        List<Utf8>: NULL when ALT is '.', otherwise a list with NO items -- the reference concatenates the alternate
//                   bases into a local string and then calls `alternates.append(true)` without ever appending a value (:191-205);
//                   reproduced as it is (results identical to the reference's), the quirk is written down in DESIGN.md
//        info       Utf8: the parsed entries printed again, not the field's bytes ("AF=0.50" -> "AF=0.5")      :216-297
//        formats    Utf8: FORMAT, a TAB, the samples printed again (by opt-in: EXON_HIP_PROJECT_VCF_FORMATS_ON_DEVICE)  :310-423
//   BAM  name       Utf8, NULL for '*'                                exon-bam/src/array_builder.rs:105-113
//        cigar      Utf8, "<len><op>..." with ops MIDNSHP=X           :144-167
//        sequence   Utf8, 4-bit codes through "=ACMGRSVTWYHKDBN"      :178-183
//        quality_scores  List<Int64>, the raw bytes as i8 -> i64      :184-201
//   GFF  attributes Map<Utf8, List<Utf8>>, never NULL                 exon-gff/src/array_builder.rs:141-165 (host/gff.h: THE ATTRIBUTE RULES)
//   GTF  attributes Map<Utf8, Utf8>, never NULL                       exon-gtf/src/array_builder.rs:82-87 (host/gtf.h: THE ATTRIBUTE RULES)
// One thread per row measures, an exclusive scan turns lengths into offsets, one thread per row fills (rows are short; the bytes
// of a slab are read twice, L2-resident the second time).  VCF `formats` alone is cut by SAMPLE, not by row (a row may hold
// thousands): see its block.  Nothing here is on the fused kernels' path: a scan that projects none of
// these columns launches none of this.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <new>

#include "host/decimal_f32.h"
#include "host/f32_print.h"
#include "host/vcf_sample_walk.h"
#include "host/vcf_text.h"
#include "internal.h"
#include "list_kernels.h"

namespace {

constexpr int TPB = 256;

// ---- exclusive scan of n u32 lengths into n + 1 int32 offsets: list_kernels.h's block sums and scan (n is known on the host), then
// the in-block prefix
__global__ __launch_bounds__(LIST_TPB) void k_write_offsets(const uint32_t* __restrict__ len, unsigned n, const unsigned* __restrict__ sums, int32_t* __restrict__ offsets) {
  const unsigned i = blockIdx.x * LIST_TPB + threadIdx.x;
  const unsigned c = i < n ? len[i] : 0u;
  const unsigned first = list_first_item(c, sums);
  if (i < n) offsets[i] = (int32_t)first;
  if (i == n - 1) offsets[n] = (int32_t)(first + c);
}

// ---- VCF ---------------------------------------------------------------------------------------------------------------------------
// line r of the slab: [begin, end) in the aligned text; fields 2, 3, 4 (ID, REF, ALT) by their tabs
struct VcfLens {
  uint32_t* id_items;   // items of the ID list (0 for '.')
  uint32_t* id_bytes;   // bytes of its items (the ';' between them do not count)
  uint32_t* ref_bytes;
  uint32_t* field_off;  // [3 n]: where ID, REF, ALT start
  uint32_t* field_len;  // [3 n]
};
__global__ __launch_bounds__(TPB) void k_vcf_measure(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned n_rows, unsigned skip, VcfLens o,
                                                     uint32_t* __restrict__ id_valid, uint32_t* __restrict__ alt_valid) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  bool idv = false, altv = false;
  if (row < n_rows) {
    const unsigned begin = row ? nl[row - 1] + 1 : skip;
    unsigned end = nl[row];
    if (end > begin && text[end - 1] == '\r') --end;
    unsigned fs[6];
    int nf = 0;
    fs[0] = begin;
    for (unsigned i = begin; i < end && nf < 5; ++i)
      if (text[i] == '\t') fs[++nf] = i + 1;
    // (rows with fewer than 5 fields are not data lines: the parser has counted them undecided, the slab goes to the host reader)
    unsigned off[3] = {0, 0, 0}, len[3] = {0, 0, 0};
    for (int f = 0; f < 3; ++f)
      if (nf >= f + 3) {
        off[f] = fs[f + 2];
        len[f] = fs[f + 3] - 1 - fs[f + 2];
      } else if (nf == f + 2) {
        off[f] = fs[f + 2];
        len[f] = end - fs[f + 2];
      }
    unsigned items = 0, bytes = 0;
    if (!(len[0] == 0 || (len[0] == 1 && text[off[0]] == '.'))) {
      items = 1;
      bytes = len[0];
      for (unsigned i = 0; i < len[0]; ++i)
        if (text[off[0] + i] == ';') {
          ++items;
          --bytes;
        }
      idv = true;
    }
    altv = !(len[2] == 0 || (len[2] == 1 && text[off[2]] == '.'));
    o.id_items[row] = items;
    o.id_bytes[row] = bytes;
    o.ref_bytes[row] = len[1];
    for (int f = 0; f < 3; ++f) {
      o.field_off[3 * row + f] = off[f];
      o.field_len[3 * row + f] = len[f];
    }
  }
  // validity bitmaps: one word per 32 rows (a wave covers two)
  const unsigned long long bi = __ballot(idv), ba = __ballot(altv);
  const unsigned lane = threadIdx.x & 63u, wrow = row - lane;
  if (lane < 2 && wrow + 32 * lane < n_rows) {
    id_valid[(wrow >> 5) + lane] = (uint32_t)(bi >> (32 * lane));
    alt_valid[(wrow >> 5) + lane] = (uint32_t)(ba >> (32 * lane));
  }
}
__global__ __launch_bounds__(TPB) void k_vcf_fill(const uint8_t* __restrict__ text, unsigned n_rows, VcfLens o, const int32_t* __restrict__ id_list_off,
                                                  const int32_t* __restrict__ id_byte_off, const int32_t* __restrict__ ref_off, int32_t* __restrict__ id_item_off,
                                                  uint8_t* __restrict__ id_values, uint8_t* __restrict__ ref_values, unsigned id_items_total, unsigned id_bytes_total) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n_rows) return;
  {  // REF
    const unsigned off = o.field_off[3 * row + 1], len = o.field_len[3 * row + 1];
    uint8_t* dst = ref_values + ref_off[row];
    for (unsigned i = 0; i < len; ++i) dst[i] = text[off + i];
  }
  const unsigned items = o.id_items[row];
  if (items) {  // ID: the items back to back, an offset per item
    const unsigned off = o.field_off[3 * row + 0], len = o.field_len[3 * row + 0];
    unsigned k = (unsigned)id_list_off[row], w = (unsigned)id_byte_off[row];
    id_item_off[k++] = (int32_t)w;
    for (unsigned i = 0; i < len; ++i) {
      const uint8_t c = text[off + i];
      if (c == ';') id_item_off[k++] = (int32_t)w;
      else id_values[w++] = c;
    }
  }
  if (row == n_rows - 1) id_item_off[id_items_total] = (int32_t)id_bytes_total;
}
enum { VCF_ID_ITEMS };  // ExonTextScratch::item_off

// ---- BAM ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ld32u(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
__device__ __forceinline__ unsigned dec_digits(uint32_t v) {
  unsigned d = 1;
  while (v >= 10) {
    v /= 10;
    ++d;
  }
  return d;
}
struct BamLens {
  uint32_t* name_bytes;
  uint32_t* cigar_bytes;
  uint32_t* seq_bytes;  // = items of quality_scores
};
__global__ __launch_bounds__(TPB) void k_bam_measure(const uint8_t* __restrict__ d, const uint32_t* __restrict__ rec_of_row, unsigned n_rows, BamLens o,
                                                     uint32_t* __restrict__ name_valid) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  bool nv = false;
  if (row < n_rows) {
    const uint8_t* r = d + rec_of_row[row];
    const uint32_t l_name = r[12], n_cigar = (uint32_t)r[16] | (uint32_t)r[17] << 8, l_seq = ld32u(r + 20);
    // noodles: a read name of "*" is a missing name (Record::name -> None)
    nv = !(l_name == 2 && r[36] == '*');
    o.name_bytes[row] = nv ? l_name - 1 : 0u;
    unsigned cb = 0;
    const uint8_t* c = r + 36 + l_name;
    for (uint32_t k = 0; k < n_cigar; ++k) cb += dec_digits(ld32u(c + 4 * k) >> 4) + 1;
    o.cigar_bytes[row] = cb;
    o.seq_bytes[row] = l_seq;
  }
  const unsigned long long b = __ballot(nv);
  const unsigned lane = threadIdx.x & 63u, wrow = row - lane;
  if (lane < 2 && wrow + 32 * lane < n_rows) name_valid[(wrow >> 5) + lane] = (uint32_t)(b >> (32 * lane));
}
__global__ __launch_bounds__(TPB) void k_bam_fill(const uint8_t* __restrict__ d, const uint32_t* __restrict__ rec_of_row, unsigned n_rows, uint64_t projection,
                                                  const int32_t* __restrict__ name_off, const int32_t* __restrict__ cigar_off, const int32_t* __restrict__ seq_off,
                                                  uint8_t* __restrict__ name_values, uint8_t* __restrict__ cigar_values, uint8_t* __restrict__ seq_values,
                                                  int64_t* __restrict__ qual_values) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n_rows) return;
  const uint8_t* r = d + rec_of_row[row];
  const uint32_t l_name = r[12], n_cigar = (uint32_t)r[16] | (uint32_t)r[17] << 8, l_seq = ld32u(r + 20);
  if (projection & EXON_HIP_PROJECT_BAM_NAME) {
    const unsigned n = (unsigned)(name_off[row + 1] - name_off[row]);
    uint8_t* dst = name_values + name_off[row];
    for (unsigned i = 0; i < n; ++i) dst[i] = r[36 + i];
  }
  const uint8_t* c = r + 36 + l_name;
  if (projection & EXON_HIP_PROJECT_BAM_CIGAR) {
    uint8_t* dst = cigar_values + cigar_off[row];
    for (uint32_t k = 0; k < n_cigar; ++k) {
      const uint32_t op = ld32u(c + 4 * k);
      uint32_t v = op >> 4;
      const unsigned nd = dec_digits(v);
      for (unsigned i = nd; i > 0; --i) {
        dst[i - 1] = (uint8_t)('0' + v % 10);
        v /= 10;
      }
      dst += nd;
      const uint32_t code = op & 0xF;
      *dst++ = code < 9 ? (uint8_t)"MIDNSHP=X"[code] : (uint8_t)'?';
    }
  }
  const uint8_t* s = c + 4 * n_cigar;
  if (projection & EXON_HIP_PROJECT_BAM_SEQUENCE) {
    uint8_t* dst = seq_values + seq_off[row];
    for (uint32_t i = 0; i < l_seq; ++i) dst[i] = (uint8_t)"=ACMGRSVTWYHKDBN"[(s[i >> 1] >> ((i & 1) ? 0 : 4)) & 0xF];
  }
  if (projection & EXON_HIP_PROJECT_BAM_QUALITY_SCORES) {
    const uint8_t* q = s + (l_seq + 1) / 2;
    int64_t* dst = qual_values + seq_off[row];
    for (uint32_t i = 0; i < l_seq; ++i) dst[i] = (int64_t)(int8_t)q[i];
  }
}

}  // namespace

// ---- host side -----------------------------------------------------------------------------------------------------------------------
// ---- FASTQ -------------------------------------------------------------------------------------------------------------------------
// name, description, sequence, quality_scores (exon-fastq/src/array_builder.rs:68-102; schema exon-fastq/src/config.rs:79-88): the
// header line behind '@' up to the first space is the name, what follows the space the description (NULL when there is no space
// or nothing behind it); sequence and quality lines as they are (CR dropped by the views).
struct FastqLens {
  uint32_t *name, *desc, *seq, *qual;
};
__global__ __launch_bounds__(TPB) void k_fastq_measure(const uint8_t* __restrict__ text, unsigned n_reads, const int32_t* __restrict__ head_s,
                                                       const int32_t* __restrict__ head_e, const int32_t* __restrict__ seq_s, const int32_t* __restrict__ seq_e,
                                                       const int32_t* __restrict__ qual_s, const int32_t* __restrict__ qual_e, FastqLens o,
                                                       uint32_t* __restrict__ desc_valid) {
  const unsigned r = blockIdx.x * TPB + threadIdx.x;
  bool has_desc = false;
  if (r < n_reads) {
    const unsigned b = (unsigned)head_s[r], e = (unsigned)head_e[r];
    unsigned sp = b;
    while (sp < e && text[sp] != ' ') ++sp;
    o.name[r] = sp - b;
    has_desc = sp + 1 < e;
    o.desc[r] = has_desc ? e - sp - 1 : 0u;
    o.seq[r] = (unsigned)(seq_e[r] - seq_s[r]);
    o.qual[r] = (unsigned)(qual_e[r] - qual_s[r]);
  }
  const unsigned long long m = __ballot(has_desc);
  if ((threadIdx.x & 63) == 0 && r < n_reads + 63) {
    desc_valid[r >> 5] = (uint32_t)m;
    desc_valid[(r >> 5) + 1] = (uint32_t)(m >> 32);
  }
}
// (copy_run, the 8-byte span copier of every fill kernel here: list_kernels.h, shared with take_rows.hip)
__global__ __launch_bounds__(TPB) void k_fastq_fill(const uint8_t* __restrict__ text, unsigned n_reads, const int32_t* __restrict__ head_s,
                                                    const int32_t* __restrict__ seq_s, const int32_t* __restrict__ qual_s, const int32_t* __restrict__ name_off,
                                                    const int32_t* __restrict__ desc_off, const int32_t* __restrict__ seq_off, const int32_t* __restrict__ qual_off,
                                                    uint8_t* __restrict__ name_v, uint8_t* __restrict__ desc_v, uint8_t* __restrict__ seq_v,
                                                    uint8_t* __restrict__ qual_v) {
  const unsigned r = blockIdx.x * TPB + threadIdx.x;
  if (r >= n_reads) return;
  const unsigned nn = (unsigned)(name_off[r + 1] - name_off[r]), nd = (unsigned)(desc_off[r + 1] - desc_off[r]);
  copy_run(name_v + name_off[r], text + head_s[r], nn);
  if (nd) copy_run(desc_v + desc_off[r], text + head_s[r] + nn + 1, nd);
  copy_run(seq_v + seq_off[r], text + seq_s[r], (unsigned)(seq_off[r + 1] - seq_off[r]));
  copy_run(qual_v + qual_off[r], text + qual_s[r], (unsigned)(qual_off[r + 1] - qual_off[r]));
}

// ---- FASTA -------------------------------------------------------------------------------------------------------------------------
// id, description, sequence (THE RULES: gpu_parse.hip, next to the FASTA parser; host/formats.h FASTAArrayBuilder::append).  The
// definition [head_s[r], head_e[r]) is ONE line, so id and description are measured and filled by a thread per record: the id
// runs up to the first ' ' or '\t' (FASTQ's rule knows the space alone and keeps what follows it as it stands: not reusable), the
// description starts behind the whole run of blanks and is NULL when nothing is left.  It ends where the definition ends, so
// the fill finds it again from its length.
__global__ __launch_bounds__(TPB) void k_fasta_measure(const uint8_t* __restrict__ text, unsigned n_records, const int32_t* __restrict__ head_s,
                                                       const int32_t* __restrict__ head_e, uint32_t* __restrict__ id_len, uint32_t* __restrict__ desc_len,
                                                       uint32_t* __restrict__ desc_valid) {
  const unsigned r = blockIdx.x * TPB + threadIdx.x;
  bool has_desc = false;
  if (r < n_records) {
    const unsigned b = (unsigned)head_s[r], e = (unsigned)head_e[r];
    unsigned ws = b;
    while (ws < e && text[ws] != ' ' && text[ws] != '\t') ++ws;
    unsigned d = ws;
    while (d < e && (text[d] == ' ' || text[d] == '\t')) ++d;
    has_desc = d < e;
    id_len[r] = ws - b;
    desc_len[r] = e - d;
  }
  const unsigned long long m = __ballot(has_desc);
  if ((threadIdx.x & 63) == 0 && r < n_records + 63) {
    desc_valid[r >> 5] = (uint32_t)m;
    desc_valid[(r >> 5) + 1] = (uint32_t)(m >> 32);
  }
}
// cap: the bytes either pool holds; n_total: the bytes readable at `text`.  A record that would reach past either writes nothing
// (never, by the capacity table: both columns are parts of the text)
__global__ __launch_bounds__(TPB) void k_fasta_head_fill(const uint8_t* __restrict__ text, unsigned n_total, unsigned n_records, const int32_t* __restrict__ head_s,
                                                         const int32_t* __restrict__ head_e, const int32_t* __restrict__ id_off, const int32_t* __restrict__ desc_off,
                                                         uint8_t* __restrict__ id_v, uint8_t* __restrict__ desc_v, unsigned cap) {
  const unsigned r = blockIdx.x * TPB + threadIdx.x;
  if (r >= n_records) return;
  const unsigned b = (unsigned)head_s[r], e = (unsigned)head_e[r];
  const unsigned ia = (unsigned)id_off[r], in = (unsigned)(id_off[r + 1] - id_off[r]);
  const unsigned da = (unsigned)desc_off[r], dn = (unsigned)(desc_off[r + 1] - desc_off[r]);
  if (e > n_total || b > e || in > e - b || dn > e - b) return;
  if (in && (uint64_t)ia + in <= cap) copy_run(id_v + ia, text + b, in);
  if (dn && (uint64_t)da + dn <= cap) copy_run(desc_v + da, text + (e - dn), dn);
}
// The hot kernel: the sequence column.  The work is cut by LINE, not by record -- a slab that is one 10 MB contig and a slab of
// 100 000 short records are the same few hundred thousand lines of 60 - 80 bytes, and nothing a lane does grows with a record.
// FASTA_LPL = 8 lanes take a line, 8 bytes each per step (64 bytes a step: one step for a 60-column line, two for 80); line l's
// bytes [begin, begin + n) go to [line_dst[l], line_dst[l] + n) with n = line_dst[l + 1] - line_dst[l] (0 for definition and empty
// lines: those lanes leave at once).  Both sides are unaligned (any line length, any offset): the 8-byte moves are two dword
// loads and two dword stores, as in copy_run -- the hardware takes unaligned dwords, and the eight lanes of a line and the lines
// of a wave are contiguous in the text and, definition lines apart, in the column.  The last 1 - 7 bytes of a line go one by one.
// BOUNDS: a load stays inside the line ([begin, begin + n), begin + n <= line_end[l] < n_total -- checked, not assumed); a store
// stays inside [line_dst[l], line_dst[l] + n) and below seq_bytes = seq_offsets[n_records] <= cap: lines of the record a
// non-final slab leaves behind start at or beyond seq_bytes and write nothing.
constexpr unsigned FASTA_LPL = 8;  // lanes per line
__global__ __launch_bounds__(TPB) void k_fasta_seq_fill(const uint8_t* __restrict__ text, unsigned n_total, unsigned skip, const unsigned* __restrict__ line_end,
                                                        const uint32_t* __restrict__ line_dst, unsigned n_lines, uint8_t* __restrict__ seq_v, unsigned seq_bytes,
                                                        unsigned cap) {
  const unsigned t = blockIdx.x * TPB + threadIdx.x;
  const unsigned line = t / FASTA_LPL, sub = t % FASTA_LPL;
  if (line >= n_lines) return;
  const unsigned at = line_dst[line], n = line_dst[line + 1] - at;
  if (n == 0) return;
  const unsigned begin = line ? line_end[line - 1] + 1u : skip, end = line_end[line];
  if (end > n_total || begin > end || n > end - begin) return;                          // loads: inside the line, inside the slab
  if ((uint64_t)at + n > seq_bytes || (uint64_t)at + n > cap) return;  // stores: inside the emitted records' bytes, inside the pool
  const uint8_t* __restrict__ src = text + begin;
  uint8_t* __restrict__ dst = seq_v + at;
  unsigned i = sub * 8u;
  for (; i + 8u <= n; i += FASTA_LPL * 8u) {
    const uint32_t a = *reinterpret_cast<const uint32_t*>(src + i), b = *reinterpret_cast<const uint32_t*>(src + i + 4);
    *reinterpret_cast<uint32_t*>(dst + i) = a;
    *reinterpret_cast<uint32_t*>(dst + i + 4) = b;
  }
  for (; i < n; ++i) dst[i] = src[i];  // (the one lane whose 8-byte group the line's end cuts: i + 8 > n here)
}

// ---- SAM ---------------------------------------------------------------------------------------------------------------------------
// The BAM columns from an alignment LINE (exon-sam/src/array_builder.rs:101-185 over noodles' RecordBuf): QNAME '*' -> NULL; the
// CIGAR printed op by op ('*' -> ""; a text the printer would change -- an op count with a leading zero -- or would refuse makes
// the row undecided: the host reader takes the file); SEQ '*' -> ""; QUAL '*' -> an empty list, else Phred = char - 33 (a
// character outside '!'..'~' is the reader's error: undecided).  Fields 1 (QNAME), 6 (CIGAR), 10 (SEQ), 11 (QUAL) by their tabs.
struct SamLens {
  uint32_t *name, *cigar, *seq, *qual;
  uint32_t* field_off;  // [4 n]: where QNAME, CIGAR, SEQ, QUAL start
};
__global__ __launch_bounds__(TPB) void k_sam_measure(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned n_rows, unsigned skip, SamLens o,
                                                     uint32_t* __restrict__ name_valid, unsigned* __restrict__ undecided) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  bool nv = false, bad = false;
  if (row < n_rows) {
    const unsigned begin = row ? nl[row - 1] + 1 : skip;
    unsigned end = nl[row];
    if (end > begin && text[end - 1] == '\r') --end;
    unsigned fs[12];
    int nf = 0;
    fs[0] = begin;
    for (unsigned i = begin; i < end && nf < 11; ++i)
      if (text[i] == '\t') fs[++nf] = i + 1;
    unsigned off[4] = {begin, begin, begin, begin}, len[4] = {0, 0, 0, 0};
    if (nf < 10) {
      bad = true;  // fewer than 11 fields
    } else {
      const int which[4] = {0, 5, 9, 10};
      for (int k = 0; k < 4; ++k) {
        const int f = which[k];
        off[k] = fs[f];
        len[k] = (f < nf ? fs[f + 1] - 1 : end) - fs[f];
      }
      auto star = [&](int k) { return len[k] == 1 && text[off[k]] == '*'; };
      nv = !star(0);
      if (star(0)) len[0] = 0;
      if (star(1)) {
        len[1] = 0;
      } else {  // digits (no leading zero: the printed form is the text) then one of MIDNSHP=X, repeated
        bool digits = false, lead = true;
        for (unsigned i = 0; i < len[1]; ++i) {
          const uint8_t c = text[off[1] + i];
          if (c >= '0' && c <= '9') {
            if (lead && c == '0') bad = true;
            lead = false;
            digits = true;
          } else {
            const bool op = c == 'M' || c == 'I' || c == 'D' || c == 'N' || c == 'S' || c == 'H' || c == 'P' || c == '=' || c == 'X';
            if (!digits || !op) bad = true;
            digits = false;
            lead = true;
          }
        }
        if (digits || len[1] == 0) bad = true;
      }
      if (star(2)) len[2] = 0;
      if (star(3)) {
        len[3] = 0;
      } else {
        for (unsigned i = 0; i < len[3]; ++i) {
          const uint8_t c = text[off[3] + i];
          if (c < 33 || c > 126) bad = true;
        }
      }
    }
    o.name[row] = len[0];
    o.cigar[row] = len[1];
    o.seq[row] = len[2];
    o.qual[row] = len[3];
    for (int k = 0; k < 4; ++k) o.field_off[4 * row + k] = off[k];
  }
  const unsigned long long bv = __ballot(nv), bb = __ballot(bad);
  const unsigned lane = threadIdx.x & 63u, wrow = row - lane;
  if (lane < 2 && wrow + 32 * lane < n_rows) name_valid[(wrow >> 5) + lane] = (uint32_t)(bv >> (32 * lane));
  if (lane == 0 && bb) atomicAdd(undecided, (unsigned)__popcll(bb));
}
__global__ __launch_bounds__(TPB) void k_sam_fill(const uint8_t* __restrict__ text, unsigned n_rows, SamLens o, uint64_t projection, const int32_t* __restrict__ name_off,
                                                  const int32_t* __restrict__ cigar_off, const int32_t* __restrict__ seq_off, const int32_t* __restrict__ qual_off,
                                                  uint8_t* __restrict__ name_v, uint8_t* __restrict__ cigar_v, uint8_t* __restrict__ seq_v, int64_t* __restrict__ qual_v) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n_rows) return;
  const uint32_t* fo = o.field_off + 4 * row;
  if (projection & EXON_HIP_PROJECT_BAM_NAME) copy_run(name_v + name_off[row], text + fo[0], o.name[row]);
  if (projection & EXON_HIP_PROJECT_BAM_CIGAR) copy_run(cigar_v + cigar_off[row], text + fo[1], o.cigar[row]);
  if (projection & EXON_HIP_PROJECT_BAM_SEQUENCE) copy_run(seq_v + seq_off[row], text + fo[2], o.seq[row]);
  if (projection & EXON_HIP_PROJECT_BAM_QUALITY_SCORES) {
    int64_t* dst = qual_v + qual_off[row];
    const uint8_t* q = text + fo[3];
    for (unsigned i = 0; i < o.qual[row]; ++i) dst[i] = (int64_t)q[i] - 33;
  }
}

// ---- BCF ---------------------------------------------------------------------------------------------------------------------------
// id / ref / alt of a BCF record (VCF specification 6.3.1): behind the 24 fixed bytes of the shared block (the record starts with
// l_shared, l_indiv) the ID as a typed string (';'-separated, "." = none) and n_allele typed strings, the first one REF.  A typed
// value's descriptor byte is count << 4 | type (7 = characters); count 15 = the real count follows as a typed integer.
struct BcfLens {
  uint32_t *id_items, *id_bytes, *ref_bytes, *alt_items, *alt_bytes;
};
// the typed string at p: where its characters start and how many there are; false: not a string (or past `end`)
__device__ __forceinline__ bool bcf_typed_string(const uint8_t* d, uint32_t* p, uint32_t end, uint32_t* at, uint32_t* len) {
  if (*p >= end) return false;
  const uint8_t b = d[(*p)++];
  uint32_t n = b >> 4;
  const uint32_t t = b & 15u;
  if (n == 15) {
    if (*p >= end) return false;
    const uint8_t c = d[(*p)++];
    const uint32_t ct = c & 15u;
    if ((c >> 4) != 1 || ct < 1 || ct > 3) return false;
    const uint32_t w = ct == 1 ? 1u : ct == 2 ? 2u : 4u;
    if (*p + w > end) return false;
    n = 0;
    for (uint32_t i = 0; i < w; ++i) n |= (uint32_t)d[*p + i] << (8 * i);
    *p += w;
  }
  if (!(t == 7 || (t == 0 && n == 0))) return false;
  if (n > end - *p) return false;  // (*p <= end here; `*p + n` would wrap for a count near 2^32)
  *at = *p;
  *len = t == 7 ? n : 0u;
  *p += *len;
  return true;
}
__global__ __launch_bounds__(TPB) void k_bcf_measure(const uint8_t* __restrict__ d, const uint32_t* __restrict__ rec_of_row, unsigned n_rows, BcfLens o,
                                                     unsigned* __restrict__ undecided) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  bool bad = false;
  if (row < n_rows) {
    const uint32_t r = rec_of_row[row];
    const uint32_t ls = ld32u(d + r), nia = ld32u(d + r + 24);
    const uint32_t n_allele = nia >> 16, end = r + 8 + ls;
    uint32_t p = r + 32, at = 0, len = 0;
    unsigned id_items = 0, id_bytes = 0, ref_bytes = 0, alt_items = 0, alt_bytes = 0;
    if (!bcf_typed_string(d, &p, end, &at, &len)) bad = true;
    if (!bad && !(len == 0 || (len == 1 && d[at] == '.'))) {
      id_items = 1;
      id_bytes = len;
      for (uint32_t i = 0; i < len; ++i)
        if (d[at + i] == ';') {
          ++id_items;
          --id_bytes;
        }
    }
    for (uint32_t a = 0; a < n_allele && !bad; ++a) {
      if (!bcf_typed_string(d, &p, end, &at, &len)) {
        bad = true;
        break;
      }
      if (a == 0) ref_bytes = len;
      else {
        ++alt_items;
        alt_bytes += len;
      }
    }
    o.id_items[row] = bad ? 0u : id_items;
    o.id_bytes[row] = bad ? 0u : id_bytes;
    o.ref_bytes[row] = bad ? 0u : ref_bytes;
    o.alt_items[row] = bad ? 0u : alt_items;
    o.alt_bytes[row] = bad ? 0u : alt_bytes;
  }
  const unsigned long long bb = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && bb) atomicAdd(undecided, (unsigned)__popcll(bb));
}
__global__ __launch_bounds__(TPB) void k_bcf_fill(const uint8_t* __restrict__ d, const uint32_t* __restrict__ rec_of_row, unsigned n_rows, uint64_t projection,
                                                  const int32_t* __restrict__ id_list_off, const int32_t* __restrict__ id_byte_off, const int32_t* __restrict__ ref_off,
                                                  const int32_t* __restrict__ alt_list_off, const int32_t* __restrict__ alt_byte_off, int32_t* __restrict__ id_item_off,
                                                  int32_t* __restrict__ alt_item_off, uint8_t* __restrict__ id_values, uint8_t* __restrict__ ref_values,
                                                  uint8_t* __restrict__ alt_values, unsigned id_items_total, unsigned id_bytes_total, unsigned alt_items_total,
                                                  unsigned alt_bytes_total) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n_rows) return;
  const uint32_t r = rec_of_row[row];
  const uint32_t ls = ld32u(d + r), nia = ld32u(d + r + 24);
  const uint32_t n_allele = nia >> 16, end = r + 8 + ls;
  uint32_t p = r + 32, at = 0, len = 0;
  if (bcf_typed_string(d, &p, end, &at, &len) && (projection & EXON_HIP_PROJECT_VCF_ID) && id_list_off[row + 1] > id_list_off[row]) {
    unsigned k = (unsigned)id_list_off[row], w = (unsigned)id_byte_off[row];
    id_item_off[k++] = (int32_t)w;
    for (uint32_t i = 0; i < len; ++i) {
      const uint8_t c = d[at + i];
      if (c == ';') id_item_off[k++] = (int32_t)w;
      else id_values[w++] = c;
    }
  }
  unsigned ak = (unsigned)alt_list_off[row], aw = (unsigned)alt_byte_off[row];
  for (uint32_t a = 0; a < n_allele; ++a) {
    if (!bcf_typed_string(d, &p, end, &at, &len)) break;
    if (a == 0) {
      if (projection & EXON_HIP_PROJECT_VCF_REF) copy_run(ref_values + ref_off[row], d + at, len);
    } else if (projection & EXON_HIP_PROJECT_VCF_ALT) {
      alt_item_off[ak++] = (int32_t)aw;
      copy_run(alt_values + aw, d + at, len);
      aw += len;
    }
  }
  if (row == n_rows - 1) {
    id_item_off[id_items_total] = (int32_t)id_bytes_total;
    alt_item_off[alt_items_total] = (int32_t)alt_bytes_total;
  }
}
enum { BCF_ID_ITEMS, BCF_ALT_ITEMS };  // ExonTextScratch::item_off

// ---- GFF ---------------------------------------------------------------------------------------------------------------------------
// `attributes`, Map<Utf8, List<Utf8>>, by THE ATTRIBUTE RULES of host/gff.h: the ninth field of row r is text[off[r], off[r] +
// len[r]) (k_parse_gff_lines<true> recorded it under the row's RANK, so ranked slabs and row = line slabs look the same here).
// Both kernels walk the field once, byte by byte, through the same states: pieces end at ';', the key at the piece's first '=',
// items at ',' behind it; "%XX" is one byte of the key or item it stands in (hex digits are no separators, so an escape never
// straddles one).  A byte >= 0x80, raw or decoded, makes the row undecided: whether it is UTF-8 is the host reader's to say.
__device__ __forceinline__ int gff_hex(unsigned c) {
  const unsigned d = c - (unsigned)'0', l = (c | 0x20u) - (unsigned)'a';
  return d <= 9u ? (int)d : l <= 5u ? (int)l + 10 : -1;
}
// the byte at text[i] of a field that ends at `end`, decoded: *step = 3 for an escape, else 1
__device__ __forceinline__ unsigned gff_attr_byte(const uint8_t* __restrict__ text, unsigned i, unsigned end, unsigned* step) {
  const unsigned c = text[i];
  *step = 1;
  if (c == '%' && i + 2 < end) {
    const int h = gff_hex(text[i + 1]), l = gff_hex(text[i + 2]);
    if ((h | l) >= 0) {
      *step = 3;
      return (unsigned)(h * 16 + l) | 0x100u;  // (bit 8: decoded, never a separator)
    }
  }
  return c;
}
struct GffLens {
  uint32_t *entries, *items, *key_bytes, *item_bytes;  // per row
};
__global__ __launch_bounds__(TPB) void k_gff_attr_measure(const uint8_t* __restrict__ text, const uint32_t* __restrict__ attr_off, const uint32_t* __restrict__ attr_len,
                                                          unsigned n_rows, GffLens o, unsigned* __restrict__ undecided) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  bool bad = false;
  if (row < n_rows) {
    const unsigned begin = attr_off[row], end = begin + attr_len[row];
    unsigned entries = 0, items = 0, kb = 0, ib = 0;
    if (!(end == begin || (end == begin + 1 && text[begin] == '.'))) {
      unsigned piece = 0;   // bytes of the piece so far (raw)
      bool in_key = true;   // in front of the piece's first '='
      for (unsigned i = begin, step; i < end; i += step) {
        const unsigned c = gff_attr_byte(text, i, end, &step);
        bad |= (c & 0x80u) != 0;
        if (c == ';') {
          bad |= piece == 0 || in_key;  // an empty piece, or one without '='
          piece = 0;
          in_key = true;
          continue;
        }
        piece += step;
        if (in_key) {
          if (c == '=') {
            in_key = false;
            ++entries;
            ++items;
          } else {
            ++kb;
          }
        } else if (c == ',') {
          ++items;
        } else {
          ++ib;
        }
      }
      bad |= piece != 0 && in_key;  // (piece == 0 here: the one empty piece behind a trailing ';')
    }
    o.entries[row] = bad ? 0u : entries;
    o.items[row] = bad ? 0u : items;
    o.key_bytes[row] = bad ? 0u : kb;
    o.item_bytes[row] = bad ? 0u : ib;
  }
  const unsigned long long bb = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && bb) atomicAdd(undecided, (unsigned)__popcll(bb));
}
// row_* : the scans of the four lengths (the row's first entry, item, key byte, item byte); row_entry is the map's offsets buffer
__global__ __launch_bounds__(TPB) void k_gff_attr_fill(const uint8_t* __restrict__ text, const uint32_t* __restrict__ attr_off, const uint32_t* __restrict__ attr_len,
                                                       unsigned n_rows, const int32_t* __restrict__ row_entry, const int32_t* __restrict__ row_item,
                                                       const int32_t* __restrict__ row_kb, const int32_t* __restrict__ row_ib, int32_t* __restrict__ key_off,
                                                       int32_t* __restrict__ list_off, int32_t* __restrict__ item_off, uint8_t* __restrict__ key_values,
                                                       uint8_t* __restrict__ item_values, unsigned entries_total, unsigned items_total, unsigned kb_total,
                                                       unsigned ib_total) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n_rows) return;
  const unsigned begin = attr_off[row], end = begin + attr_len[row];
  if (row_entry[row + 1] > row_entry[row]) {  // (a row of no entries writes nothing: "", ".")
    unsigned e = (unsigned)row_entry[row], it = (unsigned)row_item[row], kw = (unsigned)row_kb[row], iw = (unsigned)row_ib[row];
    bool in_key = true, fresh = true;  // fresh: the next byte opens a piece
    for (unsigned i = begin, step; i < end; i += step) {
      const unsigned c = gff_attr_byte(text, i, end, &step);
      if (c == ';') {
        in_key = true;
        fresh = true;
        continue;
      }
      if (fresh) {
        key_off[e] = (int32_t)kw;
        list_off[e] = (int32_t)it;
        ++e;
        fresh = false;
      }
      if (in_key) {
        if (c == '=') {
          in_key = false;
          item_off[it++] = (int32_t)iw;
        } else {
          key_values[kw++] = (uint8_t)c;
        }
      } else if (c == ',') {
        item_off[it++] = (int32_t)iw;
      } else {
        item_values[iw++] = (uint8_t)c;
      }
    }
  }
  if (row == n_rows - 1) {  // the closing offsets (entry 0 of each level when the slab has no entry at all)
    key_off[entries_total] = (int32_t)kb_total;
    list_off[entries_total] = (int32_t)items_total;
    item_off[items_total] = (int32_t)ib_total;
  }
}
enum { GFF_KEY_OFF, GFF_LIST_OFF, GFF_ITEM_OFF };  // ExonTextScratch::item_off: the entries' keys, their value lists, the items' bytes

// ---- GTF ---------------------------------------------------------------------------------------------------------------------------
// `attributes`, Map<Utf8, Utf8>, by THE ATTRIBUTE RULES of host/gtf.h: the ninth field of row r is text[off[r], off[r] + len[r])
// (k_parse_gff_lines<true, true> recorded it under the row's rank).  Both kernels walk the field once through the same five
// states -- key, gap, quoted value, bare value, after-value -- in gtf_attr_walk, which calls `emit` with the spans of every
// entry's key and value: they are parts of the text as they stand (quotes and trailing spaces lie outside the spans, nothing is
// decoded), so the measure kernel adds up their lengths and the fill kernel copies them eight bytes at a time.  A byte >= 0x80
// anywhere in the field makes the row undecided: whether it is UTF-8 is the host reader's to say.
enum : unsigned { GTF_KEY, GTF_GAP, GTF_QUOTED, GTF_BARE, GTF_AFTER };
// true: the field breaks a rule (entries emitted in front of the break do not count: the row is the host reader's)
template <class Emit>
__device__ __forceinline__ bool gtf_attr_walk(const uint8_t* __restrict__ text, unsigned begin, unsigned end, Emit&& emit) {
  unsigned st = GTF_KEY;
  unsigned kb = begin, ke = begin, vb = begin, ve = begin;  // the key [kb, ke); a bare value up to its last non-space byte [vb, ve)
  bool bad = false;
  for (unsigned i = begin; i < end; ++i) {
    const unsigned c = text[i];
    bad |= c >= 0x80u;
    if (st == GTF_KEY) {
      if (c == ' ') {
        if (i == kb) kb = i + 1;  // spaces in front of a key
        else ke = i, st = GTF_GAP;
      } else if (c == ';') {  // an empty piece, or a key without a value
        bad = true;
        kb = i + 1;
      }
    } else if (st == GTF_GAP) {
      if (c == ';') {  // a key without a value
        bad = true;
        kb = i + 1;
        st = GTF_KEY;
      } else if (c == '"') {
        vb = i + 1;
        st = GTF_QUOTED;
      } else if (c != ' ') {
        vb = i;
        ve = i + 1;
        st = GTF_BARE;
      }
    } else if (st == GTF_QUOTED) {
      if (c == '"') {
        emit(kb, ke, vb, i);
        st = GTF_AFTER;
      }
    } else if (st == GTF_BARE) {
      if (c == ';') {
        emit(kb, ke, vb, ve);
        kb = i + 1;
        st = GTF_KEY;
      } else if (c != ' ') {
        ve = i + 1;
      }
    } else {  // GTF_AFTER: spaces, then ';' or the end
      if (c == ';') {
        kb = i + 1;
        st = GTF_KEY;
      } else if (c != ' ') {
        bad = true;
      }
    }
  }
  if (st == GTF_BARE) emit(kb, ke, vb, ve);
  // the field may end behind an entry or in front of a key; not inside a key, behind one, or inside quotes
  return bad || (st == GTF_KEY && kb < end) || st == GTF_GAP || st == GTF_QUOTED;
}
struct GtfLens {
  uint32_t *entries, *key_bytes, *value_bytes;  // per row
};
__global__ __launch_bounds__(TPB) void k_gtf_attr_measure(const uint8_t* __restrict__ text, const uint32_t* __restrict__ attr_off, const uint32_t* __restrict__ attr_len,
                                                          unsigned n_rows, GtfLens o, unsigned* __restrict__ undecided) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  bool bad = false;
  if (row < n_rows) {
    const unsigned begin = attr_off[row], end = begin + attr_len[row];
    unsigned entries = 0, kbytes = 0, vbytes = 0;
    bad = gtf_attr_walk(text, begin, end, [&](unsigned kb, unsigned ke, unsigned vb, unsigned ve) {
      ++entries;
      kbytes += ke - kb;
      vbytes += ve - vb;
    });
    o.entries[row] = bad ? 0u : entries;
    o.key_bytes[row] = bad ? 0u : kbytes;
    o.value_bytes[row] = bad ? 0u : vbytes;
  }
  const unsigned long long bb = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && bb) atomicAdd(undecided, (unsigned)__popcll(bb));
}
// row_* : the scans of the three lengths (the row's first entry, key byte, value byte); row_entry is the map's offsets buffer.
// Every write is bounded by what its buffer holds (offset_cap entries in key_off / value_off, byte_cap bytes in the two pools).
__global__ __launch_bounds__(TPB) void k_gtf_attr_fill(const uint8_t* __restrict__ text, const uint32_t* __restrict__ attr_off, const uint32_t* __restrict__ attr_len,
                                                       unsigned n_rows, const int32_t* __restrict__ row_entry, const int32_t* __restrict__ row_kb,
                                                       const int32_t* __restrict__ row_vb, int32_t* __restrict__ key_off, int32_t* __restrict__ value_off,
                                                       uint8_t* __restrict__ key_values, uint8_t* __restrict__ value_values, unsigned entries_total,
                                                       unsigned kb_total, unsigned vb_total, unsigned offset_cap, unsigned byte_cap) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n_rows) return;
  if (row_entry[row + 1] > row_entry[row]) {  // (a row of no entries writes nothing)
    const unsigned begin = attr_off[row], end = begin + attr_len[row];
    unsigned e = (unsigned)row_entry[row], kw = (unsigned)row_kb[row], vw = (unsigned)row_vb[row];
    gtf_attr_walk(text, begin, end, [&](unsigned kb, unsigned ke, unsigned vb, unsigned ve) {
      const unsigned kn = ke - kb, vn = ve - vb;
      if (e < offset_cap) {
        key_off[e] = (int32_t)kw;
        value_off[e] = (int32_t)vw;
      }
      if (kw + kn <= byte_cap) copy_run(key_values + kw, text + kb, kn);
      if (vw + vn <= byte_cap) copy_run(value_values + vw, text + vb, vn);
      ++e;
      kw += kn;
      vw += vn;
    });
  }
  if (row == n_rows - 1 && entries_total < offset_cap) {  // the closing offsets (entry 0 of both levels when the slab has no entry at all)
    key_off[entries_total] = (int32_t)kb_total;
    value_off[entries_total] = (int32_t)vb_total;
  }
}
enum { GTF_KEY_OFF, GTF_VALUE_OFF };  // ExonTextScratch::item_off: the entries' keys and values

// ---- BED `name` --------------------------------------------------------------------------------------------------------------------
// The name column of a BED slab (host/bed.h: the field's bytes as they stand; NULL on 3- and 4-field lines).  The line kernel
// (gpu_parse.hip, k_parse_bed_lines<true>) has recorded where every row's name lies, how long it is (0 where NULL) and the validity
// bitmap, so there is nothing left to measure: the lengths are scanned into offsets and the fill copies the spans with
// k_fastq_fill's 8-byte copier.  Every write is bounded by the buffer's size, whatever the capacity table says.
__global__ __launch_bounds__(TPB) void k_bed_name_fill(const uint8_t* __restrict__ text, unsigned n_total, unsigned n_rows, const uint32_t* __restrict__ name_off,
                                                       const int32_t* __restrict__ off, uint8_t* __restrict__ values, unsigned cap) {
  const unsigned r = blockIdx.x * TPB + threadIdx.x;
  if (r >= n_rows) return;
  const unsigned at = (unsigned)off[r], n = (unsigned)(off[r + 1] - off[r]), src = name_off[r];
  if (n == 0 || (uint64_t)at + n > cap || (uint64_t)src + n > n_total) return;  // (the last two: never, by the capacity table)
  copy_run(values + at, text + src, n);
}

// ---- VCF `info` --------------------------------------------------------------------------------------------------------------------
// The `info` Utf8 column (host/vcf_text.h: vcf_info_string / print_value / print_i32, restated): field 8 of the line, its entries
// printed again.  "" for an empty field or "."; pieces split at ';' (empty ones skipped), a piece at its first '='; the type
// comes from the key (ExonVcfKeyTable: the header's ##INFO lines over the reserved keys, a miss is String); a Flag prints
// "key=true" whatever follows it; String values, and Character values without a comma, are copied; otherwise the items between
// ',' are printed one by one -- "." as ".", except in a Character list, which drops it; an Integer through the i32 rules (sign,
// digits, |v| <= 2^31 and v <= 2^31 - 1, printed without '+', leading zeros or "-0"); a Float through dec::parse_f32 and
// f32p::print (host/decimal_f32.h, host/f32_print.h).
// UNDECIDED (the row is counted, the file goes to the host reader, which prints it or raises with its own message): fewer than
// eight fields; a key without a value ("key", "key=", "key=."); an integer print_i32 refuses; a float dec::parse_f32 leaves
// open -- more than 19 significant digits, anything that is no plain decimal (the inf / infinity / nan spellings are NOT handed
// over: vcf_f32_word takes them, they print "inf" / "-inf" / "NaN"); a byte >= 0x80 anywhere in the field: the host builder copies such bytes as they stand, and
// whether they are UTF-8 is the host reader's to say, as for the GFF and GTF attributes.
// Both kernels are instantiations of vcf_info_walk, which calls its emitter with what the row prints: the measure kernel's adds
// lengths up, the fill kernel's writes into [offsets[r], offsets[r + 1]) and never outside it.  The measure kernel finds field 8
// by the line's tabs (as k_vcf_measure finds fields 3 - 5; k_parse_lines is not touched) and leaves its place for the fill.
__host__ __device__ __forceinline__ uint64_t vcf_key_hash(const uint8_t* p, unsigned n) {  // FNV-1a; never 0 (0 marks an empty slot)
  uint64_t h = 0xcbf29ce484222325ull;
  for (unsigned i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
  return h | (1ull << 63);
}
// the type of the key text[kb, kb + kn): by hash, then by the text (a key of the file may collide with one of the header)
__device__ __forceinline__ unsigned vcf_key_type(const ExonVcfKeyTable& t, const uint8_t* __restrict__ text, unsigned kb, unsigned kn) {
  const uint64_t h = vcf_key_hash(text + kb, kn);
  for (unsigned slot = (unsigned)h & t.mask;; slot = (slot + 1) & t.mask) {  // (at most half of the slots are taken)
    const uint64_t e = t.hash[slot];
    if (e == 0) return 's';
    if (e != h || t.len[slot] != kn) continue;
    const uint8_t* k = t.text + t.off[slot];
    unsigned i = 0;
    while (i < kn && k[i] == text[kb + i]) ++i;
    if (i == kn) return t.type[slot];
  }
}
// [sign] (inf | infinity | nan) in any letter case, the spellings Rust's f32::from_str takes next to the decimals (the host
// reader: VCFArrayBuilder::parse_f32); the sign of a NaN is kept and never printed
__device__ __forceinline__ bool vcf_f32_word(const uint8_t* __restrict__ text, unsigned a, unsigned e, uint32_t* bits) {
  uint32_t sign = 0;
  if (a < e && (text[a] == '-' || text[a] == '+')) sign = text[a++] == '-' ? 0x80000000u : 0u;
  const unsigned n = e - a;
  if (n != 3 && n != 8) return false;
  uint64_t w = 0;  // the letters, lower case, first one in the top byte
  for (unsigned i = 0; i < n; ++i) w = w << 8 | (text[a + i] | 0x20u);
  if (w == 0x696e66ull || w == 0x696e66696e697479ull) *bits = sign | 0x7F800000u;  // "inf", "infinity"
  else if (w == 0x6e616eull) *bits = sign | 0x7FC00000u;                           // "nan"
  else return false;
  return true;
}
// true: the row is undecided (what has been emitted by then does not count)
template <class Emit>
__device__ __forceinline__ bool vcf_info_walk(const uint8_t* __restrict__ text, unsigned begin, unsigned end, const ExonVcfKeyTable& kt, Emit& em) {
  if (end == begin || (end == begin + 1 && text[begin] == '.')) return false;
  bool bad = false, first_entry = true;
  for (unsigned i = begin; i < end && !bad;) {
    unsigned j = i, eq = end;  // the piece [i, j), its first '=' (end: none)
    for (; j < end; ++j) {
      const unsigned c = text[j];
      bad |= c >= 0x80u;
      if (c == ';') break;
      if (c == '=' && eq == end) eq = j;
    }
    if (j > i) {
      const bool has_eq = eq != end;
      if (!has_eq) eq = j;
      const unsigned ty = vcf_key_type(kt, text, i, eq - i);
      if (!first_entry) em.byte(';');
      first_entry = false;
      em.span(i, eq - i);
      em.byte('=');
      const unsigned vb = eq + 1, vl = has_eq ? j - vb : 0u, ve = vb + vl;
      if (ty == 'b') {
        em.word_true();
      } else if (vl == 0 || (vl == 1 && text[vb] == '.')) {
        bad = true;  // a missing value
      } else {
        bool comma = false;
        if (ty == 'c')
          for (unsigned k = vb; k < ve; ++k) comma |= text[k] == ',';
        if (ty == 's' || (ty == 'c' && !comma)) {
          em.span(vb, vl);
        } else {
          bool first_item = true;
          for (unsigned a = vb; a <= ve && !bad;) {
            unsigned e = a;
            while (e < ve && text[e] != ',') ++e;
            const bool dot = e - a == 1 && text[a] == '.';
            if (!(dot && ty == 'c')) {
              if (!first_item) em.byte(',');
              first_item = false;
              if (dot) {
                em.byte('.');
              } else if (ty == 'i') {
                unsigned k = a;
                bool neg = false;
                if (k < e && (text[k] == '-' || text[k] == '+')) neg = text[k++] == '-';
                bad |= k == e;
                uint64_t v = 0;
                for (; k < e; ++k) {
                  const unsigned d = (unsigned)text[k] - (unsigned)'0';
                  bad |= d > 9u;
                  v = v * 10 + d;
                  if (v > 0x80000000ull) v = 0x80000001ull;  // (out of range for good: print_i32 stops here)
                }
                bad |= v > 0x80000000ull || (!neg && v > 0x7FFFFFFFull);
                if (!bad) em.i32(neg && v != 0, (uint32_t)v);
              } else if (ty == 'f') {
                uint32_t bits = 0;
                if (exon::dec::parse_f32(reinterpret_cast<const char*>(text + a), (int)(e - a), &bits) || vcf_f32_word(text, a, e, &bits)) em.f32(bits);
                else bad = true;
              } else {
                em.span(a, e - a);
              }
            }
            a = e + 1;
          }
        }
      }
    }
    i = j + 1;
  }
  return bad;
}
struct VcfInfoMeasure {
  unsigned n = 0;
  __device__ __forceinline__ void byte(unsigned) { ++n; }
  __device__ __forceinline__ void span(unsigned, unsigned len) { n += len; }
  __device__ __forceinline__ void word_true() { n += 4; }
  __device__ __forceinline__ void i32(bool minus, uint32_t v) { n += (minus ? 1u : 0u) + dec_digits(v); }
  __device__ __forceinline__ void f32(uint32_t bits) { n += (unsigned)exon::f32p::length(bits); }
};
// writes at dst[w ..); `lim` = the row's bytes by the offsets: nothing is written at or behind dst[lim]
struct VcfInfoFill {
  const uint8_t* __restrict__ text;
  uint8_t* __restrict__ dst;
  unsigned lim, w = 0;
  __device__ __forceinline__ void byte(unsigned c) {
    if (w < lim) dst[w] = (uint8_t)c;
    ++w;
  }
  __device__ __forceinline__ void span(unsigned off, unsigned len) {
    if (len <= lim && w <= lim - len) copy_run(dst + w, text + off, len);
    w += len;
  }
  __device__ __forceinline__ void word_true() {
    if (w + 4 <= lim) dst[w] = 't', dst[w + 1] = 'r', dst[w + 2] = 'u', dst[w + 3] = 'e';
    w += 4;
  }
  __device__ __forceinline__ void i32(bool minus, uint32_t v) {
    const unsigned nd = dec_digits(v), len = nd + (minus ? 1u : 0u);
    if (len <= lim && w <= lim - len) {
      if (minus) dst[w] = '-';
      uint8_t* p = dst + w + (minus ? 1u : 0u);
      for (unsigned i = nd; i > 0; --i) {
        p[i - 1] = (uint8_t)('0' + v % 10);
        v /= 10;
      }
    }
    w += len;
  }
  __device__ __forceinline__ void f32(uint32_t bits) {
    const unsigned len = (unsigned)exon::f32p::length(bits);
    if (len <= lim && w <= lim - len) exon::f32p::print(bits, dst + w);
    w += len;
  }
};
// scal: [0, 1] the slab's printed bytes as one 64-bit sum (the u32 scan of the lengths may wrap), [2] undecided rows
__global__ __launch_bounds__(TPB) void k_vcf_info_measure(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned n_rows, unsigned skip,
                                                          ExonVcfKeyTable kt, uint32_t* __restrict__ field_off, uint32_t* __restrict__ field_len,
                                                          uint32_t* __restrict__ out_len, unsigned* __restrict__ scal) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  bool bad = false;
  unsigned printed = 0;
  if (row < n_rows) {
    const unsigned begin = row ? nl[row - 1] + 1 : skip;
    unsigned end = nl[row];
    if (end > begin && text[end - 1] == '\r') --end;
    unsigned fb = begin, tabs = 0;  // field 8 starts behind the seventh tab ...
    for (; fb < end && tabs < 7; ++fb) tabs += text[fb] == '\t';
    unsigned fe = fb;  // ... and ends at the eighth or with the line
    while (fe < end && text[fe] != '\t') ++fe;
    bad = tabs < 7;  // fewer than eight fields: no data line
    VcfInfoMeasure m;
    if (!bad) bad = vcf_info_walk(text, fb, fe, kt, m);
    printed = bad ? 0u : m.n;
    field_off[row] = fb;
    field_len[row] = bad ? 0u : fe - fb;
    out_len[row] = printed;
  }
  unsigned long long sum = printed;
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
  const unsigned long long bb = __ballot(bad);
  if ((threadIdx.x & 63) == 0) {
    if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(scal), sum);
    if (bb) atomicAdd(scal + 2, (unsigned)__popcll(bb));
  }
}
// cap: the bytes `values` holds (the host has compared the total with it; a row that would reach past it writes nothing)
__global__ __launch_bounds__(TPB) void k_vcf_info_fill(const uint8_t* __restrict__ text, unsigned n_rows, ExonVcfKeyTable kt, const uint32_t* __restrict__ field_off,
                                                       const uint32_t* __restrict__ field_len, const int32_t* __restrict__ off, uint8_t* __restrict__ values,
                                                       unsigned cap) {
  const unsigned row = blockIdx.x * TPB + threadIdx.x;
  if (row >= n_rows) return;
  const unsigned at = (unsigned)off[row], n = (unsigned)(off[row + 1] - off[row]);
  if (n == 0 || (uint64_t)at + n > cap) return;
  VcfInfoFill f{text, values + at, n};
  const unsigned fb = field_off[row];
  vcf_info_walk(text, fb, fb + field_len[row], kt, f);
}

// ---- VCF `formats` -----------------------------------------------------------------------------------------------------------------
// The `formats` Utf8 column (host/vcf_text.h: vcf_formats_string, restated item by item in host/vcf_sample_walk.h, THE RULES
// there): the FORMAT field, a TAB, the samples printed again and joined by TABs.  A row of 2 504 samples is 30 - 60 KB of text,
// and a slab of such rows holds a few thousand of them: the unit of work is the SAMPLE, not the row.  No thread here does work
// that grows with the samples of its row: a thread takes 64 bytes of text (the tab index), the first nine fields of a row, or
// one sample.
//   tab index  k_fmt_tab_count / scan / k_fmt_tab_fill: the position of every TAB of the slab's rows, ascending.  The count comes
//              back before the buffers behind it are sized (one position per two bytes is the worst case; nothing is allocated
//              for it up front, and no slab has more tabs than its buffer holds).
//   rows       k_fmt_rows, a thread a row: first_tab[r] = the lower bound of the line's begin in the index; FORMAT lies between
//              tabs 7 and 8 of the row; its keys -> a word of types, 4 bits a key (0: the row prints "\t" and no sample); the head
//              item's length = len(FORMAT) + 1.
//   samples    k_fmt_sample_measure, a thread a tab: tab t of row r (binary search over the line index) with ordinal
//              t - first_tab[r] >= 8 starts sample ordinal - 8, which runs to the next tab or the line's end (its CR dropped);
//              length = the sample walk's + 1 for the TAB in front of every sample but the first.  Other tabs: 0.
//   places     the lengths lie at slot(head of r) = first_tab[r] + r and slot(tab t) = t + r + 1: ONE scan over rows + tabs words
//              places every item, and the row offsets are item_off[first_tab[r] + r] (k_fmt_head_fill gathers them).
//   fill       k_fmt_head_fill (FORMAT + TAB) and k_fmt_sample_fill write their item inside [item_off[slot], item_off[slot + 1])
//              and below the buffer's size, nowhere else.
// Nothing spins or looks back; the binary searches are bounded by the index sizes.
// UNDECIDED (the row is counted, the file goes to the host reader, which prints it or raises with its own message): fewer than
// eight fields; more than 16 FORMAT keys; a byte >= 0x80 in FORMAT or in a sample; a value that has a key and is empty or "."
// (so also a line that has FORMAT and ends there: the host raises on its empty sample); an allele that is empty or not all
// digits; an integer print_i32 refuses; a float dec::parse_f32 leaves open (the inf / infinity / nan spellings are printed
// here).  A slab whose column exceeds INT32_MAX bytes, whose rows + tabs exceed INT32_MAX, or whose buffers cannot be had is
// handed over whole.
constexpr unsigned FMT_CHUNK = 64;  // bytes of text a thread of the tab index takes
__device__ __forceinline__ unsigned tabs_in_word(uint32_t w) {  // the bytes of w that are 0x09, exactly
  const uint32_t x = w ^ 0x09090909u;
  return (unsigned)__popc(~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu));
}
// chunk c = bytes [64 c, 64 c + 64) of the aligned text; the bytes in [skip, hi) count, hi = the last row's newline
__global__ __launch_bounds__(TPB) void k_fmt_tab_count(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned n_rows, unsigned skip, unsigned n_total,
                                                       unsigned n_chunks, uint32_t* __restrict__ cnt) {
  const unsigned c = blockIdx.x * TPB + threadIdx.x;
  if (c >= n_chunks) return;
  const unsigned hi = min(nl[n_rows - 1], n_total);
  unsigned n = 0;
  for (unsigned g = 0; g < FMT_CHUNK / 16; ++g) {
    const unsigned b = c * FMT_CHUNK + g * 16;
    if (b >= hi) break;
    if (b >= skip && hi - b >= 16) {
      const uint4 v = *reinterpret_cast<const uint4*>(text + b);
      n += tabs_in_word(v.x) + tabs_in_word(v.y) + tabs_in_word(v.z) + tabs_in_word(v.w);
    } else {
      for (unsigned i = max(b, skip); i < min(b + 16, hi); ++i) n += text[i] == '\t';
    }
  }
  cnt[c] = n;
}
// cap: the positions `tabs` holds (the host sized it from the count; a position beyond it is not written)
__global__ __launch_bounds__(TPB) void k_fmt_tab_fill(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned n_rows, unsigned skip, unsigned n_total,
                                                      unsigned n_chunks, const int32_t* __restrict__ chunk_first, uint32_t* __restrict__ tabs, unsigned cap) {
  const unsigned c = blockIdx.x * TPB + threadIdx.x;
  if (c >= n_chunks) return;
  unsigned w = (unsigned)chunk_first[c];
  if ((unsigned)chunk_first[c + 1] == w) return;
  const unsigned hi = min(nl[n_rows - 1], n_total);
  const unsigned b0 = max(c * FMT_CHUNK, skip), b1 = min(c * FMT_CHUNK + FMT_CHUNK, hi);
  for (unsigned i = b0; i < b1; ++i)
    if (text[i] == '\t') {
      if (w < cap) tabs[w] = i;
      ++w;
    }
}
using VcfFmtMeasure = VcfInfoMeasure;  // (byte / span / i32 / f32: what the sample walk emits)
using VcfFmtFill = VcfInfoFill;
// the line of row r without its CR: [*begin, *end)
__device__ __forceinline__ void fmt_line(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned r, unsigned skip, unsigned* begin, unsigned* end) {
  *begin = r ? nl[r - 1] + 1 : skip;
  *end = nl[r];
  if (*end > *begin && text[*end - 1] == '\r') --*end;
}
// scal: [0, 1] the slab's printed bytes as one 64-bit sum, [2] undecided items, (shared with k_fmt_sample_measure)
__device__ __forceinline__ void fmt_tally(unsigned printed, bool bad, unsigned* __restrict__ scal) {
  unsigned long long sum = printed;
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
  const unsigned long long bb = __ballot(bad);
  if ((threadIdx.x & 63) == 0) {
    if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(scal), sum);
    if (bb) atomicAdd(scal + 2, (unsigned)__popcll(bb));
  }
}
__global__ __launch_bounds__(TPB) void k_fmt_rows(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned n_rows, unsigned skip, ExonVcfKeyTable kt,
                                                  const uint32_t* __restrict__ tabs, unsigned n_tabs, uint32_t* __restrict__ first_tab,
                                                  unsigned long long* __restrict__ types, uint32_t* __restrict__ item_len, unsigned* __restrict__ scal) {
  const unsigned r = blockIdx.x * TPB + threadIdx.x;
  bool bad = false;
  unsigned head = 0;
  if (r < n_rows) {
    unsigned begin, end;
    fmt_line(text, nl, r, skip, &begin, &end);
    unsigned lo = 0, hi = n_tabs;  // the first tab at or behind the line's begin
    while (lo < hi) {
      const unsigned mid = lo + (hi - lo) / 2;
      if (tabs[mid] < begin) lo = mid + 1;
      else hi = mid;
    }
    const unsigned ft = lo;
    unsigned nt = 0;  // the row's tabs, as far as nine matter
    while (nt < 9 && ft + nt < n_tabs && tabs[ft + nt] < end) ++nt;
    uint64_t ty = 0;
    if (nt < 7) {
      bad = true;  // fewer than eight fields: no data line
    } else if (nt >= 8) {
      const unsigned fb = tabs[ft + 7] + 1, fe = nt >= 9 ? tabs[ft + 8] : end;
      bad = !exon::vsw::format_keys(text, fb, fe, [&](unsigned kb, unsigned kn) { return vcf_key_type(kt, text, kb, kn); }, &ty);
      if (!bad && ty) {
        head = fe - fb;
        bad = nt == 8;  // FORMAT and no sample: the host reader raises on the empty one
      }
    }
    head = bad ? 0u : head + 1;
    first_tab[r] = ft;
    types[r] = bad ? 0ull : ty;
    item_len[ft + r] = head;
  }
  fmt_tally(head, bad, scal);
}
__global__ __launch_bounds__(TPB) void k_fmt_sample_measure(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned n_rows, unsigned skip,
                                                            const uint32_t* __restrict__ tabs, unsigned n_tabs, const uint32_t* __restrict__ first_tab,
                                                            const unsigned long long* __restrict__ types, uint32_t* __restrict__ tab_row,
                                                            uint32_t* __restrict__ item_len, unsigned* __restrict__ scal) {
  const unsigned t = blockIdx.x * TPB + threadIdx.x;
  bool bad = false;
  unsigned printed = 0;
  if (t < n_tabs) {
    const unsigned p = tabs[t];
    unsigned lo = 0, hi = n_rows - 1;  // the row of the tab: the first line that ends behind it (every indexed tab lies in front of the last newline)
    while (lo < hi) {
      const unsigned mid = lo + (hi - lo) / 2;
      if (nl[mid] < p) lo = mid + 1;
      else hi = mid;
    }
    const unsigned r = lo, ft = first_tab[r];
    const uint64_t ty = types[r];
    if (t >= ft + 8 && ty) {
      unsigned begin, end;
      fmt_line(text, nl, r, skip, &begin, &end);
      const unsigned sb = p + 1, se = (t + 1 < n_tabs && tabs[t + 1] < end) ? tabs[t + 1] : end;
      if (sb > se) {
        bad = true;  // (never: a tab lies in front of its line's end)
      } else {
        VcfFmtMeasure m;
        bad = exon::vsw::sample(text, sb, se, ty, m);
        printed = bad ? 0u : m.n + (t > ft + 8 ? 1u : 0u);
      }
    }
    tab_row[t] = r;
    item_len[t + r + 1] = printed;
  }
  fmt_tally(printed, bad, scal);
}
// the head item of every row (FORMAT, TAB) and the row offsets out of the items' places; cap: the bytes `values` holds
__global__ __launch_bounds__(TPB) void k_fmt_head_fill(const uint8_t* __restrict__ text, unsigned n_rows, const uint32_t* __restrict__ tabs, unsigned n_tabs,
                                                       const uint32_t* __restrict__ first_tab, const int32_t* __restrict__ item_off, int32_t* __restrict__ row_off,
                                                       uint8_t* __restrict__ values, unsigned cap, unsigned n_total) {
  const unsigned r = blockIdx.x * TPB + threadIdx.x;
  if (r >= n_rows) return;
  const unsigned ft = first_tab[r], slot = ft + r;
  const unsigned at = (unsigned)item_off[slot], n = (unsigned)(item_off[slot + 1] - item_off[slot]);
  row_off[r] = (int32_t)at;
  if (r == n_rows - 1) row_off[n_rows] = item_off[n_rows + n_tabs];
  if (n == 0 || (uint64_t)at + n > cap) return;
  if (n > 1) {  // (a head longer than its TAB: the row has a FORMAT field, so eight tabs)
    if (ft + 7 >= n_tabs) return;
    const unsigned fb = tabs[ft + 7] + 1;
    if ((uint64_t)fb + (n - 1) > n_total) return;
    copy_run(values + at, text + fb, n - 1);
  }
  values[at + n - 1] = '\t';
}
__global__ __launch_bounds__(TPB) void k_fmt_sample_fill(const uint8_t* __restrict__ text, const unsigned* __restrict__ nl, unsigned skip, const uint32_t* __restrict__ tabs,
                                                         unsigned n_tabs, const uint32_t* __restrict__ first_tab, const unsigned long long* __restrict__ types,
                                                         const uint32_t* __restrict__ tab_row, const int32_t* __restrict__ item_off, uint8_t* __restrict__ values,
                                                         unsigned cap) {
  const unsigned t = blockIdx.x * TPB + threadIdx.x;
  if (t >= n_tabs) return;
  const unsigned r = tab_row[t], slot = t + r + 1;
  const unsigned at = (unsigned)item_off[slot], n = (unsigned)(item_off[slot + 1] - item_off[slot]);
  if (n == 0 || (uint64_t)at + n > cap) return;
  unsigned begin, end;
  fmt_line(text, nl, r, skip, &begin, &end);
  const unsigned sb = tabs[t] + 1, se = (t + 1 < n_tabs && tabs[t + 1] < end) ? tabs[t + 1] : end;
  if (sb > se) return;
  VcfFmtFill f{text, values + at, n};
  if (t > first_tab[r] + 8) f.byte('\t');
  exon::vsw::sample(text, sb, se, types[r], f);
}

// What a format's kernels need of the scratch.  A scratch serves the layout it was made for and no other (scratch_for).
struct TextLayout {
  int8_t cols;         // length arrays and the offsets scanned out of them (len[k], off[k])
  int8_t pools;        // byte pools (values[k])
  int8_t item_offs;    // item-offset arrays (item_off[k]: every format names its own with an enum next to its kernels)
  int8_t field_words;  // words a row in `field`: where the measure kernel found the row's fields, for the fill
  int8_t valids;       // validity bitmaps (valid[k])
  bool operator==(const TextLayout& o) const { return cols == o.cols && pools == o.pools && item_offs == o.item_offs && field_words == o.field_words && valids == o.valids; }
};
constexpr TextLayout LAYOUT_VCF{3, 3, 1, 6, 2}, LAYOUT_BCF{5, 3, 2, 0, 0}, LAYOUT_BAM{3, 3, 0, 0, 1}, LAYOUT_SAM{4, 3, 0, 4, 1}, LAYOUT_FASTQ{4, 4, 0, 0, 1},
    LAYOUT_GFF{4, 2, 3, 0, 0}, LAYOUT_GTF{3, 2, 2, 0, 0}, LAYOUT_BED{1, 1, 0, 0, 0}, LAYOUT_FASTA{2, 3, 0, 0, 1};
constexpr int RES_WORDS = 8, RES_UNDECIDED = 7;

struct ExonTextScratch {
  PoolBufs bufs, qual_bufs;  // qual_bufs: the quality_scores values, grown on demand
  // VCF `info`: per-row buffers (field place, printed length, offsets) for info_rows rows, the printed bytes (info_cap), both grown on demand
  PoolBufs info_row_bufs, info_value_bufs;
  size_t info_rows = 0, info_cap = 0;
  uint32_t *info_field_off = nullptr, *info_field_len = nullptr, *info_len = nullptr;
  int32_t* info_off = nullptr;
  uint8_t* info_values = nullptr;
  unsigned* info_scal = nullptr;    // device [4]: k_vcf_info_measure's scalars
  unsigned* h_info_scal = nullptr;  // pinned
  // VCF `formats`: the buffers sized by the slab (fmt_rows rows, fmt_chunks chunks of FMT_CHUNK bytes), by its tabs (fmt_tabs) and
  // the printed bytes (fmt_cap), each grown on demand (fmt_for)
  PoolBufs fmt_slab_bufs, fmt_tab_bufs, fmt_value_bufs;
  size_t fmt_rows = 0, fmt_chunks = 0, fmt_tabs = 0, fmt_cap = 0;
  uint32_t *fmt_cnt = nullptr, *fmt_first_tab = nullptr;            // [chunks], [rows]
  int32_t *fmt_chunk_first = nullptr, *fmt_row_off = nullptr;       // [chunks + 1], [rows + 1]
  unsigned long long* fmt_types = nullptr;                          // [rows]
  unsigned* fmt_chunk_sums = nullptr;                               // the block sums of the scan over the chunks
  uint32_t *fmt_tab_pos = nullptr, *fmt_tab_row = nullptr;          // [tabs]
  uint32_t* fmt_item_len = nullptr;                                 // [rows + tabs]
  int32_t* fmt_item_off = nullptr;                                  // [rows + tabs + 1]
  unsigned* fmt_item_sums = nullptr;                                // the block sums of the scan over the items
  uint8_t* fmt_values = nullptr;
  unsigned* fmt_scal = nullptr;    // device [8]: [0, 1] printed bytes, [2] undecided items, [3] the u32 total of the items' scan, [4] the tabs
  unsigned* h_fmt_scal = nullptr;  // pinned
  int64_t max_rows = 0, max_bytes = 0;
  TextLayout layout{};
  uint32_t* len[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int32_t* off[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  uint32_t* valid[2] = {nullptr, nullptr};
  uint32_t* field = nullptr;  // [layout.field_words * (max_rows + 64)]: SAM [4 r]; VCF [3 r] starts and, behind them, [3 r] lengths
  unsigned* sums = nullptr;
  unsigned* res = nullptr;    // device [RES_WORDS]: the totals of the scans in the low words, the undecided rows in word RES_UNDECIDED
  unsigned* h_res = nullptr;  // pinned
  int32_t* item_off[3] = {nullptr, nullptr, nullptr};
  uint8_t* values[4] = {nullptr, nullptr, nullptr, nullptr};
  int64_t* qual = nullptr;
  size_t qual_cap = 0;
  size_t value_cap = 0;  // bytes every values[k] holds
  size_t item_cap = 0;   // entries every item_off[k] holds
  explicit ExonTextScratch(exon_hip_ctx* ctx)
      : bufs(ctx), qual_bufs(ctx), info_row_bufs(ctx), info_value_bufs(ctx), fmt_slab_bufs(ctx), fmt_tab_bufs(ctx), fmt_value_bufs(ctx) {}
};

void exon_text_scratch_destroy(ExonTextScratch* s) { delete s; }

// The largest totals a slab of n_bytes bytes and n_rows rows can produce, buffer by buffer, against the sizes below (the callers
// pass max_rows >= n_rows and max_bytes as named).  "fits": the size always holds it; "checked": it may not, fits() compares the
// total on the host before the fill kernel is launched and hands a slab that does not fit to the host reader.
//   every format  len / off / valid / field / sums: n_rows lengths, n_rows + 1 offsets, a bit a row, the layout's field words a row, a sum per
//                    256 rows; sized for max_rows + 64: fits
//   VCF    values[0] (max_bytes = n_bytes): the ID fields without their ';', parts of the text: <= n_bytes: fits
//   VCF    values[2]: the REF fields, parts of the text: <= n_bytes: fits
//   VCF    item_off[VCF_ID_ITEMS]: an ID field of k bytes is up to k + 1 items (k ';') and a line has a byte more than its ID (the LF): up to n_bytes
//                    items + 1 entry, against max_bytes / 2 + max_rows + 66: checked
//   VCF    info_values: the printed `info` entries, NOT bounded by the slab ("DB" prints "DB=true", "1e38" 39 digits: up to eight times
//                    the field).  k_vcf_info_measure yields every row's exact length and their 64-bit sum; info_for grows the buffer to
//                    the sum before the fill; a sum beyond INT32_MAX (int32 offsets), or a buffer that cannot be had, hands the slab
//                    over; k_vcf_info_fill writes inside [offsets[r], offsets[r + 1]) and below the buffer's size only: checked
//   VCF    fmt_tab_pos / fmt_tab_row: a position and a row per TAB of the slab's rows; k_fmt_tab_count yields their exact number, which
//                    comes back before fmt_for makes the buffers (a quarter more than the count, at least 64 Ki): fits; k_fmt_tab_fill
//                    bounds its writes all the same
//   VCF    fmt_item_len / fmt_item_off: rows + tabs items (+ 1 entry), against fmt_rows + fmt_tabs + 64 (+ 1): fits
//   VCF    fmt_values: the printed `formats` items, NOT bounded by the slab (as info_values): the measure kernels yield every item's
//                    exact length and their 64-bit sum; fmt_for grows the buffer to the sum before the fills; a sum beyond INT32_MAX,
//                    rows + tabs beyond INT32_MAX, or a buffer that cannot be had, hands the slab over; the fills write inside
//                    [item_off[slot], item_off[slot + 1]) and below the buffer's size only: checked
//   BCF    values[0], [1], [2] (max_bytes = n_bytes): id / ref / alt, characters of typed strings inside the records: <= n_bytes each: fits
//   BCF    item_off[BCF_ID_ITEMS]: a typed ID of k characters is up to k + 1 items behind a descriptor byte: up to n_bytes items + 1 entry: checked
//   BCF    item_off[BCF_ALT_ITEMS]: an empty allele is its descriptor byte alone: up to n_bytes items + 1 entry: checked
//   BAM    values[0] (max_bytes = 2 n_bytes): names, l_read_name - 1 bytes of the record: <= n_bytes: fits
//   BAM    values[1]: a CIGAR op of 4 bytes prints as up to 9 digits and a letter: up to 2.5 n_bytes: checked
//   BAM    values[2]: two bases a byte, 2 n_bytes when every l_seq lies inside its record; l_seq is the record's own word: checked
//   BAM    qual: l_seq items a row; qual_for grows it to the total before the fill: fits
//   SAM    values[0], [1], [2] (max_bytes = n_bytes): QNAME / CIGAR / SEQ fields, copied as they are: <= n_bytes each: fits
//   SAM    qual: an item per QUAL byte; qual_for grows it to the total before the fill: fits
//   FASTQ  values[0 .. 3] (max_bytes = n_bytes + 16): name / description / sequence / quality, disjoint parts of the text: <= n_bytes: fits
//   FASTA  values[0 .. 2] (max_bytes = n_bytes + 16): id / description / sequence, disjoint parts of the text (an id and a description share
//                    a definition line, a sequence byte lies on no definition line): <= n_bytes each: fits.  The sequence offsets are the
//                    parser's (one per record, sized for a record a line).  k_fasta_head_fill and k_fasta_seq_fill bound their reads
//                    and writes all the same.
//   GFF    (max_bytes = n_bytes; F = the bytes of the slab's ninth fields; a record has at least 16 bytes in front of its ninth field
//          -- eight fields, eight TABs -- and its LF behind it: F <= n_bytes - 17 n_rows)
//   GFF    values[0]: decoded key bytes, values[1]: decoded item bytes; a byte of either comes from a byte of the field or from three: <= F each: fits
//   GFF    item_off[GFF_KEY_OFF], [GFF_LIST_OFF] (an entry's key offset and list offset): an entry is a piece of at least a byte ("=") and all but a
//                    row's last are followed by a ';': a field of k bytes holds up to (k + 1) / 2, a slab up to (F + n_rows) / 2 <=
//                    n_bytes / 2 entries + 1 closing, against max_bytes / 2 + max_rows + 66: fits
//   GFF    item_off[GFF_ITEM_OFF] (an item's byte offset): "=,,,," is an item a byte: up to F items + 1 entry, against the same size: checked
//   GTF    (max_bytes = n_bytes; F as for GFF: the eight columns in front of the ninth field are the same)
//   GTF    values[0]: key bytes, values[1]: value bytes; both are parts of the field as they stand, and a key and its value never
//                    share a byte: <= F together: fits
//   GTF    item_off[GTF_KEY_OFF], [GTF_VALUE_OFF] (an entry's key offset and value offset): the shortest entry is three bytes ("k v": a key byte, a
//                    space, a value byte; a quoted one has four) and all but a row's last are followed by a ';': a field of k
//                    bytes holds up to (k + 1) / 4, a slab up to (F + n_rows) / 4 <= n_bytes / 4 entries + 1 closing, against
//                    max_bytes / 2 + max_rows + 66: fits
//          No GTF buffer is "checked".  exon_text_gtf still passes its totals through fits() and k_gtf_attr_fill bounds its writes:
//          the derivation above is then not the only thing between a slab and the end of a buffer.
//   BED    values[0] (max_bytes = n_bytes): the name fields, disjoint parts of the text: <= n_bytes: fits.  No BED buffer is "checked":
//          the name bytes of a slab cannot exceed the slab.  k_bed_name_fill bounds its reads and writes all the same.
//   take-rows (take_rows.hip: the kept rows of the columns above as columns of their own, in a scratch of ITS own that every call
//          sizes from the inputs it is given; K kept rows of n_rows, a node of `length` elements and `n_values` bytes)
//   take   rows[K], K <= n_rows indices, against n_rows + 64: fits.  A fixed column's K values / K bits against n_rows values + 64 bytes /
//                    n_rows / 8 + 64 bytes: fits
//   take   a node's lengths [k], offsets [k + 1], validity bits [k] for the k <= length elements its rows list names (the rows list of a
//                    LIST's child is the kept rows' items: no more than the items there are), against length + 64, length + 65 entries,
//                    length / 8 + 64 bytes: fits
//   take   a UTF8 node's bytes: spans of the kept elements, disjoint parts of the input's n_values bytes, against n_values + 64: fits
//   take   a LIST's item-index list: the kept rows' item ranges, disjoint ranges of the child's `length` items, against length + 64: fits
//   take   a LIST's INT64 items (BAM / SAM quality_score; no index list): the kept rows' spans, disjoint ranges of the leaf's `length` 8-byte
//                    items, against length + 8 items: fits
//          No take buffer is "checked": a compacted buffer is never larger than its input.  The kernels bound every index and every
//          write all the same.
static int scratch_for(exon_hip_ctx* ctx, ExonTextScratch** sp, int64_t max_rows, int64_t max_bytes, TextLayout lay) {
  ExonTextScratch* s = *sp;
  if (s && s->layout == lay && s->max_rows >= max_rows && s->max_bytes >= max_bytes) return EXON_HIP_OK;
  delete s;
  *sp = nullptr;
  s = new (std::nothrow) ExonTextScratch(ctx);
  if (!s) return fail(ctx, EXON_HIP_ENOMEM, "out of host memory");
  s->max_rows = max_rows;
  s->max_bytes = max_bytes;
  s->layout = lay;
  hipSetDevice(ctx->device);
  PoolBufs& b = s->bufs;
  const size_t r = (size_t)max_rows + 64;
  s->value_cap = (size_t)max_bytes;
  s->item_cap = (size_t)max_bytes / 2 + r + 2;
  for (int k = 0; k < lay.cols; ++k) {
    s->len[k] = b.take<uint32_t>(r * 4);
    s->off[k] = b.take<int32_t>((r + 1) * 4);
  }
  for (int k = 0; k < lay.pools; ++k) s->values[k] = b.take<uint8_t>((size_t)max_bytes + 64);
  for (int k = 0; k < lay.item_offs; ++k) s->item_off[k] = b.take<int32_t>(s->item_cap * 4);
  for (int k = 0; k < lay.valids; ++k) s->valid[k] = b.take<uint32_t>(r / 8 + 64);
  if (lay.field_words) s->field = b.take<uint32_t>((size_t)lay.field_words * r * 4);
  s->sums = b.take<unsigned>((r / TPB + 4) * 4);
  s->res = b.take<unsigned>(RES_WORDS * 4);
  s->h_res = b.pinned<unsigned>(RES_WORDS * 4);
  if (b.status() != hipSuccess) {
    (void)hipGetLastError();
    delete s;
    return fail(ctx, EXON_HIP_ENOMEM, "buffers for the string columns of a slab (%lld rows, %lld bytes)", (long long)max_rows, (long long)max_bytes);
  }
  *sp = s;
  return EXON_HIP_OK;
}

// room for `items` quality scores (kept between slabs, grown to at least 1 Mi items)
static int qual_for(exon_hip_ctx* ctx, ExonTextScratch* s, unsigned items) {
  if (s->qual_cap >= (size_t)items) return EXON_HIP_OK;
  s->qual_bufs.release();
  s->qual_cap = std::max<size_t>((size_t)items, (size_t)1 << 20);
  s->qual = s->qual_bufs.take<int64_t>(s->qual_cap * 8);
  if (!s->qual) {
    s->qual_cap = 0;
    s->qual_bufs.release();
    return fail(ctx, EXON_HIP_ENOMEM, "quality_scores of a slab (%u items)", items);
  }
  return EXON_HIP_OK;
}

// the totals the measure kernels have brought back against what the fill kernel's buffers hold: `bytes` into a values buffer,
// `items` (+ the closing entry) into an item-offsets buffer.  false: the fill is not launched, the slab is the host reader's
static bool fits(const ExonTextScratch* s, std::initializer_list<unsigned> bytes, std::initializer_list<unsigned> items = {}) {
  for (unsigned b : bytes)
    if ((size_t)b > s->value_cap) return false;
  for (unsigned i : items)
    if ((size_t)i + 1 > s->item_cap) return false;
  return true;
}

// lengths -> offsets (n + 1 of them); the total -> *total
static void scan_lengths_with(hipStream_t hs, unsigned* sums, const uint32_t* len, unsigned n, int32_t* offsets, unsigned* total) {
  const int nb = (int)((n + LIST_TPB - 1) / LIST_TPB);
  launch_list_scan(hs, len, nullptr, n, nb, sums, total);
  hipLaunchKernelGGL(k_write_offsets, dim3(nb), dim3(LIST_TPB), 0, hs, len, n, sums, offsets);
}
static void scan_lengths(hipStream_t hs, ExonTextScratch* s, const uint32_t* len, unsigned n, int32_t* offsets, unsigned* total) {
  scan_lengths_with(hs, s->sums, len, n, offsets, total);  // (sums: a word per 256 rows; the `formats` scans bring block sums of their own)
}

// One builder's run.  text_begin is every builder's prologue: a scratch of the format's layout for the slab, the stream, the launch
// shape, the result block cleared (the measure kernels count undecided rows into it)
struct TextRun {
  ExonTextScratch* s;
  hipStream_t hs;
  unsigned n;  // rows
  int nb;      // blocks of TPB rows
};
static int text_begin(exon_hip_ctx* ctx, void* stream, ExonTextScratch** sp, int64_t n_rows, int64_t max_bytes, TextLayout lay, TextRun* t) {
  if (int rc = scratch_for(ctx, sp, std::max<int64_t>(n_rows, 1 << 16), std::max<int64_t>(max_bytes, 1 << 20), lay)) return rc;
  *t = TextRun{*sp, pick_stream(ctx, stream), (unsigned)n_rows, (int)(((unsigned)n_rows + TPB - 1) / TPB)};
  HIP_TRY(ctx, hipMemsetAsync(t->s->res, 0, RES_WORDS * 4, t->hs));
  return EXON_HIP_OK;
}
// len[0 .. k) -> off[0 .. k), their totals -> res[0 .. k)
static void scan_cols(const TextRun& t, int k) {
  for (int i = 0; i < k; ++i) scan_lengths(t.hs, t.s, t.s->len[i], t.n, t.s->off[i], t.s->res + i);
}
// every builder's middle: the k scans, the result block back in its pinned mirror h_res, the stream drained; the rows the measure
// kernel has counted undecided -> *undecided
static int text_totals(exon_hip_ctx* ctx, const TextRun& t, int k, int64_t* undecided = nullptr) {
  scan_cols(t, k);
  HIP_TRY(ctx, hipMemcpyAsync(t.s->h_res, t.s->res, RES_WORDS * 4, hipMemcpyDeviceToHost, t.hs));
  HIP_TRY(ctx, hipStreamSynchronize(t.hs));
  if (undecided) *undecided = t.s->h_res[RES_UNDECIDED];
  return EXON_HIP_OK;
}
// every builder's last line: a column that found no room in `out` is an error, never a column less
static int text_done(exon_hip_ctx* ctx, const ExonTextColumns* out) {
  return out->overflow ? fail(ctx, EXON_HIP_ESTATE, "more device-built text columns than ExonTextColumns holds") : EXON_HIP_OK;
}

// room for the `info` column of a slab of `rows` rows (bytes == 0) or for its `bytes` printed bytes: kept between slabs, the values
// at least 1 MiB.  false: no memory (the caller hands the slab over)
static bool info_for(ExonTextScratch* s, size_t rows, size_t bytes) {
  if (bytes == 0 && s->info_rows < rows) {
    s->info_row_bufs.release();
    s->info_rows = 0;
    const size_t r = rows + 64;
    PoolBufs& b = s->info_row_bufs;
    s->info_field_off = b.take<uint32_t>(r * 4);
    s->info_field_len = b.take<uint32_t>(r * 4);
    s->info_len = b.take<uint32_t>(r * 4);
    s->info_off = b.take<int32_t>((r + 1) * 4);
    s->info_scal = b.take<unsigned>(16);
    s->h_info_scal = b.pinned<unsigned>(16);
    if (b.status() != hipSuccess) {
      (void)hipGetLastError();
      b.release();
      return false;
    }
    s->info_rows = rows;
  }
  if (bytes > s->info_cap) {
    s->info_value_bufs.release();
    s->info_cap = 0;
    const size_t cap = std::max<size_t>(bytes + bytes / 4, (size_t)1 << 20);
    s->info_values = s->info_value_bufs.take<uint8_t>(cap + 64);
    if (!s->info_values) {
      (void)hipGetLastError();
      s->info_value_bufs.release();
      return false;
    }
    s->info_cap = cap;
  }
  return true;
}

// room for the `formats` column, each part kept between slabs and grown on demand: for a slab of `rows` rows in `bytes` aligned
// bytes (tabs == 0 and value_bytes == 0), for its `tabs` tabs, for its `value_bytes` printed bytes (at least 1 MiB).  false: no
// memory (the caller hands the slab over)
static bool fmt_for(ExonTextScratch* s, size_t rows, size_t bytes, size_t tabs, size_t value_bytes) {
  const size_t chunks = (bytes + FMT_CHUNK - 1) / FMT_CHUNK;
  if (rows && (s->fmt_rows < rows || s->fmt_chunks < chunks)) {
    PoolBufs& b = s->fmt_slab_bufs;
    const size_t r = std::max(rows, s->fmt_rows) + 64, c = std::max(chunks, s->fmt_chunks) + 64;
    b.release();
    s->fmt_rows = s->fmt_chunks = 0;
    s->fmt_tab_bufs.release();  // (the items' buffers are sized for fmt_rows + fmt_tabs items: they are made again for the new rows)
    s->fmt_tabs = 0;
    s->fmt_cnt = b.take<uint32_t>(c * 4);
    s->fmt_chunk_first = b.take<int32_t>((c + 1) * 4);
    s->fmt_chunk_sums = b.take<unsigned>((c / LIST_TPB + 4) * 4);
    s->fmt_first_tab = b.take<uint32_t>(r * 4);
    s->fmt_row_off = b.take<int32_t>((r + 1) * 4);
    s->fmt_types = b.take<unsigned long long>(r * 8);
    s->fmt_scal = b.take<unsigned>(32);
    s->h_fmt_scal = b.pinned<unsigned>(32);
    if (b.status() != hipSuccess) {
      (void)hipGetLastError();
      b.release();
      return false;
    }
    s->fmt_rows = r - 64;
    s->fmt_chunks = c - 64;
  }
  if (tabs > s->fmt_tabs) {
    PoolBufs& b = s->fmt_tab_bufs;
    b.release();
    s->fmt_tabs = 0;
    const size_t t = std::max<size_t>(tabs + tabs / 4, (size_t)1 << 16), items = t + s->fmt_rows + 64;
    s->fmt_tab_pos = b.take<uint32_t>((t + 64) * 4);
    s->fmt_tab_row = b.take<uint32_t>((t + 64) * 4);
    s->fmt_item_len = b.take<uint32_t>(items * 4);
    s->fmt_item_off = b.take<int32_t>((items + 1) * 4);
    s->fmt_item_sums = b.take<unsigned>((items / LIST_TPB + 4) * 4);
    if (b.status() != hipSuccess) {
      (void)hipGetLastError();
      b.release();
      return false;
    }
    s->fmt_tabs = t;
  }
  if (value_bytes > s->fmt_cap) {
    s->fmt_value_bufs.release();
    s->fmt_cap = 0;
    const size_t cap = std::max<size_t>(value_bytes + value_bytes / 4, (size_t)1 << 20);
    s->fmt_values = s->fmt_value_bufs.take<uint8_t>(cap + 64);
    if (!s->fmt_values) {
      (void)hipGetLastError();
      s->fmt_value_bufs.release();
      return false;
    }
    s->fmt_cap = cap;
  }
  return true;
}

// the key types of a VCF header, flattened for the device: open addressing over a power of two of slots, at most half of them taken.
// keys: n names, each with its NUL, back to back; kinds: their n type characters (i f b c s).  The first line of a key wins, as
// in the host reader; the reserved keys of the specification follow with the types noodles falls back to (VcfKeyTypes::
// reserved_info, or ::reserved_format for the table of the FORMAT keys), unless the header has typed them.  (GT is no entry of
// the FORMAT table: the walk knows it by its name, whatever the header says.)
int exon_vcf_key_table_build(exon_hip_ctx* ctx, PoolBufs* bufs, const char* keys, const char* kinds, int32_t n, ExonVcfKeySeed seed, ExonVcfKeyTable* out) {
  // (the names of VcfKeyTypes::reserved_info's three lists and of ::reserved_format's two: those functions are the authority on their types)
  static const char* const reserved[] = {"AC", "AD", "ADF", "ADR", "AN", "DP", "END", "MQ0", "NS", "SB", "SVLEN", "CIPOS", "CIEND", "HOMLEN", "CILEN", "DPADJ",
                                         "CN", "CNADJ", "CICN", "CICNADJ", "AF", "BQ", "MQ", "DB", "H2", "H3", "SOMATIC", "VALIDATED", "1000G", "IMPRECISE", "NOVEL"};
  static const char* const reserved_format[] = {"AD", "ADF", "ADR", "DP", "EC", "GQ", "HQ", "MQ", "PL", "PP", "PQ", "PS", "CN", "NQ", "HAP", "AHAP", "GL", "GP", "CNQ", "CNL", "CNP"};
  const bool format = seed == ExonVcfKeySeed::Format;
  std::vector<std::pair<std::string, char>> entries;
  const char* p = keys;
  for (int32_t k = 0; k < n; ++k) {
    entries.emplace_back(std::string(p), kinds[k]);
    p += entries.back().first.size() + 1;
  }
  if (format)
    for (const char* r : reserved_format) entries.emplace_back(r, exon::VcfKeyTypes::reserved_format(r));
  else
    for (const char* r : reserved) entries.emplace_back(r, exon::VcfKeyTypes::reserved_info(r));
  size_t slots = 64;
  while (slots < 2 * entries.size()) slots *= 2;
  std::vector<uint64_t> hash(slots, 0);
  std::vector<uint32_t> off(slots, 0), len(slots, 0);
  std::vector<uint8_t> type(slots, 0);
  std::string text;
  for (const auto& e : entries) {
    const uint64_t h = vcf_key_hash(reinterpret_cast<const uint8_t*>(e.first.data()), (unsigned)e.first.size());
    size_t slot = (size_t)h & (slots - 1);
    bool known = false;
    for (; hash[slot]; slot = (slot + 1) & (slots - 1))
      if (hash[slot] == h && len[slot] == e.first.size() && text.compare(off[slot], len[slot], e.first) == 0) {
        known = true;  // (an earlier line of the key, or the header's type of a reserved key)
        break;
      }
    if (known) continue;
    hash[slot] = h;
    off[slot] = (uint32_t)text.size();
    len[slot] = (uint32_t)e.first.size();
    type[slot] = (uint8_t)e.second;
    text += e.first;
  }
  hipSetDevice(ctx->device);
  bufs->release();
  unsigned long long* d_hash = bufs->take<unsigned long long>(slots * 8);
  uint32_t* d_off = bufs->take<uint32_t>(slots * 4);
  uint32_t* d_len = bufs->take<uint32_t>(slots * 4);
  uint8_t* d_type = bufs->take<uint8_t>(slots);
  uint8_t* d_text = bufs->take<uint8_t>(text.size() + 16);
  bufs->upload(d_hash, hash.data(), slots * 8);
  bufs->upload(d_off, off.data(), slots * 4);
  bufs->upload(d_len, len.data(), slots * 4);
  bufs->upload(d_type, type.data(), slots);
  bufs->upload(d_text, text.data(), text.size());
  if (bufs->status() != hipSuccess) {
    const std::string msg = hipGetErrorString(bufs->status());
    (void)hipGetLastError();
    bufs->release();
    memset(out, 0, sizeof *out);
    return fail(ctx, EXON_HIP_ENOMEM, "the %s key types of a VCF header (%zu keys): %s", format ? "FORMAT" : "INFO", entries.size(), msg.c_str());
  }
  *out = ExonVcfKeyTable{d_hash, d_off, d_len, d_type, d_text, (unsigned)(slots - 1)};
  return EXON_HIP_OK;
}

int exon_text_vcf(exon_hip_ctx* ctx, void* stream, ExonTextScratch** sp, const uint8_t* d_text, int64_t n_bytes, const unsigned* d_nl, int64_t n_rows, uint64_t projection,
                  const ExonVcfKeyTable* info_keys, const ExonVcfKeyTable* format_keys, ExonTextColumns* out, int64_t* n_undecided) {
  *out = ExonTextColumns();
  *n_undecided = 0;
  const bool path3 = (projection & (EXON_HIP_PROJECT_VCF_ID | EXON_HIP_PROJECT_VCF_REF | EXON_HIP_PROJECT_VCF_ALT)) != 0;
  const bool info = (projection & EXON_HIP_PROJECT_VCF_INFO) != 0;
  // (bit 16 without the modifier is the host reader's column: nothing is built for it here)
  const bool formats = (projection & EXON_HIP_PROJECT_VCF_FORMATS) && (projection & EXON_HIP_PROJECT_VCF_FORMATS_ON_DEVICE);
  if (n_rows == 0 || !(path3 || info || formats)) return EXON_HIP_OK;
  if (info && (!info_keys || !info_keys->hash)) return fail(ctx, EXON_HIP_ESTATE, "the VCF info column needs the header's key types (exon_hip_vcf_parser_set_key_types)");
  if (formats && (!format_keys || !format_keys->hash))
    return fail(ctx, EXON_HIP_ESTATE, "the VCF formats column needs the header's FORMAT key types (exon_hip_vcf_parser_set_format_key_types)");
  const unsigned skip = (unsigned)(reinterpret_cast<uintptr_t>(d_text) & 15);
  d_text -= skip;
  n_bytes += skip;
  TextRun t;
  if (int rc = text_begin(ctx, stream, sp, n_rows, n_bytes, LAYOUT_VCF, &t)) return rc;
  ExonTextScratch* s = t.s;
  VcfLens L{s->len[0], s->len[1], s->len[2], s->field, s->field + 3 * ((size_t)s->max_rows + 64)};
  unsigned n_tabs = 0, n_items = 0;
  if (formats) {  // the tab index first: its size comes back before the buffers behind it are made
    const unsigned n_total = (unsigned)n_bytes, n_chunks = (unsigned)(((size_t)n_bytes + FMT_CHUNK - 1) / FMT_CHUNK);
    const int cb = (int)((n_chunks + TPB - 1) / TPB);
    if (!fmt_for(s, (size_t)std::max<int64_t>(n_rows, 1 << 16), (size_t)std::max<int64_t>(n_bytes, 1 << 20), 0, 0))
      return fail(ctx, EXON_HIP_ENOMEM, "buffers for the formats column of a slab (%lld rows, %lld bytes)", (long long)n_rows, (long long)n_bytes);
    HIP_TRY(ctx, hipMemsetAsync(s->fmt_scal, 0, 32, t.hs));
    hipLaunchKernelGGL(k_fmt_tab_count, dim3(cb), dim3(TPB), 0, t.hs, d_text, d_nl, t.n, skip, n_total, n_chunks, s->fmt_cnt);
    scan_lengths_with(t.hs, s->fmt_chunk_sums, s->fmt_cnt, n_chunks, s->fmt_chunk_first, s->fmt_scal + 4);
    HIP_TRY(ctx, hipMemcpyAsync(s->h_fmt_scal, s->fmt_scal, 32, hipMemcpyDeviceToHost, t.hs));
    HIP_TRY(ctx, hipStreamSynchronize(t.hs));
    n_tabs = s->h_fmt_scal[4];
    // no tab at all: no row has eight fields; rows + tabs beyond int32: the items' scan has no room; no memory: all the host reader's
    if (n_tabs == 0 || (uint64_t)n_tabs + (uint64_t)t.n > (uint64_t)INT32_MAX || !fmt_for(s, 0, 0, n_tabs, 0)) {
      *n_undecided = n_rows;
      return EXON_HIP_OK;
    }
    n_items = n_tabs + t.n;
    const int tb = (int)((n_tabs + TPB - 1) / TPB);
    hipLaunchKernelGGL(k_fmt_tab_fill, dim3(cb), dim3(TPB), 0, t.hs, d_text, d_nl, t.n, skip, n_total, n_chunks, s->fmt_chunk_first, s->fmt_tab_pos,
                       (unsigned)std::min<size_t>(s->fmt_tabs, 0xFFFFFFFFu));
    hipLaunchKernelGGL(k_fmt_rows, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, d_nl, t.n, skip, *format_keys, s->fmt_tab_pos, n_tabs, s->fmt_first_tab, s->fmt_types, s->fmt_item_len,
                       s->fmt_scal);
    hipLaunchKernelGGL(k_fmt_sample_measure, dim3(tb), dim3(TPB), 0, t.hs, d_text, d_nl, t.n, skip, s->fmt_tab_pos, n_tabs, s->fmt_first_tab, s->fmt_types, s->fmt_tab_row,
                       s->fmt_item_len, s->fmt_scal);
    scan_lengths_with(t.hs, s->fmt_item_sums, s->fmt_item_len, n_items, s->fmt_item_off, s->fmt_scal + 3);
    HIP_TRY(ctx, hipMemcpyAsync(s->h_fmt_scal, s->fmt_scal, 32, hipMemcpyDeviceToHost, t.hs));
  }
  if (info) {
    if (!info_for(s, (size_t)std::max<int64_t>(n_rows, 1 << 16), 0)) return fail(ctx, EXON_HIP_ENOMEM, "buffers for the info column of a slab (%lld rows)", (long long)n_rows);
    HIP_TRY(ctx, hipMemsetAsync(s->info_scal, 0, 16, t.hs));
    hipLaunchKernelGGL(k_vcf_info_measure, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, d_nl, t.n, skip, *info_keys, s->info_field_off, s->info_field_len, s->info_len, s->info_scal);
    scan_lengths(t.hs, s, s->info_len, t.n, s->info_off, s->res + 3);
    HIP_TRY(ctx, hipMemcpyAsync(s->h_info_scal, s->info_scal, 16, hipMemcpyDeviceToHost, t.hs));
  }
  if (path3) hipLaunchKernelGGL(k_vcf_measure, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, d_nl, t.n, skip, L, s->valid[0], s->valid[1]);
  if (int rc = text_totals(ctx, t, path3 ? 3 : 0)) return rc;  // ID: list offsets, ID: byte offsets of every row's items, REF
  uint64_t info_bytes = 0;
  if (info) {
    if (s->h_info_scal[2]) {  // rows the host reader must print, or refuse
      *n_undecided = s->h_info_scal[2];
      return EXON_HIP_OK;
    }
    info_bytes = (uint64_t)s->h_info_scal[0] | (uint64_t)s->h_info_scal[1] << 32;
    if (info_bytes > (uint64_t)INT32_MAX || !info_for(s, 0, (size_t)std::max<uint64_t>(info_bytes, 1))) {  // int32 offsets; no buffer of that size
      *n_undecided = n_rows;
      return EXON_HIP_OK;
    }
  }
  uint64_t fmt_bytes = 0;
  if (formats) {
    if (s->h_fmt_scal[2]) {  // rows (or samples of rows) the host reader must print, or refuse
      *n_undecided = s->h_fmt_scal[2];
      return EXON_HIP_OK;
    }
    fmt_bytes = (uint64_t)s->h_fmt_scal[0] | (uint64_t)s->h_fmt_scal[1] << 32;
    if (fmt_bytes > (uint64_t)INT32_MAX || !fmt_for(s, 0, 0, 0, (size_t)std::max<uint64_t>(fmt_bytes, 1))) {  // int32 offsets; no buffer of that size
      *n_undecided = n_rows;
      return EXON_HIP_OK;
    }
  }
  const unsigned id_items = path3 ? s->h_res[0] : 0u, id_bytes = path3 ? s->h_res[1] : 0u, ref_bytes = path3 ? s->h_res[2] : 0u;
  if (path3 && !fits(s, {id_bytes, ref_bytes}, {id_items})) {  // (IDs of many empty items)
    *n_undecided = n_rows;
    return EXON_HIP_OK;
  }
  if (formats) {
    const unsigned cap = (unsigned)std::min<size_t>(s->fmt_cap, 0xFFFFFFFFu);
    hipLaunchKernelGGL(k_fmt_head_fill, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, t.n, s->fmt_tab_pos, n_tabs, s->fmt_first_tab, s->fmt_item_off, s->fmt_row_off, s->fmt_values, cap,
                       (unsigned)n_bytes);
    hipLaunchKernelGGL(k_fmt_sample_fill, dim3((n_tabs + TPB - 1) / TPB), dim3(TPB), 0, t.hs, d_text, d_nl, skip, s->fmt_tab_pos, n_tabs, s->fmt_first_tab, s->fmt_types,
                       s->fmt_tab_row, s->fmt_item_off, s->fmt_values, cap);
  }
  if (path3) {
    hipLaunchKernelGGL(k_vcf_fill, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, t.n, L, s->off[0], s->off[1], s->off[2], s->item_off[VCF_ID_ITEMS], s->values[0], s->values[2], id_items,
                       id_bytes);
    if (id_items == 0) HIP_TRY(ctx, hipMemsetAsync(s->item_off[VCF_ID_ITEMS], 0, 4, t.hs));
  }
  if (info)
    hipLaunchKernelGGL(k_vcf_info_fill, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, t.n, *info_keys, s->info_field_off, s->info_field_len, s->info_off, s->info_values,
                       (unsigned)std::min<size_t>(s->info_cap, 0xFFFFFFFFu));
  HIP_TRY(ctx, hipGetLastError());
  if (projection & EXON_HIP_PROJECT_VCF_ID) out->root(out->list_utf8(t.n, s->off[0], s->valid[0], id_items, s->item_off[VCF_ID_ITEMS], s->values[0], id_bytes));
  if (projection & EXON_HIP_PROJECT_VCF_REF) out->root(out->utf8(t.n, s->off[2], nullptr, s->values[2], ref_bytes));
  if (projection & EXON_HIP_PROJECT_VCF_ALT) out->root(out->list_utf8(t.n, nullptr, s->valid[1], 0, nullptr, nullptr, 0));  // (no items: the note at the top)
  if (info) out->root(out->utf8(t.n, s->info_off, nullptr, s->info_values, (int64_t)info_bytes));
  if (formats) out->root(out->utf8(t.n, s->fmt_row_off, nullptr, s->fmt_values, (int64_t)fmt_bytes));
  return text_done(ctx, out);
}

// name, cigar, sequence, quality_scores of BAM records or SAM lines, as projected; qual_off: the list offsets of quality_scores
static void bam_columns(ExonTextColumns* out, const TextRun& t, uint64_t projection, const int32_t* qual_off, unsigned qual_items) {
  const ExonTextScratch* s = t.s;
  if (projection & EXON_HIP_PROJECT_BAM_NAME) out->root(out->utf8(t.n, s->off[0], s->valid[0], s->values[0], s->h_res[0]));
  if (projection & EXON_HIP_PROJECT_BAM_CIGAR) out->root(out->utf8(t.n, s->off[1], nullptr, s->values[1], s->h_res[1]));
  if (projection & EXON_HIP_PROJECT_BAM_SEQUENCE) out->root(out->utf8(t.n, s->off[2], nullptr, s->values[2], s->h_res[2]));
  if (projection & EXON_HIP_PROJECT_BAM_QUALITY_SCORES) out->root(out->list(t.n, qual_off, nullptr, out->int64s(s->qual, qual_items)));
}
constexpr uint64_t BAM_TEXT = EXON_HIP_PROJECT_BAM_NAME | EXON_HIP_PROJECT_BAM_CIGAR | EXON_HIP_PROJECT_BAM_SEQUENCE | EXON_HIP_PROJECT_BAM_QUALITY_SCORES;

int exon_text_bam(exon_hip_ctx* ctx, void* stream, ExonTextScratch** sp, const uint8_t* d_data, int64_t n_bytes, const uint32_t* d_rec_of_row, int64_t n_rows, uint64_t projection,
                  ExonTextColumns* out, int64_t* n_undecided) {
  *out = ExonTextColumns();
  *n_undecided = 0;
  if (n_rows == 0 || !(projection & BAM_TEXT)) return EXON_HIP_OK;
  TextRun t;
  if (int rc = text_begin(ctx, stream, sp, n_rows, 2 * n_bytes, LAYOUT_BAM, &t)) return rc;  // (a sequence doubles its 4-bit codes)
  ExonTextScratch* s = t.s;
  BamLens L{s->len[0], s->len[1], s->len[2]};
  hipLaunchKernelGGL(k_bam_measure, dim3(t.nb), dim3(TPB), 0, t.hs, d_data, d_rec_of_row, t.n, L, s->valid[0]);
  if (int rc = text_totals(ctx, t, 3)) return rc;
  const unsigned name_bytes = s->h_res[0], cigar_bytes = s->h_res[1], seq_bytes = s->h_res[2];
  if (!fits(s, {name_bytes, cigar_bytes, seq_bytes})) {  // (CIGARs of long ops: up to ten characters out of four bytes)
    *n_undecided = n_rows;
    return EXON_HIP_OK;
  }
  if (projection & EXON_HIP_PROJECT_BAM_QUALITY_SCORES)
    if (int rc = qual_for(ctx, s, seq_bytes)) return rc;
  hipLaunchKernelGGL(k_bam_fill, dim3(t.nb), dim3(TPB), 0, t.hs, d_data, d_rec_of_row, t.n, projection, s->off[0], s->off[1], s->off[2], s->values[0], s->values[1], s->values[2],
                     s->qual);
  HIP_TRY(ctx, hipGetLastError());
  bam_columns(out, t, projection, s->off[2], seq_bytes);  // (a BAM record's qualities are as many as its bases)
  return text_done(ctx, out);
}

int exon_text_fastq(exon_hip_ctx* ctx, void* stream, ExonTextScratch** sp, const exon_hip_fastq_views* v, int64_t n_bytes, ExonTextColumns* out) {
  *out = ExonTextColumns();
  if (v->n_reads == 0) return EXON_HIP_OK;
  TextRun t;
  if (int rc = text_begin(ctx, stream, sp, v->n_reads, n_bytes, LAYOUT_FASTQ, &t)) return rc;
  ExonTextScratch* s = t.s;
  FastqLens L{s->len[0], s->len[1], s->len[2], s->len[3]};
  hipLaunchKernelGGL(k_fastq_measure, dim3(t.nb), dim3(TPB), 0, t.hs, v->text_base, t.n, v->head_start, v->head_end, v->seq_start, v->seq_end, v->qual_start, v->qual_end, L,
                     s->valid[0]);
  scan_cols(t, 4);  // (nothing to check: the fill goes in front of the totals' way back, the text is read when this returns)
  hipLaunchKernelGGL(k_fastq_fill, dim3(t.nb), dim3(TPB), 0, t.hs, v->text_base, t.n, v->head_start, v->seq_start, v->qual_start, s->off[0], s->off[1], s->off[2], s->off[3],
                     s->values[0], s->values[1], s->values[2], s->values[3]);
  HIP_TRY(ctx, hipGetLastError());
  if (int rc = text_totals(ctx, t, 0)) return rc;
  for (int k = 0; k < 4; ++k) out->root(out->utf8(t.n, s->off[k], k == 1 ? s->valid[0] : nullptr, s->values[k], s->h_res[k]));
  return text_done(ctx, out);
}

int exon_text_fasta(exon_hip_ctx* ctx, void* stream, ExonTextScratch** sp, const exon_hip_fasta_views* v, ExonTextColumns* out) {
  *out = ExonTextColumns();
  if (v->n_records == 0) return EXON_HIP_OK;
  TextRun t;
  if (int rc = text_begin(ctx, stream, sp, v->n_records, v->text_bytes + 16, LAYOUT_FASTA, &t)) return rc;
  ExonTextScratch* s = t.s;
  const unsigned cap = (unsigned)std::min<size_t>(s->value_cap, 0xFFFFFFFFu), n_total = (unsigned)v->text_bytes;
  hipLaunchKernelGGL(k_fasta_measure, dim3(t.nb), dim3(TPB), 0, t.hs, v->text_base, t.n, v->head_start, v->head_end, s->len[0], s->len[1], s->valid[0]);
  scan_cols(t, 2);  // (as for FASTQ: the fills go in front of the totals' way back, the text is read when this returns)
  hipLaunchKernelGGL(k_fasta_head_fill, dim3(t.nb), dim3(TPB), 0, t.hs, v->text_base, n_total, t.n, v->head_start, v->head_end, s->off[0], s->off[1], s->values[0], s->values[1], cap);
  const uint64_t fill_threads = (uint64_t)v->n_lines * FASTA_LPL;
  hipLaunchKernelGGL(k_fasta_seq_fill, dim3((unsigned)((fill_threads + TPB - 1) / TPB)), dim3(TPB), 0, t.hs, v->text_base, n_total, (unsigned)v->first_line_start, v->line_end,
                     v->line_dst, (unsigned)v->n_lines, s->values[2], (unsigned)v->seq_bytes, cap);
  HIP_TRY(ctx, hipGetLastError());
  if (int rc = text_totals(ctx, t, 0)) return rc;
  if (!fits(s, {s->h_res[0], s->h_res[1], (unsigned)v->seq_bytes})) return fail(ctx, EXON_HIP_ESTATE, "FASTA columns of %u + %u + %lld bytes in a slab of %lld", s->h_res[0], s->h_res[1], (long long)v->seq_bytes, (long long)v->text_bytes);  // (never: the table above scratch_for)
  out->root(out->utf8(t.n, s->off[0], nullptr, s->values[0], s->h_res[0]));
  out->root(out->utf8(t.n, s->off[1], s->valid[0], s->values[1], s->h_res[1]));
  out->root(out->utf8(t.n, v->seq_offsets, nullptr, s->values[2], v->seq_bytes));
  return text_done(ctx, out);
}

int exon_text_bed(exon_hip_ctx* ctx, void* stream, ExonTextScratch** sp, const uint8_t* d_text, int64_t n_bytes, const uint32_t* d_name_off, const uint32_t* d_name_len,
                  const uint8_t* d_name_valid, int64_t n_rows, ExonTextColumns* out) {
  *out = ExonTextColumns();
  if (n_rows == 0) return EXON_HIP_OK;
  TextRun t;
  if (int rc = text_begin(ctx, stream, sp, n_rows, n_bytes, LAYOUT_BED, &t)) return rc;
  ExonTextScratch* s = t.s;
  scan_lengths(t.hs, s, d_name_len, t.n, s->off[0], s->res);
  hipLaunchKernelGGL(k_bed_name_fill, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, (unsigned)n_bytes, t.n, d_name_off, s->off[0], s->values[0], (unsigned)std::min<size_t>(s->value_cap, 0xFFFFFFFFu));
  HIP_TRY(ctx, hipGetLastError());
  if (int rc = text_totals(ctx, t, 0)) return rc;
  if (!fits(s, {s->h_res[0]})) return fail(ctx, EXON_HIP_ESTATE, "BED names of %u bytes in a slab of %lld", s->h_res[0], (long long)n_bytes);  // (never: the table above scratch_for)
  out->root(out->utf8(t.n, s->off[0], d_name_valid, s->values[0], s->h_res[0]));
  return text_done(ctx, out);
}

// SAM lines -> the BAM text columns (quality_scores has list offsets of its own here: QUAL may be '*' next to a SEQ)
int exon_text_sam(exon_hip_ctx* ctx, void* stream, ExonTextScratch** sp, const uint8_t* d_text, int64_t n_bytes, const unsigned* d_nl, int64_t n_rows, uint64_t projection,
                  ExonTextColumns* out, int64_t* n_undecided) {
  *out = ExonTextColumns();
  *n_undecided = 0;
  if (n_rows == 0 || !(projection & BAM_TEXT)) return EXON_HIP_OK;
  const unsigned skip = (unsigned)(reinterpret_cast<uintptr_t>(d_text) & 15);
  d_text -= skip;
  n_bytes += skip;
  TextRun t;
  if (int rc = text_begin(ctx, stream, sp, n_rows, n_bytes, LAYOUT_SAM, &t)) return rc;
  ExonTextScratch* s = t.s;
  SamLens L{s->len[0], s->len[1], s->len[2], s->len[3], s->field};
  hipLaunchKernelGGL(k_sam_measure, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, d_nl, t.n, skip, L, s->valid[0], s->res + RES_UNDECIDED);
  if (int rc = text_totals(ctx, t, 4, n_undecided)) return rc;
  if (*n_undecided) return EXON_HIP_OK;
  const unsigned qual_items = s->h_res[3];
  if (projection & EXON_HIP_PROJECT_BAM_QUALITY_SCORES)
    if (int rc = qual_for(ctx, s, qual_items)) return rc;
  hipLaunchKernelGGL(k_sam_fill, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, t.n, L, projection, s->off[0], s->off[1], s->off[2], s->off[3], s->values[0], s->values[1], s->values[2],
                     s->qual);
  HIP_TRY(ctx, hipGetLastError());
  bam_columns(out, t, projection, s->off[3], qual_items);
  return text_done(ctx, out);
}

int exon_text_bcf(exon_hip_ctx* ctx, void* stream, ExonTextScratch** sp, const uint8_t* d_data, int64_t n_bytes, const uint32_t* d_rec_of_row, int64_t n_rows, uint64_t projection,
                  ExonTextColumns* out, int64_t* n_undecided) {
  *out = ExonTextColumns();
  *n_undecided = 0;
  if (n_rows == 0 || !(projection & (EXON_HIP_PROJECT_VCF_ID | EXON_HIP_PROJECT_VCF_REF | EXON_HIP_PROJECT_VCF_ALT))) return EXON_HIP_OK;
  TextRun t;
  if (int rc = text_begin(ctx, stream, sp, n_rows, n_bytes, LAYOUT_BCF, &t)) return rc;
  ExonTextScratch* s = t.s;
  BcfLens L{s->len[0], s->len[1], s->len[2], s->len[3], s->len[4]};
  hipLaunchKernelGGL(k_bcf_measure, dim3(t.nb), dim3(TPB), 0, t.hs, d_data, d_rec_of_row, t.n, L, s->res + RES_UNDECIDED);
  if (int rc = text_totals(ctx, t, 5, n_undecided)) return rc;
  if (*n_undecided) return EXON_HIP_OK;
  const unsigned id_items = s->h_res[0], id_bytes = s->h_res[1], ref_bytes = s->h_res[2], alt_items = s->h_res[3], alt_bytes = s->h_res[4];
  if (!fits(s, {id_bytes, ref_bytes, alt_bytes}, {id_items, alt_items})) {  // (IDs of many empty items, empty alleles)
    *n_undecided = n_rows;
    return EXON_HIP_OK;
  }
  int32_t *id_item_off = s->item_off[BCF_ID_ITEMS], *alt_item_off = s->item_off[BCF_ALT_ITEMS];
  hipLaunchKernelGGL(k_bcf_fill, dim3(t.nb), dim3(TPB), 0, t.hs, d_data, d_rec_of_row, t.n, projection, s->off[0], s->off[1], s->off[2], s->off[3], s->off[4], id_item_off, alt_item_off,
                     s->values[0], s->values[1], s->values[2], id_items, id_bytes, alt_items, alt_bytes);
  if (id_items == 0) HIP_TRY(ctx, hipMemsetAsync(id_item_off, 0, 4, t.hs));
  if (alt_items == 0) HIP_TRY(ctx, hipMemsetAsync(alt_item_off, 0, 4, t.hs));
  HIP_TRY(ctx, hipGetLastError());
  if (projection & EXON_HIP_PROJECT_VCF_ID) out->root(out->list_utf8(t.n, s->off[0], nullptr, id_items, id_item_off, s->values[0], id_bytes));
  if (projection & EXON_HIP_PROJECT_VCF_REF) out->root(out->utf8(t.n, s->off[2], nullptr, s->values[1], ref_bytes));
  if (projection & EXON_HIP_PROJECT_VCF_ALT) out->root(out->list_utf8(t.n, s->off[3], nullptr, alt_items, alt_item_off, s->values[2], alt_bytes));
  return text_done(ctx, out);
}

int exon_text_gff(exon_hip_ctx* ctx, void* stream, ExonTextScratch** sp, const uint8_t* d_text, int64_t n_bytes, const uint32_t* d_attr_off, const uint32_t* d_attr_len,
                  int64_t n_rows, ExonTextColumns* out, int64_t* n_undecided) {
  *out = ExonTextColumns();
  *n_undecided = 0;
  if (n_rows == 0) return EXON_HIP_OK;
  TextRun t;
  if (int rc = text_begin(ctx, stream, sp, n_rows, n_bytes, LAYOUT_GFF, &t)) return rc;
  ExonTextScratch* s = t.s;
  GffLens L{s->len[0], s->len[1], s->len[2], s->len[3]};
  hipLaunchKernelGGL(k_gff_attr_measure, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, d_attr_off, d_attr_len, t.n, L, s->res + RES_UNDECIDED);
  if (int rc = text_totals(ctx, t, 4, n_undecided)) return rc;  // entries (the map's offsets), items, key bytes, item bytes
  if (*n_undecided) return EXON_HIP_OK;
  const unsigned entries = s->h_res[0], items = s->h_res[1], key_bytes = s->h_res[2], item_bytes = s->h_res[3];
  if (!fits(s, {key_bytes, item_bytes}, {entries, items})) {  // (values that are mostly ',': an item a byte)
    *n_undecided = n_rows;
    return EXON_HIP_OK;
  }
  hipLaunchKernelGGL(k_gff_attr_fill, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, d_attr_off, d_attr_len, t.n, s->off[0], s->off[1], s->off[2], s->off[3], s->item_off[GFF_KEY_OFF],
                     s->item_off[GFF_LIST_OFF], s->item_off[GFF_ITEM_OFF], s->values[0], s->values[1], entries, items, key_bytes, item_bytes);
  HIP_TRY(ctx, hipGetLastError());
  const int keys = out->utf8(entries, s->item_off[GFF_KEY_OFF], nullptr, s->values[0], key_bytes);
  const int lists = out->list_utf8(entries, s->item_off[GFF_LIST_OFF], nullptr, items, s->item_off[GFF_ITEM_OFF], s->values[1], item_bytes);
  out->root(out->list(t.n, s->off[0], nullptr, out->struct2(entries, keys, lists)));
  return text_done(ctx, out);
}

int exon_text_gtf(exon_hip_ctx* ctx, void* stream, ExonTextScratch** sp, const uint8_t* d_text, int64_t n_bytes, const uint32_t* d_attr_off, const uint32_t* d_attr_len,
                  int64_t n_rows, ExonTextColumns* out, int64_t* n_undecided) {
  *out = ExonTextColumns();
  *n_undecided = 0;
  if (n_rows == 0) return EXON_HIP_OK;
  TextRun t;
  if (int rc = text_begin(ctx, stream, sp, n_rows, n_bytes, LAYOUT_GTF, &t)) return rc;
  ExonTextScratch* s = t.s;
  GtfLens L{s->len[0], s->len[1], s->len[2]};
  hipLaunchKernelGGL(k_gtf_attr_measure, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, d_attr_off, d_attr_len, t.n, L, s->res + RES_UNDECIDED);
  if (int rc = text_totals(ctx, t, 3, n_undecided)) return rc;  // entries (the map's offsets), key bytes, value bytes
  if (*n_undecided) return EXON_HIP_OK;
  const unsigned entries = s->h_res[0], key_bytes = s->h_res[1], value_bytes = s->h_res[2];
  if (!fits(s, {key_bytes, value_bytes}, {entries})) {  // (never, by the capacity table above scratch_for)
    *n_undecided = n_rows;
    return EXON_HIP_OK;
  }
  hipLaunchKernelGGL(k_gtf_attr_fill, dim3(t.nb), dim3(TPB), 0, t.hs, d_text, d_attr_off, d_attr_len, t.n, s->off[0], s->off[1], s->off[2], s->item_off[GTF_KEY_OFF],
                     s->item_off[GTF_VALUE_OFF], s->values[0], s->values[1], entries, key_bytes, value_bytes, (unsigned)std::min<size_t>(s->item_cap, 0xFFFFFFFFu),
                     (unsigned)std::min<size_t>(s->value_cap, 0xFFFFFFFFu));
  HIP_TRY(ctx, hipGetLastError());
  const int keys = out->utf8(entries, s->item_off[GTF_KEY_OFF], nullptr, s->values[0], key_bytes);
  const int values = out->utf8(entries, s->item_off[GTF_VALUE_OFF], nullptr, s->values[1], value_bytes);
  out->root(out->list(t.n, s->off[0], nullptr, out->struct2(entries, keys, values)));
  return text_done(ctx, out);
}
