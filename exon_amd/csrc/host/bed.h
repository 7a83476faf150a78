// bed.h -- BED records: the line rules, the device-layout array builder and the host reader.
//
// Counterpart of exon-bed (schema.rs:27-48: the twelve columns; batch_reader.rs:92-231: the read loop, which splits a line at
// every TAB and decodes it by its own field count; bed_record_builder.rs:203-250: what each RecordBuf<N> passes on;
// array_builder.rs:69-99: the appends) and of exon-core/src/datasources/bed/table_options.rs:34-45 (n_fields 3..12).  What the
// reference's code and fixtures fix is marked (ref), everything else is a DECISION of this library.  Columns of the device layout:
//   0 reference_sequence_name : i32 id into a dictionary built from the file (BED has no header), never NULL
//   1 start  2 end : i64, never NULL -- the operands of K2 (0, 1) and K6 / K7 (0, 1, 2), and the default columns
//   then, in bit order, what EXON_HIP_PROJECT_BED_* asks for (bit k = column k of the reference's schema):
//   3 name : Utf8?    4 score : i64?    5 strand : i32 id into ["+", "-"]?
//   6 thick_start  7 thick_end : i64?   8 color : Utf8?   9 block_count : i64?   10 block_sizes  11 block_starts : Utf8?
//     -- columns 6..11 are NULL on every row (ref: a 12-field line's fields 7..12 are dropped unread, batch_reader.rs:120-151)
//
// THE LINE RULES (the device parser, gpu_parse.hip's k_parse_bed_lines, agrees with them or hands the file over):
//   * a line ends at '\n'
//   * DECISION: one '\r' in front of the '\n' is dropped (the reference keeps it on Linux)
//   * a last line without '\n' is read whole.  KNOWN DIFFERENCE: the reference's `buf.pop()` (batch_reader.rs:107) would eat the
//     last byte of such a line; that is not reproduced
//   * (ref) a line that starts with '#' is no row (batch_reader.rs:98-104)
//   * (ref) every other line is split at every TAB and decoded by its own field count, whatever n_fields is:
//       3 fields: reference_sequence_name, start, end
//       4 fields: the same -- the name is read, but From<RecordBuf<4>> never passes it on: `name` is NULL
//       5 fields: plus name and score
//       6 and 12 fields: plus strand
//     an empty line (one field), a `track` or `browser` line and any other field count (1, 2, 7..11, 13 and more) is an error
//     that quotes the line (batch_reader.rs:220-225)
//   * every line is validated in full whatever is projected: a bad score is an error even when `score` is not a column
//   * start, end: usize::from_str of the text as it stands (no + 1): decimal digits, one leading '+' allowed
//       DECISION: 0 is a value like any other -- BED is 0-based.  KNOWN DIFFERENCE: the reference's
//       Position::from_str(..).unwrap() panics on it
//       DECISION: a value above i64::MAX is an error (the columns are Int64)
//       DECISION: end < start is accepted as it stands
//   * score: (ref) u16::from_str -- one leading '+', digits, at most 65535; '.', an empty field and 65536 are errors
//   * strand: (ref) '+', '-', or '.' -> NULL; anything else is an error (batch_reader.rs:132-146)
//   * name: (ref) the field's bytes as they stand: "." stays ".", an empty name stays ""; NULL on 3- and 4-field lines
//   * reference_sequence_name: the field's bytes as they stand
//   * UTF-8: (ref: read_line into a String) the whole line must be valid UTF-8, ignored fields included
// (ref) The reference has no region filter and no indexed table for BED: exon_hip_scan_open refuses `region` and `use_index`.
#pragma once
#include "gff.h"
#include "slab_export.h"

namespace exon {

struct BEDConfig {
  int64_t batch_size = DEFAULT_BATCH_SIZE;
  int threads = 0;            // decode threads: 0 = all host cores, 1 = sequential reader
  bool defer_decode = false;  // the caller will take the byte stream (GPU-side parsing): start no parse pipeline
  uint64_t projection = 0;    // EXON_HIP_PROJECT_BED_*: bits 3..11
};

struct BEDRecord {
  const char* chrom = nullptr;
  size_t chrom_len = 0;
  int64_t start = 0, end = 0;
  const char* name = nullptr;  // nullptr: NULL
  size_t name_len = 0;
  int64_t score = -1;   // -1: NULL
  int32_t strand = -1;  // -1: NULL
};

// digits (one leading '+' allowed) up to `max`: Rust's unsigned from_str with the column's range on top
inline bool bed_parse_uint(const char* p, size_t n, uint64_t max, int64_t* out) {
  if (n && p[0] == '+') ++p, --n;
  if (n == 0) return false;
  uint64_t v = 0;
  for (size_t i = 0; i < n; ++i) {
    const unsigned d = (unsigned)(unsigned char)p[i] - (unsigned)'0';
    if (d > 9u) return false;
    if (v > (max - d) / 10) return false;  // v * 10 + d would pass max
    v = v * 10 + d;
  }
  *out = (int64_t)v;
  return true;
}

// is the line (terminator and CR dropped) a row at all?  (An empty line is a row, and a bad one: parse_bed_record reports it.)
inline bool bed_is_record(const char* line, size_t len) { return !(len && line[0] == '#'); }

// one record line -> its columns; any violation of the line rules throws
inline void parse_bed_record(const char* line, size_t len, BEDRecord* r) {
  const char* f[13];
  size_t fl[13];
  int nf = 0;
  size_t at = 0;
  for (size_t i = 0; i <= len && nf < 13; ++i)
    if (i == len || line[i] == '\t') {
      f[nf] = line + at;
      fl[nf] = i - at;
      ++nf;
      at = i + 1;
    }
  if (!(nf == 3 || nf == 4 || nf == 5 || nf == 6 || nf == 12))
    gff_fail(line, len, len == 0 ? "empty line" : "invalid number of fields: " + (nf == 13 ? std::string("13 or more") : std::to_string(nf)) + " (3, 4, 5, 6 or 12 are read)", "BED");
  if (!gff_utf8_valid(std::string(line, len))) gff_fail(line, len, "the line is not valid UTF-8", "BED");
  r->chrom = f[0];
  r->chrom_len = fl[0];
  if (!bed_parse_uint(f[1], fl[1], (uint64_t)INT64_MAX, &r->start)) gff_fail(line, len, "invalid start '" + std::string(f[1], fl[1]) + "'", "BED");
  if (!bed_parse_uint(f[2], fl[2], (uint64_t)INT64_MAX, &r->end)) gff_fail(line, len, "invalid end '" + std::string(f[2], fl[2]) + "'", "BED");
  r->name = nullptr;
  r->name_len = 0;
  r->score = -1;
  r->strand = -1;
  if (nf >= 5) {
    r->name = f[3];
    r->name_len = fl[3];
    if (!bed_parse_uint(f[4], fl[4], 65535, &r->score)) gff_fail(line, len, "invalid score '" + std::string(f[4], fl[4]) + "' (0 .. 65535)", "BED");
  }
  if (nf >= 6) {
    const char sc = fl[5] == 1 ? f[5][0] : '\0';
    if (sc == '+') r->strand = 0;
    else if (sc == '-') r->strand = 1;
    else if (sc != '.') gff_fail(line, len, "invalid strand '" + std::string(f[5], fl[5]) + "'", "BED");
  }
}

// the reference's schema (schema.rs:27-48): name, Arrow format, nullable
struct BEDField {
  const char* name;
  const char* fmt;
  bool nullable;
};
inline const BEDField* bed_fields() {
  static const BEDField f[12] = {{"reference_sequence_name", "i", false}, {"start", "l", false}, {"end", "l", false}, {"name", "u", true},
                                 {"score", "l", true}, {"strand", "i", true}, {"thick_start", "l", true}, {"thick_end", "l", true},
                                 {"color", "u", true}, {"block_count", "l", true}, {"block_sizes", "u", true}, {"block_starts", "u", true}};
  return f;
}
constexpr uint64_t BED_PROJECTION_BITS = 0xFF8ull;  // bits 3..11

// n all-NULL rows of a column of bed_fields()[c] (c >= 6)
inline struct ArrowArray* bed_null_column(int c, size_t n) { return slab_null_column(bed_fields()[c].fmt[0] == 'u', (int64_t)n); }

class BEDArrayBuilder : public ExonArrayBuilder {
 public:
  BEDArrayBuilder(Dictionary* chroms, uint64_t projection) : dict_(chroms), proj_(projection) {}

  void append(const BEDRecord& r) {
    id_.append_value(dict_->lookup_or_insert(r.chrom, r.chrom_len));
    start_.append_value(r.start);
    end_.append_value(r.end);
    if (proj_ & (1ull << 3)) {
      if (r.name) name_.append_value(r.name, r.name_len);
      else name_.append_null();
    }
    if (proj_ & (1ull << 4)) {
      if (r.score >= 0) score_.append_value(r.score);
      else score_.append_null(0);
    }
    if (proj_ & (1ull << 5)) {
      if (r.strand >= 0) strand_.append_value(r.strand);
      else strand_.append_null(0);
    }
    ++rows_;
  }
  size_t len() const override { return rows_; }
  std::vector<struct ArrowArray*> finish() override { return slice(0, rows_, true); }
  // rows [o, o + n) as arrays of their own (values copied); `reset`: the builder starts over
  std::vector<struct ArrowArray*> slice(size_t o, size_t n, bool reset = false) {
    auto prim = [&](auto& pb, int elem, struct ArrowArray* dict) {
      struct ArrowArray* a = static_cast<struct ArrowArray*>(malloc(sizeof *a));
      const std::vector<uint8_t> valid(pb.valid.begin() + (long)o, pb.valid.begin() + (long)(o + n));
      make_primitive(a, reinterpret_cast<const uint8_t*>(pb.values.data()) + o * (size_t)elem, (int64_t)n, elem, valid, dict);
      return a;
    };
    std::vector<struct ArrowArray*> out;
    out.push_back(prim(id_, 4, utf8_array(dict_->names)));
    out.push_back(prim(start_, 8, nullptr));
    out.push_back(prim(end_, 8, nullptr));
    if (proj_ & (1ull << 3)) {
      struct ArrowArray* a = static_cast<struct ArrowArray*>(malloc(sizeof *a));
      const int32_t b0 = name_.offsets[o];
      std::vector<int32_t> off(n + 1);
      for (size_t k = 0; k <= n; ++k) off[k] = name_.offsets[o + k] - b0;
      make_utf8(a, off, name_.data.substr((size_t)b0, (size_t)off[n]), std::vector<uint8_t>(name_.valid.begin() + (long)o, name_.valid.begin() + (long)(o + n)));
      out.push_back(a);
    }
    if (proj_ & (1ull << 4)) out.push_back(prim(score_, 8, nullptr));
    if (proj_ & (1ull << 5)) out.push_back(prim(strand_, 4, utf8_array(gff_strand_names())));
    for (int c = 6; c < 12; ++c)
      if (proj_ & (1ull << c)) out.push_back(bed_null_column(c, n));
    if (reset) {
      id_ = {};
      start_ = {};
      end_ = {};
      name_ = {};
      score_ = {};
      strand_ = {};
      rows_ = 0;
    }
    return out;
  }
  PrimitiveBuilder<int32_t>& ids() { return id_; }
  void set_dictionary(Dictionary* d) { dict_ = d; }

 private:
  Dictionary* dict_;
  uint64_t proj_;
  PrimitiveBuilder<int32_t> id_, strand_;
  PrimitiveBuilder<int64_t> start_, end_, score_;
  Utf8Builder name_;
  size_t rows_ = 0;
};

// one slab of BED text parsed with a slab-local dictionary (re-keyed by the reader in file order)
struct BEDSlab : TextSlab {
  Dictionary dict;
  std::unique_ptr<BEDArrayBuilder> b;
  size_t rows = 0;
};
inline void parse_bed_slab(BEDSlab& s, const void* vcfg) {
  const uint64_t projection = *static_cast<const uint64_t*>(vcfg);
  s.b.reset(new BEDArrayBuilder(&s.dict, projection));
  const char* p = s.data();
  const char* end = p + s.len;
  BEDRecord rec;
  while (p < end) {
    const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
    size_t len = nl ? (size_t)(nl - p) : (size_t)(end - p);
    const char* next = nl ? nl + 1 : end;
    if (nl && len && p[len - 1] == '\r') --len;
    if (bed_is_record(p, len)) {
      parse_bed_record(p, len, &rec);
      s.b->append(rec);
    }
    p = next;
  }
  s.rows = s.b->len();
}

// The BED reader stands on the machinery GFFBatchReader stands on -- open_source (plain text, BGZF, gzip), BufReader,
// SlabPipeline over TextSlab, slab-local dictionaries re-keyed in file order, defer_decode / take_stream / data_offset -- as a
// sibling class: its record, its builder and its columns are its own, and it has neither a filter nor index chunks.
class BEDBatchReader : public BatchReader {
 public:
  BEDBatchReader(const std::string& path, Compression c, BEDConfig cfg) : cfg_(std::move(cfg)), projection_(cfg_.projection) {
    r_.reset(new BufReader(open_source(path, c, cfg_.threads)));
    const int threads = cfg_.threads > 0 ? cfg_.threads : decode_threads();
    if (threads > 1 && file_size(path) >= (8 << 20) && !cfg_.defer_decode)
      pipe_.reset(new SlabPipeline<BEDSlab>(r_->release_source(), std::string(), 1, threads, [](BEDSlab& s, const void* c2) { parse_bed_slab(s, c2); }, &projection_));
  }

  const BEDConfig& config() const { return cfg_; }
  // the whole file as a raw byte stream (GPU-side parsing; BED has no header to read first); only valid before the first read_batch
  std::unique_ptr<ByteSource> take_stream(std::string* carry) {
    if (pipe_ || !r_) return nullptr;
    *carry = r_->take_buffered();
    return r_->release_source();
  }
  int64_t data_offset() const { return pipe_ ? -1 : 0; }

  bool read_batch(struct ArrowArray* out) override {
    if (pipe_) return read_batch_parallel(out);
    BEDArrayBuilder b(&dict, cfg_.projection);
    std::string line;
    BEDRecord rec;
    while ((int64_t)b.len() < cfg_.batch_size && r_->read_line(&line)) {
      if (!bed_is_record(line.data(), line.size())) continue;
      parse_bed_record(line.data(), line.size(), &rec);
      b.append(rec);
    }
    if (b.is_empty()) return false;
    b.try_into_record_batch(out);
    return true;
  }

  void schema(struct ArrowSchema* out) const override {
    std::vector<struct ArrowSchema*> kids;
    for (int c = 0; c < 12; ++c) {
      if (c >= 3 && !(cfg_.projection & (1ull << c))) continue;
      const BEDField& f = bed_fields()[c];
      kids.push_back(new_field(f.fmt, f.name, f.nullable, f.fmt[0] == 'i' ? new_field("u", "", false) : nullptr));
    }
    make_schema(out, "+s", "", false, kids);
  }

  // the scan column of schema column c (3..11) under `projection`, -1 when it is not projected
  static int scan_column(uint64_t projection, int c) {
    if (!(projection & (1ull << c))) return -1;
    int k = 3;
    for (int b = 3; b < c; ++b) k += (projection >> b) & 1;
    return k;
  }

  Dictionary dict;  // reference_sequence_name: in order of first appearance in the file, no size limit
  Dictionary strand_dict{gff_strand_names()};

 private:
  bool read_batch_parallel(struct ArrowArray* out) {
    while (!cur_ || cur_pos_ >= cur_->rows) {
      cur_ = pipe_->next();
      if (!cur_) return false;
      cur_pos_ = 0;
      // slab-local ids -> the reader's: names are interned in order of first appearance in the file, as the sequential reader would
      std::vector<int32_t> map(cur_->dict.names.size(), -1);
      for (int32_t& v : cur_->b->ids().values) {
        int32_t& g = map[(size_t)v];
        if (g < 0) g = dict.lookup_or_insert(cur_->dict.names[(size_t)v].data(), cur_->dict.names[(size_t)v].size());
        v = g;
      }
      cur_->b->set_dictionary(&dict);
    }
    const size_t n = std::min<size_t>((size_t)cfg_.batch_size, cur_->rows - cur_pos_);
    make_struct(out, (int64_t)n, cur_->b->slice(cur_pos_, n));
    cur_pos_ += n;
    return true;
  }

  BEDConfig cfg_;
  uint64_t projection_;  // what the slab workers read (outlives the pipeline: declared in front of it)
  std::unique_ptr<BufReader> r_;
  std::unique_ptr<BEDSlab> cur_;
  size_t cur_pos_ = 0;
  std::unique_ptr<SlabPipeline<BEDSlab>> pipe_;  // declared last: destroyed (threads joined) first
};

}  // namespace exon
