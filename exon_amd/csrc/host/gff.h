// gff.h -- GFF3 records: the line rules, the device-layout array builder and the host reader.
//
// Counterpart of exon-gff (array_builder.rs: the schema order; batch_reader.rs:76-131: the read loop and its pushed-down
// filter) and of exon-core/src/datasources/gff (indexed_file_opener.rs: the tabix-planned scan).  Columns of the device layout:
//   0 seqname  1 source  2 type : i32 ids into dictionaries built from the file (GFF has no header), never NULL
//   3 start  4 end : i64, never NULL          5 score : f32? ('.' -> NULL)
//   6 strand : i32 id into ["+", "-"]? ('.' and '?' -> NULL)      7 phase : i32 id into ["0", "1", "2"]? ('.' -> NULL)
//   8 attributes : Map<Utf8, List<Utf8>>, only with EXON_HIP_PROJECT_GFF_ATTRIBUTES (config.rs:81-108, array_builder.rs:141-165)
//
// THE LINE RULES (the device parser, gpu_parse.hip's k_parse_gff_lines, agrees with them or hands the file over):
//   * a line ends at '\n'; one '\r' in front of it is dropped
//   * a line that starts with '#' is no row: '##' directives ('###' included, well-formed or not) and '#' comments.  The
//     reference ignores everything that is not a record (batch_reader.rs:108-118)
//   * a line that starts with "##FASTA" opens a sequence section: refused (UnsupportedError) -- the reference's loop would fail
//     on the first '>' line behind it
//   * every other line is a record of nine TAB-separated fields, the ninth being whatever follows the eighth TAB.  Every
//     record is validated against all eight columns (what SELECT * would touch), whether a pushed-down filter keeps it or not
//   * start, end: decimal, one leading '+' allowed (Rust's usize::from_str: VCFArrayBuilder::parse_pos), and >= 1
//   * score: '.' or Rust's f32::from_str (VCFArrayBuilder::parse_f32, host/decimal_f32.h)
//   * strand: one of + - . ?        phase: one of . 0 1 2
//   * seqname, source, type: the field's bytes as they stand
//   * anything else is an error that quotes the line
// Four corners could not be checked against the reference's parser (noodles-gff 0.41.0) and are DECISIONS of this library:
// an empty line and a record with fewer than eight TABs are errors; end < start is accepted as it is; percent-escapes in the
// first three fields are kept raw.
//
// THE ATTRIBUTE RULES (field 9 with the column projected; text_columns.hip's k_gff_attr_measure / k_gff_attr_fill agree with them
// or hand the file over).  array_builder.rs:141-165 fixes the shape: one entry per attribute in file order, a String value is a
// list of one item, an Array value one item per element; the map, its value lists and the items are never NULL (:149,159,164).
// How noodles-gff splits and decodes the text cannot be read here, so every rule marked DECISION is this library's own:
//   * field 9 is everything behind the eighth TAB up to the line end (CR dropped); TABs inside it are kept
//   * "" and "." give a map of 0 entries
//   * DECISION: entries are split at every ';'.  Exactly one empty piece at the very end (a trailing ';': all 7 rows of the
//     reference's ecoli.gff end so, and its slt reads them) is ignored; any other empty piece (a leading ';', ";;", "a=b;;") is
//     an error that quotes the line
//   * DECISION: a piece is split at its first '='; no '=' is an error; an empty key is accepted; an empty value is one empty item
//   * DECISION: a value that contains ',' is one item per ','-separated piece (empty pieces are empty items), else one item
//   * DECISION: percent-decoding applies to the key and to every item AFTER the splitting: '%' and two hex digits (either case)
//     become that byte, a '%' without them stays; every decoded key and item must be valid UTF-8, else it is an error
//   * DECISION: nothing is trimmed or unquoted; duplicate keys stay separate entries, in file order
//   * with the column projected, field 9 of EVERY record is validated, whether a pushed-down filter keeps it or not
#pragma once
#include "formats.h"

namespace exon {

// the input is well-formed but holds something this library does not read (EXON_HIP_EUNSUPPORTED at the C ABI)
struct UnsupportedError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

struct GFFConfig {
  int64_t batch_size = DEFAULT_BATCH_SIZE;
  int threads = 0;            // decode threads: 0 = all host cores, 1 = sequential reader
  bool defer_decode = false;  // the caller will take the byte stream (GPU-side parsing): start no parse pipeline
  uint64_t projection = 0;    // EXON_HIP_PROJECT_GFF_ATTRIBUTES: column 8
  RegionFilter filter;        // batch_reader.rs:76-97: seqname == region name AND start inside the interval (start only)
  // EXON_HIP_REFERENCE_QUIRKS=1 on an indexed scan: IndexedGffOpener (indexed_file_opener.rs:77-82) reads the COMPRESSED
  // range [chunk.start.compressed, chunk.end.compressed) -- the block that holds the chunk's end is never read, and the line
  // the last whole block cuts off is lost with it.  Off (default): every record of the chunk is read.
  bool reference_block_quirk = false;
};

inline const std::vector<std::string>& gff_strand_names() {
  static const std::vector<std::string> v = {"+", "-"};
  return v;
}
inline const std::vector<std::string>& gff_phase_names() {
  static const std::vector<std::string> v = {"0", "1", "2"};
  return v;
}

struct GFFRecord {
  const char* f[3];  // seqname, source, type
  size_t fl[3];
  int64_t start = 0, end = 0;
  float score = 0.f;
  bool has_score = false;
  int32_t strand = -1, phase = -1;  // -1: NULL
  const char* attr = nullptr;       // field 9 (TABs included)
  size_t attr_len = 0;
};

[[noreturn]] inline void gff_fail(const char* line, size_t len, const std::string& what, const char* format = "GFF") {
  throw std::runtime_error(std::string(format) + " line '" + std::string(line, std::min<size_t>(len, 120)) + (len > 120 ? "...'" : "'") + ": " + what);
}

// is the line (terminator and CR dropped) a row at all?  Throws for an empty line and for a ##FASTA section.
inline bool gff_is_record(const char* line, size_t len) {
  if (len == 0) throw std::runtime_error("GFF: empty line");
  if (line[0] != '#') return true;
  if (len >= 7 && memcmp(line, "##FASTA", 7) == 0)
    throw UnsupportedError("GFF: a ##FASTA section (embedded sequences) is not read; strip it from the file");
  return false;
}

// one record line -> its eight columns; any violation of the line rules throws.  GTF (gtf.h states its rules): the same eight
// fields, but a '?' strand is an error and the eighth column is called the frame
inline void parse_gff_columns(const char* line, size_t len, GFFRecord* r, bool gtf) {
  const char* const fmt = gtf ? "GTF" : "GFF";
  const char* f[8];
  size_t fl[8];
  int nf = 0;
  size_t at = 0;
  for (size_t i = 0; i < len && nf < 8; ++i)
    if (line[i] == '\t') {
      f[nf] = line + at;
      fl[nf] = i - at;
      ++nf;
      at = i + 1;
    }
  if (nf < 8) gff_fail(line, len, "fewer than nine TAB-separated fields", fmt);
  for (int k = 0; k < 3; ++k) {
    r->f[k] = f[k];
    r->fl[k] = fl[k];
  }
  r->attr = line + at;
  r->attr_len = len - at;
  if (!VCFArrayBuilder::parse_pos(f[3], fl[3], &r->start) || r->start < 1) gff_fail(line, len, "invalid start '" + std::string(f[3], fl[3]) + "'", fmt);
  if (!VCFArrayBuilder::parse_pos(f[4], fl[4], &r->end) || r->end < 1) gff_fail(line, len, "invalid end '" + std::string(f[4], fl[4]) + "'", fmt);
  r->has_score = !(fl[5] == 1 && f[5][0] == '.');
  r->score = 0.f;
  if (r->has_score) {
    try {
      r->score = VCFArrayBuilder::parse_f32(f[5], fl[5]);
    } catch (const std::exception&) {
      gff_fail(line, len, "invalid score '" + std::string(f[5], fl[5]) + "'", fmt);
    }
  }
  const char sc = fl[6] == 1 ? f[6][0] : '\0';
  if (sc == '+') r->strand = 0;
  else if (sc == '-') r->strand = 1;
  else if (sc == '.' || (sc == '?' && !gtf)) r->strand = -1;
  else gff_fail(line, len, "invalid strand '" + std::string(f[6], fl[6]) + "'", fmt);
  const char pc = fl[7] == 1 ? f[7][0] : '\0';
  if (pc == '.') r->phase = -1;
  else if (pc >= '0' && pc <= '2') r->phase = pc - '0';
  else gff_fail(line, len, std::string(gtf ? "invalid frame '" : "invalid phase '") + std::string(f[7], fl[7]) + "'", fmt);
}
inline void parse_gff_record(const char* line, size_t len, GFFRecord* r) { parse_gff_columns(line, len, r, false); }

// Rust's str::from_utf8: no overlong forms, no surrogates, nothing above U+10FFFF
inline bool gff_utf8_valid(const std::string& s) {
  const size_t n = s.size();
  for (size_t i = 0; i < n;) {
    const unsigned c = (unsigned char)s[i];
    if (c < 0x80) {
      ++i;
      continue;
    }
    size_t more;
    unsigned lo = 0x80, hi = 0xBF;  // the range of the first continuation byte
    if (c >= 0xC2 && c <= 0xDF) more = 1;
    else if (c >= 0xE0 && c <= 0xEF) more = 2, lo = c == 0xE0 ? 0xA0 : 0x80, hi = c == 0xED ? 0x9F : 0xBF;
    else if (c >= 0xF0 && c <= 0xF4) more = 3, lo = c == 0xF0 ? 0x90 : 0x80, hi = c == 0xF4 ? 0x8F : 0xBF;
    else return false;
    if (i + more >= n) return false;
    for (size_t k = 1; k <= more; ++k) {
      const unsigned d = (unsigned char)s[i + k];
      if (d < (k == 1 ? lo : 0x80u) || d > (k == 1 ? hi : 0xBFu)) return false;
    }
    i += more + 1;
  }
  return true;
}

// the ninth column of a run of rows as the reader's builders and slab machinery hold it, whatever its Arrow type
struct AttrColumn {
  virtual ~AttrColumn() {}
  virtual size_t rows() const = 0;
  virtual void clear() = 0;
  virtual struct ArrowArray* slice(size_t o, size_t n) const = 0;  // rows [o, o + n) as an array of their own
};

// the attributes column of a run of rows: the four offset levels and the two byte pools of Map<Utf8, List<Utf8>>
struct GFFAttrColumn : AttrColumn {
  std::vector<int32_t> map_off{0}, key_off{0}, list_off{0}, item_off{0};  // rows -> entries -> (key bytes | items -> item bytes)
  std::string keys, items;
  size_t rows() const override { return map_off.size() - 1; }
  void clear() override {
    map_off.assign(1, 0);
    key_off.assign(1, 0);
    list_off.assign(1, 0);
    item_off.assign(1, 0);
    keys.clear();
    items.clear();
  }
  // rows [o, o + n) as an array of their own (offsets rebased, bytes copied); the whole column with o = 0, n = rows()
  struct ArrowArray* slice(size_t o, size_t n) const override {
    const int32_t e0 = map_off[o], e1 = map_off[o + n], i0 = list_off[(size_t)e0], i1 = list_off[(size_t)e1];
    const int32_t k0 = key_off[(size_t)e0], k1 = key_off[(size_t)e1], b0 = item_off[(size_t)i0], b1 = item_off[(size_t)i1];
    auto rebased = [](const std::vector<int32_t>& v, int32_t from, int32_t to, int32_t base) {
      std::vector<int32_t> r((size_t)(to - from) + 1);
      for (size_t k = 0; k < r.size(); ++k) r[k] = v[(size_t)from + k] - base;
      return r;
    };
    auto arr = [] { return static_cast<struct ArrowArray*>(malloc(sizeof(struct ArrowArray))); };
    struct ArrowArray *ka = arr(), *ia = arr(), *la = arr(), *ea = arr(), *ma = arr();
    make_utf8(ka, rebased(key_off, e0, e1, k0), keys.substr((size_t)k0, (size_t)(k1 - k0)), {});
    make_utf8(ia, rebased(item_off, i0, i1, b0), items.substr((size_t)b0, (size_t)(b1 - b0)), {});
    make_list(la, rebased(list_off, e0, e1, i0), {}, ia);
    make_struct(ea, e1 - e0, {ka, la});
    make_list(ma, rebased(map_off, (int32_t)o, (int32_t)(o + n), e0), {}, ea);  // (a map's buffers are a list's: offsets over one child)
    return ma;
  }
};

// [p, p + n) percent-decoded onto `out`: '%' and two hex digits become that byte, any other '%' stays
inline void gff_percent_decode(const char* p, size_t n, std::string* out) {
  auto hex = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
  for (size_t i = 0; i < n; ++i) {
    if (p[i] == '%' && i + 2 < n && hex(p[i + 1]) >= 0 && hex(p[i + 2]) >= 0) {
      out->push_back((char)(hex(p[i + 1]) * 16 + hex(p[i + 2])));
      i += 2;
    } else {
      out->push_back(p[i]);
    }
  }
}

// field 9 of record `r` by THE ATTRIBUTE RULES: validated, and appended to `col` as one row when there is one
inline void parse_gff_attributes(const char* line, size_t len, const GFFRecord& r, AttrColumn* sink) {
  GFFAttrColumn* col = static_cast<GFFAttrColumn*>(sink);
  const char* a = r.attr;
  const size_t n = r.attr_len;
  std::string tmp;
  auto text = [&](const char* p, size_t m, std::string* pool, std::vector<int32_t>* off, const char* what) {
    tmp.clear();
    gff_percent_decode(p, m, &tmp);
    if (!gff_utf8_valid(tmp)) gff_fail(line, len, std::string("attribute ") + what + " is not valid UTF-8");
    if (col) {
      pool->append(tmp);
      off->push_back((int32_t)pool->size());
    }
  };
  if (!(n == 0 || (n == 1 && a[0] == '.'))) {
    size_t at = 0;
    while (at <= n) {
      const char* semi = static_cast<const char*>(memchr(a + at, ';', n - at));
      const size_t end = semi ? (size_t)(semi - a) : n;
      if (end == at) {
        if (!semi && at > 0) break;  // the one empty piece behind a trailing ';'
        gff_fail(line, len, "empty attribute (a ';' with nothing in front of it)");
      }
      const char* eq = static_cast<const char*>(memchr(a + at, '=', end - at));
      if (!eq) gff_fail(line, len, "attribute '" + std::string(a + at, std::min<size_t>(end - at, 60)) + "' has no '='");
      text(a + at, (size_t)(eq - (a + at)), col ? &col->keys : nullptr, col ? &col->key_off : nullptr, "key");
      size_t v = (size_t)(eq - a) + 1;
      for (;;) {
        const char* comma = static_cast<const char*>(memchr(a + v, ',', end - v));
        const size_t ve = comma ? (size_t)(comma - a) : end;
        text(a + v, ve - v, col ? &col->items : nullptr, col ? &col->item_off : nullptr, "value");
        if (!comma) break;
        v = ve + 1;
      }
      if (col) col->list_off.push_back((int32_t)col->item_off.size() - 1);
      at = end + 1;
    }
  }
  if (col) col->map_off.push_back((int32_t)col->key_off.size() - 1);
}

inline bool gff_region_hit(const GFFRecord& r, const Region& rg) {
  return r.fl[0] == rg.name.size() && memcmp(r.f[0], rg.name.data(), r.fl[0]) == 0 && r.start >= rg.start && r.start <= rg.end;
}

// a field of a schema with children
inline struct ArrowSchema* new_nested_field(const char* fmt, const char* name, bool nullable, std::vector<struct ArrowSchema*> kids) {
  struct ArrowSchema* f = static_cast<struct ArrowSchema*>(malloc(sizeof *f));
  make_schema(f, fmt, name, nullable, std::move(kids));
  return f;
}

// What differs between the two formats GFFBatchReader reads -- GFF3 (here) and GTF (gtf.h): the line rules, the ninth column and
// the eighth column's name.  Everything else (slabs, dictionaries and their re-keying, the filter, the batches) is shared.
struct GFFDialect {
  bool (*is_record)(const char* line, size_t len);                                                  // a row at all?  (throws: no line of the format)
  void (*parse_record)(const char* line, size_t len, GFFRecord* r);                                 // the eight columns
  void (*parse_attributes)(const char* line, size_t len, const GFFRecord& r, AttrColumn* sink);     // field 9: validated, appended when sink != nullptr
  AttrColumn* (*new_attributes)();
  struct ArrowSchema* (*attributes_field)();
  const char* column7;
};
inline const GFFDialect* gff3_dialect() {
  static const GFFDialect d = {gff_is_record, parse_gff_record, parse_gff_attributes, [] { return static_cast<AttrColumn*>(new GFFAttrColumn()); },
                               [] {  // Field::new_map("attributes", "entries", keys, values, sorted = false) of config.rs:81-104
                                 struct ArrowSchema* values = new_nested_field("+l", "values", true, {new_field("u", "item", true)});
                                 struct ArrowSchema* entries = new_nested_field("+s", "entries", false, {new_field("u", "keys", false), values});
                                 return new_nested_field("+m", "attributes", false, {entries});
                               },
                               "phase"};
  return &d;
}

class GFFArrayBuilder : public ExonArrayBuilder {
 public:
  GFFArrayBuilder(Dictionary* seqnames, Dictionary* sources, Dictionary* types, const GFFDialect* dialect, bool attributes = false)
      : dicts_{seqnames, sources, types}, with_attrs_(attributes), attrs_(dialect->new_attributes()) {}

  void append(const GFFRecord& r) {
    for (int k = 0; k < 3; ++k) ids_[k].append_value(dicts_[k]->lookup_or_insert(r.f[k], r.fl[k]));
    start_.append_value(r.start);
    end_.append_value(r.end);
    if (r.has_score) score_.append_value(r.score);
    else score_.append_null(0.f);
    if (r.strand >= 0) strand_.append_value(r.strand);
    else strand_.append_null(0);
    if (r.phase >= 0) phase_.append_value(r.phase);
    else phase_.append_null(0);
    ++rows_;
  }
  size_t len() const override { return rows_; }
  std::vector<struct ArrowArray*> finish() override {
    std::vector<struct ArrowArray*> out;
    for (int k = 0; k < 3; ++k) out.push_back(ids_[k].finish(utf8_array(dicts_[k]->names)));
    out.push_back(start_.finish());
    out.push_back(end_.finish());
    out.push_back(score_.finish());
    out.push_back(strand_.finish(utf8_array(gff_strand_names())));
    out.push_back(phase_.finish(utf8_array(gff_phase_names())));
    if (with_attrs_) {
      out.push_back(attrs_->slice(0, attrs_->rows()));
      attrs_->clear();
    }
    rows_ = 0;
    return out;
  }
  void reserve(size_t rows) {
    for (auto& v : ids_) { v.values.reserve(rows); v.valid.reserve(rows); }
    for (auto* v : {&start_, &end_}) { v->values.reserve(rows); v->valid.reserve(rows); }
    score_.values.reserve(rows); score_.valid.reserve(rows);
    for (auto* v : {&strand_, &phase_}) { v->values.reserve(rows); v->valid.reserve(rows); }
  }
  PrimitiveBuilder<int32_t>& ids(int k) { return ids_[k]; }
  PrimitiveBuilder<int64_t>& starts() { return start_; }
  PrimitiveBuilder<int64_t>& ends() { return end_; }
  PrimitiveBuilder<float>& scores() { return score_; }
  PrimitiveBuilder<int32_t>& strands() { return strand_; }
  PrimitiveBuilder<int32_t>& phases() { return phase_; }
  bool with_attributes() const { return with_attrs_; }
  AttrColumn& attributes() { return *attrs_; }  // (the caller appends the row's map: the dialect's parse_attributes)

 private:
  Dictionary* dicts_[3];
  PrimitiveBuilder<int32_t> ids_[3], strand_, phase_;
  PrimitiveBuilder<int64_t> start_, end_;
  PrimitiveBuilder<float> score_;
  bool with_attrs_;
  std::unique_ptr<AttrColumn> attrs_;
  size_t rows_ = 0;
};

// one slab of GFF text parsed with slab-local dictionaries (re-keyed by the reader in file order)
struct GFFSlabConfig {
  RegionFilter filter;
  bool attributes = false;
  const GFFDialect* dialect = gff3_dialect();
};
struct GFFSlab : TextSlab {
  Dictionary dicts[3];
  std::unique_ptr<GFFArrayBuilder> b;
  size_t rows = 0;
};
inline void parse_gff_slab(GFFSlab& s, const void* vcfg) {
  const GFFSlabConfig& sc = *static_cast<const GFFSlabConfig*>(vcfg);
  const RegionFilter& filter = sc.filter;
  const GFFDialect& d = *sc.dialect;
  s.b.reset(new GFFArrayBuilder(&s.dicts[0], &s.dicts[1], &s.dicts[2], &d, sc.attributes));
  const char* p = s.data();
  const char* end = p + s.len;
  s.b->reserve(s.len / 64 + 16);
  GFFRecord rec;
  while (p < end) {
    const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
    size_t len = nl ? (size_t)(nl - p) : (size_t)(end - p);
    const char* next = nl ? nl + 1 : end;
    if (nl && len && p[len - 1] == '\r') --len;
    if (d.is_record(p, len)) {
      d.parse_record(p, len, &rec);
      const bool keep = !filter.active || gff_region_hit(rec, filter.region);
      if (sc.attributes) d.parse_attributes(p, len, rec, keep ? &s.b->attributes() : nullptr);
      if (keep) s.b->append(rec);
    }
    p = next;
  }
  s.rows = s.b->len();
}

class GFFBatchReader : public BatchReader {
 public:
  GFFBatchReader(const std::string& path, Compression c, GFFConfig cfg, const GFFDialect* dialect = gff3_dialect()) : cfg_(std::move(cfg)), d_(dialect) {
    slab_cfg_.filter = cfg_.filter;
    slab_cfg_.attributes = attributes();
    slab_cfg_.dialect = d_;
    if (cfg_.filter.active && cfg_.filter.use_index) {
      // get_byte_range_for_file (indexed_bgzf_file.rs:52-112) with the index's own column preset
      const BinningIndex idx = read_tabix(path + ".tbi");
      if (idx.col_seq != 1 || idx.col_beg != 4 || idx.col_end != 5)
        throw std::runtime_error(path + ".tbi: not built with the GFF preset (sequence column " + std::to_string(idx.col_seq) + ", begin " +
                                 std::to_string(idx.col_beg) + ", end " + std::to_string(idx.col_end) + "; expected 1, 4, 5)");
      int id = -1;
      for (size_t i = 0; i < idx.names.size(); ++i)
        if (idx.names[i] == cfg_.filter.region.name) id = (int)i;
      if (id >= 0) planned_chunks = query_index(idx, id, cfg_.filter.region.start, cfg_.filter.region.end);
      n_chunks = (int)planned_chunks.size();
      if (cfg_.reference_block_quirk) bgzf_.reset(new BgzfReader(path));
      else chunks_.reset(new ChunkSource(path, planned_chunks));
      file_bytes_ = (uint64_t)std::max<long>(0, file_size(path));
      return;
    }
    r_.reset(new BufReader(open_source(path, c, cfg_.threads)));
    const int threads = cfg_.threads > 0 ? cfg_.threads : decode_threads();
    if (threads > 1 && file_size(path) >= (8 << 20) && !cfg_.defer_decode)
      pipe_.reset(new SlabPipeline<GFFSlab>(r_->release_source(), std::string(), 1, threads, [](GFFSlab& s, const void* c2) { parse_gff_slab(s, c2); },
                                            &slab_cfg_));
  }

  const GFFConfig& config() const { return cfg_; }
  bool attributes() const { return (cfg_.projection & EXON_HIP_PROJECT_GFF_ATTRIBUTES) != 0; }
  // the whole file as a raw byte stream (GPU-side parsing; GFF has no header to read first); only valid before the first read_batch
  std::unique_ptr<ByteSource> take_stream(std::string* carry) {
    if (pipe_ || n_chunks >= 0 || !r_) return nullptr;
    *carry = r_->take_buffered();
    return r_->release_source();
  }
  int64_t data_offset() const { return (pipe_ || n_chunks >= 0) ? -1 : 0; }

  bool read_batch(struct ArrowArray* out) override {
    if (pipe_) return read_batch_parallel(out);
    GFFArrayBuilder b(&dicts[0], &dicts[1], &dicts[2], d_, attributes());
    std::string line;
    GFFRecord rec;
    while ((int64_t)b.len() < cfg_.batch_size && next_line(&line)) {
      if (!d_->is_record(line.data(), line.size())) continue;
      d_->parse_record(line.data(), line.size(), &rec);
      const bool keep = !cfg_.filter.active || gff_region_hit(rec, cfg_.filter.region);
      if (attributes()) d_->parse_attributes(line.data(), line.size(), rec, keep ? &b.attributes() : nullptr);
      if (keep) b.append(rec);
    }
    if (b.is_empty()) return false;
    b.try_into_record_batch(out);
    return true;
  }

  void schema(struct ArrowSchema* out) const override {
    std::vector<struct ArrowSchema*> kids = {new_field("i", "seqname", false, new_field("u", "", false)),
                                             new_field("i", "source", false, new_field("u", "", false)),
                                             new_field("i", "type", false, new_field("u", "", false)),
                                             new_field("l", "start", false),
                                             new_field("l", "end", false),
                                             new_field("f", "score", true),
                                             new_field("i", "strand", true, new_field("u", "", false)),
                                             new_field("i", d_->column7, true, new_field("u", "", false))};
    if (attributes()) kids.push_back(d_->attributes_field());
    make_schema(out, "+s", "", false, kids);
  }

  Dictionary dicts[3];  // seqname, source, type: in order of first appearance in the file, no size limit
  Dictionary strand_dict{gff_strand_names()}, phase_dict{gff_phase_names()};
  int n_chunks = -1;                  // index chunks planned (-1: not an indexed scan)
  std::vector<Chunk> planned_chunks;  // ... and the chunks themselves

 private:
  // the next line of the scan (CR dropped), from the stream, the index chunks, or the reference's block ranges
  bool next_line(std::string* line) {
    if (chunks_) return chunks_->next_record() && chunks_->read_line(line);
    if (bgzf_) {
      for (;;) {
        if (ci_ >= planned_chunks.size()) return false;
        const Chunk& ch = planned_chunks[ci_];
        // indexed_file_opener.rs:77-82: the range ends at the chunk end's BLOCK (the whole rest of the file when both ends share one)
        const uint64_t lo = ch.start >> 16, hi = (ch.end >> 16) == lo ? file_bytes_ : (ch.end >> 16);
        if (!in_chunk_) {
          bgzf_->seek(ch.start);
          in_chunk_ = true;
        }
        // a line is whole when its '\n' lies in a block in front of `hi`
        if (bgzf_->tell() < (hi << 16) && bgzf_->read_line(line) && bgzf_->last_line_terminated() && bgzf_->tell() <= (hi << 16)) return true;
        ++ci_;
        in_chunk_ = false;
      }
    }
    return r_->read_line(line);
  }

  bool next_slab() {
    while (!cur_ || cur_pos_ >= cur_->rows) {
      cur_ = pipe_->next();
      if (!cur_) return false;
      cur_pos_ = 0;
      // slab-local ids -> the reader's: names are interned in order of first appearance in the file, as the sequential reader would
      for (int k = 0; k < 3; ++k) {
        std::vector<int32_t> map(cur_->dicts[k].names.size(), -1);
        for (int32_t& v : cur_->b->ids(k).values) {
          int32_t& g = map[(size_t)v];
          if (g < 0) g = dicts[k].lookup_or_insert(cur_->dicts[k].names[(size_t)v].data(), cur_->dicts[k].names[(size_t)v].size());
          v = g;
        }
      }
    }
    return true;
  }

  bool read_batch_parallel(struct ArrowArray* out) {
    if (!next_slab()) return false;
    const size_t n = std::min<size_t>((size_t)cfg_.batch_size, cur_->rows - cur_pos_), o = cur_pos_;
    auto slice = [&](auto& pb, int elem, struct ArrowArray* dict) {
      struct ArrowArray* a = static_cast<struct ArrowArray*>(malloc(sizeof *a));
      std::vector<uint8_t> valid(pb.valid.begin() + (long)o, pb.valid.begin() + (long)(o + n));
      make_primitive(a, reinterpret_cast<const uint8_t*>(pb.values.data()) + o * (size_t)elem, (int64_t)n, elem, valid, dict);
      return a;
    };
    GFFArrayBuilder& b = *cur_->b;
    std::vector<struct ArrowArray*> kids;
    for (int k = 0; k < 3; ++k) kids.push_back(slice(b.ids(k), 4, utf8_array(dicts[k].names)));
    kids.push_back(slice(b.starts(), 8, nullptr));
    kids.push_back(slice(b.ends(), 8, nullptr));
    kids.push_back(slice(b.scores(), 4, nullptr));
    kids.push_back(slice(b.strands(), 4, utf8_array(gff_strand_names())));
    kids.push_back(slice(b.phases(), 4, utf8_array(gff_phase_names())));
    if (b.with_attributes()) kids.push_back(b.attributes().slice(o, n));
    make_struct(out, (int64_t)n, std::move(kids));
    cur_pos_ += n;
    return true;
  }

  GFFConfig cfg_;
  const GFFDialect* d_;
  GFFSlabConfig slab_cfg_;  // what the slab workers read (outlives the pipeline: declared in front of it)
  std::unique_ptr<BufReader> r_;
  std::unique_ptr<ChunkSource> chunks_;
  std::unique_ptr<BgzfReader> bgzf_;  // reference_block_quirk: the chunks' block ranges
  size_t ci_ = 0;
  bool in_chunk_ = false;
  uint64_t file_bytes_ = 0;
  std::unique_ptr<GFFSlab> cur_;
  size_t cur_pos_ = 0;
  std::unique_ptr<SlabPipeline<GFFSlab>> pipe_;  // declared last: destroyed (threads joined) first
};

}  // namespace exon
