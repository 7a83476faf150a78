// gff.h -- GFF3 records: the line rules, the device-layout array builder and the host reader.
//
// Counterpart of exon-gff (array_builder.rs: the schema order; batch_reader.rs:76-131: the read loop and its pushed-down
// filter) and of exon-core/src/datasources/gff (indexed_file_opener.rs: the tabix-planned scan).  Columns of the device layout:
//   0 seqname  1 source  2 type : i32 ids into dictionaries built from the file (GFF has no header), never NULL
//   3 start  4 end : i64, never NULL          5 score : f32? ('.' -> NULL)
//   6 strand : i32 id into ["+", "-"]? ('.' and '?' -> NULL)      7 phase : i32 id into ["0", "1", "2"]? ('.' -> NULL)
// `attributes` (Map<Utf8, List<Utf8>>) is not built.
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
};

[[noreturn]] inline void gff_fail(const char* line, size_t len, const std::string& what) {
  throw std::runtime_error("GFF line '" + std::string(line, std::min<size_t>(len, 120)) + (len > 120 ? "...'" : "'") + ": " + what);
}

// is the line (terminator and CR dropped) a row at all?  Throws for an empty line and for a ##FASTA section.
inline bool gff_is_record(const char* line, size_t len) {
  if (len == 0) throw std::runtime_error("GFF: empty line");
  if (line[0] != '#') return true;
  if (len >= 7 && memcmp(line, "##FASTA", 7) == 0)
    throw UnsupportedError("GFF: a ##FASTA section (embedded sequences) is not read; strip it from the file");
  return false;
}

// one record line -> its eight columns; any violation of the line rules throws
inline void parse_gff_record(const char* line, size_t len, GFFRecord* r) {
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
  if (nf < 8) gff_fail(line, len, "fewer than nine TAB-separated fields");
  for (int k = 0; k < 3; ++k) {
    r->f[k] = f[k];
    r->fl[k] = fl[k];
  }
  if (!VCFArrayBuilder::parse_pos(f[3], fl[3], &r->start) || r->start < 1) gff_fail(line, len, "invalid start '" + std::string(f[3], fl[3]) + "'");
  if (!VCFArrayBuilder::parse_pos(f[4], fl[4], &r->end) || r->end < 1) gff_fail(line, len, "invalid end '" + std::string(f[4], fl[4]) + "'");
  r->has_score = !(fl[5] == 1 && f[5][0] == '.');
  r->score = 0.f;
  if (r->has_score) {
    try {
      r->score = VCFArrayBuilder::parse_f32(f[5], fl[5]);
    } catch (const std::exception&) {
      gff_fail(line, len, "invalid score '" + std::string(f[5], fl[5]) + "'");
    }
  }
  const char sc = fl[6] == 1 ? f[6][0] : '\0';
  if (sc == '+') r->strand = 0;
  else if (sc == '-') r->strand = 1;
  else if (sc == '.' || sc == '?') r->strand = -1;
  else gff_fail(line, len, "invalid strand '" + std::string(f[6], fl[6]) + "'");
  const char pc = fl[7] == 1 ? f[7][0] : '\0';
  if (pc == '.') r->phase = -1;
  else if (pc >= '0' && pc <= '2') r->phase = pc - '0';
  else gff_fail(line, len, "invalid phase '" + std::string(f[7], fl[7]) + "'");
}

inline bool gff_region_hit(const GFFRecord& r, const Region& rg) {
  return r.fl[0] == rg.name.size() && memcmp(r.f[0], rg.name.data(), r.fl[0]) == 0 && r.start >= rg.start && r.start <= rg.end;
}

class GFFArrayBuilder : public ExonArrayBuilder {
 public:
  GFFArrayBuilder(Dictionary* seqnames, Dictionary* sources, Dictionary* types) : dicts_{seqnames, sources, types} {}

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

 private:
  Dictionary* dicts_[3];
  PrimitiveBuilder<int32_t> ids_[3], strand_, phase_;
  PrimitiveBuilder<int64_t> start_, end_;
  PrimitiveBuilder<float> score_;
  size_t rows_ = 0;
};

// one slab of GFF text parsed with slab-local dictionaries (re-keyed by the reader in file order)
struct GFFSlab : TextSlab {
  Dictionary dicts[3];
  std::unique_ptr<GFFArrayBuilder> b;
  size_t rows = 0;
};
inline void parse_gff_slab(GFFSlab& s, const void* vfilter) {
  const RegionFilter& filter = *static_cast<const RegionFilter*>(vfilter);
  s.b.reset(new GFFArrayBuilder(&s.dicts[0], &s.dicts[1], &s.dicts[2]));
  const char* p = s.data();
  const char* end = p + s.len;
  s.b->reserve(s.len / 64 + 16);
  GFFRecord rec;
  while (p < end) {
    const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
    size_t len = nl ? (size_t)(nl - p) : (size_t)(end - p);
    const char* next = nl ? nl + 1 : end;
    if (nl && len && p[len - 1] == '\r') --len;
    if (gff_is_record(p, len)) {
      parse_gff_record(p, len, &rec);
      if (!filter.active || gff_region_hit(rec, filter.region)) s.b->append(rec);
    }
    p = next;
  }
  s.rows = s.b->len();
}

class GFFBatchReader : public BatchReader {
 public:
  GFFBatchReader(const std::string& path, Compression c, GFFConfig cfg) : cfg_(std::move(cfg)) {
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
                                            &cfg_.filter));
  }

  const GFFConfig& config() const { return cfg_; }
  // the whole file as a raw byte stream (GPU-side parsing; GFF has no header to read first); only valid before the first read_batch
  std::unique_ptr<ByteSource> take_stream(std::string* carry) {
    if (pipe_ || n_chunks >= 0 || !r_) return nullptr;
    *carry = r_->take_buffered();
    return r_->release_source();
  }
  int64_t data_offset() const { return (pipe_ || n_chunks >= 0) ? -1 : 0; }

  bool read_batch(struct ArrowArray* out) override {
    if (pipe_) return read_batch_parallel(out);
    GFFArrayBuilder b(&dicts[0], &dicts[1], &dicts[2]);
    std::string line;
    GFFRecord rec;
    while ((int64_t)b.len() < cfg_.batch_size && next_line(&line)) {
      if (!gff_is_record(line.data(), line.size())) continue;
      parse_gff_record(line.data(), line.size(), &rec);
      if (cfg_.filter.active && !gff_region_hit(rec, cfg_.filter.region)) continue;
      b.append(rec);
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
                                             new_field("i", "phase", true, new_field("u", "", false))};
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
    make_struct(out, (int64_t)n, std::move(kids));
    cur_pos_ += n;
    return true;
  }

  GFFConfig cfg_;
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
