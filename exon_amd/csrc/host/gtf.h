// gtf.h -- GTF records: the line rules, the attributes column and the host reader (a dialect of gff.h's GFFBatchReader).
//
// Counterpart of exon-gtf (config.rs:28-41: the schema; array_builder.rs:82-87: the attributes map; batch_reader.rs: the read
// loop).  The reference parses with noodles-gtf, whose text could not be read here: what its code and fixtures fix is marked
// (ref), everything else is a DECISION of this library.  Columns of the device layout:
//   0 seqname  1 source  2 type : i32 ids into dictionaries built from the file, never NULL
//   3 start  4 end : i64, never NULL          5 score : f32? ('.' -> NULL)
//   6 strand : i32 id into ["+", "-"]? ('.' -> NULL)      7 frame : i32 id into ["0", "1", "2"]? ('.' -> NULL)
//   8 attributes : Map<Utf8, Utf8>, only with EXON_HIP_PROJECT_GTF_ATTRIBUTES; the map is never NULL, keys are non-null, the
//     values field is nullable but no value is ever NULL (ref: config.rs:28-41, array_builder.rs:82-87)
//
// THE LINE RULES (the device parser, gpu_parse.hip's k_parse_gff_lines<ATTR, true>, agrees with them or hands the file over):
//   * a line ends at '\n'
//   * DECISION: one '\r' in front of the '\n' is dropped (the reference keeps it on Linux)
//   * a last line without '\n' is read whole.  KNOWN DIFFERENCE: the reference's `buf.pop()` (batch_reader.rs:57) would eat the
//     last byte of such a line; that is not reproduced
//   * (ref) a line that starts with '#' is no row (Line::Comment is skipped).  There is no "##FASTA" special case: it is a comment
//   * DECISION: an empty line is an error
//   * every other line is a record: eight TAB-separated fields and a ninth that is whatever follows the eighth TAB
//   * DECISION: fewer than eight TABs is an error
//   * start, end: as GFF -- decimal, one leading '+' allowed, >= 1.  DECISION: end < start is accepted as it stands
//   * score: '.' or Rust's f32::from_str
//   * strand: '+', '-', or '.' -> NULL.  DECISION: '?' is an error (the one difference from GFF3's eight columns)
//   * KNOWN DIFFERENCE: the reference declares `strand` non-nullable but appends an Option, so a '.' would fail its
//     RecordBatch::try_new; here it is NULL, as in GFF
//   * frame: '.' -> NULL, or '0' / '1' / '2'
//   * seqname, source, type: the field's bytes as they stand
//   * anything else is an error that quotes the line
//
// THE ATTRIBUTE RULES (field 9 with the column projected; then EVERY record's ninth field is validated, whether a pushed-down
// filter keeps it or not; text_columns.hip's k_gtf_attr_measure / k_gtf_attr_fill agree with them or hand the file over).  All of
// the grammar is a DECISION; (ref) fixes only the shape: one entry per attribute in file order, values are strings, quotes gone
// (gtf-scan-tests.slt: gene_id -> ENSG00000223972).
//   * "" is a map of 0 entries; otherwise the field is a run of entries
//   * an entry is `key`, one or more spaces, `value`, optional spaces, then ';' or the end of the field
//   * spaces in front of a key (at the start of the field, behind a ';') are skipped; a trailing ';' followed by spaces ends the
//     field (so a field of spaces alone is a map of 0 entries)
//   * key: the bytes up to the first space, non-empty
//   * value, quoted form: if it starts with '"', the value is the bytes up to the next '"', which may be none.  The quotes are
//     dropped, there is no escape processing, and ';' and spaces inside belong to the value
//   * value, bare form: otherwise the value is the bytes up to the next ';' or the end of the field, trailing spaces dropped (it
//     is non-empty: its first byte is none of ' ', ';', '"')
//   * errors, each quoting the line: a missing closing quote; a key with no value (the field or the entry ends behind the key or
//     behind its spaces); an empty piece (";;", a leading ';'); bytes other than spaces between a closing quote and the ';'
//   * duplicate keys stay separate entries in file order (real files repeat `tag`)
//   * nothing is percent-decoded; only ' ' (0x20) is a space -- a TAB inside the ninth field is a byte like any other
//   * keys and values must be valid UTF-8 (Rust's String): gff_utf8_valid here; on the device any byte >= 0x80 makes the row undecided
// The walk is one pass through five states -- key, gap, quoted value, bare value, after-value -- and the device kernels walk the
// same five.
#pragma once
#include "gff.h"

namespace exon {

// the attributes column of a run of rows: the three offset levels and the two byte pools of Map<Utf8, Utf8>
struct GTFAttrColumn : AttrColumn {
  std::vector<int32_t> map_off{0}, key_off{0}, val_off{0};  // rows -> entries -> (key bytes | value bytes)
  std::string keys, values;
  size_t rows() const override { return map_off.size() - 1; }
  void clear() override {
    map_off.assign(1, 0);
    key_off.assign(1, 0);
    val_off.assign(1, 0);
    keys.clear();
    values.clear();
  }
  void append(const char* k, size_t kn, const char* v, size_t vn) {
    keys.append(k, kn);
    key_off.push_back((int32_t)keys.size());
    values.append(v, vn);
    val_off.push_back((int32_t)values.size());
  }
  void close_row() { map_off.push_back((int32_t)key_off.size() - 1); }
  struct ArrowArray* slice(size_t o, size_t n) const override {
    const int32_t e0 = map_off[o], e1 = map_off[o + n];
    const int32_t k0 = key_off[(size_t)e0], k1 = key_off[(size_t)e1], v0 = val_off[(size_t)e0], v1 = val_off[(size_t)e1];
    auto rebased = [](const std::vector<int32_t>& v, int32_t from, int32_t to, int32_t base) {
      std::vector<int32_t> r((size_t)(to - from) + 1);
      for (size_t k = 0; k < r.size(); ++k) r[k] = v[(size_t)from + k] - base;
      return r;
    };
    auto arr = [] { return static_cast<struct ArrowArray*>(malloc(sizeof(struct ArrowArray))); };
    struct ArrowArray *ka = arr(), *va = arr(), *ea = arr(), *ma = arr();
    make_utf8(ka, rebased(key_off, e0, e1, k0), keys.substr((size_t)k0, (size_t)(k1 - k0)), {});
    make_utf8(va, rebased(val_off, e0, e1, v0), values.substr((size_t)v0, (size_t)(v1 - v0)), {});
    make_struct(ea, e1 - e0, {ka, va});
    make_list(ma, rebased(map_off, (int32_t)o, (int32_t)(o + n), e0), {}, ea);  // (a map's buffers are a list's: offsets over one child)
    return ma;
  }
};

// is the line (terminator and CR dropped) a row at all?  Throws for an empty line.
inline bool gtf_is_record(const char* line, size_t len) {
  if (len == 0) throw std::runtime_error("GTF: empty line");
  return line[0] != '#';
}

inline void parse_gtf_record(const char* line, size_t len, GFFRecord* r) { parse_gff_columns(line, len, r, true); }

// field 9 of record `r` by THE ATTRIBUTE RULES: validated, and appended to `sink` as one row when there is one
inline void parse_gtf_attributes(const char* line, size_t len, const GFFRecord& r, AttrColumn* sink) {
  GTFAttrColumn* col = static_cast<GTFAttrColumn*>(sink);
  const char* a = r.attr;
  const size_t n = r.attr_len;
  auto fail = [&](const std::string& what) { gff_fail(line, len, what, "GTF"); };
  auto emit = [&](size_t kb, size_t ke, size_t vb, size_t ve) {
    if (!gff_utf8_valid(std::string(a + kb, ke - kb))) fail("attribute key is not valid UTF-8");
    if (!gff_utf8_valid(std::string(a + vb, ve - vb))) fail("attribute value is not valid UTF-8");
    if (col) col->append(a + kb, ke - kb, a + vb, ve - vb);
  };
  enum { KEY, GAP, QUOTED, BARE, AFTER } st = KEY;
  size_t kb = 0, ke = 0, vb = 0, ve = 0;  // the key [kb, ke) and, in BARE, the value up to its last non-space byte [vb, ve)
  for (size_t i = 0; i < n; ++i) {
    const char c = a[i];
    switch (st) {
      case KEY:
        if (c == ' ') {
          if (i == kb) kb = i + 1;  // spaces in front of a key
          else ke = i, st = GAP;
        } else if (c == ';') {
          if (i == kb) fail("empty attribute (a ';' with nothing in front of it)");
          fail("attribute '" + std::string(a + kb, std::min<size_t>(i - kb, 60)) + "' has no value");
        }
        break;
      case GAP:
        if (c == ' ') break;
        if (c == ';') fail("attribute '" + std::string(a + kb, std::min<size_t>(ke - kb, 60)) + "' has no value");
        if (c == '"') vb = i + 1, st = QUOTED;
        else vb = i, ve = i + 1, st = BARE;
        break;
      case QUOTED:
        if (c == '"') {
          emit(kb, ke, vb, i);
          st = AFTER;
        }
        break;
      case BARE:
        if (c == ';') {
          emit(kb, ke, vb, ve);
          kb = i + 1;
          st = KEY;
        } else if (c != ' ') {
          ve = i + 1;
        }
        break;
      case AFTER:
        if (c == ';') kb = i + 1, st = KEY;
        else if (c != ' ') fail("attribute '" + std::string(a + kb, std::min<size_t>(ke - kb, 60)) + "': bytes behind the closing quote");
        break;
    }
  }
  if (st == KEY && kb < n) fail("attribute '" + std::string(a + kb, std::min<size_t>(n - kb, 60)) + "' has no value");
  if (st == GAP) fail("attribute '" + std::string(a + kb, std::min<size_t>(ke - kb, 60)) + "' has no value");
  if (st == QUOTED) fail("attribute '" + std::string(a + kb, std::min<size_t>(ke - kb, 60)) + "': missing closing quote");
  if (st == BARE) emit(kb, ke, vb, ve);
  if (col) col->close_row();
}

inline const GFFDialect* gtf_dialect() {
  static const GFFDialect d = {gtf_is_record, parse_gtf_record, parse_gtf_attributes, [] { return static_cast<AttrColumn*>(new GTFAttrColumn()); },
                               [] {  // Field::new_map("attributes", "entries", keys: Utf8 not null, values: Utf8 nullable, sorted = false), config.rs:28-41
                                 struct ArrowSchema* entries = new_nested_field("+s", "entries", false, {new_field("u", "keys", false), new_field("u", "values", true)});
                                 return new_nested_field("+m", "attributes", false, {entries});
                               },
                               "frame"};
  return &d;
}

// The GTF reader is the GFF reader with the GTF dialect: plain text, BGZF and gzip, threads, defer_decode, take_stream and
// data_offset are the shared machinery's.  (The reference has no indexed GTF table: exon_hip_scan_open refuses use_index.)
class GTFBatchReader : public GFFBatchReader {
 public:
  GTFBatchReader(const std::string& path, Compression c, GFFConfig cfg) : GFFBatchReader(path, c, std::move(cfg), gtf_dialect()) {}
};

}  // namespace exon
