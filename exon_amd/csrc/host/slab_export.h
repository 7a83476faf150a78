// slab_export.h -- the fixed-width columns of a slab on the host: what a scan's batches look like (SlabLayout, filled once per scan
// by scan.cpp's slab_layout), where every column lies in one pinned block (slab_plan), a batch's columns as views into the block
// (slab_view), the rows a region keeps as arrays of their own (slab_gather), a batch's children in order (slab_batch), the runs of
// kept rows in a row mask (slab_runs).  Host only and free of formats, the sibling of text_export.h: a column is an Arrow type, its
// width and maybe a dictionary.
#pragma once
#include <utility>
#include <vector>

#include "arrow_build.h"
#include "text_nodes.h"

namespace exon {

constexpr int SLAB_MAX_COLS = 4 + EXON_HIP_MAX_INFO_FIELDS, SLAB_MAX_TEXT = ExonTextColumns::MAX_ROOTS, SLAB_MAX_CHILDREN = SLAB_MAX_COLS + SLAB_MAX_TEXT;

// ---- layout: the scan's fixed-width columns and the order of a batch's children ----------------------------------------------------
struct SlabColumn {
  enum Type : uint8_t { U8, I32, F32, I64, FLAG };  // FLAG: no values, the bitmap is the value (Boolean: true where present, else NULL)
  Type type = I32;
  int8_t dict = -1;           // its dictionary in the slab's dictionary list (-1: none)
  bool device_names = false;  // ... whose names the device parser builds (else the host reader has them)
  int8_t field = -1;          // opaque here: what scan.cpp's slab_layout notes for parse_slab / device_names (BED: the schema's field, 4 score, 5 strand; VCF: the parser's INFO key)
  int8_t child = -1;          // where it stands among a batch's children
  int width() const { return type == FLAG ? 0 : type == U8 ? 1 : type == I64 ? 8 : 4; }
};
struct SlabChild {
  enum Kind : uint8_t { FIXED, TEXT, NULL_UTF8, NULL_I64 };  // fixed column `index`; text root `index` (skipped when the slab has fewer); NULL on every row
  Kind kind;
  int8_t index;
};
struct SlabLayout {
  int n_cols = 0, n_dicts = 0, n_children = 0, n_nulls = 0;
  SlabColumn cols[SLAB_MAX_COLS];
  SlabChild children[SLAB_MAX_CHILDREN];
  int region_col = -1;         // the child that holds the contig / reference dictionary a region is named in
  bool text_unkept = false;    // the text columns are built for a slab that keeps no row too (their build validates every record)
  int add(SlabColumn::Type t, bool dict = false, bool device_names = false, int field = -1) {
    SlabColumn& c = cols[n_cols];
    c.type = t;
    c.dict = dict ? (int8_t)n_dicts++ : (int8_t)-1;
    c.device_names = device_names;
    c.field = (int8_t)field;
    return n_cols++;
  }
  // one column a character: C u8, i i32, f f32, l i64, b Flag; H / D: i32 ids of a dictionary the host reader / the device parser builds
  void add(const char* spec) {
    for (; *spec; ++spec)
      add(*spec == 'C' ? SlabColumn::U8 : *spec == 'f' ? SlabColumn::F32 : *spec == 'l' ? SlabColumn::I64 : *spec == 'b' ? SlabColumn::FLAG : SlabColumn::I32, *spec == 'H' || *spec == 'D', *spec == 'D');
  }
  void child(SlabChild::Kind k, int index) {
    if (k == SlabChild::FIXED) cols[index].child = (int8_t)n_children;
    children[n_children++] = SlabChild{k, (int8_t)index};
    n_nulls += k == SlabChild::NULL_UTF8 || k == SlabChild::NULL_I64;
  }
  void plain_children() {  // every fixed column, then every text root the builders can make
    for (int c = 0; c < n_cols; ++c) child(SlabChild::FIXED, c);
    for (int k = 0; k < SLAB_MAX_TEXT; ++k) child(SlabChild::TEXT, k);
  }
  int view_nodes() const { return n_cols + n_dicts + n_nulls + 1; }  // arena nodes of a batch of views: columns, dictionaries, NULL columns, the struct
};
typedef std::vector<std::shared_ptr<const SharedUtf8>> SlabDicts;  // by SlabColumn::dict

// ---- plan: rows [c_lo, c_lo + c_n) of every column in one block of 64-byte-aligned parts -------------------------------------------
struct SlabPlan {
  int64_t c_lo = 0, c_n = 0;  // c_lo a multiple of 8: bitmaps are cut at a byte
  size_t voff[SLAB_MAX_COLS], boff[SLAB_MAX_COLS];  // per column: values, validity bitmap
  size_t moff = 0;               // the slab's row mask (gathered slabs)
  size_t zoff = 0, zbytes = 0;   // NULL columns: one run of zeros serves them all as validity bitmap (every row NULL), offsets and values
  size_t bytes = 0;
  uint32_t has_bits = 0;         // bit c: column c came with a validity bitmap (set by whoever fills the block)
  size_t bits_bytes() const { return (size_t)(c_n + 7) / 8; }
};
inline SlabPlan slab_plan(const SlabLayout& L, int64_t lo, int64_t hi) {
  SlabPlan p;
  p.c_lo = lo & ~int64_t(7);
  p.c_n = hi - p.c_lo;
  const size_t nb = (p.bits_bytes() + 63) & ~size_t(63);
  for (int c = 0; c < L.n_cols; ++c) {
    p.voff[c] = p.bytes;
    p.bytes += ((size_t)p.c_n * (size_t)L.cols[c].width() + 63) & ~size_t(63);
    p.boff[c] = p.bytes;
    p.bytes += nb;
  }
  p.moff = p.bytes;
  p.bytes += nb;
  p.zoff = p.bytes;
  p.zbytes = L.n_nulls ? (((size_t)p.c_n + 1) * 8 + 63) & ~size_t(63) : 0;
  p.bytes += p.zbytes;
  return p;
}

// ---- view: rows [b0, b0 + n) of fixed column c as an array of the arena.  The bitmap is the slab's (where there is one the null
// count is left to the consumer); a Flag's values are its bitmap -----------------------------------------------------------------------
inline struct ArrowArray* slab_view(BatchArena* a, const SlabLayout& L, const SlabPlan& p, const uint8_t* blk, const SlabDicts& dicts, int c, int64_t b0, int64_t n) {
  const void* bits = (p.has_bits >> c) & 1 ? blk + p.boff[c] : nullptr;
  const void* vals = L.cols[c].width() ? (const void*)(blk + p.voff[c]) : bits;
  struct ArrowArray* dict = L.cols[c].dict >= 0 ? arena_dictionary(a, *dicts[(size_t)L.cols[c].dict]) : nullptr;
  return arena_array(a, n, b0 - p.c_lo, bits ? -1 : 0, 2, bits, vals, nullptr, nullptr, dict);
}

// ---- gather: rows[0 .. n) of fixed column c (of a slab planned from row 0) as an owned array of the layout's type: exact null
// count, a bitmap where a gathered row is NULL; a Flag becomes a Boolean, true where present and NULL elsewhere ------------------------
inline struct ArrowArray* slab_gather(const SlabLayout& L, const SlabPlan& p, const uint8_t* blk, const SlabDicts& dicts, int c, const int64_t* rows, int64_t n) {
  const uint8_t* bits = (p.has_bits >> c) & 1 ? blk + p.boff[c] : nullptr;
  const size_t w = (size_t)L.cols[c].width();
  std::vector<uint8_t> valid((size_t)n, 1), vals((size_t)n * w);
  for (int64_t i = 0; bits && i < n; ++i) valid[(size_t)i] = (bits[(size_t)(rows[i] >> 3)] >> (rows[i] & 7)) & 1;
  auto take = [&](auto tag) {  // (a loop of its own per width: a copy of a width known at run time only made the gather a quarter slower)
    typedef decltype(tag) T;
    for (int64_t i = 0; i < n; ++i) reinterpret_cast<T*>(vals.data())[i] = reinterpret_cast<const T*>(blk + p.voff[c])[rows[i]];
  };
  if (w) w == 1 ? take(uint8_t()) : w == 4 ? take(uint32_t()) : take(uint64_t());
  struct ArrowArray* out = static_cast<struct ArrowArray*>(malloc(sizeof *out));
  if (!w) make_boolean(out, valid, valid);
  else make_primitive(out, vals.data(), n, (int)w, valid, L.cols[c].dict >= 0 ? shared_utf8_array(dicts[(size_t)L.cols[c].dict]) : nullptr);
  return out;
}
inline struct ArrowArray* slab_null_column(bool utf8, int64_t n) {  // n NULL rows, owned
  struct ArrowArray* a = static_cast<struct ArrowArray*>(malloc(sizeof *a));
  const std::vector<uint8_t> valid((size_t)n, 0);
  if (utf8) make_utf8(a, std::vector<int32_t>((size_t)n + 1, 0), std::string(), valid);
  else make_primitive(a, std::vector<int64_t>((size_t)n, 0).data(), n, 8, valid);
  return a;
}

// ---- batch: the children of one batch in the layout's order, appended to `kids`: views of rows [b0, b0 + n) in arena `a`, or
// (rows != nullptr) rows[0 .. n) gathered; `text` are the batch's text roots, made the same way ---------------------------------------
inline void slab_batch(BatchArena* a, const SlabLayout& L, const SlabPlan& p, const uint8_t* blk, const SlabDicts& dicts, const int64_t* rows, int64_t b0, int64_t n,
                       const std::vector<struct ArrowArray*>& text, std::vector<struct ArrowArray*>* kids) {
  const uint8_t* z = blk + p.zoff;  // (a NULL column's view: every buffer the same zeros; Utf8 has three of them)
  for (int k = 0; k < L.n_children; ++k) {
    const int c = L.children[k].index;
    const bool utf8 = L.children[k].kind == SlabChild::NULL_UTF8;
    switch (L.children[k].kind) {
      case SlabChild::FIXED: kids->push_back(rows ? slab_gather(L, p, blk, dicts, c, rows, n) : slab_view(a, L, p, blk, dicts, c, b0, n)); break;
      case SlabChild::TEXT:
        if ((size_t)c < text.size()) kids->push_back(text[(size_t)c]);
        break;
      default: kids->push_back(rows ? slab_null_column(utf8, n) : arena_array(a, n, 0, n, utf8 ? 3 : 2, z, z, utf8 ? z : nullptr));
    }
  }
}

// ---- runs: the runs [first, last) of consecutive kept rows of a row mask (bits behind n_rows clear): one for a point region over
// a sorted file, a handful when reads reach into it from the left.  too_many: more than SLAB_MAX_RUNS, `kept` and `runs` incomplete
constexpr size_t SLAB_MAX_RUNS = 256;
struct SlabRuns {
  std::vector<std::pair<int64_t, int64_t>> runs;
  int64_t kept = 0;
  bool too_many = false;
};
inline SlabRuns slab_runs(const uint8_t* mask, int64_t n_rows) {
  SlabRuns s;
  const size_t n_bytes = (size_t)(n_rows + 7) / 8;
  int64_t open_lo = -1;
  for (size_t byte = 0; byte < n_bytes && !s.too_many; ++byte) {
    const uint8_t m = mask[byte];
    if (m == 0xFF) {
      if (open_lo < 0) open_lo = (int64_t)byte * 8;
      s.kept += 8;
      continue;
    }
    if (m == 0 && open_lo < 0) continue;
    for (int b = 0; b < 8; ++b) {
      const int64_t r = (int64_t)byte * 8 + b;
      if ((m >> b) & 1) {
        if (open_lo < 0) open_lo = r;
        ++s.kept;
      } else if (open_lo >= 0) {
        s.runs.emplace_back(open_lo, r);
        open_lo = -1;
        if (s.runs.size() > SLAB_MAX_RUNS) s.too_many = true;
      }
    }
  }
  if (open_lo >= 0) s.runs.emplace_back(open_lo, n_rows);
  return s;
}
inline std::vector<int64_t> slab_kept_rows(const uint8_t* mask, int64_t n_rows) {  // the kept rows themselves
  std::vector<int64_t> keep;
  for (int64_t r = 0; r < n_rows; ++r)
    if ((mask[(size_t)(r >> 3)] >> (r & 7)) & 1) keep.push_back(r);
  return keep;
}

}  // namespace exon
