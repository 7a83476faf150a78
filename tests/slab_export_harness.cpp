// slab_export_harness.cpp -- exon_amd/csrc/host/slab_export.h in a stand-alone program (tests/test_slab_export_harness.py builds it
// with AddressSanitizer and UndefinedBehaviorSanitizer): 19 hand-made rows of the fixed-width columns of every layout a scan has,
// their buffers exact-size heap copies standing in for the device's, through slab_plan into a block of exactly the planned size,
// then every row of the views and gathers the Python test asks for, printed -- and the runs scan of a few row masks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "host/slab_export.h"

namespace {

using exon::SlabChild;
using exon::SlabColumn;
using exon::SlabLayout;
constexpr int N = 19;
typedef std::vector<std::string> SL;

const int V1[N] = {1, 1, 0, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0};
const int V2[N] = {0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1};
const int FLAGV[N] = {1, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1};
const char* const NAME[N] = {"a", "bc", "", "d", "efg", "h", "ij", "k", "lmn", "", "o", "pq", "x", "r", "stu", "v", "w", "xyz", "end"};  // NULL where V2 is 0

std::vector<void*> g_heap;
template <class T>
const T* heap(const std::vector<T>& v) {  // the bytes of `v` in a heap block of exactly their size
  void* p = malloc(v.size() * sizeof(T));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  g_heap.push_back(p);
  return static_cast<const T*>(p);
}
const uint8_t* bitmap(const int* valid, int n) {
  std::vector<uint8_t> bm((size_t)(n + 7) / 8, 0);
  for (int r = 0; r < n; ++r)
    if (valid[r]) bm[(size_t)r >> 3] |= (uint8_t)(1u << (r & 7));
  return heap(bm);
}

// One layout with its 19 rows as the device parser would hold them: values (nullptr for a Flag) and validity per column
struct Case {
  std::string name;
  SlabLayout L;
  const void* values[exon::SLAB_MAX_COLS] = {};
  const uint8_t* validity[exon::SLAB_MAX_COLS] = {};
  exon::SlabDicts dicts;
  bool text = false;  // one text root (`name`, Utf8, NULL where V2 is 0)
  // column values: a dictionary id r % size, else a formula of (c, r) the Python side repeats
  int col(SlabColumn::Type t, const int* valid, const SL& dict = {}, bool device = false, int field = -1) {
    const int c = L.add(t, !dict.empty(), device, field);
    if (!dict.empty()) dicts.push_back(std::make_shared<const exon::SharedUtf8>(dict));
    std::vector<uint8_t> u8;
    std::vector<int32_t> i32;
    std::vector<float> f32;
    std::vector<int64_t> i64;
    for (int r = 0; r < N; ++r) {
      u8.push_back((uint8_t)((r * 13 + c) % 256));
      i32.push_back(dict.empty() ? 10 * r - 50 + c : r % (int)dict.size());
      f32.push_back((float)r * 0.5f - 2.0f + (float)c);
      i64.push_back(((int64_t)r + 1) * 4294967296ll + r + c);
    }
    values[c] = t == SlabColumn::U8 ? (const void*)heap(u8) : t == SlabColumn::I32 ? (const void*)heap(i32) : t == SlabColumn::F32 ? (const void*)heap(f32) : t == SlabColumn::I64 ? (const void*)heap(i64) : nullptr;
    validity[c] = valid ? bitmap(valid, N) : nullptr;
    return c;
  }
};

Case make_case(const std::string& name) {
  typedef SlabColumn C;
  Case k;
  k.name = name;
  if (name == "vcf") {
    k.col(C::I32, nullptr, {"chr1", "chr2", "chrX"});
    k.col(C::I64, V2);
    k.col(C::F32, V1);
    k.col(C::I32, nullptr, {"PASS", "q10", "q10;s50"}, true);
    k.col(C::I32, V1);
    k.col(C::F32, V2);
    k.col(C::FLAG, FLAGV);
    k.L.plain_children();
  } else if (name == "bam") {
    k.col(C::I32, nullptr);
    k.col(C::U8, V1);
    k.col(C::I32, V2, {"ref0", "ref1"});
    k.col(C::I64, V2);
    k.col(C::I64, V2);
    k.L.plain_children();
    k.text = true;
  } else if (name == "gff") {
    k.col(C::I32, nullptr, {"s1", "s2"}, true);
    k.col(C::I32, nullptr, {"src"}, true);
    k.col(C::I32, nullptr, {"gene", "exon", "CDS", "mRNA"}, true);
    k.col(C::I64, nullptr);
    k.col(C::I64, nullptr);
    k.col(C::F32, V1);
    k.col(C::I32, V1, {"+", "-"});
    k.col(C::I32, V2, {"0", "1", "2"});
    k.L.plain_children();
  } else if (name.rfind("bed_", 0) == 0) {  // bed_<letters>: n name, s score, t strand, z two NULL columns (thick_start Int64, color Utf8)
    const std::string p = name.substr(4);
    auto has = [&](char x) { return p.find(x) != std::string::npos; };
    k.col(C::I32, nullptr, {"chr1", "chr2"}, true);
    k.col(C::I64, nullptr);
    k.col(C::I64, nullptr);
    for (int c = 0; c < 3; ++c) k.L.child(SlabChild::FIXED, c);
    if (has('n')) k.L.child(SlabChild::TEXT, 0);
    if (has('s')) k.L.child(SlabChild::FIXED, k.col(C::I64, V1, {}, false, 4));
    if (has('t')) k.L.child(SlabChild::FIXED, k.col(C::I32, V2, {"+", "-"}, false, 5));
    if (has('z')) {
      k.L.child(SlabChild::NULL_I64, 6);
      k.L.child(SlabChild::NULL_UTF8, 8);
    }
    k.text = has('n');
  } else {
    fprintf(stderr, "unknown case %s\n", name.c_str());
    exit(2);
  }
  if ((int)k.dicts.size() != k.L.n_dicts) exit(3);
  return k;
}

// the block of rows [lo, hi) of the case, filled the way the exporter fills it: exactly the planned bytes, every copy out of an
// exact-size source
uint8_t* fill_block(const Case& k, exon::SlabPlan* p) {
  uint8_t* blk = static_cast<uint8_t*>(malloc(p->bytes));
  memset(blk, 0xAB, p->bytes);
  for (int c = 0; c < k.L.n_cols; ++c) {
    const size_t w = (size_t)k.L.cols[c].width();
    if (p->voff[c] % 64 || p->boff[c] % 64 || p->boff[c] + p->bits_bytes() > p->bytes) exit(5);
    if (w && k.values[c]) memcpy(blk + p->voff[c], static_cast<const uint8_t*>(k.values[c]) + (size_t)p->c_lo * w, (size_t)p->c_n * w);
    if (k.validity[c]) {
      memcpy(blk + p->boff[c], k.validity[c] + (p->c_lo >> 3), p->bits_bytes());
      p->has_bits |= 1u << c;
    }
  }
  if (p->zoff % 64 || p->zoff + p->zbytes != p->bytes) exit(5);
  if (p->zbytes) memset(blk + p->zoff, 0, p->zbytes);
  return blk;
}

bool is_valid(const struct ArrowArray* a, int64_t x) {
  const uint8_t* v = static_cast<const uint8_t*>(a->buffers[0]);
  return !v || ((v[x >> 3] >> (x & 7)) & 1);
}
void print_utf8(const struct ArrowArray* a, int64_t x) {
  const int32_t* off = static_cast<const int32_t*>(a->buffers[1]);
  printf("\"%.*s\"", (int)(off[x + 1] - off[x]), static_cast<const char*>(a->buffers[2]) + off[x]);
}
// type(length,offset,null_count,has a validity buffer)[dictionary] of every child, then every row
void print_batch(const char* head, const struct ArrowArray* batch, const SlabLayout& L, int n_text) {
  std::vector<char> types;
  for (int k = 0; k < L.n_children; ++k) {
    const SlabChild& ch = L.children[k];
    if (ch.kind == SlabChild::TEXT && ch.index >= n_text) continue;
    types.push_back(ch.kind == SlabChild::TEXT ? 'T' : ch.kind == SlabChild::NULL_UTF8 ? 'u' : ch.kind == SlabChild::NULL_I64 ? 'n' : "cifIb"[L.cols[ch.index].type]);
  }
  if ((int64_t)types.size() != batch->n_children) exit(4);
  printf("%s sig", head);
  for (size_t k = 0; k < types.size(); ++k) {
    const struct ArrowArray* a = batch->children[k];
    if (a->n_buffers != (types[k] == 'T' || types[k] == 'u' ? 3 : 2)) exit(4);
    printf(" %c(%lld,%lld,%lld,%d)", types[k], (long long)a->length, (long long)a->offset, (long long)a->null_count, a->buffers[0] ? 1 : 0);
    if (a->dictionary) {
      printf("[");
      for (int64_t i = 0; i < a->dictionary->length; ++i) {
        if (i) printf("|");
        print_utf8(a->dictionary, i);
      }
      printf("]");
    }
  }
  printf("\n");
  for (int64_t i = 0; i < batch->length; ++i) {
    printf("%s %lld", head, (long long)i);
    for (size_t k = 0; k < types.size(); ++k) {
      const struct ArrowArray* a = batch->children[k];
      const int64_t x = i + a->offset;
      printf("\t");
      if (!is_valid(a, x)) {
        printf("NULL");
        continue;
      }
      switch (types[k]) {
        case 'c': printf("%u", (unsigned)static_cast<const uint8_t*>(a->buffers[1])[x]); break;
        case 'i': printf("%d", static_cast<const int32_t*>(a->buffers[1])[x]); break;
        case 'f': printf("%g", (double)static_cast<const float*>(a->buffers[1])[x]); break;
        case 'I':
        case 'n': printf("%lld", (long long)static_cast<const int64_t*>(a->buffers[1])[x]); break;
        case 'b': printf("%s", (static_cast<const uint8_t*>(a->buffers[1])[x >> 3] >> (x & 7)) & 1 ? "true" : "false"); break;
        default: print_utf8(a, x); break;
      }
    }
    printf("\n");
  }
}

void print_runs(const char* name, const std::vector<uint8_t>& mask, int64_t n_rows) {
  const uint8_t* m = heap(mask);
  const exon::SlabRuns s = exon::slab_runs(m, n_rows);
  printf("R %s too_many=%d", name, s.too_many ? 1 : 0);
  if (!s.too_many) {
    printf(" kept=%lld runs=", (long long)s.kept);
    for (const auto& r : s.runs) printf("(%lld,%lld)", (long long)r.first, (long long)r.second);
    printf(" rows=");
    for (int64_t r : exon::slab_kept_rows(m, n_rows)) printf("%lld,", (long long)r);
  }
  printf("\n");
}

}  // namespace

int main() {
  static_assert(SlabColumn::U8 == 0 && SlabColumn::I32 == 1 && SlabColumn::F32 == 2 && SlabColumn::I64 == 3 && SlabColumn::FLAG == 4, "print_batch's letters");
  const int64_t cuts[6][2] = {{0, 19}, {0, 8}, {8, 8}, {16, 3}, {5, 9}, {18, 1}};
  std::vector<int64_t> all;
  for (int64_t r = 0; r < N; ++r) all.push_back(r);
  const std::pair<const char*, std::vector<int64_t>> lists[4] = {{"all", all}, {"last", {18}}, {"edges", {0, 7, 8, 15, 16, 18}}, {"hollow", {2, 7, 9}}};
  // the text root: offsets, bytes and bitmap of all 19 names
  std::vector<int32_t> name_off{0};
  std::vector<uint8_t> name_bytes;
  for (int r = 0; r < N; ++r) {
    if (V2[r]) name_bytes.insert(name_bytes.end(), NAME[r], NAME[r] + strlen(NAME[r]));
    name_off.push_back((int32_t)name_bytes.size());
  }
  const int32_t* h_off = heap(name_off);
  const uint8_t *h_bytes = heap(name_bytes), *h_valid = bitmap(V2, N);
  for (const char* name : {"vcf", "bam", "gff", "bed_", "bed_n", "bed_st", "bed_t", "bed_nstz"}) {
    const Case k = make_case(name);
    const SlabLayout& L = k.L;
    char head[96];
    // views: the whole slab cut six ways, then the span of one kept run that starts inside a byte (rows 11 .. 17: c_lo = 8)
    for (int span = 0; span < 2; ++span) {
      exon::SlabPlan plan = span ? exon::slab_plan(L, 11, 18) : exon::slab_plan(L, 0, N);
      uint8_t* blk = fill_block(k, &plan);
      printf("P %s %d c_lo=%lld c_n=%lld bytes=%zu zbytes=%zu\n", name, span, (long long)plan.c_lo, (long long)plan.c_n, plan.bytes, plan.zbytes);
      const int64_t one[1][2] = {{11, 7}};
      for (int q = 0; q < (span ? 1 : 6); ++q) {
        const int64_t b0 = span ? one[q][0] : cuts[q][0], n = span ? one[q][1] : cuts[q][1];
        exon::BatchArena* arena = exon::new_batch_arena(L.view_nodes() + (k.text ? 1 : 0), L.n_children, nullptr, nullptr, nullptr);
        std::vector<struct ArrowArray*> text, kids;
        if (k.text) text.push_back(exon::arena_array(arena, n, b0, -1, 3, h_valid, h_off, h_bytes));
        exon::slab_batch(arena, L, plan, blk, k.dicts, nullptr, b0, n, text, &kids);
        for (struct ArrowArray* a : kids)
          if (!a) exit(6);  // (the arena was sized from the layout)
        struct ArrowArray batch;
        exon::make_struct_of_arena(&batch, n, arena, kids);
        snprintf(head, sizeof head, "V %s %lld %lld", name, (long long)b0, (long long)n);
        print_batch(head, &batch, L, k.text ? 1 : 0);
        batch.release(&batch);
      }
      free(blk);
    }
    exon::SlabPlan plan = exon::slab_plan(L, 0, N);
    uint8_t* blk = fill_block(k, &plan);
    for (const auto& l : lists) {
      std::vector<struct ArrowArray*> text, kids;
      if (k.text) {
        exon::Utf8Builder b;
        for (int64_t r : l.second) {
          if (V2[r]) b.append_value(NAME[r]);
          else b.append_null();
        }
        text.push_back(b.finish());
      }
      exon::slab_batch(nullptr, L, plan, blk, k.dicts, l.second.data(), 0, (int64_t)l.second.size(), text, &kids);
      struct ArrowArray batch;
      exon::make_struct(&batch, (int64_t)l.second.size(), kids);
      snprintf(head, sizeof head, "G %s %s", name, l.first);
      print_batch(head, &batch, L, k.text ? 1 : 0);
      batch.release(&batch);
    }
    free(blk);
  }
  print_runs("ones", {0xFF, 0xFF, 0x07}, N);
  print_runs("zeros", {0, 0, 0}, N);
  print_runs("one", {0xE0, 0xFF, 0x01}, N);    // rows 5 .. 16, a whole byte inside
  print_runs("three", {0xC6, 0x03, 0x06}, N);  // rows 1-2, 6-9 (across a byte boundary), 17-18 (to the end)
  std::vector<uint8_t> many(65, 0);
  for (int r = 0; r <= 512; r += 2) many[(size_t)r >> 3] |= (uint8_t)(1u << (r & 7));  // 257 single-row runs over 520 rows
  print_runs("many", many, 520);
  many[64] = 0;  // 256 runs are still runs
  print_runs("most", many, 520);
  for (void* p : g_heap) free(p);
  return 0;
}
