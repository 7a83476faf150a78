// text_export_harness.cpp -- exon_amd/csrc/host/text_export.h in a stand-alone program (tests/test_text_export_harness.py builds it
// with AddressSanitizer and UndefinedBehaviorSanitizer): 19 hand-made rows of every column shape the device builders produce, their
// buffers exact-size heap copies standing in for the device's, through text_plan / text_place into a block of exactly the planned
// size, then every row of the views and gathers the Python test asks for, printed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "host/text_export.h"

namespace {

constexpr int N = 19;
typedef std::vector<std::string> SL;

const char* const UTF8N[N] = {"a", "bc", "", nullptr, "defg", "h", "ij", "k", "lmn", "", "o", "pq", nullptr, "r", "stu", "v", "w", "xyz", "end"};
const std::vector<std::optional<SL>> LISTN = {SL{"a"}, SL{"b", "c"}, SL{"", "d"}, std::nullopt, SL{"e"}, SL{}, SL{"f", "g", "h"}, SL{"i"}, SL{"j", ""}, SL{},
                                              SL{"k"}, SL{"l"}, std::nullopt, SL{"m", "n"}, SL{"o"}, SL{"p"}, SL{"q", "r"}, SL{""}, SL{"s", "t"}};
const int NOLIST[N] = {1, 1, 0, 0, 1, 1, 0, 1, 1, 1, 0, 1, 0, 1, 1, 0, 1, 1, 1};  // 1: an empty list, 0: NULL
const char* const SEQ[N] = {"ACGT", "A", "", "", "GG", "TTT", "C", "AC", "GTA", "", "N", "ACGTN", "", "T", "CA", "G", "TT", "ACG", "TA"};  // qual item j of row i: 100 i + j
const std::vector<std::vector<std::pair<std::string, std::string>>> MAP_UU = {
    {{"a", "1"}}, {{"b", "2"}, {"c", "3"}}, {}, {}, {{"d", ""}}, {{"e", "5"}}, {{"f", "6"}, {"g", "7"}, {"h", "8"}}, {{"i", "9"}}, {{"j", "10"}}, {},
    {{"k", "11"}}, {{"l", "12"}}, {}, {{"m", "13"}}, {{"n", "14"}}, {{"o", "15"}}, {{"p", "16"}}, {{"q", "17"}}, {{"r", "18"}, {"s", "19"}}};
const std::vector<std::vector<std::pair<std::string, SL>>> MAP_UL = {
    {{"a", {"1"}}}, {{"b", {"2", "3"}}, {"c", {}}}, {}, {}, {{"d", {""}}}, {{"e", {"5"}}}, {{"f", {"6", "7"}}, {"g", {"8"}}}, {{"h", {}}}, {{"i", {"9"}}}, {},
    {{"j", {"10"}}}, {{"k", {"11", "12"}}}, {}, {{"l", {"13"}}}, {{"m", {}}}, {{"n", {"14"}}}, {{"o", {"15"}}}, {{"p", {"16"}}}, {{"q", {"17"}}, {"r", {"18", "19"}}}};

std::vector<void*> g_heap;
// the bytes of `v` in a heap block of exactly their size
template <class T>
const T* heap(const std::vector<T>& v) {
  void* p = malloc(v.size() * sizeof(T));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  g_heap.push_back(p);
  return static_cast<const T*>(p);
}
struct Strings {  // offsets + bytes of a run of strings
  std::vector<int32_t> off{0};
  std::vector<uint8_t> bytes;
  void add(const std::string& s) {
    bytes.insert(bytes.end(), s.begin(), s.end());
    off.push_back((int32_t)bytes.size());
  }
  int node(ExonTextColumns* c, const void* validity) const { return c->utf8((int64_t)off.size() - 1, heap(off), validity, heap(bytes), (int64_t)bytes.size()); }
};
struct Bits {
  std::vector<uint8_t> bm = std::vector<uint8_t>((N + 7) / 8, 0);
  void set(int r) { bm[(size_t)r >> 3] |= (uint8_t)(1u << (r & 7)); }
};

ExonTextColumns make_case(const std::string& name) {
  ExonTextColumns c;
  if (name == "utf8n") {
    Strings s;
    Bits v;
    for (int r = 0; r < N; ++r) {
      s.add(UTF8N[r] ? UTF8N[r] : "");
      if (UTF8N[r]) v.set(r);
    }
    c.root(s.node(&c, heap(v.bm)));
  } else if (name == "listn") {
    Strings items;
    std::vector<int32_t> off{0};
    Bits v;
    for (int r = 0; r < N; ++r) {
      if (LISTN[(size_t)r]) {
        v.set(r);
        for (const std::string& s : *LISTN[(size_t)r]) items.add(s);
      }
      off.push_back((int32_t)items.off.size() - 1);
    }
    c.root(c.list(N, heap(off), heap(v.bm), items.node(&c, nullptr)));
  } else if (name == "nolist" || name == "nolist_slab") {
    Bits v;
    for (int r = 0; r < N; ++r)
      if (NOLIST[r]) v.set(r);
    c.root(c.list_utf8(N, nullptr, heap(v.bm), 0, nullptr, nullptr, 0));
  } else if (name == "shared") {
    Strings s;
    std::vector<int64_t> q;
    for (int r = 0; r < N; ++r) {
      s.add(SEQ[r]);
      for (size_t j = 0; j < strlen(SEQ[r]); ++j) q.push_back(100 * r + (int64_t)j);
    }
    const int32_t* off = heap(s.off);
    c.root(c.utf8(N, off, nullptr, heap(s.bytes), (int64_t)s.bytes.size()));
    c.root(c.list(N, off, nullptr, c.int64s(heap(q), (int64_t)q.size())));
  } else if (name == "map_uu") {
    Strings k, v;
    std::vector<int32_t> off{0};
    for (const auto& row : MAP_UU) {
      for (const auto& e : row) {
        k.add(e.first);
        v.add(e.second);
      }
      off.push_back((int32_t)k.off.size() - 1);
    }
    const int keys = k.node(&c, nullptr), values = v.node(&c, nullptr);
    c.root(c.list(N, heap(off), nullptr, c.struct2((int64_t)k.off.size() - 1, keys, values)));
  } else if (name == "map_ul") {
    Strings k, items;
    std::vector<int32_t> off{0}, list_off{0};
    for (const auto& row : MAP_UL) {
      for (const auto& e : row) {
        k.add(e.first);
        for (const std::string& s : e.second) items.add(s);
        list_off.push_back((int32_t)items.off.size() - 1);
      }
      off.push_back((int32_t)k.off.size() - 1);
    }
    const int keys = k.node(&c, nullptr);
    const int lists = c.list((int64_t)list_off.size() - 1, heap(list_off), nullptr, items.node(&c, nullptr));
    c.root(c.list(N, heap(off), nullptr, c.struct2((int64_t)k.off.size() - 1, keys, lists)));
  } else {
    fprintf(stderr, "unknown case %s\n", name.c_str());
    exit(2);
  }
  if (c.overflow) exit(3);
  return c;
}

// element i of `a` (before its offset), typed by node `nd` of `h`
void print_elem(const struct ArrowArray* a, const ExonTextColumns& h, int nd, int64_t i) {
  const ExonTextNode& t = h.nodes[nd];
  const int64_t x = i + a->offset;
  const uint8_t* valid = static_cast<const uint8_t*>(a->buffers[0]);
  if (valid && !((valid[x >> 3] >> (x & 7)) & 1)) {
    printf("NULL");
    return;
  }
  const int32_t* off = a->n_buffers > 1 ? static_cast<const int32_t*>(a->buffers[1]) : nullptr;
  switch (t.kind) {
    case ExonTextNode::UTF8: printf("\"%.*s\"", (int)(off[x + 1] - off[x]), static_cast<const char*>(a->buffers[2]) + off[x]); break;
    case ExonTextNode::INT64: printf("%lld", (long long)static_cast<const int64_t*>(a->buffers[1])[x]); break;
    case ExonTextNode::STRUCT2:
      print_elem(a->children[0], h, t.kid[0], x);
      printf(":");
      print_elem(a->children[1], h, t.kid[1], x);
      break;
    case ExonTextNode::LIST:
      printf("[");
      for (int32_t j = off[x]; j < off[x + 1]; ++j) {
        if (j > off[x]) printf(",");
        print_elem(a->children[0], h, t.kid[0], j);
      }
      printf("]");
      break;
  }
}
// kind(length,null_count,has a validity buffer)[children]
void print_sig(const struct ArrowArray* a, const ExonTextColumns& h, int nd) {
  const ExonTextNode& t = h.nodes[nd];
  printf("%c(%lld,%lld,%d)", "ULSI"[t.kind], (long long)a->length, (long long)a->null_count, a->buffers[0] ? 1 : 0);
  if (a->n_children != (t.kind == ExonTextNode::LIST ? 1 : t.kind == ExonTextNode::STRUCT2 ? 2 : 0)) exit(4);
  if (a->n_children) printf("[");
  for (int64_t k = 0; k < a->n_children; ++k) {
    if (k) printf(",");
    print_sig(a->children[k], h, t.kid[k]);
  }
  if (a->n_children) printf("]");
}
void print_batch(const char* head, const struct ArrowArray* batch, const ExonTextColumns& h) {
  printf("%s sig", head);
  for (int k = 0; k < h.n_roots; ++k) {
    printf(" ");
    print_sig(batch->children[k], h, h.roots[k]);
  }
  printf("\n");
  for (int64_t i = 0; i < batch->length; ++i) {
    printf("%s %lld", head, (long long)i);
    for (int k = 0; k < h.n_roots; ++k) {
      printf("\t");
      print_elem(batch->children[k], h, h.roots[k], i);
    }
    printf("\n");
  }
}

}  // namespace

int main() {
  static_assert(ExonTextNode::UTF8 == 0 && ExonTextNode::LIST == 1 && ExonTextNode::STRUCT2 == 2 && ExonTextNode::INT64 == 3, "print_sig's letters");
  const int64_t cuts[6][2] = {{0, 19}, {0, 8}, {8, 8}, {16, 3}, {5, 9}, {18, 1}};
  std::vector<int64_t> all;
  for (int64_t r = 0; r < N; ++r) all.push_back(r);
  const std::pair<const char*, std::vector<int64_t>> lists[4] = {{"all", all}, {"last", {18}}, {"edges", {0, 7, 8, 15, 16, 18}}, {"hollow", {3, 9, 12}}};
  for (const char* name : {"utf8n", "listn", "nolist", "nolist_slab", "shared", "map_uu", "map_ul"}) {
    const ExonTextColumns dev = make_case(name);
    const exon::TextPlan plan = exon::text_plan(dev, std::string(name) == "nolist_slab");
    size_t buffers = 0, bytes = 0;
    for (int i = 0; i < dev.n_nodes; ++i) buffers += (dev.nodes[i].offsets != nullptr) + (dev.nodes[i].validity != nullptr) + (dev.nodes[i].values != nullptr);
    uint8_t* blk = static_cast<uint8_t*>(malloc(plan.total));
    memset(blk, 0xAB, plan.total);
    for (const exon::TextCopy& c : plan.copies) {
      bytes += c.bytes;
      if (c.at % 64 || c.at + c.bytes > plan.total) exit(5);
      if (c.src) memcpy(blk + c.at, c.src, c.bytes);  // (reads exactly the bytes the plan names from an exact-size source)
      else memset(blk + c.at, 0, c.bytes);
    }
    printf("P %s copies=%zu buffers=%zu bytes=%zu total=%zu\n", name, plan.copies.size(), buffers, bytes, plan.total);
    const ExonTextColumns h = exon::text_place(dev, plan, blk);
    char head[96];
    for (const auto& cut : cuts) {
      exon::BatchArena* arena = exon::new_batch_arena(h.n_nodes + 1, h.n_roots, nullptr, nullptr, nullptr);
      std::vector<struct ArrowArray*> kids;
      for (int k = 0; k < h.n_roots; ++k) kids.push_back(exon::text_view(arena, h, h.roots[k], cut[0], cut[1]));
      for (struct ArrowArray* a : kids)
        if (!a) exit(6);  // (the arena was sized from the container)
      struct ArrowArray batch;
      exon::make_struct_of_arena(&batch, cut[1], arena, kids);
      snprintf(head, sizeof head, "V %s %lld %lld", name, (long long)cut[0], (long long)cut[1]);
      print_batch(head, &batch, h);
      batch.release(&batch);
    }
    for (const auto& l : lists) {
      std::vector<struct ArrowArray*> kids;
      for (int k = 0; k < h.n_roots; ++k) kids.push_back(exon::text_gather_rows(h, h.roots[k], l.second.data(), (int64_t)l.second.size()));
      struct ArrowArray batch;
      exon::make_struct(&batch, (int64_t)l.second.size(), kids);
      snprintf(head, sizeof head, "G %s %s", name, l.first);
      print_batch(head, &batch, h);
      batch.release(&batch);
    }
    free(blk);
  }
  for (void* p : g_heap) free(p);
  return 0;
}
