// text_export.h -- the device-built text columns of a slab (text_nodes.h) on the host: which buffers come back and where they
// lie in one pinned block (text_plan, text_place), a batch's columns as views into the block (text_view), the rows a region keeps
// as arrays of their own (text_gather).  Host only and free of formats: every column is a tree of the four node kinds.
#pragma once
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "arrow_build.h"
#include "text_nodes.h"

namespace exon {

// zero offsets for nodes without offsets (the item-less `alt` lists): every batch of up to K_ZERO_ROWS rows points at the same
// static array; a scan of larger batches gets n_rows + 1 zeros in the slab's block
constexpr int64_t K_ZERO_ROWS = 65000;
inline const int32_t k_zero_offsets[K_ZERO_ROWS + 64] = {0};

// ---- plan: the device-to-host copies of a slab and each buffer's place in one block of 64-byte-aligned parts ----------------------
struct TextCopy {
  const void* src;  // nullptr: `bytes` zeros, nothing to copy
  size_t at, bytes;
};
struct TextPlan {
  std::vector<TextCopy> copies;
  size_t total = 64;
  void want(const void* src, size_t bytes) {  // a device buffer two nodes share is copied once
    for (TextCopy& c : copies)
      if (c.src == src) return;
    copies.push_back(TextCopy{src, total - 64, bytes});
    total += (bytes + 63) & ~(size_t)63;
  }
  const uint8_t* at(const uint8_t* base, const void* src) const {
    for (const TextCopy& c : copies)
      if (c.src == src) return base + c.at;
    return nullptr;
  }
};
inline size_t text_offsets_bytes(const ExonTextNode& nd) { return nd.kind == ExonTextNode::UTF8 || nd.kind == ExonTextNode::LIST ? ((size_t)nd.length + 1) * 4 : 0; }
inline size_t text_values_bytes(const ExonTextNode& nd) { return nd.kind == ExonTextNode::UTF8 ? (size_t)nd.n_values : nd.kind == ExonTextNode::INT64 ? (size_t)nd.n_values * 8 : 0; }
// slab_zeros: nodes without offsets get zeros of their own in the block (batches larger than k_zero_offsets)
inline TextPlan text_plan(const ExonTextColumns& dev, bool slab_zeros) {
  TextPlan p;
  size_t zeros = 0;
  for (int i = 0; i < dev.n_nodes; ++i) {
    const ExonTextNode& nd = dev.nodes[i];
    if (nd.offsets) p.want(nd.offsets, text_offsets_bytes(nd));
    else zeros = std::max(zeros, text_offsets_bytes(nd));
    if (nd.validity) p.want(nd.validity, ((size_t)nd.length + 7) / 8);
    if (nd.values) p.want(nd.values, text_values_bytes(nd));
  }
  if (slab_zeros && zeros) p.want(nullptr, zeros);
  return p;
}
// the same columns over the block at `base` (a node without offsets keeps nullptr unless the plan has slab-wide zeros)
inline ExonTextColumns text_place(const ExonTextColumns& dev, const TextPlan& p, const uint8_t* base) {
  ExonTextColumns h = dev;
  for (int i = 0; i < h.n_nodes; ++i) {
    ExonTextNode& nd = h.nodes[i];
    if (text_offsets_bytes(nd)) nd.offsets = reinterpret_cast<const int32_t*>(p.at(base, nd.offsets));
    if (nd.validity) nd.validity = p.at(base, nd.validity);
    if (nd.values) nd.values = p.at(base, nd.values);
  }
  return h;
}

// ---- view: rows [r0, r0 + n) of node i as an array of the arena; children are slab-wide, the cut is ArrowArray::offset -----------
inline struct ArrowArray* text_view(BatchArena* a, const ExonTextColumns& h, int i, int64_t r0, int64_t n) {
  const ExonTextNode& nd = h.nodes[i];
  struct ArrowArray* kid[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k)
    if (nd.kid[k] >= 0) kid[k] = text_view(a, h, nd.kid[k], 0, h.nodes[nd.kid[k]].length);
  const int64_t nulls = nd.validity ? -1 : 0;
  const void* off = nd.offsets ? nd.offsets : k_zero_offsets;
  switch (nd.kind) {
    case ExonTextNode::UTF8: return arena_array(a, n, r0, nulls, 3, nd.validity, off, nd.values ? nd.values : off);
    case ExonTextNode::INT64: return arena_array(a, n, r0, 0, 2, nullptr, nd.values, nullptr);
    case ExonTextNode::STRUCT2: return arena_struct2(a, n, kid[0], kid[1]);
    case ExonTextNode::LIST:
      if (nd.offsets) return arena_array(a, n, r0, nulls, 2, nd.validity, off, nullptr, kid[0]);
      // the shared zeros hold K_ZERO_ROWS rows: the bitmap from the byte the batch starts in, the offsets from their start
      return arena_array(a, n, r0 & 7, nulls, 2, nd.validity ? nd.validity + (r0 >> 3) : nullptr, off, nullptr, kid[0]);
  }
  return nullptr;
}

// ---- gather: the elements `ranges` name (runs [first, last) in order) of node i as an owned array ---------------------------------
typedef std::vector<std::pair<int64_t, int64_t>> TextRanges;
inline void text_ranges_add(TextRanges* r, int64_t a, int64_t z) {
  if (a == z) return;
  if (!r->empty() && r->back().second == a) r->back().second = z;
  else r->emplace_back(a, z);
}
// A validity bitmap is there where the node has one and a gathered element is NULL, as the typed builders make it (pack_validity)
inline struct ArrowArray* text_gather(const ExonTextColumns& h, int i, const TextRanges& ranges) {
  const ExonTextNode& nd = h.nodes[i];
  struct ArrowArray* out = static_cast<struct ArrowArray*>(malloc(sizeof *out));
  auto is_valid = [&](int64_t r) { return !nd.validity || ((nd.validity[(size_t)(r >> 3)] >> (r & 7)) & 1); };
  auto first = [&](int64_t r) { return nd.offsets ? nd.offsets[(size_t)r] : 0; };
  int64_t total = 0;
  for (const auto& g : ranges) total += g.second - g.first;
  std::vector<uint8_t> valid;
  if (nd.validity) valid.reserve((size_t)total);
  switch (nd.kind) {
    case ExonTextNode::UTF8: {
      std::vector<int32_t> offsets{0};
      offsets.reserve((size_t)total + 1);
      std::string data;
      for (const auto& g : ranges)
        for (int64_t r = g.first; r < g.second; ++r) {
          if (is_valid(r)) data.append(static_cast<const char*>(nd.values) + first(r), (size_t)(first(r + 1) - first(r)));
          offsets.push_back((int32_t)data.size());
          if (nd.validity) valid.push_back(is_valid(r));
        }
      make_utf8(out, offsets, data, valid);
      break;
    }
    case ExonTextNode::INT64: {
      std::vector<int64_t> v;
      v.reserve((size_t)total);
      for (const auto& g : ranges) v.insert(v.end(), static_cast<const int64_t*>(nd.values) + g.first, static_cast<const int64_t*>(nd.values) + g.second);
      make_primitive(out, v.data(), total, 8, {});
      break;
    }
    case ExonTextNode::STRUCT2: make_struct(out, total, {text_gather(h, nd.kid[0], ranges), text_gather(h, nd.kid[1], ranges)}); break;
    case ExonTextNode::LIST: {
      std::vector<int32_t> offsets{0};
      offsets.reserve((size_t)total + 1);
      TextRanges items;
      int32_t n_items = 0;
      for (const auto& g : ranges)
        for (int64_t r = g.first; r < g.second; ++r) {
          if (is_valid(r)) {  // (a NULL list takes no items, whatever its offsets say)
            text_ranges_add(&items, first(r), first(r + 1));
            n_items += first(r + 1) - first(r);
          }
          offsets.push_back(n_items);
          if (nd.validity) valid.push_back(is_valid(r));
        }
      make_list(out, offsets, valid, text_gather(h, nd.kid[0], items));
      break;
    }
  }
  return out;
}
// rows[0 .. n) of root node i
inline struct ArrowArray* text_gather_rows(const ExonTextColumns& h, int i, const int64_t* rows, int64_t n) {
  TextRanges ranges;
  for (int64_t k = 0; k < n; ++k) text_ranges_add(&ranges, rows[k], rows[k] + 1);
  return text_gather(h, i, ranges);
}

}  // namespace exon
