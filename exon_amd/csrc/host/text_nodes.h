// text_nodes.h -- one description of the string / list / map columns text_columns.hip builds on the device: what exon_text_*
// fill, what host/text_export.h copies back and cuts into batches.  Plain data, no HIP: internal.h includes it for the builders,
// text_export.h for the host side.
#pragma once
#include <cstdint>

// One Arrow array.  The builders fill it with device pointers; text_place() makes the same nodes over the pinned block.
struct ExonTextNode {
  enum Kind : uint8_t { UTF8, LIST, STRUCT2, INT64 };  // a map is a LIST over a STRUCT2 of keys and values
  Kind kind;
  int8_t kid[2];            // children by index (-1: none): a LIST's items, a STRUCT2's two fields
  int64_t length;
  const int32_t* offsets;   // [length + 1] of UTF8 and LIST; nullptr: all zero -- every list empty (VCF `alt`) and its item-less child
  const uint8_t* validity;  // bitmap; nullptr: never NULL
  const void* values;       // UTF8: n_values bytes; INT64: n_values (= length) items
  int64_t n_values;
};

// The projected columns of one slab: `roots` in schema order (an unprojected column is absent), children behind their parents'
// indexes.  Eight nodes cover every format (VCF id, ref, alt, info: six).  A node too many sets `overflow`, which the builders
// turn into EXON_HIP_ESTATE: nothing is dropped silently.
struct ExonTextColumns {
  static constexpr int MAX_NODES = 8, MAX_ROOTS = 5;
  ExonTextNode nodes[MAX_NODES];
  int8_t roots[MAX_ROOTS];
  int n_nodes = 0, n_roots = 0;
  bool overflow = false;

  int add(const ExonTextNode& nd) {
    if (n_nodes == MAX_NODES) {
      overflow = true;
      return -1;
    }
    nodes[n_nodes] = nd;
    return n_nodes++;
  }
  int utf8(int64_t length, const int32_t* offsets, const void* validity, const uint8_t* values, int64_t n_bytes) {
    return add(ExonTextNode{ExonTextNode::UTF8, {-1, -1}, length, offsets, static_cast<const uint8_t*>(validity), values, n_bytes});
  }
  int int64s(const int64_t* values, int64_t n) { return add(ExonTextNode{ExonTextNode::INT64, {-1, -1}, n, nullptr, nullptr, values, n}); }
  int list(int64_t length, const int32_t* offsets, const void* validity, int items) {
    return add(ExonTextNode{ExonTextNode::LIST, {(int8_t)items, -1}, length, offsets, static_cast<const uint8_t*>(validity), nullptr, 0});
  }
  int struct2(int64_t length, int k0, int k1) { return add(ExonTextNode{ExonTextNode::STRUCT2, {(int8_t)k0, (int8_t)k1}, length, nullptr, nullptr, nullptr, 0}); }
  // a list of strings, a map of strings to strings: the shapes more than one format has
  int list_utf8(int64_t length, const int32_t* offsets, const void* validity, int64_t n_items, const int32_t* item_offsets, const uint8_t* values, int64_t n_bytes) {
    return list(length, offsets, validity, utf8(n_items, item_offsets, nullptr, values, n_bytes));
  }
  void root(int node) {
    if (node < 0 || n_roots == MAX_ROOTS) overflow = true;
    else roots[n_roots++] = (int8_t)node;
  }
};
