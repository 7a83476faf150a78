// cigar_blocks.h -- THE RULE that turns one alignment record into its aligned blocks, stated once for the host and the device
// (DESIGN.md 3.9).  No includes beyond <stdint.h>, no allocation: tests/cigar_blocks_host_harness.cpp compiles it alone.
//
//   ops        BAM encoding, `len << 4 | code`; code i is "MIDNSHP=X"[i] for i < 9, codes 9 .. 15 have no letter.
//   cover_ops  bit i = "positions under an op of code i are covered".  Legal bits are the reference-consuming ops M(0) D(2) N(3)
//              =(7) X(8): a non-empty subset of COVER_OPS_LEGAL = 0x18D.
//
//   THE WALK.  pos = start.  An op whose code is in 0x18D advances pos by its length, counted or not; every other op (I, S, H, P and
//   the codes 9 .. 15) advances nothing, as the readers' `end` does.  The covered positions are the union of the counted ops'
//   intervals; a BLOCK is a maximal run of consecutive covered positions.  So 10M5I10M is one block, 5M0N5M is one block, 5M3D5M with
//   D uncounted is two, a zero-length counted op makes none, and a record yields k >= 0 blocks, in increasing order, never touching.
//
//   ONE FUNCTION, walk_blocks, templated on where the ops come from and on what is done with a block: the count pass and the fill
//   pass of cigar_blocks.hip, the host readers (formats.h) and exon_hip_cigar_blocks_host all call it, so they cannot disagree.  An
//   op source is a cursor, `bool next(uint32_t* op)`, taken by value: aligned u32 (ArrayOps: Arrow list items), the unaligned u32 of
//   a BAM record (ByteOps), the text of a SAM line's sixth field (TextOps).
//
//   Positions are int64 and the sums run modulo 2^64 (unsigned adds): start + the op lengths of a record of BAM's limits (65 535 ops
//   of at most 2^28 - 1) stays far inside; a caller's own list may not, and then wraps the same way everywhere.
//
//   DECISIONS
//   (a) CG-tag placeholder.  A BAM record whose CIGAR is exactly two ops, `<l_seq>S` then `<n>N`, keeps its real ops in a CG tag that
//       this library does not read.  is_cg_placeholder names it; in blocks mode the host reader throws an error that names the tag
//       and the device marks the record undecided, so that the host reader reports it: never a record of zero coverage.  The
//       list-form operator has no l_seq and cannot see it: its caller's columns are taken as they are.
//   (b) SAM op length.  BAM's own limit is OP_LEN_MAX = 2^28 - 1 and the u32 encoding cannot hold a longer op.  In blocks mode a SAM
//       op longer than that, an op without digits, digits without an op and a letter outside MIDNSHP=X are all refused by
//       text_ops_ok: undecided on the device, `invalid CIGAR '...'` from the host reader.  ('*' is no CIGAR: no ops.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EXON_CIGAR_HD __host__ __device__
#else
#define EXON_CIGAR_HD
#endif

namespace exon {
namespace cigar {

constexpr uint32_t COVER_OPS_LEGAL = 0x18D;  // M D N = X
constexpr uint32_t OP_LEN_MAX = (1u << 28) - 1;

EXON_CIGAR_HD inline bool cover_ops_ok(uint32_t cover_ops) { return cover_ops != 0 && (cover_ops & ~COVER_OPS_LEGAL) == 0; }

// ops[0 .. n) in memory that may be read as aligned u32
struct ArrayOps {
  const uint32_t* ops;
  uint32_t n;
  EXON_CIGAR_HD bool next(uint32_t* op) {
    if (!n) return false;
    *op = *ops++;
    --n;
    return true;
  }
};
// n little-endian u32 at any byte address (a BAM record's CIGAR in the slab)
struct ByteOps {
  const uint8_t* p;
  uint32_t n;
  EXON_CIGAR_HD bool next(uint32_t* op) {
    if (!n) return false;
    *op = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    p += 4;
    --n;
    return true;
  }
};
EXON_CIGAR_HD inline int op_code_of(uint8_t ch) {
  switch (ch) {
    case 'M': return 0;
    case 'I': return 1;
    case 'D': return 2;
    case 'N': return 3;
    case 'S': return 4;
    case 'H': return 5;
    case 'P': return 6;
    case '=': return 7;
    case 'X': return 8;
    default: return -1;
  }
}
// the text [p, end) of a SAM CIGAR that text_ops_ok has accepted
struct TextOps {
  const uint8_t *p, *end;
  EXON_CIGAR_HD bool next(uint32_t* op) {
    if (p >= end) return false;
    uint32_t len = 0;
    while (*p >= '0' && *p <= '9') len = len * 10 + (uint32_t)(*p++ - '0');
    *op = len << 4 | (uint32_t)op_code_of(*p++);
    return true;
  }
};
// DECISION (b).  "*" is accepted (and must be handed to TextOps as the empty text).
EXON_CIGAR_HD inline bool text_ops_ok(const uint8_t* p, const uint8_t* end) {
  if (end - p == 1 && *p == '*') return true;
  if (p == end) return false;
  while (p < end) {
    uint64_t len = 0;
    int digits = 0;
    while (p < end && *p >= '0' && *p <= '9' && digits < 10) len = len * 10 + (uint64_t)(*p++ - '0'), ++digits;
    if (!digits || len > OP_LEN_MAX || p == end || op_code_of(*p) < 0) return false;
    ++p;
  }
  return true;
}
// DECISION (a): the two-op stand-in of a CIGAR that lives in the CG tag
EXON_CIGAR_HD inline bool is_cg_placeholder(ByteOps ops, uint32_t l_seq) {
  uint32_t a = 0, b = 0;
  return ops.n == 2 && ops.next(&a) && ops.next(&b) && a == (l_seq << 4 | 4u) && (b & 15u) == 3u;
}

// emit(j, first, last) is called for block j = 0, 1, ... with its inclusive ends.  Returns k.
template <typename Ops, typename Emit>
EXON_CIGAR_HD inline uint32_t walk_blocks(Ops ops, int64_t start, uint32_t cover_ops, Emit&& emit) {
  uint64_t pos = (uint64_t)start, first = 0, stop = 0;  // the open block is [first, stop)
  bool open = false;
  uint32_t k = 0, v;
  while (ops.next(&v)) {
    const uint32_t code = v & 15u, len = v >> 4;
    if (!((COVER_OPS_LEGAL >> code) & 1u)) continue;
    if (len && ((cover_ops >> code) & 1u)) {
      if (!(open && stop == pos)) {  // (pos never goes back: an open block that does not end here ended before)
        if (open) emit(k++, (int64_t)first, (int64_t)(stop - 1));
        first = pos;
        open = true;
      }
      stop = pos + len;
    }
    pos += len;
  }
  if (open) emit(k++, (int64_t)first, (int64_t)(stop - 1));
  return k;
}

template <typename Ops>
EXON_CIGAR_HD inline uint32_t count_blocks(Ops ops, int64_t start, uint32_t cover_ops) {
  return walk_blocks(ops, start, cover_ops, [](uint32_t, int64_t, int64_t) {});
}

// the blocks of one record into out_start / out_end, the first min(k, cap) of them; returns k
template <typename Ops>
EXON_CIGAR_HD inline uint32_t fill_blocks(Ops ops, int64_t start, uint32_t cover_ops, int64_t* out_start, int64_t* out_end, uint32_t cap) {
  return walk_blocks(ops, start, cover_ops, [=](uint32_t j, int64_t a, int64_t b) {
    if (j < cap) out_start[j] = a, out_end[j] = b;
  });
}

}  // namespace cigar
}  // namespace exon
