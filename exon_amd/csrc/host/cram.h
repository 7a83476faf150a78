// cram.h -- CRAM 3.0 / 3.1 front end (host): containers -> slices -> records -> the BAM device layout (flag, mapq, reference id,
// start, end), so that the fused kernels K3 / K6 run on CRAM input as they do on BAM / SAM.
//
// Replaces exon-cram/src/{async_batch_stream,array_builder}.rs (columns of the schema shared by SAM, BAM and CRAM:
// exon-sam/src/schema_builder.rs:371-402) and the noodles-cram reader underneath (absent from /root/reference; restated from
// the published CRAM 3.0 specification).  What the path needs is decoded -- BF, CF, RI, RL, AP, RG, RN, the mate fields, the tag
// line, the read features (for the reference span), MQ -- everything else is consumed to keep the streams in step.  The
// reference sequence is NOT needed for these columns (the reference opens it to rebuild the bases; a missing FASTA is an error
// there and irrelevant here).
//   block codecs   raw, gzip, rANS 4x8 orders 0 and 1 (what htslib writes by default and the reference's fixtures use), and
//                  bzip2 / lzma (methods 2 / 3: htslib's use_bzip2 / use_lzma and its archive profile) through the system's
//                  libbz2.so.1.0 / liblzma.so.5, bound at first use with dlopen (this image ships the runtime libraries but not
//                  their headers; without them such a block is an error); CRAM 3.1's rANS Nx16 (method 5: htslib's default
//                  entropy coder since 1.22) with all of its transforms.  The other 3.1 codecs -- adaptive arithmetic coder 6,
//                  fqzcomp 7, name tokeniser 8 -- are an error naming the codec, and only when a series this path READS sits in
//                  such a block: htslib uses 7 and 8 for quality scores and read names, which stay closed (lazy blocks)
//   encodings      EXTERNAL, HUFFMAN, BETA, BYTE_ARRAY_LEN, BYTE_ARRAY_STOP (GOLOMB / SUBEXP / GAMMA are CRAM 2 leftovers -> error)
// Every length is checked against the bytes in hand; a malformed file is an error, never a read past a buffer.
#pragma once
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <dlfcn.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <future>
#include <thread>
#include <utility>
#include <vector>

#include "formats.h"

namespace exon {
namespace cram {

// a byte of the file inside an error message: itself when printable ASCII, \\xHH otherwise
inline std::string printable(char ch) {
  const unsigned char u = (unsigned char)ch;
  if (u >= 0x20 && u < 0x7F) return std::string(1, ch);
  char buf[8];
  snprintf(buf, sizeof buf, "\\x%02X", u);
  return buf;
}

struct Cursor {  // bounds-checked reads from a byte buffer
  const uint8_t* p;
  size_t n, o = 0;
  Cursor(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
  uint8_t u8() {
    if (o >= n) throw std::runtime_error("CRAM: truncated data");
    return p[o++];
  }
  void need(size_t k) const {
    if (k > n - o) throw std::runtime_error("CRAM: truncated data");
  }
  int32_t i32le() {
    need(4);
    int32_t v;
    memcpy(&v, p + o, 4);
    o += 4;
    return v;
  }
  uint32_t itf8() {
    const uint32_t v = u8();
    if (v < 0x80) return v;
    if (v < 0xC0) return ((v & 0x3F) << 8) | u8();
    if (v < 0xE0) {
      const uint32_t a = u8(), b = u8();
      return ((v & 0x1F) << 16) | (a << 8) | b;
    }
    if (v < 0xF0) {
      const uint32_t a = u8(), b = u8(), c = u8();
      return ((v & 0x0F) << 24) | (a << 16) | (b << 8) | c;
    }
    const uint32_t a = u8(), b = u8(), c = u8(), d = u8();
    return ((v & 0x0F) << 28) | (a << 20) | (b << 12) | (c << 4) | (d & 0x0F);
  }
  int32_t itf8s() { return (int32_t)itf8(); }
  uint64_t ltf8() {
    const uint32_t v = u8();
    int k = 0;
    while (k < 8 && ((v << k) & 0x80)) ++k;
    uint64_t val = k < 7 ? (v & (0xFFu >> (k + 1))) : 0;
    for (int i = 0; i < k; ++i) val = (val << 8) | u8();
    return val;
  }
  void skip(size_t k) {
    need(k);
    o += k;
  }
};

// ---- rANS 4x8 (CRAM 3.0 section 13): four interleaved states, 12-bit frequencies, byte renormalisation ------------------
struct RansTable {
  uint16_t F[256], C[257];
  uint8_t lut[4096];
};
inline void rans_read_freqs(Cursor& c, RansTable* t) {
  memset(t->F, 0, sizeof t->F);
  int sym = c.u8(), last = sym, rle = 0;
  for (;;) {
    uint32_t f = c.u8();
    if (f >= 128) f = ((f & 127) << 8) | c.u8();
    t->F[sym] = (uint16_t)f;
    if (rle) {
      --rle;
      ++sym;
      if (sym > 255) throw std::runtime_error("CRAM: rANS symbol run past 255");
    } else {
      sym = c.u8();
      if (sym == last + 1) rle = c.u8();
    }
    last = sym;
    if (sym == 0) break;
  }
  uint32_t acc = 0;
  for (int i = 0; i < 256; ++i) {
    t->C[i] = (uint16_t)acc;
    if (acc + t->F[i] > 4096) throw std::runtime_error("CRAM: rANS frequencies exceed 4096");
    memset(t->lut + acc, i, t->F[i]);
    acc += t->F[i];
  }
  t->C[256] = (uint16_t)acc;
  memset(t->lut + acc, 0, 4096 - acc);
}
inline void rans_step(uint32_t& R, const RansTable& t, uint8_t* out, Cursor& c) {
  const uint32_t f = R & 0xFFF;
  const uint8_t s = t.lut[f];
  *out = s;
  R = (uint32_t)t.F[s] * (R >> 12) + f - t.C[s];
  while (R < (1u << 23)) R = (R << 8) | c.u8();
}
// An rANS encoder starts every state at the lower bound of the renormalisation interval and the decoder retraces it backwards, so
// a stream decoded to its end leaves each state AT that bound.  Checked (round 3): raw and rANS blocks carry no checksum of the
// DECODED bytes, and this is what pins the rANS Nx16 decoder below, for which no htslib-written stream is at hand -- every rANS
// 4x8 stream of the reference's four htslib-written fixtures passes it.
inline void rans_4x8_done(const uint32_t* R) {
  for (int j = 0; j < 4; ++j)
    if (R[j] != (1u << 23)) throw std::runtime_error("CRAM: rANS 4x8 stream does not end in its initial state (corrupt block)");
}
inline std::vector<uint8_t> rans_4x8(const uint8_t* data, size_t size) {
  Cursor c(data, size);
  const int order = c.u8();
  (void)c.i32le();
  const uint32_t n = (uint32_t)c.i32le();
  if (n > (1u << 28)) throw std::runtime_error("CRAM: rANS block too large");
  std::vector<uint8_t> out(n);
  if (order == 0) {
    std::unique_ptr<RansTable> t(new RansTable);
    rans_read_freqs(c, t.get());
    uint32_t R[4];
    for (int j = 0; j < 4; ++j) R[j] = (uint32_t)c.i32le();
    for (uint32_t i = 0; i < n; ++i) rans_step(R[i & 3], *t, &out[i], c);
    rans_4x8_done(R);
    return out;
  }
  if (order != 1) throw std::runtime_error("CRAM: rANS order " + std::to_string(order));
  std::vector<std::unique_ptr<RansTable>> tabs(256);
  int ctx = c.u8(), last = ctx, rle = 0;
  for (;;) {
    tabs[(size_t)ctx].reset(new RansTable);
    rans_read_freqs(c, tabs[(size_t)ctx].get());
    if (rle) {
      --rle;
      ++ctx;
      if (ctx > 255) throw std::runtime_error("CRAM: rANS context run past 255");
    } else {
      ctx = c.u8();
      if (ctx == last + 1) rle = c.u8();
    }
    last = ctx;
    if (ctx == 0) break;
  }
  uint32_t R[4];
  for (int j = 0; j < 4; ++j) R[j] = (uint32_t)c.i32le();
  const uint32_t q = n >> 2;
  const uint32_t idx[4] = {0, q, 2 * q, 3 * q};
  uint8_t prev[4] = {0, 0, 0, 0};
  auto tab = [&](uint8_t ctx_) -> const RansTable& {
    if (!tabs[ctx_]) throw std::runtime_error("CRAM: rANS context without a table");
    return *tabs[ctx_];
  };
  for (uint32_t k = 0; k < q; ++k)
    for (int j = 0; j < 4; ++j) {
      rans_step(R[j], tab(prev[j]), &out[idx[j] + k], c);
      prev[j] = out[idx[j] + k];
    }
  for (uint32_t i = 4 * q; i < n; ++i) {  // the remainder belongs to the last state
    rans_step(R[3], tab(prev[3]), &out[i], c);
    prev[3] = out[i];
  }
  rans_4x8_done(R);
  return out;
}

// ---- rANS Nx16 (CRAM 3.1, block method 5) ---------------------------------------------------------------------------------
// The entropy coder htslib >= 1.22 writes by default ("CRAM codecs" specification section 3; noodles-cram, which the reference
// reads CRAM through, decodes it): N = 4 or 32 interleaved states, 16-bit renormalisation above a lower bound of 2^15,
// frequencies summing to 2^12 (order 0) or 2^shift (order 1, shift from the stream), and, in front of the entropy coder, up to
// three byte transforms the flags byte announces: bit-packing of <= 16 distinct symbols, run-length coding with the run lengths in
// a side stream, and N-way striping into separately coded sub-streams.  No htslib-written 3.1 file exists in this image or in the
// reference's fixtures, so every stream is also CHECKED rather than trusted: an encoder starts each state at the lower bound,
// so a decoder that has undone the encoding exactly ends with every state equal to it -- a stream decoded under a wrong reading
// of the format fails that test (and the size tests) instead of yielding wrong columns.  The same test on the rANS 4x8
// streams of the reference's own fixtures (written by htslib) holds, which pins the premise on the encoder family.
enum : int { RANS16_ORDER = 0x01, RANS16_X32 = 0x04, RANS16_STRIPE = 0x08, RANS16_NOSZ = 0x10, RANS16_CAT = 0x20, RANS16_RLE = 0x40, RANS16_PACK = 0x80 };
constexpr uint32_t RANS16_LOW = 1u << 15;
constexpr uint32_t RANS16_MAX_OUT = 1u << 28;
inline uint32_t uint7(Cursor& c) {  // big-endian base-128, high bit = "more"
  uint32_t v = 0;
  for (int i = 0; i < 5; ++i) {
    const uint8_t b = c.u8();
    if (v >> 25) throw std::runtime_error("CRAM: rANS Nx16 length does not fit 32 bits");
    v = (v << 7) | (b & 0x7Fu);
    if (!(b & 0x80)) return v;
  }
  throw std::runtime_error("CRAM: rANS Nx16 length longer than 5 bytes");
}
inline void rans16_alphabet(Cursor& c, bool* A) {  // the run-length coded symbol list rANS 4x8 uses too
  std::fill(A, A + 256, false);
  int sym = c.u8(), last = sym, rle = 0;
  do {
    A[sym] = true;
    if (rle) {
      --rle;
      if (++sym > 255) throw std::runtime_error("CRAM: rANS symbol run past 255");
    } else {
      sym = c.u8();
      if (sym == last + 1) rle = c.u8();
    }
    last = sym;
  } while (sym != 0);
}
struct Rans16Table {
  uint16_t F[256], C[256];
  uint8_t lut[4096];
  bool live = false;  // false: every frequency is zero (an order-1 context the data never enters)
  // frequencies as read -> scaled up by a power of two to 2^bits, cumulative sums, slot -> symbol table
  void finish(int bits) {
    uint32_t tot = 0;
    for (int i = 0; i < 256; ++i) tot += F[i];
    live = tot != 0;
    if (!live) return;
    const uint32_t full = 1u << bits;
    int up = 0;
    while ((tot << up) < full) ++up;
    if ((tot << up) != full) throw std::runtime_error("CRAM: rANS Nx16 frequencies do not sum to a power of two <= 2^" + std::to_string(bits));
    uint32_t acc = 0;
    for (int i = 0; i < 256; ++i) {
      const uint32_t f = (uint32_t)F[i] << up;
      F[i] = (uint16_t)f;
      C[i] = (uint16_t)acc;
      memset(lut + acc, i, f);
      acc += f;
    }
  }
};
struct Rans16States {
  uint32_t R[32];
  const uint8_t *p, *end;
  int N;
  Rans16States(Cursor& c, int n_states) : N(n_states) {
    for (int j = 0; j < N; ++j) R[j] = (uint32_t)c.i32le();
    p = c.p + c.o;
    end = c.p + c.n;
  }
  inline uint8_t step(int j, const Rans16Table& t, int bits) {
    uint32_t r = R[j];
    const uint32_t f = r & ((1u << bits) - 1);
    const uint8_t s = t.lut[f];
    r = (uint32_t)t.F[s] * (r >> bits) + f - t.C[s];
    if (r < RANS16_LOW) {
      if (end - p < 2) throw std::runtime_error("CRAM: truncated data");
      r = (r << 16) | (uint32_t)p[0] | ((uint32_t)p[1] << 8);
      p += 2;
    }
    R[j] = r;
    return s;
  }
  void done(Cursor& c) {  // see the note above: every state is back at the encoder's initial value
    for (int j = 0; j < N; ++j)
      if (R[j] != RANS16_LOW) throw std::runtime_error("CRAM: rANS Nx16 stream does not end in its initial state (corrupt, or not this codec)");
    c.o = (size_t)(p - c.p);
  }
};
inline void rans16_order0(Cursor& c, uint8_t* out, size_t n, int N) {
  if (n == 0) return;
  bool A[256];
  rans16_alphabet(c, A);
  std::unique_ptr<Rans16Table> t(new Rans16Table);
  for (int i = 0; i < 256; ++i) {
    const uint32_t f = A[i] ? uint7(c) : 0;
    if (f > 4096) throw std::runtime_error("CRAM: rANS Nx16 frequency above 4096");
    t->F[i] = (uint16_t)f;
  }
  t->finish(12);
  if (!t->live) throw std::runtime_error("CRAM: rANS Nx16 table without a symbol");
  Rans16States st(c, N);
  for (size_t i = 0; i < n; ++i) out[i] = st.step((int)(i & (size_t)(N - 1)), *t, 12);
  st.done(c);
}
inline void rans16_order1(Cursor& c, uint8_t* out, size_t n, int N) {
  if (n == 0) return;
  const int comp = c.u8(), bits = comp >> 4;
  if (bits < 1 || bits > 12) throw std::runtime_error("CRAM: rANS Nx16 order-1 frequency width " + std::to_string(bits));
  std::vector<uint8_t> plain;
  Cursor own(nullptr, 0);
  Cursor* tc = &c;
  if (comp & 1) {  // the table itself went through the order-0 coder (always four states)
    const uint32_t usz = uint7(c), csz = uint7(c);
    if (usz > (1u << 20)) throw std::runtime_error("CRAM: rANS Nx16 order-1 table too large");
    c.need(csz);
    plain.resize(usz);
    Cursor sub(c.p + c.o, csz);
    rans16_order0(sub, plain.data(), usz, 4);
    c.o += csz;
    own = Cursor(plain.data(), plain.size());
    tc = &own;
  }
  bool A[256];
  rans16_alphabet(*tc, A);
  std::vector<std::unique_ptr<Rans16Table>> tabs(256);
  for (int i = 0; i < 256; ++i) {
    if (!A[i]) continue;
    tabs[(size_t)i].reset(new Rans16Table);
    Rans16Table& t = *tabs[(size_t)i];
    int run = 0;
    for (int j = 0; j < 256; ++j) {
      t.F[j] = 0;
      if (!A[j]) continue;
      if (run) {
        --run;
        continue;
      }
      const uint32_t f = uint7(*tc);
      if (f > (1u << bits)) throw std::runtime_error("CRAM: rANS Nx16 frequency above its total");
      t.F[j] = (uint16_t)f;
      if (f == 0) run = tc->u8();
    }
    t.finish(bits);
  }
  Rans16States st(c, N);
  auto tab = [&](uint8_t ctx) -> const Rans16Table& {
    if (!tabs[ctx] || !tabs[ctx]->live) throw std::runtime_error("CRAM: rANS context without a table");
    return *tabs[ctx];
  };
  const size_t seg = n / (size_t)N;  // state j codes out[j * seg ...), the last one also the remainder
  uint8_t last[32] = {0};
  for (size_t k = 0; k < seg; ++k)
    for (int j = 0; j < N; ++j) last[j] = out[(size_t)j * seg + k] = st.step(j, tab(last[j]), bits);
  for (size_t i = seg * (size_t)N; i < n; ++i) last[N - 1] = out[i] = st.step(N - 1, tab(last[N - 1]), bits);
  st.done(c);
}
// `expect`: the decoded size the caller knows (the block's raw size; a stripe's share); read from the stream unless NOSZ is set
inline std::vector<uint8_t> rans_nx16(const uint8_t* data, size_t size, uint32_t expect, int depth = 0) {
  Cursor c(data, size);
  const int flags = c.u8();
  uint32_t n = (flags & RANS16_NOSZ) ? expect : uint7(c);
  // the stream's own size must be the one the block header (or the stripe's share) announced: checked BEFORE anything is
  // allocated for it (run lengths and packing expand without bound, so no ratio to the compressed size can be asked for)
  if (n != expect) throw std::runtime_error("CRAM: rANS Nx16 stream of " + std::to_string(n) + " bytes in a block of " + std::to_string(expect));
  if (n > RANS16_MAX_OUT) throw std::runtime_error("CRAM: rANS block too large");
  const int N = (flags & RANS16_X32) ? 32 : 4;
  if (flags & RANS16_STRIPE) {  // byte i of the data went to sub-stream i mod X; each sub-stream is a stream of its own
    if (depth) throw std::runtime_error("CRAM: rANS Nx16 stripes inside stripes");
    const uint32_t X = c.u8();
    if (X == 0) throw std::runtime_error("CRAM: rANS Nx16 with zero stripes");
    std::vector<uint32_t> clen(X);
    for (uint32_t j = 0; j < X; ++j) clen[j] = uint7(c);
    std::vector<uint8_t> out(n);
    for (uint32_t j = 0; j < X; ++j) {
      const uint32_t share = n / X + ((n % X) > j ? 1u : 0u);
      c.need(clen[j]);
      const std::vector<uint8_t> sub = rans_nx16(c.p + c.o, clen[j], share, depth + 1);
      if (sub.size() != share) throw std::runtime_error("CRAM: rANS Nx16 stripe of the wrong length");
      c.o += clen[j];
      for (uint32_t i = 0; i < share; ++i) out[(size_t)i * X + j] = sub[i];
    }
    return out;
  }
  uint8_t pack_map[16] = {0};
  uint32_t pack_nsym = 0, pack_out = 0;
  if (flags & RANS16_PACK) {
    pack_nsym = c.u8();
    if (pack_nsym > 16) throw std::runtime_error("CRAM: rANS Nx16 packs more than 16 symbols");
    for (uint32_t i = 0; i < pack_nsym; ++i) pack_map[i] = c.u8();
    pack_out = n;
    n = uint7(c);
    const uint32_t per = pack_nsym <= 1 ? 0 : pack_nsym <= 2 ? 8 : pack_nsym <= 4 ? 4 : 2;  // symbols per packed byte
    if (pack_out && (pack_nsym == 0 || (per && (uint64_t)n * per < pack_out))) throw std::runtime_error("CRAM: rANS Nx16 packed data too short");
    if (n > RANS16_MAX_OUT) throw std::runtime_error("CRAM: rANS block too large");
  }
  std::vector<uint8_t> rle_meta;
  uint32_t rle_out = 0;
  if (flags & RANS16_RLE) {
    const uint32_t m2 = uint7(c);
    rle_out = n;
    n = uint7(c);
    if (n > RANS16_MAX_OUT || m2 / 2 > RANS16_MAX_OUT) throw std::runtime_error("CRAM: rANS block too large");
    if (m2 & 1) {  // run lengths stored as they are
      c.need(m2 / 2);
      rle_meta.assign(c.p + c.o, c.p + c.o + m2 / 2);
      c.o += m2 / 2;
    } else {
      const uint32_t csz = uint7(c);
      c.need(csz);
      rle_meta.resize(m2 / 2);
      Cursor sub(c.p + c.o, csz);
      rans16_order0(sub, rle_meta.data(), rle_meta.size(), N);
      c.o += csz;
    }
  }
  std::vector<uint8_t> out(n);
  if (flags & RANS16_CAT) {
    c.need(n);
    if (n) memcpy(out.data(), c.p + c.o, n);
    c.o += n;
  } else if (flags & RANS16_ORDER) {
    rans16_order1(c, out.data(), n, N);
  } else {
    rans16_order0(c, out.data(), n, N);
  }
  if (flags & RANS16_RLE) {  // literals -> runs: a symbol on the list is followed (in the side stream) by how often it repeats
    Cursor m(rle_meta.data(), rle_meta.size());
    bool runs[256] = {false};
    uint32_t nsym = rle_out ? m.u8() : 0;
    if (rle_out && nsym == 0) nsym = 256;
    for (uint32_t i = 0; i < nsym; ++i) runs[m.u8()] = true;
    std::vector<uint8_t> wide(rle_out);
    size_t w = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint8_t b = out[i];
      const size_t reps = runs[b] ? (size_t)uint7(m) + 1 : 1;
      if (reps > wide.size() - w) throw std::runtime_error("CRAM: rANS Nx16 runs exceed the block");
      memset(wide.data() + w, b, reps);
      w += reps;
    }
    if (w != wide.size()) throw std::runtime_error("CRAM: rANS Nx16 runs fall short of the block");
    out.swap(wide);
  }
  if (flags & RANS16_PACK) {
    std::vector<uint8_t> wide(pack_out);
    if (pack_nsym <= 1) {
      std::fill(wide.begin(), wide.end(), pack_map[0]);
    } else {
      const int width = pack_nsym <= 2 ? 1 : pack_nsym <= 4 ? 2 : 4, per = 8 / width;
      const uint32_t mask = (1u << width) - 1;
      for (size_t i = 0; i < wide.size(); ++i) {  // low bits first
        const uint32_t v = (out[i / (size_t)per] >> ((i % (size_t)per) * (size_t)width)) & mask;
        if (v >= pack_nsym) throw std::runtime_error("CRAM: rANS Nx16 packed value without a symbol");
        wide[i] = pack_map[v];
      }
    }
    out.swap(wide);
  }
  return out;
}

// bzip2 / xz block payloads: one-shot decoders of the system libraries, bound by name (their C ABIs: bzlib.h 1.0, lzma.h 5.x)
using bz2_decompress_fn = int (*)(char* dest, unsigned* dest_len, char* source, unsigned source_len, int small, int verbosity);
using lzma_buffer_decode_fn = int (*)(uint64_t* memlimit, uint32_t flags, const void* allocator, const uint8_t* in, size_t* in_pos,
                                      size_t in_size, uint8_t* out, size_t* out_pos, size_t out_size);
inline bz2_decompress_fn bz2_decompress() {
  static const bz2_decompress_fn fn = [] {
    void* h = dlopen("libbz2.so.1.0", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libbz2.so.1", RTLD_NOW | RTLD_LOCAL);
    return h ? reinterpret_cast<bz2_decompress_fn>(dlsym(h, "BZ2_bzBuffToBuffDecompress")) : nullptr;
  }();
  return fn;
}
inline lzma_buffer_decode_fn lzma_buffer_decode() {
  static const lzma_buffer_decode_fn fn = [] {
    void* h = dlopen("liblzma.so.5", RTLD_NOW | RTLD_LOCAL);
    return h ? reinterpret_cast<lzma_buffer_decode_fn>(dlsym(h, "lzma_stream_buffer_decode")) : nullptr;
  }();
  return fn;
}

// What a decode thread keeps from one slice to the next: the byte vectors expanded blocks live in and the inflate state.  Without it
// every slice allocates and frees a few hundred KiB in 5-50 KiB pieces (and zlib 40 KiB per gzip block); with dozens of threads doing
// that, glibc grows and trims their heaps continuously, and those calls and the page faults behind them queue on the process-wide
// memory-map lock (the per-container decode time doubled from 8 to 64 threads).
struct ByteCache {
  std::vector<std::vector<uint8_t>> spare;
  z_stream z;
  bool z_ready = false;
  ByteCache() { memset(&z, 0, sizeof z); }
  ByteCache(const ByteCache&) = delete;
  ByteCache& operator=(const ByteCache&) = delete;
  ~ByteCache() {
    if (z_ready) inflateEnd(&z);
  }
  std::vector<uint8_t> take() {
    if (spare.empty()) return {};
    std::vector<uint8_t> v = std::move(spare.back());
    spare.pop_back();
    v.clear();
    return v;
  }
  void give(std::vector<uint8_t>&& v) {
    if (v.capacity() && spare.size() < 256) spare.push_back(std::move(v));
  }
};

struct Block {
  int type = 0;
  uint32_t id = 0;
  std::vector<uint8_t> data;
  // a block read lazily (read_block(c, true)) keeps its compressed payload -- which lives in the container's buffer -- until
  // expand() is called: the external blocks of data series this path never looks at (quality scores, bases, names, tag
  // values: most of a file) are then never decompressed (what htslib's `required_fields` does; the reference decodes all)
  int method = 0;
  uint32_t csz = 0, rsz = 0;
  const uint8_t* src = nullptr;
  bool ready = true;
  ByteCache* cache = nullptr;  // where `data` comes from and goes back to (may be null)
  void expand();
};
inline void Block::expand() {
  if (ready) return;
  Block& b = *this;
  if (cache) b.data = cache->take();
  if (method == 0) {
    b.data.assign(src, src + csz);
  } else if (method == 1) {
    b.data.resize(rsz);
    z_stream own;
    z_stream* z = &own;
    if (cache) {  // one inflate state per decode thread, reset per block
      z = &cache->z;
      if (cache->z_ready ? inflateReset2(z, 15 + 32) != Z_OK : inflateInit2(z, 15 + 32) != Z_OK) throw std::runtime_error("inflateInit2 failed");
      cache->z_ready = true;
    } else {
      memset(&own, 0, sizeof own);
      if (inflateInit2(z, 15 + 32) != Z_OK) throw std::runtime_error("inflateInit2 failed");
    }
    z->next_in = const_cast<uint8_t*>(src);
    z->avail_in = csz;
    z->next_out = b.data.data();
    z->avail_out = rsz;
    const int rc = rsz ? inflate(z, Z_FINISH) : Z_STREAM_END;
    const bool whole = z->avail_out == 0;
    if (!cache) inflateEnd(z);
    if (rc != Z_STREAM_END || !whole) throw std::runtime_error("CRAM: corrupt gzip block");
  } else if (method == 2) {  // bzip2 (CRAM 3.0 section 8.1)
    const bz2_decompress_fn f = bz2_decompress();
    if (!f) throw std::runtime_error("CRAM: bzip2 block, but libbz2.so.1.0 is not on this machine");
    b.data.resize(rsz ? rsz : 1);
    unsigned got = (unsigned)b.data.size();
    const int rc = f(reinterpret_cast<char*>(b.data.data()), &got, reinterpret_cast<char*>(const_cast<uint8_t*>(src)), csz, 0, 0);
    if (rc != 0 /* BZ_OK */ || got != rsz) throw std::runtime_error("CRAM: corrupt bzip2 block");
    b.data.resize(rsz);
  } else if (method == 3) {  // lzma: an .xz stream
    const lzma_buffer_decode_fn f = lzma_buffer_decode();
    if (!f) throw std::runtime_error("CRAM: lzma block, but liblzma.so.5 is not on this machine");
    b.data.resize(rsz);
    uint64_t memlimit = 1ull << 30;
    size_t in_pos = 0, out_pos = 0;
    const int rc = f(&memlimit, 0, nullptr, src, &in_pos, csz, b.data.data(), &out_pos, rsz);
    if (rc != 0 /* LZMA_OK */ || out_pos != rsz) throw std::runtime_error("CRAM: corrupt lzma block");
  } else if (method == 4) {
    b.data = rans_4x8(src, csz);
  } else if (method == 5) {
    b.data = rans_nx16(src, csz, rsz);
  } else {
    // 6 adaptive arithmetic coder, 7 fqzcomp (quality scores), 8 name tokeniser: reached only when a data series this path
    // READS lives in such a block -- the blocks of discarded series (names, quality scores: where htslib's 3.1 profiles put
    // 7 and 8) are never expanded
    static const char* const names[] = {"adaptive arithmetic coder", "fqzcomp", "name tokeniser"};
    throw std::runtime_error("CRAM: block compression method " + std::to_string(method) +
                             (method >= 6 && method <= 8 ? std::string(" (") + names[method - 6] + ")" : std::string()) +
                             " is not supported (raw, gzip, bzip2, lzma, rANS 4x8 and rANS Nx16 are)");
  }
  if (b.data.size() != rsz) throw std::runtime_error("CRAM: block size mismatch");
  ready = true;
}
inline Block read_block(Cursor& c, bool lazy = false, ByteCache* cache = nullptr) {
  Block b;
  b.cache = cache;
  const size_t block_start = c.o;
  b.method = c.u8();
  b.type = c.u8();
  b.id = c.itf8();
  const uint32_t csz = c.itf8(), rsz = c.itf8();
  c.need((size_t)csz + 4);
  b.csz = csz;
  b.rsz = rsz;
  b.src = c.p + c.o;
  b.ready = false;
  // a corrupt size must not turn into a huge allocation: DEFLATE expands at most ~1032x, rANS blocks are capped outright
  if (rsz > (1u << 28) || (b.method == 1 && (uint64_t)rsz > (uint64_t)csz * 1032u + 1024u)) throw std::runtime_error("CRAM: block too large");
  if (b.method < 0 || b.method > 8) throw std::runtime_error("CRAM: block compression method " + std::to_string(b.method) + " does not exist");
  // CRC-32 over the block's header and payload (CRAM 3.0 section 8): a raw or rANS block has no other integrity check, and
  // a flipped byte in an external block would otherwise become silently wrong flag / position columns (noodles-cram
  // reports a checksum mismatch).  Checked for every block, expanded or not.
  c.o += (size_t)csz;
  const uint32_t want = (uint32_t)c.i32le();
  const uint32_t got = (uint32_t)crc32(crc32(0L, Z_NULL, 0), c.p + block_start, (uInt)(c.o - 4 - block_start));
#ifndef EXON_CRAM_FUZZ_SKIP_CRC  // defined by the sanitizer harness only: lets corrupted payloads reach the decoders behind the check
  if (got != want) throw std::runtime_error("CRAM: block CRC-32 mismatch");
#else
  (void)got, (void)want;
#endif
  if (!lazy) b.expand();
  return b;
}

struct Encoding {
  enum Kind { NONE, EXTERNAL, HUFFMAN, BYTE_ARRAY_LEN, BYTE_ARRAY_STOP, BETA, UNSUPPORTED } kind = NONE;
  uint32_t codec = 0;               // UNSUPPORTED: the codec id, reported when (and only when) the series is read
  uint32_t id = 0;                  // EXTERNAL / BYTE_ARRAY_STOP: block content id
  uint8_t stop = 0;                 // BYTE_ARRAY_STOP
  int32_t offset = 0, nbits = 0;    // BETA
  std::vector<int32_t> syms;        // HUFFMAN
  std::vector<uint32_t> lens, codes;
  std::shared_ptr<Encoding> len_enc, val_enc;  // BYTE_ARRAY_LEN
  int slot = -1;  // EXTERNAL / BYTE_ARRAY_STOP: index of the block with content id `id` in the current slice (SliceData::bind)
};
// depth: BYTE_ARRAY_LEN (codec 4) nests two encodings.  The specification only ever puts scalar encodings there (the length
// is an integer series, the values a byte series), so a BYTE_ARRAY_LEN inside a BYTE_ARRAY_LEN is rejected -- a crafted header
// nesting them ~100 k deep would otherwise overflow the decoding thread's stack (read_encoding and SliceData::bind recurse).
inline Encoding read_encoding(Cursor& c, int depth = 0) {
  Encoding e;
  const uint32_t codec = c.itf8(), ln = c.itf8();
  c.need(ln);
  Cursor p(c.p + c.o, ln);
  switch (codec) {
    case 0: break;
    case 1:
      e.kind = Encoding::EXTERNAL;
      e.id = p.itf8();
      break;
    case 3: {
      e.kind = Encoding::HUFFMAN;
      const uint32_t n = p.itf8();
      for (uint32_t i = 0; i < n; ++i) e.syms.push_back(p.itf8s());
      const uint32_t n2 = p.itf8();
      for (uint32_t i = 0; i < n2; ++i) e.lens.push_back(p.itf8());
      if (n != n2 || n == 0) throw std::runtime_error("CRAM: malformed Huffman encoding");
      // canonical codes: by (length, symbol)
      std::vector<size_t> order(n);
      for (size_t i = 0; i < n; ++i) order[i] = i;
      std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return e.lens[a] != e.lens[b] ? e.lens[a] < e.lens[b] : e.syms[a] < e.syms[b]; });
      e.codes.assign(n, 0);
      uint32_t code = 0, prev = 0;
      for (size_t k = 0; k < n; ++k) {
        const size_t i = order[k];
        if (e.lens[i] > 31) throw std::runtime_error("CRAM: Huffman code too long");
        code <<= (e.lens[i] - prev);
        e.codes[i] = code++;
        prev = e.lens[i];
      }
      break;
    }
    case 4:
      if (depth >= 1) throw std::runtime_error("CRAM: BYTE_ARRAY_LEN nested inside BYTE_ARRAY_LEN");
      e.kind = Encoding::BYTE_ARRAY_LEN;
      e.len_enc = std::make_shared<Encoding>(read_encoding(p, depth + 1));
      e.val_enc = std::make_shared<Encoding>(read_encoding(p, depth + 1));
      break;
    case 5:
      e.kind = Encoding::BYTE_ARRAY_STOP;
      e.stop = p.u8();
      e.id = p.itf8();
      break;
    case 6:
      e.kind = Encoding::BETA;
      e.offset = p.itf8s();
      e.nbits = (int32_t)p.itf8();
      if (e.nbits > 32) throw std::runtime_error("CRAM: BETA width");
      break;
    default:
      // GOLOMB / SUBEXP / GAMMA ...: recorded, and an error only if a value of this series is ever decoded -- a file that
      // uses one on a series this reader never touches (TC, TN) still decodes
      e.kind = Encoding::UNSUPPORTED;
      e.codec = codec;
      break;
  }
  c.o += ln;
  return e;
}

// the blocks of one slice + read positions.  External blocks are flat streams addressed by slot; an encoding is bound to its
// slot once per slice (a map lookup per VALUE made the decoder 10x slower).
struct SliceData {
  ByteCache* cache = nullptr;
  SliceData() = default;
  SliceData(const SliceData&) = delete;
  SliceData& operator=(const SliceData&) = delete;
  ~SliceData() {
    if (!cache) return;
    cache->give(std::move(core));
    for (Block& b : blocks) cache->give(std::move(b.data));
  }
  std::vector<uint8_t> core;
  size_t core_bit = 0;
  std::vector<Block> blocks;            // external blocks in file order
  std::vector<const uint8_t*> ptr;
  std::vector<size_t> len, pos;

  void add(Block&& b) {
    blocks.push_back(std::move(b));
  }
  // needed[k]: some data series whose VALUES the columns depend on lives in external block k.  A block that only holds series
  // this path discards (quality scores, bases, names, tag values, mate fields ...) is never expanded and the skip_* calls on
  // it are no-ops: every external block is its own stream, so nothing else falls out of step.  (A block that mixes both kinds
  // is `needed` and consumed value by value as before.)
  std::vector<char> needed;
  void finish_blocks() {
    ptr.assign(blocks.size(), nullptr);
    len.assign(blocks.size(), 0);
    pos.assign(blocks.size(), 0);
    needed.assign(blocks.size(), 0);
    for (size_t i = 0; i < blocks.size(); ++i)
      if (blocks[i].ready) {
        ptr[i] = blocks[i].data.data();
        len[i] = blocks[i].data.size();
      }
  }
  void ensure(int k) {  // expand block k on first use
    if (blocks[(size_t)k].ready) return;
    blocks[(size_t)k].expand();
    ptr[(size_t)k] = blocks[(size_t)k].data.data();
    len[(size_t)k] = blocks[(size_t)k].data.size();
  }
  void need_values(const Encoding& e) {  // call after bind()
    if ((e.kind == Encoding::EXTERNAL || e.kind == Encoding::BYTE_ARRAY_STOP) && e.slot >= 0) needed[(size_t)e.slot] = 1;
    else if (e.kind == Encoding::BYTE_ARRAY_LEN) {
      need_values(*e.len_enc);
      need_values(*e.val_enc);
    }
  }
  bool discardable(const Encoding& e) const {  // an external series alone (with other discarded ones) in its block
    return (e.kind == Encoding::EXTERNAL || e.kind == Encoding::BYTE_ARRAY_STOP) && e.slot >= 0 && !needed[(size_t)e.slot];
  }
  void bind(Encoding& e) const {
    e.slot = -1;
    if (e.kind == Encoding::EXTERNAL || e.kind == Encoding::BYTE_ARRAY_STOP) {
      for (size_t i = 0; i < blocks.size(); ++i)
        if (blocks[i].id == e.id) e.slot = (int)i;
    } else if (e.kind == Encoding::BYTE_ARRAY_LEN) {
      bind(*e.len_enc);
      bind(*e.val_enc);
    }
  }
  int slot_of(const Encoding& e) const {
    if (e.slot < 0) throw std::runtime_error("CRAM: external block " + std::to_string(e.id) + " is missing");
    return e.slot;
  }
  uint32_t bits(int n) {
    uint32_t v = 0;
    for (int i = 0; i < n; ++i) {
      if ((core_bit >> 3) >= core.size()) throw std::runtime_error("CRAM: core block exhausted");
      v = (v << 1) | ((core[core_bit >> 3] >> (7 - (core_bit & 7))) & 1u);
      ++core_bit;
    }
    return v;
  }
  int32_t get_int(const Encoding& e) {
    switch (e.kind) {
      case Encoding::EXTERNAL: {
        const int k = slot_of(e);
        ensure(k);
        Cursor c(ptr[k], len[k]);
        c.o = pos[k];
        const int32_t v = c.itf8s();
        pos[k] = c.o;
        return v;
      }
      case Encoding::HUFFMAN: {
        if (e.syms.size() == 1 && e.lens[0] == 0) return e.syms[0];
        uint32_t code = 0, l = 0;
        for (;;) {
          code = (code << 1) | bits(1);
          ++l;
          for (size_t i = 0; i < e.syms.size(); ++i)
            if (e.lens[i] == l && e.codes[i] == code) return e.syms[i];
          if (l > 31) throw std::runtime_error("CRAM: bad Huffman code");
        }
      }
      case Encoding::BETA:
        return (int32_t)bits(e.nbits) - e.offset;
      case Encoding::UNSUPPORTED:
        throw std::runtime_error("CRAM: encoding " + std::to_string(e.codec) + " is not supported");
      default:
        throw std::runtime_error("CRAM: integer data series with a byte-array encoding");
    }
  }
  // a value this path discards: nothing to do when its block holds nothing else of interest
  void skip_int(const Encoding& e) {
    if (!discardable(e)) (void)get_int(e);
  }
  void skip_byte(const Encoding& e) {
    if (!discardable(e)) (void)get_byte(e);
  }
  uint8_t get_byte(const Encoding& e) {
    if (e.kind == Encoding::EXTERNAL) {
      const int k = slot_of(e);
      ensure(k);
      if (pos[k] >= len[k]) throw std::runtime_error("CRAM: truncated data");
      return ptr[k][pos[k]++];
    }
    return (uint8_t)get_int(e);
  }
  void skip_n(const Encoding& e, size_t n) {  // n single-byte values of one series
    if (e.kind == Encoding::EXTERNAL) {
      const int k = slot_of(e);
      if (!needed[(size_t)k]) return;
      ensure(k);
      if (n > len[k] - pos[k]) throw std::runtime_error("CRAM: truncated data");
      pos[k] += n;
      return;
    }
    for (size_t i = 0; i < n; ++i) (void)get_int(e);
  }
  // length of the byte array; the bytes themselves are skipped (only lengths matter to the columns of this path)
  // `want_len` false: the caller uses neither the bytes nor their count
  size_t skip_bytes(const Encoding& e, std::string* keep = nullptr, bool want_len = true) {
    if (e.kind == Encoding::BYTE_ARRAY_STOP) {
      const int k = slot_of(e);
      if (!want_len && !keep && !needed[(size_t)k]) return 0;
      ensure(k);
      const uint8_t* b = ptr[k] + pos[k];
      const void* hit = memchr(b, e.stop, len[k] - pos[k]);
      if (!hit) throw std::runtime_error("CRAM: truncated data");
      const size_t n = (size_t)(static_cast<const uint8_t*>(hit) - b);
      if (keep) keep->assign(reinterpret_cast<const char*>(b), n);
      pos[k] += n + 1;
      return n;
    }
    if (e.kind == Encoding::BYTE_ARRAY_LEN) {
      if (!want_len && !keep && discardable(*e.len_enc) && discardable(*e.val_enc)) return 0;
      const int32_t n = get_int(*e.len_enc);
      if (n < 0) throw std::runtime_error("CRAM: negative byte-array length");
      if (e.val_enc->kind == Encoding::EXTERNAL) {
        const int k = slot_of(*e.val_enc);
        if (!keep && !needed[(size_t)k]) return (size_t)n;  // the bytes live alone in a block nobody reads
        ensure(k);
        if ((size_t)n > len[k] - pos[k]) throw std::runtime_error("CRAM: truncated data");
        if (keep) keep->assign(reinterpret_cast<const char*>(ptr[k] + pos[k]), (size_t)n);
        pos[k] += (size_t)n;
      } else {
        if (keep) keep->clear();
        for (int32_t i = 0; i < n; ++i) {
          const uint8_t v = get_byte(*e.val_enc);
          if (keep) keep->push_back((char)v);
        }
      }
      return (size_t)n;
    }
    throw std::runtime_error("CRAM: byte-array data series with an integer encoding");
  }
};

}  // namespace cram

// Blocks that hold the buffers of one batch.  Batches are built on the decoder threads and released on the consumer's; with
// malloc / free that pattern makes glibc grow and trim the decoder threads' heaps for every batch (32-64 KiB buffers: page
// faults under the process-wide mmap lock -- 8 threads decoded 3.8 M records/s instead of 19), so the blocks cycle through a
// small pool instead: no system call in the steady state.  At most 128 MiB are kept; the rest is freed.
class BlockPool {
 public:
  void* get(size_t bytes) {
    {
      std::lock_guard<std::mutex> g(mu_);
      auto it = free_.find(bytes);
      if (it != free_.end() && !it->second.empty()) {
        void* p = it->second.back();
        it->second.pop_back();
        held_ -= bytes;
        return p;
      }
    }
    void* p = malloc(bytes);
    if (!p) throw std::bad_alloc();
    return p;
  }
  static void put(void* p, size_t bytes) { instance().put_(p, bytes); }
  static BlockPool& instance() {
    static BlockPool pool;
    return pool;
  }
  ~BlockPool() {
    for (auto& kv : free_)
      for (void* p : kv.second) free(p);
  }

 private:
  void put_(void* p, size_t bytes) {
    {
      std::lock_guard<std::mutex> g(mu_);
      if (held_ + bytes <= (size_t(128) << 20)) {
        free_[bytes].push_back(p);
        held_ += bytes;
        return;
      }
    }
    free(p);
  }
  std::mutex mu_;
  std::map<size_t, std::vector<void*>> free_;
  size_t held_ = 0;
};

class CRAMBatchReader : public BatchReader {
 public:
  CRAMBatchReader(const std::string& path, BAMConfig cfg) : cfg_(std::move(cfg)) {
    fd_ = fdh_.v = ::open(path.c_str(), O_RDONLY);
    if (fd_ < 0) throw std::runtime_error("cannot open " + path);
    struct stat st;
    if (fstat(fd_, &st) != 0 || st.st_size < 26) throw std::runtime_error("not a CRAM file: " + path);
    size_ = (size_t)st.st_size;
    const std::vector<uint8_t> def = read_at(0, 26);
    if (memcmp(def.data(), "CRAM", 4) != 0) throw std::runtime_error("not a CRAM file: " + path);
    // 3.1 = 3.0 + four more block compression methods (no change to containers, slices, encodings or ITF8 integers)
    if (def[4] != 3 || def[5] > 1) throw std::runtime_error("CRAM " + std::to_string(def[4]) + "." + std::to_string(def[5]) + " is not supported (3.0 and 3.1 are)");
    off_ = 26;
    // the first container holds the SAM header
    ContainerHeader h = read_container_header();
    const std::vector<uint8_t> first = read_at(off_, h.length);
    cram::Cursor c(first.data(), first.size());
    cram::Block b = cram::read_block(c);
    cram::Cursor t(b.data.data(), b.data.size());
    const int32_t l_text = t.i32le();
    if (l_text < 0) throw std::runtime_error("CRAM: bad header length");
    t.need((size_t)l_text);
    header_text.assign(reinterpret_cast<const char*>(t.p + t.o), (size_t)l_text);
    off_ += h.length;
    size_t ls = 0;
    while (ls < header_text.size()) {
      size_t le = header_text.find('\n', ls);
      if (le == std::string::npos) le = header_text.size();
      if (header_text.compare(ls, 3, "@SQ") == 0) {
        std::string name;
        int32_t len = 0;
        size_t start = ls;
        for (size_t i = ls; i <= le; ++i)
          if (i == le || header_text[i] == '\t') {
            if (header_text.compare(start, 3, "SN:") == 0) name = header_text.substr(start + 3, i - start - 3);
            if (header_text.compare(start, 3, "LN:") == 0) len = atoi(header_text.c_str() + start + 3);
            start = i + 1;
          }
        ref_names.push_back(name);
        ref_lengths.push_back(len);
      }
      ls = le + 1;
    }
    if (cfg_.filter.active) {
      region_ref_id_ = -2;
      for (size_t i = 0; i < ref_names.size(); ++i)
        if (ref_names[i] == cfg_.filter.region.name) region_ref_id_ = (int32_t)i;
    }
    // decode threads: cfg.threads, else EXON_HIP_CRAM_THREADS, else the host's cores, at most 32.  Containers are independent
    // and the threads also build the batches, so the caller's thread only hands them out.  (On the GPU box -- 256 hardware
    // threads that deliver about 16 cores' worth of work -- throughput is flat from 16 threads up: 80-100 M records/s, the
    // per-container thread time growing in step with the thread count; EXON_HIP_CRAM_TRACE=1 prints the split.)
    // (round 4: the "16 cores' worth" is the container's CFS quota -- usable_cpus() in parallel.h reads it)
    const unsigned hc = (unsigned)usable_cpus();
    const char* ev = getenv("EXON_HIP_CRAM_THREADS");
    threads_ = cfg_.threads > 0 ? cfg_.threads : ev && atoi(ev) > 0 ? atoi(ev) : (int)std::min(32u, hc ? hc : 1u);
  }

  CRAMBatchReader(const CRAMBatchReader&) = delete;
  CRAMBatchReader& operator=(const CRAMBatchReader&) = delete;
  const BAMConfig& config() const { return cfg_; }

  // Batches are built by the threads that decode the containers (round 3, last): a container's records become its own
  // batches of at most batch_size rows -- a batch never spans two containers -- so this call, the only serial step of the
  // reader, hands out finished arrays.  (The reference's reader fills every batch to batch_size across container borders;
  // batch boundaries carry no meaning for the operators above a scan.)
  bool read_batch(struct ArrowArray* out) override {
    while (pending_.empty())
      if (!next_container()) return false;
    *out = pending_.front().a;
    pending_.front().a.release = nullptr;  // moved out
    pending_.pop_front();
    return true;
  }
  void schema(struct ArrowSchema* out) const override {
    make_schema(out, "+s", "", false,
                {new_field("i", "flag", false), new_field("C", "mapping_quality", true),
                 new_field("i", "reference", true, new_field("u", "", false)), new_field("l", "start", true),
                 new_field("l", "end", true)});
  }
  // read names of the records decoded so far (tests: the reference pins the first row's name)
  std::vector<std::string> names;
  bool keep_names = false;
  int64_t containers_skipped = 0;
  std::string header_text;
  std::vector<std::string> ref_names;
  std::vector<int32_t> ref_lengths;

 private:
  struct Rec {
    int32_t flag, ref_id;
    int64_t pos0, ref_len;
    int mapq;
  };
  struct OwnedBatch {  // an Arrow struct array that is released unless it is handed out
    struct ArrowArray a;
    OwnedBatch() { memset(&a, 0, sizeof a); }
    OwnedBatch(OwnedBatch&& o) noexcept : a(o.a) { o.a.release = nullptr; }
    OwnedBatch& operator=(OwnedBatch&& o) noexcept {
      if (this != &o) {
        if (a.release) a.release(&a);
        a = o.a;
        o.a.release = nullptr;
      }
      return *this;
    }
    OwnedBatch(const OwnedBatch&) = delete;
    OwnedBatch& operator=(const OwnedBatch&) = delete;
    ~OwnedBatch() {
      if (a.release) a.release(&a);
    }
  };
  // the records of one container as the columns BAMArrayBuilder keeps (values + one validity byte per row; NULL placeholders as
  // BAMArrayBuilder::append writes them), built by the thread that decoded the container
  struct Cols {
    std::vector<int32_t> flag, ref;
    std::vector<uint8_t> mapq, mapq_ok, ref_ok, pos_ok;
    std::vector<int64_t> start, end;
    size_t size() const { return flag.size(); }
    void clear() { flag.clear(), ref.clear(), mapq.clear(), mapq_ok.clear(), ref_ok.clear(), pos_ok.clear(), start.clear(), end.clear(); }
    void reserve(size_t n) {
      flag.reserve(n), ref.reserve(n), mapq.reserve(n), mapq_ok.reserve(n), ref_ok.reserve(n), pos_ok.reserve(n), start.reserve(n), end.reserve(n);
    }
    void push(const Rec& r) {
      flag.push_back(r.flag);
      mapq.push_back((uint8_t)r.mapq);  // 255 = missing (its own placeholder)
      mapq_ok.push_back(r.mapq != 255);
      ref.push_back(r.ref_id < 0 ? -1 : r.ref_id);
      ref_ok.push_back(r.ref_id >= 0);
      const bool has = r.pos0 >= 0;
      start.push_back(has ? r.pos0 + 1 : 0);                // 1-based
      end.push_back(has ? r.pos0 + 1 + r.ref_len - 1 : 0);  // alignment end = start + reference span - 1
      pos_ok.push_back(has);
    }
  };
  struct ContainerHeader {
    size_t length = 0;
    int32_t ref_id = 0;
    int64_t start = 0, span = 0;
    uint32_t n_records = 0, n_blocks = 0;
  };
  // The file is read container by container (positional reads: the workers fetch their own payloads); it is never held whole.
  std::vector<uint8_t> read_at(size_t off, size_t n) const {
    std::vector<uint8_t> buf;
    read_into(off, n, &buf);
    return buf;
  }
  void read_into(size_t off, size_t n, std::vector<uint8_t>* out) const {
    if (off > size_ || n > size_ - off) throw std::runtime_error("CRAM: read past the end of the file");
    std::vector<uint8_t>& buf = *out;
    buf.resize(n);
    size_t got = 0;
    while (got < n) {
      const ssize_t r = pread(fd_, buf.data() + got, n - got, (off_t)(off + got));
      if (r <= 0) throw std::runtime_error("CRAM: read error");
      got += (size_t)r;
    }
  }
  ContainerHeader read_container_header() {
    for (size_t window = 4096;; window *= 16) {  // the header is tens of bytes plus one ITF8 per slice landmark
      const size_t n = std::min(window, size_ - off_);
      const std::vector<uint8_t> buf = read_at(off_, n);
      try {
        cram::Cursor c(buf.data(), buf.size());
        ContainerHeader h;
        const int32_t len = c.i32le();
        if (len < 0) throw std::runtime_error("CRAM: negative container length");
        h.length = (size_t)len;
        h.ref_id = c.itf8s();
        h.start = c.itf8s();
        h.span = c.itf8s();
        h.n_records = c.itf8();
        (void)c.ltf8();
        (void)c.ltf8();
        h.n_blocks = c.itf8();
        const uint32_t nl = c.itf8();
        for (uint32_t i = 0; i < nl; ++i) (void)c.itf8();
        {  // CRC-32 of the container header bytes before it (CRAM 3.0 section 7)
          const size_t hdr = c.o;
          const uint32_t want = (uint32_t)c.i32le();
          {
#ifndef EXON_CRAM_FUZZ_SKIP_CRC
            if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), buf.data(), (uInt)hdr) != want) throw std::runtime_error("CRAM: container header CRC-32 mismatch");
#else
            (void)want;
#endif
          }
        }
        off_ += c.o;
        if (h.length > size_ - off_) throw std::runtime_error("CRAM: container runs past the end of the file");
        return h;
      } catch (const std::runtime_error& e) {
        if (n == size_ - off_ || window >= (size_t(1) << 28) || std::string(e.what()) != "CRAM: truncated data") throw;
      }
    }
  }

  // The next group of containers (those that can hold a hit), decoded on `threads` threads, appended in file order.  The group
  // after it is decoded in the background while the caller turns this one into batches (round 3: building the Arrow batches is
  // single-threaded and had the decoder threads idle for half of the time).
  // rows [o, o + n) of `k` as one struct array (the BAM device layout) whose nine buffers share one pooled block of the size a
  // full batch of `per` rows needs
  void make_batch(const Cols& k, size_t o, size_t n, size_t per, struct ArrowArray* out) const {
    auto pad = [](size_t b) { return (b + 63) & ~size_t(63); };
    // the block is sized for the rows it holds, rounded up to a power of two (size classes the pool can reuse) -- not for
    // batch_size, which a caller may set to millions of rows while a container holds ten thousand
    size_t cls = 1024;
    while (cls < n) cls <<= 1;
    per = std::min(per, cls);
    const size_t bm = pad(per / 8 + 16);
    const size_t bytes = 2 * pad(per * 8 + 64) + 2 * pad(per * 4 + 64) + pad(per + 64) + 4 * bm;
    uint8_t* base = static_cast<uint8_t*>(BlockPool::instance().get(bytes));
    uint8_t* p = base;
    auto take = [&](size_t b) {
      uint8_t* q = p;
      p += b;
      return q;
    };
    int64_t* start = reinterpret_cast<int64_t*>(take(pad(per * 8 + 64)));
    int64_t* end = reinterpret_cast<int64_t*>(take(pad(per * 8 + 64)));
    int32_t* flag = reinterpret_cast<int32_t*>(take(pad(per * 4 + 64)));
    int32_t* ref = reinterpret_cast<int32_t*>(take(pad(per * 4 + 64)));
    uint8_t* mapq = take(pad(per + 64));
    uint8_t* v_mapq = take(bm);
    uint8_t* v_ref = take(bm);
    uint8_t* v_pos = take(bm);
    uint8_t* v_pos2 = take(bm);  // start and end are separate arrays: separate bitmaps, same bits
    memcpy(start, k.start.data() + o, n * 8);
    memcpy(end, k.end.data() + o, n * 8);
    memcpy(flag, k.flag.data() + o, n * 4);
    memcpy(ref, k.ref.data() + o, n * 4);
    memcpy(mapq, k.mapq.data() + o, n);
    memset(reinterpret_cast<uint8_t*>(start) + n * 8, 0, 64);  // slack: consumers may read whole 16-byte vectors
    memset(reinterpret_cast<uint8_t*>(end) + n * 8, 0, 64);
    memset(reinterpret_cast<uint8_t*>(flag) + n * 4, 0, 64);
    memset(reinterpret_cast<uint8_t*>(ref) + n * 4, 0, 64);
    memset(mapq + n, 0, 64);
    auto pack = [&](const uint8_t* ok, uint8_t* bits) -> int64_t {  // byte per row -> Arrow bitmap; returns the NULL count
      memset(bits, 0, bm);
      int64_t nulls = 0;
      for (size_t i = 0; i < n; ++i) {
        bits[i >> 3] |= (uint8_t)((ok[i] & 1u) << (i & 7));
        nulls += !ok[i];
      }
      return nulls;
    };
    const int64_t n_mapq = pack(k.mapq_ok.data() + o, v_mapq), n_ref = pack(k.ref_ok.data() + o, v_ref), n_pos = pack(k.pos_ok.data() + o, v_pos);
    if (n_pos) memcpy(v_pos2, v_pos, bm);
    // the parent and every child hold a reference to the block: a consumer may move children out and release the parent first
    SharedBlock* blk = new SharedBlock();
    blk->block = base;
    blk->bytes = bytes;
    blk->put = &BlockPool::put;
    std::vector<struct ArrowArray*> kids = {
        new_view_array(blk, nullptr, flag, (int64_t)n, 0),
        new_view_array(blk, n_mapq ? v_mapq : nullptr, mapq, (int64_t)n, n_mapq),
        new_view_array(blk, n_ref ? v_ref : nullptr, ref, (int64_t)n, n_ref, utf8_array(ref_names)),
        new_view_array(blk, n_pos ? v_pos : nullptr, start, (int64_t)n, n_pos),
        new_view_array(blk, n_pos ? v_pos2 : nullptr, end, (int64_t)n, n_pos)};
    make_struct(out, (int64_t)n, std::move(kids));
    static_cast<OwnedArray*>(out->private_data)->block = blk;  // the creator's reference passes to the parent
  }

  struct Job {
    size_t off, length;
    std::vector<OwnedBatch> batches;
    std::vector<std::string> names;
    std::string error;
  };
  std::vector<Job> plan_group() {  // walks container headers (caller's thread)
    std::vector<Job> jobs;
    // a group = up to four containers per decode thread (the threads of a group are started once and pick containers from a
    // shared counter: one container per thread and group spent a third of the time starting threads and waiting for the
    // slowest one), at most 256 MiB of compressed containers; the sequential reader keeps one container at a time
    const size_t want = threads_ <= 1 ? 1 : (size_t)threads_ * 4;
    size_t bytes = 0;
    while (jobs.size() < want && bytes < (size_t(256) << 20) && off_ < size_) {
      const ContainerHeader h = read_container_header();
      const size_t end = off_ + h.length;
      bool take = h.n_records != 0;  // 0: the EOF container (or an empty one)
      // a pushed-down region: the container header says which reference and span its records cover (what a .crai entry
      // repeats), so containers that cannot hold a hit are skipped undecoded; multi-reference (-2) ones are always decoded
      if (take && cfg_.filter.active && h.ref_id != -2) {
        const Region& rg = cfg_.filter.region;
        take = h.ref_id == region_ref_id_ && h.ref_id >= 0 && (h.span <= 0 || (h.start <= rg.end && rg.start <= h.start + h.span - 1));
        if (!take) ++containers_skipped;
      }
      if (take) {
        Job j;
        j.off = off_;
        j.length = h.length;
        bytes += h.length;
        jobs.push_back(std::move(j));
      }
      off_ = end;
    }
    return jobs;
  }
  std::vector<Job> decode_group(std::vector<Job> jobs) const {  // any thread: positional reads, no shared state
    const long tg0 = now_us();
    // A decode thread keeps its large buffers (compressed container, records, columns) from one container to the next: freeing
    // and re-allocating them per container made glibc grow and trim the threads' heaps under the process-wide mmap lock (8
    // threads: 3.4 instead of 20+ M records/s).
    struct Scratch {
      std::vector<uint8_t> buf;
      std::vector<Rec> recs;
      Cols cols;
      cram::ByteCache bytes;
    };
    auto run = [this](Job& j, Scratch& sc) {
      try {
        const bool want_names = keep_names;
        const long t0 = now_us();
        read_into(j.off, j.length, &sc.buf);
        const long t1 = now_us();
        const std::vector<uint8_t>& buf = sc.buf;
        cram::Cursor c(buf.data(), buf.size());
        std::vector<Rec>& recs = sc.recs;
        recs.clear();
        decode_container(c, &recs, want_names ? &j.names : nullptr, &sc.bytes);
        const long t2 = now_us();
        Cols& cols = sc.cols;
        cols.clear();
        cols.reserve(recs.size());
        const bool filter = cfg_.filter.active;
        const Region& rg = cfg_.filter.region;
        for (const Rec& r : recs) {
          if (filter) {  // the range hit of the indexed BAM stream (cram_region_filter has the same meaning)
            if (r.ref_id < 0 || r.pos0 < 0) continue;
            const int64_t s = r.pos0 + 1, e = s + r.ref_len - 1;
            if (!(r.ref_id == region_ref_id_ && s <= rg.end && rg.start <= e)) continue;
          }
          cols.push(r);
        }
        const long t3 = now_us();
        const size_t per = (size_t)std::max<int64_t>(1, cfg_.batch_size);
        for (size_t o = 0; o < cols.size(); o += per) {
          const size_t n = std::min(per, cols.size() - o);
          OwnedBatch ob;
          make_batch(cols, o, n, per, &ob.a);
          j.batches.push_back(std::move(ob));
        }
        if (tracing()) {
          const long t4 = now_us();
          trace_.read += t1 - t0, trace_.decode += t2 - t1, trace_.columns += t3 - t2, trace_.batches += t4 - t3, ++trace_.containers;
        }
      } catch (const std::exception& e) {
        j.error = e.what();
        if (j.error.empty()) j.error = "CRAM: decode error";
      }
    };
    if (jobs.size() == 1 || threads_ <= 1) {
      Scratch sc;
      for (Job& j : jobs) run(j, sc);
    } else {
      // the reader's decode threads live as long as the reader (started with the first group): starting `threads_` threads per
      // group cost their stacks' mmap / munmap under the process-wide lock every few milliseconds
      Workers& w = *workers_;
      std::unique_lock<std::mutex> lk(w.mu);
      if (w.threads.empty()) {
        const size_t n = (size_t)std::max(1, threads_);
        for (size_t i = 0; i < n; ++i)
          w.threads.emplace_back([&w, run] {
            Scratch sc;
            std::unique_lock<std::mutex> l(w.mu);
            for (;;) {
              w.cv_work.wait(l, [&w] { return w.stop || (w.jobs && w.next < w.jobs->size()); });
              if (w.stop) return;
              Job& j = (*w.jobs)[w.next++];
              l.unlock();
              run(j, sc);  // never throws: errors are kept in the job
              l.lock();
              if (++w.done == w.jobs->size()) w.cv_done.notify_all();
            }
          });
      }
      w.jobs = &jobs;
      w.next = w.done = 0;
      w.cv_work.notify_all();
      w.cv_done.wait(lk, [&w, &jobs] { return w.done == jobs.size(); });
      w.jobs = nullptr;
    }
    if (tracing()) trace_.group += now_us() - tg0, ++trace_.groups;
    return jobs;
  }
  void start_ahead() {  // header errors (a malformed container header) surface here, in file order, as before
    const long tp0 = now_us();
    std::vector<Job> jobs = plan_group();
    trace_.plan += now_us() - tp0;
    if (jobs.empty()) return;
    if (threads_ <= 1) {  // sequential reader: no helper thread either
      std::promise<std::vector<Job>> p;
      ahead_ = p.get_future();
      p.set_value(std::move(jobs));
      ahead_deferred_ = true;
      return;
    }
    ahead_deferred_ = false;
    ahead_ = std::async(std::launch::async, [this](std::vector<Job> j) { return decode_group(std::move(j)); }, std::move(jobs));
  }
  bool next_container() {
    if (!ahead_.valid()) start_ahead();
    if (!ahead_.valid()) return false;
    const long tw0 = now_us();
    std::vector<Job> jobs = ahead_.get();
    trace_.wait += now_us() - tw0;
    if (ahead_deferred_) jobs = decode_group(std::move(jobs));
    start_ahead();  // the next group decodes while this one is consumed
    for (auto& j : jobs) {
      if (!j.error.empty()) throw std::runtime_error(j.error);
      for (auto& ob : j.batches) pending_.push_back(std::move(ob));
      if (keep_names) names.insert(names.end(), j.names.begin(), j.names.end());
    }
    return true;
  }

  struct Series {  // the data series this decoder reads, resolved once per container
    cram::Encoding BF, CF, RI, RL, AP, RG, RN, MF, NS, NP, TS, NF, TL, FN, FC, FP, DL, BA, QS, BS, IN, SC, RS, PD, HC, MQ, BB, QQ;
  };

  void decode_container(cram::Cursor& c, std::vector<Rec>* out, std::vector<std::string>* out_names, cram::ByteCache* cache = nullptr) const {
    using namespace cram;
    Block ch = read_block(c);
    if (ch.type != 1) throw std::runtime_error("CRAM: compression header expected");
    Cursor h(ch.data.data(), ch.data.size());
    bool rn_preserved = true, ap_delta = true;
    std::vector<std::vector<uint32_t>> tag_lines;
    {
      (void)h.itf8();
      const uint32_t n = h.itf8();
      for (uint32_t i = 0; i < n; ++i) {
        const char k0 = (char)h.u8(), k1 = (char)h.u8();
        if (k0 == 'R' && k1 == 'N') rn_preserved = h.u8() != 0;
        else if (k0 == 'A' && k1 == 'P') ap_delta = h.u8() != 0;
        else if (k0 == 'R' && k1 == 'R') (void)h.u8();
        else if (k0 == 'S' && k1 == 'M') h.skip(5);
        else if (k0 == 'T' && k1 == 'D') {
          const uint32_t ln = h.itf8();
          h.need(ln);
          std::vector<uint32_t> line;
          for (uint32_t q = 0; q < ln;) {
            if (h.p[h.o + q] == 0) {
              tag_lines.push_back(line);
              line.clear();
              ++q;
              continue;
            }
            if (q + 3 > ln) throw std::runtime_error("CRAM: malformed tag dictionary");
            line.push_back(((uint32_t)h.p[h.o + q] << 16) | ((uint32_t)h.p[h.o + q + 1] << 8) | h.p[h.o + q + 2]);
            q += 3;
          }
          h.skip(ln);
        } else {
          throw std::runtime_error("CRAM: preservation key " + cram::printable(k0) + cram::printable(k1));
        }
      }
    }
    Series S;
    {
      (void)h.itf8();
      const uint32_t n = h.itf8();
      for (uint32_t i = 0; i < n; ++i) {
        const char k0 = (char)h.u8(), k1 = (char)h.u8();
        Encoding e = read_encoding(h);
#define EXON_CRAM_DS(K) if (k0 == #K[0] && k1 == #K[1]) S.K = std::move(e); else
        EXON_CRAM_DS(BF) EXON_CRAM_DS(CF) EXON_CRAM_DS(RI) EXON_CRAM_DS(RL) EXON_CRAM_DS(AP) EXON_CRAM_DS(RG) EXON_CRAM_DS(RN)
        EXON_CRAM_DS(MF) EXON_CRAM_DS(NS) EXON_CRAM_DS(NP) EXON_CRAM_DS(TS) EXON_CRAM_DS(NF) EXON_CRAM_DS(TL) EXON_CRAM_DS(FN)
        EXON_CRAM_DS(FC) EXON_CRAM_DS(FP) EXON_CRAM_DS(DL) EXON_CRAM_DS(BA) EXON_CRAM_DS(QS) EXON_CRAM_DS(BS) EXON_CRAM_DS(IN)
        EXON_CRAM_DS(SC) EXON_CRAM_DS(RS) EXON_CRAM_DS(PD) EXON_CRAM_DS(HC) EXON_CRAM_DS(MQ) EXON_CRAM_DS(BB) EXON_CRAM_DS(QQ)
        {}  // a data series this path never reads (TC, TN, TM, TV ...)
#undef EXON_CRAM_DS
      }
    }
    std::vector<std::pair<uint32_t, Encoding>> tags;
    {
      (void)h.itf8();
      const uint32_t n = h.itf8();
      for (uint32_t i = 0; i < n; ++i) {
        const uint32_t key = h.itf8();
        tags.emplace_back(key, read_encoding(h));
      }
    }
    // tag lines as indexes into `tags`
    std::vector<std::vector<int>> tag_idx(tag_lines.size());
    for (size_t l = 0; l < tag_lines.size(); ++l)
      for (uint32_t key : tag_lines[l]) {
        int at = -1;
        for (size_t t = 0; t < tags.size(); ++t)
          if (tags[t].first == key) at = (int)t;
        if (at < 0) throw std::runtime_error("CRAM: tag without an encoding");
        tag_idx[l].push_back(at);
      }
    auto need = [](const Encoding& e, const char* k) -> const Encoding& {
      if (e.kind == Encoding::NONE) throw std::runtime_error(std::string("CRAM: data series ") + k + " has no encoding");
      return e;
    };
#define DS(K) need(S.K, #K)
    while (c.o < c.n) {
      Block sh = read_block(c);
      if (sh.type != 2) throw std::runtime_error("CRAM: slice header expected");
      Cursor s(sh.data.data(), sh.data.size());
      const int32_t s_ref = s.itf8s();
      const int32_t s_start = s.itf8s();
      (void)s.itf8();
      const uint32_t s_nrec = s.itf8();
      (void)s.ltf8();
      const uint32_t s_nblocks = s.itf8();
      SliceData sl;
      sl.cache = cache;
      for (uint32_t i = 0; i < s_nblocks; ++i) {
        static const bool eager = getenv("EXON_HIP_CRAM_EAGER") != nullptr;  // A/B: expand every block, as round 2 did
        Block b = read_block(c, /*lazy=*/true, cache);  // external blocks are expanded when a series first reads them
        if (eager && b.method <= 5) b.expand();  // (a block in a codec this reader lacks stays closed either way)
        if (b.type == 5) {
          b.expand();
          sl.core.swap(b.data);
        } else if (b.type == 4) {
          sl.add(std::move(b));
        }
      }
      sl.finish_blocks();
      for (Encoding* e : {&S.BF, &S.CF, &S.RI, &S.RL, &S.AP, &S.RG, &S.RN, &S.MF, &S.NS, &S.NP, &S.TS, &S.NF, &S.TL, &S.FN, &S.FC, &S.FP,
                          &S.DL, &S.BA, &S.QS, &S.BS, &S.IN, &S.SC, &S.RS, &S.PD, &S.HC, &S.MQ, &S.BB, &S.QQ})
        sl.bind(*e);
      for (auto& t : tags) sl.bind(t.second);
      // the series whose values reach the columns (or steer the decode): everything else is discarded unread
      for (const Encoding* e : {&S.BF, &S.CF, &S.RI, &S.RL, &S.AP, &S.TL, &S.FN, &S.FC, &S.DL, &S.RS, &S.MQ}) sl.need_values(*e);
      for (const Encoding* e : {&S.IN, &S.SC})  // byte arrays of which only the LENGTH counts (reference span)
        if (e->kind == Encoding::BYTE_ARRAY_LEN) sl.need_values(*e->len_enc);
        else sl.need_values(*e);  // BYTE_ARRAY_STOP: the length is found by scanning the bytes
      if (out_names) sl.need_values(S.RN);
      out->reserve(out->size() + s_nrec);
      int64_t prev = s_start;
      for (uint32_t r = 0; r < s_nrec; ++r) {
        Rec rec;
        rec.flag = sl.get_int(DS(BF));
        const int32_t cf = sl.get_int(DS(CF));
        rec.ref_id = s_ref == -2 ? sl.get_int(DS(RI)) : s_ref;
        const int32_t rl = sl.get_int(DS(RL));
        if (rl < 0) throw std::runtime_error("CRAM: negative read length");
        int64_t ap = sl.get_int(DS(AP));
        if (ap_delta) {
          ap += prev;
          prev = ap;
        }
        sl.skip_int(DS(RG));
        std::string name;
        if (rn_preserved) sl.skip_bytes(DS(RN), out_names ? &name : nullptr, false);
        if (cf & 2) {
          sl.skip_int(DS(MF));
          if (!rn_preserved) sl.skip_bytes(DS(RN), out_names ? &name : nullptr, false);
          sl.skip_int(DS(NS));
          sl.skip_int(DS(NP));
          sl.skip_int(DS(TS));
        } else if (cf & 4) {
          sl.skip_int(DS(NF));
        }
        const int32_t tl = sl.get_int(DS(TL));
        if (tl < 0 || (size_t)tl >= tag_idx.size()) throw std::runtime_error("CRAM: tag line out of range");
        for (int t : tag_idx[(size_t)tl]) sl.skip_bytes(tags[(size_t)t].second, nullptr, false);
        int64_t span = rl;
        rec.mapq = 255;
        if (!(rec.flag & 4)) {
          const int32_t fn = sl.get_int(DS(FN));
          for (int32_t i = 0; i < fn; ++i) {
            const char code = (char)sl.get_byte(DS(FC));
            sl.skip_int(DS(FP));
            switch (code) {
              case 'B': sl.skip_byte(DS(BA)); sl.skip_byte(DS(QS)); break;
              case 'X': sl.skip_byte(DS(BS)); break;
              case 'I': span -= (int64_t)sl.skip_bytes(DS(IN)); break;
              case 'i': sl.skip_byte(DS(BA)); span -= 1; break;
              case 'D': span += sl.get_int(DS(DL)); break;
              case 'S': span -= (int64_t)sl.skip_bytes(DS(SC)); break;
              case 'N': span += sl.get_int(DS(RS)); break;
              case 'P': sl.skip_int(DS(PD)); break;
              case 'H': sl.skip_int(DS(HC)); break;
              case 'Q': sl.skip_byte(DS(QS)); break;
              case 'b': sl.skip_bytes(DS(BB), nullptr, false); break;
              case 'q': sl.skip_bytes(DS(QQ), nullptr, false); break;
              default: throw std::runtime_error("CRAM: read feature " + printable(code));
            }
          }
          rec.mapq = sl.get_int(DS(MQ));
          if (cf & 1) sl.skip_n(DS(QS), (size_t)rl);
        } else {
          sl.skip_n(DS(BA), (size_t)rl);
          if (cf & 1) sl.skip_n(DS(QS), (size_t)rl);
          span = 0;  // no CIGAR: as in the BAM path, end = start - 1
        }
        rec.pos0 = ap - 1;  // 0 -> "no position" (-1)
        rec.ref_len = span;
        if (rec.mapq < 0 || rec.mapq > 255) rec.mapq = 255;
        out->push_back(rec);
        if (out_names) out_names->push_back(name);
      }
    }
#undef DS
  }

  BAMConfig cfg_;
  int threads_ = 1;
  struct Fd {  // closes on destruction, also when the constructor throws
    int v = -1;
    ~Fd() {
      if (v >= 0) ::close(v);
    }
  } fdh_;
  int fd_ = -1;
  size_t size_ = 0, off_ = 0;
  std::deque<OwnedBatch> pending_;  // finished batches of the decoded containers, in file order
  int32_t region_ref_id_ = -2;
  // EXON_HIP_CRAM_TRACE=1: where a scan's wall time went, printed when the reader closes (microseconds; the per-container
  // parts are sums over all decode threads)
  struct Trace {
    std::atomic<long> plan{0}, wait{0}, group{0}, read{0}, decode{0}, columns{0}, batches{0}, groups{0}, containers{0};
  };
  mutable Trace trace_;
  static bool tracing() {
    static const bool on = getenv("EXON_HIP_CRAM_TRACE") != nullptr;
    return on;
  }
  static long now_us() { return (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  struct Workers {  // decode threads + the group they are working on (decode_group)
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::vector<std::thread> threads;
    std::vector<Job>* jobs = nullptr;
    size_t next = 0, done = 0;
    bool stop = false;
  };
  std::unique_ptr<Workers> workers_{new Workers};
  bool ahead_deferred_ = false;
  std::future<std::vector<Job>> ahead_;  // a group being decoded in the background

 public:
  ~CRAMBatchReader() {  // the background group first (it uses the decode threads and the file), then the threads
    if (ahead_.valid()) ahead_.wait();
    {
      std::lock_guard<std::mutex> g(workers_->mu);
      workers_->stop = true;
    }
    workers_->cv_work.notify_all();
    for (auto& t : workers_->threads) t.join();
    if (tracing())
      fprintf(stderr, "[exon-hip cram] %ld containers in %ld groups on %d threads: caller planned %.1f ms, waited %.1f ms for groups; groups took %.1f ms; "
              "per container (thread time) read %.0f us, decode %.0f us, columns %.0f us, batches %.0f us\n",
              trace_.containers.load(), trace_.groups.load(), threads_, trace_.plan / 1e3, trace_.wait / 1e3, trace_.group / 1e3,
              (double)trace_.read / std::max(1L, trace_.containers.load()), (double)trace_.decode / std::max(1L, trace_.containers.load()),
              (double)trace_.columns / std::max(1L, trace_.containers.load()), (double)trace_.batches / std::max(1L, trace_.containers.load()));
  }
};

}  // namespace exon
