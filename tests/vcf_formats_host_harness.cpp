// vcf_formats_host_harness.cpp -- a stand-alone program over the per-item walk of the `formats` column
// (exon_amd/csrc/host/vcf_sample_walk.h: format_keys, sample, value, genotype -- what the k_fmt_* kernels of text_columns.hip
// instantiate) for tests/test_vcf_formats_host_harness.py, which builds it with -fsanitize=address,undefined and compares what it
// prints with oracle/decode.py.
//   vcf_formats_host_harness <file>
//       line 1 of <file>: the FORMAT key types, "KEY=kind,KEY=kind,..." (kinds i f c s; may be empty)
//       every other line: what follows the INFO field of a VCF data line -- "" (no FORMAT field), else TAB FORMAT (TAB sample)*
//   For every such line four lines come out:
//       the column's string put together item by item the way the kernels do (head = FORMAT + TAB, then every sample with its
//         TAB in front), measured first and then filled into a heap buffer of exactly the measured size with 16 guard bytes
//         behind it -- or UNDECIDED
//       exon::vcf_formats_string's string on the same input (host/vcf_text.h, the authority) -- or ERROR
//       len=1 when the fill wrote exactly the measured bytes (0 otherwise; 1 for UNDECIDED)
//       guard=1 when the guard bytes are intact
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "exon_hip.h"
#include "host/formats.h"
#include "host/vcf_sample_walk.h"

namespace {

unsigned dec_digits(uint32_t v) {
  unsigned d = 1;
  while (v >= 10) {
    v /= 10;
    ++d;
  }
  return d;
}
struct Measure {
  unsigned n = 0;
  void byte(unsigned) { ++n; }
  void span(unsigned, unsigned len) { n += len; }
  void i32(bool minus, uint32_t v) { n += (minus ? 1u : 0u) + dec_digits(v); }
  void f32(uint32_t bits) { n += (unsigned)exon::f32p::length(bits); }
};
// writes at dst[w ..); nothing at or behind dst[lim] (the device emitter's bounds)
struct Fill {
  const uint8_t* text;
  uint8_t* dst;
  unsigned lim, w = 0;
  void byte(unsigned c) {
    if (w < lim) dst[w] = (uint8_t)c;
    ++w;
  }
  void span(unsigned off, unsigned len) {
    if (len <= lim && w <= lim - len) memcpy(dst + w, text + off, len);
    w += len;
  }
  void i32(bool minus, uint32_t v) {
    const unsigned nd = dec_digits(v), len = nd + (minus ? 1u : 0u);
    if (len <= lim && w <= lim - len) {
      if (minus) dst[w] = '-';
      uint8_t* p = dst + w + (minus ? 1u : 0u);
      for (unsigned i = nd; i > 0; --i) {
        p[i - 1] = (uint8_t)('0' + v % 10);
        v /= 10;
      }
    }
    w += len;
  }
  void f32(uint32_t bits) {
    const unsigned len = (unsigned)exon::f32p::length(bits);
    if (len <= lim && w <= lim - len) exon::f32p::print(bits, dst + w);
    w += len;
  }
};

// the items of one line tail, walked with emitter `em` (one for all items: the places add up as the device's scan does).  false: undecided
template <class Emit>
bool walk_line(const uint8_t* text, unsigned n, const exon::VcfKeyTypes& types, Emit& em) {
  std::vector<unsigned> tabs;  // (the tab index of the line: tab 0 is the one in front of FORMAT)
  for (unsigned i = 0; i < n; ++i)
    if (text[i] == '\t') tabs.push_back(i);
  uint64_t ty = 0;
  if (!tabs.empty()) {
    const unsigned fb = tabs[0] + 1, fe = tabs.size() > 1 ? tabs[1] : n;
    auto type_of = [&](unsigned kb, unsigned kn) {
      const char t = types.format_type(reinterpret_cast<const char*>(text) + kb, kn);
      return t == 'b' ? 's' : t;
    };
    if (!exon::vsw::format_keys(text, fb, fe, type_of, &ty)) return false;
    if (ty) {
      if (tabs.size() == 1) return false;  // FORMAT and no sample
      em.span(fb, fe - fb);
    }
  }
  em.byte('\t');
  if (!ty) return true;
  for (size_t t = 1; t < tabs.size(); ++t) {
    if (t > 1) em.byte('\t');
    if (exon::vsw::sample(text, tabs[t] + 1, t + 1 < tabs.size() ? tabs[t + 1] : n, ty, em)) return false;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: vcf_formats_host_harness <file>\n");
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  std::string line;
  if (!std::getline(in, line)) return 2;
  exon::VcfKeyTypes types;
  for (size_t a = 0; a < line.size();) {
    size_t e = line.find(',', a);
    if (e == std::string::npos) e = line.size();
    const size_t eq = line.find('=', a);
    if (eq != std::string::npos && eq + 1 < e) types.format.emplace(line.substr(a, eq - a), line[eq + 1]);
    a = e + 1;
  }
  auto pf = [](const char* p, size_t n) { return exon::VCFArrayBuilder::parse_f32(p, n); };
  while (std::getline(in, line)) {
    // heap copies of exactly the line's bytes: a read past either end is the sanitizer's to report
    const unsigned n = (unsigned)line.size();
    std::vector<uint8_t> text(line.begin(), line.end());
    const uint8_t* tp = text.empty() ? reinterpret_cast<const uint8_t*>("") : text.data();
    Measure m;
    const bool decided = walk_line(tp, n, types, m);
    bool len_ok = true, guard_ok = true;
    if (decided) {
      std::vector<uint8_t> buf((size_t)m.n + 16, 0xA5);
      Fill f{tp, buf.data(), m.n};
      const bool again = walk_line(tp, n, types, f);
      len_ok = again && f.w == m.n;
      for (size_t i = m.n; i < buf.size(); ++i) guard_ok = guard_ok && buf[i] == 0xA5;
      fwrite(buf.data(), 1, m.n, stdout);
      fputc('\n', stdout);
    } else {
      puts("UNDECIDED");
    }
    std::string host;
    try {
      const bool has = n > 0;  // (the builder: nf >= 9)
      const size_t f0 = 1;
      size_t f1 = has ? line.find('\t', f0) : std::string::npos;
      const bool has_samples = f1 != std::string::npos;
      if (!has_samples) f1 = line.size();
      exon::vcf_formats_string(has ? line.data() + f0 : nullptr, has ? f1 - f0 : 0, has_samples ? line.data() + f1 + 1 : nullptr, has_samples ? line.size() - f1 - 1 : 0, types, pf,
                               &host);
      fwrite(host.data(), 1, host.size(), stdout);
      fputc('\n', stdout);
    } catch (const std::exception&) {
      puts("ERROR");
    }
    printf("len=%d\nguard=%d\n", len_ok ? 1 : 0, guard_ok ? 1 : 0);
  }
  return 0;
}
