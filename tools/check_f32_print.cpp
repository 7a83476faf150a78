// check_f32_print -- host/f32_print.h against exon::rust_f32_display (host/vcf_text.h, std::to_chars) bit pattern by bit pattern:
// the same bytes, the same length from the length-only mode, nothing written past the length, never more than kF32PrintMax.
//   g++ -O2 -std=c++17 -pthread tools/check_f32_print.cpp -o check_f32_print
//   ./check_f32_print            the boundary sets + every 64th bit pattern
//   ./check_f32_print --stride N every Nth bit pattern instead
//   ./check_f32_print --all      all 2^32 bit patterns, on 16 threads
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../exon_amd/csrc/host/f32_print.h"
#include "../exon_amd/csrc/host/vcf_text.h"

namespace {
struct Tally {
  uint64_t checked = 0, mismatches = 0;
  int longest = 0;
};
void check(uint32_t bits, Tally* t) {
  float v;
  memcpy(&v, &bits, 4);
  std::string want;
  exon::rust_f32_display(v, &want);
  char buf[exon::f32p::kF32PrintMax + 8];
  memset(buf, '#', sizeof buf);
  const int n = exon::f32p::print(bits, buf), m = exon::f32p::length(bits);
  bool ok = n == m && n <= exon::f32p::kF32PrintMax && (size_t)n == want.size() && memcmp(buf, want.data(), (size_t)n) == 0;
  for (size_t i = (size_t)(n < 0 ? 0 : n); ok && i < sizeof buf; ++i) ok = buf[i] == '#';
  ++t->checked;
  if (n > t->longest) t->longest = n;
  if (!ok) {
    if (t->mismatches < 20) printf("MISMATCH %08x got '%.*s' (%d, length %d) want '%s'\n", bits, n > 0 && n < (int)sizeof buf ? n : 0, buf, n, m, want.c_str());
    ++t->mismatches;
  }
}
void both_signs(uint32_t mag, Tally* t) {
  check(mag, t);
  check(mag | 0x80000000u, t);
}
}  // namespace

int main(int argc, char** argv) {
  bool all = false;
  uint32_t stride = 64;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--all")) all = true;
    else if (!strcmp(argv[i], "--stride") && i + 1 < argc) stride = (uint32_t)strtoul(argv[++i], nullptr, 10);
    else return fprintf(stderr, "usage: %s [--all | --stride N]\n", argv[0]), 2;
  }
  if (stride == 0) stride = 1;
  Tally t;
  // every exponent (0 = subnormals, 255 = inf / NaN) with the mantissas at the ends and in the middle
  const uint32_t mants[] = {0u, 1u, 2u, 1u << 22, (1u << 23) - 2u, (1u << 23) - 1u};
  for (uint32_t e = 0; e < 256; ++e)
    for (uint32_t m : mants) both_signs(e << 23 | m, &t);
  // the subnormals 2^k and 2^k +- 1
  for (int k = 0; k < 23; ++k)
    for (int d = -1; d <= 1; ++d) {
      const uint32_t b = (uint32_t)((int64_t)(1u << k) + d);
      if (b < (1u << 23)) both_signs(b, &t);
    }
  // the binary32 next to every power of ten it can hold, and both neighbours of it
  for (int k = -45; k <= 38; ++k) {
    const std::string s = "1e" + std::to_string(k);
    const float f = strtof(s.c_str(), nullptr);
    uint32_t b;
    memcpy(&b, &f, 4);
    for (int d = -1; d <= 1; ++d) both_signs((uint32_t)((int64_t)b + d), &t);
  }
  if (!all) {
    for (uint64_t b = 0; b < (1ull << 32); b += stride) check((uint32_t)b, &t);
  } else {
    const int nt = 16;
    std::vector<Tally> part((size_t)nt);
    std::vector<std::thread> th;
    for (int k = 0; k < nt; ++k)
      th.emplace_back([&part, k, nt] {
        const uint64_t lo = (1ull << 32) / nt * k, hi = (1ull << 32) / nt * (k + 1);
        for (uint64_t b = lo; b < hi; ++b) check((uint32_t)b, &part[(size_t)k]);
      });
    for (auto& x : th) x.join();
    for (const Tally& p : part) {
      t.checked += p.checked;
      t.mismatches += p.mismatches;
      if (p.longest > t.longest) t.longest = p.longest;
    }
  }
  printf("checked %llu, longest %d, mismatches %llu\n", (unsigned long long)t.checked, t.longest, (unsigned long long)t.mismatches);
  return t.mismatches != 0;
}
