// bitmap_host_harness.cpp -- a stand-alone program over the bit appender of the staging layer (exon_amd/csrc/host/bitmap.h:
// append_bits) for tests/test_bitmap_host_harness.py, which builds it with -fsanitize=address,undefined and compares what it
// prints with np.packbits.
//   bitmap_host_harness <script>
// The script is text, one token list a line:
//   case <start> <total>     a destination of exactly (total + 7) / 8 zeroed heap bytes; appending begins at bit <start>
//   run <n> <src_off> <hex>  append n bits read from bit <src_off> of the bytes <hex>, which are copied to a heap block of
//                            exactly their size ("-" as <hex>: no source, src == nullptr = n valid rows; "." : zero bytes)
//   end                      print the destination as hex ("." when it has no byte)
// Every block has its exact size, so a byte read or written past either end is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host/bitmap.h"

static int nibble(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: bitmap_host_harness <script>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::string line, word;
  uint8_t* dst = nullptr;
  size_t dst_bytes = 0;
  int64_t pos = 0, total = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    if (!(ls >> word)) continue;
    if (word == "case") {
      ls >> pos >> total;
      dst_bytes = (size_t)((total + 7) / 8);
      dst = static_cast<uint8_t*>(malloc(dst_bytes));  // (malloc(0) is a valid block of no bytes)
      if (dst_bytes) memset(dst, 0, dst_bytes);
    } else if (word == "run") {
      int64_t n = 0, src_off = 0;
      std::string hex;
      ls >> n >> src_off >> hex;
      uint8_t* src = nullptr;
      if (hex != "-") {
        const size_t nb = hex == "." ? 0 : hex.size() / 2;
        src = static_cast<uint8_t*>(malloc(nb));
        for (size_t i = 0; i < nb; ++i) src[i] = (uint8_t)(nibble(hex[2 * i]) * 16 + nibble(hex[2 * i + 1]));
      }
      if (pos + n > total) {
        fprintf(stderr, "script error: run past the end of its case\n");
        return 2;
      }
      exon::append_bits(dst, pos, src, src_off, n);
      pos += n;
      free(src);
    } else if (word == "end") {
      std::string out;
      static const char* digits = "0123456789abcdef";
      for (size_t i = 0; i < dst_bytes; ++i) {
        out.push_back(digits[dst[i] >> 4]);
        out.push_back(digits[dst[i] & 15]);
      }
      puts(out.empty() ? "." : out.c_str());
      free(dst);
      dst = nullptr;
    } else {
      fprintf(stderr, "script error: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
