// The host readers' block inflater (exon_amd/csrc/host/bgzf_block.h: header walk, zlib inflateInit2(-15), ISIZE and CRC-32 checks) over
// BGZF members handed in on stdin, for tests/test_deflate_expect.py.  No GPU, no library: the header the product is built from.
//   in : repeated { u32 n, n bytes of one member }
//   out: repeated { u8 ok, u32 n, n bytes: the inflated bytes, or the refusal's text }
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host/bgzf_block.h"

int main() {
  z_stream z;
  memset(&z, 0, sizeof z);
  if (inflateInit2(&z, -15) != Z_OK) return 2;
  std::vector<uint8_t> in, out(exon::BGZF_MAX_BLOCK + 8);
  for (;;) {
    uint32_t n = 0;
    if (fread(&n, 4, 1, stdin) != 1) break;
    in.resize(n);
    if (n && fread(in.data(), 1, n, stdin) != n) return 3;
    uint8_t ok = 1;
    std::string msg;
    uint32_t len = 0;
    try {
      exon::BgzfBlockInfo info;
      exon::bgzf_block_info(in.data(), in.size(), &info, "member");
      exon::inflate_bgzf_block(&z, in.data(), info, out.data(), "member");
      len = info.isize;
    } catch (const std::exception& e) {
      ok = 0;
      msg = e.what();
      len = (uint32_t)msg.size();
    }
    fwrite(&ok, 1, 1, stdout);
    fwrite(&len, 4, 1, stdout);
    fwrite(ok ? (const void*)out.data() : (const void*)msg.data(), 1, len, stdout);
  }
  inflateEnd(&z);
  return 0;
}
