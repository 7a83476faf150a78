// fasta_host_harness.cpp -- a stand-alone program over the FASTA reader of exon_amd/csrc/host/formats.h for
// tests/test_fasta_host_harness.py, which builds it with -fsanitize=address,undefined and compares what it prints with
// tests/fasta_expect.py.  What the GPU pipeline needs of the reader: a look at the first byte that loses nothing, and the whole input
// handed over as a byte stream.
//   fasta_host_harness rows <file> <batch_size> <peek>   the file through FASTABatchReader, first_byte() called first when <peek> is 1:
//                                                        "FIRST <byte or -1>", then a row a line: id TAB description (\N for NULL) TAB
//                                                        sequence, every byte outside 0x21 .. 0x7e and the backslash as \xHH
//   fasta_host_harness stream <file>                     "FIRST <byte>", "OFFSET <data_offset>", then "BYTES <n>" and the n bytes
//                                                        take_stream() yields: the carry, then the source to its end
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "host/formats.h"

static void put(const char* p, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const unsigned char c = (unsigned char)p[i];
    if (c < 0x21 || c > 0x7e || c == '\\') printf("\\x%02X", c);
    else putchar(c);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  try {
    exon::FASTAConfig cfg;
    if (mode == "rows") {
      cfg.batch_size = atoll(argv[3]);
      exon::FASTABatchReader r(argv[2], exon::Compression::Auto, cfg);
      if (atoi(argv[4])) printf("FIRST %d\n", r.first_byte());
      struct ArrowArray a;
      for (;;) {
        memset(&a, 0, sizeof a);
        if (!r.read_batch(&a)) break;
        if (a.n_children != 3) return 3;
        for (int64_t i = 0; i < a.length; ++i) {
          for (int c = 0; c < 3; ++c) {
            const struct ArrowArray* k = a.children[c];
            const uint8_t* valid = static_cast<const uint8_t*>(k->buffers[0]);
            const int32_t* off = static_cast<const int32_t*>(k->buffers[1]);
            const char* data = static_cast<const char*>(k->buffers[2]);
            const int64_t j = i + k->offset;
            if (c) putchar('\t');
            if (valid && !((valid[j >> 3] >> (j & 7)) & 1)) printf("\\N");
            else put(data + off[j], (size_t)(off[j + 1] - off[j]));
          }
          putchar('\n');
        }
        a.release(&a);
      }
      return 0;
    }
    if (mode == "stream") {
      exon::FASTABatchReader r(argv[2], exon::Compression::Auto, cfg);
      printf("FIRST %d\nOFFSET %lld\n", r.first_byte(), (long long)r.data_offset());
      std::string all;
      std::unique_ptr<exon::ByteSource> src = r.take_stream(&all);
      std::vector<uint8_t> buf(1 << 16);
      for (size_t n; src && (n = src->read(buf.data(), buf.size())) > 0;) all.append(reinterpret_cast<const char*>(buf.data()), n);
      printf("BYTES %zu\n", all.size());
      fwrite(all.data(), 1, all.size(), stdout);
      return 0;
    }
  } catch (const std::exception& e) {
    printf("ERROR %s\n", e.what());
    return 0;
  }
  return 2;
}
