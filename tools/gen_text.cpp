// gen_text.cpp -- developer tool: writes the synthetic config-4 table as VCF text (same counter-based generator as
// kernels.hip / oracle) so the decode -> HBM -> kernel pipeline can be timed end to end on real files.
// `gen_text fastq <reads> <out> [read_len=150] [ragged=0]` writes 4-line FASTQ records (config 5 end to end);
// `gen_text bam <reads> <out> [read_len=100]` an uncompressed BAM stream (bgzip it to get a .bam; config 3 end to end).
// `gen_text gff <rows> <out>` a GFF3 table sorted by (seqname, start), so that bgzip + a tabix index (GFF preset) serve it;
// `gen_text gff <rows> <out> attrs` the same rows with rich ninth fields (every shape of the attribute rules, ASCII only).
// `gen_text gtf <rows> <out> [attrs]` an Ensembl-like GTF table with the same (seqname, start) layout; attrs: rich ninth fields.
// `gen_text bed <rows> <out> [n=6]` a BED table of n-field lines (3, 4, 5, 6 or 12; `mix`: all five, changing from row to row),
// sorted by (reference_sequence_name, start); 0-based starts, scores 0 .. 65535, strands + - .
// `gen_text vcf <rows> <out> [samples=0]` with samples > 0: a FORMAT field GT:DP:GQ:PL and that many samples behind every row
// (##FORMAT lines and sample names in the header); 0 writes the file without them, byte for byte as before.
// build: g++ -O2 -std=c++17 tools/gen_text.cpp -o tools/bin/gen_text      run: gen_text vcf <rows> <out.vcf>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
static inline uint64_t mix64(uint64_t z) { z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
static inline uint64_t rnd(uint64_t seed, uint64_t col, uint64_t i) { return mix64(seed + col * 0xD1B54A32D192ED03ULL + (i + 1) * 0x9E3779B97F4A7C15ULL); }
static inline uint32_t pct_thr(int p) { return (uint32_t)((((uint64_t)p) << 32) / 100); }
int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: gen_text vcf|bcf|fastq|bam|sam|gff|gtf|bed <rows> <out> [read_len | attrs | n | samples] [ragged]\n"); return 2; }
  const int64_t n = (int64_t)atof(argv[2]);
  FILE* f = fopen(argv[3], "wb");
  if (!f) return 1;
  static char buf[1 << 22];
  setvbuf(f, buf, _IOFBF, sizeof buf);
  if (!strcmp(argv[1], "sam")) {
    // text SAM with the same flag / reference / mapq mix as `gen_text bam`: `gen_text sam <reads> <out> [read_len=100]`
    const int L = argc > 4 ? atoi(argv[4]) : 100;
    const int NREF = 25;
    fputs("@HD\tVN:1.6\tSO:unsorted\n", f);
    for (int r = 0; r < NREF; ++r) fprintf(f, "@SQ\tSN:chr%d\tLN:250000000\n", r + 1);
    static const uint16_t FLAGS[12] = {99, 147, 83, 163, 0, 16, 4, 77, 141, 1024 + 99, 256 + 16, 2048 + 0};
    std::string seq((size_t)L, 'A'), qual((size_t)L, 'I');
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t a = rnd(3, 0, (uint64_t)i), b = rnd(3, 1, (uint64_t)i), c = rnd(3, 2, (uint64_t)i);
      const uint16_t flag = FLAGS[a % 12];
      const bool unmapped = (flag & 4) != 0;
      const uint32_t mq = (uint32_t)(b % 100);
      const int mapq = mq < 2 ? 255 : mq < 10 ? 0 : mq < 22 ? (int)(1 + b % 29) : mq < 42 ? (int)(30 + b % 30) : 60;
      const int len = L - (int)((b >> 32) % (uint64_t)(L / 3 + 1));
      char cigar[64] = "*";
      if (!unmapped) {
        const int kind = (int)((c >> 12) % 4);
        if (kind == 0) snprintf(cigar, sizeof cigar, "%dM", len);
        else if (kind == 1) snprintf(cigar, sizeof cigar, "5S%dM", len - 5);
        else if (kind == 2) snprintf(cigar, sizeof cigar, "%dM%dN%dM", len / 2, (int)(100 + (c >> 20) % 5000), len - len / 2);
        else snprintf(cigar, sizeof cigar, "%dM2D3M", len - 3);
      }
      if (unmapped) fprintf(f, "read%lld\t%u\t*\t0\t%d\t*\t*\t0\t0\t", (long long)i, (unsigned)flag, mapq);
      else fprintf(f, "read%lld\t%u\tchr%d\t%d\t%d\t%s\t*\t0\t0\t", (long long)i, (unsigned)flag, (int)((a >> 8) % NREF) + 1,
                   (int)((a >> 16) % 249000000) + 1, mapq, cigar);
      fwrite(seq.data(), 1, (size_t)len, f);
      fputc('\t', f);
      fwrite(qual.data(), 1, (size_t)len, f);
      fputs(i % 3 ? "\tNM:i:1\n" : "\n", f);
    }
    fclose(f);
    return 0;
  }
  if (!strcmp(argv[1], "gff")) {
    // 24 seqnames in contiguous runs, starts ascending inside a run (step 100 + jitter < 100), 10 types, 3 sources, scores present
    // and '.', all four strand and phase spellings, "###" every 1000 rows, a '#' comment every 7777 rows
    static const char* TYPES[10] = {"gene", "mRNA", "exon", "CDS", "five_prime_UTR", "three_prime_UTR", "ncRNA_gene", "lnc_RNA", "pseudogene", "biological_region"};
    static const char* SOURCES[3] = {"ensembl", "havana", "ensembl_havana"};
    static const char STRAND[4] = {'+', '-', '.', '?'}, PHASE[4] = {'.', '0', '1', '2'};
    const int NSEQ = 24;
    const bool attrs = argc > 4 && !strcmp(argv[4], "attrs");
    // attrs: 0-12 entries a row; '.' and empty fields; a trailing ';' on every other row; keys that repeat inside a row, an escaped
    // key, now and then an empty one; values of 0, 1, 7, 8, 9 bytes, comma lists with empty pieces, %3B / %2c / %25 and a lone '%',
    // and (7 in 16) up to 300 bytes
    static const char* KEYS[8] = {"ID", "Parent", "Name", "gene_id", "Dbxref", "Note", "tag%20x", "Alias"};
    static const char* LISTS[4] = {"a,b", ",x,,y,", "GO:0001,GO:0002,GO:0003", ","};
    static const char* ESCAPES[4] = {"a%3Bb%2cc%25d", "100%", "%zz%3", "x%3Dy%2C%09z"};
    auto attributes = [&](int64_t i, std::string* out) {
      out->clear();
      const uint64_t r = rnd(9, 0, (uint64_t)i);
      const int n_entries = (int)((r >> 4) % 13);
      if ((r & 15) == 0 || n_entries == 0) {
        if (r & 16) *out = ".";
        return;
      }
      for (int j = 0; j < n_entries; ++j) {
        const uint64_t q = rnd(9, 1, (uint64_t)(i * 16 + j));
        if (j) out->push_back(';');
        if ((q >> 40) % 64 != 0) *out += KEYS[(q >> 4) & 7];
        out->push_back('=');
        const int kind = (int)(q & 15);
        const int fixed[5] = {0, 1, 7, 8, 9};
        int len = -1;
        if (kind < 5) len = fixed[kind];
        else if (kind < 7) *out += LISTS[(q >> 8) & 3];
        else if (kind < 9) *out += ESCAPES[(q >> 8) & 3];
        else len = (int)((q >> 8) % 301);
        for (int k = 0; k < len; ++k) out->push_back("abcdefghijklmnopqrstuvwxyz0123456789 _-.:|"[((q >> 20) + (uint64_t)k * 7) % 42]);
      }
      if (r & 32) out->push_back(';');
    };
    std::string field9;
    fputs("##gff-version 3\n", f);
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t a = rnd(8, 0, (uint64_t)i), b = rnd(8, 1, (uint64_t)i);
      const int seq = (int)((i * NSEQ) / n);
      const int64_t first = ((int64_t)seq * n + NSEQ - 1) / NSEQ;  // the first row of this seqname's run
      const int64_t start = 1 + (i - first) * 100 + (int64_t)(a % 100), end = start + (int64_t)((a >> 8) % 5000);
      char name[16], score[16];
      if (seq < 22) snprintf(name, sizeof name, "chr%d", seq + 1);
      else strcpy(name, seq == 22 ? "chrX" : "chrY");
      const uint32_t k = (uint32_t)((a >> 24) % 10000u);
      if ((b & 3) == 0) strcpy(score, ".");
      else snprintf(score, sizeof score, "%u.%u", k / 10, k % 10);
      if (i && i % 1000 == 0) fputs("###\n", f);
      if (i % 7777 == 5) fprintf(f, "# rows from %lld on\n", (long long)i);
      if (attrs) {
        attributes(i, &field9);
        fprintf(f, "%s\t%s\t%s\t%lld\t%lld\t%s\t%c\t%c\t", name, SOURCES[(b >> 2) % 3], TYPES[(b >> 8) % 10], (long long)start, (long long)end, score,
                STRAND[(b >> 16) & 3], PHASE[(b >> 18) & 3]);
        fwrite(field9.data(), 1, field9.size(), f);
        fputc('\n', f);
        continue;
      }
      fprintf(f, "%s\t%s\t%s\t%lld\t%lld\t%s\t%c\t%c\tID=f%lld;Name=n%u\n", name, SOURCES[(b >> 2) % 3], TYPES[(b >> 8) % 10], (long long)start, (long long)end,
              score, STRAND[(b >> 16) & 3], PHASE[(b >> 18) & 3], (long long)i, (unsigned)(b >> 40) & 0xFFFFu);
    }
    fclose(f);
    return 0;
  }
  if (!strcmp(argv[1], "gtf")) {
    // the GFF mode's rows as GTF: 24 seqnames in contiguous runs, starts ascending inside a run, Ensembl's sources and feature types,
    // scores present and '.', strands + - . (never '?'), every frame spelling; "#!" header lines, and a '#' comment every 1000 rows so
    // that most slabs are ranked.  The default ninth field is Ensembl's (gene_id, transcript_id, exon_number, gene_name, ..).
    static const char* TYPES[8] = {"gene", "transcript", "exon", "CDS", "start_codon", "stop_codon", "five_prime_utr", "three_prime_utr"};
    static const char* SOURCES[3] = {"ensembl", "havana", "ensembl_havana"};
    static const char* BIOTYPES[4] = {"protein_coding", "lncRNA", "processed_pseudogene", "miRNA"};
    static const char STRAND[4] = {'+', '-', '.', '+'}, FRAME[4] = {'.', '0', '1', '2'};
    const int NSEQ = 24;
    const bool attrs = argc > 4 && !strcmp(argv[4], "attrs");
    // attrs: 0-12 entries a row; empty fields; the last entry with or without its ';' and spaces behind it; quoted values with ';'
    // and spaces inside, empty ones, of 1, 7, 8, 9 and (now and then) up to 300 bytes; bare numeric values, with spaces in front of
    // the ';'; several spaces between key and value and behind a ';'; `tag` repeated inside a row
    static const char* KEYS[8] = {"gene_id", "transcript_id", "gene_name", "gene_biotype", "exon_id", "transcript_support_level", "ccdsid", "note"};
    static const char* QUOTED[4] = {"a;b", "basic; CCDS ;x", "", "Ensembl canonical"};
    auto attributes = [&](int64_t i, std::string* out) {
      out->clear();
      const uint64_t r = rnd(11, 0, (uint64_t)i);
      const int n_entries = (int)((r >> 4) % 13);
      if ((r & 15) == 0) return;
      for (int j = 0; j < n_entries; ++j) {
        const uint64_t q = rnd(11, 1, (uint64_t)(i * 16 + j));
        const int kind = (int)(q & 15);
        if (j) *out += (q >> 50) % 5 == 0 ? ";  " : "; ";
        *out += kind >= 13 ? "tag" : KEYS[(q >> 4) & 7];
        *out += (q >> 44) % 9 == 0 ? "   " : " ";
        if (kind < 3) {  // bare numbers
          *out += std::to_string((q >> 8) % 100000);
          if (kind == 2) *out += " ";
        } else {
          out->push_back('"');
          const int fixed[4] = {1, 7, 8, 9};
          int len = 0;
          if (kind < 7) len = fixed[kind - 3];
          else if (kind < 10) *out += QUOTED[(q >> 8) & 3];
          else if (kind == 10) len = (int)((q >> 8) % 301);
          else len = 4 + (int)((q >> 8) % 12);
          for (int k = 0; k < len; ++k) out->push_back("abcdefghijklmnopqrstuvwxyz0123456789 _-.:;|"[((q >> 20) + (uint64_t)k * 7) % 43]);
          out->push_back('"');
        }
      }
      if (n_entries && (r & 32)) *out += (r & 64) ? "; " : ";";
    };
    std::string field9;
    fputs("#!genome-build GRCh38.p14\n#!genome-version GRCh38\n", f);
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t a = rnd(10, 0, (uint64_t)i), b = rnd(10, 1, (uint64_t)i);
      const int seq = (int)((i * NSEQ) / n);
      const int64_t first = ((int64_t)seq * n + NSEQ - 1) / NSEQ;  // the first row of this seqname's run
      const int64_t start = 1 + (i - first) * 100 + (int64_t)(a % 100), end = start + (int64_t)((a >> 8) % 5000);
      char name[16], score[16];
      if (seq < 22) snprintf(name, sizeof name, "chr%d", seq + 1);
      else strcpy(name, seq == 22 ? "chrX" : "chrY");
      const uint32_t k = (uint32_t)((a >> 24) % 10000u);
      if ((b & 3) != 0) strcpy(score, ".");
      else snprintf(score, sizeof score, "%u.%u", k / 10, k % 10);
      if (i % 1000 == 500) fprintf(f, "# rows from %lld on\n", (long long)i);
      fprintf(f, "%s\t%s\t%s\t%lld\t%lld\t%s\t%c\t%c\t", name, SOURCES[(b >> 2) % 3], TYPES[(b >> 8) % 8], (long long)start, (long long)end, score,
              STRAND[(b >> 16) & 3], FRAME[(b >> 18) & 3]);
      if (attrs) {
        attributes(i, &field9);
        fwrite(field9.data(), 1, field9.size(), f);
        fputc('\n', f);
        continue;
      }
      fprintf(f, "gene_id \"ENSG%011lld\"; transcript_id \"ENST%011lld\"; exon_number %u; gene_name \"G%u\"; gene_biotype \"%s\"; tag \"basic\"; tag \"CCDS\";\n",
              (long long)(i / 40), (long long)(i / 8), (unsigned)(i % 8) + 1, (unsigned)(b >> 40) & 0xFFFFu, BIOTYPES[(b >> 20) & 3]);
    }
    fclose(f);
    return 0;
  }
  if (!strcmp(argv[1], "bed")) {
    // the GFF mode's layout: 24 names in contiguous runs, starts ascending inside a run (the first of a run may be 0), names of 0 to
    // 40 bytes ("." now and then), scores 0 .. 1000 and the two ends of u16, a '#' comment first and every 1000 rows so that most
    // slabs are ranked; 12-field lines carry thick / colour / block fields as UCSC writes them (they are never read)
    static const int COUNTS[5] = {3, 4, 5, 6, 12};
    static const char STRAND[3] = {'+', '-', '.'};
    const int NSEQ = 24;
    const bool mix = argc > 4 && !strcmp(argv[4], "mix");
    const int fixed = argc > 4 && !mix ? atoi(argv[4]) : 6;
    if (!mix && fixed != 3 && fixed != 4 && fixed != 5 && fixed != 6 && fixed != 12) { fprintf(stderr, "gen_text bed: n is 3, 4, 5, 6, 12 or mix\n"); return 2; }
    fputs("#chrom\tchromStart\tchromEnd\n", f);
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t a = rnd(11, 0, (uint64_t)i), b = rnd(11, 1, (uint64_t)i);
      const int seq = (int)((i * NSEQ) / n);
      const int64_t first = ((int64_t)seq * n + NSEQ - 1) / NSEQ;  // the first row of this name's run
      const int64_t start = (i - first) * 100 + (int64_t)(a % 100) - (i == first ? (int64_t)(a % 100) : 0), end = start + (int64_t)((a >> 8) % 5000);
      const int nf = mix ? COUNTS[(b >> 50) % 5] : fixed;
      char chrom[16];
      if (seq < 22) snprintf(chrom, sizeof chrom, "chr%d", seq + 1);
      else strcpy(chrom, seq == 22 ? "chrX" : "chrY");
      if (i && i % 1000 == 0) fprintf(f, "# rows from %lld on\n", (long long)i);
      fprintf(f, "%s\t%lld\t%lld", chrom, (long long)start, (long long)end);
      if (nf >= 4) {
        char name[64];
        const int kind = (int)(b & 15);
        if (kind == 0) strcpy(name, ".");
        else if (kind == 1) name[0] = 0;
        else {
          const int len = snprintf(name, sizeof name, "NR_%06u_exon_%u_0_%s_%lld_%c", (unsigned)((b >> 8) % 1000000u), (unsigned)((b >> 28) % 40u), chrom, (long long)start + 1, (b & 16) ? 'f' : 'r');
          if (kind == 2) name[len / 3] = 0;
        }
        fprintf(f, "\t%s", name);
      }
      if (nf >= 5) {
        const unsigned k = (unsigned)((a >> 24) % 1003u);
        fprintf(f, "\t%u", k == 1001 ? 65535u : k == 1002 ? 0u : k);
      }
      if (nf >= 6) fprintf(f, "\t%c", STRAND[(b >> 20) % 3]);
      if (nf == 12) fprintf(f, "\t%lld\t%lld\t%u,%u,%u\t2\t%u,%u\t0,%u", (long long)start, (long long)end, (unsigned)(b >> 30) & 255u, (unsigned)(b >> 38) & 255u, (unsigned)(b >> 46) & 255u,
                            (unsigned)(a >> 40) % 500u + 1, (unsigned)(a >> 50) % 500u + 1, (unsigned)(a >> 44) % 4000u + 600u);
      fputc('\n', f);
    }
    fclose(f);
    return 0;
  }
  if (!strcmp(argv[1], "bcf")) {
    // uncompressed BCF2 stream with the SAME rows as `gen_text vcf` (bgzip it to get a .bcf): `gen_text bcf <rows> <out>`
    std::string text = "##fileformat=VCFv4.3\n##FILTER=<ID=PASS,Description=\"All filters passed\",IDX=0>\n##contig=<ID=1,IDX=0>\n"
                       "##FILTER=<ID=q10,Description=\"q\",IDX=1>\n##FILTER=<ID=s50,Description=\"s\",IDX=2>\n"
                       "##INFO=<ID=AF,Number=1,Type=Float,Description=\"AF\",IDX=3>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
    text.push_back('\0');
    fwrite("BCF\2\2", 1, 5, f);
    const uint32_t lt = (uint32_t)text.size();
    fwrite(&lt, 4, 1, f);
    fwrite(text.data(), 1, text.size(), f);
    const uint32_t t0 = pct_thr(85), t1 = pct_thr(90), t2 = pct_thr(96), t3 = pct_thr(99);
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t r0 = rnd(4, 0, i), r1 = rnd(4, 1, i), r2 = rnd(4, 2, i);
      const uint32_t e = (uint32_t)((((r0 >> 23) & 0xFF) * 14) >> 8);
      uint32_t bits = ((126u - e) << 23) | (uint32_t)(r0 & 0x7FFFFF);
      float a; memcpy(&a, &bits, 4);
      if (((r0 >> 31) & 0x3FF) == 0) a = 0.01f;
      const bool av = (r0 >> 44) >= 10486, qv = (r1 >> 44) >= 31457;
      const uint32_t kq = (uint32_t)(r1 & 0xFFFFFFFFu) % 10000u;
      const uint32_t u = (uint32_t)(r2 >> 32);
      const int fid = (u >= t0) + (u >= t1) + (u >= t2) + (u >= t3);
      // the text twin prints AF with 9 significant digits and QUAL as k/10: parse them back the same way
      char tmp[32];
      snprintf(tmp, sizeof tmp, "%.9g", (double)a);
      const float af = strtof(tmp, nullptr);
      snprintf(tmp, sizeof tmp, "%u.%u", kq / 10, kq % 10);
      const float q = strtof(tmp, nullptr);
      uint8_t rec[96];
      size_t o = 8;
      auto p32 = [&](uint32_t v) { memcpy(rec + o, &v, 4); o += 4; };
      p32(0);                      // CHROM
      p32((uint32_t)i);            // POS (0-based) = i  ->  1-based i + 1 as in the text twin
      p32(1);                      // rlen
      uint32_t qb = 0x7F800001u;
      if (qv) memcpy(&qb, &q, 4);
      p32(qb);
      p32((uint32_t)(av ? 1 : 0) | (2u << 16));  // n_info | n_allele << 16
      p32(0);                      // n_fmt << 24 | n_sample
      rec[o++] = 0x07;             // ID: missing
      rec[o++] = 0x17; rec[o++] = 'A';
      rec[o++] = 0x17; rec[o++] = 'C';
      switch (fid) {               // PASS, ".", q10, q10;s50, s50
        case 0: rec[o++] = 0x11; rec[o++] = 0; break;
        case 1: rec[o++] = 0x00; break;
        case 2: rec[o++] = 0x11; rec[o++] = 1; break;
        case 3: rec[o++] = 0x21; rec[o++] = 1; rec[o++] = 2; break;
        default: rec[o++] = 0x11; rec[o++] = 2; break;
      }
      if (av) {
        rec[o++] = 0x11; rec[o++] = 3;  // key AF
        rec[o++] = 0x15;                // one float
        memcpy(rec + o, &af, 4); o += 4;
      }
      const uint32_t ls = (uint32_t)(o - 8), li = 0;
      memcpy(rec, &ls, 4);
      memcpy(rec + 4, &li, 4);
      fwrite(rec, 1, o, f);
    }
    fclose(f);
    return 0;
  }
  if (!strcmp(argv[1], "bam")) {
    // uncompressed BAM stream (header + records; tools/bin/bgzip turns it into a .bam): `gen_text bam <reads> <out> [read_len=100]`
    const int L = argc > 4 ? atoi(argv[4]) : 100;
    auto w32 = [&](int32_t v) { fwrite(&v, 4, 1, f); };
    const int NREF = 25;
    std::string text = "@HD\tVN:1.6\tSO:unsorted\n";
    for (int r = 0; r < NREF; ++r) text += "@SQ\tSN:chr" + std::to_string(r + 1) + "\tLN:250000000\n";
    fwrite("BAM\1", 1, 4, f);
    w32((int32_t)text.size());
    fwrite(text.data(), 1, text.size(), f);
    w32(NREF);
    for (int r = 0; r < NREF; ++r) {
      const std::string nm = "chr" + std::to_string(r + 1);
      w32((int32_t)nm.size() + 1);
      fwrite(nm.c_str(), 1, nm.size() + 1, f);
      w32(250000000);
    }
    static const uint16_t FLAGS[12] = {99, 147, 83, 163, 0, 16, 4, 77, 141, 1024 + 99, 256 + 16, 2048 + 0};
    std::string rec;
    for (int64_t i = 0; i < n; ++i) {
      const uint64_t a = rnd(3, 0, (uint64_t)i), b = rnd(3, 1, (uint64_t)i), c = rnd(3, 2, (uint64_t)i);
      const uint16_t flag = FLAGS[a % 12];
      const bool unmapped = (flag & 4) != 0;
      const int32_t ref = unmapped ? -1 : (int32_t)((a >> 8) % NREF);
      const int32_t pos = unmapped ? -1 : (int32_t)((a >> 16) % 249000000);
      const uint32_t mq = (uint32_t)(b % 100);
      const uint8_t mapq = mq < 2 ? 255 : mq < 10 ? 0 : mq < 22 ? (uint8_t)(1 + b % 29) : mq < 42 ? (uint8_t)(30 + b % 30) : 60;
      const int len = L - (int)((b >> 32) % (uint64_t)(L / 3 + 1));
      char name[40];
      const int ln = snprintf(name, sizeof name, "read%lld:%u", (long long)i, (unsigned)(c & 0xFFF)) + 1;
      uint32_t cig[3];
      int ncig = 0;
      if (!unmapped) {
        const int kind = (int)((c >> 12) % 4);
        if (kind == 0) cig[ncig++] = (uint32_t)len << 4 | 0;                                    // lenM
        else if (kind == 1) { cig[ncig++] = 5u << 4 | 4; cig[ncig++] = (uint32_t)(len - 5) << 4 | 0; }  // 5S..M
        else if (kind == 2) { cig[ncig++] = (uint32_t)(len / 2) << 4 | 0; cig[ncig++] = (uint32_t)(100 + (c >> 20) % 5000) << 4 | 3; cig[ncig++] = (uint32_t)(len - len / 2) << 4 | 0; }  // M N M
        else { cig[ncig++] = (uint32_t)(len - 3) << 4 | 0; cig[ncig++] = 2u << 4 | 2; cig[ncig++] = 3u << 4 | 0; }  // M 2D M
      }
      const int aux = (int)((c >> 40) % 3) * 7;  // 0, 7 or 14 bytes of aux (NM:i / AS:i as 'C' + padding tags)
      const int32_t bs = 32 + ln + 4 * ncig + (len + 1) / 2 + len + aux;
      rec.assign((size_t)bs + 4, '\0');
      auto p32 = [&](size_t o, int32_t v) { memcpy(&rec[o], &v, 4); };
      p32(0, bs); p32(4, ref); p32(8, pos);
      rec[12] = (char)ln; rec[13] = (char)mapq;
      const uint16_t bin = 4680, nc = (uint16_t)ncig;
      memcpy(&rec[14], &bin, 2); memcpy(&rec[16], &nc, 2); memcpy(&rec[18], &flag, 2);
      p32(20, len); p32(24, -1); p32(28, -1); p32(32, 0);
      memcpy(&rec[36], name, (size_t)ln);
      size_t o = 36 + (size_t)ln;
      memcpy(&rec[o], cig, 4u * (size_t)ncig); o += 4u * (size_t)ncig;
      // bases: 4-bit codes of A/C/G/T; qualities: binned Illumina-like values in runs (what real BAMs look like to DEFLATE)
      static const uint8_t NIB[4] = {1, 2, 4, 8}, QBIN[4] = {37, 37, 25, 11};
      for (int k = 0; k < (len + 1) / 2; ++k) {
        const uint64_t x = rnd(3, 3, (uint64_t)(i * 128 + k));
        rec[o + (size_t)k] = (char)(NIB[x & 3] << 4 | NIB[(x >> 2) & 3]);
      }
      o += (size_t)(len + 1) / 2;
      for (int k = 0; k < len;) {
        const uint64_t x = rnd(3, 4, (uint64_t)(i * 256 + k));
        const int run = 1 + (int)((x >> 8) % 12);
        for (int j = 0; j < run && k < len; ++j, ++k) rec[o + (size_t)k] = (char)QBIN[x & 3];
      }
      o += (size_t)len;
      for (int k = 0; k < aux; k += 7) memcpy(&rec[o + (size_t)k], "NMC\5ASC", 7);
      fwrite(rec.data(), 1, rec.size(), f);
    }
    fclose(f);
    return 0;
  }
  if (!strcmp(argv[1], "fastq")) {
    const int L = argc > 4 ? atoi(argv[4]) : 150;
    const bool ragged = argc > 5 && atoi(argv[5]) != 0;
    std::string seq((size_t)L, 'A'), qual((size_t)L, '!');
    for (int64_t i = 0; i < n; ++i) {
      int len = L;
      if (ragged) len = L - (int)(rnd(5, 2, (uint64_t)i) % (uint64_t)(L / 4 + 1));
      for (int p = 0; p < len; p += 8) {
        uint64_t a = rnd(5, 0, (uint64_t)(i * ((L + 7) / 8) + p / 8)), b = rnd(5, 1, (uint64_t)(i * ((L + 7) / 8) + p / 8));
        for (int k = 0; k < 8 && p + k < len; ++k) {
          seq[(size_t)(p + k)] = "ACGT"[a & 3];
          qual[(size_t)(p + k)] = (char)(33 + (b & 0xFF) % 42);
          a >>= 8;
          b >>= 8;
        }
      }
      fprintf(f, "@read%lld sample=%d\n", (long long)i, (int)(i % 7));
      fwrite(seq.data(), 1, (size_t)len, f);
      fputs("\n+\n", f);
      fwrite(qual.data(), 1, (size_t)len, f);
      fputc('\n', f);
    }
    fclose(f);
    return 0;
  }
  const int n_samples = argc > 4 ? atoi(argv[4]) : 0;
  fputs("##fileformat=VCFv4.3\n##contig=<ID=1>\n##INFO=<ID=AF,Number=1,Type=Float,Description=\"AF\">\n"
        "##FILTER=<ID=q10,Description=\"q\">\n##FILTER=<ID=s50,Description=\"s\">\n", f);
  if (n_samples > 0) {
    fputs("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"GT\">\n##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"DP\">\n"
          "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"GQ\">\n##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"PL\">\n", f);
    fputs("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT", f);
    for (int k = 0; k < n_samples; ++k) fprintf(f, "\tS%d", k + 1);
    fputc('\n', f);
  } else {
    fputs("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n", f);
  }
  // sample k of row i: a genotype of two alleles in either phasing, a depth, a quality, three likelihoods (one of them 0)
  auto samples = [&](int64_t i) {
    if (n_samples <= 0) return;
    fputs("\tGT:DP:GQ:PL", f);
    for (int k = 0; k < n_samples; ++k) {
      const uint64_t r = rnd(9, (uint64_t)k, i);
      const unsigned a0 = (unsigned)(r & 1), a1 = (unsigned)((r >> 1) & 1), dp = (unsigned)((r >> 8) % 60) + 1, gq = (unsigned)((r >> 16) % 100);
      const unsigned p1 = (unsigned)((r >> 24) % 255), p2 = (unsigned)((r >> 32) % 255);
      fprintf(f, "\t%u%c%u:%u:%u:%u,%u,%u", a0, ((r >> 2) & 1) ? '|' : '/', a1, dp, gq, a0 + a1 == 0 ? 0u : p1 + 1, a0 + a1 == 1 ? 0u : p1 + 2, a0 + a1 == 2 ? 0u : p2 + 3);
    }
  };
  const char* FILT[5] = {"PASS", ".", "q10", "q10;s50", "s50"};
  const uint32_t t0 = pct_thr(85), t1 = pct_thr(90), t2 = pct_thr(96), t3 = pct_thr(99);
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t r0 = rnd(4, 0, i), r1 = rnd(4, 1, i), r2 = rnd(4, 2, i);
    const uint32_t e = (uint32_t)((((r0 >> 23) & 0xFF) * 14) >> 8);
    uint32_t bits = ((126u - e) << 23) | (uint32_t)(r0 & 0x7FFFFF);
    float a; memcpy(&a, &bits, 4);
    if (((r0 >> 31) & 0x3FF) == 0) a = 0.01f;
    const bool av = (r0 >> 44) >= 10486, qv = (r1 >> 44) >= 31457;
    const uint32_t kq = (uint32_t)(r1 & 0xFFFFFFFFu) % 10000u;
    const uint32_t u = (uint32_t)(r2 >> 32);
    const int fid = (u >= t0) + (u >= t1) + (u >= t2) + (u >= t3);
    char q[16];
    if (qv) snprintf(q, sizeof q, "%u.%u", kq / 10, kq % 10); else strcpy(q, ".");
    if (av) fprintf(f, "1\t%lld\t.\tA\tC\t%s\t%s\tAF=%.9g", (long long)(i + 1), q, FILT[fid], (double)a);
    else fprintf(f, "1\t%lld\t.\tA\tC\t%s\t%s\t.", (long long)(i + 1), q, FILT[fid]);
    samples(i);
    fputc('\n', f);
  }
  fclose(f);
  return 0;
}
