// cli.cpp -- exon-hip-cli: the build's own small command line.
//
// Mirrors the part of exon-cli that the hot path needs (exon/exon-cli/src/main.rs:31-146: `-c <sql>...`,
// `-f <file>...`, `-q`, print a table): a session with external tables, the *_scan table functions and the
// four fused query shapes.  Plain `SELECT COUNT(*)` without a predicate is CPU plumbing (decode + count, no
// GPU, like config 1); predicates / GROUP BY run through exon_hip_plan_* / exon_hip_stream_* on the GPU.
//
//   SET exon.vcf_parse_info = true;
//   CREATE EXTERNAL TABLE t STORED AS FASTA|FASTQ|VCF|BAM|GFF|GTF|BED|INDEXED_VCF|INDEXED_BAM|INDEXED_GFF [OPTIONS (compression gzip, n_fields 6)] LOCATION '<path|dir>';
//   SELECT COUNT(*) FROM t | fasta_scan('<p>'[, 'gzip']) | fastq_scan(..) | vcf_scan(..) | bam_scan(..)
//                         | vcf_indexed_scan('<p>', '<region>') | bam_indexed_scan('<p>', '<region>') | gff_scan(..) | gtf_scan(..) | bed_scan(..) | gff_indexed_scan(..)
//   SELECT COUNT(*) FROM v WHERE chrom = '7' AND pos >= 50000000 AND pos <= 100000000            -- K2
//   SELECT COUNT(*) FROM v WHERE vcf_region_filter('7:50000000-100000000', chrom[, pos]) [= true] -- pushed down
//   SELECT COUNT(*) FROM b WHERE bam_region_filter('chr1:1-100', reference, start, end) [= true]  -- pushed down
//   SELECT COUNT(*) FROM g WHERE gff_region_filter('chr1[:a-b]', seqname[, start]) [= true]       -- K2 over (seqname, start); GFF and GTF sources
//   SELECT COUNT(*) FROM b WHERE gff_region_filter('chr1[:a-b]', reference_sequence_name[, start]) [= true] -- the same over a BED source: K2 over (0, 1)
//   SELECT COUNT(*) FROM b WHERE [bam_region_filter(..) AND] flag & 1284 = 0 [AND CAST(mapping_quality AS INT) >= 30]  -- pushed into the BAM / SAM scan (exon_hip_scan_set_flag_predicate)
//   SELECT reference, COUNT(*) FROM b WHERE flag & 1284 = 0 AND CAST(mapping_quality AS INT) >= 30 GROUP BY reference  -- K3
//   SELECT filter, AVG(qual), COUNT(*) FROM v WHERE info."AF" > 0.01 GROUP BY filter            -- K4
//   SELECT filter, MIN(qual), MAX(qual), COUNT(*) FROM v WHERE info."AF" > 0.01 GROUP BY filter -- K8 (also MIN / MAX(info."DP"))
//   SELECT * FROM fastq_quality_histogram('<p>'[, 'gzip'])                                        -- K5
//   SELECT * FROM fastq_read_stats('<p>'[, 'gzip'])                                               -- K9
//   SELECT * FROM fasta_seq_stats('<p>'[, 'gzip'])                                                -- K10
//   SELECT COUNT(*) FROM <bam table> WHERE bam_region_filter('<r>', reference, start, end)          -- K6 (plain table; INDEXED_BAM plans chunks on the host)
//   SELECT * FROM overlap_counts('<bam|sam|cram|gff|gtf file>', '<regions.bed>'[, 'gzip'])       -- K11: one row per BED line, in file order
//   SELECT * FROM covered_bases('<bam|sam|cram|gff|gtf file>', '<regions.bed>'[, 'gzip'])        -- K12: the rows' bases inside each BED line
//   SELECT * FROM depth_thresholds('<bam|sam|cram|gff|gtf file>', '<regions.bed>', '<T1,T2,...>'[, 'gzip'])  -- K14: per BED line its bases and how many are covered >= T times
//   SELECT * FROM window_depth('<bam|sam|cram file>', <W>[, '<genome file>'])                     -- K13: the rows' bases per window of width W along every contig
//   DROP TABLE t;
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/exon_hip.h"

namespace {

struct Err : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// ---- tokens -------------------------------------------------------------------------------------------
struct Tok {
  enum Kind { Ident, QIdent, Str, Num, Sym, End } kind;
  std::string text;
};

std::vector<Tok> tokenize(const std::string& s) {
  std::vector<Tok> out;
  size_t i = 0;
  while (i < s.size()) {
    const char c = s[i];
    if (isspace((unsigned char)c)) { ++i; continue; }
    if (c == '-' && i + 1 < s.size() && s[i + 1] == '-') { while (i < s.size() && s[i] != '\n') ++i; continue; }
    if (isalpha((unsigned char)c) || c == '_') {
      size_t j = i;
      while (j < s.size() && (isalnum((unsigned char)s[j]) || s[j] == '_' || s[j] == '.')) ++j;
      out.push_back({Tok::Ident, s.substr(i, j - i)});
      i = j;
    } else if (isdigit((unsigned char)c)) {
      size_t j = i;
      while (j < s.size() && (isalnum((unsigned char)s[j]) || s[j] == '.' || ((s[j] == '-' || s[j] == '+') && (s[j - 1] == 'e' || s[j - 1] == 'E')))) ++j;
      out.push_back({Tok::Num, s.substr(i, j - i)});
      i = j;
    } else if (c == '\'' || c == '"') {
      std::string v;
      size_t j = i + 1;
      for (;; ++j) {
        if (j >= s.size()) throw Err("unterminated string literal");
        if (s[j] == c) {
          if (j + 1 < s.size() && s[j + 1] == c) { v += c; ++j; continue; }
          break;
        }
        v += s[j];
      }
      out.push_back({c == '\'' ? Tok::Str : Tok::QIdent, v});
      i = j + 1;
    } else {
      std::string sym(1, c);
      if ((c == '<' || c == '>' || c == '!') && i + 1 < s.size() && (s[i + 1] == '=' || (c == '<' && s[i + 1] == '>'))) sym += s[i + 1];
      out.push_back({Tok::Sym, sym});
      i += sym.size();
    }
  }
  out.push_back({Tok::End, ""});
  return out;
}

std::string lower(std::string s) {
  for (auto& c : s) c = (char)tolower((unsigned char)c);
  return s;
}

struct Parser {
  std::vector<Tok> t;
  size_t p = 0;
  const Tok& peek(size_t k = 0) const { return t[std::min(p + k, t.size() - 1)]; }
  bool is_kw(const char* kw, size_t k = 0) const { return peek(k).kind == Tok::Ident && lower(peek(k).text) == kw; }
  bool is_sym(const char* s, size_t k = 0) const { return peek(k).kind == Tok::Sym && peek(k).text == s; }
  bool accept_kw(const char* kw) { if (is_kw(kw)) { ++p; return true; } return false; }
  bool accept_sym(const char* s) { if (is_sym(s)) { ++p; return true; } return false; }
  void expect_kw(const char* kw) { if (!accept_kw(kw)) throw Err(std::string("expected ") + kw + " near '" + peek().text + "'"); }
  void expect_sym(const char* s) { if (!accept_sym(s)) throw Err(std::string("expected '") + s + "' near '" + peek().text + "'"); }
  std::string ident() {
    if (peek().kind != Tok::Ident && peek().kind != Tok::QIdent) throw Err("expected identifier near '" + peek().text + "'");
    return t[p++].text;
  }
  std::string str() {
    if (peek().kind != Tok::Str) throw Err("expected string literal near '" + peek().text + "'");
    return t[p++].text;
  }
  std::string number() {
    std::string sign;
    if (accept_sym("-")) sign = "-";
    if (peek().kind != Tok::Num) throw Err("expected number near '" + peek().text + "'");
    return sign + t[p++].text;
  }
  bool at_end() const { return peek().kind == Tok::End; }
};

// ---- session --------------------------------------------------------------------------------------------
struct Table {
  int format = 0;
  bool indexed = false;
  int compression = EXON_HIP_COMPRESSION_AUTO;
  int n_fields = 12;  // BED: the schema's leading columns (exon-core/src/datasources/bed/table_options.rs:34-45)
  std::string location, extension;
};

struct Source {  // resolved FROM clause
  int format = 0;
  int compression = EXON_HIP_COMPRESSION_AUTO;
  std::vector<std::string> files;
  std::string region;  // from *_indexed_scan
  bool indexed = false;
  int n_fields = 12;  // BED
  std::string regions_bed;  // overlap_counts / covered_bases: the BED file of the region set
  bool bases = false;       // covered_bases: K12's sums instead of K11's counts
  bool depth = false;       // depth_thresholds: K14's bases and threshold counts
  std::vector<int64_t> thresholds;  // depth_thresholds: strictly increasing, each >= 1, at most 8
  int64_t window = 0;       // window_depth: the window width (0: another source)
  std::string genome_file;  // window_depth: contigs and lengths from a bedtools genome file / .fai instead of the file's header
  uint32_t cover_ops = 0;   // covered_bases / depth_thresholds / window_depth: 'cover=aligned' / 'cover=aligned+del' (exon_hip_scan_set_cover_ops); 0: the span
};

struct Session {
  std::map<std::string, Table> tables;
  bool vcf_parse_info = false;
  bool quiet = false;
  exon_hip_ctx* ctx = nullptr;
  ~Session() { if (ctx) exon_hip_ctx_destroy(ctx); }
  exon_hip_ctx* gpu() {
    if (!ctx && exon_hip_ctx_create(0, &ctx) != 0) throw Err(std::string("GPU required for this query: ") + exon_hip_last_error(nullptr));
    return ctx;
  }
};

void ck(exon_hip_ctx* ctx, int rc) {
  if (rc < 0) {
    std::string m = ctx ? exon_hip_last_error(ctx) : "";
    if (m.empty()) m = exon_hip_last_error(nullptr);
    throw Err(m);
  }
}

bool ends_with(const std::string& s, const std::string& suf) { return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0; }

// object_store_files_from_table_path (exon-common/src/object_store_files_from_table_path.rs:21-47): a file, or every
// file under a directory whose name carries the format's extension (optionally + compression suffix)
void list_files(const std::string& path, const std::vector<std::string>& exts, std::vector<std::string>* out) {
  struct stat st;
  if (stat(path.c_str(), &st) != 0) throw Err("no such file or directory: " + path);
  if (!S_ISDIR(st.st_mode)) { out->push_back(path); return; }
  DIR* d = opendir(path.c_str());
  if (!d) throw Err("cannot list " + path);
  std::vector<std::string> names;
  while (dirent* e = readdir(d)) if (e->d_name[0] != '.') names.push_back(e->d_name);
  closedir(d);
  std::sort(names.begin(), names.end());
  for (const auto& n : names) {
    const std::string full = path + (ends_with(path, "/") ? "" : "/") + n;
    if (stat(full.c_str(), &st) != 0) continue;
    if (S_ISDIR(st.st_mode)) { list_files(full, exts, out); continue; }
    for (const auto& e : exts)
      if (ends_with(n, e) || ends_with(n, e + ".gz") || ends_with(n, e + ".bgz")) { out->push_back(full); break; }
  }
}

std::vector<std::string> format_exts(int format, const std::string& custom) {
  if (!custom.empty()) return {"." + custom};
  switch (format) {
    case EXON_HIP_FORMAT_FASTA: return {".fasta", ".fa", ".fna", ".faa"};
    case EXON_HIP_FORMAT_FASTQ: return {".fastq", ".fq"};
    case EXON_HIP_FORMAT_VCF: return {".vcf"};
    case EXON_HIP_FORMAT_SAM: return {".sam"};
    case EXON_HIP_FORMAT_BCF: return {".bcf"};
    case EXON_HIP_FORMAT_CRAM: return {".cram"};
    case EXON_HIP_FORMAT_GFF: return {".gff", ".gff3"};
    case EXON_HIP_FORMAT_GTF: return {".gtf"};
    case EXON_HIP_FORMAT_BED: return {".bed"};
    default: return {".bam"};
  }
}

int format_of(const std::string& name, bool* indexed) {
  std::string f = lower(name);
  *indexed = false;
  if (f.rfind("indexed_", 0) == 0) { *indexed = true; f = f.substr(8); }
  if (f == "fasta") return EXON_HIP_FORMAT_FASTA;
  if (f == "fastq") return EXON_HIP_FORMAT_FASTQ;
  if (f == "vcf") return EXON_HIP_FORMAT_VCF;
  if (f == "bam") return EXON_HIP_FORMAT_BAM;
  if (f == "sam") return EXON_HIP_FORMAT_SAM;
  if (f == "bcf") return EXON_HIP_FORMAT_BCF;
  if (f == "cram") return EXON_HIP_FORMAT_CRAM;
  if (f == "gff") return EXON_HIP_FORMAT_GFF;
  if (f == "gtf") {
    if (*indexed) throw Err("unsupported file type " + name + " (there is no indexed GTF table)");
    return EXON_HIP_FORMAT_GTF;
  }
  if (f == "bed") {
    if (*indexed) throw Err("unsupported file type " + name + " (there is no indexed BED table)");
    return EXON_HIP_FORMAT_BED;
  }
  throw Err("unsupported file type " + name);
}

int compression_of(const std::string& v) {
  const std::string c = lower(v);
  if (c == "gzip" || c == "gz" || c == "bgzip") return EXON_HIP_COMPRESSION_GZIP;
  if (c == "none" || c == "uncompressed" || c.empty()) return EXON_HIP_COMPRESSION_NONE;
  throw Err("unsupported compression " + v);
}

// ---- output ---------------------------------------------------------------------------------------------
void print_table(const std::vector<std::string>& cols, const std::vector<std::vector<std::string>>& rows, bool quiet) {
  std::vector<size_t> w(cols.size());
  for (size_t i = 0; i < cols.size(); ++i) w[i] = cols[i].size();
  for (const auto& r : rows) for (size_t i = 0; i < cols.size(); ++i) w[i] = std::max(w[i], r[i].size());
  auto line = [&]() { for (size_t i = 0; i < cols.size(); ++i) printf("+%s", std::string(w[i] + 2, '-').c_str()); printf("+\n"); };
  line();
  for (size_t i = 0; i < cols.size(); ++i) printf("| %-*s ", (int)w[i], cols[i].c_str());
  printf("|\n");
  line();
  for (const auto& r : rows) {
    for (size_t i = 0; i < cols.size(); ++i) printf("| %-*s ", (int)w[i], r[i].c_str());
    printf("|\n");
  }
  line();
  if (!quiet) printf("%zu row(s) fetched.\n", rows.size());
}

std::string fmt_f64(double v) {
  char b[64];
  snprintf(b, sizeof b, "%.17g", v);
  // shortest representation that round-trips, like Rust's Display for f64
  for (int p = 1; p < 17; ++p) {
    char t[64];
    snprintf(t, sizeof t, "%.*g", p, v);
    if (strtod(t, nullptr) == v) { snprintf(b, sizeof b, "%s", t); break; }
  }
  std::string s = b;
  if (s.find_first_of(".eEn") == std::string::npos) s += ".0";
  return s;
}

// ---- execution --------------------------------------------------------------------------------------------
struct ScanGuard {
  exon_hip_scan* s = nullptr;
  ~ScanGuard() { if (s) exon_hip_scan_close(s); }
};
struct StreamGuard {
  exon_hip_plan* p = nullptr;
  exon_hip_stream* s = nullptr;
  ~StreamGuard() { if (s) exon_hip_stream_close(s); if (p) exon_hip_plan_destroy(p); }
};

// VCF / FASTQ queries that end in a fused GPU kernel ship the text to HBM and parse it there (EXON_HIP_GPU_PARSE=0: host decode)
bool gpu_parse_enabled() {
  const char* v = getenv("EXON_HIP_GPU_PARSE");
  return !(v && v[0] == '0');
}

void open_scan(const Source& src, const std::string& file, const char* info_field, const std::string& region, ScanGuard* g,
               bool for_gpu_query = false, uint64_t projection = 0) {
  exon_hip_scan_options o;
  memset(&o, 0, sizeof o);
  o.format = src.format;
  o.compression = src.compression;
  o.info_field = info_field;
  o.region = region.empty() ? nullptr : region.c_str();
  o.projection = projection;
  // INDEXED_* tables / *_indexed_scan: plan BGZF chunks from <file>.tbi / <file>.bai
  // (exon-core/src/datasources/indexed_file/indexed_bgzf_file.rs:129-155)
  o.use_index = (src.indexed && !region.empty()) ? 1 : 0;
  o.gpu_parse = (for_gpu_query && (src.format == EXON_HIP_FORMAT_VCF || src.format == EXON_HIP_FORMAT_FASTQ || src.format == EXON_HIP_FORMAT_BAM || src.format == EXON_HIP_FORMAT_BCF || src.format == EXON_HIP_FORMAT_SAM || src.format == EXON_HIP_FORMAT_GFF || src.format == EXON_HIP_FORMAT_GTF || src.format == EXON_HIP_FORMAT_BED || src.format == EXON_HIP_FORMAT_FASTA) &&
                 region.empty() && gpu_parse_enabled()) ? 1 : 0;
  ck(nullptr, exon_hip_scan_open(file.c_str(), &o, &g->s));
  if (src.cover_ops) ck(nullptr, exon_hip_scan_set_cover_ops(g->s, src.cover_ops));  // (a source without a CIGAR: the scan's own refusal)
}

// CPU plumbing: decode and count rows (optionally with a pushed-down region filter)
struct Predicate;
void push_flags(exon_hip_scan* s, const Predicate* pr);
int64_t count_rows(const Source& src, const std::string& region, const Predicate* flags = nullptr) {
  int64_t total = 0;
  for (const auto& f : src.files) {
    ScanGuard g;
    open_scan(src, f, nullptr, region, &g);
    push_flags(g.s, flags);
    for (;;) {
      struct ArrowArray b;
      const int rc = exon_hip_scan_next(g.s, &b);
      if (rc == 1) break;
      ck(nullptr, rc);
      total += b.length;
      b.release(&b);
    }
  }
  return total;
}

struct Predicate {  // what the WHERE clause turned into
  enum Kind { None, Region, PushedRegion, FlagMapq, InfoCmp } kind = None;
  std::string chrom; int64_t start = 1, end = INT64_MAX;      // Region
  std::string region;                                          // PushedRegion
  int32_t flag_mask = 0, flag_value = 0, mapq_min = INT32_MIN; // FlagMapq
  bool flags = false;  // a flag / mapping_quality conjunct was given (FlagMapq, or ANDed with a pushed bam_region_filter)
  // the scan's own form of it (exon_hip_scan_set_flag_predicate): an unset mapq conjunct is -1; a negative bound still drops NULLs
  int32_t scan_mapq_min() const { return mapq_min == INT32_MIN ? -1 : std::max(mapq_min, 0); }
  std::string info_field; int cmp_op = 0; double literal = 0;  // InfoCmp
};

// the WHERE clause's flag / mapping_quality conjuncts into the scan itself (BAM, SAM; any other source: the scan's own refusal)
void push_flags(exon_hip_scan* s, const Predicate* pr) {
  if (pr && pr->flags) ck(nullptr, exon_hip_scan_set_flag_predicate(s, pr->flag_mask, pr->flag_value, pr->scan_mapq_min()));
}

// The last optional argument of covered_bases / depth_thresholds / window_depth: 'cover=span' (the default: a read's whole span),
// 'cover=aligned' (M = X: samtools depth, bedcov -j) or 'cover=aligned+del' (+ D: samtools depth -J).  false: `arg` is something else.
bool cover_arg(const std::string& fn, const std::string& arg, Source* src) {
  if (arg.rfind("cover=", 0) != 0) return false;
  if (fn == "overlap_counts")
    throw Err("overlap_counts: 'cover=' belongs to covered_bases, depth_thresholds and window_depth, which add per base; overlap_counts counts records, and a record would count once per aligned block");
  const std::string v = arg.substr(6);
  if (v == "span") src->cover_ops = 0;
  else if (v == "aligned") src->cover_ops = EXON_HIP_COVER_ALIGNED;
  else if (v == "aligned+del") src->cover_ops = EXON_HIP_COVER_ALIGNED_DEL;
  else throw Err(fn + ": cover= takes span, aligned or aligned+del, got '" + v + "'");
  return true;
}

int cmp_code(const std::string& s) {
  if (s == ">") return EXON_HIP_GT;
  if (s == ">=") return EXON_HIP_GE;
  if (s == "<") return EXON_HIP_LT;
  if (s == "<=") return EXON_HIP_LE;
  if (s == "=") return EXON_HIP_EQ;
  if (s == "!=" || s == "<>") return EXON_HIP_NE;
  throw Err("unsupported comparison " + s);
}

Predicate parse_where(Parser& ps, int format) {
  Predicate pr;
  // pushed-down marker UDFs (exon-core/src/udfs/vcf/vcf_region_filter.rs:23-75, udfs/sam/bam_region_filter.rs:23-86, udfs/gff/gff_region_filter.rs)
  if (ps.is_kw("vcf_region_filter") || ps.is_kw("bam_region_filter") || ps.is_kw("gff_region_filter")) {
    ps.ident();
    ps.expect_sym("(");
    pr.kind = Predicate::PushedRegion;
    pr.region = ps.str();
    while (ps.accept_sym(",")) ps.ident();
    ps.expect_sym(")");
    if (ps.accept_sym("=")) ps.expect_kw("true");
    if (!ps.is_kw("and")) return pr;  // (else: bam_region_filter(..) AND flag & M = V [AND CAST(mapping_quality AS INT) >= q])
  }
  if (ps.is_kw("region_match")) {  // region_match(chrom, pos, 'r')
    ps.ident(); ps.expect_sym("("); ps.ident(); ps.expect_sym(","); ps.ident(); ps.expect_sym(",");
    char name[512];
    ck(nullptr, exon_hip_parse_region(ps.str().c_str(), name, sizeof name, &pr.start, &pr.end));
    pr.chrom = name;
    pr.kind = Predicate::Region;
    ps.expect_sym(")");
    return pr;
  }
  bool first = pr.kind == Predicate::None;
  while (first || ps.accept_kw("and")) {
    first = false;
    if (ps.is_kw("bam_region_filter")) {  // ... AND bam_region_filter(..): pushed down beside the flag conjuncts
      ps.ident();
      ps.expect_sym("(");
      pr.region = ps.str();
      while (ps.accept_sym(",")) ps.ident();
      ps.expect_sym(")");
      if (ps.accept_sym("=")) ps.expect_kw("true");
      continue;
    }
    if (ps.is_kw("cast")) {  // CAST(mapping_quality AS INT) >= q
      ps.ident(); ps.expect_sym("("); ps.ident(); ps.expect_kw("as"); ps.ident(); ps.expect_sym(")");
      const std::string op = ps.peek().text; ps.p++;
      const int q = atoi(ps.number().c_str());
      if (op == ">=") pr.mapq_min = q; else if (op == ">") pr.mapq_min = q + 1; else throw Err("only >= / > on CAST(mapping_quality AS INT)");
      pr.kind = Predicate::FlagMapq;
      pr.flags = true;
      continue;
    }
    const std::string col = lower(ps.ident());
    if (col == "chrom") { ps.expect_sym("="); pr.chrom = ps.str(); pr.kind = Predicate::Region; }
    else if (col == "pos") {
      pr.kind = Predicate::Region;
      if (ps.accept_kw("between")) { pr.start = atoll(ps.number().c_str()); ps.expect_kw("and"); pr.end = atoll(ps.number().c_str()); }
      else {
        const std::string op = ps.peek().text; ps.p++;
        const int64_t v = atoll(ps.number().c_str());
        if (op == ">=") pr.start = std::max(pr.start, v); else if (op == ">") pr.start = std::max(pr.start, v + 1);
        else if (op == "<=") pr.end = std::min(pr.end, v); else if (op == "<") pr.end = std::min(pr.end, v - 1);
        else if (op == "=") { pr.start = std::max(pr.start, v); pr.end = std::min(pr.end, v); }
        else throw Err("unsupported operator on pos: " + op);
      }
    } else if (col == "flag") {  // flag & M = V
      ps.expect_sym("&"); pr.flag_mask = atoi(ps.number().c_str()); ps.expect_sym("="); pr.flag_value = atoi(ps.number().c_str());
      pr.kind = Predicate::FlagMapq;
      pr.flags = true;
    } else if (col == "info" || col.rfind("info.", 0) == 0) {  // info."AF" <op> lit
      if (col.size() > 5) pr.info_field = col.substr(5);  // unquoted identifiers fold to lower case, as in DataFusion
      else { ps.accept_sym("."); pr.info_field = ps.ident(); }
      pr.cmp_op = cmp_code(ps.peek().text); ps.p++;
      pr.literal = atof(ps.number().c_str());
      pr.kind = Predicate::InfoCmp;
    } else {
      throw Err("unsupported predicate column '" + col + "' for this build (the fused shapes are listed in --help)");
    }
  }
  if (!pr.region.empty()) {  // a pushed region with further conjuncts: only the flag / mapping_quality ones go into the scan with it
    if (pr.kind != Predicate::FlagMapq && pr.kind != Predicate::PushedRegion) throw Err("a region filter is ANDed with flag & M = V and CAST(mapping_quality AS INT) >= q only");
    pr.kind = Predicate::PushedRegion;
  }
  (void)format;
  return pr;
}

Source resolve_from(Session& se, Parser& ps) {
  Source src;
  const std::string name = ps.ident();
  const std::string lname = lower(name);
  if (ps.accept_sym("(")) {  // table function: <fmt>_scan / <fmt>_indexed_scan / fastq_quality_histogram / fastq_read_stats / fasta_seq_stats / overlap_counts / covered_bases / depth_thresholds / window_depth
    const std::string path = ps.str();
    if (lname == "overlap_counts" || lname == "covered_bases" || lname == "depth_thresholds" || lname == "window_depth") {  // the source's format by its extension
      ps.expect_sym(",");
      if (lname == "window_depth") {  // ('<file>', <W>[, '<genome file>'])
        const std::string w = ps.number();
        char* endp = nullptr;
        src.window = strtoll(w.c_str(), &endp, 10);
        if (*endp) throw Err("window_depth: the window width must be a whole number, got " + w);
        if (src.window < 1) throw Err("window_depth: the window width must be at least 1, got " + w);
        if (ps.accept_sym(",")) {
          const std::string a = ps.str();
          if (!cover_arg(lname, a, &src)) {
            src.genome_file = a;
            if (ps.accept_sym(",") && !cover_arg(lname, ps.str(), &src)) throw Err(lname + ": the argument behind the genome file is 'cover=span', 'cover=aligned' or 'cover=aligned+del'");
          }
        }
      } else {  // ('<file>', '<regions.bed>'[, '<compression>'])
        src.regions_bed = ps.str();
        src.bases = lname == "covered_bases";
        src.depth = lname == "depth_thresholds";
        if (src.depth) {  // ('<file>', '<regions.bed>', '<T1,T2,...>'[, '<compression>'])
          ps.expect_sym(",");
          const std::string list = ps.str();
          const Err bad("depth_thresholds: the thresholds are whole numbers >= 1 in strictly increasing order, at most " +
                        std::to_string(EXON_HIP_REGION_DEPTH_MAX_THRESHOLDS) + " of them, separated by commas; got '" + list + "'");
          std::istringstream ts(list);
          for (std::string item; std::getline(ts, item, ',');) {
            char* endp = nullptr;
            errno = 0;
            const long long t = strtoll(item.c_str(), &endp, 10);
            while (*endp == ' ') ++endp;
            if (item.empty() || endp == item.c_str() || *endp || errno || t < 1 || (!src.thresholds.empty() && t <= src.thresholds.back())) throw bad;
            src.thresholds.push_back(t);
          }
          if (src.thresholds.empty() || src.thresholds.size() > EXON_HIP_REGION_DEPTH_MAX_THRESHOLDS || (!list.empty() && list.back() == ',')) throw bad;
        }
        if (ps.accept_sym(",")) {
          const std::string a = ps.str();
          if (!cover_arg(lname, a, &src)) {
            src.compression = compression_of(a);
            if (ps.accept_sym(",") && !cover_arg(lname, ps.str(), &src)) throw Err(lname + ": the argument behind the compression is 'cover=span', 'cover=aligned' or 'cover=aligned+del'");
          }
        }
      }
      ps.expect_sym(")");
      std::string stem = lower(path);
      for (const char* z : {".gz", ".bgz"})
        if (ends_with(stem, z)) stem.resize(stem.size() - strlen(z));
      if (ends_with(stem, ".bam")) src.format = EXON_HIP_FORMAT_BAM;
      else if (ends_with(stem, ".sam")) src.format = EXON_HIP_FORMAT_SAM;
      else if (ends_with(stem, ".cram")) src.format = EXON_HIP_FORMAT_CRAM;
      else if (ends_with(stem, ".gff") || ends_with(stem, ".gff3")) src.format = EXON_HIP_FORMAT_GFF;
      else if (ends_with(stem, ".gtf")) src.format = EXON_HIP_FORMAT_GTF;
      else if (ends_with(stem, ".bed")) throw Err(lname + ": a BED source is not served (its half-open columns need the strict form); sources are BAM, SAM, CRAM, GFF and GTF files");
      else throw Err(lname + ": cannot tell the format of '" + path + "' from its extension (.bam .sam .cram .gff .gff3 .gtf, optionally .gz / .bgz)");
      list_files(path, format_exts(src.format, ""), &src.files);
      return src;
    }
    std::string arg2;
    if (ps.accept_sym(",")) arg2 = ps.str();
    ps.expect_sym(")");
    const size_t us = lname.find('_');
    bool idx = false;
    src.format = format_of(lname.substr(0, us), &idx);
    src.indexed = lname.find("_indexed_scan") != std::string::npos;
    if (src.indexed) src.region = arg2;
    else if (!arg2.empty()) src.compression = compression_of(arg2);
    list_files(path, format_exts(src.format, ""), &src.files);
    return src;
  }
  auto it = se.tables.find(lname);
  if (it == se.tables.end()) throw Err("table '" + name + "' not found");
  src.format = it->second.format;
  src.n_fields = it->second.n_fields;
  src.compression = it->second.compression;
  src.indexed = it->second.indexed;
  list_files(it->second.location, format_exts(src.format, it->second.extension), &src.files);
  return src;
}

// SELECT <columns | *> FROM <GFF or GTF source> [LIMIT n]: rows of the eight leading columns through the host reader (the
// attributes map is not printed); values rendered like datafusion's CLI: NULL for a null, a float in its shortest form
void select_annotation_rows(const Source& src, bool star, const std::vector<std::string>& proj, int64_t limit, bool quiet) {
  const std::vector<std::string> names = {"seqname", "source", "type", "start", "end", "score", "strand", src.format == EXON_HIP_FORMAT_GTF ? "frame" : "phase"};
  std::vector<int> cols;
  if (star) for (int c = 0; c < 8; ++c) cols.push_back(c);
  for (const auto& p : proj) {
    const auto it = std::find(names.begin(), names.end(), p);
    if (it == names.end()) throw Err("column '" + p + "' is not one this build prints (" + names[0] + " .. " + names[7] + ")");
    cols.push_back((int)(it - names.begin()));
  }
  std::vector<std::string> head;
  for (int c : cols) head.push_back(names[(size_t)c]);
  std::vector<std::vector<std::string>> rows;
  auto valid = [](const struct ArrowArray* a, int64_t i) {
    const uint8_t* bm = static_cast<const uint8_t*>(a->buffers[0]);
    return !bm || ((bm[(i + a->offset) >> 3] >> ((i + a->offset) & 7)) & 1);
  };
  for (const auto& f : src.files) {
    ScanGuard g;
    open_scan(src, f, nullptr, "", &g);
    for (;;) {
      if (limit >= 0 && (int64_t)rows.size() >= limit) break;
      struct ArrowArray b;
      const int rc = exon_hip_scan_next(g.s, &b);
      if (rc == 1) break;
      ck(nullptr, rc);
      for (int64_t i = 0; i < b.length && (limit < 0 || (int64_t)rows.size() < limit); ++i) {
        std::vector<std::string> row;
        for (int c : cols) {
          const struct ArrowArray* a = b.children[c];
          if (!valid(a, i)) { row.push_back("NULL"); continue; }
          const int64_t at = i + a->offset;
          if (c == 3 || c == 4) {
            row.push_back(std::to_string(static_cast<const int64_t*>(a->buffers[1])[at]));
          } else if (c == 5) {
            const float v = static_cast<const float*>(a->buffers[1])[at];
            char t[64];
            for (int p = 1; p <= 9; ++p) { snprintf(t, sizeof t, "%.*g", p, (double)v); if (strtof(t, nullptr) == v) break; }
            std::string sv = t;
            if (sv.find_first_of(".eEn") == std::string::npos) sv += ".0";
            row.push_back(sv);
          } else {  // a dictionary: the id's name
            const int32_t id = static_cast<const int32_t*>(a->buffers[1])[at];
            const struct ArrowArray* d = a->dictionary;
            const int32_t* off = static_cast<const int32_t*>(d->buffers[1]) + d->offset;
            row.push_back(std::string(static_cast<const char*>(d->buffers[2]) + off[id], (size_t)(off[id + 1] - off[id])));
          }
        }
        rows.push_back(std::move(row));
      }
      if (b.release) b.release(&b);
    }
  }
  print_table(head, rows, quiet);
}

// SELECT <columns | *> FROM <BED source> [LIMIT n]: rows of the table's n_fields leading columns (schema.rs:27-48) through the host
// reader, NULLs printed as datafusion's CLI prints them
void select_bed_rows(const Source& src, bool star, const std::vector<std::string>& proj, int64_t limit, bool quiet) {
  static const char* const NAMES[12] = {"reference_sequence_name", "start", "end", "name", "score", "strand", "thick_start", "thick_end", "color", "block_count",
                                        "block_sizes", "block_starts"};
  static const bool UTF8[12] = {false, false, false, true, false, false, false, false, true, false, true, true};
  uint64_t mask = 0;
  for (int c = 3; c < src.n_fields; ++c) mask |= 1ull << c;
  std::vector<int> cols;
  if (star) for (int c = 0; c < src.n_fields; ++c) cols.push_back(c);
  for (const auto& p : proj) {
    int at = -1;
    for (int c = 0; c < src.n_fields; ++c) if (p == NAMES[c] || p == std::string("\"") + NAMES[c] + "\"") at = c;
    if (at < 0) throw Err("column '" + p + "' is not one of this BED table's " + std::to_string(src.n_fields) + " (n_fields)");
    cols.push_back(at);
  }
  std::vector<std::string> head;
  for (int c : cols) head.push_back(NAMES[c]);
  std::vector<std::vector<std::string>> rows;
  auto valid = [](const struct ArrowArray* a, int64_t i) {
    const uint8_t* bm = static_cast<const uint8_t*>(a->buffers[0]);
    return !bm || ((bm[(i + a->offset) >> 3] >> ((i + a->offset) & 7)) & 1);
  };
  auto utf8 = [](const struct ArrowArray* a, int64_t at) {
    const int32_t* off = static_cast<const int32_t*>(a->buffers[1]);
    return std::string(static_cast<const char*>(a->buffers[2]) + off[at], (size_t)(off[at + 1] - off[at]));
  };
  for (const auto& f : src.files) {
    ScanGuard g;
    open_scan(src, f, nullptr, "", &g, false, mask);
    for (;;) {
      if (limit >= 0 && (int64_t)rows.size() >= limit) break;
      struct ArrowArray b;
      const int rc = exon_hip_scan_next(g.s, &b);
      if (rc == 1) break;
      ck(nullptr, rc);
      for (int64_t i = 0; i < b.length && (limit < 0 || (int64_t)rows.size() < limit); ++i) {
        std::vector<std::string> row;
        for (int c : cols) {
          const struct ArrowArray* a = b.children[c];  // (the mask is a prefix of the schema: scan column = schema column)
          if (!valid(a, i)) { row.push_back("NULL"); continue; }
          const int64_t at = i + a->offset;
          if (c == 0 || c == 5) row.push_back(utf8(a->dictionary, static_cast<const int32_t*>(a->buffers[1])[at] + a->dictionary->offset));
          else if (UTF8[c]) row.push_back(utf8(a, at));
          else row.push_back(std::to_string(static_cast<const int64_t*>(a->buffers[1])[at]));
        }
        rows.push_back(std::move(row));
      }
      if (b.release) b.release(&b);
    }
  }
  print_table(head, rows, quiet);
}

void exec_select(Session& se, Parser& ps) {
  // projection
  std::vector<std::string> proj;
  bool star = false;
  do {
    if (ps.accept_sym("*")) { star = true; continue; }
    std::string item = lower(ps.ident());
    if (ps.accept_sym("(")) {
      if (ps.accept_sym("*")) item += "(*)";
      else {  // a column, or info."DP" (a quoted key keeps its case; info.dp arrives as one folded identifier)
        std::string arg = lower(ps.ident());
        if (arg == "info.") arg += ps.ident();  // (the tokenizer leaves the dot with the identifier in front of a quoted key)
        item += "(" + arg + ")";
      }
      ps.expect_sym(")");
    }
    if (ps.accept_kw("as")) ps.ident();
    else if (ps.peek().kind == Tok::Ident && !ps.is_kw("from")) ps.ident();  // bare alias
    proj.push_back(item);
  } while (ps.accept_sym(","));
  ps.expect_kw("from");
  const bool hist = ps.is_kw("fastq_quality_histogram"), read_stats = ps.is_kw("fastq_read_stats"), seq_stats = ps.is_kw("fasta_seq_stats");
  Source src = resolve_from(se, ps);
  Predicate pr;
  if (ps.accept_kw("where")) pr = parse_where(ps, src.format);
  std::string group_by;
  if (ps.accept_kw("group")) { ps.expect_kw("by"); group_by = lower(ps.ident()); while (ps.accept_sym(",")) ps.ident(); }
  if (ps.accept_kw("order")) { ps.expect_kw("by"); while (!ps.at_end() && !ps.is_sym(";") && !ps.is_kw("limit")) ps.p++; }
  int64_t limit = -1;
  if (ps.accept_kw("limit")) limit = atoll(ps.number().c_str());
  if (!ps.at_end()) throw Err("unexpected '" + ps.peek().text + "'");

  if (src.indexed && src.region.empty() && pr.kind != Predicate::PushedRegion)
    throw Err("an INDEXED table requires a region filter");  // slt/vcf-indexed-tests.slt:6-8, :48-49
  if (!src.region.empty()) { pr.kind = Predicate::PushedRegion; pr.region = src.region; }

  if (hist) {  // K5
    exon_hip_ctx* ctx = se.gpu();
    const int lmax = 512;
    std::vector<int64_t> total((size_t)lmax * 256, 0);
    for (const auto& f : src.files) {
      ScanGuard g; open_scan(src, f, nullptr, "", &g, true);
      StreamGuard sg;
      exon_hip_plan_desc d; memset(&d, 0, sizeof d);
      d.kind = EXON_HIP_PLAN_QUAL_POS_HIST; d.lmax = lmax; d.columns[0] = 3;
      ck(ctx, exon_hip_plan_create(ctx, &d, &sg.p));
      ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
      std::vector<int64_t> h((size_t)lmax * 256);
      ck(ctx, exon_hip_stream_finish(sg.s, h.data(), nullptr));
      for (size_t i = 0; i < h.size(); ++i) total[i] += h[i];
    }
    std::vector<std::vector<std::string>> rows;
    for (int p = 0; p < lmax; ++p)
      for (int b = 0; b < 256; ++b)
        if (total[(size_t)p * 256 + b]) rows.push_back({std::to_string(p + 1), std::to_string(b - 33), std::to_string(total[(size_t)p * 256 + b])});
    print_table({"position", "quality_score", "count(*)"}, rows, se.quiet);
    return;
  }

  if (read_stats) {  // K9: the per-read tables; every word of the state adds, so the files' states do
    exon_hip_ctx* ctx = se.gpu();
    const int lmax = 65536;
    int64_t at[5];
    ck(nullptr, exon_hip_read_stats_layout(lmax, at));
    std::vector<int64_t> total((size_t)at[4], 0);
    for (const auto& f : src.files) {
      ScanGuard g; open_scan(src, f, nullptr, "", &g, true);
      StreamGuard sg;
      exon_hip_plan_desc d; memset(&d, 0, sizeof d);
      d.kind = EXON_HIP_PLAN_READ_STATS_HIST; d.lmax = lmax; d.columns[0] = 2; d.columns[1] = 3;
      ck(ctx, exon_hip_plan_create(ctx, &d, &sg.p));
      ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
      std::vector<int64_t> h((size_t)at[4]);
      ck(ctx, exon_hip_stream_finish(sg.s, h.data(), nullptr));
      for (size_t i = 0; i < h.size(); ++i) total[i] += h[i];
    }
    static const char* const stat_names[4] = {"total", "length", "gc_percent", "mean_quality"};
    static const char* const total_names[4] = {"reads", "bases", "gc", "quality_sum"};
    std::vector<std::vector<std::string>> rows;
    for (int st = 0; st < 4; ++st)
      for (int64_t w = at[st]; w < at[st + 1]; ++w)
        if (st == 0 || total[(size_t)w]) rows.push_back({stat_names[st], st == 0 ? std::string(total_names[w]) : std::to_string(w - at[st]), std::to_string(total[(size_t)w])});
    print_table({"stat", "bin", "count"}, rows, se.quiet);
    return;
  }

  if (!src.regions_bed.empty()) {  // K11 / K12 / K14: every region of the BED file over the source in ONE pass; the names are resolved per file
    std::ifstream in(src.regions_bed);
    if (!in) throw Err("no such file: " + src.regions_bed);
    std::vector<std::string> names;
    std::vector<int64_t> starts, ends;
    std::string packed, line;
    for (int64_t ln = 1; std::getline(in, line); ++ln) {
      if (!line.empty() && line.back() == '\r') line.pop_back();
      if (line.empty() || line[0] == '#' || line.rfind("track", 0) == 0 || line.rfind("browser", 0) == 0) continue;
      std::istringstream ls(line);
      std::string chrom;
      long long s = -1, e = -1;
      if (!(ls >> chrom >> s >> e) || s < 0 || e < s) throw Err(src.regions_bed + " line " + std::to_string(ln) + ": expected <chrom> <start> <end> with 0 <= start <= end");
      // BED is 0-based half-open: (chrom, s, e) is the 1-based closed interval [s + 1, e], which is empty when s == e
      if (s == e) throw Err(src.regions_bed + " line " + std::to_string(ln) + ": zero-length region " + chrom + ":" + std::to_string(s) + "-" + std::to_string(e));
      names.push_back(chrom);
      packed += chrom;
      packed.push_back('\0');
      starts.push_back(s + 1);
      ends.push_back(e);
    }
    if (names.empty()) throw Err(src.regions_bed + ": no regions");
    exon_hip_ctx* ctx = se.gpu();  // (the region file is judged first: its errors need no device)
    const bool annotation = src.format == EXON_HIP_FORMAT_GFF || src.format == EXON_HIP_FORMAT_GTF;
    const int32_t columns[3] = {annotation ? 0 : 2, 3, 4};
    StreamGuard sg;
    if (src.depth)
      ck(ctx, exon_hip_plan_create_region_set_depth(ctx, columns, packed.data(), packed.size(), nullptr, starts.data(), ends.data(), (int32_t)names.size(),
                                                    src.thresholds.data(), (int32_t)src.thresholds.size(), &sg.p));
    else
      ck(ctx, (src.bases ? exon_hip_plan_create_region_set_bases : exon_hip_plan_create_region_set)(ctx, columns, packed.data(), packed.size(), nullptr, starts.data(),
                                                                                                     ends.data(), (int32_t)names.size(), &sg.p));
    ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
    for (const auto& f : src.files) {  // one stream: the state is keyed by the region set, the files add up
      ScanGuard g; open_scan(src, f, nullptr, "", &g, true);
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
    }
    int64_t n_i64 = 0, n_f64 = 0;
    ck(ctx, exon_hip_plan_state_size(sg.p, &n_i64, &n_f64));
    std::vector<int64_t> state((size_t)n_i64), counts(names.size());
    ck(ctx, exon_hip_stream_finish(sg.s, state.data(), nullptr));
    if (src.depth) {  // one row per BED line: bases, then the bases covered at least T times for every threshold
      const size_t w = 1 + src.thresholds.size();
      std::vector<int64_t> tab(names.size() * w);
      ck(ctx, exon_hip_region_depth_decode(sg.p, state.data(), tab.data()));
      std::vector<std::string> head = {"contig", "start", "end", "bases"};
      for (int64_t t : src.thresholds) head.push_back("ge_" + std::to_string(t));
      std::vector<std::vector<std::string>> rows;
      for (size_t i = 0; i < names.size(); ++i) {
        rows.push_back({names[i], std::to_string(starts[i]), std::to_string(ends[i])});
        for (size_t c = 0; c < w; ++c) rows.back().push_back(std::to_string(tab[i * w + c]));
      }
      print_table(head, rows, se.quiet);
      return;
    }
    ck(ctx, (src.bases ? exon_hip_region_bases_decode : exon_hip_region_set_decode)(sg.p, state.data(), counts.data()));
    std::vector<std::vector<std::string>> rows;
    for (size_t i = 0; i < names.size(); ++i) rows.push_back({names[i], std::to_string(starts[i]), std::to_string(ends[i]), std::to_string(counts[i])});
    print_table({"contig", "start", "end", src.bases ? "bases" : "count"}, rows, se.quiet);
    return;
  }

  if (src.window > 0) {  // K13: the rows' bases per window along every contig; contigs and lengths from the genome file or the first file's header
    std::vector<std::string> names;
    std::vector<int64_t> lengths;
    const bool annotation = src.format == EXON_HIP_FORMAT_GFF || src.format == EXON_HIP_FORMAT_GTF;
    if (!src.genome_file.empty()) {
      std::ifstream in(src.genome_file);
      if (!in) throw Err("no such file: " + src.genome_file);
      std::string line;
      for (int64_t ln = 1; std::getline(in, line); ++ln) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ls(line);
        std::string chrom;
        long long len = 0;
        if (!(ls >> chrom >> len) || len < 1 || len > INT32_MAX)
          throw Err(src.genome_file + " line " + std::to_string(ln) + ": expected <name> <length> with 1 <= length <= 2147483647");
        names.push_back(chrom);
        lengths.push_back(len);
      }
      if (names.empty()) throw Err(src.genome_file + ": no contigs");
    } else {
      if (annotation) throw Err("window_depth: a GFF / GTF source has no contig lengths: give a genome file, window_depth('<file>', <W>, '<genome file>')");
      if (src.files.empty()) throw Err("window_depth: no input file");
      ScanGuard g; open_scan(src, src.files[0], nullptr, "", &g);
      int32_t n = 0;
      ck(nullptr, exon_hip_scan_reference_lengths(g.s, nullptr, 0, &n));
      std::vector<int64_t> len((size_t)n);
      if (n) ck(nullptr, exon_hip_scan_reference_lengths(g.s, len.data(), n, &n));
      for (int32_t i = 0; i < n; ++i) {
        if (len[(size_t)i] < 1) continue;  // (a SAM @SQ without LN: it has no windows)
        const char* name = nullptr;
        ck(nullptr, exon_hip_scan_dictionary_value(g.s, 2, i, &name));
        names.push_back(name);
        lengths.push_back(len[(size_t)i]);
      }
      if (names.empty()) throw Err("window_depth: the header of " + src.files[0] + " names no contig with a length");
    }
    std::string packed;
    for (const auto& nm : names) {
      packed += nm;
      packed.push_back('\0');
    }
    exon_hip_ctx* ctx = se.gpu();  // (the genome file and the header are judged first: their errors need no device)
    const int32_t columns[3] = {annotation ? 0 : 2, 3, 4};
    StreamGuard sg;
    ck(ctx, exon_hip_plan_create_window_bases(ctx, columns, packed.data(), packed.size(), nullptr, lengths.data(), (int32_t)names.size(), src.window, &sg.p));
    ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
    for (const auto& f : src.files) {  // one stream: the state is keyed by the windows, the files add up
      ScanGuard g; open_scan(src, f, nullptr, "", &g, true);
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
    }
    int64_t n_i64 = 0, n_f64 = 0;
    ck(ctx, exon_hip_plan_state_size(sg.p, &n_i64, &n_f64));
    std::vector<int64_t> state((size_t)n_i64), woff(names.size() + 1);
    ck(ctx, exon_hip_stream_finish(sg.s, state.data(), nullptr));
    ck(ctx, exon_hip_window_bases_offsets(sg.p, woff.data()));
    std::vector<int64_t> bases((size_t)woff.back());
    ck(ctx, exon_hip_window_bases_decode(sg.p, state.data(), bases.data()));
    std::vector<std::vector<std::string>> rows;
    for (size_t c = 0; c < names.size(); ++c)
      for (int64_t b = woff[c]; b < woff[c + 1]; ++b) {
        const int64_t j = b - woff[c];
        rows.push_back({names[c], std::to_string(j * src.window + 1), std::to_string(b + 1 == woff[c + 1] ? lengths[c] : (j + 1) * src.window), std::to_string(bases[(size_t)b])});
      }
    print_table({"contig", "start", "end", "bases"}, rows, se.quiet);
    return;
  }

  if (seq_stats) {  // K10: the per-record FASTA tables; every word of the state adds, so the files' states do
    exon_hip_ctx* ctx = se.gpu();
    const int lmax = 65536;
    int64_t at[6];
    ck(nullptr, exon_hip_seq_stats_layout(lmax, at));
    std::vector<int64_t> total((size_t)at[5], 0);
    for (const auto& f : src.files) {
      ScanGuard g; open_scan(src, f, nullptr, "", &g, true);
      StreamGuard sg;
      exon_hip_plan_desc d; memset(&d, 0, sizeof d);
      d.kind = EXON_HIP_PLAN_SEQ_STATS_HIST; d.lmax = lmax; d.columns[0] = 2;
      ck(ctx, exon_hip_plan_create(ctx, &d, &sg.p));
      ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
      std::vector<int64_t> h((size_t)at[5]);
      ck(ctx, exon_hip_stream_finish(sg.s, h.data(), nullptr));
      for (size_t i = 0; i < h.size(); ++i) total[i] += h[i];
    }
    static const char* const stat_names[5] = {"total", "composition", "length", "length_log2", "gc_percent"};
    static const char* const total_names[3] = {"records", "bases", "gc"};
    std::vector<std::vector<std::string>> rows;  // (a composition row shows its byte as a number)
    for (int st = 0; st < 5; ++st)
      for (int64_t w = at[st]; w < at[st + 1]; ++w)
        if (st == 0 || total[(size_t)w]) rows.push_back({stat_names[st], st == 0 ? std::string(total_names[w]) : std::to_string(w - at[st]), std::to_string(total[(size_t)w])});
    print_table({"stat", "bin", "count"}, rows, se.quiet);
    return;
  }

  const bool count_only = proj.size() == 1 && proj[0] == "count(*)" && group_by.empty() && !star;
  if (!count_only && group_by.empty() && pr.kind == Predicate::None && (src.format == EXON_HIP_FORMAT_GFF || src.format == EXON_HIP_FORMAT_GTF)) {
    select_annotation_rows(src, star, proj, limit, se.quiet);
    return;
  }
  if (!count_only && group_by.empty() && pr.kind == Predicate::None && src.format == EXON_HIP_FORMAT_BED) {
    select_bed_rows(src, star, proj, limit, se.quiet);
    return;
  }
  if (count_only && pr.kind == Predicate::PushedRegion && src.format == EXON_HIP_FORMAT_BED) {
    // the region test the CLI knows for GFF sources, over a BED source: reference_sequence_name = name AND start inside the interval,
    // K2 over scan columns (0, 1).  The reference has no region filter for BED, so nothing is pushed into the reader: the text is
    // parsed on the device (EXON_HIP_GPU_PARSE=0: by the host reader) and the plan filters
    exon_hip_ctx* ctx = se.gpu();
    char name[512];
    int64_t a = 1, b = INT64_MAX;
    ck(nullptr, exon_hip_parse_region(pr.region.c_str(), name, sizeof name, &a, &b));
    int64_t total = 0;
    for (const auto& f : src.files) {
      ScanGuard g; open_scan(src, f, nullptr, "", &g, true);
      int32_t sid = -1;
      ck(nullptr, exon_hip_scan_dictionary_intern(g.s, 0, name, &sid));  // (BED has no header: the name seeds the scan's dictionary)
      StreamGuard sg;
      exon_hip_plan_desc d; memset(&d, 0, sizeof d);
      d.kind = EXON_HIP_PLAN_REGION_COUNT; d.region_chrom_id = sid; d.region_start = a; d.region_end = b;
      d.columns[0] = 0; d.columns[1] = 1;
      ck(ctx, exon_hip_plan_create(ctx, &d, &sg.p));
      ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
      int64_t c = 0;
      ck(ctx, exon_hip_stream_finish(sg.s, &c, nullptr));
      total += c;
    }
    print_table({"count(*)"}, {{std::to_string(total)}}, se.quiet);
    return;
  }
  if (count_only && pr.kind == Predicate::PushedRegion && !src.indexed && gpu_parse_enabled() &&
      (src.format == EXON_HIP_FORMAT_BAM || src.format == EXON_HIP_FORMAT_SAM || src.format == EXON_HIP_FORMAT_CRAM)) {  // K6: interval overlap on the GPU
    exon_hip_ctx* ctx = se.gpu();
    char name[512];
    int64_t a = 1, b = INT64_MAX;
    ck(nullptr, exon_hip_parse_region(pr.region.c_str(), name, sizeof name, &a, &b));
    int64_t total = 0;
    for (const auto& f : src.files) {
      ScanGuard g; open_scan(src, f, nullptr, "", &g, true);
      int32_t rid = -1;
      ck(nullptr, exon_hip_scan_dictionary_intern(g.s, 2, name, &rid));
      if (rid < 0) continue;  // the reference is not in this file's header
      push_flags(g.s, &pr);  // (K6 then counts the rows the scan keeps)
      StreamGuard sg;
      exon_hip_plan_desc d; memset(&d, 0, sizeof d);
      d.kind = EXON_HIP_PLAN_OVERLAP_COUNT; d.region_chrom_id = rid; d.region_start = a; d.region_end = b;
      d.columns[0] = 2; d.columns[1] = 3; d.columns[2] = 4;
      ck(ctx, exon_hip_plan_create(ctx, &d, &sg.p));
      ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
      int64_t c = 0;
      ck(ctx, exon_hip_stream_finish(sg.s, &c, nullptr));
      total += c;
    }
    print_table({"count(*)"}, {{std::to_string(total)}}, se.quiet);
    return;
  }
  if (count_only && pr.kind == Predicate::PushedRegion && !src.indexed && gpu_parse_enabled() && (src.format == EXON_HIP_FORMAT_GFF || src.format == EXON_HIP_FORMAT_GTF)) {
    // gff_region_filter is the reference reader's own test (exon-gff/src/batch_reader.rs:76-97: seqname = name AND start inside
    // the interval): K2 over scan columns (0, 3), the text parsed on the device
    exon_hip_ctx* ctx = se.gpu();
    char name[512];
    int64_t a = 1, b = INT64_MAX;
    ck(nullptr, exon_hip_parse_region(pr.region.c_str(), name, sizeof name, &a, &b));
    int64_t total = 0;
    for (const auto& f : src.files) {
      ScanGuard g; open_scan(src, f, nullptr, "", &g, true);
      int32_t sid = -1;
      ck(nullptr, exon_hip_scan_dictionary_intern(g.s, 0, name, &sid));  // (GFF has no header: the name seeds the scan's dictionary)
      StreamGuard sg;
      exon_hip_plan_desc d; memset(&d, 0, sizeof d);
      d.kind = EXON_HIP_PLAN_REGION_COUNT; d.region_chrom_id = sid; d.region_start = a; d.region_end = b;
      d.columns[0] = 0; d.columns[1] = 3;
      ck(ctx, exon_hip_plan_create(ctx, &d, &sg.p));
      ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
      int64_t c = 0;
      ck(ctx, exon_hip_stream_finish(sg.s, &c, nullptr));
      total += c;
    }
    print_table({"count(*)"}, {{std::to_string(total)}}, se.quiet);
    return;
  }
  if (count_only && (pr.kind == Predicate::None || pr.kind == Predicate::PushedRegion)) {
    // config-1 plumbing / pushed-down region: the decoder's per-record filter is the only filter
    print_table({"count(*)"}, {{std::to_string(count_rows(src, pr.region, &pr))}}, se.quiet);
    return;
  }
  if (count_only && pr.kind == Predicate::FlagMapq) {  // WHERE flag & M = V [AND CAST(mapping_quality AS INT) >= q] without GROUP BY: the scan's own filter
    print_table({"count(*)"}, {{std::to_string(count_rows(src, "", &pr))}}, se.quiet);
    return;
  }
  if (count_only && pr.kind == Predicate::Region && (src.format == EXON_HIP_FORMAT_VCF || src.format == EXON_HIP_FORMAT_BCF)) {  // K2
    exon_hip_ctx* ctx = se.gpu();
    int64_t total = 0;
    for (const auto& f : src.files) {
      ScanGuard g; open_scan(src, f, nullptr, "", &g, true);
      int32_t cid = -1;
      ck(nullptr, exon_hip_scan_dictionary_intern(g.s, 0, pr.chrom.c_str(), &cid));
      StreamGuard sg;
      exon_hip_plan_desc d; memset(&d, 0, sizeof d);
      d.kind = EXON_HIP_PLAN_REGION_COUNT; d.region_chrom_id = cid; d.region_start = pr.start; d.region_end = pr.end;
      d.columns[0] = 0; d.columns[1] = 1;
      if (pr.end < pr.start) continue;  // empty interval
      ck(ctx, exon_hip_plan_create(ctx, &d, &sg.p));
      ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
      int64_t c = 0;
      ck(ctx, exon_hip_stream_finish(sg.s, &c, nullptr));
      total += c;
    }
    print_table({"count(*)"}, {{std::to_string(total)}}, se.quiet);
    return;
  }
  if (pr.kind == Predicate::FlagMapq && (src.format == EXON_HIP_FORMAT_BAM || src.format == EXON_HIP_FORMAT_SAM || src.format == EXON_HIP_FORMAT_CRAM) && group_by == "reference") {  // K3
    exon_hip_ctx* ctx = se.gpu();
    std::map<std::string, int64_t> merged;  // AggregateExec(Final): merge per-file partials by key
    int64_t null_group = 0;
    std::vector<std::string> order;
    for (const auto& f : src.files) {
      ScanGuard g; open_scan(src, f, nullptr, "", &g, true);
      int32_t R = 0;
      ck(nullptr, exon_hip_scan_dictionary_size(g.s, 2, &R));
      StreamGuard sg;
      exon_hip_plan_desc d; memset(&d, 0, sizeof d);
      d.kind = EXON_HIP_PLAN_FLAG_MAPQ_GROUP_COUNT; d.n_groups = R; d.flag_mask = pr.flag_mask; d.flag_value = pr.flag_value;
      d.mapq_min = pr.mapq_min; d.columns[0] = 0; d.columns[1] = 1; d.columns[2] = 2;
      ck(ctx, exon_hip_plan_create(ctx, &d, &sg.p));
      ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
      std::vector<int64_t> c((size_t)R + 1);
      ck(ctx, exon_hip_stream_finish(sg.s, c.data(), nullptr));
      for (int32_t r = 0; r < R; ++r)
        if (c[(size_t)r]) {
          const char* nm; ck(nullptr, exon_hip_scan_dictionary_value(g.s, 2, r, &nm));
          if (!merged.count(nm)) order.push_back(nm);
          merged[nm] += c[(size_t)r];
        }
      null_group += c[(size_t)R];
    }
    std::vector<std::vector<std::string>> rows;
    for (const auto& k : order) rows.push_back({k, std::to_string(merged[k])});
    if (null_group) rows.push_back({"NULL", std::to_string(null_group)});
    print_table({"reference", "count(*)"}, rows, se.quiet);
    return;
  }
  if (pr.kind == Predicate::InfoCmp && (src.format == EXON_HIP_FORMAT_VCF || src.format == EXON_HIP_FORMAT_BCF) && group_by == "filter") {  // K4
    if (!se.vcf_parse_info) throw Err("info." + pr.info_field + " needs `SET exon.vcf_parse_info = true` (info is a Utf8 column otherwise)");
    exon_hip_ctx* ctx = se.gpu();
    bool minmax = false;
    for (const auto& it : proj) minmax = minmax || it.rfind("min(", 0) == 0 || it.rfind("max(", 0) == 0;
    if (minmax) {  // K8: ONE stream over all files (their FILTER dictionaries are merged by value inside it)
      std::string arg;  // the one argument of MIN / MAX: qual or info.<key>
      for (const auto& it : proj) {
        if (it == "filter" || it == "count(*)") continue;
        const bool mm = it.rfind("min(", 0) == 0 || it.rfind("max(", 0) == 0;
        const std::string a = mm ? it.substr(4, it.size() - 5) : "";
        if (!mm || (!arg.empty() && a != arg) || (a != "qual" && a.rfind("info.", 0) != 0))
          throw Err("unsupported select item '" + it + "' next to MIN / MAX (supported: filter, MIN(c), MAX(c), COUNT(*) with c = qual or info.\"KEY\")");
        arg = a;
      }
      std::string fields = pr.info_field;
      int ycol = 2;
      if (arg != "qual") {
        const std::string key = arg.substr(5);
        ycol = key == pr.info_field ? 4 : 5;
        if (ycol == 5) fields += "," + key;
      }
      const int G = EXON_HIP_MAX_GROUPS;  // distinct FILTER lists over all files: what the plan kind takes (a 128 KiB state)
      StreamGuard sg;
      exon_hip_plan_desc d; memset(&d, 0, sizeof d);
      d.kind = EXON_HIP_PLAN_CMP_MINMAX_BY_GROUP; d.n_groups = G; d.cmp_op = pr.cmp_op; d.threshold = pr.literal;
      d.columns[0] = 4; d.columns[1] = ycol; d.columns[2] = 3;
      ck(ctx, exon_hip_plan_create(ctx, &d, &sg.p));
      ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
      for (const auto& f : src.files) {
        ScanGuard g; open_scan(src, f, fields.c_str(), "", &g, true);
        ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
      }
      int32_t nk = 0; size_t kb = 0;
      ck(ctx, exon_hip_stream_keys(sg.s, nullptr, 0, &nk, &kb, nullptr));
      std::vector<char> packed(kb + 1);
      ck(ctx, exon_hip_stream_keys(sg.s, packed.data(), kb, &nk, &kb, nullptr));
      std::vector<std::string> keys;
      for (size_t o = 0; (int32_t)keys.size() < nk; o += keys.back().size() + 1) keys.emplace_back(packed.data() + o);
      struct ArrowArray st; struct ArrowSchema sch;  // group, min[min], max[max], count[count], count(*)[count]
      ck(ctx, exon_hip_stream_finish_arrow(sg.s, &st, &sch));
      const bool is_int = sch.children[1]->format[0] == 'i';
      auto cell = [&](int c, int64_t i) -> std::string {
        const struct ArrowArray* a = st.children[c];
        const uint8_t* bm = static_cast<const uint8_t*>(a->buffers[0]);  // (the state batch has no offset)
        if (bm && !((bm[i >> 3] >> (i & 7)) & 1)) return "NULL";
        if (is_int) return std::to_string(static_cast<const int32_t*>(a->buffers[1])[i]);
        return fmt_f64((double)static_cast<const float*>(a->buffers[1])[i]);
      };
      std::vector<std::string> head;
      for (const auto& it : proj) head.push_back(it);
      std::vector<std::vector<std::string>> rows;
      for (int64_t i = 0; i < st.length; ++i) {
        const int32_t gk = static_cast<const int32_t*>(st.children[0]->buffers[1])[i];
        const std::string k = gk < (int32_t)keys.size() ? keys[(size_t)gk] : "";
        std::string list = "[";  // List<Utf8> rendered like datafusion: [a, b]
        for (size_t p0 = 0; !k.empty() && p0 <= k.size();) {
          const size_t sc = k.find(';', p0);
          list += (p0 ? ", " : "") + k.substr(p0, sc == std::string::npos ? std::string::npos : sc - p0);
          if (sc == std::string::npos) break;
          p0 = sc + 1;
        }
        list += "]";
        std::vector<std::string> row;
        for (const auto& it : proj)
          row.push_back(it == "filter" ? list : it == "count(*)" ? std::to_string(static_cast<const int64_t*>(st.children[4]->buffers[1])[i])
                        : cell(it[1] == 'i' ? 1 : 2, i));
        rows.push_back(std::move(row));
      }
      if (st.release) st.release(&st);
      if (sch.release) sch.release(&sch);
      print_table(head, rows, se.quiet);
      return;
    }
    struct Acc { double sum = 0; int64_t cnt = 0, rows = 0; };
    std::map<std::string, Acc> merged;
    std::vector<std::string> order;
    for (const auto& f : src.files) {
      ScanGuard g; open_scan(src, f, pr.info_field.c_str(), "", &g, true);
      StreamGuard sg;
      const int G = 256;  // distinct FILTER lists supported per file (8 in registers + LDS overflow table)
      exon_hip_plan_desc d; memset(&d, 0, sizeof d);
      d.kind = EXON_HIP_PLAN_CMP_AVG_BY_GROUP; d.n_groups = G; d.cmp_op = pr.cmp_op; d.threshold = pr.literal;
      d.columns[0] = 4; d.columns[1] = 2; d.columns[2] = 3;
      ck(ctx, exon_hip_plan_create(ctx, &d, &sg.p));
      ck(ctx, exon_hip_stream_open(sg.p, 0, &sg.s));
      ck(ctx, exon_hip_stream_consume_scan(sg.s, g.s, nullptr));
      int32_t nd = 0;
      ck(nullptr, exon_hip_scan_dictionary_size(g.s, 3, &nd));
      if (nd > G) throw Err("more than " + std::to_string(G) + " distinct FILTER lists in one file");
      std::vector<int64_t> c((size_t)2 * G);
      std::vector<double> s((size_t)G);
      ck(ctx, exon_hip_stream_finish(sg.s, c.data(), s.data()));
      for (int32_t k = 0; k < nd; ++k)
        if (c[(size_t)(G + k)]) {
          const char* nm; ck(nullptr, exon_hip_scan_dictionary_value(g.s, 3, k, &nm));
          if (!merged.count(nm)) order.push_back(nm);
          Acc& a = merged[nm];
          a.sum += s[(size_t)k]; a.cnt += c[(size_t)k]; a.rows += c[(size_t)(G + k)];
        }
    }
    std::vector<std::vector<std::string>> rows;
    for (const auto& k : order) {
      const Acc& a = merged[k];
      std::string list = "[";  // List<Utf8> rendered like datafusion: [a, b]
      size_t st = 0;
      while (!k.empty() && st <= k.size()) {
        const size_t sc = k.find(';', st);
        list += (st ? ", " : "") + k.substr(st, sc == std::string::npos ? std::string::npos : sc - st);
        if (sc == std::string::npos) break;
        st = sc + 1;
      }
      list += "]";
      rows.push_back({list, a.cnt ? fmt_f64(a.sum / (double)a.cnt) : "NULL", std::to_string(a.rows)});
    }
    print_table({"filter", "avg(qual)", "count(*)"}, rows, se.quiet);
    return;
  }
  throw Err("query shape not supported by this build: supported shapes are listed in `exon-hip-cli --help`");
}

void exec_statement(Session& se, const std::string& sql) {
  Parser ps{tokenize(sql)};
  if (ps.at_end()) return;
  if (ps.accept_kw("set")) {
    const std::string key = lower(ps.ident());
    if (!ps.accept_sym("=")) ps.accept_kw("to");
    const std::string val = ps.peek().kind == Tok::Str ? ps.str() : lower(ps.ident());
    if (key == "exon.vcf_parse_info") se.vcf_parse_info = (val == "true");
    return;  // other exon.* options (config/mod.rs:65-78) are accepted and ignored
  }
  if (ps.accept_kw("create")) {
    ps.expect_kw("external"); ps.expect_kw("table");
    const std::string name = lower(ps.ident());
    Table t;
    bool have_loc = false;
    while (!ps.at_end()) {
      if (ps.accept_kw("stored")) { ps.expect_kw("as"); t.format = format_of(ps.ident(), &t.indexed); }
      else if (ps.accept_kw("location")) { t.location = ps.str(); have_loc = true; }
      else if (ps.accept_kw("partitioned")) { ps.expect_kw("by"); ps.expect_sym("("); while (!ps.accept_sym(")")) ps.p++; }
      else if (ps.accept_kw("options")) {
        ps.expect_sym("(");
        while (!ps.accept_sym(")")) {
          std::string k = ps.peek().kind == Tok::Str ? ps.str() : ps.ident();
          std::string v = ps.peek().kind == Tok::Str ? ps.str() : ps.peek().kind == Tok::Num ? ps.number() : ps.ident();
          k = lower(k);
          if (k == "n_fields" || ends_with(k, ".n_fields")) {
            t.n_fields = atoi(v.c_str());
            if (t.n_fields < 3 || t.n_fields > 12) throw Err("n_fields " + v + ": a BED table has 3 to 12 fields");
          }
          if (k == "compression" || ends_with(k, ".compression")) t.compression = compression_of(v);
          if (k == "file_extension" || ends_with(k, ".file_extension")) t.extension = v;
          if (k == "indexed" && lower(v) == "true") t.indexed = true;
          ps.accept_sym(",");
        }
      } else throw Err("unexpected '" + ps.peek().text + "' in CREATE EXTERNAL TABLE");
    }
    if (!t.format || !have_loc) throw Err("CREATE EXTERNAL TABLE needs STORED AS and LOCATION");
    se.tables[name] = t;
    return;
  }
  if (ps.accept_kw("drop")) { ps.expect_kw("table"); se.tables.erase(lower(ps.ident())); return; }
  if (ps.accept_kw("select")) { exec_select(se, ps); return; }
  throw Err("unsupported statement starting with '" + ps.peek().text + "'");
}

void exec_script(Session& se, const std::string& text) {
  std::string cur;
  bool inq = false;
  for (char c : text) {
    if (c == '\'') inq = !inq;
    if (c == ';' && !inq) { exec_statement(se, cur); cur.clear(); }
    else cur += c;
  }
  exec_statement(se, cur);
}

}  // namespace

int main(int argc, char** argv) {
  Session se;
  std::vector<std::string> commands, files;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "-c" || a == "--command") { while (i + 1 < argc && argv[i + 1][0] != '-') commands.push_back(argv[++i]); }
    else if (a == "-f" || a == "--file") { while (i + 1 < argc && argv[i + 1][0] != '-') files.push_back(argv[++i]); }
    else if (a == "-q" || a == "--quiet") se.quiet = true;
    else if (a == "-h" || a == "--help") {
      printf("exon-hip-cli [-q] -c '<sql>'... | -f <file>...\n"
             "  tables:    CREATE EXTERNAL TABLE t STORED AS FASTA|FASTQ|VCF|BAM|GFF|GTF|BED|INDEXED_VCF|INDEXED_BAM|INDEXED_GFF [OPTIONS (compression gzip, n_fields 6)] LOCATION '<path>'\n"
             "  functions: fasta_scan fastq_scan vcf_scan bam_scan gff_scan gtf_scan bed_scan ('<path>'[, 'gzip']); vcf_indexed_scan bam_indexed_scan gff_indexed_scan ('<path>', '<region>');\n"
             "             fastq_quality_histogram('<path>')\n"
             "             fastq_read_stats('<path>')\n"
             "             fasta_seq_stats('<path>'[, 'gzip'])\n"
             "             overlap_counts('<bam|sam|cram|gff|gtf file>', '<regions.bed>'[, 'gzip'])   one row per BED line: contig, start, end (1-based closed), count\n"
             "             covered_bases('<bam|sam|cram|gff|gtf file>', '<regions.bed>'[, 'gzip'])    one row per BED line: contig, start, end (1-based closed), bases\n"
             "             depth_thresholds('<bam|sam|cram|gff|gtf file>', '<regions.bed>', '<T1,T2,...>'[, 'gzip'])  one row per BED line: contig, start, end, bases, ge_<T> = its bases covered at least T times\n"
             "             window_depth('<bam|sam|cram file>', <W>)                                   one row per window of width W along every contig of the header: contig, start, end, bases\n"
             "             window_depth('<bam|sam|cram|gff|gtf file>', <W>, '<genome file>')          the contigs and lengths from `name<TAB>length` lines (a bedtools genome file, a .fai)\n"
             "             covered_bases, depth_thresholds and window_depth take one more last argument over a BAM or SAM file: 'cover=span' (the default: a read's whole\n"
             "             span), 'cover=aligned' (its aligned blocks, M = X: samtools depth, bedcov -j) or 'cover=aligned+del' (+ D: samtools depth -J)\n"
             "  queries:  SELECT COUNT(*) FROM <src> [WHERE chrom = 'c' AND pos >= a AND pos <= b | vcf_region_filter('r', chrom) | bam_region_filter('r', reference, start, end)\n"
             "             | gff_region_filter('r', seqname[, start])]\n"
             "             SELECT COUNT(*) FROM <bam|sam> WHERE [bam_region_filter('r', reference, start, end) AND] flag & M = V [AND CAST(mapping_quality AS INT) >= q]\n"
             "             SELECT reference, COUNT(*) FROM <bam> WHERE flag & M = V AND CAST(mapping_quality AS INT) >= q GROUP BY reference\n"
             "             SET exon.vcf_parse_info = true; SELECT filter, AVG(qual), COUNT(*) FROM <vcf> WHERE info.\"AF\" > 0.01 GROUP BY filter\n"
             "             SELECT filter, MIN(qual), MAX(qual), COUNT(*) FROM <vcf> WHERE info.\"AF\" > 0.01 GROUP BY filter   (also MIN / MAX(info.\"DP\");\n"
             "               at most 4096 distinct FILTER lists over the table's files, one type of the argument in all of them)\n");
      return 0;
    } else { fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
  }
  try {
    for (const auto& c : commands) exec_script(se, c);
    for (const auto& f : files) {
      std::ifstream in(f);
      if (!in) throw Err("cannot read " + f);
      std::stringstream ss;
      ss << in.rdbuf();
      exec_script(se, ss.str());
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "Error: %s\n", e.what());
    return 1;
  }
  return 0;
}
