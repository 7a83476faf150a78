// vcf_sample_walk.h -- the `formats` Utf8 column of a VCF record cut into items nobody has to walk a whole row for: the FORMAT
// field (its keys -> a packed word of value types) and ONE sample (its values printed by those types).  host/vcf_text.h
// (vcf_formats_string, print_value, print_i32, print_genotype) is the authority and what the host reader runs; this restates it
// allocation-free, for host and device, templated on an emitter with the methods of text_columns.hip's `info` emitters:
//   byte(c)            one byte
//   span(off, len)     text[off, off + len) as it stands
//   i32(minus, v)      an Integer item: '-' when `minus`, then v in decimal
//   f32(bits)          a Float item through f32p::print
// THE RULES (restated):
//   FORMAT   empty, "." or absent: the row prints "\t" and none of its samples (types = 0).  Otherwise the keys between ':' give
//            the types, in order: "GT" by its name, whatever the header says; else what `type_of` answers for the key ('i' 'f' 'c',
//            anything else a String; an empty key is a key).  More than MAX_KEYS keys: undecided.
//   sample   values between ':'; value k is printed by type k, values behind the last key are dropped, fewer values than keys are
//            fine; the printed values are joined by ':'.  A value that has a key and is empty or ".": undecided (the host raises).
//   value    String values, and Character values without a comma, are copied.  Otherwise the items between ',' one by one: "."
//            prints "." except in a Character list, which drops it; an Integer by the i32 rules (sign, digits, |v| <= 2^31 and
//            v <= 2^31 - 1; printed without '+', leading zeros or "-0"), else undecided; a Float through dec::parse_f32, or one of
//            the inf / infinity / nan spellings, then f32p; what parse_f32 leaves open is undecided.
//   GT       alleles between '/' and '|'; an allele is "." or digits, copied without their leading zeros (any length: nothing is
//            converted); an empty allele or any other byte: undecided.  Allele 0's phasing is '/' when any separator of the
//            genotype is '/', else '|'; allele i >= 1 has the phasing of the separator in front of it; what is printed in front
//            of allele i >= 1 is the phasing of allele i - 1 ("0|1/2" prints "0/1|2").
//   bytes    a byte >= 0x80 anywhere in FORMAT or in the sample: undecided (whether it is UTF-8 is the host reader's to say).
#pragma once
#include <stdint.h>

#include "decimal_f32.h"
#include "f32_print.h"

namespace exon {
namespace vsw {

enum : unsigned { T_NONE = 0, T_STRING = 1, T_CHAR = 2, T_INT = 3, T_FLOAT = 4, T_GT = 5 };  // 4 bits a key; 0: no key here
constexpr unsigned MAX_KEYS = 16;                                                             // a uint64_t of types

EXON_HD unsigned type_code(unsigned kind) { return kind == 'i' ? T_INT : kind == 'f' ? T_FLOAT : kind == 'c' ? T_CHAR : kind == 'g' ? T_GT : T_STRING; }

// [sign] (inf | infinity | nan) in any letter case: the spellings Rust's f32::from_str takes next to the decimals
EXON_HD bool f32_word(const uint8_t* text, unsigned a, unsigned e, uint32_t* bits) {
  uint32_t sign = 0;
  if (a < e && (text[a] == '-' || text[a] == '+')) sign = text[a++] == '-' ? 0x80000000u : 0u;
  const unsigned n = e - a;
  if (n != 3 && n != 8) return false;
  uint64_t w = 0;  // the letters, lower case, first one in the top byte
  for (unsigned i = 0; i < n; ++i) w = w << 8 | (uint64_t)(text[a + i] | 0x20u);
  if (w == 0x696e66ull || w == 0x696e66696e697479ull) *bits = sign | 0x7F800000u;  // "inf", "infinity"
  else if (w == 0x6e616eull) *bits = sign | 0x7FC00000u;                           // "nan"
  else return false;
  return true;
}

// the FORMAT field text[begin, end) -> *types (0: the row prints "\t" alone).  type_of(key begin, key length) -> 'i' 'f' 'c' 's'.
// false: undecided
template <class TypeOf>
EXON_HD bool format_keys(const uint8_t* text, unsigned begin, unsigned end, TypeOf&& type_of, uint64_t* types) {
  *types = 0;
  if (end == begin || (end == begin + 1 && text[begin] == '.')) return true;
  uint64_t ty = 0;
  unsigned n = 0, kb = begin;
  bool bad = false;
  for (unsigned i = begin; i <= end; ++i) {
    if (i < end) {
      const unsigned c = text[i];
      bad |= c >= 0x80u;
      if (c != ':') continue;
    }
    if (n == MAX_KEYS) return false;
    const bool gt = i - kb == 2 && text[kb] == 'G' && text[kb + 1] == 'T';
    ty |= (uint64_t)(gt ? (unsigned)T_GT : type_code((unsigned)type_of(kb, i - kb))) << (4 * n);
    ++n;
    kb = i + 1;
  }
  if (bad) return false;
  *types = ty;
  return true;
}

// a genotype text[vb, ve) (not empty); true: undecided
template <class Emit>
EXON_HD bool genotype(const uint8_t* text, unsigned vb, unsigned ve, Emit& em) {
  bool any_unphased = false, bad = false;
  for (unsigned i = vb; i < ve; ++i) any_unphased |= text[i] == '/';
  unsigned prev = any_unphased ? '/' : '|';  // the phasing of the allele in front of the next one
  unsigned a = vb, index = 0;
  for (unsigned i = vb; i <= ve && !bad; ++i) {
    if (i < ve && text[i] != '/' && text[i] != '|') continue;
    if (i == a) {
      bad = true;  // an empty allele
    } else {
      if (index) em.byte(prev);
      if (i - a == 1 && text[a] == '.') {
        em.byte('.');
      } else {
        for (unsigned k = a; k < i; ++k) bad |= (unsigned)text[k] - (unsigned)'0' > 9u;
        unsigned z = a;
        while (z + 1 < i && text[z] == '0') ++z;
        if (!bad) em.span(z, i - z);
      }
      if (index) prev = text[a - 1];  // (the separator in front of this allele)
    }
    a = i + 1;
    ++index;
  }
  return bad;
}

// a value text[vb, ve) (not empty, not ".") of type ty (not T_GT); true: undecided
template <class Emit>
EXON_HD bool value(const uint8_t* text, unsigned vb, unsigned ve, unsigned ty, Emit& em) {
  bool comma = false;
  if (ty == T_CHAR)
    for (unsigned k = vb; k < ve; ++k) comma |= text[k] == ',';
  if (ty == T_STRING || (ty == T_CHAR && !comma)) {
    em.span(vb, ve - vb);
    return false;
  }
  bool bad = false, first_item = true;
  for (unsigned a = vb; a <= ve && !bad;) {
    unsigned e = a;
    while (e < ve && text[e] != ',') ++e;
    const bool dot = e - a == 1 && text[a] == '.';
    if (!(dot && ty == T_CHAR)) {
      if (!first_item) em.byte(',');
      first_item = false;
      if (dot) {
        em.byte('.');
      } else if (ty == T_INT) {
        unsigned k = a;
        bool neg = false;
        if (k < e && (text[k] == '-' || text[k] == '+')) neg = text[k++] == '-';
        bad |= k == e;
        uint64_t v = 0;
        for (; k < e; ++k) {
          const unsigned d = (unsigned)text[k] - (unsigned)'0';
          bad |= d > 9u;
          v = v * 10 + d;
          if (v > 0x80000000ull) v = 0x80000001ull;  // (out of range for good: print_i32 stops here)
        }
        bad |= v > 0x80000000ull || (!neg && v > 0x7FFFFFFFull);
        if (!bad) em.i32(neg && v != 0, (uint32_t)v);
      } else if (ty == T_FLOAT) {
        uint32_t bits = 0;
        if (dec::parse_f32(reinterpret_cast<const char*>(text + a), (int)(e - a), &bits) || f32_word(text, a, e, &bits)) em.f32(bits);
        else bad = true;
      } else {
        em.span(a, e - a);
      }
    }
    a = e + 1;
  }
  return bad;
}

// ONE sample text[begin, end) (between two TABs, or a TAB and the line's end without its CR) printed by `types`; the TAB in front
// of a sample is the caller's.  true: undecided (what has been emitted by then does not count)
template <class Emit>
EXON_HD bool sample(const uint8_t* text, unsigned begin, unsigned end, uint64_t types, Emit& em) {
  bool bad = false, first_value = true;
  unsigned k = 0;
  for (unsigned a = begin; a <= end && !bad; ++k) {
    unsigned q = a;
    for (; q < end && text[q] != ':'; ++q) bad |= text[q] >= 0x80u;
    const unsigned ty = k < MAX_KEYS ? (unsigned)(types >> (4 * k)) & 15u : 0u;
    if (ty && !bad) {
      if (q == a || (q == a + 1 && text[a] == '.')) {
        bad = true;  // a missing value
      } else {
        if (!first_value) em.byte(':');
        first_value = false;
        bad = ty == T_GT ? genotype(text, a, q, em) : value(text, a, q, ty, em);
      }
    }
    a = q + 1;
  }
  return bad;
}

}  // namespace vsw
}  // namespace exon
