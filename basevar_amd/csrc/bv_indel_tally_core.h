// bv_indel_tally_core.h -- the CVG row's indel column (column 9) as a function of the row's indel tokens: what
// host/vcf_emit.hpp's indel_string gives, stated on bytes and without reference to lanes.  The kernels of bv_indel_tally.hip
// compile these functions and are their schedule; tests/cpp/indel_tally_check.cpp compiles them with g++ and holds them to
// indel_string byte for byte.
//
// THE DEFINITION.  A row has tokens t[0 .. n), byte strings in any order.
//   kept     a token that is not empty and whose first byte is none of 'N' 'A' 'C' 'G' 'T' (indel_string's filter; the pileup
//            makes no other token, a host caller may)
//   classes  the distinct texts of the kept tokens; a class's count is the number of kept tokens of that text
//   order    std::map<std::string>'s: the bytes compared as UNSIGNED, a proper prefix before the longer text
//   column   text '|' decimal(count) of every class in that order, joined by ','; no class: the empty column, which the
//            record-text interface (bv_record_lines.indel) prints as "."
// A class's entry lies at bv_it_class_at(): the bytes of the entries of the classes below it and their commas.  That is the one
// ranking routine: the column's length is the end of its last entry (bv_it_column_len) and the write puts every entry at its
// place (bv_it_column_put), so a count pass and a write pass that both go through it cannot disagree.
//
// THE DOMAIN.  Nothing outside it is handled; such a row is flagged (BV_IT_OUTSIDE) and left to the caller:
//   * at most BV_INDEL_ROW_TOKENS_MAX tokens in a row, kept or not.  What bounds it: a wave keeps, per token, a 4-byte key and a
//     2-byte class number, and per class 6 bytes, in the 160 KiB of LDS one workgroup of a gfx950 CU may have.  An entry takes
//     at least 4 bytes of the column ("+|1,"), so a column inside the domain has at most BV_IT_CLASSES_MAX = 4,096 classes, and
//     16,384 tokens take 96 + 24 = 120 KiB; token indices, counts and entry offsets then fit 16 bits, with two class numbers
//     reserved.  (A cohort of 10,000 samples can put 10,000 tokens into a row; 4,096 would not hold it.)
//   * at most BV_IT_COLUMN_MAX (BV_RECORD_TEXT_INDEL_MAX, 16,384) bytes in a row's column
//   * a token may have any length up to 2^32 - 1; one of more than BV_IT_COLUMN_MAX bytes, if kept, puts its row outside
// A token whose text does not lie inside the text buffer is damage, not a row outside the domain (BV_IT_BAD): no byte of it is read.
//
// Keys.  Texts are compared byte by byte, at any address, no word is loaded across a token's edge.  To keep most compares off
// the text, a token carries a key: its first four bytes, big-endian, a shorter text padded with zero bytes.  Two different keys
// order their texts as the texts themselves do (at the first byte where the keys differ either both texts have a byte there, or
// the shorter has ended and its pad 0 is below the other's non-zero byte: a proper prefix); equal keys say that the texts agree
// over min(4, both lengths) bytes, and the compare goes on from there.  tests/cpp/indel_tally_check.cpp holds bv_it_cmp to
// std::string's operator< on pairs built for every such edge.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BV_IT_FN __host__ __device__ __forceinline__
#else
#define BV_IT_FN inline
#endif

#define BV_INDEL_ROW_TOKENS_MAX 16384u
#define BV_IT_COLUMN_MAX 16384u
#define BV_IT_CLASSES_MAX ((BV_IT_COLUMN_MAX + 1u) / 4u)  // of a column inside the domain: bv_it_column_grow
#define BV_IT_UNASSIGNED 0xffffu  // bv_it_row.cls: a kept token of no class yet
#define BV_IT_DROPPED 0xfffeu     //                a token the filter drops
enum { BV_IT_OK = 0, BV_IT_OUTSIDE = 1, BV_IT_BAD = 2 };  // a row: tallied here; outside the domain; a token beyond the text

// one token: bv_pileup_token's layout (include/basevar_amd_pileup.h); `sample` is not read
struct bv_it_token {
    uint32_t pos, sample;
    uint64_t text_off;
    uint32_t text_len, reserved_;
};

// A row's tokens tok[0 .. n) over `text`, and the working storage of its tally
struct bv_it_row {
    const bv_it_token *tok;
    const uint8_t *text;
    uint32_t n;
    uint32_t *key;   // [n] bv_it_key of the token
    uint16_t *cls;   // [n] the token's class, BV_IT_UNASSIGNED or BV_IT_DROPPED
    uint16_t *rep;   // [classes] the class's first token
    uint16_t *cnt;   // [classes] its tokens
};

BV_IT_FN bool bv_it_token_ok(const bv_it_token *t, uint64_t text_bytes) { return t->text_off <= text_bytes && t->text_len <= text_bytes - t->text_off; }

BV_IT_FN bool bv_it_keep(const uint8_t *p, uint32_t len) {
    if (len == 0) return false;
    const uint8_t c = p[0];
    return c != 'N' && c != 'A' && c != 'C' && c != 'G' && c != 'T';
}

BV_IT_FN uint32_t bv_it_key(const uint8_t *p, uint32_t len) {
    uint32_t k = 0;
    for (uint32_t i = 0; i < 4u; ++i) k = (k << 8) | (i < len ? (uint32_t)p[i] : 0u);
    return k;
}

// < 0, 0, > 0: text a below, equal to, above text b; ka, kb their keys
BV_IT_FN int bv_it_cmp(uint32_t ka, const uint8_t *a, uint32_t alen, uint32_t kb, const uint8_t *b, uint32_t blen) {
    if (ka != kb) return ka < kb ? -1 : 1;
    const uint32_t m = alen < blen ? alen : blen;
    for (uint32_t i = m < 4u ? m : 4u; i < m; ++i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return alen == blen ? 0 : alen < blen ? -1 : 1;
}

BV_IT_FN const uint8_t *bv_it_text(const bv_it_row *r, uint32_t i) { return r->text + r->tok[i].text_off; }

// tokens i and j of the row, both inside the text: the same text?
BV_IT_FN bool bv_it_same(const bv_it_row *r, uint32_t i, uint32_t j) {
    const uint32_t len = r->tok[i].text_len;
    if (r->key[i] != r->key[j] || len != r->tok[j].text_len) return false;
    const uint8_t *a = bv_it_text(r, i), *b = bv_it_text(r, j);
    for (uint32_t k = len < 4u ? len : 4u; k < len; ++k)
        if (a[k] != b[k]) return false;
    return true;
}

BV_IT_FN uint32_t bv_it_dec_len(uint32_t v) {
    uint32_t n = 1;
    while (v >= 10u) { v /= 10u; ++n; }
    return n;
}

// the decimal digits of v, bv_it_dec_len(v) of them
BV_IT_FN void bv_it_dec_put(uint32_t v, uint8_t *out) {
    for (uint32_t n = bv_it_dec_len(v); n > 0; --n) { out[n - 1u] = (uint8_t)('0' + v % 10u); v /= 10u; }
}

// a class's entry: text '|' count
BV_IT_FN uint32_t bv_it_entry_len(uint32_t text_len, uint32_t count) { return text_len + 1u + bv_it_dec_len(count); }

// token i's key and state, before any class is made; false: the token does not lie inside the text
BV_IT_FN bool bv_it_token_prepare(const bv_it_row *r, uint32_t i, uint64_t text_bytes) {
    if (!bv_it_token_ok(r->tok + i, text_bytes)) {
        r->key[i] = 0; r->cls[i] = BV_IT_DROPPED;
        return false;
    }
    const uint8_t *p = bv_it_text(r, i);
    const uint32_t len = r->tok[i].text_len;
    r->key[i] = bv_it_key(p, len);
    r->cls[i] = bv_it_keep(p, len) ? BV_IT_UNASSIGNED : BV_IT_DROPPED;
    return true;
}

// A new class's bytes join the running sum of the entries and a comma each; false: the column has left the domain
BV_IT_FN bool bv_it_column_grow(uint32_t *sum, uint32_t text_len, uint32_t count) {
    if (text_len > BV_IT_COLUMN_MAX) return false;
    *sum += bv_it_entry_len(text_len, count) + 1u;
    return *sum <= BV_IT_COLUMN_MAX + 1u;  // (the last entry has no comma)
}

// The classes of the row, class first: the first token of no class is the next class's representative, and every later token
// of its text joins it.  Classes are numbered in the order of their representatives.  BV_IT_OK: *n_cls classes in rep / cnt.
BV_IT_FN int bv_it_classify(const bv_it_row *r, uint64_t text_bytes, uint32_t *n_cls) {
    *n_cls = 0;
    if (r->n > BV_INDEL_ROW_TOKENS_MAX) return BV_IT_OUTSIDE;
    bool ok = true;
    for (uint32_t i = 0; i < r->n; ++i) ok = bv_it_token_prepare(r, i, text_bytes) && ok;
    if (!ok) return BV_IT_BAD;
    uint32_t sum = 0, c = 0;
    for (uint32_t i = 0; i < r->n; ++i) {
        if (r->cls[i] != BV_IT_UNASSIGNED) continue;
        uint32_t count = 0;
        for (uint32_t j = i; j < r->n; ++j)
            if (r->cls[j] == BV_IT_UNASSIGNED && bv_it_same(r, i, j)) { r->cls[j] = (uint16_t)c; ++count; }
        if (!bv_it_column_grow(&sum, r->tok[i].text_len, count)) return BV_IT_OUTSIDE;  // (so c < BV_IT_CLASSES_MAX here)
        r->rep[c] = (uint16_t)i; r->cnt[c] = (uint16_t)count;
        ++c;
    }
    *n_cls = c;
    return BV_IT_OK;
}

// The one ranking routine: where class c's entry begins in the column -- the entries of the classes below it, a comma each
BV_IT_FN uint32_t bv_it_class_at(const bv_it_row *r, uint32_t n_cls, uint32_t c) {
    const uint32_t i = r->rep[c], ki = r->key[i], li = r->tok[i].text_len;
    const uint8_t *ti = bv_it_text(r, i);
    uint32_t at = 0;
    for (uint32_t d = 0; d < n_cls; ++d) {
        const uint32_t j = r->rep[d];
        if (d != c && bv_it_cmp(r->key[j], bv_it_text(r, j), r->tok[j].text_len, ki, ti, li) < 0) at += bv_it_entry_len(r->tok[j].text_len, r->cnt[d]) + 1u;
    }
    return at;
}

BV_IT_FN uint32_t bv_it_class_end(const bv_it_row *r, uint32_t n_cls, uint32_t c) {
    return bv_it_class_at(r, n_cls, c) + bv_it_entry_len(r->tok[r->rep[c]].text_len, r->cnt[c]);
}

// the column's bytes: where its last entry ends (0: no class)
BV_IT_FN uint32_t bv_it_column_len(const bv_it_row *r, uint32_t n_cls) {
    uint32_t len = 0;
    for (uint32_t c = 0; c < n_cls; ++c) {
        const uint32_t end = bv_it_class_end(r, n_cls, c);
        if (end > len) len = end;
    }
    return len;
}

// what class c's entry puts behind its text, at out: '|', the count, and the comma of every entry but the column's last
BV_IT_FN void bv_it_entry_tail_put(uint32_t count, bool last, uint8_t *out) {
    out[0] = '|';
    bv_it_dec_put(count, out + 1);
    if (!last) out[1u + bv_it_dec_len(count)] = ',';
}

// the column of bv_it_column_len bytes
BV_IT_FN void bv_it_column_put(const bv_it_row *r, uint32_t n_cls, uint8_t *out) {
    const uint32_t total = bv_it_column_len(r, n_cls);
    for (uint32_t c = 0; c < n_cls; ++c) {
        const uint32_t i = r->rep[c], len = r->tok[i].text_len, at = bv_it_class_at(r, n_cls, c);
        const uint8_t *t = bv_it_text(r, i);
        for (uint32_t k = 0; k < len; ++k) out[at + k] = t[k];
        bv_it_entry_tail_put(r->cnt[c], at + bv_it_entry_len(len, r->cnt[c]) == total, out + at + len);
    }
}
