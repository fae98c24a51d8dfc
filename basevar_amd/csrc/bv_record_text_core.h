// bv_record_text_core.h -- the bytes of one VCF head (CHROM through FORMAT) and of one CVG row, from the engine's records
// (bv_engine_vcf_format_records / bv_engine_cvg_format, include/basevar_amd_record_text.h), as inline functions that the
// device kernels (bv_record_text.hip) and a plain g++ harness (tests/cpp/record_text_check.cpp) both compile.  The numbers'
// text is bv_numfmt_core.h's.
//
// THE BYTES, defined without reference to lanes.  A line is the concatenation of its ITEMS, and an item is
//   lit || txt || lit2 || chars || num      (any part may be empty)
// For a record r, its group records g[0 .. G), the group names, CHROM, POS, the REF character and the row's indel column:
//
//   VCF head, 26 + 3 G items; the empty text if r.n_alt == 0.  a_i = r.alt[i] & 3; items with i >= r.n_alt are empty.
//     0  CHROM                          1  '\t' u32(POS)                      2  "\t.\t" REF
//     3  '\t' "ACGT"[a_0] { ',' "ACGT"[a_i] }                                 4  '\t' f6(qual)
//     5  (qual > 20 ? "\t.\t" : "\tLowQual\t") "CM_DP=" i32(total_depth)
//     6+i   (i ? "," : ";CM_AC=")  i32(depth[a_i])      9+i  (i ? "," : ";CM_AF=") g6(af[i])     12+i  (i ? "," : ";CM_CAF=") g6(caf[i])
//     15 ";MQRankSum=" iod(mq_ranksum)  16 ";ReadPosRankSum=" iod(rpr_ranksum)  17 ";BaseQRankSum=" iod(bq_ranksum)
//     18 ";QD=" f6(qd)   19 ";SOR=" f6(var_sor)   20 ";FS=" f6(var_fs)
//     21 ";SB_REF=" i32(var_sb[0])   22 "," i32(var_sb[1])   23 ";SB_ALT=" i32(var_sb[2])   24 "," i32(var_sb[3])
//     25+3j+i  group j, empty if g[j].n_alt <= i:  (i ? "," : ";" name_j "_AF=") g6(g[j].af[i])
//     25+3G  "\tGT:AB:SO:BP"
//   CVG row, 16 items; the empty text if r.total_depth == 0.
//     0  CHROM    1  '\t' u32(POS)    2  '\t' REF    3  '\t' i32(total_depth)    4+b  '\t' i32(depth[b]), b = 0 .. 3
//     8  '\t' and the indel column, "." where the row brings none             9  '\t' f6(cvg_fs)    10  '\t' f6(cvg_sor)
//     11+b  (b ? "," : "\t") i32(cvg_sb[b])                                   15  '\n'
// These are the bytes of host/vcf_emit.hpp's format_vcf_head and format_cvg_line; the harness holds this file to them.
// The indel column (the sorted "TOKEN|count" tally, indel_string()) is NOT computed here: a row brings it as text.
//
// A line is on the device's side iff every number it prints is inside its format's domain (bv_numfmt_*_ok):
// bv_rt_on_device, which the C ABI exports as bv_record_text_on_device.
#ifndef BV_RECORD_TEXT_CORE_H
#define BV_RECORD_TEXT_CORE_H

#include "../../include/basevar_amd.h"
#include "bv_numfmt_core.h"

#define BV_RT_VCF_FIXED_ITEMS 26u  // items of a VCF head beside its groups'
#define BV_RT_VCF_GROUP0 25u       // the first group item
#define BV_RT_CVG_ITEMS 16u
#define BV_RT_TXT_MAX 255u         // CHROM and a group name, bytes
#define BV_RT_INDEL_MAX 16384u     // an indel column, bytes
#define BV_RT_ITEM_MAX (1u + BV_RT_TXT_MAX + 4u + 12u)  // the longest item but an indel column: ';' name "_AF=" g6

// What a line is made from.  The pointers are read only through the item functions below.
typedef struct bv_rt_ctx {
    const bv_site_result *r;
    const bv_group_result *g;   // [n_groups]
    const uint8_t *names;       // group j's name is names[name_off[j] .. name_off[j + 1])
    const uint32_t *name_off;   // [n_groups + 1]
    const uint8_t *chrom;
    const uint8_t *indel;       // CVG: the row's indel column, indel_len == 0: "."
    uint32_t n_groups, chrom_len, indel_len, pos;
    uint8_t ref;
} bv_rt_ctx;

typedef struct bv_rt_item {
    const char *lit, *lit2;
    const uint8_t *txt;
    uint32_t lit_len, lit2_len, txt_len, n_chars;
    uint64_t chars;  // n_chars bytes, the first in the low byte
    bv_numfmt_val num;
} bv_rt_item;

BV_NUMFMT_FN bv_rt_item bv_rt_item_empty(void) {
    bv_rt_item it;
    it.lit = it.lit2 = 0; it.txt = 0;
    it.lit_len = it.lit2_len = it.txt_len = it.n_chars = 0;
    it.chars = 0;
    it.num = bv_numfmt_none();
    return it;
}
#define BV_RT_LIT(it, s) ((it).lit = (s), (it).lit_len = (uint32_t)sizeof(s) - 1u)

#define BV_RT_MAX_ALT 3u  // ALTs of a record that is formatted here; a record of BV_MAX_ALT = 4 (REF outside ACGT) is the host's
BV_NUMFMT_FN uint32_t bv_rt_n_alt(uint8_t n_alt) { return n_alt < BV_RT_MAX_ALT ? n_alt : BV_RT_MAX_ALT; }

BV_NUMFMT_FN uint32_t bv_rt_vcf_items(const bv_rt_ctx *c) { return c->r->n_alt == 0 ? 0u : BV_RT_VCF_FIXED_ITEMS + 3u * c->n_groups; }
BV_NUMFMT_FN uint32_t bv_rt_cvg_items(const bv_rt_ctx *c) { return c->r->total_depth == 0 ? 0u : BV_RT_CVG_ITEMS; }

BV_NUMFMT_FN bv_rt_item bv_rt_vcf_item(const bv_rt_ctx *c, uint32_t idx) {
    const bv_site_result *r = c->r;
    bv_rt_item it = bv_rt_item_empty();
    const uint32_t n_alt = bv_rt_n_alt(r->n_alt), last = BV_RT_VCF_GROUP0 + 3u * c->n_groups;
    if (idx == last) { BV_RT_LIT(it, "\tGT:AB:SO:BP"); return it; }
    if (idx >= BV_RT_VCF_GROUP0) {
        const uint32_t j = (idx - BV_RT_VCF_GROUP0) / 3u, i = (idx - BV_RT_VCF_GROUP0) % 3u;
        if (idx > last || i >= bv_rt_n_alt(c->g[j].n_alt)) return it;
        if (i == 0) {
            BV_RT_LIT(it, ";");
            if (c->name_off) { it.txt = c->names + c->name_off[j]; it.txt_len = c->name_off[j + 1u] - c->name_off[j]; }
            it.lit2 = "_AF="; it.lit2_len = 4u;
        } else {
            BV_RT_LIT(it, ",");
        }
        it.num = bv_numfmt_g6(c->g[j].af[i]);
        return it;
    }
    if (idx >= 6u && idx < 15u) {
        const uint32_t f = (idx - 6u) / 3u, i = (idx - 6u) % 3u;
        if (i >= n_alt) return it;
        if (i) BV_RT_LIT(it, ",");
        else if (f == 0) BV_RT_LIT(it, ";CM_AC=");
        else if (f == 1) BV_RT_LIT(it, ";CM_AF=");
        else BV_RT_LIT(it, ";CM_CAF=");
        it.num = f == 0 ? bv_numfmt_i32(r->depth[r->alt[i] & 3u]) : f == 1 ? bv_numfmt_g6(r->af[i]) : bv_numfmt_g6(r->caf[i]);
        return it;
    }
    switch (idx) {
        case 0: it.txt = c->chrom; it.txt_len = c->chrom_len; break;
        case 1: BV_RT_LIT(it, "\t"); it.num = bv_numfmt_u32(c->pos); break;
        case 2: BV_RT_LIT(it, "\t.\t"); it.chars = c->ref; it.n_chars = 1; break;
        case 3:
            BV_RT_LIT(it, "\t");
            for (uint32_t i = 0; i < n_alt; ++i) {
                if (i) it.chars |= (uint64_t)',' << (8u * it.n_chars++);
                it.chars |= (uint64_t)(uint8_t)"ACGT"[r->alt[i] & 3u] << (8u * it.n_chars++);
            }
            break;
        case 4: BV_RT_LIT(it, "\t"); it.num = bv_numfmt_f6(r->qual); break;
        case 5:
            if (r->qual > 20) BV_RT_LIT(it, "\t.\tCM_DP=");
            else BV_RT_LIT(it, "\tLowQual\tCM_DP=");
            it.num = bv_numfmt_i32(r->total_depth);
            break;
        case 15: BV_RT_LIT(it, ";MQRankSum="); it.num = bv_numfmt_iod(r->mq_ranksum); break;
        case 16: BV_RT_LIT(it, ";ReadPosRankSum="); it.num = bv_numfmt_iod(r->rpr_ranksum); break;
        case 17: BV_RT_LIT(it, ";BaseQRankSum="); it.num = bv_numfmt_iod(r->bq_ranksum); break;
        case 18: BV_RT_LIT(it, ";QD="); it.num = bv_numfmt_f6(r->qd); break;
        case 19: BV_RT_LIT(it, ";SOR="); it.num = bv_numfmt_f6(r->var_sor); break;
        case 20: BV_RT_LIT(it, ";FS="); it.num = bv_numfmt_f6(r->var_fs); break;
        case 21: BV_RT_LIT(it, ";SB_REF="); it.num = bv_numfmt_i32(r->var_sb[0]); break;
        case 22: BV_RT_LIT(it, ","); it.num = bv_numfmt_i32(r->var_sb[1]); break;
        case 23: BV_RT_LIT(it, ";SB_ALT="); it.num = bv_numfmt_i32(r->var_sb[2]); break;
        default: BV_RT_LIT(it, ","); it.num = bv_numfmt_i32(r->var_sb[3]); break;  // 24
    }
    return it;
}

BV_NUMFMT_FN bv_rt_item bv_rt_cvg_item(const bv_rt_ctx *c, uint32_t idx) {
    const bv_site_result *r = c->r;
    bv_rt_item it = bv_rt_item_empty();
    if (idx >= BV_RT_CVG_ITEMS) return it;
    if (idx == 0) { it.txt = c->chrom; it.txt_len = c->chrom_len; return it; }
    if (idx == 15u) { BV_RT_LIT(it, "\n"); return it; }
    if (idx > 11u) BV_RT_LIT(it, ",");
    else BV_RT_LIT(it, "\t");
    if (idx == 1u) it.num = bv_numfmt_u32(c->pos);
    else if (idx == 2u) { it.chars = c->ref; it.n_chars = 1; }
    else if (idx == 3u) it.num = bv_numfmt_i32(r->total_depth);
    else if (idx < 8u) it.num = bv_numfmt_i32(r->depth[idx - 4u]);
    else if (idx == 8u) {
        if (c->indel_len) { it.txt = c->indel; it.txt_len = c->indel_len; }
        else { it.chars = '.'; it.n_chars = 1; }
    } else if (idx == 9u) it.num = bv_numfmt_f6(r->cvg_fs);
    else if (idx == 10u) it.num = bv_numfmt_f6(r->cvg_sor);
    else it.num = bv_numfmt_i32(r->cvg_sb[idx - 11u]);
    return it;
}

BV_NUMFMT_FN bool bv_rt_item_bad(const bv_rt_item *it) { return it->num.kind == BV_NUM_BAD; }
BV_NUMFMT_FN uint32_t bv_rt_item_len(const bv_rt_item *it) { return it->lit_len + it->txt_len + it->lit2_len + it->n_chars + bv_numfmt_len(it->num); }

// writes bv_rt_item_len(it) bytes
BV_NUMFMT_FN void bv_rt_item_put(const bv_rt_item *it, uint8_t *out) {
    for (uint32_t i = 0; i < it->lit_len; ++i) *out++ = (uint8_t)it->lit[i];
    for (uint32_t i = 0; i < it->txt_len; ++i) *out++ = it->txt[i];
    for (uint32_t i = 0; i < it->lit2_len; ++i) *out++ = (uint8_t)it->lit2[i];
    for (uint32_t i = 0; i < it->n_chars; ++i) *out++ = (uint8_t)(it->chars >> (8u * i));
    bv_numfmt_put(it->num, out);
}

// The serial line builders: the line's bytes to out (NULL: only counted); return its length.  *bad_item, if given, is
// the first item with a number outside its domain, or UINT32_MAX; such an item contributes its text without the number.
BV_NUMFMT_FN uint64_t bv_rt_line(const bv_rt_ctx *c, bool cvg, uint8_t *out, uint32_t *bad_item) {
    const uint32_t n = cvg ? bv_rt_cvg_items(c) : bv_rt_vcf_items(c);
    uint64_t at = 0;
    if (bad_item) *bad_item = 0xffffffffu;
    for (uint32_t idx = 0; idx < n; ++idx) {
        const bv_rt_item it = cvg ? bv_rt_cvg_item(c, idx) : bv_rt_vcf_item(c, idx);
        if (bv_rt_item_bad(&it) && bad_item && *bad_item == 0xffffffffu) *bad_item = idx;
        if (out) bv_rt_item_put(&it, out + at);
        at += bv_rt_item_len(&it);
    }
    return at;
}

// Is every number that the record's VCF head and CVG row print inside its format's domain?  (Stated field by field; the harness
// holds it to the items: true iff no item of the two lines is BV_NUM_BAD.)
BV_NUMFMT_FN bool bv_rt_on_device(const bv_site_result *r, const bv_group_result *g, uint32_t n_groups) {
    if (!g) n_groups = 0;
    if (r->n_alt > BV_RT_MAX_ALT) return false;
    for (uint32_t j = 0; j < n_groups; ++j)
        if (g[j].n_alt > BV_RT_MAX_ALT) return false;
    if (r->total_depth != 0 && !(bv_numfmt_f6_ok(r->cvg_fs) && bv_numfmt_f6_ok(r->cvg_sor))) return false;  // the CVG row's two
    if (r->n_alt == 0) return true;                                                                           // no VCF head
    if (!(bv_numfmt_f6_ok(r->qual) && bv_numfmt_f6_ok(r->qd) && bv_numfmt_f6_ok(r->var_sor) && bv_numfmt_f6_ok(r->var_fs))) return false;
    if (!(bv_numfmt_iod_ok(r->mq_ranksum) && bv_numfmt_iod_ok(r->rpr_ranksum) && bv_numfmt_iod_ok(r->bq_ranksum))) return false;
    for (uint32_t i = 0; i < r->n_alt; ++i)
        if (!(bv_numfmt_g6_ok(r->af[i]) && bv_numfmt_g6_ok(r->caf[i]))) return false;
    for (uint32_t j = 0; j < n_groups; ++j)
        for (uint32_t i = 0; i < g[j].n_alt; ++i)
            if (!bv_numfmt_g6_ok(g[j].af[i])) return false;
    return true;
}

// gt[4] of a line, one character per base A, C, G, T (bv_vcf_lines.gt): vcf_gt_codes()'s rule
BV_NUMFMT_FN uint8_t bv_rt_gt_code(const bv_site_result *r, uint8_t ref, uint32_t b) {
    const uint8_t up = (ref >= 'a' && ref <= 'z') ? (uint8_t)(ref - 32) : ref;
    const uint8_t base = (uint8_t)(0x54474341u >> (8u * b));  // "ACGT"[b]
    if (base == up) return '0';
    uint8_t c = '.';
    for (uint32_t i = 0, n = r->n_alt < BV_MAX_ALT ? r->n_alt : BV_MAX_ALT; i < n; ++i)
        if ((r->alt[i] & 3u) == b) c = (uint8_t)('1' + i);
    return c;
}
BV_NUMFMT_FN void bv_rt_gt_codes(const bv_site_result *r, uint8_t ref, uint8_t gt[4]) {
    for (uint32_t b = 0; b < 4u; ++b) gt[b] = bv_rt_gt_code(r, ref, b);
}

// What an item prints, for a message
inline const char *bv_rt_item_name(bool cvg, uint32_t idx) {
    static const char *const cvg_names[BV_RT_CVG_ITEMS] = {"CHROM", "POS", "REF", "Depth", "A", "C", "G", "T", "Indels", "FS", "SOR",
                                                           "Strand_Coverage", "Strand_Coverage", "Strand_Coverage", "Strand_Coverage", "end of line"};
    static const char *const vcf_names[BV_RT_VCF_GROUP0] = {"CHROM", "POS", "REF", "ALT", "QUAL", "CM_DP", "CM_AC", "CM_AC", "CM_AC", "CM_AF", "CM_AF", "CM_AF", "CM_CAF",
                                                            "CM_CAF", "CM_CAF", "MQRankSum", "ReadPosRankSum", "BaseQRankSum", "QD", "SOR", "FS", "SB_REF", "SB_REF", "SB_ALT", "SB_ALT"};
    if (cvg) return idx < BV_RT_CVG_ITEMS ? cvg_names[idx] : "?";
    return idx < BV_RT_VCF_GROUP0 ? vcf_names[idx] : "a group's AF";
}

#endif  // BV_RECORD_TEXT_CORE_H
