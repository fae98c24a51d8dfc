/*
 * basevar_amd_record_text.h -- whole VCF records and CVG rows written on the device from the engine's records
 * (INTEGRATION.md section 2l).
 *
 * basevar_amd_vcf.h expands a VCF record's sample columns on the device and takes the record's head (CHROM through FORMAT,
 * the "%f" / "%g" part) as host text.  Here the heads, and the rows of the CVG file, are formatted on the device too, from the
 * bv_site_result / bv_group_result records where they lie (basevar_amd/csrc/bv_record_text.hip).  The bytes are those of
 * host/vcf_emit.hpp's format_vcf_head and format_cvg_line and are defined at the head of
 * basevar_amd/csrc/bv_record_text_core.h; the numbers' text at the head of basevar_amd/csrc/bv_numfmt_core.h, which is exact
 * inside these domains and handles nothing outside them:
 *     "%f"  (QUAL, QD, the two FS, the two SOR)        finite, |v| < 2^63
 *     "%g"  (CM_AF, CM_CAF, the groups' AF)            +-0, or 2^-40 <= |v| < 999999.5
 *     (int) (the three rank sums)                      finite, |v| < 2^31
 * A record with a number outside them (AF = NaN of a site with a Q0 base) is the host's to format:
 * bv_record_text_on_device says which, and the calls take such lines as host text.
 *
 * Same conventions as basevar_amd_vcf.h: plain C, BV_OK or a negative status, bv_last_error() has the message.
 */
#ifndef BASEVAR_AMD_RECORD_TEXT_H
#define BASEVAR_AMD_RECORD_TEXT_H

#include "basevar_amd_vcf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BV_RECORD_TEXT_NAME_MAX 255u    /* bytes of CHROM and of a group name */
#define BV_RECORD_TEXT_INDEL_MAX 16384u /* bytes of a row's indel column; a longer one goes as host text */

/* n_lines lines, one per record.  Line k is made from records[k], groups[k * n_groups .. (k + 1) * n_groups), chrom,
 * pos[k], ref_char[k] (letter case kept) and the group names, in emission order. */
typedef struct bv_record_lines {
    const bv_site_result *records;   /* [n_lines], BV_MEM_HOST or BV_MEM_DEVICE (mem_kind)                                  */
    const bv_group_result *groups;   /* [n_lines][n_groups], same memory; NULL with n_groups == 0                          */
    const uint32_t *pos;             /* host [n_lines]                                                                     */
    const char *ref_char;            /* host [n_lines]                                                                     */
    const char *chrom;               /* host, chrom_len bytes, 1 .. BV_RECORD_TEXT_NAME_MAX                                */
    const char *group_names;         /* host: group j's name is group_names[group_name_off[j] .. group_name_off[j + 1])    */
    const uint32_t *group_name_off;  /* host [n_groups + 1], ascending                                                     */
    const char *host_text;           /* host: line k's text formatted by the caller, host_text[host_text_off[k] ..         */
    const uint64_t *host_text_off;   /*   host_text_off[k + 1]); zero length: format on the device.  Both NULL: no such line.
                                          bv_engine_cvg_format: the whole row with its '\n'.
                                          bv_engine_vcf_format_records: the head, CHROM through FORMAT; the sample columns
                                          and the '\n' follow it as behind a head formatted here                           */
    const char *indel;               /* bv_engine_cvg_format: row k's indel column is indel[indel_off[k] .. indel_off[k+1]), */
    const uint64_t *indel_off;       /*   host; zero length: "."; both NULL: every row "."                                 */
    const bv_slab *slab;             /* bv_engine_vcf_format_records: as bv_vcf_lines.slab                                 */
    const uint32_t *site;            /* bv_engine_vcf_format_records: host [n_lines], as bv_vcf_lines.site                 */
    uint32_t n_lines, n_groups, chrom_len;
    int32_t mem_kind;                /* of records and groups                                                              */
    uint32_t reserved_;              /* must be 0                                                                          */
} bv_record_lines;

/* Is every number that the record's VCF head and CVG row print inside its format's domain?  (Host memory; no engine.) */
int bv_record_text_on_device(const bv_site_result *record, const bv_group_result *groups, uint32_t n_groups);

/* Write the n_lines CVG rows back to back into a text buffer the engine owns: row k is text[line_off[k] .. line_off[k + 1]),
 * line_off [n_lines + 1] (host) is written for the caller.  A record with total_depth == 0 and no host text gives an empty row.
 * The text stays valid until the engine's next bv_engine_cvg_format.  Checked on the host before anything is launched,
 * BV_ERR_INVALID_ARG with line_off unwritten: NULL arguments, reserved_ != 0, mem_kind, offsets out of order, chrom_len or a
 * group name of 0 or more than BV_RECORD_TEXT_NAME_MAX bytes, an indel column beyond BV_RECORD_TEXT_INDEL_MAX, and of
 * BV_MEM_HOST records n_alt > 3 and an alt code above 3 (of BV_MEM_DEVICE records these are found by the first kernel and
 * refused the same way, before any text is written).  A line without host text whose record has a number outside the
 * domains above: BV_ERR_DATA, the message names the line and the field; no text is held and line_off stays unwritten.
 * n_lines == 0: BV_OK, line_off[0] = 0, an empty text.  Blocks until line_off is written and the text is complete. */
int bv_engine_cvg_format(bv_engine *e, const bv_record_lines *in, uint64_t *line_off, void *stream);
/* bv_engine_vcf_fetch's and bv_engine_vcf_deflate's contracts, for the text of the last bv_engine_cvg_format */
int bv_engine_cvg_fetch(bv_engine *e, void *dst, uint64_t dst_capacity, int dst_mem_kind, void *stream);
int bv_engine_cvg_deflate(bv_engine *e, const uint64_t *block_off, uint32_t n_blocks, int level, uint8_t *dst, uint64_t dst_capacity,
                          uint64_t *member_off, void *stream);

/* Write whole VCF lines: line k is its head, formatted on the device from record k (or the line's host text), and the sample
 * columns of row site[k] of `slab` exactly as bv_vcf_lines defines them, with the gt characters derived on the device from
 * ref_char[k] and the record's ALTs ('0' the REF base, '1' .. the ALT of that number, '.' otherwise).  A record with
 * n_alt == 0 and no host text gives an empty line.  The text is the one bv_engine_vcf_format leaves: bv_engine_vcf_fetch and
 * bv_engine_vcf_deflate take it from there.  The refusals are bv_engine_cvg_format's and, for slab and site,
 * bv_engine_vcf_format's. */
int bv_engine_vcf_format_records(bv_engine *e, const bv_record_lines *in, uint64_t *line_off, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BASEVAR_AMD_RECORD_TEXT_H */
