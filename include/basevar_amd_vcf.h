/*
 * basevar_amd_vcf.h -- the per-sample GT:AB:SO:BP columns of VCF records written on the device, straight into BGZF members
 * (INTEGRATION.md section 2h).
 *
 * A VCF record of the reference (_out_vcf_line, src/basetype_caller.cpp:1103-1209) is a head of a few hundred bytes -- CHROM
 * through FORMAT, "%f" / "%g" formatting that these calls take as host text (basevar_amd_record_text.h formats it on the device
 * too) -- and one column per sample whose bytes depend only on the
 * sample's cell and phred bytes, four characters per line and a table of 256 strings.  Here those columns are expanded from
 * the planes where they lie in device memory (basevar_amd/csrc/bv_vcf.hip; the bytes are defined at the head of
 * basevar_amd/csrc/bv_vcf_core.h) and deflated from there (basevar_amd/csrc/bv_deflate.hip).
 *
 * Same conventions as basevar_amd_bgzf.h: plain C, BV_OK or a negative status, bv_last_error() has the message.
 */
#ifndef BASEVAR_AMD_VCF_H
#define BASEVAR_AMD_VCF_H

#include "basevar_amd_bgzf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n_lines VCF records.  Line k is
 *   head[head_off[k] .. head_off[k + 1])  then, for every sample s of row site[k],  '\t' tok(cell[s], phred[s])  then '\n'
 *   tok(c, q) = "./."                                                          if c & BV_CELL_NOCALL
 *             = G:B:S:P  with  G = "0/." if gt[k][c & 3] == '0', else "./" and the character gt[k][c & 3],
 *                              B = "ACGT"[c & 3],  S = '-' if c & BV_CELL_REV else '+',
 *                              P = "%f" of 1.0 - exp(q * -0.23025850929940458) (8 characters for every q)
 * so line k has |head_k| + 4 * n_samples + 13 * (covered samples of the row) + 1 bytes. */
typedef struct bv_vcf_lines {
    const bv_slab *slab;      /* rows are read from its base_strand and qual planes only (BV_MEM_HOST or BV_MEM_DEVICE);
                                 NULL: the rows kept by this engine's last bv_engine_text_submit, in record order        */
    const uint32_t *site;     /* [n_lines] row of the slab / record index; any order, repeats allowed                    */
    const char *head;         /* host: line k's text before its first sample column is head[head_off[k] .. head_off[k+1]) */
    const uint64_t *head_off; /* [n_lines + 1], ascending                                                                */
    const uint8_t *gt;        /* [n_lines][4]: one character per base A, C, G, T: '0' the REF base, '.' no allele of the
                                 record, '1' .. '4' the record's ALT of that number                                      */
    uint32_t n_lines, reserved_; /* reserved_ must be 0 */
} bv_vcf_lines;

/* Format the lines back to back into a text buffer the engine owns: line k is text[line_off[k] .. line_off[k + 1]),
 * line_off[0] = 0; line_off[n_lines + 1] (host) is written for the caller.  The text stays in device memory and stays valid
 * until the engine's next bv_engine_vcf_format or its next text parse.  Of a BV_MEM_HOST slab the named rows' two planes are
 * copied up, nothing else; cells at pitch positions at or beyond n_samples are never read into the output.
 * Everything is checked on the host before anything is launched; BV_ERR_INVALID_ARG, with line_off unwritten, for NULL
 * arguments, reserved_ != 0, head_off out of order, a gt byte that is none of the characters above, a site beyond the slab's
 * rows (slab == NULL: beyond the record count of the last bv_engine_text_submit, or no such submit before this call), and for
 * a slab that bv_engine_submit would refuse for its base_strand and qual planes (n_samples == 0, pitch below n_samples or no
 * multiple of 16, a NULL or misaligned plane, mem_kind, unknown layout bits).  n_lines == 0: BV_OK, line_off[0] = 0, and the
 * engine then holds an empty text.  Blocks until line_off is written and the text is complete.
 * `stream`: a hipStream_t, or NULL for the engine's own; device planes must be complete on it. */
int bv_engine_vcf_format(bv_engine *e, const bv_vcf_lines *lines, uint64_t *line_off, void *stream);

/* Copy the formatted text, line_off[n_lines] bytes, to dst: a host or a device buffer (dst_mem_kind) of dst_capacity bytes.
 * BV_ERR_INVALID_ARG, and nothing written, without a bv_engine_vcf_format before it, for a NULL dst where there is text, a
 * dst_mem_kind that is neither BV_MEM_HOST nor BV_MEM_DEVICE, or a dst_capacity below the text's bytes.  Blocks until dst is
 * written. */
int bv_engine_vcf_fetch(bv_engine *e, void *dst, uint64_t dst_capacity, int dst_mem_kind, void *stream);

/* bv_engine_bgzf_deflate_level (basevar_amd_bgzf.h) with the formatted text as its text: block k is text[block_off[k] ..
 * block_off[k + 1]), of 1 to 65,280 bytes, and becomes one whole BGZF member at dst + member_off[k] (host memory) whose bytes
 * depend on the block's text and the level alone -- they are the bytes that call writes for the fetched text.  member_off
 * [n_blocks + 1] is written for the caller; dst_capacity >= the text's bytes + 31 * n_blocks.  The refusals are that call's,
 * and BV_ERR_INVALID_ARG without a bv_engine_vcf_format before it.  Blocks until dst is written. */
int bv_engine_vcf_deflate(bv_engine *e, const uint64_t *block_off, uint32_t n_blocks, int level, uint8_t *dst, uint64_t dst_capacity,
                          uint64_t *member_off, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BASEVAR_AMD_VCF_H */
