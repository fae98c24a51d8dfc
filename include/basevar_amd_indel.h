/*
 * basevar_amd_indel.h -- the CVG row's indel column tallied on the device.
 *
 * basevar_amd_record_text.h writes the CVG rows on the device and takes column 9, the sorted "TOKEN|count" tally of the row's
 * indel tokens, as host text (bv_record_lines.indel).  Here the column is made on the device too, from the tokens where they
 * lie -- the last pileup's, or tokens the caller hands in --, one wave per row (basevar_amd/csrc/bv_indel_tally.hip), and
 * bv_engine_cvg_format_tallied writes the rows around it.  The bytes are those of host/vcf_emit.hpp's indel_string and are
 * defined at the head of basevar_amd/csrc/bv_indel_tally_core.h, with the domain: a row of at most bv_indel_row_tokens_max()
 * tokens whose column has at most BV_RECORD_TEXT_INDEL_MAX bytes.  A row outside it is flagged and left to the caller.
 *
 * Same conventions as basevar_amd_vcf.h: plain C, BV_OK or a negative status, bv_last_error() has the message.
 */
#ifndef BASEVAR_AMD_INDEL_H
#define BASEVAR_AMD_INDEL_H

#include "basevar_amd_pileup.h"
#include "basevar_amd_record_text.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bv_indel_tokens {      /* tokens ascending by pos; the order inside one pos is free */
    const bv_pileup_token *tokens;    /* the sample field is not read */
    const uint8_t *text;
    uint64_t n_tokens, text_bytes;
    int32_t mem_kind;                 /* BV_MEM_HOST | BV_MEM_DEVICE, of both */
    uint32_t reserved_;               /* must be 0 */
} bv_indel_tokens;

/* The most tokens a row may have, kept by the filter or not. */
uint32_t bv_indel_row_tokens_max(void);

/* Tally n rows: row k's tokens are those whose pos equals key[k] (host [n], any order; keys may repeat and may match no
 * token; tokens whose pos matches no key are skipped).  Column k is text[col_off[k] .. col_off[k + 1]) of a text the engine
 * owns, col_off [n + 1] and row_flag [n] (host) are written for the caller: row_flag[k] == 0 the column is tallied here (zero
 * length: no class, the row prints "."), 1 the row is outside the domain, its column has zero length and is the caller's.
 * tok == NULL: the tokens of the engine's last bv_engine_pileup / bv_engine_pileup_bgzf, read where they lie.
 * BV_ERR_INVALID_ARG, nothing written and the last tally still held: NULL arguments, reserved_ != 0, a bad mem_kind,
 * tok == NULL without a completed pileup, tokens whose pos descends or whose text runs beyond text_bytes (host tokens: found
 * before anything is launched; device tokens: found by the first kernel, before any text is written).  BV_ERR_TOO_LARGE: 2^26
 * rows or more.  n == 0: BV_OK, col_off[0] = 0.  Blocks until col_off and row_flag are written and the text is complete; the
 * text stays valid until the engine's next tally.  `stream`: a hipStream_t, or NULL for the engine's own; device tokens must
 * be complete on it. */
int bv_engine_indel_tally(bv_engine *e, const bv_indel_tokens *tok, const uint32_t *key, uint32_t n, uint64_t *col_off, uint8_t *row_flag,
                          void *stream);
/* bv_engine_cvg_fetch's contract, for the text of the last bv_engine_indel_tally */
int bv_engine_indel_fetch(bv_engine *e, void *dst, uint64_t dst_capacity, int dst_mem_kind, void *stream);

/* bv_engine_cvg_format with row k's indel column taken from column k of the engine's last tally, where it lies.  Besides
 * bv_engine_cvg_format's refusals, BV_ERR_INVALID_ARG: in->indel / in->indel_off not NULL, no tally or one whose n differs
 * from in->n_lines, a flagged row that brings no host text. */
int bv_engine_cvg_format_tallied(bv_engine *e, const bv_record_lines *in, uint64_t *line_off, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BASEVAR_AMD_INDEL_H */
