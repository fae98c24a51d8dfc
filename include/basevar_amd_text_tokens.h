/*
 * basevar_amd_text_tokens.h -- the '+SEQ' / '-SEQ' tokens of parsed batchfile rows, taken on the device (INTEGRATION.md
 * section 2n).
 *
 * bv_engine_text_parse and bv_engine_text_parse_bgzf mark a row whose Readbases column holds such a token (BV_TEXT_INDEL) and
 * leave the tokens to the host: bv_engine_text_rows_fetch brings every marked row back whole.  With the mode of this header on,
 * a parse also lists the tokens on the device -- bv_pileup_token descriptors over a text the engine owns, as the pileup lists
 * its own --, ready for bv_engine_indel_tally; bv_engine_text_heads_fetch then brings back no more of a marked row than of any
 * other.  What the list holds is defined at the head of basevar_amd/csrc/bv_text_tokens_core.h: the tokens of field 5 that begin
 * with '+' or '-', of the rows of positions whose final row_state is 0, position ascending, then file, then sample;
 * pos = the position's index in the batch, sample = the sample's index in the position's row of all files.  The tokens of a
 * BV_TEXT_HOST position are the host reader's, never the list's.
 *
 * Same conventions as basevar_amd_vcf.h: plain C, BV_OK or a negative status, bv_last_error() has the message.  With the mode
 * off (the default) every call of the other headers does and launches what it did without this one.
 */
#ifndef BASEVAR_AMD_TEXT_TOKENS_H
#define BASEVAR_AMD_TEXT_TOKENS_H

#include "basevar_amd_indel.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The mode for the engine's later parses: on != 0 lists the tokens.  Turning it off keeps the last list (it is handed out
 * again once the mode is back on, if no parse came between). */
int bv_engine_text_tokens_enable(bv_engine *e, int on);

/* The tokens of the engine's last parse where they lie: device pointers, counts, BV_MEM_DEVICE; ready for
 * bv_engine_indel_tally with key[k] = a position's index.  text_off is ascending and without overlap.  n_tokens == 0 is a
 * valid answer (NULL pointers).  Valid through bv_engine_text_submit and until the engine's next parse.
 * BV_ERR_INVALID_ARG, nothing written: a NULL argument, the mode off, no completed parse since the mode was turned on. */
int bv_engine_text_tokens(bv_engine *e, bv_indel_tokens *out);

/* The same list copied to host memory: descriptors with text_off counted in a text without gaps, and that text.  *n_tokens
 * and *text_bytes are always written (unless they are NULL, or bv_engine_text_tokens would refuse); with a capacity below
 * them BV_ERR_INVALID_ARG, nothing else is written and the call may be repeated.  Blocks until the buffers are written. */
int bv_engine_text_tokens_fetch(bv_engine *e, bv_pileup_token *tokens, uint64_t tokens_capacity, uint8_t *text, uint64_t text_capacity,
                                uint64_t *n_tokens, uint64_t *text_bytes, void *stream);

/* bv_engine_text_rows_fetch's contract (include/basevar_amd_bgzf.h), except that a BV_TEXT_INDEL row is cut like any other
 * parsed row: file 0's through its fourth tab, nothing of the others.  BV_TEXT_HOST positions still come whole, skipped ones
 * not at all.  The marked rows' tokens do not come with it, so besides bv_engine_text_rows_fetch's refusals it is
 * BV_ERR_INVALID_ARG, nothing written, wherever bv_engine_text_tokens would refuse: the mode off, or a parse made without it. */
int bv_engine_text_heads_fetch(bv_engine *e, void *buf, uint64_t capacity, uint64_t *row_off, uint64_t *bytes_needed, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BASEVAR_AMD_TEXT_TOKENS_H */
