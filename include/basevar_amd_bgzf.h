/*
 * basevar_amd_bgzf.h -- BGZF members inflated and written (section 2g) on the device.
 *
 * The reference reads its batchfiles through htslib's BGZF reader (src/basetype_caller.cpp:428 requires that format): a
 * chain of independent gzip members of at most 64 KiB of text each, inflated one after the other by zlib on the host.  Here
 * the members go to the device as they lie in the file and one wave inflates each of them (basevar_amd/csrc/bv_inflate.hip).
 *
 * Same conventions as basevar_amd.h: plain C, BV_OK or a negative status, bv_last_error() has the message.
 */
#ifndef BASEVAR_AMD_BGZF_H
#define BASEVAR_AMD_BGZF_H

#include "basevar_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one more bv_status value: the input data, not the call, is wrong (a BGZF member that does not inflate to what it states) */
#define BV_ERR_DATA (-6)

/* what became of one member */
typedef enum bv_bgzf_status {
    BV_BGZF_OK = 0,
    BV_BGZF_BAD_HEADER = 1,  /* not a gzip member with the 'BC' extra field, or its length there is not the packing's */
    BV_BGZF_BAD_DEFLATE = 2, /* the DEFLATE stream is invalid (what zlib calls a data error)                          */
    BV_BGZF_BAD_SIZE = 3,    /* the stream ends before ISIZE bytes, or holds more; ISIZE above 65,536                 */
    BV_BGZF_BAD_CRC = 4      /* ISIZE bytes came out and their CRC32 is not the member's                              */
} bv_bgzf_status;

/* n_members whole BGZF members in host memory, as they lie in a file: member k is data[member_off[k] .. member_off[k + 1])
 * (18-byte header with the 'BC' extra field, DEFLATE payload, CRC32, ISIZE).  They need not be neighbours in `data`. */
typedef struct bv_bgzf_members {
    const uint8_t *data;
    const uint64_t *member_off; /* [n_members + 1], ascending */
    uint64_t data_bytes;        /* size of `data`: every offset is <= it */
    uint32_t n_members;
    uint32_t reserved_;         /* must be 0 */
} bv_bgzf_members;

/* Inflate the members.  Member k's bytes land at dst + dst_off[k], where dst_off[0] = 0 and dst_off[k + 1] - dst_off[k] is
 * member k's ISIZE field (0 for a member with a bad header or an ISIZE above 65,536, which no BGZF member has): dst_off
 * [n_members + 1] is written for the caller.  dst is a host or a device buffer (mem_kind) of dst_capacity bytes;
 * status[n_members] (host) receives a bv_bgzf_status per member.  A member whose status is not BV_BGZF_OK leaves its range of
 * dst unspecified and touches nothing outside it.  Per member the device checks every read against the payload's length,
 * every write against ISIZE, the inflated size against ISIZE and the CRC32 of the inflated bytes against the member's.
 * Payload bytes behind the final DEFLATE block are ignored, as zlib's inflate() ignores them.
 * Returns BV_OK when the call ran, whatever the statuses; BV_ERR_INVALID_ARG for NULL arguments, offsets out of order or
 * beyond data_bytes, a member shorter than 26 bytes or longer than 65,536, mem_kind neither BV_MEM_HOST nor BV_MEM_DEVICE, or
 * dst_capacity < dst_off[n_members] (dst_off is written even then, so the caller learns the size).  Any number of members:
 * the engine stages the compressed bytes in chunks through pinned memory.  Blocks until dst and status are written.
 * `stream`: a hipStream_t, or NULL for the engine's own. */
int bv_engine_bgzf_inflate(bv_engine *e, const bv_bgzf_members *members, void *dst, uint64_t dst_capacity, int mem_kind,
                           uint64_t *dst_off, uint8_t *status, void *stream);

/* ---- batchfile rows that are still compressed: bv_engine_text_parse (basevar_amd.h) without the host's inflate, line split
 * and row packing.  For each of n_files batchfiles a RUN of consecutive whole members: file f's run is members
 * file_member[f] .. file_member[f + 1] - 1 of (data, member_off), packed as in bv_bgzf_members.  File f's first row starts
 * skip_bytes[f] inflated bytes into its run and then skip_lines[f] further lines (the header lines of a file's first run: a
 * reader knows their number, not their bytes). */
typedef struct bv_bgzf_rows {
    const uint8_t *data;
    const uint64_t *member_off;   /* [file_member[n_files] + 1], ascending */
    uint64_t data_bytes;
    const uint32_t *file_member;  /* [n_files + 1], ascending, file_member[0] = 0 */
    const uint32_t *file_samples; /* [n_files] samples per batchfile, each > 0 */
    const uint64_t *skip_bytes;   /* [n_files], each <= the bytes the file's run inflates to */
    const uint32_t *skip_lines;   /* [n_files] */
    uint32_t n_files;
    uint32_t max_positions;       /* > 0: take at most this many positions */
    uint32_t at_end;              /* 1: every run reaches the end of its file, so a last line without '\n' is a line */
    uint32_t reserved_;           /* must be 0 */
} bv_bgzf_rows;

/* where file f's next run starts: the first line not taken begins `offset` inflated bytes into member `member` of the run
 * this call was given (member = the run's member count, offset = 0: everything was taken) */
typedef struct bv_bgzf_cursor {
    uint32_t member;
    uint32_t offset;
} bv_bgzf_cursor;

/* Stateless.  The device inflates every run (file f's members back to back, so a row may span members), finds the line ends
 * and takes *n_positions = min(max_positions, cfg.max_sites, min over f of file f's complete lines behind the skip).  Row
 * (p, f) is file f's p-th line behind the skip.  The rows are then parsed exactly as bv_engine_text_parse parses them: the
 * same strict form, the same row_state values (written for the first *n_positions * n_files rows; give room for
 * min(max_positions, cfg.max_sites) * n_files), the same planes, and bv_engine_text_submit runs unchanged behind it (one
 * submit per parse; this call counts as the parse).  cursor[n_files] is written for the caller.  *n_positions = 0 (some file
 * has no complete line behind its skip): nothing is parsed and nothing is consumed -- cursor[f] is the place of skip_bytes[f]
 * itself, and the skip_lines[f] lines behind it are still to be skipped: the caller comes back with longer runs and the same
 * skip_lines (or, with at_end = 1, has reached the end of the files).
 * Any member whose status is not BV_BGZF_OK: nothing is parsed, the call returns BV_ERR_DATA and bv_last_error() names the
 * file index, the member's index inside its run and the status; the caller re-reads with its host reader.
 * BV_ERR_INVALID_ARG as for bv_engine_text_parse and bv_engine_bgzf_inflate, and for a skip_bytes beyond its run. */
int bv_engine_text_parse_bgzf(bv_engine *e, const bv_bgzf_rows *rows, const uint8_t *group_id, uint32_t n_groups, uint32_t *n_positions,
                              uint8_t *row_state, bv_bgzf_cursor *cursor, void *stream);

/* The text the host still needs after bv_engine_text_parse_bgzf (valid until the engine's next parse): one call gathers into
 * buf, without line breaks, row (p, 0) through its fourth tab (CHROM, POS, REF, Depth) for every position not skipped, every
 * row of a BV_TEXT_HOST position and every BV_TEXT_INDEL row whole, and nothing of any other row.  Row r = p * n_files + f is
 * buf[row_off[r] .. row_off[r + 1]); row_off has n_positions * n_files + 1 entries.  *bytes_needed is always written; if
 * capacity is smaller, nothing else is written, the call returns BV_OK and may be repeated with more room. */
int bv_engine_text_rows_fetch(bv_engine *e, uint8_t *buf, uint64_t capacity, uint64_t *row_off, uint64_t *bytes_needed, void *stream);

/* ---- the way back: text deflated into BGZF members on the device (basevar_amd/csrc/bv_deflate.hip).
 * Block k is text[block_off[k] .. block_off[k + 1]), of 1 to 65,280 (0xff00) bytes; `text` is a host or a device buffer
 * (text_mem_kind) of text_bytes bytes.  Every block becomes one whole BGZF member -- the 18-byte header with the 'BC' field,
 * one raw DEFLATE stream (LZ77 with a 32 KiB window and the fixed Huffman codes, or a stored block where that is not smaller),
 * CRC32, ISIZE -- of at most the block's bytes + 31.  The bytes of a member depend on the block's text and on nothing else.
 * Member k lands at dst + member_off[k] (host memory), member_off[0] = 0; member_off[n_blocks + 1] is written for the caller.
 * No end-of-file marker is written: that stays with the writer.
 * Returns BV_ERR_INVALID_ARG for NULL arguments, a block of 0 bytes or of more than 65,280, offsets out of order or beyond
 * text_bytes, text_mem_kind neither BV_MEM_HOST nor BV_MEM_DEVICE, or dst_capacity < text_bytes + 31 * n_blocks (the worst
 * case, known before the call).  n_blocks = 0: BV_OK, member_off[0] alone is written.  Any number of blocks: the engine stages
 * them in chunks.  Blocks until dst is written.  `stream`: a hipStream_t, or NULL for the engine's own; text in device memory
 * must be complete on it. */
int bv_engine_bgzf_deflate(bv_engine *e, const void *text, uint64_t text_bytes, int text_mem_kind, const uint64_t *block_off,
                           uint32_t n_blocks, uint8_t *dst, uint64_t dst_capacity, uint64_t *member_off, void *stream);

/* The same with a level.  The contract, the refusals and the bound of text + 31 bytes a member are bv_engine_bgzf_deflate's;
 * any other level is BV_ERR_INVALID_ARG, and nothing is written.
 *   BV_DEFLATE_FAST   what bv_engine_bgzf_deflate writes, byte for byte: one candidate per position from a 4-byte hash, the
 *                     fixed Huffman codes.  About twice zlib level 6's size on VCF text.
 *   BV_DEFLATE_SMALL  opt-in: smaller files for more seconds.  Three 12-bit head tables for the 4-, 8- and 16-byte gram at
 *                     every position; the match at p is the first of 16, 8, 4 whose candidate exists, lies within 32,768 and
 *                     agrees for at least the gram's bytes; greedy.  The block is written with dynamic Huffman codes (lengths
 *                     by two-queue Huffman over the symbols sorted by (count, symbol), counts halved while the tree is deeper
 *                     than 15 bits, or 7 for the code-length alphabet; the header spelled greedily with 16, 17, 18), with the
 *                     fixed codes or stored, whichever is smallest (fixed on a tie with dynamic, stored on a tie with
 *                     either).  The definition stands at the head of basevar_amd/csrc/bv_deflate_small_core.h; a member's
 *                     bytes depend on its text alone.  Sizes: 1.03 to 1.07 times zlib level 6 on VCF, CVG and batchfile
 *                     text.  The kernel holds 103 KiB of LDS, so ONE workgroup runs per CU where BV_DEFLATE_FAST has two,
 *                     and the first call at this level allocates 4 bytes of device memory per byte of a staged chunk's
 *                     text for the tokens.  Times: INTEGRATION.md section 2g. */
#define BV_DEFLATE_FAST 0
#define BV_DEFLATE_SMALL 1
int bv_engine_bgzf_deflate_level(bv_engine *e, const void *text, uint64_t text_bytes, int text_mem_kind, const uint64_t *block_off,
                                 uint32_t n_blocks, int level, uint8_t *dst, uint64_t dst_capacity, uint64_t *member_off, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BASEVAR_AMD_BGZF_H */
