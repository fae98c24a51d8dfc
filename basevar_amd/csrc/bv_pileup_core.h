// bv_pileup_core.h -- the pileup of BAM records into first-read-wins cells (bv_engine_pileup, include/basevar_amd_pileup.h), as
// inline functions that the device kernels (bv_pileup.hip) and a plain g++ harness (tests/cpp/pileup_core_check.cpp) both compile,
// as bv_vcf_core.h and bv_inflate_core.h are.
//
// THE RESULT, defined without reference to lanes.  It restates on RAW BAM RECORD BYTES (SAM/BAM specification 4.2: a block_size
// word, then the block) what host/bamio.hpp's BamFile::next() and host/pileup.hpp's pileup_one_sample / pileup_claim_read do on
// decoded records; the tests hold this file to them byte for byte.
//
//   A sample's records arrive as RUNS: byte ranges of the uncompressed BAM stream that hold whole records back to back.  Taken
//   in order, a sample's runs are its file order.  For every record, in that order:
//     decode      block_size >= 32, the record inside its run, 32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq inside the
//                 block; else the sample FAILS with a status (BV_PILEUP_BAD_*), whatever the record's other fields say
//     next()      tid != the query's: smaller -> skip, larger or negative -> BREAK;  pos >= q_end -> BREAK;  end_pos <= q_beg ->
//                 skip, with q_beg = lo - 1, q_end = hi, lo / hi the window -/+ BV_PILEUP_PAD (lo at least 1)
//     filter      mapq below the threshold, duplicate or QC-fail of a mapped read -> skip;  with first / last the read's 1-based
//                 span (0 / -1 for an unmapped read):  gb > last -> skip;  ge < first -> BREAK;  end + 1 < first -> BREAK;
//                 beg > last + 1 -> skip, where [gb, ge] is the 500 kb step of the window (bv_pileup_step)
//     claim       the CIGAR walk below
//   The stored rank SATURATES at 65,535 (bv_pileup_rank): a claimed cell's rank is never zero, whatever the read's length, so
//   "claimed <=> rank != 0" holds and the depth of a row is the number of its cells of rank != 0.
//   BREAK: every later record of that sample is ignored (not even decoded), whichever run it lies in.
//
//   The walk keeps rpos (0-based reference position of the next reference base, 64-bit) and qpos (query bases consumed, 32-bit and
//   wrapping as the host's is).  A cell (position p, this sample) is CLAIMED by the first attempt on it, in record order and within
//   a record in CIGAR order, if beg <= p <= end.  Per operation of length len:
//     M = X   base i (0 <= i < len) lies at p = rpos + i + 1.  The bases with gb <= p <= ge are looked at: query index qpos + i must be
//             below l_seq (else BV_PILEUP_BAD_QUERY), its nibble one of A C G T N (else BV_PILEUP_BAD_BASE: the host's "[ERROR] Why
//             dose the size of aligned base is not 1?", raised for such a base anywhere in the step, claimed or not); then an
//             attempt on p with (code | strand, qual[q], mapq, min(q + 1, 65535)).  Of one operation BAD_QUERY is reported before
//             BAD_BASE.  The walk ends behind the operation if it reaches beyond ge (len > 0 and rpos + len > ge).
//     I D     tested on the UN-anchored position rpos + 1: beyond ge the walk ends; if gb <= rpos + 1 and rpos >= 1, one attempt on
//             p = rpos (the base to the left) with (BV_CELL_INS / _DEL | strand, mean_q, mapq, min(qpos + 1, 65535)), mean_q =
//             (uint8_t)(int)(sum of qual / l_seq), 255 for an empty read.  So an indel is refused when the same read's own match
//             holds its anchor, and an I and then a D at one break point both anchor at the same position.  A claimed indel has a
//             TOKEN: '+' or '-', the anchor's reference base ref[rpos - 1], then the inserted read letters seq[qpos, qpos + len)
//             clipped to l_seq (A C G T N, ' ' for any other nibble) or the deleted reference bases ref[rpos, rpos + len) clipped
//             to the reference's end, both as std::string::substr clips.  rpos - 1 beyond the reference: BV_PILEUP_BAD_REF; qpos
//             beyond l_seq for an insertion: BV_PILEUP_BAD_QUERY (where substr throws).
//     N       beyond ge (rpos + 1 > ge) the walk ends; rpos += len.       S P   the same test; qpos += len.       H, 9-15: nothing.
//
// Every index the host takes without a check is a status here; nothing is read outside a run or the reference.
#ifndef BV_PILEUP_CORE_H
#define BV_PILEUP_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define BV_PU_FN __host__ __device__ inline
#else
#define BV_PU_FN inline
#endif

#define BV_PILEUP_STEP 500000u  // host/pileup.hpp: PILEUP_STEP
#define BV_PILEUP_PAD 200u      // PILEUP_PAD
#define BV_PILEUP_MAX_ROWS BV_PILEUP_STEP  // a window never crosses a step: one `seen` bit a row, 62,500 bytes

// cell codes (include/basevar_amd.h: BV_CELL_*), restated so that this file stands alone
#define BV_PU_CELL_REV 0x04u
#define BV_PU_CELL_N 0x08u
#define BV_PU_CELL_INS 0x09u
#define BV_PU_CELL_DEL 0x0Au
#define BV_PU_CELL_BAD 0xFFu  // bv_pileup_base_cell of a nibble that is none of A C G T N

// status of a sample
enum {
    BV_PILEUP_OK = 0,
    BV_PILEUP_BAD_BLOCK = 1,    // block_size below 32
    BV_PILEUP_BAD_RUN = 2,      // a record overruns its run
    BV_PILEUP_BAD_LENGTHS = 3,  // n_cigar / l_seq / l_read_name beyond the block
    BV_PILEUP_BAD_QUERY = 4,    // the CIGAR consumes more query bases than l_seq
    BV_PILEUP_BAD_REF = 5,      // an indel's anchor lies outside the reference sequence
    BV_PILEUP_BAD_BASE = 6      // a match base that is none of A C G T N
};

// what becomes of a decoded record
enum { BV_PILEUP_CLAIM = 0, BV_PILEUP_SKIP = 1, BV_PILEUP_BREAK = 2 };

struct BvPileupQuery {
    int32_t tid;
    uint32_t beg, end;     // the window, 1-based inclusive
    uint32_t gb, ge;       // its step
    int32_t mapq_thd;
    uint64_t ref_len;
};

struct BvPileupRec {
    int32_t tid, pos;
    uint32_t mapq, flag, n_cigar, l_seq;
    uint64_t cigar_at;                   // byte offset in the run; the packed bases and the qualities follow the CIGAR
    uint64_t next_at;                    // the record behind it
    int64_t end_pos;                     // bam_endpos
};

// one indel token as the library hands it out
struct BvPileupToken {
    uint32_t pos, sample;
    uint64_t text_off;
    uint32_t text_len, reserved_;
};

// per sample: how its walk ended and what its tokens take
struct BvPileupSample {
    uint64_t at;          // failed: byte offset of the record in its run
    uint64_t text_bytes;  // of its tokens
    uint32_t status;      // BV_PILEUP_*
    uint32_t run;         // failed: the run
    uint32_t n_tokens;
    uint32_t reserved_;
};

BV_PU_FN uint32_t bv_pileup_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
BV_PU_FN uint32_t bv_pileup_u32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// The step [gb, ge] of the grid laid out from region_beg that holds `beg`, as pileup_tile computes it; false if [beg, end] is no
// window of it (pileup_tile's own refusal, and the arguments it takes on trust)
BV_PU_FN bool bv_pileup_step(uint32_t region_beg, uint32_t region_end, uint32_t beg, uint32_t end, uint32_t *gb, uint32_t *ge) {
    if (region_beg == 0 || beg < region_beg || end < beg || end > region_end) return false;
    const uint64_t b = (uint64_t)region_beg + (uint64_t)(beg - region_beg) / BV_PILEUP_STEP * BV_PILEUP_STEP;
    const uint64_t e = b + BV_PILEUP_STEP - 1 < region_end ? b + BV_PILEUP_STEP - 1 : region_end;
    *gb = (uint32_t)b;
    *ge = (uint32_t)e;
    return end <= e;
}

BV_PU_FN void bv_pileup_query(int32_t tid, uint32_t beg, uint32_t end, uint32_t gb, uint32_t ge, int32_t mapq_thd, uint64_t ref_len,
                              BvPileupQuery *q) {
    q->tid = tid; q->beg = beg; q->end = end; q->gb = gb; q->ge = ge;
    q->mapq_thd = mapq_thd;
    q->ref_len = ref_len;
}

BV_PU_FN bool bv_pileup_op_is_match(uint32_t op) { return op == 0u || op == 7u || op == 8u; }

// The record at run[at ..]: BV_PILEUP_OK and *r, or why it cannot be read.  at < run_bytes.
BV_PU_FN uint32_t bv_pileup_record(const uint8_t *run, uint64_t run_bytes, uint64_t at, BvPileupRec *r) {
    if (run_bytes - at < 4u) return BV_PILEUP_BAD_RUN;
    const uint64_t block_size = bv_pileup_u32(run + at);
    if (block_size < 32u) return BV_PILEUP_BAD_BLOCK;
    if (run_bytes - at - 4u < block_size) return BV_PILEUP_BAD_RUN;
    const uint8_t *p = run + at + 4u;
    r->tid = (int32_t)bv_pileup_u32(p);
    r->pos = (int32_t)bv_pileup_u32(p + 4);
    const uint64_t l_read_name = p[8];
    r->mapq = p[9];
    r->n_cigar = bv_pileup_u16(p + 12);
    r->flag = bv_pileup_u16(p + 14);
    r->l_seq = bv_pileup_u32(p + 16);
    const uint64_t o = 32u + l_read_name;
    if (o + 4ull * r->n_cigar + ((uint64_t)r->l_seq + 1u) / 2u + r->l_seq > block_size) return BV_PILEUP_BAD_LENGTHS;
    r->cigar_at = at + 4u + o;
    r->next_at = at + 4u + block_size;
    int64_t rlen = 0;
    for (uint32_t c = 0; c < r->n_cigar; ++c) {
        const uint32_t cig = bv_pileup_u32(run + r->cigar_at + 4ull * c), op = cig & 15u;
        if (bv_pileup_op_is_match(op) || op == 2u || op == 3u) rlen += cig >> 4;
    }
    r->end_pos = (int64_t)r->pos + (rlen ? rlen : 1);
    return BV_PILEUP_OK;
}

BV_PU_FN uint64_t bv_pileup_seq_at(const BvPileupRec *r) { return r->cigar_at + 4ull * r->n_cigar; }
BV_PU_FN uint64_t bv_pileup_qual_at(const BvPileupRec *r) { return bv_pileup_seq_at(r) + ((uint64_t)r->l_seq + 1u) / 2u; }

BV_PU_FN uint32_t bv_pileup_filter(const BvPileupQuery *q, const BvPileupRec *r) {
    // BamFile::fetch's [q_beg, q_end), 0-based: the window -/+ BV_PILEUP_PAD as pileup_one_sample asks for it
    const int64_t q_beg = (int64_t)(q->beg > BV_PILEUP_PAD ? q->beg - BV_PILEUP_PAD : 1u) - 1, q_end = (int64_t)q->end + BV_PILEUP_PAD;
    if (r->tid != q->tid) return (r->tid > q->tid || r->tid < 0) ? BV_PILEUP_BREAK : BV_PILEUP_SKIP;
    if ((int64_t)r->pos >= q_end) return BV_PILEUP_BREAK;
    if (r->end_pos <= q_beg) return BV_PILEUP_SKIP;
    const bool mapped = !(r->flag & 4u);
    if ((int32_t)r->mapq < q->mapq_thd || (mapped && (r->flag & (1024u | 512u)))) return BV_PILEUP_SKIP;
    const int64_t first = (mapped ? (int64_t)r->pos : -1) + 1, last = mapped ? r->end_pos : -1;
    if ((int64_t)q->gb > last) return BV_PILEUP_SKIP;
    if ((int64_t)q->ge < first) return BV_PILEUP_BREAK;
    if ((int64_t)q->end + 1 < first) return BV_PILEUP_BREAK;
    if ((int64_t)q->beg > last + 1) return BV_PILEUP_SKIP;
    return BV_PILEUP_CLAIM;
}

BV_PU_FN uint32_t bv_pileup_nibble(const uint8_t *seq, uint32_t q) { return (seq[q >> 1] >> ((~q & 1u) << 2)) & 15u; }
// a match base's cell code: A C G T, BV_CELL_N, or BV_PU_CELL_BAD
BV_PU_FN uint32_t bv_pileup_base_cell(uint32_t nibble) {
    return nibble == 1u ? 0u : nibble == 2u ? 1u : nibble == 4u ? 2u : nibble == 8u ? 3u : nibble == 15u ? BV_PU_CELL_N : BV_PU_CELL_BAD;
}
// the letter BamFile decodes a nibble to
BV_PU_FN uint8_t bv_pileup_letter(uint32_t nibble) {
    return nibble == 1u ? 'A' : nibble == 2u ? 'C' : nibble == 4u ? 'G' : nibble == 8u ? 'T' : nibble == 15u ? 'N' : ' ';
}
// (uint8_t)(int)mean_qqual() of a mapped read.  The quotient is exact in integers (the sum is below 2^40: the double quotient of
// two such integers never rounds up to the next whole number) and at most 255: eight compare steps instead of a 64-bit division.
BV_PU_FN uint8_t bv_pileup_mean_q(uint64_t qual_sum, uint32_t l_seq) {
    if (l_seq == 0u) return (uint8_t)255;
    uint32_t m = 0;
    for (uint32_t bit = 128u; bit; bit >>= 1)
        if ((uint64_t)(m | bit) * l_seq <= qual_sum) m |= bit;
    return (uint8_t)m;
}

// The rank a cell stores for read-position rank qpos + 1: saturated at 65,535, so that a claimed cell's rank is never zero
BV_PU_FN uint32_t bv_pileup_rank(uint32_t rank) { return rank < 65535u ? rank : 65535u; }

// The bases [*i_lo, *i_hi) of a match operation that lie in the step, and whether the walk ends behind the operation
BV_PU_FN bool bv_pileup_match_range(const BvPileupQuery *q, int64_t rpos, int64_t len, int64_t *i_lo, int64_t *i_hi) {
    const int64_t lo = (int64_t)q->gb - rpos - 1, hi = (int64_t)q->ge - rpos;
    *i_lo = lo > 0 ? lo : 0;
    *i_hi = hi < len ? hi : len;
    return len > 0 && rpos + len > (int64_t)q->ge;
}

// bytes of a claimed indel's token (its anchor is inside the reference): sign, anchor base, and the clipped letters
BV_PU_FN uint64_t bv_pileup_token_bytes(bool ins, int64_t rpos, uint32_t qpos, int64_t len, uint32_t l_seq, uint64_t ref_len) {
    const uint64_t room = ins ? (uint64_t)(l_seq - qpos) : ref_len - (uint64_t)rpos;
    return 2u + ((uint64_t)len < room ? (uint64_t)len : room);
}

// ---------------------------------------------------------------------------------------------------------------- the serial form
// Where a sample's cells and tokens go.  Planes [rows][pitch]; seen: one bit a row, zeroed by the caller for every sample.
struct BvPileupSink {
    uint8_t *cell, *qual, *mapq;
    uint16_t *rank;
    uint64_t pitch;
    uint32_t *seen;
    BvPileupToken *tokens;  // NULL: count only
    uint8_t *text;
    uint64_t text_at;       // where this sample's next token text goes
    uint64_t token_at;
};

BV_PU_FN bool bv_pileup_attempt(const BvPileupQuery *q, BvPileupSink *k, uint32_t sample, int64_t p, uint32_t code, uint32_t qual, uint32_t mapq,
                                uint32_t rank) {
    if (p < (int64_t)q->beg || p > (int64_t)q->end) return false;
    const uint64_t row = (uint64_t)(p - q->beg);
    const uint32_t bit = 1u << (row & 31u);
    if (k->seen[row >> 5] & bit) return false;
    k->seen[row >> 5] |= bit;
    const uint64_t c = row * k->pitch + sample;
    k->cell[c] = (uint8_t)code; k->qual[c] = (uint8_t)qual; k->mapq[c] = (uint8_t)mapq; k->rank[c] = (uint16_t)bv_pileup_rank(rank);
    return true;
}

// One record that bv_pileup_filter let through
BV_PU_FN uint32_t bv_pileup_walk(const BvPileupQuery *q, const uint8_t *run, const BvPileupRec *r, const uint8_t *ref, uint32_t sample,
                                 BvPileupSink *k, BvPileupSample *s) {
    const uint32_t strand = (r->flag & 16u) ? BV_PU_CELL_REV : 0u;
    const uint8_t *seq = run + bv_pileup_seq_at(r), *qual = run + bv_pileup_qual_at(r);
    uint64_t qsum = 0;
    for (uint32_t i = 0; i < r->l_seq; ++i) qsum += qual[i];
    const uint32_t mean_q = bv_pileup_mean_q(qsum, r->l_seq);
    int64_t rpos = r->pos;
    uint32_t qpos = 0;
    for (uint32_t c = 0; c < r->n_cigar; ++c) {
        const uint32_t cig = bv_pileup_u32(run + r->cigar_at + 4ull * c), op = cig & 15u;
        const int64_t len = cig >> 4;
        if (bv_pileup_op_is_match(op)) {
            int64_t i_lo, i_hi;
            const bool ends = bv_pileup_match_range(q, rpos, len, &i_lo, &i_hi);
            bool over = false, bad = false;
            for (int64_t i = i_lo; i < i_hi; ++i) {
                const uint32_t qi = qpos + (uint32_t)i;
                if (qi >= r->l_seq) { over = true; continue; }
                const uint32_t code = bv_pileup_base_cell(bv_pileup_nibble(seq, qi));
                if (code == BV_PU_CELL_BAD) { bad = true; continue; }
                bv_pileup_attempt(q, k, sample, rpos + i + 1, code | strand, qual[qi], r->mapq, qi + 1u);
            }
            if (over) return BV_PILEUP_BAD_QUERY;
            if (bad) return BV_PILEUP_BAD_BASE;
            if (ends) return BV_PILEUP_OK;
            rpos += len; qpos += (uint32_t)len;
        } else if (op == 1u || op == 2u) {
            const bool ins = op == 1u;
            if ((int64_t)q->ge < rpos + 1) return BV_PILEUP_OK;
            if ((int64_t)q->gb <= rpos + 1 && rpos >= 1 &&
                bv_pileup_attempt(q, k, sample, rpos, (ins ? BV_PU_CELL_INS : BV_PU_CELL_DEL) | strand, mean_q, r->mapq, qpos + 1u)) {
                if ((uint64_t)rpos - 1u >= q->ref_len) return BV_PILEUP_BAD_REF;
                if (ins && qpos > r->l_seq) return BV_PILEUP_BAD_QUERY;
                const uint64_t bytes = bv_pileup_token_bytes(ins, rpos, qpos, len, r->l_seq, q->ref_len);
                if (k->tokens) {
                    BvPileupToken *t = k->tokens + k->token_at;
                    t->pos = (uint32_t)rpos; t->sample = sample; t->text_off = k->text_at; t->text_len = (uint32_t)bytes; t->reserved_ = 0;
                    uint8_t *o = k->text + k->text_at;
                    o[0] = ins ? '+' : '-';
                    o[1] = ref[rpos - 1];
                    for (uint64_t j = 0; j + 2u < bytes; ++j) o[2u + j] = ins ? bv_pileup_letter(bv_pileup_nibble(seq, qpos + (uint32_t)j)) : ref[(uint64_t)rpos + j];
                }
                k->token_at += 1u; k->text_at += bytes;
                s->n_tokens += 1u; s->text_bytes += bytes;
            }
            if (ins) qpos += (uint32_t)len; else rpos += len;
        } else if (op == 3u) {
            if ((int64_t)q->ge < rpos + 1) return BV_PILEUP_OK;
            rpos += len;
        } else if (op == 4u || op == 6u) {
            if ((int64_t)q->ge < rpos + 1) return BV_PILEUP_OK;
            qpos += (uint32_t)len;
        }
    }
    return BV_PILEUP_OK;
}

// One sample: its runs [run_lo, run_hi) of records[run_off[r] - rec_lo ..], in order.  *s is its outcome (s->status is returned).
BV_PU_FN uint32_t bv_pileup_sample(const BvPileupQuery *q, const uint8_t *records, uint64_t rec_lo, const uint64_t *run_off, uint32_t run_lo,
                                   uint32_t run_hi, const uint8_t *ref, uint32_t sample, BvPileupSink *k, BvPileupSample *s) {
    s->at = 0; s->text_bytes = 0; s->status = BV_PILEUP_OK; s->run = 0; s->n_tokens = 0; s->reserved_ = 0;
    for (uint32_t r = run_lo; r < run_hi; ++r) {
        const uint8_t *run = records + (run_off[r] - rec_lo);
        const uint64_t bytes = run_off[r + 1] - run_off[r];
        for (uint64_t at = 0; at < bytes;) {
            BvPileupRec rec;
            uint32_t st = bv_pileup_record(run, bytes, at, &rec);
            if (st == BV_PILEUP_OK) {
                const uint32_t what = bv_pileup_filter(q, &rec);
                if (what == BV_PILEUP_BREAK) return BV_PILEUP_OK;
                if (what == BV_PILEUP_CLAIM) st = bv_pileup_walk(q, run, &rec, ref, sample, k, s);
            }
            if (st != BV_PILEUP_OK) {
                s->status = st; s->run = r; s->at = at;
                return st;
            }
            at = rec.next_at;
        }
    }
    return BV_PILEUP_OK;
}

BV_PU_FN const char *bv_pileup_status_text(uint32_t st) {
    return st == BV_PILEUP_BAD_BLOCK ? "a block_size below 32" : st == BV_PILEUP_BAD_RUN ? "a record overruns its run"
         : st == BV_PILEUP_BAD_LENGTHS ? "n_cigar / l_seq beyond the record's block"
         : st == BV_PILEUP_BAD_QUERY ? "a CIGAR consumes more query bases than l_seq"
         : st == BV_PILEUP_BAD_REF ? "an indel's anchor lies outside the reference sequence"
         : st == BV_PILEUP_BAD_BASE ? "[ERROR] Why dose the size of aligned base is not 1? Check:  " : "ok";
}

#endif  // BV_PILEUP_CORE_H
