// basetype_gpu.hpp -- header-only C++17 host wrapper over the C ABI (include/basevar_amd.h).
//
// This is what a maintainer of the reference would include in src/basetype_caller.cpp: it
// mirrors the per-site interface of the reference, batched.
//
//   reference (per site, src/basetype_caller.cpp:742-743, 1113-1164)      here (per batch of sites)
//   ---------------------------------------------------------------      ---------------------------------
//   BatchInfo bi; ... fill from batchfile lines                            SlabBuilder::add_site(bi)
//   BaseType bt(&bi, min_af); bt.lrt();                                    BaseTypeEngine::lrt(builder) -> batch
//   bt.get_alt_bases() / get_lrt_af(b) / get_var_qual()                    batch.get_alt_bases(i) / get_lrt_af(i,b) / ...
//   strand_bias(...), ref_vs_alt_ranksumtest(...)                          batch.strand_bias(i, flavour), batch.rank_sums(i)
//
// Errors keep the reference's type (std::runtime_error) and, where the reference has one,
// its message (src/basetype.cpp:54-56, 113-115, 272; src/basetype.h:133-149).
#pragma once

#include <cctype>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../include/basevar_amd_indel.h"
#include "../../include/basevar_amd_text_tokens.h"
#include "../../include/basevar_amd_record_text.h"
#include "../../include/basevar_amd_region.h"
#include "../../include/basevar_amd_vcf.h"
#include "../../include/basevar_amd_text_job.h"
#include "indel_tokens.hpp"  // TokenList, row_indel_tokens
#include "vcf_emit.hpp"  // SiteText

namespace bvamd {

static const std::vector<char> BASES = {'A', 'C', 'G', 'T'};  // src/basetype.h:19

inline int base_code(char b) {
    switch (b) {
        case 'A': return BV_BASE_A;
        case 'C': return BV_BASE_C;
        case 'G': return BV_BASE_G;
        case 'T': return BV_BASE_T;
        default: return BV_BASE_OTHER;
    }
}

// Packs reference-style per-site inputs (any type with the members of `struct BatchInfo`,
// src/basetype.h:25-43) into the SoA planes of bv_slab.  Host memory; the engine stages it.
class SlabBuilder {
public:
    explicit SlabBuilder(uint32_t n_samples) : n_(n_samples), pitch_((n_samples + 255u) / 256u * 256u) {}

    template <class BatchInfoLike>
    void add_site(const BatchInfoLike &bi) {
        if (bi.align_bases.size() != n_ || bi.align_base_quals.size() != n_ || bi.mapqs.size() != n_ ||
            bi.map_strands.size() != n_ || bi.base_pos_ranks.size() != n_)
            throw std::runtime_error("[ERROR] Something is wrong in batchfiles.");  // caller.cpp:736
        plain_only();
        // The reference's order of complaints (basetype_caller.cpp:738-743): _out_cvg_line -> strand_bias runs BEFORE the
        // BaseType constructor, over every sample whose token does not start with N / + / - -- an empty token (its [0] is the
        // terminator) and characters outside ACGT included -- and refuses a strand that is neither + nor - (basetype.cpp:253-273);
        // only a position that passes gets the constructor's checks.  (Held against the reference's own _basevar_caller by
        // tests/test_host_formats.py.)
        for (uint32_t i = 0; i < n_; ++i) {
            const std::string &tok = bi.align_bases[i];
            const char fb = tok.empty() ? '\0' : tok[0];
            if (fb == 'N' || fb == '+' || fb == '-') continue;
            const char s = bi.map_strands[i];
            if (s != '+' && s != '-') throw std::runtime_error(std::string("[ERROR] Get strange strand symbol: ") + s);
        }
        const size_t off = bs_.size();
        bs_.resize(off + pitch_, BV_CELL_N);
        q_.resize(off + pitch_, 0);
        mq_.resize(off + pitch_, 0);
        rp_.resize(off + pitch_, 0);
        struct Undo {  // a refused site leaves nothing behind
            SlabBuilder &sb; size_t off; bool keep = false;
            ~Undo() { if (!keep) { sb.bs_.resize(off); sb.q_.resize(off); sb.mq_.resize(off); sb.rp_.resize(off); } }
        } undo{*this, off};
        for (uint32_t i = 0; i < n_; ++i) {
            const std::string &tok = bi.align_bases[i];
            const char fb = tok.empty() ? '\0' : tok[0];  // (an empty token fails the size() != 1 check below, as in the reference)
            uint8_t cell;
            if (fb == 'N') {
                cell = BV_CELL_N;
            } else if (fb == '+') {
                cell = BV_CELL_INS;
            } else if (fb == '-') {
                cell = BV_CELL_DEL;
            } else {
                if (tok.size() != 1)  // src/basetype.cpp:54-56
                    throw std::runtime_error("[ERROR] Why dose the size of aligned base is not 1? Check: " + tok);
                const int c = base_code(fb);
                if (c == BV_BASE_OTHER) {
                    // A single character outside ACGTN+- : the reference would count it in total_depth and give it
                    // an all-eps/3 likelihood row (src/basetype.cpp:58-64).  Its own pileup never writes one
                    // (bam_record.h:28-31, caller.cpp:1060-1077) and the slab has no code for it, so such a token is
                    // refused loudly instead of being dropped silently.
                    throw std::runtime_error(std::string("[ERROR] base character '") + fb +
                                             "' is outside ACGTN+-: not representable in the slab (the reference would "
                                             "count it in the depth)");
                } else {
                    cell = (uint8_t)(c | (bi.map_strands[i] == '-' ? BV_CELL_REV : 0));  // (+ or -: checked above)
                }
            }
            bs_[off + i] = cell;
            q_[off + i] = (uint8_t)(bi.align_base_quals[i] - 33);  // src/basetype.cpp:47
            mq_[off + i] = (uint8_t)bi.mapqs[i];
            rp_[off + i] = (uint16_t)bi.base_pos_ranks[i];
        }
        ref_.push_back((uint8_t)base_code((char)std::toupper((unsigned char)(bi.ref_base.empty() ? 'N' : bi.ref_base[0]))));
        undo.keep = true;
    }

    // One site straight from per-sample planes in the slab's own encoding (e.g. a row of a PileupTile, pileup.hpp).
    void add_row(const uint8_t *cell, const uint8_t *phred, const uint8_t *mapq, const uint16_t *rank, uint8_t ref_code) {
        plain_only();
        const size_t off = bs_.size();
        bs_.resize(off + pitch_, BV_CELL_N);
        q_.resize(off + pitch_, 0);
        mq_.resize(off + pitch_, 0);
        rp_.resize(off + pitch_, 0);
        std::memcpy(&bs_[off], cell, n_);
        std::memcpy(&q_[off], phred, n_);
        std::memcpy(&mq_[off], mapq, n_);
        std::memcpy(&rp_[off], rank, (size_t)n_ * sizeof(uint16_t));
        ref_.push_back(ref_code);
    }
    // A row filled in place (batchfile_fast.hpp): begin_row() appends an all-'N' row and hands out its planes; commit_row()
    // makes it a site, drop_row() takes it back.
    struct Row {
        uint8_t *cell, *phred, *mapq;
        uint16_t *rank;
    };
    Row begin_row() {
        plain_only();
        const size_t off = (size_t)n_sites() * pitch_;
        bs_.resize(off + pitch_, BV_CELL_N);
        q_.resize(off + pitch_, 0);
        mq_.resize(off + pitch_, 0);
        rp_.resize(off + pitch_, 0);
        std::memset(&bs_[off], BV_CELL_N, pitch_);
        std::memset(&q_[off], 0, pitch_);
        std::memset(&mq_[off], 0, pitch_);
        std::memset(&rp_[off], 0, pitch_ * sizeof(uint16_t));
        return Row{&bs_[off], &q_[off], &mq_[off], &rp_[off]};
    }
    void commit_row(uint8_t ref_code) { ref_.push_back(ref_code); }
    void drop_row() {
        const size_t off = (size_t)n_sites() * pitch_;
        bs_.resize(off); q_.resize(off); mq_.resize(off); rp_.resize(off);
    }
    // All rows of `o` (same sample count), behind this builder's: blocks of sites parsed by several threads into builders
    // of their own are joined in site order this way (bv_call).
    void append(const SlabBuilder &o) {
        if (o.n_ != n_) throw std::runtime_error("[ERROR] SlabBuilder::append: different sample counts");
        plain_only(); o.plain_only();
        bs_.insert(bs_.end(), o.bs_.begin(), o.bs_.end());
        q_.insert(q_.end(), o.q_.begin(), o.q_.end());
        mq_.insert(mq_.end(), o.mq_.begin(), o.mq_.end());
        rp_.insert(rp_.end(), o.rp_.begin(), o.rp_.end());
        ref_.insert(ref_.end(), o.ref_.begin(), o.ref_.end());
    }
    // rows [first, first + k) of `o` only
    void append_rows(const SlabBuilder &o, size_t first, size_t k) {
        if (o.n_ != n_) throw std::runtime_error("[ERROR] SlabBuilder::append: different sample counts");
        plain_only(); o.plain_only();
        const size_t a = first * pitch_, b = (first + k) * pitch_;
        bs_.insert(bs_.end(), o.bs_.begin() + a, o.bs_.begin() + b);
        q_.insert(q_.end(), o.q_.begin() + a, o.q_.begin() + b);
        mq_.insert(mq_.end(), o.mq_.begin() + a, o.mq_.begin() + b);
        rp_.insert(rp_.end(), o.rp_.begin() + a, o.rp_.begin() + b);
        ref_.insert(ref_.end(), o.ref_.begin() + first, o.ref_.begin() + first + k);
    }
    void reserve_rows(size_t rows) {
        bs_.reserve(rows * pitch_); q_.reserve(rows * pitch_); mq_.reserve(rows * pitch_); rp_.reserve(rows * pitch_); ref_.reserve(rows);
    }
    const uint8_t *cell_row(size_t site) const { return &bs_[site * pitch_]; }
    const uint8_t *phred_row(size_t site) const { return &q_[site * pitch_]; }
    const uint8_t *mapq_row(size_t site) const { return &mq_[site * pitch_]; }
    const uint16_t *rank_row(size_t site) const { return &rp_[site * pitch_]; }
    uint8_t ref_code(size_t site) const { return ref_[site]; }

    void set_groups(const std::vector<uint8_t> &group_id, uint32_t n_groups) {
        gid_ = group_id;
        gid_.resize(pitch_, BV_NO_GROUP);
        n_groups_ = n_groups;
    }
    void clear() { bs_.clear(); q_.clear(); mq_.clear(); rp_.clear(); ref_.clear(); layout_ = 0; }
    // The producer's choice of the rank plane's layout (include/basevar_amd.h, BV_SLAB_RPR_TAGGED): when every read-position
    // rank of the slab is <= 8,191 -- every short-read cohort -- each rank word also takes its cell's call, and the engine's rank
    // sums (ref_vs_alt_ranksumtest, src/basetype.cpp:201-242) read mapq + rpr only.  Call it on a COMPLETE slab, before slab():
    // rows cannot be added afterwards (clear() starts a plain slab again), rank_row() then returns the tagged words.  Returns
    // whether the slab is tagged now; a slab with a longer read stays plain and is submitted as such.  Records do not depend on it.
    bool tag_ranks() {
        if (layout_ & BV_SLAB_RPR_TAGGED) return true;
        uint16_t any = 0;
        for (uint16_t v : rp_) any |= v;
        if (any & (uint16_t)~BV_RPR_TAG_MAX_RANK) return false;
        for (size_t i = 0; i < rp_.size(); ++i) rp_[i] = BV_RPR_TAGGED((uint32_t)bs_[i], (uint32_t)rp_[i]);
        layout_ = BV_SLAB_RPR_TAGGED;
        return true;
    }
    uint32_t layout() const { return layout_; }
    uint32_t n_sites() const { return (uint32_t)ref_.size(); }
    uint32_t n_samples() const { return n_; }
    uint32_t n_groups() const { return n_groups_; }

    bv_slab slab() const {
        bv_slab s{};
        s.n_sites = n_sites(); s.n_samples = n_; s.pitch = pitch_;
        s.base_strand = bs_.data(); s.qual = q_.data(); s.mapq = mq_.data(); s.rpr = rp_.data();
        s.ref_base = ref_.data();
        s.group_id = n_groups_ ? gid_.data() : nullptr;
        s.n_groups = n_groups_;
        s.mem_kind = BV_MEM_HOST;
        s.layout = layout_;
        return s;
    }

private:
    void plain_only() const {
        if (layout_) throw std::runtime_error("[ERROR] SlabBuilder: rows cannot be added to a slab whose ranks are tagged (tag_ranks)");
    }
    uint32_t n_, n_groups_ = 0, layout_ = 0;
    uint64_t pitch_;
    std::vector<uint8_t> bs_, q_, mq_, ref_, gid_;
    std::vector<uint16_t> rp_;
};

struct StrandBiasInfo {  // src/basetype.h:57-62
    int ref_fwd, ref_rev, alt_fwd, alt_rev;
    double fs, sor;
};

// Results of one batch; getters carry the reference's names (src/basetype.h:121-151).
class BaseTypeBatch {
public:
    std::vector<bv_site_result> sites;
    std::vector<bv_group_result> groups;
    uint32_t n_groups = 0;

    std::vector<char> get_alt_bases(size_t i) const {
        std::vector<char> v;
        for (int k = 0; k < sites[i].n_alt; ++k) v.push_back(BASES[sites[i].alt[k] & 3]);
        return v;
    }
    double get_lrt_af(size_t i, char b) const {
        for (int k = 0; k < sites[i].n_alt; ++k)
            if (BASES[sites[i].alt[k] & 3] == b) return sites[i].af[k];
        throw std::runtime_error(std::string("[ERROR] out_of_range:: map::at '") + b + "' not found.");
    }
    double get_var_qual(size_t i) const { return sites[i].qual; }
    int get_total_depth(size_t i) const { return (int)sites[i].total_depth; }
    double get_base_depth(size_t i, char b) const {
        const int c = base_code(b);
        if (c == BV_BASE_OTHER) throw std::runtime_error(std::string("[ERROR] out_of_range:: map::at '") + b + "' not found.");
        return (double)sites[i].depth[c];
    }
    bool has_variant(size_t i) const { return (sites[i].status & BV_SITE_VARIANT) != 0; }
    StrandBiasInfo strand_bias(size_t i, bool vcf_flavour) const {
        const bv_site_result &r = sites[i];
        const uint32_t *sb = vcf_flavour ? r.var_sb : r.cvg_sb;
        return {(int)sb[0], (int)sb[1], (int)sb[2], (int)sb[3], vcf_flavour ? r.var_fs : r.cvg_fs,
                vcf_flavour ? r.var_sor : r.cvg_sor};
    }
    // the three INFO rank sums, truncated to int exactly as the caller does (caller.cpp:1151-1157)
    int mq_rank_sum(size_t i) const { return (int)sites[i].mq_ranksum; }
    int read_pos_rank_sum(size_t i) const { return (int)sites[i].rpr_ranksum; }
    int base_q_rank_sum(size_t i) const { return (int)sites[i].bq_ranksum; }
    const bv_group_result &group(size_t i, uint32_t g) const { return groups[i * n_groups + g]; }
};

class BaseTypeEngine {
public:
    // user_min_af is the CLI value (float, src/basetype_utils.h:94); the engine applies
    // min(100/n_samples, user_min_af) in float exactly as caller.cpp:122 does.
    BaseTypeEngine(uint32_t max_sites, uint32_t n_samples, float user_min_af = 0.01f, int device = 0) {
        bv_engine_config cfg{};
        cfg.device = device; cfg.max_sites = max_sites; cfg.max_samples = n_samples;
        cfg.flags = BV_FLAG_SPARSE_TIMING;  // nobody here reads the engine's per-pass timing: spare the launches its event records
        cfg.min_af = bv_min_af(n_samples, user_min_af);
        if (bv_engine_create(&cfg, &e_) != BV_OK) throw std::runtime_error(bv_last_error(nullptr));
    }
    ~BaseTypeEngine() { if (e_) bv_engine_destroy(e_); }
    BaseTypeEngine(const BaseTypeEngine &) = delete;
    BaseTypeEngine &operator=(const BaseTypeEngine &) = delete;

    bv_engine *handle() { return e_; }  // for the entry points that have no wrapper here (include/basevar_amd_pileup.h)

    BaseTypeBatch lrt(const SlabBuilder &b) {
        BaseTypeBatch out;
        out.sites.resize(b.n_sites());
        out.n_groups = b.n_groups();
        out.groups.resize((size_t)b.n_sites() * b.n_groups());
        bv_slab s = b.slab();
        if (bv_engine_submit(e_, &s, out.sites.data(), out.n_groups ? out.groups.data() : nullptr, nullptr) != BV_OK)
            throw std::runtime_error(bv_last_error(e_));
        if (bv_engine_wait(e_) != BV_OK) throw std::runtime_error(bv_last_error(e_));
        return out;
    }

    // A batch of positions as the batchfiles' own text rows (bv_engine_text_parse): row (p, f) of `rows` is position p's line of
    // batchfile f.  The device parses every position it can; the others go to `read_host` -- the host reader,
    // bool(const std::vector<std::string> &rows, size_t n_samples, SlabBuilder &, SiteText &) as parse_site_rows_fast -- in
    // position order.  When that reader throws, the positions before the offending one are delivered and `error` holds its
    // exception (the caller rethrows it after emitting them: BatchfileProducer's order).
    enum TokenMode { TOKENS_HOST = 0, TOKENS_DEVICE = 1, TOKENS_DEVICE_KEEP = 2 };  // (text_tokens_mode, below)
    struct TextBatch {
        BaseTypeBatch batch;               // one record per position that was not skipped
        std::vector<uint32_t> position;    // ... its index in the batch
        std::vector<SiteText> text;        // ... coordinates, REF and '+'/'-' tokens (the CVG indel column)
        std::vector<uint8_t> cell, phred;  // ... [records][n_samples]: the GT:AB:SO:BP strings of format_vcf_line
        std::vector<uint8_t> row_state;    // [n_positions][n_files] as bv_engine_text_parse reported it (HOST -> SKIP where the host skipped)
        std::vector<uint8_t> host_read;    // [records]: 1 where the host reader made the record (its tokens are the host reader's)
        uint32_t n_positions_used = 0;
        TokenMode tokens = TOKENS_HOST;    // who took the '+'/'-' tokens of the device-parsed positions (below)
        uint64_t tokens_device = 0;        // TOKENS_DEVICE*: the tokens the engine listed for the batch (those of positions behind n_positions_used too)
        uint64_t fetch_bytes = 0;          // bytes the rows / heads fetch and the token fetch brought back
        std::exception_ptr error;
    };
    // Who takes the '+SEQ' / '-SEQ' tokens of the device-parsed positions (include/basevar_amd_text_tokens.h):
    //   TOKENS_HOST         finish_text walks the marked rows on this thread (the default: the path as it was)
    //   TOKENS_DEVICE       the engine lists them during the parse; SiteText::indel_tokens is filled from one text_tokens_fetch
    //   TOKENS_DEVICE_KEEP  ... and they stay there for the caller's bv_engine_indel_tally (text_tokens()): indel_tokens of the
    //                       device-parsed positions stay empty
    // The tokens of a host-read position are the host reader's in every mode.
    void text_tokens_mode(TokenMode m) {
        const bool on = m != TOKENS_HOST;
        if (on == tokens_on_) return;
        if (bv_engine_text_tokens_enable(e_, on ? 1 : 0) != BV_OK) throw std::runtime_error(bv_last_error(e_));
        tokens_on_ = on;
    }
    bv_indel_tokens text_tokens() {
        bv_indel_tokens t;
        if (bv_engine_text_tokens(e_, &t) != BV_OK) throw std::runtime_error(bv_last_error(e_));
        return t;
    }
    void text_tokens_fetch(std::vector<bv_pileup_token> &tokens, std::vector<uint8_t> &text) {
        const bv_indel_tokens t = text_tokens();
        tokens.resize((size_t)t.n_tokens);
        text.resize((size_t)t.text_bytes);
        uint64_t n = 0, nb = 0;
        if (bv_engine_text_tokens_fetch(e_, tokens.data(), tokens.size(), text.data(), text.size(), &n, &nb, nullptr) != BV_OK)
            throw std::runtime_error(bv_last_error(e_));
    }
    template <class HostReader>
    TextBatch lrt_text(const bv_text_rows &rows, HostReader &&read_host, const uint8_t *group_id = nullptr, uint32_t n_groups = 0,
                       bool keep_planes = true, TokenMode tokens = TOKENS_HOST) {
        TextBatch tb;
        tb.tokens = tokens;
        text_tokens_mode(tokens);
        const size_t F = rows.n_files;
        tb.row_state.resize((size_t)rows.n_positions * F);
        if (bv_engine_text_parse(e_, &rows, group_id, n_groups, tb.row_state.data(), nullptr) != BV_OK)
            throw std::runtime_error(bv_last_error(e_));
        uint32_t N = 0;
        for (size_t f = 0; f < F; ++f) N += rows.file_samples[f];
        auto row_text = [&](size_t p, size_t f) {  // the row without its '\n'
            const uint64_t a = rows.row_off[p * F + f], b = rows.row_off[p * F + f + 1];
            return std::string(rows.text + a, (size_t)(b - a - 1));
        };
        finish_text(tb, rows.n_positions, F, N, row_text,
                    [&](size_t p, size_t f, std::vector<std::string> &out) { row_indel_tokens(rows.text + rows.row_off[p * F + f], out); }, read_host, n_groups,
                    keep_planes);
        return tb;
    }

    // Text deflated into BGZF members on the device (bv_engine_bgzf_deflate, include/basevar_amd_bgzf.h): block k is
    // text[block_off[k] .. block_off[k + 1]) of host memory, 1 to 0xff00 bytes; member k lands at dst + member_off[k].  `dst`
    // has room for text_bytes + 31 * n_blocks bytes, `member_off` for n_blocks + 1 entries.  Blocks until dst is written.
    // `level`: BV_DEFLATE_FAST, or BV_DEFLATE_SMALL for files near zlib level 6's size and more kernel time (README has both).
    void bgzf_deflate(const char *text, uint64_t text_bytes, const uint64_t *block_off, uint32_t n_blocks, uint8_t *dst, uint64_t *member_off,
                      int level = BV_DEFLATE_FAST) {
        if (bv_engine_bgzf_deflate_level(e_, text, text_bytes, BV_MEM_HOST, block_off, n_blocks, level, dst, text_bytes + 31ull * n_blocks, member_off, nullptr) != BV_OK)
            throw std::runtime_error(bv_last_error(e_));
    }

    // The VCF lines of records, their sample columns written on the device (include/basevar_amd_vcf.h): line k is heads[k] -- the
    // record through "GT:AB:SO:BP", vcf_emit.hpp's format_vcf_head -- then one column per sample of row site[k] of `slab`, or,
    // with slab == nullptr, of record site[k] of this engine's last lrt_text / finish_bgzf; gt[4 k ..] are vcf_gt_codes' four
    // characters.  The text stays on the device; returns line_off [n + 1].  vcf_fetch() copies it to the host; vcf_deflate()
    // is bgzf_deflate() over it where it lies: block k is text[block_off[k] .. block_off[k + 1]), `dst` has room for
    // line_off[n] + 31 * n_blocks bytes.
    std::vector<uint64_t> vcf_format(const std::vector<uint32_t> &site, const std::vector<std::string> &heads, const std::vector<uint8_t> &gt,
                                     const bv_slab *slab = nullptr) {
        const size_t n = site.size();
        if (heads.size() != n || gt.size() != 4 * n) throw std::runtime_error("[ERROR] vcf_format: one head and four gt characters per line");
        std::string head;
        std::vector<uint64_t> head_off(n + 1, 0), line_off(n + 1, 0);
        for (size_t k = 0; k < n; ++k) { head += heads[k]; head_off[k + 1] = head.size(); }
        const bv_vcf_lines lines{slab, site.data(), head.data(), head_off.data(), gt.data(), (uint32_t)n, 0};
        if (bv_engine_vcf_format(e_, &lines, line_off.data(), nullptr) != BV_OK) throw std::runtime_error(bv_last_error(e_));
        return line_off;
    }
    void vcf_fetch(char *dst, uint64_t bytes) {
        if (bv_engine_vcf_fetch(e_, dst, bytes, BV_MEM_HOST, nullptr) != BV_OK) throw std::runtime_error(bv_last_error(e_));
    }
    void vcf_deflate(uint64_t text_bytes, const uint64_t *block_off, uint32_t n_blocks, uint8_t *dst, uint64_t *member_off, int level = BV_DEFLATE_FAST) {
        if (bv_engine_vcf_deflate(e_, block_off, n_blocks, level, dst, text_bytes + 31ull * n_blocks, member_off, nullptr) != BV_OK)
            throw std::runtime_error(bv_last_error(e_));
    }

    // Whole VCF lines and CVG rows written on the device from the records (include/basevar_amd_record_text.h): the heads and the
    // rows are vcf_emit.hpp's format_vcf_head and format_cvg_line, byte for byte, for every record record_text_on_device()
    // accepts; the others go in as host text.  vcf_format_records() leaves vcf_format()'s text (vcf_fetch, vcf_deflate);
    // cvg_format() a text of its own (cvg_fetch).  Both return line_off [n_lines + 1].
    static bool record_text_on_device(const bv_site_result &r, const bv_group_result *groups, uint32_t n_groups) {
        return bv_record_text_on_device(&r, groups, n_groups) != 0;
    }
    std::vector<uint64_t> vcf_format_records(const bv_record_lines &in) {
        std::vector<uint64_t> line_off((size_t)in.n_lines + 1, 0);
        if (bv_engine_vcf_format_records(e_, &in, line_off.data(), nullptr) != BV_OK) throw std::runtime_error(bv_last_error(e_));
        return line_off;
    }
    std::vector<uint64_t> cvg_format(const bv_record_lines &in) {
        std::vector<uint64_t> line_off((size_t)in.n_lines + 1, 0);
        if (bv_engine_cvg_format(e_, &in, line_off.data(), nullptr) != BV_OK) throw std::runtime_error(bv_last_error(e_));
        return line_off;
    }
    void cvg_fetch(char *dst, uint64_t bytes) {
        if (bv_engine_cvg_fetch(e_, dst, bytes, BV_MEM_HOST, nullptr) != BV_OK) throw std::runtime_error(bv_last_error(e_));
    }

    // The CVG rows' indel columns tallied on the device (include/basevar_amd_indel.h): indel_string's bytes for every row inside
    // the tally's domain.  indel_tally() leaves the columns of rows `key` on the device and returns col_off [n + 1]; row_flag [n]
    // says which rows it left to the caller.  `tok` == nullptr: the tokens of this engine's last pileup, where they lie.
    // cvg_format_tallied() is cvg_format() with those columns; indel_fetch() copies them out.
    std::vector<uint64_t> indel_tally(const bv_indel_tokens *tok, const std::vector<uint32_t> &key, std::vector<uint8_t> &row_flag) {
        std::vector<uint64_t> col_off(key.size() + 1, 0);
        row_flag.assign(key.size(), 0);
        if (bv_engine_indel_tally(e_, tok, key.data(), (uint32_t)key.size(), col_off.data(), row_flag.data(), nullptr) != BV_OK)
            throw std::runtime_error(bv_last_error(e_));
        return col_off;
    }
    void indel_fetch(char *dst, uint64_t bytes) {
        if (bv_engine_indel_fetch(e_, dst, bytes, BV_MEM_HOST, nullptr) != BV_OK) throw std::runtime_error(bv_last_error(e_));
    }
    std::vector<uint64_t> cvg_format_tallied(const bv_record_lines &in) {
        std::vector<uint64_t> line_off((size_t)in.n_lines + 1, 0);
        if (bv_engine_cvg_format_tallied(e_, &in, line_off.data(), nullptr) != BV_OK) throw std::runtime_error(bv_last_error(e_));
        return line_off;
    }

    // lrt_text for rows that are still BGZF members (bv_engine_text_parse_bgzf, include/basevar_amd_bgzf.h), in two steps so
    // that a reader can hand the cursors to the next batch as soon as the parse has returned: parse_bgzf() inflates, indexes
    // and parses on the device (throws BgzfDataError for a damaged member); finish_bgzf() fetches the text the host still needs
    // (bv_engine_text_rows_fetch), runs the host reader on the positions left to it and submits, exactly as lrt_text does.
    struct BgzfDataError : std::runtime_error {
        using std::runtime_error::runtime_error;
    };
    struct BgzfParse {
        uint32_t n_positions = 0;
        std::vector<uint8_t> row_state;
        std::vector<bv_bgzf_cursor> cursor;
        TokenMode tokens = TOKENS_HOST;
        bool region_done = false;  // parse_bgzf_region
    };
    BgzfParse parse_bgzf(const bv_bgzf_rows &rows, uint32_t max_sites, const uint8_t *group_id = nullptr, uint32_t n_groups = 0,
                         TokenMode tokens = TOKENS_HOST) {
        BgzfParse bp;
        bp.tokens = tokens;
        text_tokens_mode(tokens);
        bp.row_state.resize((size_t)std::max<uint32_t>(1, std::min(rows.max_positions, max_sites)) * rows.n_files);
        bp.cursor.resize(rows.n_files);
        const int rc = bv_engine_text_parse_bgzf(e_, &rows, group_id, n_groups, &bp.n_positions, bp.row_state.data(), bp.cursor.data(), nullptr);
        if (rc == BV_ERR_DATA) throw BgzfDataError(bv_last_error(e_));
        if (rc != BV_OK) throw std::runtime_error(bv_last_error(e_));
        bp.row_state.resize((size_t)bp.n_positions * rows.n_files);
        return bp;
    }
    // parse_bgzf() on the lines of a region (bv_engine_text_parse_bgzf_region, include/basevar_amd_region.h): bp.region_done says
    // whether the region has further rows; BgzfDataError also for a malformed head and for files that disagree on the region's
    // lines or on POS.  finish_bgzf() runs unchanged behind it.
    BgzfParse parse_bgzf_region(const bv_bgzf_rows &rows, const bv_text_region &region, uint32_t max_sites, const uint8_t *group_id = nullptr,
                                uint32_t n_groups = 0, TokenMode tokens = TOKENS_HOST) {
        BgzfParse bp;
        bp.tokens = tokens;
        text_tokens_mode(tokens);
        bp.row_state.resize((size_t)std::max<uint32_t>(1, std::min(rows.max_positions, max_sites)) * rows.n_files);
        bp.cursor.resize(rows.n_files);
        uint32_t done = 0;
        const int rc = bv_engine_text_parse_bgzf_region(e_, &rows, &region, group_id, n_groups, &bp.n_positions, bp.row_state.data(), bp.cursor.data(), &done,
                                                        nullptr);
        if (rc == BV_ERR_DATA) throw BgzfDataError(bv_last_error(e_));
        if (rc != BV_OK) throw std::runtime_error(bv_last_error(e_));
        bp.row_state.resize((size_t)bp.n_positions * rows.n_files);
        bp.region_done = done != 0;
        return bp;
    }
    template <class HostReader>
    TextBatch finish_bgzf(BgzfParse &bp, const uint32_t *file_samples, size_t F, HostReader &&read_host, uint32_t n_groups = 0,
                          bool keep_planes = true) {
        TextBatch tb;
        tb.tokens = bp.tokens;
        tb.row_state.swap(bp.row_state);
        uint32_t N = 0;
        for (size_t f = 0; f < F; ++f) N += file_samples[f];
        const size_t R = (size_t)bp.n_positions * F;
        std::vector<uint64_t> off(R + 1);
        std::vector<uint8_t> buf;
        uint64_t need = 0;
        // (the tokens listed on the device: a marked row is needed no further than any other)
        auto fetch = [&](uint8_t *dst, uint64_t cap) {
            return tb.tokens == TOKENS_HOST ? bv_engine_text_rows_fetch(e_, dst, cap, off.data(), &need, nullptr)
                                            : bv_engine_text_heads_fetch(e_, dst, cap, off.data(), &need, nullptr);
        };
        if (fetch(nullptr, 0) != BV_OK) throw std::runtime_error(bv_last_error(e_));
        buf.resize((size_t)need + 1);
        if (fetch(buf.data(), need) != BV_OK) throw std::runtime_error(bv_last_error(e_));
        tb.fetch_bytes += need;
        const char *text = reinterpret_cast<const char *>(buf.data());
        finish_text(tb, bp.n_positions, F, N,
                    [&](size_t p, size_t f) { return std::string(text + off[p * F + f], (size_t)(off[p * F + f + 1] - off[p * F + f])); },
                    [&](size_t p, size_t f, std::vector<std::string> &out) { row_indel_tokens(text + off[p * F + f], out); }, read_host, n_groups, keep_planes);
        return tb;
    }

    // The host's part of a parsed batch and its submit (shared by lrt_text and lrt_bgzf): row_text(p, f) is a row without its
    // line break (whole for the positions left to the host, through its fourth tab at least for file 0's row of any other),
    // row_tokens(p, f, out) appends the '+'/'-' tokens of a row flagged BV_TEXT_INDEL, in sample order.  keep_planes = false: the records' cell / phred rows are
    // not copied back (tb.cell / tb.phred stay empty); they stand on the device for vcf_format().
    template <class RowText, class RowTokens, class HostReader>
    void finish_text(TextBatch &tb, uint32_t P, size_t F, uint32_t N, RowText &&row_text, RowTokens &&row_tokens, HostReader &&read_host, uint32_t n_groups,
                     bool keep_planes = true) {
        SlabBuilder host(N);
        std::vector<std::string> lines(F);
        uint32_t used = 0;
        for (; used < P; ++used) {
            uint8_t *rs = &tb.row_state[(size_t)used * F];
            if (rs[0] & BV_TEXT_SKIP) continue;
            SiteText st;
            const bool host_read = (rs[0] & BV_TEXT_HOST) != 0;
            if (host_read) {
                for (size_t f = 0; f < F; ++f) lines[f] = row_text(used, f);
                bool kept = false;
                try { kept = read_host(lines, (size_t)N, host, st); }
                catch (...) { tb.error = std::current_exception(); break; }
                if (!kept) { for (size_t f = 0; f < F; ++f) rs[f] = BV_TEXT_SKIP; continue; }
            } else {
                // device-parsed: the first three fields of file 0's row, and the '+'/'-' tokens of the flagged rows, in sample order
                const std::string r0 = row_text(used, 0);
                const size_t t1 = r0.find('\t'), t2 = r0.find('\t', t1 + 1), t3 = r0.find('\t', t2 + 1);
                st.ref_id = r0.substr(0, t1);
                st.ref_pos = (uint32_t)std::stoi(r0.substr(t1 + 1, t2 - t1 - 1));
                st.ref_base = r0.substr(t2 + 1, t3 - t2 - 1);
                for (size_t f = 0; f < F && tb.tokens == TOKENS_HOST; ++f)
                    if (rs[f] & BV_TEXT_INDEL) row_tokens(used, f, st.indel_tokens);
            }
            tb.position.push_back(used);
            tb.host_read.push_back(host_read ? 1 : 0);
            tb.text.push_back(std::move(st));
        }
        tb.n_positions_used = used;
        if (tb.tokens != TOKENS_HOST) {
            // the list is in position order, as tb.position is: one pass hands every token to its record (the tokens of a
            // position behind the one the host reader stopped at belong to no record)
            tb.tokens_device = text_tokens().n_tokens;
            if (tb.tokens == TOKENS_DEVICE && tb.tokens_device) {
                TokenList list;
                text_tokens_fetch(list.tokens, list.text);
                tb.fetch_bytes += list.bytes();
                size_t cursor = 0;
                list.deal(tb.position.data(), tb.position.size(), tb.text.data(), cursor);
            }
        }
        const size_t R = tb.position.size();
        tb.batch.sites.resize(R);
        tb.batch.n_groups = n_groups;
        tb.batch.groups.resize(R * n_groups);
        if (keep_planes) {
            tb.cell.resize(R * N);
            tb.phred.resize(R * N);
        }
        const bv_slab hs = host.slab();
        if (bv_engine_text_submit(e_, tb.row_state.data(), hs.n_sites ? &hs : nullptr, used, tb.batch.sites.data(),
                                  n_groups ? tb.batch.groups.data() : nullptr, keep_planes ? tb.cell.data() : nullptr,
                                  keep_planes ? tb.phred.data() : nullptr, nullptr) != BV_OK)
            throw std::runtime_error(bv_last_error(e_));
        if (R && bv_engine_wait(e_) != BV_OK) throw std::runtime_error(bv_last_error(e_));
    }

private:
    bv_engine *e_ = nullptr;
    bool tokens_on_ = false;
};

// lrt_text with the files delivered in groups (include/basevar_amd_text_job.h): a job over P positions of F files; add() takes
// the rows of a run of adjacent files, in any file order, and may free them when it returns; finish() returns what lrt_text
// returns for the rows of all files joined position-major.  What finish_text wants of the rows is kept at add time: the
// coordinates of every position (CHROM, POS, REF of whichever row came first -- they are equal in every row of a position that
// ends parsed) and, with TOKENS_HOST, the '+'/'-' tokens of the rows the add's row_flag marks, per (position, file).
class TextJob {
public:
    TextJob(BaseTypeEngine &eng, uint32_t n_positions, const std::vector<uint32_t> &file_samples, const uint8_t *group_id, uint32_t n_groups,
            BaseTypeEngine::TokenMode tokens)
        : eng_(eng), P_(n_positions), fs_(file_samples), tokens_(tokens), head_(n_positions) {
        eng_.text_tokens_mode(tokens);
        if (bv_engine_text_job_begin(eng_.handle(), P_, (uint32_t)fs_.size(), fs_.data(), group_id, n_groups, nullptr) != BV_OK)
            throw std::runtime_error(bv_last_error(eng_.handle()));
        if (tokens_ == BaseTypeEngine::TOKENS_HOST) row_tokens_.resize((size_t)P_ * fs_.size());
    }
    void add(const bv_text_rows &rows, uint32_t first_file) {
        const size_t K = rows.n_files;
        flag_.assign((size_t)P_ * K, 0);
        if (bv_engine_text_job_add(eng_.handle(), &rows, first_file, flag_.data(), nullptr) != BV_OK) throw std::runtime_error(bv_last_error(eng_.handle()));
        for (size_t p = 0; p < P_; ++p) {
            if (!have_head_) {  // through the third tab (a row without one belongs to a position the host reads)
                const char *r = rows.text + rows.row_off[p * K], *end = rows.text + rows.row_off[p * K + 1];
                const char *t = r;
                for (int tabs = 0; t < end && tabs < 3; ++t) tabs += *t == '\t';
                head_[p].assign(r, (size_t)(t - r));
            }
            for (size_t k = 0; k < K && tokens_ == BaseTypeEngine::TOKENS_HOST; ++k)
                if (flag_[p * K + k] & BV_TEXT_INDEL) row_indel_tokens(rows.text + rows.row_off[p * K + k], row_tokens_[p * fs_.size() + first_file + k]);
        }
        have_head_ = true;
    }
    // reread(p): position p's F lines (without their line breaks), for the positions left to the host reader -- in position
    // order, and none behind the one at which the reader throws.  n_used <= P: the positions that have a row in every file.
    template <class Reread, class HostReader>
    BaseTypeEngine::TextBatch finish(Reread &&reread, HostReader &&read_host, uint32_t n_groups, bool keep_planes = true, uint32_t n_used = UINT32_MAX) {
        BaseTypeEngine::TextBatch tb;
        tb.tokens = tokens_;
        const size_t F = fs_.size();
        tb.row_state.resize((size_t)P_ * F);
        if (bv_engine_text_job_finish(eng_.handle(), tb.row_state.data(), nullptr) != BV_OK) throw std::runtime_error(bv_last_error(eng_.handle()));
        uint32_t N = 0;
        for (uint32_t n : fs_) N += n;
        size_t have = (size_t)-1;
        std::vector<std::string> lines;
        auto row_text = [&](size_t p, size_t f) -> std::string {
            if (!(tb.row_state[p * F] & BV_TEXT_HOST)) return head_[p];  // (asked of file 0 only: the coordinates)
            if (have != p) { lines = reread(p); have = p; }
            return lines[f];
        };
        eng_.finish_text(tb, std::min(P_, n_used), F, N, row_text,
                         [&](size_t p, size_t f, std::vector<std::string> &out) { const auto &t = row_tokens_[p * F + f]; out.insert(out.end(), t.begin(), t.end()); },
                         read_host, n_groups, keep_planes);
        return tb;
    }

private:
    BaseTypeEngine &eng_;
    uint32_t P_;
    std::vector<uint32_t> fs_;
    BaseTypeEngine::TokenMode tokens_;
    std::vector<std::string> head_;
    bool have_head_ = false;
    std::vector<uint8_t> flag_;
    std::vector<std::vector<std::string>> row_tokens_;  // TOKENS_HOST: [P][F]
};

}  // namespace bvamd
