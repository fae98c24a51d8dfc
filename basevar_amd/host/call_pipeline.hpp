// call_pipeline.hpp -- the stages of bv_call (bv_call.cpp) and what they hand each other, apart from the command line.
//
//   one producer  --to_gpu-->  engine workers  --to_emit-->  OrderedEmitter  -->  the VCF and CVG outputs
//
// Batches of consecutive sites, numbered in genomic order (Batch::seq).  The three producers run on the caller's thread:
//   produce_batchfile_text   blocks of batchfile rows as text, parsed on the device by the workers      -> to_gpu
//   produce_bam_host         BAM files piled up on the host threads (pileup.hpp), slab rows             -> to_gpu
//   produce_bam_device       BAM windows piled up and called on an engine of its own (device_pileup.hpp) -> to_emit
// (`--inflate device` on batchfiles has none: the workers take turns at the raw reader, RawReaderTurns.)  A new BAM route
// provides one such function: it takes the CallContext, the BamInput, the queue it feeds, the StageClock and the ErrorSink, walks
// the regions with for_each_bam_region and pushes batches in seq order.
// An engine worker (EngineWorker: a thread, an engine on one GPU) shares with the emitter the to_emit queue and nothing else; all
// stages share the CallContext (immutable), the StageClock and the ErrorSink (a mutex of their own each).  The emitter
// (OrderedEmitter: a thread) alone writes the outputs and counts sites, VCF records and device-written lines.
// --emit device (the lines written on the worker's / the pileup's engine) is device_emit.hpp; the host's lists of indel tokens
// and parallel_ranges are indel_tokens.hpp.
#pragma once

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <exception>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "basetype_gpu.hpp"
#include "batch_producer.hpp"
#include "file_major.hpp"
#include "bgzf_tabix.hpp"
#include "device_pileup.hpp"
#include "indel_tokens.hpp"
#include "pileup.hpp"
#include "tabix_query.hpp"
#include "../csrc/bv_text_region_core.h"  // the definition of a region's rows, for the host reader
#include "vcf_emit.hpp"

namespace bvamd {

// What --timing says of the lines and tokens of a batch, summed by the emitter over the batches it wrote
struct EmitCounts {
    // --emit device: VCF lines and CVG rows the device wrote, and records that the host formatted because the device's number
    // formats do not cover them
    uint64_t vcf_lines_device = 0, cvg_lines_device = 0, lines_host_formatted = 0;
    uint64_t indel_columns_device = 0;  // of the rows the device wrote: those whose indel column, not ".", it tallied too
    uint64_t indel_columns_host = 0;    // of the rows the host formatted: those whose indel column is not "."
    // batchfile input: the tokens the engine listed, and the bytes its row and token fetches brought back
    uint64_t indel_tokens_device = 0, text_fetch_bytes = 0;
    EmitCounts &operator+=(const EmitCounts &o) {
        vcf_lines_device += o.vcf_lines_device; cvg_lines_device += o.cvg_lines_device; lines_host_formatted += o.lines_host_formatted;
        indel_columns_device += o.indel_columns_device; indel_columns_host += o.indel_columns_host;
        indel_tokens_device += o.indel_tokens_device; text_fetch_bytes += o.text_fetch_bytes;
        return *this;
    }
};

// One batch of consecutive sites on its way through the pipeline.
struct Batch {
    uint64_t seq = 0;
    SlabBuilder slab;
    std::vector<SiteText> text;
    BaseTypeBatch result;
    std::string error;
    // batchfile input: the block's rows as text (parsed on the device by the engine worker, bv_engine_text_parse), and the
    // cell / phred rows of the records that come back; `error` then follows the records before the offending position
    bool from_text = false;
    std::string rows;
    std::vector<uint64_t> row_off;
    uint32_t n_positions = 0;
    std::vector<uint8_t> cell, phred;
    // --emit device: the VCF lines of the batch's variant records were written on the worker's engine (bv_engine_vcf_format).
    // line j is text[vcf_line_off[j] .. vcf_line_off[j + 1]) and belongs to record vcf_record[j]; the text comes as BGZF members
    // of 0xff00 bytes counted from its first byte (a *.vcf.gz output) or as it is (a plain one)
    bool emit_device = false;
    std::vector<uint32_t> vcf_record;
    std::vector<uint64_t> vcf_line_off, vcf_member_off;
    std::vector<uint8_t> vcf_members;
    std::string vcf_text;
    // ... and its CVG rows there too (bv_engine_cvg_format): the batch's rows back to back
    bool cvg_device = false;
    std::string cvg_text;
    EmitCounts counts;
    // batchfile input: the records' positions in the batch and who read them (TextBatch::position, ::host_read), and who took
    // the device-parsed positions' tokens
    std::vector<uint32_t> position;
    std::vector<uint8_t> host_read;
    BaseTypeEngine::TokenMode tokens = BaseTypeEngine::TOKENS_HOST;
    // --files-per-pass: `rows` are those of files [job_first_file, job_first_file + job_files) for the n_positions of a window, one
    // add of the worker's parse job (basetype_gpu.hpp: TextJob).  The window's last part carries its records on to the emitter:
    // job_used positions have a row in every file, reread(p) brings a position's lines again for the host reader
    bool job_part = false, job_last = false;
    uint32_t job_first_file = 0, job_files = 0, job_used = 0;
    std::function<std::vector<std::string>(size_t)> reread;
    explicit Batch(uint32_t n_samples) : slab(n_samples) {}
    const uint8_t *cell_row(size_t i, size_t n) const { return from_text ? &cell[i * n] : slab.cell_row(i); }
    const uint8_t *phred_row(size_t i, size_t n) const { return from_text ? &phred[i * n] : slab.phred_row(i); }
};
typedef std::unique_ptr<Batch> BatchPtr;

// Bounded hand-off queue (mutex + condition variables); close() lets the consumers drain and stop.
class BatchQueue {
public:
    explicit BatchQueue(size_t cap) : cap_(cap) {}
    void push(BatchPtr b) {
        std::unique_lock<std::mutex> lk(mu_);
        not_full_.wait(lk, [&] { return q_.size() < cap_; });
        q_.push_back(std::move(b));
        not_empty_.notify_one();
    }
    BatchPtr pop() {  // nullptr once closed and empty
        std::unique_lock<std::mutex> lk(mu_);
        not_empty_.wait(lk, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return nullptr;
        BatchPtr b = std::move(q_.front());
        q_.pop_front();
        not_full_.notify_one();
        return b;
    }
    void close() {
        std::lock_guard<std::mutex> lk(mu_);
        closed_ = true;
        not_empty_.notify_all();
    }
private:
    size_t cap_;
    std::deque<BatchPtr> q_;
    bool closed_ = false;
    std::mutex mu_;
    std::condition_variable not_full_, not_empty_;
};

// Wall-clock seconds per stage, the way the reference prints its phases (src/basetype_caller.cpp:193-215, 625-632).  Any thread adds.
class StageClock {
public:
    enum Field { READ, PARSE, ENGINE, EMIT };  // ENGINE: summed over the workers; READ / PARSE: thread-seconds of the producer's side
    void add(Field f, double seconds) { std::lock_guard<std::mutex> lk(mu_); s_[f] += seconds; }
    double get(Field f) const { std::lock_guard<std::mutex> lk(mu_); return s_[f]; }
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
private:
    mutable std::mutex mu_;
    double s_[4] = {0, 0, 0, 0};
};

// The run's error: the first one reported wins, the producers and the raw reader stop once there is one.
class ErrorSink {
public:
    void fail(const std::string &m) { std::lock_guard<std::mutex> lk(mu_); if (first_.empty()) first_ = m; }
    bool ok() const { std::lock_guard<std::mutex> lk(mu_); return first_.empty(); }
    std::string first() const { std::lock_guard<std::mutex> lk(mu_); return first_; }
private:
    mutable std::mutex mu_;
    std::string first_;
};

// Which way each stage goes, resolved from the options and the inputs before any thread starts (bv_call.cpp: resolve_routes)
struct Routes {
    bool device_inflate = false;      // --inflate device: BGZF batchfiles reach the engine compressed (RawReaderTurns)
    bool device_deflate = false;      // --deflate device: the emitter's whole output blocks are compressed by an engine
    bool emit_device = false;         // --emit device: the VCF lines and the CVG rows are written on the worker's / the pileup's engine
    bool device_pileup = false;       // --pileup device: produce_bam_device
    bool bam_inflate_device = false;  // ... with --inflate device: the BAM files' members reach the engine compressed
    bool indel_tokens_device = false; // --indel-tokens device: the engine lists the '+'/'-' tokens of batchfile rows (text_tokens_mode)
};

// One region of batchfile input ("CHR", "CHR:BEG", "CHR:BEG-END" as tabix reads them; open ends reach to 2^29), and where the
// files' indexes say it may begin: index[f] is file f's .tbi where indexed[f], else the file is scanned from its first row
struct BatchRegion {
    std::string name;
    uint32_t beg = 1, end = 1u << 29;
};
struct RegionIndexes {
    std::vector<TabixReader> index;
    std::vector<char> indexed;
    std::vector<size_t> header_lines;
};
// "CHR[:BEG[-END]]"; false for anything else (an empty name, signs, BEG of 0, END < BEG, values beyond 2^29)
inline bool parse_batch_region(const std::string &s, BatchRegion &out) {
    auto number = [](const std::string &t, uint32_t &v) {
        if (t.empty() || t.size() > 9) return false;
        uint32_t x = 0;
        for (char c : t) {
            if (c < '0' || c > '9') return false;
            x = x * 10u + (uint32_t)(c - '0');
        }
        v = x;
        return x >= 1u && x <= (1u << 29);
    };
    out = BatchRegion();
    const size_t colon = s.rfind(':');
    out.name = s.substr(0, colon);
    if (out.name.empty()) return false;
    if (colon == std::string::npos) return true;
    const std::string span = s.substr(colon + 1);
    const size_t dash = span.find('-');
    if (!number(span.substr(0, dash), out.beg)) return false;
    if (dash == std::string::npos) return true;
    return number(span.substr(dash + 1), out.end) && out.end >= out.beg;
}

// What every stage reads and none writes: built once before any thread starts, passed as const &
struct CallContext {
    std::vector<std::string> sample_ids, group_names;
    std::vector<uint8_t> group_id;       // [samples]: index into group_names, BV_NO_GROUP
    std::vector<uint32_t> file_samples;  // samples per batchfile, in batchfile order (the header scan)
    uint32_t batch_sites = 0;
    std::vector<int> devices;            // one engine per entry
    int threads = 4;
    float user_min_af = 0.01f;
    int deflate_level = BV_DEFLATE_FAST;
    bool from_bam = false, vcf_gz = false;
    Routes routes;
    std::vector<BatchRegion> regions;    // batchfile input with --regions: called in this order (empty: the whole files)
    size_t n_sample() const { return sample_ids.size(); }
    uint32_t n_groups() const { return (uint32_t)group_names.size(); }
    const uint8_t *group_ids() const { return group_names.empty() ? nullptr : group_id.data(); }
};

// BAM input: the files, the FASTA and the regions in the order given
struct BamInput {
    std::vector<std::string> bams;
    std::string reference;
    std::vector<Region> regions;
    int mapq_thd = 10;
};

// ---------------------------------------------------------------------------------------------------------------- the emitter

// Writes the batches in seq order, whatever order they arrive in.  A failed slab batch stops everything from itself on; a
// failed text batch (its host reader refused a position) first writes its records, which lie before that position.  The lines
// of a batch are formatted by `ctx.threads` threads (ranges of consecutive sites, a text buffer each) and written in site order.
// `deflate` (may be empty; used with routes.device_deflate): compresses the whole blocks a batch completes, bgzf_tabix.hpp.  It
// is let go in finish(), on the emitter's thread.  Without one nothing here needs an engine.
class OrderedEmitter {
public:
    OrderedEmitter(const CallContext &ctx, TextOut &vcf, TextOut &cvg, StageClock &clk, ErrorSink &errors, BlockDeflater deflate = nullptr)
        : ctx_(ctx), vcf_(vcf), cvg_(cvg), clk_(clk), errors_(errors), inner_(std::move(deflate)) {
        deflate_ = [this](const char *text, uint64_t text_bytes, const uint64_t *block_off, uint32_t n_blocks, uint8_t *dst, uint64_t *member_off) {
            const double t0 = StageClock::now();
            inner_(text, text_bytes, block_off, n_blocks, dst, member_off);
            members_deflated_ += n_blocks;
            deflate_s_ += StageClock::now() - t0;
        };
    }
    OrderedEmitter(const OrderedEmitter &) = delete;
    OrderedEmitter &operator=(const OrderedEmitter &) = delete;

    void run(BatchQueue &in) {  // the thread's body
        for (BatchPtr b; (b = in.pop());) accept(std::move(b));
        finish();
    }
    void accept(BatchPtr b) {
        const uint64_t seq = b->seq;
        waiting_[seq] = std::move(b);
        for (auto it = waiting_.find(next_seq_); it != waiting_.end(); it = waiting_.find(next_seq_)) {
            Batch &d = *it->second;
            if (stopped_) {
            } else if (!d.error.empty() && !d.from_text) {
                stopped_ = true;
                errors_.fail(d.error);
            } else {
                write(d);
                if (!d.error.empty()) { stopped_ = true; errors_.fail(d.error); }
            }
            waiting_.erase(it);
            ++next_seq_;
        }
    }
    // No more batches: what still waits behind a gap is dropped, and both outputs are closed (a *.gz gets its last block, its
    // end-of-file member and its index) whether or not the run failed.
    void finish() {
        waiting_.clear();
        inner_ = nullptr;
        try { vcf_.close(); cvg_.close(); } catch (const std::exception &ex) { errors_.fail(ex.what()); }
    }
    // (for the thread that joined the emitter's)
    size_t n_sites() const { return n_sites_; }
    size_t n_variants() const { return n_variants_; }
    const EmitCounts &counts() const { return counts_; }
    uint64_t members_deflated() const { return members_deflated_; }
    double deflate_s() const { return deflate_s_; }

private:
    void write(Batch &d) {
        const double t0 = StageClock::now();
        const size_t nt = (size_t)std::max(1, ctx_.threads), n_sample = ctx_.n_sample();
        const bool device_deflate = ctx_.routes.device_deflate;
        std::vector<std::string> cvg_txt(nt), vcf_txt(nt);
        std::vector<size_t> nv(nt, 0);
        if (d.cvg_device) cvg_txt[0].swap(d.cvg_text);  // (the CVG rows are there already, and with them the VCF lines)
        else parallel_ranges(d.text.size(), ctx_.threads, [&](size_t t, size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i) {
                cvg_txt[t] += format_cvg_line(d.text[i], d.result.sites[i]);
                if (d.emit_device) continue;  // (the VCF lines are there already)
                if (d.result.has_variant(i)) {
                    vcf_txt[t] += format_vcf_line(d.text[i], d.cell_row(i, n_sample), d.phred_row(i, n_sample), n_sample, d.result.sites[i],
                                                  ctx_.group_names.empty() ? nullptr : &d.result.group(i, 0), ctx_.group_names);
                    ++nv[t];
                }
            }
        });
        try {
            if (d.emit_device || device_deflate) {
                // one piece a file and batch (a deflate call takes as long as its slowest block, however few blocks it has)
                for (size_t t = 1; t < nt; ++t) {
                    cvg_txt[0] += cvg_txt[t]; std::string().swap(cvg_txt[t]);
                    vcf_txt[0] += vcf_txt[t]; std::string().swap(vcf_txt[t]);
                }
                if (device_deflate) cvg_.write_lines(cvg_txt[0], deflate_);
                else cvg_.write_lines(cvg_txt[0]);
                std::string().swap(cvg_txt[0]);
                if (d.emit_device) write_device_lines(d, nv[0]);
                else vcf_.write_lines(vcf_txt[0], deflate_);
            } else {
                for (size_t t = 0; t < nt; ++t) {
                    cvg_.write_lines(cvg_txt[t]);
                    vcf_.write_lines(vcf_txt[t]);
                }
            }
            for (size_t t = 0; t < nt; ++t) n_variants_ += nv[t];
        } catch (const std::exception &ex) { errors_.fail(ex.what()); }
        n_sites_ += d.text.size();
        counts_ += d.counts;
        clk_.add(StageClock::EMIT, StageClock::now() - t0);
    }
    // --emit device: the VCF lines as the worker's engine left them
    void write_device_lines(const Batch &d, size_t &n_variant) {
        if (ctx_.vcf_gz) {
            std::vector<std::pair<std::string, int64_t>> keys;
            for (uint32_t i : d.vcf_record) keys.emplace_back(d.text[i].ref_id, (int64_t)d.text[i].ref_pos);
            vcf_.write_members(d.vcf_members.data(), d.vcf_member_off.data(), d.vcf_member_off.empty() ? 0 : d.vcf_member_off.size() - 1, d.vcf_line_off.data(),
                               keys);
        } else {
            vcf_.write_lines(d.vcf_text);
        }
        for (size_t i = 0; i < d.text.size(); ++i) n_variant += d.result.has_variant(i) ? 1 : 0;
    }

    const CallContext &ctx_;
    TextOut &vcf_, &cvg_;
    StageClock &clk_;
    ErrorSink &errors_;
    BlockDeflater inner_, deflate_;
    std::map<uint64_t, BatchPtr> waiting_;  // finished out of order
    uint64_t next_seq_ = 0;
    bool stopped_ = false;  // a batch failed: nothing behind it is written
    size_t n_sites_ = 0, n_variants_ = 0;
    EmitCounts counts_;
    uint64_t members_deflated_ = 0;
    double deflate_s_ = 0;
};

// --deflate device: an engine is not re-entrant and the workers' engines are busy, so the emitter gets a small one of its own
// on the first engine's device, made when its first batch arrives
inline BlockDeflater device_block_deflater(const CallContext &ctx) {
    std::shared_ptr<std::unique_ptr<BaseTypeEngine>> engine(new std::unique_ptr<BaseTypeEngine>());
    const float min_af = ctx.user_min_af;
    const int device = ctx.devices[0], level = ctx.deflate_level;
    return [engine, min_af, device, level](const char *text, uint64_t text_bytes, const uint64_t *block_off, uint32_t n_blocks, uint8_t *dst, uint64_t *member_off) {
        if (!*engine) engine->reset(new BaseTypeEngine(1, 1, min_af, device));
        (*engine)->bgzf_deflate(text, text_bytes, block_off, n_blocks, dst, member_off, level);
    };
}

// ---------------------------------------------------------------------------------------------------------- the engine workers

}  // namespace bvamd
#include "device_emit.hpp"  // (behind Batch and CallContext)
namespace bvamd {

// --indel-tokens device: who takes the tokens of a batch of batchfile rows -- listed on the worker's engine and left there for
// its tally (--emit device), or fetched once into the SiteTexts (--emit host)
inline BaseTypeEngine::TokenMode text_token_mode(const CallContext &ctx) {
    return !ctx.routes.indel_tokens_device ? BaseTypeEngine::TOKENS_HOST
           : ctx.routes.emit_device        ? BaseTypeEngine::TOKENS_DEVICE_KEEP
                                           : BaseTypeEngine::TOKENS_DEVICE;
}

// --inflate device: BGZF batchfiles go to the engine compressed (bv_engine_text_parse_bgzf inflates, finds the lines and
// parses).  There is no producer then: the engine workers take turns at the raw reader -- a worker reads the next runs from the
// cursors, parses them on its engine, hands the new cursors back and only then lets go of the reader, so its row fetch, host
// reader, submit and records overlap the next worker's parse.
class RawReaderTurns {
public:
    RawReaderTurns(const CallContext &ctx, BgzfRawReader &raw, size_t target, const RegionIndexes *idx = nullptr)
        : ctx_(ctx), raw_(raw), target_(target), target0_(target), idx_(idx), seek_(!ctx.regions.empty()) {}
    // One turn: the next batch, numbered and parsed on `engine` (`bp`: for its finish_bgzf), or with the error that ends the
    // file; nullptr when the files are at their end or the run has failed.
    // With ctx.regions: per region every file is sought to where its index says the region may begin, then next / parse-region
    // / advance alternate until the parse says the region is done; the batches carry on in sequence.
    BatchPtr take(BaseTypeEngine &engine, BaseTypeEngine::BgzfParse &bp, StageClock &clk, const ErrorSink &errors) {
        std::lock_guard<std::mutex> lk(mu_);
        const bool by_region = !ctx_.regions.empty();
        while (!done_) {
            if (!errors.ok()) { done_ = true; break; }
            std::string error;
            BgzfRawRuns runs;
            try {
                if (by_region && seek_ && !seek_region()) continue;  // (no index holds a line of it: the next region)
                if (done_) break;
                const double t0 = StageClock::now();
                raw_.next(runs, target_);
                const double t1 = StageClock::now();
                const bv_bgzf_rows rows{runs.data.data(), runs.member_off.data(), runs.data.size(), runs.file_member.data(), ctx_.file_samples.data(),
                                        runs.skip_bytes.data(), runs.skip_lines.data(), (uint32_t)ctx_.file_samples.size(), ctx_.batch_sites,
                                        runs.at_end ? 1u : 0u, 0};
                if (by_region) {
                    const BatchRegion &rg = ctx_.regions[region_];
                    bp = engine.parse_bgzf_region(rows, bv_text_region{rg.name.data(), (uint32_t)rg.name.size(), rg.beg, rg.end, 0}, ctx_.batch_sites, ctx_.group_ids(),
                                                  ctx_.n_groups(), text_token_mode(ctx_));
                } else {
                    bp = engine.parse_bgzf(rows, ctx_.batch_sites, ctx_.group_ids(), ctx_.n_groups(), text_token_mode(ctx_));
                }
                clk.add(StageClock::READ, t1 - t0);
                clk.add(StageClock::ENGINE, StageClock::now() - t1);
            } catch (const BaseTypeEngine::BgzfDataError &ex) {
                // the message the host reader has for such a file; what a region parse refuses is said as it is
                error = std::strstr(ex.what(), "bad header")  ? "[ERROR] not a BGZF member where one was expected (truncated or damaged batchfile)"
                        : std::strstr(ex.what(), "BGZF status") ? "[ERROR] a BGZF member does not inflate to its recorded size"
                                                                : std::string("[ERROR] ") + ex.what();
            } catch (const std::exception &ex) { error = ex.what(); }
            if (error.empty() && by_region) {
                std::vector<uint32_t> cm(bp.cursor.size()), co(bp.cursor.size());
                for (size_t f = 0; f < bp.cursor.size(); ++f) { cm[f] = bp.cursor[f].member; co[f] = bp.cursor[f].offset; }
                const bool moved = raw_.advance_region(runs, cm.data(), co.data());
                if (bp.region_done) {
                    seek_ = true;
                    if (++region_ == ctx_.regions.size()) done_ = true;
                } else if (bp.n_positions == 0 && !moved) {
                    target_ *= 2;  // not one complete line in some run: longer runs
                }
                if (bp.n_positions == 0) continue;
            } else if (error.empty() && bp.n_positions == 0) {
                if (runs.at_end) { done_ = true; break; }
                target_ *= 2;  // not one complete row in every run: longer runs
                continue;
            }
            BatchPtr b(new Batch((uint32_t)ctx_.n_sample()));
            b->from_text = true;
            b->seq = seq_++;
            if (!error.empty()) {
                b->error = error;
                done_ = true;
            } else if (!by_region) {
                std::vector<uint32_t> cm(bp.cursor.size()), co(bp.cursor.size());
                for (size_t f = 0; f < bp.cursor.size(); ++f) { cm[f] = bp.cursor[f].member; co[f] = bp.cursor[f].offset; }
                raw_.advance(runs, cm.data(), co.data());
            }
            return b;
        }
        return nullptr;
    }
private:
    // every file to the start of ctx_.regions[region_]; false (and the next region, or the end) when no file has a line there.
    // A file whose index holds nothing of the region beside files whose indexes do starts at the linear index's offset for the
    // region's first window: the selection finds its terminating line there at once (or its end), and the files' disagreement
    // is refused by the parse, not waited for.
    bool seek_region() {
        const BatchRegion &rg = ctx_.regions[region_];
        size_t nothing = 0;
        target_ = target0_;
        for (size_t f = 0; f < raw_.n_files(); ++f) {
            uint64_t voff = 0;
            bool window = false;
            if (!idx_ || !idx_->indexed[f]) { raw_.rewind(f, idx_ ? idx_->header_lines[f] : 0); continue; }
            const TabixReader::Hit h = idx_->index[f].query(rg.name, rg.beg, rg.end, &voff, &window);  // (an unknown name was refused before the run began)
            if (h != TabixReader::FOUND && !window) raw_.seek_end(f);
            else if (voff == 0) raw_.rewind(f, idx_->header_lines[f]);
            else raw_.seek(f, voff);
            nothing += h != TabixReader::FOUND;
        }
        seek_ = false;
        if (nothing < raw_.n_files()) return true;
        seek_ = true;
        if (++region_ == ctx_.regions.size()) done_ = true;
        return false;
    }
    const CallContext &ctx_;
    BgzfRawReader &raw_;
    std::mutex mu_;
    bool done_ = false;
    uint64_t seq_ = 0;
    size_t target_, target0_ = 0;
    const RegionIndexes *idx_;
    size_t region_ = 0;
    bool seek_;
};

// One worker thread: an engine on devices[w % G], batches from `in` (or from its turns at the raw reader) to `out`
class EngineWorker {
public:
    EngineWorker(const CallContext &ctx, size_t w, BatchQueue &in, BatchQueue &out, RawReaderTurns *raw, StageClock &clk, ErrorSink &errors)
        : ctx_(ctx), device_(ctx.devices[w % ctx.devices.size()]), in_(in), out_(out), raw_(raw), clk_(clk), errors_(errors) {}

    void run() {  // the thread's body
        // this worker feeds one GPU: keep it (and the staging memory it touches first) on the CPUs of that GPU's NUMA node
        (void)bv_bind_thread_to_device_node(device_);
        try {
            engine_.reset(new BaseTypeEngine(ctx_.batch_sites, (uint32_t)ctx_.n_sample(), ctx_.user_min_af, device_));
        } catch (const std::exception &ex) { errors_.fail(ex.what()); }
        if (raw_ && engine_) run_raw_turns();
        for (BatchPtr b; (b = in_.pop());) {
            if (engine_) {
                const double t0 = StageClock::now();
                bool passes_on = true;
                if (b->job_part) passes_on = call_job_part(*b);
                else if (b->from_text) call_text_rows(*b);
                else call_slab(*b);
                clk_.add(StageClock::ENGINE, StageClock::now() - t0);
                if (!passes_on) continue;  // (an add of a window that has more to come)
            } else {
                b->error = "no engine on device " + std::to_string(device_);
            }
            out_.push(std::move(b));
        }
        engine_.reset();  // (here, on this thread and beside the other workers', while the emitter still writes the last batches)
    }

private:
    static bool host_reader(const std::vector<std::string> &r, size_t n, SlabBuilder &sb, SiteText &st) { return parse_site_rows_fast(r, n, sb, st); }

    void run_raw_turns() {
        for (;;) {
            BaseTypeEngine::BgzfParse bp;
            BatchPtr b = raw_->take(*engine_, bp, clk_, errors_);
            if (!b) break;
            if (b->error.empty()) {
                const double t0 = StageClock::now();
                text_batch(*b, [&]() {
                    return engine_->finish_bgzf(bp, ctx_.file_samples.data(), ctx_.file_samples.size(), host_reader, ctx_.n_groups(), !ctx_.routes.emit_device);
                });
                clk_.add(StageClock::ENGINE, StageClock::now() - t0);
            }
            out_.push(std::move(b));
        }
    }
    // the device parses the rows; the positions it leaves to the host go to the host reader in between
    void call_text_rows(Batch &b) {
        text_batch(b, [&]() {
            const bv_text_rows rows{b.rows.data(), b.row_off.data(), ctx_.file_samples.data(), b.rows.size(), b.n_positions, (uint32_t)ctx_.file_samples.size(), 0};
            return engine_->lrt_text(rows, host_reader, ctx_.group_ids(), ctx_.n_groups(), !ctx_.routes.emit_device, text_token_mode(ctx_));
        });
        std::string().swap(b.rows);
    }
    // --files-per-pass: one add of the window's job; the window's last part finishes it and takes the records.  What an add threw
    // is the window's error.  Returns whether the batch goes on to the emitter.
    bool call_job_part(Batch &b) {
        try {
            if (!job_) {
                job_error_.clear();
                job_.reset(new TextJob(*engine_, b.n_positions, ctx_.file_samples, ctx_.group_ids(), ctx_.n_groups(), text_token_mode(ctx_)));
            }
            if (job_error_.empty()) {
                const bv_text_rows rows{b.rows.data(), b.row_off.data(), ctx_.file_samples.data() + b.job_first_file, b.rows.size(), b.n_positions, b.job_files, 0};
                job_->add(rows, b.job_first_file);
            }
        } catch (const std::exception &ex) { if (job_error_.empty()) job_error_ = ex.what(); }
        std::string().swap(b.rows);
        if (!b.job_last) return false;
        b.from_text = true;
        if (job_error_.empty()) text_batch(b, [&]() { return job_->finish(b.reread, host_reader, ctx_.n_groups(), !ctx_.routes.emit_device, b.job_used); });
        else b.error = job_error_;
        job_.reset();
        return true;
    }
    // (the producer's choice of layout: short reads -> the rank words carry the calls, basetype_gpu.hpp)
    void call_slab(Batch &b) {
        try { b.slab.tag_ranks(); b.result = engine_->lrt(b.slab); } catch (const std::exception &ex) { b.error = ex.what(); }
    }
    // a text batch through `make`, which parses and calls it; a failure of the engine leaves the batch without records
    template <class Make>
    void text_batch(Batch &b, Make make) {
        try { take_text_result(b, make()); } catch (const std::exception &ex) { b.error = ex.what(); b.text.clear(); b.emit_device = b.cvg_device = false; b.counts = EmitCounts(); }
    }
    // the records of a text batch into the batch; what the host reader threw becomes the batch's error, behind its records
    void take_text_result(Batch &b, BaseTypeEngine::TextBatch &&tb) {
        b.result = std::move(tb.batch);
        b.text = std::move(tb.text);
        b.cell = std::move(tb.cell);
        b.phred = std::move(tb.phred);
        b.position = std::move(tb.position);
        b.host_read = std::move(tb.host_read);
        b.tokens = tb.tokens;
        b.counts.indel_tokens_device = tb.tokens_device;
        b.counts.text_fetch_bytes = tb.fetch_bytes;
        if (ctx_.routes.emit_device) {  // (over the rows the text submit kept)
            LazyTokenList listed{[&](TokenList &l) { engine_->text_tokens_fetch(l.tokens, l.text); b.counts.text_fetch_bytes += l.bytes(); }};
            emit_records_on_device(ctx_, *engine_, b, b.tokens == BaseTypeEngine::TOKENS_DEVICE_KEEP ? IndelTokenSource::engine_list(*engine_, b, listed)
                                                                                                       : IndelTokenSource::site_texts(b.text, ctx_.threads), nullptr, 0);
        }
        if (tb.error) {
            try { std::rethrow_exception(tb.error); } catch (const std::exception &ex) { b.error = ex.what(); }
        }
    }
    const CallContext &ctx_;
    const int device_;
    BatchQueue &in_, &out_;
    RawReaderTurns *raw_;
    StageClock &clk_;
    ErrorSink &errors_;
    std::unique_ptr<BaseTypeEngine> engine_;
    std::unique_ptr<TextJob> job_;  // --files-per-pass: the window under way
    std::string job_error_;
};

// --------------------------------------------------------------------------------------------------------------- the producers

inline BatchPtr new_slab_batch(const CallContext &ctx, uint64_t seq) {
    BatchPtr b(new Batch((uint32_t)ctx.n_sample()));
    if (!ctx.from_bam) b->slab.reserve_rows(ctx.batch_sites);  // (address space; the pages come as the rows do -- no regrowth copies)
    if (!ctx.group_names.empty()) b->slab.set_groups(ctx.group_id, ctx.n_groups());
    b->seq = seq;
    return b;
}

// One row from every batchfile per position (caller.cpp:586-611), on `ctx.threads` host threads: files read and positions cut
// in blocks by a pipeline of tasks (batch_producer.hpp), joined here in position order.  Every block goes to the engines as its
// rows' text: the device parses them (bv_engine_text_parse), the engine worker re-reads with the host reader only the positions
// the device leaves to it.  A block is one batch; text is about twice the 5 B per cell of planes, so a batch carries half the
// cells of the planes' budget.
inline void produce_batchfile_text(const CallContext &ctx, BatchfileHeaders &headers, const std::vector<std::string> &batchfiles, size_t block_bytes,
                                   BatchQueue &to_gpu, StageClock &clk, const ErrorSink &errors) {
    BatchfileProducer producer(headers.readers, headers.first_row, headers.have_row, ctx.n_sample(), ctx.threads);
    producer.set_paths(batchfiles, headers.header_lines);  // BGZF files (what the reference writes): members inflated in parallel
    struct AddClock {  // (whether run_text returns or throws)
        const BatchfileProducer &p; StageClock &clk;
        ~AddClock() { clk.add(StageClock::READ, p.clock.read); clk.add(StageClock::PARSE, p.clock.parse); }
    } add_clock{producer, clk};
    uint64_t seq = 0;
    producer.run_text([&](std::string &rows, std::vector<uint64_t> &row_off, size_t n_positions) {
        BatchPtr b = new_slab_batch(ctx, seq++);
        b->from_text = true;
        b->rows.swap(rows);
        b->row_off.swap(row_off);
        b->n_positions = (uint32_t)n_positions;
        to_gpu.push(std::move(b));
        return errors.ok();
    }, block_bytes, ctx.batch_sites);
}

// --files-per-pass K: the batchfiles read file-major (file_major.hpp), a window of ctx.batch_sites positions at a time and K files
// at a time within it; every group of files goes to the one engine worker as an add of the window's parse job, the last one with
// what the worker needs to finish the window.  A window that a file ends in is the run's last.
inline void produce_batchfile_file_major(const CallContext &ctx, FileMajorReader &reader, BatchQueue &to_gpu, StageClock &clk, const ErrorSink &errors) {
    const size_t G = reader.groups();
    for (uint64_t seq = 0; errors.ok(); ++seq) {
        double t0 = StageClock::now();
        FileMajorReader::Group g;
        const size_t P = reader.begin(ctx.batch_sites, g);
        if (P == 0) break;
        std::vector<BatchPtr> parts;
        for (size_t gi = 0; gi < G; ++gi) {
            if (gi) reader.group(gi, g);
            BatchPtr b(new Batch((uint32_t)ctx.n_sample()));
            b->seq = seq;
            b->job_part = true;
            b->job_first_file = (uint32_t)g.first_file; b->job_files = (uint32_t)g.n_files;
            b->rows.swap(g.text);
            b->row_off.swap(g.row_off);
            b->n_positions = (uint32_t)P;
            clk.add(StageClock::READ, StageClock::now() - t0);  // (wall seconds of the group's read and pack on this thread and its helpers)
            if (gi + 1 < G) {
                to_gpu.push(std::move(b));
                t0 = StageClock::now();
                continue;
            }
            const size_t used = reader.used();
            b->job_last = true;
            b->job_used = (uint32_t)used;
            const std::vector<FileMajorReader::Cursor> start = reader.window_start();
            FileMajorReader *rd = &reader;
            b->reread = [rd, start](size_t p) { return rd->reread_at(start, p); };
            reader.end();
            to_gpu.push(std::move(b));
            if (used < P || P < ctx.batch_sites) return;  // a file ended in this window
        }
    }
}

// --regions with the host reader (--inflate host, and whatever --inflate device cannot take: plain and plain-gzip files, more
// than one engine).  The rows of a region by the definition of csrc/bv_text_region_core.h, read as a stream: an indexed BGZF file
// starts at the virtual offset its index gives, any other file at its first row; lines are dropped until one is reached, then
// one line per file per position is taken while all are IN, with POS held equal across the files; the same refusals, naming
// file and line.  One thread reads; the batches are text batches as produce_batchfile_text makes them.
class RegionLineSource {
public:
    RegionLineSource(const std::string &path, bool indexed, size_t header_lines) : path_(path), indexed_(indexed), header_lines_(header_lines) {}
    // at the file's first row, or at virtual offset voff
    void start(bool seek, uint64_t voff) {
        line_no_ = 0;
        if (indexed_ && seek) {
            if (!bg_) bg_.reset(new BgzfReader(path_));
            bg_->seek(voff);
            use_bg_ = true;
            return;
        }
        use_bg_ = false;
        gz_.reset(new GzLineReader());
        if (!gz_->open(path_)) throw std::runtime_error("[ERROR] " + path_ + " open failure.");
        std::string skip;
        for (size_t k = 0; k < header_lines_; ++k) gz_->getline(skip);
    }
    void start_empty() { use_bg_ = false; gz_.reset(); }
    bool next(std::string &line) {
        const bool got = use_bg_ ? bg_->getline(line) : gz_ ? gz_->getline(line) : false;
        line_no_ += got ? 1 : 0;
        return got;
    }
    size_t line_no() const { return line_no_ - 1; }  // of the line next() gave last, from where the file was started
    const std::string &path() const { return path_; }
private:
    std::string path_;
    bool indexed_, use_bg_ = false;
    size_t header_lines_, line_no_ = 0;
    std::unique_ptr<BgzfReader> bg_;
    std::unique_ptr<GzLineReader> gz_;
};

inline void produce_batchfile_regions_host(const CallContext &ctx, const std::vector<std::string> &batchfiles, const RegionIndexes &idx, size_t block_bytes,
                                           BatchQueue &to_gpu, StageClock &clk, const ErrorSink &errors) {
    const size_t F = batchfiles.size();
    std::vector<std::unique_ptr<RegionLineSource>> src;
    for (size_t f = 0; f < F; ++f) src.emplace_back(new RegionLineSource(batchfiles[f], idx.indexed[f] != 0, idx.header_lines[f]));
    uint64_t seq = 0;
    BatchPtr cur;
    auto flush = [&]() {
        if (cur && cur->n_positions) to_gpu.push(std::move(cur));
        cur.reset();
    };
    std::vector<std::string> line(F);
    std::vector<uint32_t> cls(F), pos(F);
    for (const BatchRegion &rg : ctx.regions) {
        if (!errors.ok()) break;
        const double t0 = StageClock::now();
        const bv_tr_region key{rg.name.data(), (uint32_t)rg.name.size(), rg.beg, rg.end};
        // the head of file f's next line: 0 at the end of the file, else BV_TR_* bits (| 8: a line); a malformed head is thrown
        auto read = [&](size_t f) {
            if (!src[f]->next(line[f])) { cls[f] = 0; return; }
            line[f].push_back('\n');
            const uint32_t c = bv_tr_head(line[f].data(), line[f].size(), key, &pos[f]);
            if (c & BV_TR_MAL)
                throw std::runtime_error("[ERROR] " + src[f]->path() + ", line " + std::to_string(src[f]->line_no()) + " behind the region's start: the head is not CHROM, a tab, POS, a tab");
            cls[f] = c | 8u;
        };
        size_t nothing = 0;
        std::vector<char> empty(F, 0);
        for (size_t f = 0; f < F; ++f) {
            uint64_t voff = 0;
            bool window = false;
            if (!idx.indexed[f]) { src[f]->start(false, 0); continue; }
            const TabixReader::Hit h = idx.index[f].query(rg.name, rg.beg, rg.end, &voff, &window);
            if (h == TabixReader::FOUND || window) src[f]->start(voff != 0, voff);
            else { src[f]->start_empty(); empty[f] = 1; }
            nothing += h != TabixReader::FOUND;
        }
        if (nothing == F) continue;  // no index holds a line of it
        for (size_t f = 0; f < F; ++f)
            do read(f); while (cls[f] && !(cls[f] & BV_TR_REACHED));  // the lines in front of the region
        for (size_t p = 0; errors.ok(); ++p) {
            size_t in = 0, first_out = F, first_in = F;
            for (size_t f = 0; f < F; ++f) {
                const bool is_in = (cls[f] & BV_TR_IN) != 0;
                in += is_in;
                if (is_in && first_in == F) first_in = f;
                if (!is_in && first_out == F) first_out = f;
            }
            if (in == 0) break;
            if (in < F)
                throw std::runtime_error("[ERROR] " + src[first_out]->path() + ": the file's lines of " + rg.name + ":" + std::to_string(rg.beg) + "-" + std::to_string(rg.end) +
                                         " end behind " + std::to_string(p) + " positions, " + src[first_in]->path() + " has more");
            for (size_t f = 1; f < F; ++f)
                if (pos[f] != pos[0])
                    throw std::runtime_error("[ERROR] " + src[f]->path() + ", position " + std::to_string(p) + " of " + rg.name + ":" + std::to_string(rg.beg) + "-" +
                                             std::to_string(rg.end) + ": POS " + std::to_string(pos[f]) + " differs from " + src[0]->path() + "'s " + std::to_string(pos[0]));
            if (!cur) {
                cur = new_slab_batch(ctx, seq++);
                cur->from_text = true;
                cur->row_off.assign(1, 0);
            }
            for (size_t f = 0; f < F; ++f) {
                cur->rows += line[f];
                cur->row_off.push_back(cur->rows.size());
            }
            if (++cur->n_positions == ctx.batch_sites || cur->rows.size() >= block_bytes) flush();
            for (size_t f = 0; f < F; ++f) read(f);
        }
        clk.add(StageClock::READ, StageClock::now() - t0);
    }
    flush();
}

// fn(region, fa_seq) for the regions in the order given ("-r chr:beg-end[,chr:beg-end ...]", caller.cpp:311-356), with the
// sequence of the region's contig; a region that is not inside its contig is thrown
template <class Fn>
void for_each_bam_region(const BamInput &in, Fn fn) {
    std::string fa_seq, fa_of;
    for (const Region &rg : in.regions) {
        if (fa_of != rg.ref_id) { fa_seq = load_fasta_sequence(in.reference, rg.ref_id); fa_of = rg.ref_id; }
        if (rg.beg < 1 || rg.end < rg.beg || rg.end > fa_seq.size()) throw std::runtime_error("[ERROR] region outside " + rg.ref_id);
        fn(rg, fa_seq);
    }
}

// Pileup windows -> slab rows, straight from the tile planes (no text round trip); a site is a position that at least one
// sample covers (the reference skips rows of total depth 0, caller.cpp:718)
inline void produce_bam_host(const CallContext &ctx, const BamInput &in, BatchQueue &to_gpu, StageClock &clk, const ErrorSink &errors) {
    uint64_t seq = 0;
    BatchPtr cur;
    for_each_bam_region(in, [&](const Region &rg, const std::string &fa_seq) {
        const double tp0 = StageClock::now();
        pileup_region(in.bams, fa_seq, rg.ref_id, rg.beg, rg.end, in.mapq_thd, true, ctx.threads, [&](const PileupTile &t) {
            size_t next_indel = 0;
            for (uint32_t pos = t.beg; pos <= t.end && errors.ok(); ++pos) {
                if (t.depth[pos - t.beg] == 0) continue;
                if (!cur) cur = new_slab_batch(ctx, seq++);
                const size_t k = t.at(pos, 0);
                const char rb = fa_seq[pos - 1];
                cur->slab.add_row(&t.cell[k], &t.qual[k], &t.mapq[k], &t.rank[k], (uint8_t)base_code((char)std::toupper((unsigned char)rb)));
                SiteText st;
                st.ref_id = rg.ref_id; st.ref_pos = pos; st.ref_base = std::string(1, rb);
                while (next_indel < t.indels.size() && t.indels[next_indel].pos < pos) ++next_indel;
                for (; next_indel < t.indels.size() && t.indels[next_indel].pos == pos; ++next_indel) st.indel_tokens.push_back(t.indels[next_indel].text);
                cur->text.push_back(std::move(st));
                if (cur->slab.n_sites() == ctx.batch_sites) to_gpu.push(std::move(cur));
            }
        });
        clk.add(StageClock::PARSE, StageClock::now() - tp0);
    });
    if (cur) to_gpu.push(std::move(cur));  // (a batch in the making has a row)
}

// --pileup device: the samples' raw BAM records of a window go to an engine of the producer's own, which piles them up
// (bv_engine_pileup), gathers the covered rows and submits them where they lie (bv_engine_pileup_rows / _submit); the host
// threads only read and inflate -- or, with routes.bam_inflate_device, read the compressed BGZF members of every sample's fetch
// and the cut points (raw_members.hpp), which the engine inflates too (bv_engine_pileup_bgzf).  Its batches are called already:
// they go to the emitter's queue.
class DevicePileupProducer {
public:
    struct Stats {
        uint64_t reads_bytes = 0;                       // raw BAM records handed to the engine
        uint64_t members_inflated = 0, members_bytes = 0;  // ... or the compressed members handed to it instead
        double pileup_s = 0;                            // seconds inside the pileup calls (part of PARSE)
    };
    DevicePileupProducer(const CallContext &ctx, const BamInput &in, BatchQueue &to_emit, StageClock &clk, const ErrorSink &errors)
        : ctx_(ctx), in_(in), out_(to_emit), clk_(clk), errors_(errors) {}

    void run() {
        struct LetGo {  // the engine and the open files go when the last window is through (or an error ends the walk), not with the producer:
            DevicePileupProducer &p;  // the emitter still writes the last batches then
            ~LetGo() { p.engine_.reset(); p.pool_.reset(); }
        } let_go{*this};
        for_each_bam_region(in_, [&](const Region &rg, const std::string &fa_seq) {
            if (!engine_) engine_.reset(new BaseTypeEngine(ctx_.batch_sites, (uint32_t)ctx_.n_sample(), ctx_.user_min_af, ctx_.devices[0]));
            if (!pool_) pool_.reset(new BamPool(in_.bams, true));
            check(bv_engine_pileup_set_reference(engine_->handle(), fa_seq.data(), fa_seq.size()));
            PileupRegionCall call;
            call.entry.pileup = bv_engine_pileup; call.entry.pileup_bgzf = bv_engine_pileup_bgzf; call.entry.last_error = bv_last_error;
            call.engine = engine_->handle();
            call.n_samples = (uint32_t)ctx_.n_sample(); call.region_beg = rg.beg; call.region_end = rg.end; call.mapq_thd = in_.mapq_thd;
            call.skip_empty = true;
            const uint32_t window = std::min<uint32_t>(pileup_window(in_.bams.size()), bv_pileup_max_rows());
            for_each_pileup_window(rg.beg, rg.end, window, [&](uint32_t wb, uint32_t we) {
                if (errors_.ok()) this->window(call, rg.ref_id, fa_seq, wb, we);
                return errors_.ok();
            });
        });
    }
    const Stats &stats() const { return stats_; }

private:
    void check(int rc) { if (rc != BV_OK) throw std::runtime_error(bv_last_error(engine_->handle())); }

    void window(const PileupRegionCall &call, const std::string &ref_id, const std::string &fa_seq, uint32_t wb, uint32_t we) {
        // every sample's records of the fetch, undecoded (or the members that hold them), on `threads` threads
        const double tr0 = StageClock::now();
        WindowReads reads;
        WindowMembers wm;
        if (ctx_.routes.bam_inflate_device) read_window_members(*pool_, in_.bams, ref_id, wb, we, ctx_.threads, wm);
        else read_window_raw(*pool_, in_.bams, ref_id, wb, we, ctx_.threads, reads);
        const double tp0 = StageClock::now();
        clk_.add(StageClock::READ, tp0 - tr0);
        uint32_t n_cov = 0;
        if (ctx_.routes.bam_inflate_device) {
            if (!wm.plan.runs.empty()) { stats_.members_inflated += wm.plan.member_pos.size(); stats_.members_bytes += wm.plan.data.size(); }
            if (!pileup_window_members(call, wm, wb, we, &n_cov)) return;
        } else {
            stats_.reads_bytes += reads.records.size();
            if (!pileup_window_reads(call, reads, wb, we, &n_cov)) return;
        }
        bv_engine *pe = engine_->handle();
        std::vector<uint32_t> pos(n_cov), depth(n_cov);
        bv_slab slab;
        // (short reads: the rank words carry the calls, as SlabBuilder::tag_ranks chooses on the host path)
        if (bv_engine_pileup_rows(pe, 1, &slab, pos.data(), depth.data()) != BV_OK) check(bv_engine_pileup_rows(pe, 0, &slab, pos.data(), depth.data()));
        // the indel tokens: --emit device tallies them where they lie, and fetches them only for a row it leaves to the host
        window_tokens_.fetched = false;
        if (!ctx_.routes.emit_device) window_tokens_.get();
        const double dt = StageClock::now() - tp0;
        stats_.pileup_s += dt;
        clk_.add(StageClock::PARSE, dt);
        size_t next_token = 0;  // (the window's batches take its tokens in turn)
        for (uint32_t first = 0; first < n_cov && errors_.ok(); first += ctx_.batch_sites)
            call_rows(slab, ref_id, fa_seq, pos, next_token, first, std::min(ctx_.batch_sites, n_cov - first));
    }
    // the last pileup's tokens and their text, to the host
    void fetch_tokens(TokenList &l) {
        bv_engine *pe = engine_->handle();
        bv_pileup_result res{};
        res.mem_kind = BV_MEM_HOST;
        check(bv_engine_pileup_fetch(pe, &res, nullptr));  // (no buffers: the sizes)
        l.tokens.resize(res.n_tokens);
        l.text.resize(res.text_bytes);
        res.tokens = l.tokens.data(); res.text = l.text.data();
        res.tokens_capacity = l.tokens.size(); res.text_capacity = l.text.size();
        check(bv_engine_pileup_fetch(pe, &res, nullptr));
    }
    // rows [first, first + rows) of the window's covered positions: called where they lie, their records and planes into a batch
    // -- or, with --emit device, their records alone: the lines are written from the rows where they lie, before the next window's
    // pileup takes the slab's place, and only the text (or its BGZF members) comes back
    void call_rows(const bv_slab &slab, const std::string &ref_id, const std::string &fa_seq, const std::vector<uint32_t> &pos, size_t &next_token, uint32_t first,
                   uint32_t rows) {
        const size_t n_sample = ctx_.n_sample();
        BatchPtr b(new Batch((uint32_t)n_sample));
        b->seq = seq_++;
        b->from_text = true;  // (its cell / phred rows come back beside the records)
        b->result.sites.resize(rows);
        b->result.n_groups = ctx_.n_groups();
        b->result.groups.resize((size_t)rows * ctx_.n_groups());
        const bool emit_device = ctx_.routes.emit_device;
        if (!emit_device) {
            b->cell.resize((size_t)rows * n_sample);
            b->phred.resize((size_t)rows * n_sample);
        }
        const double te0 = StageClock::now();
        check(bv_engine_pileup_submit(engine_->handle(), first, rows, ctx_.group_ids(), ctx_.n_groups(), b->result.sites.data(),
                                      ctx_.group_names.empty() ? nullptr : b->result.groups.data(), emit_device ? nullptr : b->cell.data(),
                                      emit_device ? nullptr : b->phred.data(), nullptr));
        clk_.add(StageClock::ENGINE, StageClock::now() - te0);
        for (uint32_t k = 0; k < rows; ++k) {
            SiteText st;
            st.ref_id = ref_id; st.ref_pos = pos[first + k]; st.ref_base = std::string(1, fa_seq[st.ref_pos - 1]);
            b->text.push_back(std::move(st));
        }
        if (emit_device) {  // (the column is tallied on the engine: the SiteTexts stay without tokens)
            const double tw0 = StageClock::now();
            emit_records_on_device(ctx_, *engine_, *b, IndelTokenSource::pileup(b->text, window_tokens_), &slab, first);
            clk_.add(StageClock::ENGINE, StageClock::now() - tw0);
        } else {
            window_tokens_.get().deal(&pos[first], rows, b->text.data(), next_token);
        }
        out_.push(std::move(b));
    }

    const CallContext &ctx_;
    const BamInput &in_;
    BatchQueue &out_;
    StageClock &clk_;
    const ErrorSink &errors_;
    std::unique_ptr<BaseTypeEngine> engine_;
    std::unique_ptr<BamPool> pool_;
    Stats stats_;
    uint64_t seq_ = 0;
    LazyTokenList window_tokens_{[this](TokenList &l) { fetch_tokens(l); }};  // the current window's: --emit device fetches them only if a row asks
};

}  // namespace bvamd
