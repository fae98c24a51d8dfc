// bv_call.cpp -- calling phase of `basevar basetype` on the GPU engine: reference-format
// batchfiles in, reference-format VCF + CVG text out.  It is the composition of the rows either
// side of the hot path: batchfile rows -> BatchInfo
// (batchfile.hpp) -> slab -> engine (C ABI) -> VCF/CVG lines (vcf_emit.hpp), following
// _variant_calling_unit (src/basetype_caller.cpp:529-635), with `--pop-group` handled as
// _get_popgroup_info does (src/basetype_caller.cpp:372-410).
//
// Pipeline: the main thread produces batches of sites in genomic order (a slab + one SiteText per site -- not the
// sites' BatchInfo text); `--gpus G` worker threads, one engine on one GPU each, take whichever batch is next; an
// emitter thread writes the results in batch order.  It replaces the reference's fan-out of 100 kb sub-regions over a
// thread pool and its ordered merge of per-task files (_variants_discovery + merge_file_by_line,
// src/basetype_caller.cpp:469-525).
//
//   bv_call --batchfiles a.bf.gz,b.bf.gz --output-vcf out.vcf --output-cvg out.cvg
//           [--pop-group FILE] [--min-af 0.01] [--batch-sites N (default: 2^28 cells / samples, at most 65536)]
//           [--timing FILE.json] [--inflate device|host] [--deflate device|host] [--deflate-level fast|small] [--emit device|host]
//           [--pileup device|host]   (BAM input; with it, --inflate device also hands the BAM files' BGZF members to the engine compressed)
//           [--gpus G] [--devices 0,1,... | --device 0]
//           [--reference ref.fa --contig NAME:LENGTH ...]
//   bv_call -I a.bam [-I b.bam ...] [-L bam.list] -R ref.fa[.gz] --regions CHR:BEG-END[,CHR:BEG-END...] [--mapq 10]
//           [--thread T] ...   (same outputs)
//
// Batchfiles may be bgzip/gzip-compressed or plain (zlib reads all three).  With BAM inputs the pileup
// (pileup.hpp) feeds the engine directly: the same cells the batchfile rows would carry,
// without the text round trip.
#include <algorithm>
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <condition_variable>
#include <deque>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <chrono>

#include "basetype_gpu.hpp"
#include "batch_producer.hpp"
#include "batchfile_fast.hpp"
#include "pileup.hpp"
#include "raw_members.hpp"
#include "raw_reads.hpp"
#include "basevar_amd_pileup.h"
#include "basevar_amd_pileup_bgzf.h"
#include "bgzf_tabix.hpp"
#include "vcf_emit.hpp"

namespace {

// One batch of consecutive sites on its way through the pipeline.
struct Batch {
    uint64_t seq = 0;
    bvamd::SlabBuilder slab;
    std::vector<bvamd::SiteText> text;
    bvamd::BaseTypeBatch result;
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

// Wall-clock seconds per stage, the way the reference prints its phases (src/basetype_caller.cpp:193-215, 625-632).
struct StageClock {
    double read = 0, parse = 0, engine = 0, emit = 0;  // engine: summed over the workers; the others run on one thread each
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
};

// fn(i) for i in [0, n) on up to `threads` threads (contiguous ranges; the caller's thread takes the first)
// An exception in any range (a malformed row, bad_alloc under large batches) is caught on its thread and the first one rethrown
// on the caller's thread once all ranges are done -- the tool's "[ERROR] ..." exit path, not std::terminate.
template <typename Fn>
void parallel_ranges(size_t n, int threads, Fn fn) {
    const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), n));
    if (nt <= 1) { fn(0, 0, n); return; }
    std::vector<std::thread> pool;
    std::vector<std::exception_ptr> errs(nt);
    for (size_t t = 1; t < nt; ++t)
        pool.emplace_back([&, t]() { try { fn(t, n * t / nt, n * (t + 1) / nt); } catch (...) { errs[t] = std::current_exception(); } });
    try { fn(0, 0, n / nt); } catch (...) { errs[0] = std::current_exception(); }
    for (auto &th : pool) th.join();
    for (auto &e : errs) if (e) std::rethrow_exception(e);
}

[[noreturn]] void die(const std::string &m) {
    std::cerr << m << std::endl;
    std::exit(1);
}

}  // namespace

int main(int argc, char **argv) {
    std::vector<std::string> batchfiles, bams;
    std::string out_vcf, out_cvg, pop_group_file, reference = ".", regions, bam_list, devices_arg, timing_file, inflate_arg = "host", deflate_arg = "host",
                deflate_level_arg = "fast", emit_arg = "host", pileup_arg = "host";
    int mapq_thd = 10, threads = 4, n_gpus = 1;  // (`-t`: 4, the reference's default, src/basetype_utils.h:33,94)
    std::vector<bvamd::Contig> contigs;
    float user_min_af = 0.01f;  // BaseTypeARGS default, src/basetype_utils.h:94
    uint32_t batch_sites = 0;   // 0 = from a cell budget once the sample count is known
    int device = 0;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) die("missing value for " + a); return argv[++i]; };
        if (a == "--batchfiles") batchfiles = bvamd::pieces(next(), ',');
        else if (a == "--output-vcf") out_vcf = next();
        else if (a == "--output-cvg") out_cvg = next();
        else if (a == "--pop-group") pop_group_file = next();
        else if (a == "--min-af") user_min_af = std::stof(next());
        else if (a == "--batch-sites") batch_sites = (uint32_t)std::stoul(next());
        else if (a == "--timing") timing_file = next();
        else if (a == "--inflate") inflate_arg = next();
        else if (a == "--deflate") deflate_arg = next();
        else if (a == "--deflate-level") deflate_level_arg = next();
        else if (a == "--emit") emit_arg = next();
        else if (a == "--pileup") pileup_arg = next();
        else if (a == "--device") device = std::stoi(next());
        else if (a == "--gpus") n_gpus = std::stoi(next());
        else if (a == "--devices") devices_arg = next();
        else if (a == "--reference" || a == "-R") reference = next();
        else if (a == "-I" || a == "--input") bams.push_back(next());
        else if (a == "-L" || a == "--align-file-list") bam_list = next();
        else if (a == "-r" || a == "--regions") regions = next();
        else if (a == "-q" || a == "--mapq") mapq_thd = std::stoi(next());
        else if (a == "-t" || a == "--thread") threads = std::stoi(next());
        else if (a == "--contig") {
            const std::vector<std::string> p = bvamd::pieces(next(), ':');
            if (p.size() != 2) die("--contig wants NAME:LENGTH");
            contigs.push_back({p[0], (uint32_t)std::stoul(p[1])});
        } else die("unknown argument " + a);
    }
    if (!bam_list.empty()) {
        std::ifstream f(bam_list);
        if (!f) die("[ERROR] cannot open " + bam_list);
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty() || line[0] == '#') continue;
            const size_t e = line.find_first_of(" \t");
            bams.push_back(e == std::string::npos ? line : line.substr(0, e));
        }
    }
    if (!(user_min_af > 0.f)) die("[ERROR] --min-af must be > 0");  // the reference refuses it too (caller.cpp:73)
    if (n_gpus < 1) die("[ERROR] --gpus must be >= 1");
    if (inflate_arg != "host" && inflate_arg != "device") die("[ERROR] --inflate wants device or host");
    if (deflate_arg != "host" && deflate_arg != "device") die("[ERROR] --deflate wants device or host");
    if (deflate_level_arg != "fast" && deflate_level_arg != "small") die("[ERROR] --deflate-level wants fast or small");
    if (emit_arg != "host" && emit_arg != "device") die("[ERROR] --emit wants device or host");
    if (pileup_arg != "host" && pileup_arg != "device") die("[ERROR] --pileup wants device or host");
    // (the host path is zlib at its own level: the device encoder's levels do not apply to it)
    if (deflate_level_arg != "fast" && deflate_arg != "device") die("[ERROR] --deflate-level small needs --deflate device");
    const int deflate_level = deflate_level_arg == "small" ? BV_DEFLATE_SMALL : BV_DEFLATE_FAST;
    // one engine per entry: --devices a,b,... (an ordinal may repeat: several engines on one GPU), else device, device+1, ...
    std::vector<int> devices;
    if (!devices_arg.empty()) {
        const std::vector<std::string> d = bvamd::pieces(devices_arg, ',');
        for (const auto &x : d) devices.push_back(std::stoi(x));
        if (n_gpus != 1 && (size_t)n_gpus != devices.size()) die("[ERROR] --gpus and --devices disagree");
    } else {
        for (int g = 0; g < n_gpus; ++g) devices.push_back(device + g);
    }
    const bool from_bam = !bams.empty();
    if ((batchfiles.empty() && !from_bam) || out_vcf.empty() || out_cvg.empty() || (from_bam && (regions.empty() || reference == ".")))
        die("usage: bv_call (--batchfiles a,b,... | -I a.bam [-I ...] -R ref.fa --regions CHR:BEG-END [--mapq Q]) --output-vcf FILE "
            "--output-cvg FILE [--pop-group FILE] [--min-af F] [--gpus G]");

    // ---- headers: sample ids in batchfile order (caller.cpp:637-665)
    std::vector<bvamd::GzLineReader> readers(batchfiles.size());
    std::vector<std::string> sample_ids;
    std::vector<std::string> first_row(batchfiles.size());
    std::vector<bool> have_row(batchfiles.size(), false);
    try {
        for (const auto &b : bams) sample_ids.push_back(bvamd::BamFile(b, false).sample_name());
    } catch (const std::exception &ex) { die(ex.what()); }
    std::vector<size_t> header_lines(batchfiles.size(), 0);  // lines in front of the first data row
    std::vector<size_t> file_sample_count(batchfiles.size(), 0);
    for (size_t b = 0; b < batchfiles.size() && !from_bam; ++b) {
        if (!readers[b].open(batchfiles[b])) die("[ERROR] " + batchfiles[b] + " open failure.");
        std::string line;
        while (readers[b].getline(line)) {
            if (line.empty() || line[0] != '#') { first_row[b] = line; have_row[b] = !line.empty(); header_lines[b] += line.empty() ? 1 : 0; break; }
            const size_t before = sample_ids.size();
            bvamd::parse_sample_ids(line, sample_ids);
            file_sample_count[b] += sample_ids.size() - before;
            ++header_lines[b];
        }
    }
    const size_t n_sample = sample_ids.size();
    if (n_sample == 0) die("[ERROR] no ##SampleIDs= header found in the batchfiles");
    if (from_bam) batchfiles.clear();

    // ---- pop groups (caller.cpp:372-410): sample -> group, later rows override; groups iterate by name
    std::map<std::string, std::vector<size_t>> groups_idx;
    if (!pop_group_file.empty()) {
        std::ifstream in(pop_group_file);
        if (!in) die("[ERROR] Cannot open file: " + pop_group_file);
        std::map<std::string, std::string> sample2group;
        std::string sn, gn, skip;
        while (true) {
            in >> sn >> gn;
            if (in.eof()) break;
            sample2group[sn] = gn;
            std::getline(in, skip, '\n');
        }
        for (size_t i = 0; i < n_sample; ++i) {
            auto it = sample2group.find(sample_ids[i]);
            if (it != sample2group.end()) groups_idx[it->second].push_back(i);
        }
    }
    std::vector<std::string> group_names;
    std::vector<uint8_t> group_id(n_sample, BV_NO_GROUP);
    for (const auto &kv : groups_idx) {
        if (group_names.size() >= BV_MAX_GROUPS) die("[ERROR] more than 255 population groups");
        for (size_t i : kv.second) group_id[i] = (uint8_t)group_names.size();
        group_names.push_back(kv.first);
    }

    // ---- outputs
    // a name that ends in ".gz": BGZF blocks + a tabix index beside it (bgzf_tabix.hpp; caller.cpp:242-254), else plain text
    bvamd::TextOut VCF, CVG;
    try { VCF.open(out_vcf); CVG.open(out_cvg); } catch (const std::exception &ex) { die(ex.what()); }
    std::vector<std::string> add_group_info;
    for (const auto &g : group_names)  // caller.cpp:229-236
        add_group_info.push_back("##INFO=<ID=" + g + "_AF,Number=A,Type=Float,Description=\"Allele frequency in the " + g +
                                 " populations calculated base on LRT, in the range (0,1)\">");
    std::string hv = bvamd::vcf_header(reference, reference, contigs, add_group_info, sample_ids) + "\n";
    std::string hc = bvamd::cvg_header() + "\n";
    VCF.write_header(hv);
    CVG.write_header(hc);
    // --deflate device: the whole 0xff00-byte blocks of every batch of lines are compressed by one bv_engine_bgzf_deflate call
    // instead of one zlib deflate() each on the emitter thread (bgzf_tabix.hpp: TextOut::write_lines with a BlockDeflater; the
    // headers and the last partial block of a file stay with zlib).  An engine is not re-entrant and the workers' engines are
    // busy: the emitter thread makes a small one of its own on the first engine's device when its first batch arrives.
    const auto ends_in_gz = [](const std::string &s) { return s.size() > 3 && s.compare(s.size() - 3, 3, ".gz") == 0; };
    bool device_deflate = false;
    if (deflate_arg == "device") {
        device_deflate = ends_in_gz(out_vcf) || ends_in_gz(out_cvg);
        if (!ends_in_gz(out_vcf) || !ends_in_gz(out_cvg))
            std::cerr << "[NOTE] --deflate device applies to *.gz outputs: " << (device_deflate ? (ends_in_gz(out_vcf) ? out_cvg : out_vcf) : "both outputs")
                      << " take" << (device_deflate ? "s" : "") << " the host path" << std::endl;
    }
    uint64_t members_deflated = 0;
    double deflate_s = 0;
    // --emit device: the sample columns of the VCF lines are written by the engine that called the batch, from the rows its text
    // submit left on the device (bv_engine_vcf_format), and a *.vcf.gz is deflated there too (bv_engine_vcf_deflate, at
    // --deflate-level): the planes do not come back and the text does not go up.  Batches of batchfile rows only.
    bool emit_device = emit_arg == "device";
    if (emit_device && from_bam) {
        std::cerr << "[NOTE] --emit device applies to batchfile rows parsed on the device, not to BAM input: the host path is taken" << std::endl;
        emit_device = false;
    }
    const bool vcf_gz = ends_in_gz(out_vcf);
    uint64_t vcf_lines_device = 0;

    // ---- batches are bounded by cells (2^28 cells = 5 x 256 MiB of planes per batch in flight), not by a site count that
    // ignores the row length: a launch carries ~0.1 ms of fill and drain whatever its size, so small batches run the engine
    // in its worst regime (round 2's default was 671 sites at 100 k samples: 0.2 of the large-batch rate).  Per pending
    // site the host keeps the slab row and a SiteText, nothing else.
    // The pipeline below holds up to (G + 1) + (2 G + 2) + G + 1 = 4 G + 4 batches at once (queued, on the engines, waiting for the
    // emitter): the cell budget of a batch shrinks with the number of engines so that all of them together stay under 16 GiB of
    // host planes (8 engines: 2^26.4 cells per batch instead of 2^28, 36 x 0.44 GB).
    if (batch_sites == 0) {
        const size_t pitch = (n_sample + 255) / 256 * 256;
        const size_t in_flight = 4 * devices.size() + 4;
        const size_t budget = std::min<size_t>((size_t)1 << 28, (((size_t)16 << 30) / 5) / in_flight);
        const size_t by_cells = budget / std::max<size_t>(pitch, 1);
        batch_sites = (uint32_t)std::min<size_t>(65536, std::max<size_t>(by_cells, 64));
    }
    // batchfile input: a batch is one block of rows as text, ~10 B per cell.  32 MiB blocks, the size of the host reader's
    // blocks: larger ones left the read tasks waiting on the packing of the few blocks in flight (measured: 512 MiB blocks on
    // 16 threads ran at 0.6 x the host reader's rate).  In flight: 4 G + 7 blocks, far below the planes' 16 GiB budget.
    const size_t text_block_bytes = (size_t)1 << 25;
    std::vector<uint32_t> file_samples;  // samples per batchfile, in batchfile order (the header scan)
    for (size_t f = 0; f < file_sample_count.size(); ++f) file_samples.push_back((uint32_t)file_sample_count[f]);

    // ---- the pipeline: producer (this thread) -> G engine workers -> emitter, results written in batch order
    const size_t G = devices.size();
    // --inflate device: BGZF batchfiles go to the engine compressed (bv_engine_text_parse_bgzf inflates, finds the lines and
    // parses).  There is no producer then: the engine workers take turns at the raw reader -- a worker reads the next runs from
    // the cursors, parses them on its engine, hands the new cursors back and only then lets go of the reader, so its row fetch,
    // host reader, submit and records overlap the next worker's parse.  Anything else keeps the host path.
    bvamd::BgzfRawReader raw;
    bool device_inflate = false;
    if (inflate_arg == "device" && !(from_bam && pileup_arg == "device")) {  // (with --pileup device: the BAM files' own members, below)
        if (from_bam) std::cerr << "[NOTE] --inflate device applies to BGZF batchfiles, not to BAM input: the host path is taken" << std::endl;
        else if (G > 1) std::cerr << "[NOTE] --inflate device runs on one engine (--gpus 1): the host path is taken" << std::endl;
        else if (!raw.open(batchfiles, header_lines)) std::cerr << "[NOTE] --inflate device needs BGZF batchfiles: the host path is taken" << std::endl;
        else device_inflate = true;
    }
    // --pileup device: the samples' raw BAM records of a window go to an engine of the producer's own, which piles them up
    // (bv_engine_pileup), gathers the covered rows and submits them where they lie (bv_engine_pileup_rows / _submit); the host
    // threads only read and inflate.  BAM input on one engine; anything else keeps the host path.
    bool device_pileup = false;
    if (pileup_arg == "device") {
        if (!from_bam) std::cerr << "[NOTE] --pileup device applies to BAM input, not to batchfiles: nothing changes" << std::endl;
        else if (G > 1) std::cerr << "[NOTE] --pileup device runs on one engine (--gpus 1): the host path is taken" << std::endl;
        else device_pileup = true;
    }
    // --pileup device --inflate device: the host threads inflate nothing either -- they read the compressed BGZF members of every
    // sample's fetch and the cut points (host/raw_members.hpp), and the engine inflates and piles up (bv_engine_pileup_bgzf)
    bool bam_inflate_device = false;
    if (from_bam && pileup_arg == "device" && inflate_arg == "device") {
        bam_inflate_device = device_pileup;
        if (!device_pileup) std::cerr << "[NOTE] --inflate device on BAM input runs with --pileup device on one engine: the host threads read and inflate" << std::endl;
        for (size_t i = 0; bam_inflate_device && i < bams.size(); ++i)
            if (!bvamd::bam_members_supported(bams[i])) {
                std::cerr << "[NOTE] --inflate device: the BGZF members of " << bams[i] << " are not of the XLEN = 6 packing: the host threads read and inflate" << std::endl;
                bam_inflate_device = false;
            }
    }
    uint64_t bam_members_inflated = 0, bam_members_bytes = 0;
    uint64_t reads_bytes = 0;
    double pileup_s = 0;
    std::mutex raw_mu;
    bool raw_done = false;
    uint64_t raw_seq = 0;
    size_t raw_target = std::max<size_t>(text_block_bytes / std::max<size_t>(1, batchfiles.size()), 1);
    // batchfile input: three engine workers per GPU -- a text batch has host work on its worker (the rows into pinned staging,
    // the host reader for the positions the device leaves to it, the records and planes back), which the other two overlap
    const size_t W = from_bam ? G : 3 * G;
    BatchQueue to_gpu(W + 1), to_emit(2 * W + 2);
    std::mutex err_mu;
    std::string first_error;
    StageClock clk;
    const double t_start = StageClock::now();
    auto fail = [&](const std::string &m) {
        std::lock_guard<std::mutex> g(err_mu);
        if (first_error.empty()) first_error = m;
    };
    std::vector<std::thread> workers;
    for (size_t w = 0; w < W; ++w)
        workers.emplace_back([&, w]() {
            const size_t g = w % G;
            std::unique_ptr<bvamd::BaseTypeEngine> engine;
            // this worker feeds one GPU: keep it (and the staging memory it touches first) on the CPUs of that GPU's NUMA node
            (void)bv_bind_thread_to_device_node(devices[g]);
            try {
                engine.reset(new bvamd::BaseTypeEngine(batch_sites, (uint32_t)n_sample, user_min_af, devices[g]));
            } catch (const std::exception &ex) { fail(ex.what()); }
            auto host_reader = [](const std::vector<std::string> &r, size_t n, bvamd::SlabBuilder &sb, bvamd::SiteText &st) {
                return bvamd::parse_site_rows_fast(r, n, sb, st);
            };
            // --emit device: heads and gt of the batch's variant records, the lines on this worker's engine, then members or text
            auto emit_on_device = [&](Batch &b) {
                b.emit_device = true;
                std::vector<std::string> heads;
                std::vector<uint8_t> gt;
                for (size_t i = 0; i < b.text.size(); ++i) {
                    if (!b.result.has_variant(i)) continue;
                    std::string head = bvamd::format_vcf_head(b.text[i], b.result.sites[i], group_names.empty() ? nullptr : &b.result.group(i, 0), group_names);
                    if (head.empty()) continue;  // (no ALT: format_vcf_line writes nothing)
                    uint8_t g[4];
                    bvamd::vcf_gt_codes(b.text[i], b.result.sites[i], g);
                    b.vcf_record.push_back((uint32_t)i);
                    heads.push_back(std::move(head));
                    gt.insert(gt.end(), g, g + 4);
                }
                b.vcf_line_off = engine->vcf_format(b.vcf_record, heads, gt);
                const uint64_t total = b.vcf_line_off.back();
                if (total == 0) return;
                if (vcf_gz) {
                    const size_t nb = (size_t)((total + bvamd::BgzfWriter::kBlock - 1) / bvamd::BgzfWriter::kBlock);
                    std::vector<uint64_t> block_off(nb + 1);
                    for (size_t k = 0; k <= nb; ++k) block_off[k] = std::min<uint64_t>(total, (uint64_t)k * bvamd::BgzfWriter::kBlock);
                    b.vcf_members.resize(total + 31 * nb);
                    b.vcf_member_off.assign(nb + 1, 0);
                    engine->vcf_deflate(total, block_off.data(), (uint32_t)nb, b.vcf_members.data(), b.vcf_member_off.data(), deflate_level);
                    b.vcf_members.resize(b.vcf_member_off[nb]);
                } else {
                    b.vcf_text.resize(total);
                    engine->vcf_fetch(&b.vcf_text[0], total);
                }
            };
            while (device_inflate && engine) {
                BatchPtr b;
                bvamd::BaseTypeEngine::BgzfParse bp;
                {
                    std::lock_guard<std::mutex> lk(raw_mu);
                    if (raw_done) break;
                    {
                        std::lock_guard<std::mutex> g2(err_mu);
                        if (!first_error.empty()) { raw_done = true; break; }
                    }
                    std::string error;
                    bvamd::BgzfRawRuns runs;
                    try {
                        const double t0 = StageClock::now();
                        raw.next(runs, raw_target);
                        const double t1 = StageClock::now();
                        const bv_bgzf_rows rows{runs.data.data(), runs.member_off.data(), runs.data.size(), runs.file_member.data(), file_samples.data(),
                                                runs.skip_bytes.data(), runs.skip_lines.data(), (uint32_t)file_samples.size(), batch_sites,
                                                runs.at_end ? 1u : 0u, 0};
                        bp = engine->parse_bgzf(rows, batch_sites, group_names.empty() ? nullptr : group_id.data(), (uint32_t)group_names.size());
                        const double t2 = StageClock::now();
                        std::lock_guard<std::mutex> g2(err_mu);
                        clk.read += t1 - t0;
                        clk.engine += t2 - t1;
                    } catch (const bvamd::BaseTypeEngine::BgzfDataError &ex) {
                        // the message the host reader has for such a file
                        error = std::strstr(ex.what(), "bad header") ? "[ERROR] not a BGZF member where one was expected (truncated or damaged batchfile)"
                                                                    : "[ERROR] a BGZF member does not inflate to its recorded size";
                    } catch (const std::exception &ex) { error = ex.what(); }
                    if (error.empty() && bp.n_positions == 0) {
                        if (runs.at_end) { raw_done = true; break; }
                        raw_target *= 2;  // not one complete row in every run: longer runs
                        continue;
                    }
                    b.reset(new Batch((uint32_t)n_sample));
                    b->from_text = true;
                    b->seq = raw_seq++;
                    if (!error.empty()) {
                        b->error = error;
                        raw_done = true;
                    } else {
                        std::vector<uint32_t> cm(bp.cursor.size()), co(bp.cursor.size());
                        for (size_t f = 0; f < bp.cursor.size(); ++f) { cm[f] = bp.cursor[f].member; co[f] = bp.cursor[f].offset; }
                        raw.advance(runs, cm.data(), co.data());
                    }
                }
                if (b->error.empty()) {
                    const double t0 = StageClock::now();
                    try {
                        auto tb = engine->finish_bgzf(bp, file_samples.data(), file_samples.size(), host_reader, (uint32_t)group_names.size(), !emit_device);
                        b->result = std::move(tb.batch);
                        b->text = std::move(tb.text);
                        b->cell = std::move(tb.cell);
                        b->phred = std::move(tb.phred);
                        if (emit_device) emit_on_device(*b);
                        if (tb.error) {
                            try { std::rethrow_exception(tb.error); } catch (const std::exception &ex) { b->error = ex.what(); }
                        }
                    } catch (const std::exception &ex) { b->error = ex.what(); b->text.clear(); b->emit_device = false; }
                    const double dt = StageClock::now() - t0;
                    std::lock_guard<std::mutex> lk(err_mu);
                    clk.engine += dt;
                }
                to_emit.push(std::move(b));
            }
            for (BatchPtr b; (b = to_gpu.pop());) {
                if (engine) {
                    const double t0 = StageClock::now();
                    if (b->from_text) {
                        // the device parses the rows; the positions it leaves to the host go to the host reader in between
                        try {
                            const bv_text_rows rows{b->rows.data(), b->row_off.data(), file_samples.data(), b->rows.size(), b->n_positions,
                                                    (uint32_t)file_samples.size(), 0};
                            auto tb = engine->lrt_text(rows, host_reader, group_names.empty() ? nullptr : group_id.data(), (uint32_t)group_names.size(),
                                                       !emit_device);
                            b->result = std::move(tb.batch);
                            b->text = std::move(tb.text);
                            b->cell = std::move(tb.cell);
                            b->phred = std::move(tb.phred);
                            if (emit_device) emit_on_device(*b);
                            if (tb.error) {
                                try { std::rethrow_exception(tb.error); } catch (const std::exception &ex) { b->error = ex.what(); }
                            }
                        } catch (const std::exception &ex) { b->error = ex.what(); b->text.clear(); b->emit_device = false; }
                        std::string().swap(b->rows);
                    } else {
                        // (the producer's choice of layout: short reads -> the rank words carry the calls, basetype_gpu.hpp)
                        try { b->slab.tag_ranks(); b->result = engine->lrt(b->slab); } catch (const std::exception &ex) { b->error = ex.what(); }
                    }
                    const double dt = StageClock::now() - t0;
                    std::lock_guard<std::mutex> lk(err_mu);
                    clk.engine += dt;
                } else {
                    b->error = "no engine on device " + std::to_string(devices[g]);
                }
                to_emit.push(std::move(b));
            }
        });
    size_t n_sites = 0, n_variants = 0;
    std::thread emitter([&]() {
        std::map<uint64_t, BatchPtr> waiting;  // finished out of order
        std::unique_ptr<bvamd::BaseTypeEngine> deflate_engine;
        const bvamd::BlockDeflater deflate = [&](const char *text, uint64_t text_bytes, const uint64_t *block_off, uint32_t n_blocks, uint8_t *dst,
                                                 uint64_t *member_off) {
            const double t0 = StageClock::now();
            if (!deflate_engine) deflate_engine.reset(new bvamd::BaseTypeEngine(1, 1, user_min_af, devices[0]));
            deflate_engine->bgzf_deflate(text, text_bytes, block_off, n_blocks, dst, member_off, deflate_level);
            members_deflated += n_blocks;
            deflate_s += StageClock::now() - t0;
        };
        uint64_t next_seq = 0;
        bool stopped = false;  // a batch failed: nothing behind it is written
        for (BatchPtr b; (b = to_emit.pop());) {
            waiting[b->seq] = std::move(b);
            for (auto it = waiting.find(next_seq); it != waiting.end(); it = waiting.find(next_seq)) {
                Batch &d = *it->second;
                // (a text batch whose host reader refused a position: its records before that position are written first)
                if (stopped) {
                } else if (!d.error.empty() && !d.from_text) {
                    stopped = true;
                    fail(d.error);
                } else {
                    const double t0 = StageClock::now();
                    // the lines of a batch are formatted by `--thread` threads (ranges of consecutive sites, a text buffer each)
                    // and written in site order
                    const size_t nt = (size_t)std::max(1, threads);
                    std::vector<std::string> cvg_txt(nt), vcf_txt(nt);
                    std::vector<size_t> nv(nt, 0);
                    parallel_ranges(d.text.size(), threads, [&](size_t t, size_t lo, size_t hi) {
                        for (size_t i = lo; i < hi; ++i) {
                            cvg_txt[t] += bvamd::format_cvg_line(d.text[i], d.result.sites[i]);
                            if (d.emit_device) continue;  // (the VCF lines are there already)
                            if (d.result.has_variant(i)) {
                                vcf_txt[t] += bvamd::format_vcf_line(d.text[i], d.cell_row(i, n_sample), d.phred_row(i, n_sample), n_sample, d.result.sites[i],
                                                                     group_names.empty() ? nullptr : &d.result.group(i, 0), group_names);
                                ++nv[t];
                            }
                        }
                    });
                    try {
                        if (d.emit_device) {
                            // the CVG lines as ever, the VCF lines as the worker's engine left them
                            for (size_t t = 1; t < nt; ++t) { cvg_txt[0] += cvg_txt[t]; std::string().swap(cvg_txt[t]); }
                            if (device_deflate) CVG.write_lines(cvg_txt[0], deflate);
                            else CVG.write_lines(cvg_txt[0]);
                            std::string().swap(cvg_txt[0]);
                            if (vcf_gz) {
                                std::vector<std::pair<std::string, int64_t>> keys;
                                for (uint32_t i : d.vcf_record) keys.emplace_back(d.text[i].ref_id, (int64_t)d.text[i].ref_pos);
                                VCF.write_members(d.vcf_members.data(), d.vcf_member_off.data(), d.vcf_member_off.empty() ? 0 : d.vcf_member_off.size() - 1,
                                                  d.vcf_line_off.data(), keys);
                            } else {
                                VCF.write_lines(d.vcf_text);
                            }
                            for (size_t i = 0; i < d.text.size(); ++i) nv[0] += d.result.has_variant(i) ? 1 : 0;
                            vcf_lines_device += d.vcf_record.size();
                        } else if (device_deflate) {
                            // one call a file and batch: a call takes as long as its slowest block, however few blocks it has
                            for (size_t t = 1; t < nt; ++t) {
                                cvg_txt[0] += cvg_txt[t]; std::string().swap(cvg_txt[t]);
                                vcf_txt[0] += vcf_txt[t]; std::string().swap(vcf_txt[t]);
                            }
                            CVG.write_lines(cvg_txt[0], deflate);
                            VCF.write_lines(vcf_txt[0], deflate);
                        }
                        for (size_t t = 0; t < nt; ++t) {
                            if (!device_deflate && !d.emit_device) {
                                CVG.write_lines(cvg_txt[t]);
                                VCF.write_lines(vcf_txt[t]);
                            }
                            n_variants += nv[t];
                        }
                    } catch (const std::exception &ex) { fail(ex.what()); }
                    n_sites += d.text.size();
                    clk.emit += StageClock::now() - t0;
                    if (!d.error.empty()) { stopped = true; fail(d.error); }
                }
                waiting.erase(it);
                ++next_seq;
            }
        }
    });

    uint64_t seq = 0;
    BatchPtr cur;
    auto fresh = [&]() {
        cur.reset(new Batch((uint32_t)n_sample));
        if (!from_bam) cur->slab.reserve_rows(batch_sites);  // (address space; the pages come as the rows do -- no regrowth copies)
        if (!group_names.empty()) cur->slab.set_groups(group_id, (uint32_t)group_names.size());
        cur->seq = seq++;
    };
    auto ship = [&]() {
        if (cur && cur->slab.n_sites()) to_gpu.push(std::move(cur));
        else if (cur) --seq;
        cur.reset();
    };
    auto still_ok = [&]() { std::lock_guard<std::mutex> g(err_mu); return first_error.empty(); };

    try {
        if (from_bam) {
            // ---- pileup windows -> slab rows, straight from the tile planes (no text round trip); a site is a position that
            // at least one sample covers (the reference skips rows of total depth 0, caller.cpp:718)
            std::vector<std::string> region_list;  // "-r chr:beg-end[,chr:beg-end ...]" (caller.cpp:311-356), in the order given
            region_list = bvamd::pieces(regions, ',');
            std::string fa_seq, fa_of;
            std::unique_ptr<bvamd::BaseTypeEngine> pileup_engine;  // --pileup device
            std::unique_ptr<bvamd::BamPool> pileup_pool;
            for (const std::string &rg : region_list) {
                const size_t colon = rg.rfind(':'), dash = rg.rfind('-');
                if (colon == std::string::npos || dash == std::string::npos || dash < colon) die("--regions wants CHR:BEG-END[,CHR:BEG-END...]");
                const std::string ref_id = rg.substr(0, colon);
                const uint32_t beg = (uint32_t)std::stoul(rg.substr(colon + 1, dash - colon - 1));
                const uint32_t end = (uint32_t)std::stoul(rg.substr(dash + 1));
                if (fa_of != ref_id) { fa_seq = bvamd::load_fasta_sequence(reference, ref_id); fa_of = ref_id; }
                if (beg < 1 || end < beg || end > fa_seq.size()) die("[ERROR] region outside " + ref_id);
                if (device_pileup) {
                    if (!pileup_engine) pileup_engine.reset(new bvamd::BaseTypeEngine(batch_sites, (uint32_t)n_sample, user_min_af, devices[0]));
                    if (!pileup_pool) pileup_pool.reset(new bvamd::BamPool(bams, true));
                    bv_engine *pe = pileup_engine->handle();
                    auto check = [&](int rc) { if (rc != BV_OK) throw std::runtime_error(bv_last_error(pe)); };
                    check(bv_engine_pileup_set_reference(pe, fa_seq.data(), fa_seq.size()));
                    const uint32_t window = std::min<uint32_t>(bvamd::pileup_window(bams.size()), bv_pileup_max_rows());
                    for (uint32_t sb = beg; sb <= end && still_ok(); sb += bvamd::PILEUP_STEP) {
                        const uint32_t se = std::min(end, sb + bvamd::PILEUP_STEP - 1);
                        for (uint32_t wb = sb; wb <= se && still_ok(); wb += window) {
                            const uint32_t we = std::min(se, wb + window - 1);
                            // every sample's records of the fetch, undecoded, on `--thread` threads
                            const double tr0 = StageClock::now();
                            bvamd::WindowReads reads;
                            bvamd::WindowMembers wm;
                            if (bam_inflate_device) bvamd::read_window_members(*pileup_pool, bams, ref_id, wb, we, threads, wm);
                            else bvamd::read_window_raw(*pileup_pool, bams, ref_id, wb, we, threads, reads);
                            const double tp0 = StageClock::now();
                            clk.read += tp0 - tr0;
                            uint32_t n_cov = 0;
                            if (bam_inflate_device) {
                                if (wm.plan.runs.empty()) { if (we == UINT32_MAX) break; continue; }
                                static_assert(sizeof(bvamd::MemberRun) == sizeof(bv_pileup_bgzf_run), "one run layout");
                                bv_pileup_bgzf in{};
                                in.members.data = wm.plan.data.data(); in.members.member_off = wm.plan.member_off.data(); in.members.data_bytes = wm.plan.data.size();
                                in.members.n_members = (uint32_t)wm.plan.member_pos.size();
                                in.runs = reinterpret_cast<const bv_pileup_bgzf_run *>(wm.plan.runs.data());
                                in.pitch = (n_sample + 15) / 16 * 16; in.n_runs = (uint32_t)wm.plan.runs.size(); in.n_samples = (uint32_t)n_sample;
                                in.tid = wm.tid; in.region_beg = beg; in.region_end = end; in.beg = wb; in.end = we; in.mapq_thd = mapq_thd;
                                bam_members_inflated += in.members.n_members; bam_members_bytes += in.members.data_bytes;
                                check(bv_engine_pileup_bgzf(pe, &in, &n_cov, nullptr));
                            } else {
                                reads_bytes += reads.records.size();
                                if (reads.run_sample.empty()) { if (we == UINT32_MAX) break; continue; }
                                bv_pileup_reads in{};
                                in.records = reads.records.data(); in.run_off = reads.run_off.data(); in.run_sample = reads.run_sample.data();
                                in.pitch = (n_sample + 15) / 16 * 16; in.n_runs = (uint32_t)reads.run_sample.size(); in.n_samples = (uint32_t)n_sample;
                                in.tid = reads.tid; in.region_beg = beg; in.region_end = end; in.beg = wb; in.end = we; in.mapq_thd = mapq_thd;
                                in.mem_kind = BV_MEM_HOST;
                                check(bv_engine_pileup(pe, &in, &n_cov, nullptr));
                            }
                            std::vector<uint32_t> pos(n_cov), depth(n_cov);
                            bv_slab slab;
                            // (short reads: the rank words carry the calls, as SlabBuilder::tag_ranks chooses on the host path)
                            if (bv_engine_pileup_rows(pe, 1, &slab, pos.data(), depth.data()) != BV_OK) check(bv_engine_pileup_rows(pe, 0, &slab, pos.data(), depth.data()));
                            bv_pileup_result res{};
                            res.mem_kind = BV_MEM_HOST;
                            check(bv_engine_pileup_fetch(pe, &res, nullptr));  // (no buffers: the sizes)
                            std::vector<bv_pileup_token> tokens(res.n_tokens);
                            std::vector<uint8_t> token_text(res.text_bytes);
                            res.tokens = tokens.data(); res.text = token_text.data();
                            res.tokens_capacity = tokens.size(); res.text_capacity = token_text.size();
                            check(bv_engine_pileup_fetch(pe, &res, nullptr));
                            pileup_s += StageClock::now() - tp0;
                            clk.parse += StageClock::now() - tp0;
                            size_t next_token = 0;
                            for (uint32_t first = 0; first < n_cov && still_ok(); first += batch_sites) {
                                const uint32_t rows = std::min(batch_sites, n_cov - first);
                                BatchPtr b(new Batch((uint32_t)n_sample));
                                b->seq = seq++;
                                b->from_text = true;  // (its cell / phred rows come back beside the records)
                                b->result.sites.resize(rows);
                                b->result.n_groups = (uint32_t)group_names.size();
                                b->result.groups.resize((size_t)rows * group_names.size());
                                b->cell.resize((size_t)rows * n_sample);
                                b->phred.resize((size_t)rows * n_sample);
                                const double te0 = StageClock::now();
                                check(bv_engine_pileup_submit(pe, first, rows, group_names.empty() ? nullptr : group_id.data(), (uint32_t)group_names.size(),
                                                              b->result.sites.data(), group_names.empty() ? nullptr : b->result.groups.data(), b->cell.data(),
                                                              b->phred.data(), nullptr));
                                {
                                    std::lock_guard<std::mutex> lk(err_mu);
                                    clk.engine += StageClock::now() - te0;
                                }
                                for (uint32_t k = 0; k < rows; ++k) {
                                    bvamd::SiteText st;
                                    st.ref_id = ref_id; st.ref_pos = pos[first + k]; st.ref_base = std::string(1, fa_seq[st.ref_pos - 1]);
                                    while (next_token < tokens.size() && tokens[next_token].pos < st.ref_pos) ++next_token;
                                    for (; next_token < tokens.size() && tokens[next_token].pos == st.ref_pos; ++next_token)
                                        st.indel_tokens.emplace_back(reinterpret_cast<const char *>(token_text.data()) + tokens[next_token].text_off, tokens[next_token].text_len);
                                    b->text.push_back(std::move(st));
                                }
                                to_emit.push(std::move(b));
                            }
                            if (we == UINT32_MAX) break;
                        }
                        if (se == UINT32_MAX) break;
                    }
                    continue;
                }
                const double tp0 = StageClock::now();
                bvamd::pileup_region(bams, fa_seq, ref_id, beg, end, mapq_thd, true, threads, [&](const bvamd::PileupTile &t) {
                    size_t next_indel = 0;
                    for (uint32_t pos = t.beg; pos <= t.end && still_ok(); ++pos) {
                        if (t.depth[pos - t.beg] == 0) continue;
                        if (!cur) fresh();
                        const size_t k = t.at(pos, 0);
                        const char rb = fa_seq[pos - 1];
                        cur->slab.add_row(&t.cell[k], &t.qual[k], &t.mapq[k], &t.rank[k],
                                          (uint8_t)bvamd::base_code((char)std::toupper((unsigned char)rb)));
                        bvamd::SiteText st;
                        st.ref_id = ref_id; st.ref_pos = pos; st.ref_base = std::string(1, rb);
                        while (next_indel < t.indels.size() && t.indels[next_indel].pos < pos) ++next_indel;
                        for (; next_indel < t.indels.size() && t.indels[next_indel].pos == pos; ++next_indel)
                            st.indel_tokens.push_back(t.indels[next_indel].text);
                        cur->text.push_back(std::move(st));
                        if (cur->slab.n_sites() == batch_sites) ship();
                    }
                });
                clk.parse += StageClock::now() - tp0;
            }
        } else if (device_inflate) {
            // (the engine workers read the files themselves: see `raw` above)
        } else {
            // ---- one row from every batchfile per position (caller.cpp:586-611), on `--thread` host threads: files read and
            // positions parsed in blocks by a pipeline of tasks (batch_producer.hpp), joined here in position order
            // Every block goes to the engines as its rows' text: the device parses them (bv_engine_text_parse), the engine worker
            // re-reads with the host reader only the positions the device leaves to it.  A block is one batch; text is about twice
            // the 5 B per cell of planes, so a batch carries half the cells of the planes' budget.
            bvamd::BatchfileProducer producer(readers, first_row, have_row, n_sample, threads);
            producer.set_paths(batchfiles, header_lines);  // BGZF files (what the reference writes): members inflated in parallel
            try {
                producer.run_text([&](std::string &rows, std::vector<uint64_t> &row_off, size_t n_positions) {
                    fresh();
                    cur->from_text = true;
                    cur->rows.swap(rows);
                    cur->row_off.swap(row_off);
                    cur->n_positions = (uint32_t)n_positions;
                    to_gpu.push(std::move(cur));
                    return still_ok();
                }, text_block_bytes, batch_sites);
            } catch (...) {
                clk.read += producer.clock.read; clk.parse += producer.clock.parse;
                throw;
            }
            clk.read += producer.clock.read; clk.parse += producer.clock.parse;
        }
        ship();
    } catch (const std::exception &ex) { fail(ex.what()); }
    to_gpu.close();
    for (auto &w : workers) w.join();
    to_emit.close();
    emitter.join();
    try { VCF.close(); CVG.close(); } catch (const std::exception &ex) { if (first_error.empty()) first_error = ex.what(); }
    if (!first_error.empty()) die(first_error);
    const double total = StageClock::now() - t_start;
    std::cout << "[INFO] bv_call: " << n_sites << " covered positions, " << n_variants << " VCF records, " << n_sample
              << " samples, " << group_names.size() << " groups, " << G << " engine(s)" << std::endl;
    // stage seconds: read / parse+pack summed over the producer's threads (BAM input: pileup + pack on the producer thread, all under
    // "parse"), engine summed over the workers (staging copies + kernels + records back), emit on the emitter thread; the
    // stages overlap, total is wall time
    char line[512];
    std::snprintf(line, sizeof line,
                  "[INFO] -- %.3f s elapsed, %.1f sites/s: read %.3f s, parse+pack %.3f s (%s; thread-seconds), engine %.3f s (%zu worker(s), batches of %u sites), emit %.3f s",
                  total, total > 0 ? n_sites / total : 0.0, clk.read, clk.parse, from_bam ? "pileup" : "batchfile", clk.engine, W, batch_sites, clk.emit);
    std::cout << line << std::endl;
    if (!timing_file.empty()) {
        std::ofstream tf(timing_file);
        tf << "{\"sites\": " << n_sites << ", \"vcf_records\": " << n_variants << ", \"samples\": " << n_sample << ", \"engines\": " << G
           << ", \"batch_sites\": " << batch_sites << ", \"input\": \"" << (from_bam ? "bam" : "batchfile") << "\", \"parser\": \""
           << (from_bam ? "pileup" : "batchfile") << "\", \"total_s\": " << total << ", \"sites_per_s\": " << (total > 0 ? n_sites / total : 0.0)
           << ", \"read_s\": " << clk.read << ", \"parse_pack_s\": " << clk.parse << ", \"engine_s\": " << clk.engine
           << ", \"emit_s\": " << clk.emit;
        // --inflate device: members handed to the device (those that hold a partial last row, and the surplus rows of longer
        // runs, are inflated again with the next batch) against the members the files hold
        if (device_inflate)
            tf << ", \"inflate\": \"device\", \"members_inflated\": " << raw.members_handed << ", \"members_in_files\": " << raw.members_passed;
        // --deflate device: whole output blocks compressed by the device, and the emitter's seconds inside those calls (part of emit_s)
        if (device_deflate) tf << ", \"deflate\": \"device\", \"deflate_level\": \"" << deflate_level_arg << "\", \"members_deflated\": " << members_deflated << ", \"deflate_s\": " << deflate_s;
        // --emit device: VCF lines whose sample columns the engines wrote (all of them, on batchfile input)
        if (emit_device) tf << ", \"emit\": \"device\", \"vcf_lines_device\": " << vcf_lines_device;
        // --pileup device: bytes of raw BAM records handed to the engine, and the producer's seconds inside the pileup calls (part of parse_pack_s)
        if (device_pileup) tf << ", \"pileup\": \"device\", \"reads_bytes\": " << reads_bytes << ", \"pileup_s\": " << pileup_s;
        // ... --inflate device with it: the BAM files' compressed members handed to the engine instead, and their bytes
        if (bam_inflate_device) tf << ", \"bam_inflate\": \"device\", \"members_inflated\": " << bam_members_inflated << ", \"members_bytes\": " << bam_members_bytes;
        tf << "}\n";
    }
    return 0;
}
