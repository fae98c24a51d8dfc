// bv_call.cpp -- calling phase of `basevar basetype` on the GPU engine: reference-format
// batchfiles in, reference-format VCF + CVG text out.  It is the composition of the rows either
// side of the hot path: batchfile rows -> BatchInfo
// (batchfile.hpp) -> slab -> engine (C ABI) -> VCF/CVG lines (vcf_emit.hpp), following
// _variant_calling_unit (src/basetype_caller.cpp:529-635), with `--pop-group` handled as
// _get_popgroup_info does (src/basetype_caller.cpp:372-410).
//
// Pipeline (call_pipeline.hpp has the stages): the main thread runs one producer of batches of sites in genomic order; `--gpus G`
// engine workers, one engine on one GPU each, take whichever batch is next; an emitter thread writes the results in batch
// order.  It replaces the reference's fan-out of 100 kb sub-regions over a thread pool and its ordered merge of per-task files
// (_variants_discovery + merge_file_by_line, src/basetype_caller.cpp:469-525).  This file is the command line around them:
// options -> checks -> headers, pop-groups, outputs -> routes -> context -> threads -> producer -> report.
//
//   bv_call --batchfiles a.bf.gz,b.bf.gz --output-vcf out.vcf --output-cvg out.cvg
//           [--pop-group FILE] [--min-af 0.01] [--batch-sites N (default: 2^28 cells / samples, at most 65536)]
//           [--timing FILE.json] [--inflate device|host] [--deflate device|host] [--deflate-level fast|small] [--emit device|host]
//           [--pileup device|host]   (BAM input; with it, --inflate device also hands the BAM files' BGZF members to the engine compressed)
//           [--gpus G] [--devices 0,1,... | --device 0]
//           [--reference ref.fa --contig NAME:LENGTH ...]
//           [--regions CHR[:BEG[-END]][,...]]   (batchfile input: the regions in the order given, each from where the file's .tbi
//                                                says it may begin -- a seek, not a scan)
//           [--files-per-pass K]   (batchfile input: the files are read K at a time, a window of --batch-sites positions at a
//                                   time, and parsed as one job per window -- never more than K batchfiles are open, so a
//                                   cohort may have more files than the process may hold descriptors; one engine, host inflate,
//                                   no --regions; INTEGRATION.md section 2q.  The window's default is the plane budget's:
//                                   2^28 cells / samples, at most 65536 -- the text-block size of the default route does not cut it)
//   bv_call -I a.bam [-I b.bam ...] [-L bam.list] -R ref.fa[.gz] --regions CHR:BEG-END[,CHR:BEG-END...] [--mapq 10]
//           [--thread T] ...   (same outputs)
//
// Batchfiles may be bgzip/gzip-compressed or plain (zlib reads all three).  With BAM inputs the pileup
// (pileup.hpp) feeds the engine directly: the same cells the batchfile rows would carry,
// without the text round trip.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "call_pipeline.hpp"

namespace {

using bvamd::StageClock;

[[noreturn]] void die(const std::string &m) {
    std::cerr << m << std::endl;
    std::exit(1);
}

struct Options {
    std::vector<std::string> batchfiles, bams;
    std::string out_vcf, out_cvg, pop_group_file, reference = ".", regions, bam_list, devices_arg, timing_file, inflate = "host", deflate = "host",
                deflate_level = "fast", emit = "host", pileup = "host", indel_tokens = "host";
    int mapq_thd = 10, threads = 4, n_gpus = 1, device = 0;  // (`-t`: 4, the reference's default, src/basetype_utils.h:33,94)
    std::vector<bvamd::Contig> contigs;
    float user_min_af = 0.01f;  // BaseTypeARGS default, src/basetype_utils.h:94
    uint32_t batch_sites = 0;   // 0 = from a cell budget once the sample count is known
    uint32_t files_per_pass = 0;  // batchfile input: > 0 reads the files file-major, this many at a time (file_major.hpp)
    size_t fm_passes = 0, fm_max_open = 0;  // ... what that route counted, for --timing
    // what validate() makes of them
    std::vector<int> devices;            // one engine per entry
    std::vector<bvamd::Region> region_list;
    std::vector<bvamd::BatchRegion> batch_regions;  // --regions on batchfile input
    bool from_bam() const { return !bams.empty(); }
};

Options parse_options(int argc, char **argv) {
    Options o;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) die("missing value for " + a); return argv[++i]; };
        if (a == "--batchfiles") o.batchfiles = bvamd::pieces(next(), ',');
        else if (a == "--output-vcf") o.out_vcf = next();
        else if (a == "--output-cvg") o.out_cvg = next();
        else if (a == "--pop-group") o.pop_group_file = next();
        else if (a == "--min-af") o.user_min_af = std::stof(next());
        else if (a == "--batch-sites") o.batch_sites = (uint32_t)std::stoul(next());
        else if (a == "--files-per-pass") {
            o.files_per_pass = (uint32_t)std::stoul(next());
            if (o.files_per_pass == 0) die("[ERROR] --files-per-pass wants a number >= 1");
        }
        else if (a == "--timing") o.timing_file = next();
        else if (a == "--inflate") o.inflate = next();
        else if (a == "--deflate") o.deflate = next();
        else if (a == "--deflate-level") o.deflate_level = next();
        else if (a == "--emit") o.emit = next();
        else if (a == "--pileup") o.pileup = next();
        else if (a == "--indel-tokens") o.indel_tokens = next();
        else if (a == "--device") o.device = std::stoi(next());
        else if (a == "--gpus") o.n_gpus = std::stoi(next());
        else if (a == "--devices") o.devices_arg = next();
        else if (a == "--reference" || a == "-R") o.reference = next();
        else if (a == "-I" || a == "--input") o.bams.push_back(next());
        else if (a == "-L" || a == "--align-file-list") o.bam_list = next();
        else if (a == "-r" || a == "--regions") o.regions = next();
        else if (a == "-q" || a == "--mapq") o.mapq_thd = std::stoi(next());
        else if (a == "-t" || a == "--thread") o.threads = std::stoi(next());
        else if (a == "--contig") {
            const std::vector<std::string> p = bvamd::pieces(next(), ':');
            if (p.size() != 2) die("--contig wants NAME:LENGTH");
            o.contigs.push_back({p[0], (uint32_t)std::stoul(p[1])});
        } else die("unknown argument " + a);
    }
    return o;
}

void validate(Options &o) {
    if (!o.bam_list.empty() && !bvamd::read_first_column(o.bam_list, o.bams)) die("[ERROR] cannot open " + o.bam_list);
    if (!(o.user_min_af > 0.f)) die("[ERROR] --min-af must be > 0");  // the reference refuses it too (caller.cpp:73)
    if (o.n_gpus < 1) die("[ERROR] --gpus must be >= 1");
    if (o.inflate != "host" && o.inflate != "device") die("[ERROR] --inflate wants device or host");
    if (o.deflate != "host" && o.deflate != "device") die("[ERROR] --deflate wants device or host");
    if (o.deflate_level != "fast" && o.deflate_level != "small") die("[ERROR] --deflate-level wants fast or small");
    if (o.emit != "host" && o.emit != "device") die("[ERROR] --emit wants device or host");
    if (o.pileup != "host" && o.pileup != "device") die("[ERROR] --pileup wants device or host");
    if (o.indel_tokens != "host" && o.indel_tokens != "device") die("[ERROR] --indel-tokens wants device or host");
    // (the host path is zlib at its own level: the device encoder's levels do not apply to it)
    if (o.deflate_level != "fast" && o.deflate != "device") die("[ERROR] --deflate-level small needs --deflate device");
    // one engine per entry: --devices a,b,... (an ordinal may repeat: several engines on one GPU), else device, device+1, ...
    if (!o.devices_arg.empty()) {
        for (const auto &x : bvamd::pieces(o.devices_arg, ',')) o.devices.push_back(std::stoi(x));
        if (o.n_gpus != 1 && (size_t)o.n_gpus != o.devices.size()) die("[ERROR] --gpus and --devices disagree");
    } else {
        for (int g = 0; g < o.n_gpus; ++g) o.devices.push_back(o.device + g);
    }
    if ((o.batchfiles.empty() && !o.from_bam()) || o.out_vcf.empty() || o.out_cvg.empty() || (o.from_bam() && (o.regions.empty() || o.reference == ".")))
        die("usage: bv_call (--batchfiles a,b,... | -I a.bam [-I ...] -R ref.fa --regions CHR:BEG-END [--mapq Q]) --output-vcf FILE "
            "--output-cvg FILE [--pop-group FILE] [--min-af F] [--gpus G]");
    // --files-per-pass: batchfiles, whole files, one engine, inflated on the host
    if (o.files_per_pass) {
        if (o.from_bam()) die("[ERROR] --files-per-pass applies to batchfile input, not to BAM input");
        if (!o.regions.empty()) die("[ERROR] --files-per-pass with --regions is not built: the file-major route reads whole files");
        if (o.devices.size() > 1) {
            std::cerr << "[NOTE] --files-per-pass runs on one engine: device " << o.devices[0] << " is taken" << std::endl;
            o.devices.resize(1);
        }
        if (o.inflate == "device") {
            std::cerr << "[NOTE] --files-per-pass reads and inflates on the host: --inflate host is taken" << std::endl;
            o.inflate = "host";
        }
    }
    // "-r chr:beg-end[,chr:beg-end ...]" (caller.cpp:311-356): the syntax here, before any engine exists; whether a region lies
    // inside its contig takes the contig's sequence (for_each_bam_region)
    for (const std::string &rg : o.from_bam() ? bvamd::pieces(o.regions, ',') : std::vector<std::string>()) {
        bvamd::Region r;
        if (!bvamd::parse_region(rg, r)) die("--regions wants CHR:BEG-END[,CHR:BEG-END...]");
        o.region_list.push_back(r);
    }
    // batchfile input: "CHR", "CHR:BEG", "CHR:BEG-END" as tabix reads them (the list is cut at commas, so numbers carry none).
    // With --inflate device the rows are selected on the device, where the inflated text lies
    // (bv_engine_text_parse_bgzf_region); the host reader selects them by the same definition.
    for (const std::string &rg : !o.from_bam() && !o.regions.empty() ? bvamd::pieces(o.regions, ',') : std::vector<std::string>()) {
        bvamd::BatchRegion r;
        if (!bvamd::parse_batch_region(rg, r)) die("[ERROR] --regions on batchfiles wants CHR, CHR:BEG or CHR:BEG-END (1 <= BEG <= END <= 2^29), not '" + rg + "'");
        o.batch_regions.push_back(r);
    }
    // a *.gz output is indexed as it is written, which takes sorted lines: the regions of a contig together, ascending, apart
    if (bvamd::ends_in_gz(o.out_vcf) || bvamd::ends_in_gz(o.out_cvg)) {
        for (size_t i = 0; i < o.batch_regions.size(); ++i)
            for (size_t j = 0; j < i; ++j) {
                const bvamd::BatchRegion &a = o.batch_regions[j], &b = o.batch_regions[i];
                if (a.name != b.name) continue;
                if (o.batch_regions[i - 1].name != b.name || a.end >= b.beg)
                    die("[ERROR] --regions with a *.gz output: the regions of " + b.name + " must stand together, ascending and without overlap ('" +
                        b.name + ":" + std::to_string(b.beg) + "-" + std::to_string(b.end) + "' does not)");
            }
    }
}

// --regions on batchfiles: every file's index, read before any engine exists.  A file without one, and a plain or plain-gzip
// file (no virtual offset leads into it), is scanned from its first row for every region (one note for all of them); a contig
// that no index knows fails as the reference does (caller.cpp:566).
void load_region_indexes(const Options &o, const bvamd::BatchfileHeaders &headers, bvamd::RegionIndexes &idx) {
    const size_t F = o.batchfiles.size();
    idx.index.resize(F);
    idx.indexed.assign(F, 0);
    idx.header_lines = headers.header_lines;
    std::string scanned;
    for (size_t f = 0; f < F; ++f) {
        unsigned char h[18];
        std::FILE *fp = std::fopen(o.batchfiles[f].c_str(), "rb");
        const bool bgzf = fp && std::fread(h, 1, 18, fp) == 18 && bvamd::bgzf_member_header(h);
        if (fp) std::fclose(fp);
        try { idx.indexed[f] = bgzf && idx.index[f].load(o.batchfiles[f] + ".tbi") ? 1 : 0; } catch (const std::exception &ex) { die(ex.what()); }
        if (!idx.indexed[f]) scanned += (scanned.empty() ? "" : ", ") + o.batchfiles[f];
    }
    if (!scanned.empty()) std::cerr << "[NOTE] --regions: no .tbi beside " << scanned << " (or no BGZF file): scanned from the first row for every region" << std::endl;
    for (const bvamd::BatchRegion &rg : o.batch_regions)
        for (size_t f = 0; f < F; ++f) {
            uint64_t voff = 0;
            if (idx.indexed[f] && idx.index[f].query(rg.name, rg.beg, rg.end, &voff) == bvamd::TabixReader::UNKNOWN_NAME)
                die("[ERROR] load data in " + rg.name + ":" + std::to_string(rg.beg) + "-" + std::to_string(rg.end) + " failed. Check input file: " + o.batchfiles[f]);
        }
}

// Pop groups (caller.cpp:372-410): sample -> group, later rows override; groups iterate by name
void read_pop_groups(const std::string &path, bvamd::CallContext &ctx) {
    std::map<std::string, std::vector<size_t>> groups_idx;
    if (!path.empty()) {
        std::ifstream in(path);
        if (!in) die("[ERROR] Cannot open file: " + path);
        std::map<std::string, std::string> sample2group;
        std::string sn, gn, skip;
        while (true) {
            in >> sn >> gn;
            if (in.eof()) break;
            sample2group[sn] = gn;
            std::getline(in, skip, '\n');
        }
        for (size_t i = 0; i < ctx.n_sample(); ++i) {
            auto it = sample2group.find(ctx.sample_ids[i]);
            if (it != sample2group.end()) groups_idx[it->second].push_back(i);
        }
    }
    ctx.group_id.assign(ctx.n_sample(), BV_NO_GROUP);
    for (const auto &kv : groups_idx) {
        if (ctx.group_names.size() >= BV_MAX_GROUPS) die("[ERROR] more than 255 population groups");
        for (size_t i : kv.second) ctx.group_id[i] = (uint8_t)ctx.group_names.size();
        ctx.group_names.push_back(kv.first);
    }
}

// A name that ends in ".gz": BGZF blocks + a tabix index beside it (bgzf_tabix.hpp; caller.cpp:242-254), else plain text
void open_outputs(const Options &o, const bvamd::CallContext &ctx, bvamd::TextOut &VCF, bvamd::TextOut &CVG) {
    try { VCF.open(o.out_vcf); CVG.open(o.out_cvg); } catch (const std::exception &ex) { die(ex.what()); }
    std::vector<std::string> add_group_info;
    for (const auto &g : ctx.group_names)  // caller.cpp:229-236
        add_group_info.push_back("##INFO=<ID=" + g + "_AF,Number=A,Type=Float,Description=\"Allele frequency in the " + g +
                                 " populations calculated base on LRT, in the range (0,1)\">");
    VCF.write_header(bvamd::vcf_header(o.reference, o.reference, o.contigs, add_group_info, ctx.sample_ids) + "\n");
    CVG.write_header(bvamd::cvg_header() + "\n");
}

// Batches are bounded by cells (2^28 cells = 5 x 256 MiB of planes per batch in flight), not by a site count that ignores the
// row length: a launch carries ~0.1 ms of fill and drain whatever its size, so small batches run the engine in its worst regime
// (round 2's default was 671 sites at 100 k samples: 0.2 of the large-batch rate).  Per pending site the host keeps the slab row
// and a SiteText, nothing else.
// The pipeline holds up to (G + 1) + (2 G + 2) + G + 1 = 4 G + 4 batches at once (queued, on the engines, waiting for the
// emitter): the cell budget of a batch shrinks with the number of engines so that all of them together stay under 16 GiB of
// host planes (8 engines: 2^26.4 cells per batch instead of 2^28, 36 x 0.44 GB).
uint32_t default_batch_sites(size_t n_sample, size_t n_engines) {
    const size_t pitch = (n_sample + 255) / 256 * 256;
    const size_t in_flight = 4 * n_engines + 4;
    const size_t budget = std::min<size_t>((size_t)1 << 28, (((size_t)16 << 30) / 5) / in_flight);
    const size_t by_cells = budget / std::max<size_t>(pitch, 1);
    return (uint32_t)std::min<size_t>(65536, std::max<size_t>(by_cells, 64));
}

// Which way each stage goes (call_pipeline.hpp: Routes), with a note for every request that the inputs or outputs cannot take;
// `raw` is opened on the batchfiles when they go to the engine compressed
bvamd::Routes resolve_routes(const Options &o, const bvamd::BatchfileHeaders &headers, bvamd::BgzfRawReader &raw) {
    bvamd::Routes r;
    const bool from_bam = o.from_bam();
    const size_t G = o.devices.size();
    // --deflate device: the whole 0xff00-byte blocks of every batch of lines are compressed by one bv_engine_bgzf_deflate call
    // instead of one zlib deflate() each on the emitter thread (bgzf_tabix.hpp: TextOut::write_lines with a BlockDeflater; the
    // headers and the last partial block of a file stay with zlib)
    const bool vcf_gz = bvamd::ends_in_gz(o.out_vcf), cvg_gz = bvamd::ends_in_gz(o.out_cvg);
    if (o.deflate == "device") {
        r.device_deflate = vcf_gz || cvg_gz;
        if (!vcf_gz || !cvg_gz)
            std::cerr << "[NOTE] --deflate device applies to *.gz outputs: " << (r.device_deflate ? (vcf_gz ? o.out_cvg : o.out_vcf) : "both outputs")
                      << " take" << (r.device_deflate ? "s" : "") << " the host path" << std::endl;
    }
    // --inflate device on batchfiles (RawReaderTurns); anything else keeps the host path
    if (o.inflate == "device" && !(from_bam && o.pileup == "device")) {  // (with --pileup device: the BAM files' own members, below)
        if (from_bam) std::cerr << "[NOTE] --inflate device applies to BGZF batchfiles, not to BAM input: the host path is taken" << std::endl;
        else if (G > 1) std::cerr << "[NOTE] --inflate device runs on one engine (--gpus 1): the host path is taken" << std::endl;
        else if (!raw.open(o.batchfiles, headers.header_lines)) std::cerr << "[NOTE] --inflate device needs BGZF batchfiles: the host path is taken" << std::endl;
        else r.device_inflate = true;
    }
    // --pileup device (DevicePileupProducer): BAM input on one engine; anything else keeps the host path
    if (o.pileup == "device") {
        if (!from_bam) std::cerr << "[NOTE] --pileup device applies to BAM input, not to batchfiles: nothing changes" << std::endl;
        else if (G > 1) std::cerr << "[NOTE] --pileup device runs on one engine (--gpus 1): the host path is taken" << std::endl;
        else r.device_pileup = true;
    }
    // --emit device (device_emit.hpp: emit_records_on_device): batches of batchfile rows parsed on the device, and BAM input piled up there
    r.emit_device = o.emit == "device";
    if (r.emit_device && from_bam && !r.device_pileup) {
        std::cerr << "[NOTE] --emit device on BAM input needs --pileup device (on one engine): the host path is taken" << std::endl;
        r.emit_device = false;
    }
    // --indel-tokens device: the '+SEQ' / '-SEQ' tokens of batchfile rows are listed on the engine that parses the rows
    // (bv_engine_text_tokens_enable); the mode is the engine's own, so every worker has it
    if (o.indel_tokens == "device") {
        if (from_bam) std::cerr << "[NOTE] --indel-tokens device applies to batchfile input: on BAM input the pileup's tokens are on the device already" << std::endl;
        else r.indel_tokens_device = true;
    }
    // --pileup device --inflate device: the host threads inflate nothing either
    if (from_bam && o.pileup == "device" && o.inflate == "device") {
        r.bam_inflate_device = r.device_pileup;
        if (!r.device_pileup) std::cerr << "[NOTE] --inflate device on BAM input runs with --pileup device on one engine: the host threads read and inflate" << std::endl;
        for (size_t i = 0; r.bam_inflate_device && i < o.bams.size(); ++i)
            if (!bvamd::bam_members_supported(o.bams[i])) {
                std::cerr << "[NOTE] --inflate device: the BGZF members of " << o.bams[i] << " are not of the XLEN = 6 packing: the host threads read and inflate" << std::endl;
                r.bam_inflate_device = false;
            }
    }
    return r;
}

// Stage seconds: read / parse+pack summed over the producer's threads (BAM input: pileup + pack on the producer thread, all under
// "parse"), engine summed over the workers (staging copies + kernels + records back), emit on the emitter thread; the stages
// overlap, total is wall time
void report(const Options &o, const bvamd::CallContext &ctx, size_t n_workers, double total, const StageClock &clk, const bvamd::OrderedEmitter &emitter,
            const bvamd::BgzfRawReader &raw, const bvamd::DevicePileupProducer::Stats &pileup) {
    const size_t n_sites = emitter.n_sites(), G = ctx.devices.size();
    const bvamd::EmitCounts &counts = emitter.counts();
    const double read_s = clk.get(StageClock::READ), parse_s = clk.get(StageClock::PARSE), engine_s = clk.get(StageClock::ENGINE), emit_s = clk.get(StageClock::EMIT);
    std::cout << "[INFO] bv_call: " << n_sites << " covered positions, " << emitter.n_variants() << " VCF records, " << ctx.n_sample()
              << " samples, " << ctx.group_names.size() << " groups, " << G << " engine(s)" << std::endl;
    char line[512];
    std::snprintf(line, sizeof line,
                  "[INFO] -- %.3f s elapsed, %.1f sites/s: read %.3f s, parse+pack %.3f s (%s; thread-seconds), engine %.3f s (%zu worker(s), batches of %u sites), emit %.3f s",
                  total, total > 0 ? n_sites / total : 0.0, read_s, parse_s, ctx.from_bam ? "pileup" : "batchfile", engine_s, n_workers, ctx.batch_sites, emit_s);
    std::cout << line << std::endl;
    if (o.timing_file.empty()) return;
    std::ofstream tf(o.timing_file);
    tf << "{\"sites\": " << n_sites << ", \"vcf_records\": " << emitter.n_variants() << ", \"samples\": " << ctx.n_sample() << ", \"engines\": " << G
       << ", \"batch_sites\": " << ctx.batch_sites << ", \"input\": \"" << (ctx.from_bam ? "bam" : "batchfile") << "\", \"parser\": \""
       << (ctx.from_bam ? "pileup" : "batchfile") << "\", \"total_s\": " << total << ", \"sites_per_s\": " << (total > 0 ? n_sites / total : 0.0)
       << ", \"read_s\": " << read_s << ", \"parse_pack_s\": " << parse_s << ", \"engine_s\": " << engine_s << ", \"emit_s\": " << emit_s;
    // --inflate device: members handed to the device (those that hold a partial last row, and the surplus rows of longer
    // runs, are inflated again with the next batch) against the members the files hold
    if (ctx.routes.device_inflate)
        tf << ", \"inflate\": \"device\", \"members_inflated\": " << raw.members_handed << ", \"members_in_files\": " << raw.members_passed;
    // --deflate device: whole output blocks compressed by the device, and the emitter's seconds inside those calls (part of emit_s)
    if (ctx.routes.device_deflate)
        tf << ", \"deflate\": \"device\", \"deflate_level\": \"" << o.deflate_level << "\", \"members_deflated\": " << emitter.members_deflated()
           << ", \"deflate_s\": " << emitter.deflate_s();
    // --emit device: VCF lines and CVG rows the engines wrote, and the records among them that the host formatted (numbers the
    // device's formats do not cover: a NaN AF); and the rows whose indel column is not ".", by who wrote the row (the
    // device's own are tallied there too)
    if (ctx.routes.emit_device)
        tf << ", \"emit\": \"device\", \"vcf_lines_device\": " << counts.vcf_lines_device << ", \"cvg_lines_device\": " << counts.cvg_lines_device
           << ", \"lines_host_formatted\": " << counts.lines_host_formatted << ", \"indel_columns_device\": " << counts.indel_columns_device
           << ", \"indel_columns_host\": " << counts.indel_columns_host;
    // batchfile input: the bytes the workers' row (or head) fetches and token fetches brought back from their engines; with
    // --indel-tokens device, the tokens the engines listed
    if (!ctx.from_bam) tf << ", \"text_fetch_bytes\": " << counts.text_fetch_bytes;
    if (!ctx.regions.empty()) tf << ", \"regions\": " << ctx.regions.size();  // --regions on batchfiles
    // --files-per-pass: groups of files read (windows x groups), and the most batchfiles the producer had open at once
    if (o.files_per_pass) tf << ", \"files_per_pass\": " << o.files_per_pass << ", \"passes\": " << o.fm_passes << ", \"max_open_batchfiles\": " << o.fm_max_open;
    if (ctx.routes.indel_tokens_device) tf << ", \"indel_tokens\": \"device\", \"indel_tokens_device\": " << counts.indel_tokens_device;
    // --pileup device: bytes of raw BAM records handed to the engine, and the producer's seconds inside the pileup calls (part of parse_pack_s)
    if (ctx.routes.device_pileup) tf << ", \"pileup\": \"device\", \"reads_bytes\": " << pileup.reads_bytes << ", \"pileup_s\": " << pileup.pileup_s;
    // ... --inflate device with it: the BAM files' compressed members handed to the engine instead, and their bytes
    if (ctx.routes.bam_inflate_device)
        tf << ", \"bam_inflate\": \"device\", \"members_inflated\": " << pileup.members_inflated << ", \"members_bytes\": " << pileup.members_bytes;
    tf << "}\n";
}

}  // namespace

int main(int argc, char **argv) {
    Options o = parse_options(argc, argv);
    validate(o);

    // ---- headers: sample ids in batchfile order (caller.cpp:637-665), or the BAM files' sample names; pop groups; outputs
    bvamd::CallContext ctx;
    bvamd::BatchfileHeaders headers;
    bvamd::FileMajorHeaders fm_headers;
    try {
        for (const auto &b : o.bams) ctx.sample_ids.push_back(bvamd::BamFile(b, false).sample_name());
        if (o.files_per_pass) {  // (file by file, each closed again)
            bvamd::scan_batchfile_headers_closing(o.batchfiles, fm_headers);
            ctx.sample_ids = fm_headers.sample_ids;
            ctx.file_samples = fm_headers.file_samples;
        } else if (!o.from_bam()) {
            bvamd::scan_batchfile_headers(o.batchfiles, headers);
            ctx.sample_ids = headers.sample_ids;
            ctx.file_samples = headers.file_samples;
        }
    } catch (const std::exception &ex) { die(ex.what()); }
    if (ctx.n_sample() == 0) die("[ERROR] no ##SampleIDs= header found in the batchfiles");
    bvamd::RegionIndexes region_indexes;
    if (!o.batch_regions.empty()) load_region_indexes(o, headers, region_indexes);
    if (o.from_bam()) o.batchfiles.clear();
    read_pop_groups(o.pop_group_file, ctx);
    bvamd::TextOut VCF, CVG;
    open_outputs(o, ctx, VCF, CVG);

    // ---- the routes, and with them everything the stages share
    bvamd::BgzfRawReader raw;
    ctx.routes = resolve_routes(o, headers, raw);
    ctx.batch_sites = o.batch_sites ? o.batch_sites : default_batch_sites(ctx.n_sample(), o.devices.size());
    ctx.devices = o.devices;
    ctx.threads = o.threads;
    ctx.user_min_af = o.user_min_af;
    ctx.deflate_level = o.deflate_level == "small" ? BV_DEFLATE_SMALL : BV_DEFLATE_FAST;
    ctx.from_bam = o.from_bam();
    ctx.vcf_gz = bvamd::ends_in_gz(o.out_vcf);
    ctx.regions = o.batch_regions;
    const bvamd::BamInput bam_input{o.bams, o.reference, o.region_list, o.mapq_thd};
    // batchfile input: a batch is one block of rows as text, ~10 B per cell.  32 MiB blocks, the size of the host reader's
    // blocks: larger ones left the read tasks waiting on the packing of the few blocks in flight (measured: 512 MiB blocks on
    // 16 threads ran at 0.6 x the host reader's rate).  In flight: 4 G + 7 blocks, far below the planes' 16 GiB budget.
    const size_t text_block_bytes = (size_t)1 << 25;

    // ---- the pipeline: producer (this thread) -> engine workers -> emitter, results written in batch order
    // batchfile input: three engine workers per GPU -- a text batch has host work on its worker (the rows into pinned staging,
    // the host reader for the positions the device leaves to it, the records and planes back), which the other two overlap
    // (--files-per-pass: one worker, whose engine holds the window's job from its first add to its finish)
    const size_t W = o.files_per_pass ? 1 : (ctx.from_bam ? 1 : 3) * ctx.devices.size();
    bvamd::BatchQueue to_gpu(W + 1), to_emit(2 * W + 2);
    StageClock clk;
    bvamd::ErrorSink errors;
    const double t_start = StageClock::now();
    bvamd::RawReaderTurns raw_turns(ctx, raw, std::max<size_t>(text_block_bytes / std::max<size_t>(1, o.batchfiles.size()), 1),
                                     ctx.regions.empty() ? nullptr : &region_indexes);
    std::deque<bvamd::EngineWorker> workers;
    std::vector<std::thread> worker_threads;
    for (size_t w = 0; w < W; ++w) {
        workers.emplace_back(ctx, w, to_gpu, to_emit, ctx.routes.device_inflate ? &raw_turns : nullptr, clk, errors);
        worker_threads.emplace_back(&bvamd::EngineWorker::run, &workers.back());
    }
    bvamd::OrderedEmitter emitter(ctx, VCF, CVG, clk, errors, ctx.routes.device_deflate ? bvamd::device_block_deflater(ctx) : nullptr);
    std::thread emitter_thread(&bvamd::OrderedEmitter::run, &emitter, std::ref(to_emit));

    bvamd::DevicePileupProducer device_pileup(ctx, bam_input, to_emit, clk, errors);
    std::unique_ptr<bvamd::FileMajorReader> file_major;
    try {
        if (o.files_per_pass) {
            file_major.reset(new bvamd::FileMajorReader(o.batchfiles, fm_headers.header_lines, o.files_per_pass, ctx.threads));
            bvamd::produce_batchfile_file_major(ctx, *file_major, to_gpu, clk, errors);
        }
        else if (ctx.routes.device_pileup) device_pileup.run();
        else if (ctx.from_bam) bvamd::produce_bam_host(ctx, bam_input, to_gpu, clk, errors);
        else if (!ctx.routes.device_inflate && !ctx.regions.empty())
            bvamd::produce_batchfile_regions_host(ctx, o.batchfiles, region_indexes, text_block_bytes, to_gpu, clk, errors);
        else if (!ctx.routes.device_inflate)  // (else the engine workers read the files themselves: RawReaderTurns)
            bvamd::produce_batchfile_text(ctx, headers, o.batchfiles, text_block_bytes, to_gpu, clk, errors);
    } catch (const std::exception &ex) { errors.fail(ex.what()); }

    to_gpu.close();
    for (auto &t : worker_threads) t.join();
    to_emit.close();
    emitter_thread.join();  // (the emitter has closed both outputs)
    if (file_major) { o.fm_passes = file_major->passes(); o.fm_max_open = file_major->max_open(); }
    if (!errors.ok()) die(errors.first());
    report(o, ctx, W, StageClock::now() - t_start, clk, emitter, raw, device_pileup.stats());
    return 0;
}
