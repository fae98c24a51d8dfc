// bv_pileup.cpp -- batchfile creation phase of `basevar basetype` (_create_batchfiles ->
// __create_a_batchfile, src/basetype_caller.cpp:412-470, 800-874) without htslib: BAM files of one
// batch of samples + the reference FASTA + a region -> one reference-format batchfile, which
// `bv_call --batchfiles` (or the reference's own calling phase) consumes.  Host-only by default: no GPU involved.
//
//   bv_pileup -R ref.fa[.gz] --regions CHR:BEG-END [--mapq 10] -I a.bam [-I b.bam ...] [-L bam.list]
//             [--filename-has-samplename] [--no-index] [--thread T] [--window POSITIONS] -o out.bf[.gz]
//             [--rows host|device] [--inflate host|device] [--deflate-level fast|small] [--rows-per-call N]
//             [-B N [--batches-per-pass K] [--output-plain]]
//
// -B N (--batch-count N; -o is then a PREFIX): the reference's batches (_create_batchfiles, :427-442).  The samples, in input order
// (-I then -L), are cut into bn = ceil(n / N) batches of N, the last one maybe smaller, and batch j = 1 .. bn goes to
// PREFIX.<j>_<bn>.bf.gz (with --output-plain to PREFIX.<j>_<bn>.bf, plain text) with a header of its own: the file a run without
// -B over that slice of the samples writes.  With --rows host that is one create_a_batchfile per batch.  With --rows device ONE
// engine serves the whole run and the batches are taken --batches-per-pass K at a time (default 1: one batch, one 500 kb window,
// the reference's shape; 0 = all): a pass reads its K N samples' records (or members) per window, piles them up in one
// bv_engine_pileup[_bgzf] -- the window is pileup_window(K N) -- and writes the rows of the K batches as K sample parts of that
// pileup (bv_engine_pileup_text_parts, include/basevar_amd_pileup_text_parts.h), a sub-range of rows a call, with one deflate call
// whose blocks are cut at the parts' boundaries; each part's members, or text, are appended to its own file.  Neither --window,
// --rows-per-call, --batches-per-pass nor --deflate-level changes an inflated byte.
//
// --rows device (builds with -DBV_PILEUP_DEVICE; the engine library beside the tool is loaded on demand, so the default route
// needs neither it nor a GPU): the host threads read the samples' raw records, one engine piles them up
// (bv_engine_pileup) and writes the rows where the planes lie (bv_engine_pileup_text, include/basevar_amd_pileup_text.h), a
// sub-range of rows a call; a `.gz` output takes each sub-range as BGZF members deflated on the device, a plain one as text.  The
// inflated output is the default route's byte for byte; neither --window nor --rows-per-call changes it.
// --inflate device (with --rows device): the host threads inflate nothing -- they read the compressed BGZF members of every
// sample's fetch and the cut points (host/raw_members.hpp) and the engine inflates and piles up (bv_engine_pileup_bgzf,
// include/basevar_amd_pileup_bgzf.h).  Without --rows device, or on files whose members are not of the XLEN = 6 packing, a
// note is printed and the host reads as before.
//
// Sample ids come from the first @RG SM tag of each BAM (BamHeader::get_sample_name) or, with
// --filename-has-samplename, from the file name up to its first '.' (src/basetype_caller.cpp:262-294).
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "bgzf_tabix.hpp"
#include "pileup.hpp"
#ifdef BV_PILEUP_DEVICE
#include <dlfcn.h>
#include <unistd.h>

#include "../../include/basevar_amd_pileup_text.h"
#include "device_pileup.hpp"
#endif

namespace {
[[noreturn]] void die(const std::string &m) {
    std::cerr << m << std::endl;
    std::exit(1);
}
std::string basename_of(const std::string &p) {
    const size_t s = p.find_last_of('/');
    return s == std::string::npos ? p : p.substr(s + 1);
}

// One output batchfile: BGZF (`.gz`) or plain text
struct BatchOut {
    bvamd::BgzfWriter zf;
    std::FILE *pf = nullptr;
    bool gz = false;
    std::string path;
    bool is_open() const { return gz ? zf.is_open() : pf != nullptr; }
    void open(const std::string &p, bool gz_) {
        path = p; gz = gz_;
        if (gz) zf.open(p);
        else { pf = std::fopen(p.c_str(), "wb"); if (!pf) throw std::runtime_error("[ERROR] " + p + " open failure."); }
    }
    void bytes(const void *p, size_t nb) {
        if (nb && std::fwrite(p, 1, nb, pf) != nb) throw std::runtime_error("[ERROR] fail to write data");
    }
    void text(const std::string &s) {
        if (s.empty()) return;
        if (gz) zf.write(s);
        else bytes(s.data(), s.size());
    }
    void flush() { if (gz) zf.flush(); }
    void members(const uint8_t *m, const uint64_t *off, size_t nm) { zf.write_members(m, off, nm); }
    void close() {
        if (gz) zf.close();
        else if (pf) { std::fclose(pf); pf = nullptr; }
    }
    ~BatchOut() { if (!gz && pf) std::fclose(pf); }
};

#ifdef BV_PILEUP_DEVICE
// The engine library, loaded when --rows device asks for it: $BASEVAR_AMD_LIB, else libbasevar_amd.so beside this program
struct EngineLib {
    void *so = nullptr;
    decltype(&bv_engine_create) create = nullptr;
    decltype(&bv_engine_destroy) destroy = nullptr;
    decltype(&bv_last_error) last_error = nullptr;
    decltype(&bv_pileup_max_rows) max_rows = nullptr;
    decltype(&bv_engine_pileup_set_reference) set_reference = nullptr;
    decltype(&bv_engine_pileup) pileup = nullptr;
    decltype(&bv_engine_pileup_bgzf) pileup_bgzf = nullptr;
    decltype(&bv_engine_pileup_text) text = nullptr;
    decltype(&bv_engine_pileup_text_parts) text_parts = nullptr;
    decltype(&bv_engine_pileup_text_fetch) fetch = nullptr;
    decltype(&bv_engine_pileup_text_deflate) deflate = nullptr;

    template <typename F>
    void sym(F &f, const char *name) {
        f = reinterpret_cast<F>(dlsym(so, name));
        if (!f) throw std::runtime_error(std::string("[ERROR] --rows device: ") + name + " is not in the engine library");
    }
    void load() {
        std::string path;
        if (const char *env = std::getenv("BASEVAR_AMD_LIB")) path = env;
        if (path.empty()) {
            char exe[4096];
            const ssize_t n = readlink("/proc/self/exe", exe, sizeof exe - 1);
            if (n <= 0) throw std::runtime_error("[ERROR] --rows device: cannot find this program's directory");
            path = std::string(exe, (size_t)n);
            path = path.substr(0, path.find_last_of('/') + 1) + "libbasevar_amd.so";
        }
        so = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!so) throw std::runtime_error(std::string("[ERROR] --rows device: ") + dlerror());
        sym(create, "bv_engine_create"); sym(destroy, "bv_engine_destroy"); sym(last_error, "bv_last_error"); sym(max_rows, "bv_pileup_max_rows");
        sym(set_reference, "bv_engine_pileup_set_reference"); sym(pileup, "bv_engine_pileup"); sym(pileup_bgzf, "bv_engine_pileup_bgzf"); sym(text, "bv_engine_pileup_text");
        sym(fetch, "bv_engine_pileup_text_fetch"); sym(deflate, "bv_engine_pileup_text_deflate"); sym(text_parts, "bv_engine_pileup_text_parts");
    }
};

// One engine for the run: the library, an engine for up to max_samples samples a pileup, the reference uploaded
struct DeviceEngine {
    EngineLib L;
    bv_engine *e = nullptr;
    DeviceEngine(size_t max_samples, const std::string &fa_seq) {
        L.load();
        bv_engine_config cfg{};
        cfg.device = 0; cfg.max_sites = 64; cfg.max_samples = (uint32_t)max_samples; cfg.min_af = 0.01;
        if (L.create(&cfg, &e) != BV_OK) throw std::runtime_error(std::string("[ERROR] --rows device: ") + L.last_error(nullptr));
        if (L.set_reference(e, fa_seq.data(), fa_seq.size()) != BV_OK) {
            const std::string m = L.last_error(e);
            L.destroy(e);
            throw std::runtime_error(m);
        }
    }
    ~DeviceEngine() { L.destroy(e); }
    DeviceEngine(const DeviceEngine &) = delete;
    DeviceEngine &operator=(const DeviceEngine &) = delete;
};

// The rows of the region through the engine, for the samples `bams` of one pileup cut into the sample parts
// [part_first[p], part_first[p + 1]) (one part of all samples: the rows of the whole pileup, bv_engine_pileup_text);
// `members(part, bytes, member_off, n)` / `plain(part, text, bytes)` receive a sub-range of a part's rows each
template <typename Members, typename Plain>
bool device_rows(DeviceEngine &dev, const std::vector<std::string> &bams, const std::vector<uint32_t> &part_first, const std::string &ref_id, uint32_t beg,
                 uint32_t end, int mapq, int threads, uint32_t window, uint32_t rows_per_call, int level, bool gz, bool inflate_device, uint64_t *members_inflated,
                 uint64_t *members_bytes, uint64_t *pileup_calls, Members members, Plain plain) {
    EngineLib &L = dev.L;
    bv_engine *e = dev.e;
    auto check = [&](int rc) { if (rc != BV_OK) throw std::runtime_error(L.last_error(e)); };
    bool has_data = false;
    bvamd::BamPool pool(bams, true);
    const size_t n = bams.size(), n_parts = part_first.size() - 1;
    if (window == 0) window = bvamd::pileup_window(n);
    window = std::min<uint32_t>(window, L.max_rows());
    bvamd::PileupRegionCall call;
    call.entry.pileup = L.pileup; call.entry.pileup_bgzf = L.pileup_bgzf; call.entry.last_error = L.last_error;
    call.engine = e;
    call.n_samples = (uint32_t)n; call.region_beg = beg; call.region_end = end; call.mapq_thd = mapq;
    call.skip_empty = false;  // (a window without any run is piled up all the same: every row of it is placeholders)
    call.clamp_tid = true;
    std::vector<uint8_t> buf;
    std::vector<uint64_t> row_off, member_off, block_off;
    std::vector<size_t> first_block;
    bvamd::for_each_pileup_window(beg, end, window, [&](uint32_t wb, uint32_t we) {
        const uint32_t rows = we - wb + 1;
        uint32_t n_cov = 0;
        if (inflate_device) {
            bvamd::WindowMembers wm;
            bvamd::read_window_members(pool, bams, ref_id, wb, we, threads, wm);
            bvamd::pileup_window_members(call, wm, wb, we, &n_cov);
            *members_inflated += wm.plan.member_pos.size(); *members_bytes += wm.plan.data.size();
        } else {
            bvamd::WindowReads reads;
            bvamd::read_window_raw(pool, bams, ref_id, wb, we, threads, reads);
            bvamd::pileup_window_reads(call, reads, wb, we, &n_cov);
        }
        *pileup_calls += 1;
        has_data = has_data || n_cov != 0;
        // rows a call from a fixed text budget: 16 bytes a cell and the window's token text bound a sub-range's text
        uint32_t step = rows_per_call;
        if (step == 0) step = (uint32_t)std::max<uint64_t>(1, ((uint64_t)1 << 28) / (16ull * std::max<size_t>(n, 1)));
        for (uint32_t first = 0; first < rows; first += step) {
            const uint32_t cnt = std::min(step, rows - first);
            bv_pileup_text req{};
            req.tile = nullptr; req.chrom = ref_id.data(); req.chrom_len = (uint32_t)ref_id.size(); req.first_row = first; req.n_rows = cnt;
            row_off.assign(n_parts * cnt + 1, 0);
            if (n_parts == 1 && part_first[0] == 0 && part_first[1] == n) {
                check(L.text(e, &req, row_off.data(), nullptr));
            } else {
                bv_pileup_text_parts parts{};
                parts.rows = &req; parts.part_first = part_first.data(); parts.n_parts = (uint32_t)n_parts;
                check(L.text_parts(e, &parts, row_off.data(), nullptr));
            }
            const uint64_t bytes = row_off[n_parts * cnt];
            if (gz) {
                // one deflate call; a part's blocks are counted from the part's first byte, so that no member spans two files
                block_off.clear();
                first_block.assign(1, 0);
                for (size_t p = 0; p < n_parts; ++p) {
                    const uint64_t lo = row_off[p * cnt], hi = row_off[(p + 1) * cnt];
                    for (uint64_t at = lo; at < hi; at += 0xff00) block_off.push_back(at);
                    first_block.push_back(block_off.size());
                }
                block_off.push_back(bytes);
                const uint32_t nb = (uint32_t)block_off.size() - 1;
                buf.resize(bytes + 31ull * nb);
                member_off.assign((size_t)nb + 1, 0);
                check(L.deflate(e, block_off.data(), nb, level, buf.data(), buf.size(), member_off.data(), nullptr));
                for (size_t p = 0; p < n_parts; ++p) {
                    // (the part's member offsets, counted from its first member)
                    const uint64_t base = member_off[first_block[p]];
                    std::vector<uint64_t> off(member_off.begin() + first_block[p], member_off.begin() + first_block[p + 1] + 1);
                    for (uint64_t &o : off) o -= base;
                    members(p, buf.data() + base, off.data(), off.size() - 1);
                }
            } else {
                buf.resize(bytes);
                check(L.fetch(e, buf.data(), buf.size(), BV_MEM_HOST, nullptr));
                for (size_t p = 0; p < n_parts; ++p) plain(p, buf.data() + row_off[p * cnt], (size_t)(row_off[(p + 1) * cnt] - row_off[p * cnt]));
            }
        }
        return true;
    });
    return has_data;
}
#endif
}  // namespace

int main(int argc, char **argv) {
    std::vector<std::string> bams;
    std::string fasta, regions, out_path, bam_list;
    int mapq = 10;  // BaseTypeARGS default, src/basetype_utils.h
    int threads = 1;
    uint32_t window = 0;  // positions per pileup window (0 = from a cell budget); the rows do not depend on it
    bool name_from_file = false, use_index = true;
    std::string rows_arg = "host", level_arg = "fast", inflate_arg = "host";
    uint32_t rows_per_call = 0;  // --rows device: rows a bv_engine_pileup_text call (0 = from a text budget); the rows do not depend on it
    // -B: samples a batchfile (0: one file of all samples, -o names it); --rows device: batches a pass (0 = all).  The default of 1
    // is the reference's shape -- one batch, one 500 kb window -- and the fastest of K = 1, 4, 16, 50 on the 10,000-sample cohort
    // at 1 and 16 threads (profiles/pileup_batches_bench.txt).  That cohort's windows cover whole files, so it cannot show what a
    // shorter window (more batches a pass) costs in repeated member reads on real low-pass BAM files.
    size_t batch_count = 0, batches_per_pass = 1;
    bool output_plain = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) die("missing value for " + a); return argv[++i]; };
        if (a == "-I" || a == "--input") bams.push_back(next());
        else if (a == "-L" || a == "--align-file-list") bam_list = next();
        else if (a == "-R" || a == "--reference") fasta = next();
        else if (a == "-r" || a == "--regions") regions = next();
        else if (a == "-q" || a == "--mapq") mapq = std::stoi(next());
        else if (a == "-o" || a == "--output") out_path = next();
        else if (a == "--filename-has-samplename") name_from_file = true;
        else if (a == "--no-index") use_index = false;
        else if (a == "-t" || a == "--thread") threads = std::stoi(next());
        else if (a == "--window") window = (uint32_t)std::stoul(next());
        else if (a == "--rows") rows_arg = next();
        else if (a == "--inflate") inflate_arg = next();
        else if (a == "--deflate-level") level_arg = next();
        else if (a == "--rows-per-call") rows_per_call = (uint32_t)std::stoul(next());
        else if (a == "-B" || a == "--batch-count") { batch_count = std::stoul(next()); if (batch_count == 0) die("--batch-count wants a number >= 1"); }
        else if (a == "--batches-per-pass") batches_per_pass = std::stoul(next());
        else if (a == "--output-plain") output_plain = true;
        else die("unknown argument " + a);
    }
    if (!bam_list.empty() && !bvamd::read_first_column(bam_list, bams)) die("[ERROR] cannot open " + bam_list);
    if (rows_arg != "host" && rows_arg != "device") die("--rows wants host or device");
    if (level_arg != "fast" && level_arg != "small") die("--deflate-level wants fast or small");
    if (inflate_arg != "host" && inflate_arg != "device") die("--inflate wants host or device");
    bool inflate_device = inflate_arg == "device";
#ifndef BV_PILEUP_DEVICE
    if (inflate_device) die("[ERROR] --inflate device: this bv_pileup was built without the device route");
#endif
    if (bams.empty() || fasta.empty() || regions.empty() || out_path.empty())
        die("usage: bv_pileup -R ref.fa --regions CHR:BEG-END [--mapq Q] -I a.bam [-I ...] [-L list] -o out.bf[.gz]");
    try {
        bvamd::Region rg;
        if (!bvamd::parse_region(regions, rg)) die("--regions wants CHR:BEG-END");
        const std::string &ref_id = rg.ref_id;
        const uint32_t beg = rg.beg, end = rg.end;
        if (beg < 1 || end < beg) die("--regions wants 1 <= BEG <= END");

        std::vector<std::string> sample_ids;
        for (const auto &b : bams) {
            if (name_from_file) {
                std::string fn = basename_of(b);
                const size_t ext = fn.rfind('.');  // remove_filename_extension
                if (ext != std::string::npos && ext > 0) fn = fn.substr(0, ext);
                const size_t si = fn.find('.');
                sample_ids.push_back(si > 0 && si != std::string::npos ? fn.substr(0, si) : fn);
            } else {
                sample_ids.push_back(bvamd::BamFile(b, false).sample_name());
            }
        }
        const std::string fa_seq = bvamd::load_fasta_sequence(fasta, ref_id);
        if (end > fa_seq.size()) die("[ERROR] region end beyond the end of " + ref_id);

        // `.gz`: BGZF, as the reference writes its batchfiles ("must be compressed by BGZF", src/basetype_caller.cpp:428) -- a chain
        // of independent gzip members, which bv_call inflates in parallel (batch_producer.hpp); gzip tools read it as they read .gz
        const bool gz = batch_count ? !output_plain : bvamd::ends_in_gz(out_path);
        // the output files: one of all samples, or with -B batch j = 1 .. bn of samples [(j - 1) B, j B) as PREFIX.<j>_<bn>.bf.gz
        const size_t n = bams.size(), per_file = batch_count ? batch_count : n, n_files = (n + per_file - 1) / per_file;
        auto file_name = [&](size_t j) { return batch_count ? out_path + "." + std::to_string(j + 1) + "_" + std::to_string(n_files) + (gz ? ".bf.gz" : ".bf") : out_path; };
        auto slice = [&](const std::vector<std::string> &v, size_t j, size_t files) {
            return std::vector<std::string>(v.begin() + j * per_file, v.begin() + std::min(n, (j + files) * per_file));
        };
        bool has_data = false;
        uint64_t members_inflated = 0, members_bytes = 0, pileup_calls = 0;
        size_t passes = 0;
#ifdef BV_PILEUP_DEVICE
        if (inflate_device && rows_arg != "device") {
            std::cerr << "[NOTE] --inflate device takes effect with --rows device; the host threads read and inflate the BAM files" << std::endl;
            inflate_device = false;
        }
        for (size_t i = 0; inflate_device && i < bams.size(); ++i)
            if (!bvamd::bam_members_supported(bams[i])) {
                std::cerr << "[NOTE] --inflate device: the BGZF members of " << bams[i] << " are not of the XLEN = 6 packing; the host threads read and inflate the BAM files" << std::endl;
                inflate_device = false;
            }
#endif
        if (rows_arg == "device") {
#ifdef BV_PILEUP_DEVICE
            const size_t files_a_pass = batches_per_pass ? std::min(batches_per_pass, n_files) : n_files;
            std::vector<std::unique_ptr<BatchOut>> outs;
            for (size_t j = 0; j < n_files; ++j) {  // (every file is opened before the engine is made, as the one file was)
                outs.emplace_back(new BatchOut());
                if (j < files_a_pass) outs[j]->open(file_name(j), gz);
            }
            DeviceEngine dev(std::min(n, files_a_pass * per_file), fa_seq);
            for (size_t j0 = 0; j0 < n_files; j0 += files_a_pass, ++passes) {
                const size_t files = std::min(files_a_pass, n_files - j0);
                std::vector<uint32_t> part_first(1, 0);
                for (size_t j = j0; j < j0 + files; ++j) {
                    if (!outs[j]->is_open()) outs[j]->open(file_name(j), gz);
                    // the header goes through the host writer; flush(): the device's members follow on a member boundary
                    outs[j]->text(bvamd::batchfile_header(slice(sample_ids, j, 1)));
                    outs[j]->flush();
                    part_first.push_back((uint32_t)(std::min(n, (j + 1) * per_file) - j0 * per_file));
                }
                const bool any = device_rows(dev, slice(bams, j0, files), part_first, ref_id, beg, end, mapq, threads, window, rows_per_call, level_arg == "small" ? 1 : 0, gz,
                                             inflate_device, &members_inflated, &members_bytes, &pileup_calls,
                                             [&](size_t p, const uint8_t *m, const uint64_t *off, size_t nm) { outs[j0 + p]->members(m, off, nm); },
                                             [&](size_t p, const uint8_t *t, size_t nb) { outs[j0 + p]->bytes(t, nb); });
                has_data = has_data || any;
                for (size_t j = j0; j < j0 + files; ++j) outs[j]->close();
            }
#else
            die("[ERROR] --rows device: this bv_pileup was built without the device route");
#endif
        } else {
            for (size_t j = 0; j < n_files; ++j) {
                BatchOut out;
                out.open(file_name(j), gz);
                const bool any = bvamd::create_a_batchfile(slice(bams, j, 1), slice(sample_ids, j, 1), fa_seq, std::make_tuple(ref_id, beg, end), mapq,
                                                           [&](const std::string &t) { out.text(t); }, use_index, threads, window);
                has_data = has_data || any;
                out.close();
            }
        }
        std::cerr << "[INFO] " << out_path << ": " << bams.size() << " samples, " << ref_id << ":" << beg << "-" << end
                  << (has_data ? "" : " (no covering reads)");
        if (batch_count) {
            std::cerr << "; " << n_files << " batchfiles of " << per_file << " samples";
            if (rows_arg == "device") std::cerr << ", " << passes << " passes, " << pileup_calls << " pileup calls";
        }
        if (inflate_device) std::cerr << "; BAM members inflated on the device: " << members_inflated << " (" << members_bytes << " bytes)";
        std::cerr << std::endl;
    } catch (const std::exception &ex) {
        die(ex.what());
    }
    return 0;
}
