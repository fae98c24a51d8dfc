// bv_pileup.cpp -- batchfile creation phase of `basevar basetype` (_create_batchfiles ->
// __create_a_batchfile, src/basetype_caller.cpp:412-470, 800-874) without htslib: BAM files of one
// batch of samples + the reference FASTA + a region -> one reference-format batchfile, which
// `bv_call --batchfiles` (or the reference's own calling phase) consumes.  Host-only by default: no GPU involved.
//
//   bv_pileup -R ref.fa[.gz] --regions CHR:BEG-END [--mapq 10] -I a.bam [-I b.bam ...] [-L bam.list]
//             [--filename-has-samplename] [--no-index] [--thread T] [--window POSITIONS] -o out.bf[.gz]
//             [--rows host|device] [--inflate host|device] [--deflate-level fast|small] [--rows-per-call N]
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
        sym(fetch, "bv_engine_pileup_text_fetch"); sym(deflate, "bv_engine_pileup_text_deflate");
    }
};

// The rows of the region through the engine; `members(bytes, member_off, n)` / `plain(text)` receive a sub-range each
template <typename Members, typename Plain>
bool device_rows(const std::vector<std::string> &bams, const std::string &fa_seq, const std::string &ref_id, uint32_t beg, uint32_t end, int mapq,
                 int threads, uint32_t window, uint32_t rows_per_call, int level, bool gz, bool inflate_device, uint64_t *members_inflated,
                 uint64_t *members_bytes, Members members, Plain plain) {
    EngineLib L;
    L.load();
    bv_engine_config cfg{};
    cfg.device = 0; cfg.max_sites = 64; cfg.max_samples = (uint32_t)bams.size(); cfg.min_af = 0.01;
    bv_engine *e = nullptr;
    if (L.create(&cfg, &e) != BV_OK) throw std::runtime_error(std::string("[ERROR] --rows device: ") + L.last_error(nullptr));
    auto check = [&](int rc) { if (rc != BV_OK) throw std::runtime_error(L.last_error(e)); };
    bool has_data = false;
    try {
        check(L.set_reference(e, fa_seq.data(), fa_seq.size()));
        bvamd::BamPool pool(bams, true);
        const size_t n = bams.size();
        if (window == 0) window = bvamd::pileup_window(n);
        window = std::min<uint32_t>(window, L.max_rows());
        bvamd::PileupRegionCall call;
        call.entry.pileup = L.pileup; call.entry.pileup_bgzf = L.pileup_bgzf; call.entry.last_error = L.last_error;
        call.engine = e;
        call.n_samples = (uint32_t)n; call.region_beg = beg; call.region_end = end; call.mapq_thd = mapq;
        call.skip_empty = false;  // (a window without any run is piled up all the same: every row of it is placeholders)
        call.clamp_tid = true;
        std::vector<uint8_t> buf;
        std::vector<uint64_t> row_off, member_off;
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
            has_data = has_data || n_cov != 0;
            // rows a call from a fixed text budget: 16 bytes a cell and the window's token text bound a sub-range's text
            uint32_t step = rows_per_call;
            if (step == 0) step = (uint32_t)std::max<uint64_t>(1, ((uint64_t)1 << 28) / (16ull * std::max<size_t>(n, 1)));
            for (uint32_t first = 0; first < rows; first += step) {
                const uint32_t cnt = std::min(step, rows - first);
                bv_pileup_text req{};
                req.tile = nullptr; req.chrom = ref_id.data(); req.chrom_len = (uint32_t)ref_id.size(); req.first_row = first; req.n_rows = cnt;
                row_off.assign((size_t)cnt + 1, 0);
                check(L.text(e, &req, row_off.data(), nullptr));
                const uint64_t bytes = row_off[cnt];
                if (gz) {
                    const std::vector<uint64_t> block_off = bvamd::bgzf_block_table(bytes);
                    const uint32_t nb = (uint32_t)block_off.size() - 1;
                    buf.resize(bytes + 31ull * nb);
                    member_off.assign((size_t)nb + 1, 0);
                    check(L.deflate(e, block_off.data(), nb, level, buf.data(), buf.size(), member_off.data(), nullptr));
                    members(buf.data(), member_off.data(), (size_t)nb);
                } else {
                    buf.resize(bytes);
                    check(L.fetch(e, buf.data(), buf.size(), BV_MEM_HOST, nullptr));
                    plain(buf.data(), (size_t)bytes);
                }
            }
            return true;
        });
    } catch (...) {
        L.destroy(e);
        throw;
    }
    L.destroy(e);
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

        const bool gz = bvamd::ends_in_gz(out_path);
        // `.gz`: BGZF, as the reference writes its batchfiles ("must be compressed by BGZF", src/basetype_caller.cpp:428) -- a chain
        // of independent gzip members, which bv_call inflates in parallel (batch_producer.hpp); gzip tools read it as they read .gz
        bvamd::BgzfWriter zf;
        std::FILE *pf = nullptr;
        if (gz) zf.open(out_path);
        else { pf = std::fopen(out_path.c_str(), "wb"); if (!pf) die("[ERROR] " + out_path + " open failure."); }
        auto sink = [&](const std::string &s) {
            if (s.empty()) return;
            if (gz) zf.write(s);
            else if (std::fwrite(s.data(), 1, s.size(), pf) != s.size()) throw std::runtime_error("[ERROR] fail to write data");
        };
        bool has_data = false;
        uint64_t members_inflated = 0, members_bytes = 0;
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
            // the header goes through the host writer; flush(): the device's members follow on a member boundary
            sink(bvamd::batchfile_header(sample_ids));
            if (gz) zf.flush();
            has_data = device_rows(bams, fa_seq, ref_id, beg, end, mapq, threads, window, rows_per_call, level_arg == "small" ? 1 : 0, gz, inflate_device, &members_inflated, &members_bytes,
                                   [&](const uint8_t *m, const uint64_t *off, size_t nm) { zf.write_members(m, off, nm); },
                                   [&](const uint8_t *p, size_t nb) {
                                       if (nb && std::fwrite(p, 1, nb, pf) != nb) throw std::runtime_error("[ERROR] fail to write data");
                                   });
#else
            die("[ERROR] --rows device: this bv_pileup was built without the device route");
#endif
        } else {
            has_data = bvamd::create_a_batchfile(bams, sample_ids, fa_seq, std::make_tuple(ref_id, beg, end), mapq, sink, use_index, threads, window);
        }
        if (gz) zf.close(); else std::fclose(pf);
        std::cerr << "[INFO] " << out_path << ": " << bams.size() << " samples, " << ref_id << ":" << beg << "-" << end
                  << (has_data ? "" : " (no covering reads)");
        if (inflate_device) std::cerr << "; BAM members inflated on the device: " << members_inflated << " (" << members_bytes << " bytes)";
        std::cerr << std::endl;
    } catch (const std::exception &ex) {
        die(ex.what());
    }
    return 0;
}
