// vcf_lines_check.cpp -- the authority for the bytes of bv_engine_vcf_format (include/basevar_amd_vcf.h): the host formatter's
// lines, host/vcf_emit.hpp's format_vcf_line, for planes, heads and records given in a file, and on the way the check that
// the serial line builder of basevar_amd/csrc/bv_vcf_core.h (the definition the kernels compile) writes the same bytes and
// that the length formula gives their number.  No engine, no GPU; the tests build it with g++ (ASan + UBSan) and run it.
//
//   vcf_lines_check IN OUT      exit 0: OUT written;  1: the core and the host formatter differ (stderr says where);  2: bad input
//   vcf_lines_check IN OUT --time   the host formatter alone, timed (tools/vcf_lines_bench.py): OUT is the lines back to back, and
//                                   stdout "format_vcf_line_s <seconds of the format_vcf_line calls, one thread> bytes <of the lines>"
//
// IN  (little endian):  u32 n_rows, n_samples, n_lines, n_groups;  n_groups x (u32 len, name);  cell [n_rows][n_samples];
//     phred [n_rows][n_samples];  per line: u32 site, u32 ref_pos, (u32 len, ref_id), (u32 len, ref_base), i32 head_len
//     (-1: the formatter's own head, else that many bytes follow and stand in its place), bv_site_result, n_groups x bv_group_result
// OUT per line:  u32 head_len, head, gt[4] (vcf_gt_codes), u64 line_len, line
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "../../basevar_amd/csrc/bv_vcf_core.h"
#include "../../basevar_amd/host/vcf_emit.hpp"

namespace {
struct In {
    std::vector<char> d;
    size_t at = 0;
    void need(size_t n) { if (at + n > d.size()) { std::cerr << "vcf_lines_check: input ends early" << std::endl; std::exit(2); } }
    template <class T> T get() { need(sizeof(T)); T v; std::memcpy(&v, &d[at], sizeof(T)); at += sizeof(T); return v; }
    std::string str(size_t n) { need(n); std::string s(&d[at], n); at += n; return s; }
    const uint8_t *bytes(size_t n) { need(n); const uint8_t *p = reinterpret_cast<const uint8_t *>(&d[at]); at += n; return p; }
};
template <class T> void put(std::ofstream &o, T v) { o.write(reinterpret_cast<const char *>(&v), sizeof v); }
}  // namespace

int main(int argc, char **argv) {
    const bool timed = argc == 4 && std::string(argv[3]) == "--time";
    if (argc != 3 && !timed) { std::cerr << "usage: vcf_lines_check IN OUT [--time]" << std::endl; return 2; }
    double format_s = 0;
    uint64_t format_bytes = 0;
    In in;
    {
        std::ifstream f(argv[1], std::ios::binary);
        if (!f) { std::cerr << "vcf_lines_check: cannot open " << argv[1] << std::endl; return 2; }
        in.d.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    const uint32_t n_rows = in.get<uint32_t>(), n = in.get<uint32_t>(), n_lines = in.get<uint32_t>(), n_groups = in.get<uint32_t>();
    std::vector<std::string> group_names;
    for (uint32_t g = 0; g < n_groups; ++g) { const uint32_t len = in.get<uint32_t>(); group_names.push_back(in.str(len)); }
    const uint8_t *cell = in.bytes((size_t)n_rows * n), *phred = in.bytes((size_t)n_rows * n);
    uint8_t bp[256 * BV_VCF_BP_CHARS];
    if (!bv_vcf_bp_table(bp)) { std::cerr << "vcf_lines_check: a BP string is not 8 characters" << std::endl; return 1; }
    std::ofstream out(argv[2], std::ios::binary);
    if (!out) { std::cerr << "vcf_lines_check: cannot write " << argv[2] << std::endl; return 2; }
    for (uint32_t k = 0; k < n_lines; ++k) {
        const uint32_t site = in.get<uint32_t>();
        bvamd::SiteText st;
        st.ref_pos = in.get<uint32_t>();
        { const uint32_t len = in.get<uint32_t>(); st.ref_id = in.str(len); }
        { const uint32_t len = in.get<uint32_t>(); st.ref_base = in.str(len); }
        const int32_t head_len = in.get<int32_t>();
        const std::string given = head_len >= 0 ? in.str((size_t)head_len) : std::string();
        const bv_site_result r = in.get<bv_site_result>();
        std::vector<bv_group_result> groups(n_groups);
        for (auto &g : groups) g = in.get<bv_group_result>();
        if (site >= n_rows || r.n_alt == 0 || r.n_alt > BV_MAX_ALT || st.ref_base.empty()) {
            std::cerr << "vcf_lines_check: line " << k << ": site beyond the rows, a record without ALT, or no REF" << std::endl;
            return 2;
        }
        const uint8_t *c = cell + (size_t)site * n, *q = phred + (size_t)site * n;
        const bv_group_result *gp = n_groups ? groups.data() : nullptr;
        // the authority: the whole line as the host writes it; its head is a prefix of it
        const auto t0 = std::chrono::steady_clock::now();
        const std::string full = bvamd::format_vcf_line(st, c, q, n, r, gp, group_names);
        if (timed) {
            format_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            format_bytes += full.size();
            out.write(full.data(), (std::streamsize)full.size());
            continue;
        }
        const std::string own = bvamd::format_vcf_head(st, r, gp, group_names);
        if (full.compare(0, own.size(), own) != 0) { std::cerr << "line " << k << ": format_vcf_head is no prefix of format_vcf_line" << std::endl; return 1; }
        const std::string head = head_len >= 0 ? given : own;
        const std::string line = head + full.substr(own.size());
        // the definition the device compiles
        uint8_t gt[4];
        bvamd::vcf_gt_codes(st, r, gt);
        uint64_t covered = 0;
        for (uint32_t s = 0; s < n; ++s) covered += bv_vcf_covered(c[s]) ? 1 : 0;
        for (int b = 0; b < 4; ++b)
            if (!bv_vcf_gt_char_ok(gt[b])) { std::cerr << "line " << k << ": vcf_gt_codes gave a character the core refuses" << std::endl; return 1; }
        std::vector<uint8_t> built(bv_vcf_line_bytes(head.size(), n, n));
        const uint64_t len = bv_vcf_line(head.data(), head.size(), c, q, n, gt, bp, built.data());
        if (len != bv_vcf_line_bytes(head.size(), n, covered)) {
            std::cerr << "line " << k << ": built " << len << " bytes, the formula says " << bv_vcf_line_bytes(head.size(), n, covered) << std::endl;
            return 1;
        }
        if (len != line.size() || std::memcmp(built.data(), line.data(), len) != 0) {
            size_t i = 0;
            while (i < len && i < line.size() && built[i] == (uint8_t)line[i]) ++i;
            std::cerr << "line " << k << ": bv_vcf_line and format_vcf_line differ at byte " << i << " (" << len << " / " << line.size() << " bytes)" << std::endl;
            return 1;
        }
        put<uint32_t>(out, (uint32_t)head.size());
        out.write(head.data(), (std::streamsize)head.size());
        out.write(reinterpret_cast<const char *>(gt), 4);
        put<uint64_t>(out, (uint64_t)line.size());
        out.write(line.data(), (std::streamsize)line.size());
    }
    out.close();
    if (timed) std::cout << "format_vcf_line_s " << format_s << " bytes " << format_bytes << std::endl;
    return out ? 0 : 2;
}
