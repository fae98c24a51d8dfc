// emit_corpus -- VCF records and CVG rows as basevar_amd/host/vcf_emit.hpp writes them, from seeded pseudo-random site records:
// the text that the DEFLATE encoder (bv_deflate_core.h) is measured and tested on.  No engine, no GPU.
//
//   emit_corpus vcf|cvg N_SAMPLES N_LINES SEED [COVERAGE = 0.08]      -> stdout
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../basevar_amd/host/vcf_emit.hpp"

namespace {
struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    double unit() { return next() / 2147483648.0; }
    uint32_t below(uint32_t n) { return next() % n; }
};
}  // namespace

int main(int argc, char **argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: emit_corpus vcf|cvg N_SAMPLES N_LINES SEED [COVERAGE]\n"); return 2; }
    const bool vcf = std::strcmp(argv[1], "vcf") == 0;
    const size_t n = std::strtoull(argv[2], nullptr, 10), lines = std::strtoull(argv[3], nullptr, 10);
    Rng rng{std::strtoull(argv[4], nullptr, 10) * 2654435761ull + 1};
    const double coverage = argc > 5 ? std::atof(argv[5]) : 0.08;
    std::vector<uint8_t> cell(n), phred(n);
    uint32_t pos = 10000 + rng.below(1000);
    for (size_t l = 0; l < lines; ++l) {
        bvamd::SiteText st;
        st.ref_id = "chr" + std::to_string(1 + l * 3 / (lines + 1));
        pos += 1 + rng.below(40);
        st.ref_pos = pos;
        const int ref = (int)rng.below(4), alt = (ref + 1 + (int)rng.below(3)) & 3;
        st.ref_base = std::string(1, bvamd::EMIT_BASES[ref]);
        if (rng.below(10) == 0) st.indel_tokens = {"+AT", "-C", "+AT"};
        bv_site_result r;
        std::memset(&r, 0, sizeof r);
        const double alt_frac = rng.unit() * 0.5;
        for (size_t i = 0; i < n; ++i) {
            cell[i] = BV_CELL_NOCALL;
            phred[i] = 0;
            if (rng.unit() >= coverage) continue;
            const int b = rng.unit() < alt_frac ? alt : (rng.below(100) == 0 ? (int)rng.below(4) : ref);
            const bool rev = rng.below(2) != 0;
            cell[i] = (uint8_t)(b | (rev ? BV_CELL_REV : 0));
            phred[i] = (uint8_t)(2 + rng.below(40));
            r.depth[b] += 1; r.total_depth += 1;
            r.cvg_sb[(b == ref ? 0 : 2) + (rev ? 1 : 0)] += 1;
        }
        r.cvg_fs = rng.unit() * 30; r.cvg_sor = rng.unit() * 4;
        r.n_alt = 1; r.alt[0] = (uint8_t)alt;
        r.af[0] = alt_frac; r.caf[0] = r.total_depth ? (double)r.depth[alt] / r.total_depth : 0.0;
        r.qual = rng.unit() * 5000; r.qd = rng.unit() * 40;
        for (int k = 0; k < 4; ++k) r.var_sb[k] = r.cvg_sb[k];
        r.var_fs = r.cvg_fs; r.var_sor = r.cvg_sor;
        r.mq_ranksum = rng.unit() * 6 - 3; r.rpr_ranksum = rng.unit() * 6 - 3; r.bq_ranksum = rng.unit() * 6 - 3;
        const std::string s = vcf ? bvamd::format_vcf_line(st, cell.data(), phred.data(), n, r, nullptr, {}) : bvamd::format_cvg_line(st, r);
        std::fwrite(s.data(), 1, s.size(), stdout);
    }
    return 0;
}
