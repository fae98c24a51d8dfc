// record_text_check.cpp -- a stand-alone harness (its own main; built with g++, plain or with ASan + UBSan) that holds
// basevar_amd/csrc/bv_numfmt_core.h to snprintf("%f") / snprintf("%g") / std::to_string((int)) and
// basevar_amd/csrc/bv_record_text_core.h to host/vcf_emit.hpp's format_vcf_head and format_cvg_line, byte for byte.
//   record_text_check numbers            the number corpus; prints what it formatted, exits 1 at the first difference
//   record_text_check lines IN OUT       the records of IN through both; OUT is the host's text per line (see dump())
// Every value that is formatted is one whose bv_numfmt_*_ok predicate is true; the others are only counted.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../basevar_amd/csrc/bv_record_text_core.h"
#include "../../basevar_amd/host/vcf_emit.hpp"

namespace {

uint64_t n_f6 = 0, n_g6 = 0, n_iod = 0, n_out = 0;

std::string text_of(bv_numfmt_val x) {
    uint8_t buf[64];
    std::memset(buf, '#', sizeof buf);
    const uint32_t len = bv_numfmt_len(x);
    if (len > 40) { std::fprintf(stderr, "a number of %u bytes\n", len); std::exit(1); }
    bv_numfmt_put(x, buf + 8);
    for (uint32_t i = 0; i < sizeof buf; ++i)
        if ((i < 8 || i >= 8 + len) && buf[i] != '#') { std::fprintf(stderr, "bv_numfmt_put wrote outside its %u bytes (at %d)\n", len, (int)i - 8); std::exit(1); }
    return std::string(reinterpret_cast<char *>(buf + 8), len);
}

[[noreturn]] void differ(const char *what, double v, const std::string &got, const char *want) {
    std::fprintf(stderr, "%s of %a (%.17g): core \"%s\", libc \"%s\"\n", what, v, v, got.c_str(), want);
    std::exit(1);
}

// v through every format whose domain holds it
void check(double v) {
    char want[400];
    if (bv_numfmt_f6_ok(v)) {
        std::snprintf(want, sizeof want, "%f", v);
        const std::string got = text_of(bv_numfmt_f6(v));
        if (got != want) differ("%f", v, got, want);
        ++n_f6;
    } else if (bv_numfmt_f6(v).kind != BV_NUM_BAD) differ("%f outside its domain", v, "a value", "BV_NUM_BAD");
    if (bv_numfmt_g6_ok(v)) {
        std::snprintf(want, sizeof want, "%g", v);
        const std::string got = text_of(bv_numfmt_g6(v));
        if (got != want) differ("%g", v, got, want);
        ++n_g6;
    } else {
        if (bv_numfmt_g6(v).kind != BV_NUM_BAD) differ("%g outside its domain", v, "a value", "BV_NUM_BAD");
        ++n_out;
    }
    if (bv_numfmt_iod_ok(v)) {
        const std::string w = std::to_string((int)v), got = text_of(bv_numfmt_iod(v));
        if (got != w) differ("(int)", v, got, w.c_str());
        ++n_iod;
    } else if (bv_numfmt_iod(v).kind != BV_NUM_BAD) differ("(int) outside its domain", v, "a value", "BV_NUM_BAD");
}
void check_both_signs(double v) { check(v); check(-v); }

void expect(bool ok, const char *what) {
    if (!ok) { std::fprintf(stderr, "expected: %s\n", what); std::exit(1); }
}
void expect_text(const std::string &got, const char *want, const char *what) {
    if (got != want) { std::fprintf(stderr, "%s: \"%s\", expected \"%s\"\n", what, got.c_str(), want); std::exit(1); }
}

uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int numbers() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    double d;
    uint64_t b = BV_NUMFMT_BITS_2M40;
    std::memcpy(&d, &b, 8); expect(d == std::ldexp(1.0, -40), "BV_NUMFMT_BITS_2M40 is 2^-40");
    b = BV_NUMFMT_BITS_999999_5;
    std::memcpy(&d, &b, 8); expect(d == 999999.5, "BV_NUMFMT_BITS_999999_5 is 999999.5");
    // ties of %f: every odd m / 128 up to m = 2^20
    for (uint32_t m = 1; m <= (1u << 20); m += 2) check_both_signs(m / 128.0);
    // ties of %g: odd c / 2^(6-E) in [10^E, 10^(E+1)) has seven significant digits, the last a 5, for every E that has any
    for (int E = -4; E <= 5; ++E) {
        const double unit = std::ldexp(1.0, E - 6), lo = std::pow(10.0, E), hi = std::pow(10.0, E + 1);
        uint64_t c = (uint64_t)std::ceil(lo / unit) | 1ull, n = 0;
        for (; c * unit < hi && c * unit < 999999.5; c += 2, ++n) check_both_signs(c * unit);
        expect(n > 0, "a %g tie at every E from -4 to 5");
    }
    expect_text(text_of(bv_numfmt_g6(13.0 / 128)), "0.101562", "13/128");
    expect_text(text_of(bv_numfmt_g6(12345.25)), "12345.2", "12345.25");
    expect_text(text_of(bv_numfmt_g6(100000.5)), "100000", "100000.5");
    expect_text(text_of(bv_numfmt_g6(100001.5)), "100002", "100001.5");
    // carries, the notation switch, powers of ten and their neighbours
    for (double v : {9.9999995, 0.9999995, 99999.95, 999999.4999, 9.9999996, 0.99999949999, 1e-4, std::nextafter(1e-4, 0.0), 1e-5, 1.5e-5, 0.5, 1.0, 20.0,
                     std::nextafter(20.0, 30.0), 5000.0, 10000.0})
        check_both_signs(v);
    for (int E = -13; E <= 6; ++E) {
        const double p = std::pow(10.0, E);
        for (double v : {p, std::nextafter(p, 0.0), std::nextafter(p, inf), 9.9999995 * p, 9.999995 * p, 1.0000005 * p}) check_both_signs(v);
    }
    for (int t = -45; t <= 64; ++t) {  // powers of two and their neighbours, across both domains' ends
        const double p = std::ldexp(1.0, t);
        for (double v : {p, std::nextafter(p, 0.0), std::nextafter(p, inf)}) check_both_signs(v);
    }
    // the ends of the domains
    const double g_lo = std::ldexp(1.0, -40), f_hi = std::ldexp(1.0, 63), i_hi = std::ldexp(1.0, 31);
    for (double s : {1.0, -1.0}) {
        expect(bv_numfmt_g6_ok(s * g_lo) && !bv_numfmt_g6_ok(s * std::nextafter(g_lo, 0.0)), "%g begins at 2^-40");
        expect(bv_numfmt_g6_ok(s * std::nextafter(999999.5, 0.0)) && !bv_numfmt_g6_ok(s * 999999.5) && !bv_numfmt_g6_ok(s * 1e6), "%g ends below 999999.5");
        expect(bv_numfmt_f6_ok(s * std::nextafter(f_hi, 0.0)) && !bv_numfmt_f6_ok(s * f_hi), "%f ends below 2^63");
        expect(bv_numfmt_iod_ok(s * std::nextafter(i_hi, 0.0)) && !bv_numfmt_iod_ok(s * i_hi), "(int) ends below 2^31");
        expect(bv_numfmt_g6_ok(s * 0.0) && bv_numfmt_f6_ok(s * 0.0) && bv_numfmt_iod_ok(s * 0.0), "zeros are inside");
        for (double v : {nan, inf}) expect(!bv_numfmt_g6_ok(s * v) && !bv_numfmt_f6_ok(s * v) && !bv_numfmt_iod_ok(s * v), "NaN and inf are outside");
        for (double v : {std::numeric_limits<double>::denorm_min(), std::numeric_limits<double>::min() / 2, std::numeric_limits<double>::min()})
            expect(!bv_numfmt_g6_ok(s * v) && bv_numfmt_f6_ok(s * v), "denormals: %f only");
    }
    for (double v : {0.0, std::numeric_limits<double>::denorm_min(), std::numeric_limits<double>::min(), 4e-7, 5e-7, 5.000001e-7, 1.5e-6, 2.5e-6, 0.5, 1.5, 2.5,
                     nan, inf, g_lo, std::nextafter(g_lo, 0.0), 999999.5, std::nextafter(999999.5, 0.0), f_hi, std::nextafter(f_hi, 0.0), i_hi, std::nextafter(i_hi, 0.0)})
        check_both_signs(v);
    expect_text(text_of(bv_numfmt_f6(-0.0)), "-0.000000", "-0.0");
    expect_text(text_of(bv_numfmt_f6(-1e-9)), "-0.000000", "-1e-9");
    expect_text(text_of(bv_numfmt_g6(-0.0)), "-0", "%g of -0.0");
    expect_text(text_of(bv_numfmt_iod(-0.5)), "0", "(int)-0.5");
    // uint32_t as (int), and as it is
    for (uint32_t u : {0u, 1u, 9u, 10u, 99999u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xffffffffu}) {
        expect_text(text_of(bv_numfmt_i32(u)), std::to_string((int)u).c_str(), "uint32_t as (int)");
        expect_text(text_of(bv_numfmt_u32(u)), std::to_string(u).c_str(), "uint32_t");
    }
    expect_text(text_of(bv_numfmt_i32(0x80000000u)), "-2147483648", "0x80000000");
    // seeded doubles from random bit patterns
    uint64_t seed = 20240607;
    const uint64_t N = 10000000;
    for (uint64_t i = 0; i < N; ++i) {
        const uint64_t bits = splitmix(seed);
        std::memcpy(&d, &bits, 8);
        check(d);
    }
    // seeded doubles in [0, 1) scaled by 10^0 .. 10^-11
    const uint64_t g_before = n_g6;
    for (uint64_t i = 0; i < N; ++i) {
        const double u = (double)(splitmix(seed) >> 11) * (1.0 / 9007199254740992.0);
        check(u * std::pow(10.0, -(double)(i % 12)));
    }
    const uint64_t g_scaled = n_g6 - g_before;
    std::printf("formatted: %%f %llu, %%g %llu, (int) %llu; outside %%g's domain %llu; of the scaled [0, 1) set %llu of %llu in %%g's domain\n",
                (unsigned long long)n_f6, (unsigned long long)n_g6, (unsigned long long)n_iod, (unsigned long long)n_out, (unsigned long long)g_scaled,
                (unsigned long long)N);
    if (g_scaled * 10 < N * 9) { std::fprintf(stderr, "fewer than 90 %% of the scaled set are in %%g's domain\n"); return 1; }
    return 0;
}

struct Reader {
    std::vector<uint8_t> data;
    size_t at = 0;
    const uint8_t *take(size_t n) {
        if (at + n > data.size()) { std::fprintf(stderr, "input ends early\n"); std::exit(2); }
        const uint8_t *p = data.data() + at;
        at += n;
        return p;
    }
    uint32_t u32() { uint32_t v; std::memcpy(&v, take(4), 4); return v; }
    std::string str() { const uint32_t n = u32(); return std::string(reinterpret_cast<const char *>(take(n)), n); }
};

void dump(FILE *f, const std::string &s) {
    const uint32_t n = (uint32_t)s.size();
    std::fwrite(&n, 4, 1, f);
    std::fwrite(s.data(), 1, n, f);
}

// IN:  u32 n_lines, u32 n_groups, the group names (u32 length, bytes); then per line u32 POS, CHROM (u32, bytes), u8 REF,
//      u32 n_tokens and the indel tokens (u32, bytes), a bv_site_result, n_groups bv_group_result.
// OUT: per line u8 on_device, u8 gt[4], then (u32 length, bytes) of format_vcf_head, format_cvg_line and indel_string.
int lines(const char *in_path, const char *out_path) {
    Reader in;
    FILE *fi = std::fopen(in_path, "rb");
    if (!fi) { std::perror(in_path); return 2; }
    uint8_t buf[1 << 16];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, fi)) > 0;) in.data.insert(in.data.end(), buf, buf + n);
    std::fclose(fi);
    FILE *fo = std::fopen(out_path, "wb");
    if (!fo) { std::perror(out_path); return 2; }
    const uint32_t n_lines = in.u32(), n_groups = in.u32();
    std::vector<std::string> names;
    std::string name_bytes;
    std::vector<uint32_t> name_off(1, 0);
    for (uint32_t j = 0; j < n_groups; ++j) {
        names.push_back(in.str());
        name_bytes += names.back();
        name_off.push_back((uint32_t)name_bytes.size());
    }
    uint64_t on_dev = 0;
    for (uint32_t k = 0; k < n_lines; ++k) {
        bvamd::SiteText st;
        st.ref_pos = in.u32();
        st.ref_id = in.str();
        st.ref_base = std::string(1, (char)*in.take(1));
        for (uint32_t t = in.u32(); t > 0; --t) st.indel_tokens.push_back(in.str());
        bv_site_result r;
        std::memcpy(&r, in.take(sizeof r), sizeof r);
        std::vector<bv_group_result> g(n_groups);
        if (n_groups) std::memcpy(g.data(), in.take(n_groups * sizeof(bv_group_result)), n_groups * sizeof(bv_group_result));
        if (r.n_alt > BV_MAX_ALT) { std::fprintf(stderr, "line %u: n_alt %u\n", k, r.n_alt); return 2; }
        const std::string indel = bvamd::indel_string(st.indel_tokens);
        const bool on = bv_rt_on_device(&r, n_groups ? g.data() : nullptr, n_groups);
        uint8_t gt_host[4], gt_core[4];
        bvamd::vcf_gt_codes(st, r, gt_host);
        bv_rt_gt_codes(&r, (uint8_t)st.ref_base[0], gt_core);
        if (std::memcmp(gt_host, gt_core, 4)) { std::fprintf(stderr, "line %u: gt differs\n", k); return 1; }
        // a record the formatters cannot be asked about (NaN to int is undefined) is the host's to print, but not here
        const bool askable = bv_numfmt_iod_ok(r.mq_ranksum) && bv_numfmt_iod_ok(r.rpr_ranksum) && bv_numfmt_iod_ok(r.bq_ranksum);
        const std::string vcf = !askable ? std::string() : bvamd::format_vcf_head(st, r, n_groups ? g.data() : nullptr, names);
        const std::string cvg = bvamd::format_cvg_line(st, r);
        bv_rt_ctx c;
        c.r = &r; c.g = g.data(); c.names = reinterpret_cast<const uint8_t *>(name_bytes.data()); c.name_off = name_off.data();
        c.chrom = reinterpret_cast<const uint8_t *>(st.ref_id.data()); c.chrom_len = (uint32_t)st.ref_id.size();
        c.indel = reinterpret_cast<const uint8_t *>(indel.data()); c.indel_len = indel == "." ? 0u : (uint32_t)indel.size();
        c.n_groups = n_groups; c.pos = st.ref_pos; c.ref = (uint8_t)st.ref_base[0];
        uint32_t bad[2];
        bool few = r.n_alt <= BV_RT_MAX_ALT;  // a record of four ALTs is the host's
        for (const bv_group_result &x : g) few = few && x.n_alt <= BV_RT_MAX_ALT;
        for (int cv = 0; cv < 2; ++cv) {
            const uint64_t len = bv_rt_line(&c, cv != 0, nullptr, &bad[cv]);
            std::vector<uint8_t> out(len + 32, '#');
            const uint64_t len2 = bv_rt_line(&c, cv != 0, out.data() + 16, nullptr);
            for (size_t i = 0; i < out.size(); ++i)
                if ((i < 16 || i >= 16 + len) && out[i] != '#') { std::fprintf(stderr, "line %u: the core wrote outside its line\n", k); return 1; }
            const std::string &want = cv ? cvg : vcf;
            if (len2 != len) { std::fprintf(stderr, "line %u: counted %llu, wrote %llu\n", k, (unsigned long long)len, (unsigned long long)len2); return 1; }
            if (few && bad[cv] == 0xffffffffu && std::string(reinterpret_cast<char *>(out.data() + 16), len) != want) {
                std::fprintf(stderr, "line %u, %s: core\n%.*s\nhost\n%s\n", k, cv ? "CVG" : "VCF", (int)len, out.data() + 16, want.c_str());
                return 1;
            }
        }
        if (on != (few && bad[0] == 0xffffffffu && bad[1] == 0xffffffffu)) { std::fprintf(stderr, "line %u: the predicate and the items disagree\n", k); return 1; }
        on_dev += on;
        const uint8_t flag = on;
        std::fwrite(&flag, 1, 1, fo);
        std::fwrite(gt_host, 1, 4, fo);
        dump(fo, vcf); dump(fo, cvg); dump(fo, indel);
    }
    if (std::fclose(fo)) { std::perror(out_path); return 2; }
    std::printf("lines %u, on the device %llu\n", n_lines, (unsigned long long)on_dev);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "numbers")) return numbers();
    if (argc == 4 && !std::strcmp(argv[1], "lines")) return lines(argv[2], argv[3]);
    std::fprintf(stderr, "usage: record_text_check numbers | lines IN OUT\n");
    return 2;
}
