// Test infrastructure (tests/ only, host code, its own main): basevar_amd/csrc/bv_text_tokens_core.h -- the code the kernels of
// bv_text_tokens.hip compile -- held to the tokens the host collects today, byte for byte and in order:
//   * the host reader (host/batchfile_fast.hpp, parse_site_rows_fast) on every position in state 0, and
//   * the walk of a marked row that BaseTypeEngine::finish_text makes (host/indel_tokens.hpp: row_indel_tokens),
// on the batches tests/text_tokens_model.py writes.  The core is also run over the rows of every other position (a row it is
// never asked about on the device may be anything: it must stay inside the row).  The list goes to a dump that the Python
// model compares and from which tests/test_text_tokens_cpu.py asserts the corpus's reach.  Built with ASan + UBSan and run as
// a program.
//
//   text_tokens_check <in> <out>     exit 0: all agree
//   text_tokens_check walk <in>      what the host route costs on one thread (tools/text_tokens_bench.py): finish_text's walk of the
//                                    marked rows of the state-0 positions, a std::string a token, then the descriptors and the text
//                                    laid out as bv_call --emit device lays them out (TokenList::from_site_texts); best of 5 passes
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../basevar_amd/csrc/bv_text_tokens_core.h"
#include "../../basevar_amd/host/batchfile_fast.hpp"
#include "../../basevar_amd/host/indel_tokens.hpp"

namespace {

struct Token {
    uint32_t pos, sample, file;
    std::string text;
};

template <class T>
T get(std::istream &in) {
    T v;
    in.read(reinterpret_cast<char *>(&v), sizeof v);
    if (!in) throw std::runtime_error("short input");
    return v;
}
template <class T>
void put(std::ostream &o, T v) { o.write(reinterpret_cast<const char *>(&v), sizeof v); }

// the core's tokens of one row (with its line break), exactly sized buffers so that ASan sees a store beyond the counts
std::vector<Token> core_row(const std::string &row, uint32_t pos, uint32_t file, uint32_t sample0) {
    uint32_t n_txt = 0;
    const uint32_t n = bv_tt_row_serial(row.data(), (uint32_t)row.size(), pos, sample0, nullptr, nullptr, &n_txt);
    std::vector<bv_tt_token> tok(n);
    std::vector<uint8_t> text(n_txt);
    for (bv_tt_token &t : tok) t.text_len = 0xFFFFFFFFu;
    uint32_t n_txt2 = 0;
    const uint32_t n2 = bv_tt_row_serial(row.data(), (uint32_t)row.size(), pos, sample0, tok.data(), text.data(), &n_txt2);
    if (n2 != n || n_txt2 != n_txt) throw std::runtime_error("count and write passes disagree");
    std::vector<Token> out;
    uint64_t end = 0;
    for (const bv_tt_token &t : tok) {
        if (t.pos != pos || t.reserved_ || t.text_len == 0 || t.text_len == 0xFFFFFFFFu || t.text_off != end || t.text_off + t.text_len > n_txt)
            throw std::runtime_error("a descriptor of position " + std::to_string(pos) + " is out of place");
        end = t.text_off + t.text_len;
        Token k;
        k.pos = pos; k.sample = t.sample; k.file = file;
        k.text.assign(reinterpret_cast<const char *>(text.data()) + t.text_off, t.text_len);
        out.push_back(k);
    }
    if (end != n_txt) throw std::runtime_error("text bytes outside every descriptor");
    return out;
}

struct WalkBatch {
    uint32_t P = 0, F = 0;
    std::vector<uint8_t> state;
    std::vector<std::string> rows;  // [P * F], each with its line break
};

int time_walk(const char *path) {
    std::ifstream in(path, std::ios::binary);
    char magic[4];
    in.read(magic, 4);
    if (!in || std::memcmp(magic, "TTIN", 4) || get<uint32_t>(in) != 1) throw std::runtime_error("walk: a TTIN file of one batch");
    WalkBatch b;
    b.P = get<uint32_t>(in); b.F = get<uint32_t>(in);
    for (uint32_t f = 0; f < b.F; ++f) (void)get<uint32_t>(in);
    b.state.resize(b.P);
    in.read(reinterpret_cast<char *>(b.state.data()), b.P);
    b.rows.resize((size_t)b.P * b.F);
    for (std::string &r : b.rows) {
        r.resize(get<uint32_t>(in));
        in.read(&r[0], (std::streamsize)r.size());
    }
    if (!in) throw std::runtime_error("walk: short input");
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double best_walk = 1e30, best_layout = 1e30;
    size_t n_rows = 0, n_tokens = 0, n_text = 0;
    for (int pass = 0; pass < 5; ++pass) {
        const double t0 = now();
        std::vector<bvamd::SiteText> per_pos(b.P);
        n_rows = 0;
        for (uint32_t p = 0; p < b.P; ++p) {
            if (b.state[p]) continue;
            for (uint32_t f = 0; f < b.F; ++f) {
                const std::string &row = b.rows[(size_t)p * b.F + f];
                if (row.find_first_of("+-") == std::string::npos) continue;  // (the device's mark says more; a row without either byte has no token)
                ++n_rows;
                bvamd::row_indel_tokens(row.c_str(), per_pos[p].indel_tokens);
            }
        }
        const double t1 = now();
        const bvamd::TokenList list = bvamd::TokenList::from_site_texts(per_pos, 1);
        const double t2 = now();
        best_walk = std::min(best_walk, t1 - t0);
        best_layout = std::min(best_layout, t2 - t1);
        n_tokens = list.tokens.size(); n_text = list.text.size();
    }
    std::printf("walk: rows %zu tokens %zu text %zu walk_ms %.3f layout_ms %.3f\n", n_rows, n_tokens, n_text, 1e3 * best_walk, 1e3 * best_layout);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && std::string(argv[1]) == "walk") {
        try { return time_walk(argv[2]); } catch (const std::exception &e) { std::cerr << "text_tokens_check: " << e.what() << "\n"; return 1; }
    }
    if (argc != 3) {
        std::cerr << "usage: text_tokens_check <in> <out>\n";
        return 2;
    }
    try {
        std::ifstream in(argv[1], std::ios::binary);
        std::ofstream out(argv[2], std::ios::binary);
        char magic[4];
        in.read(magic, 4);
        if (!in || std::memcmp(magic, "TTIN", 4)) throw std::runtime_error("not a TTIN file");
        const uint32_t n_batches = get<uint32_t>(in);
        size_t n_all = 0, n_rows = 0;
        for (uint32_t b = 0; b < n_batches; ++b) {
            const uint32_t P = get<uint32_t>(in), F = get<uint32_t>(in);
            std::vector<uint32_t> fs(F), foff(F);
            uint32_t N = 0;
            for (uint32_t f = 0; f < F; ++f) { fs[f] = get<uint32_t>(in); foff[f] = N; N += fs[f]; }
            std::vector<uint8_t> state(P);
            in.read(reinterpret_cast<char *>(state.data()), P);
            std::vector<Token> list;
            for (uint32_t p = 0; p < P; ++p) {
                std::vector<std::string> rows(F), lines(F);
                for (uint32_t f = 0; f < F; ++f) {
                    const uint32_t len = get<uint32_t>(in);
                    rows[f].resize(len);
                    in.read(&rows[f][0], len);
                    if (!in || rows[f].back() != '\n') throw std::runtime_error("a row without its line break");
                    lines[f] = rows[f].substr(0, len - 1);
                }
                std::vector<Token> pos_tokens;
                for (uint32_t f = 0; f < F; ++f) {
                    ++n_rows;
                    const std::vector<Token> got = core_row(rows[f], p, f, foff[f]);  // (every row: it stays inside the row whatever the row is)
                    if (state[p]) continue;
                    std::vector<std::string> walk;
                    bvamd::row_indel_tokens(rows[f].c_str(), walk);
                    if (walk.size() != got.size()) throw std::runtime_error("batch " + std::to_string(b) + " position " + std::to_string(p) + ": the core has " +
                                                                            std::to_string(got.size()) + " tokens, finish_text's walk " + std::to_string(walk.size()));
                    for (size_t i = 0; i < got.size(); ++i)
                        if (walk[i] != got[i].text) throw std::runtime_error("batch " + std::to_string(b) + " position " + std::to_string(p) + ": token " + std::to_string(i) + " differs from finish_text's walk");
                    pos_tokens.insert(pos_tokens.end(), got.begin(), got.end());
                }
                if (state[p]) continue;
                bvamd::SlabBuilder sb(N);
                bvamd::SiteText st;
                if (!bvamd::parse_site_rows_fast(lines, N, sb, st)) throw std::runtime_error("batch " + std::to_string(b) + " position " + std::to_string(p) + ": the host reader skips a position of state 0");
                if (st.indel_tokens.size() != pos_tokens.size()) throw std::runtime_error("batch " + std::to_string(b) + " position " + std::to_string(p) + ": the host reader has another count");
                for (size_t i = 0; i < pos_tokens.size(); ++i)
                    if (st.indel_tokens[i] != pos_tokens[i].text) throw std::runtime_error("batch " + std::to_string(b) + " position " + std::to_string(p) + ": token " + std::to_string(i) + " differs from the host reader's");
                list.insert(list.end(), pos_tokens.begin(), pos_tokens.end());
            }
            put<uint64_t>(out, list.size());
            for (const Token &t : list) {
                put<uint32_t>(out, t.pos); put<uint32_t>(out, t.sample); put<uint32_t>(out, t.file); put<uint32_t>(out, (uint32_t)t.text.size());
                out.write(t.text.data(), (std::streamsize)t.text.size());
            }
            n_all += list.size();
        }
        out.flush();
        if (!out) throw std::runtime_error("cannot write the dump");
        std::cout << "text_tokens_check: " << n_batches << " batches, " << n_rows << " rows, " << n_all << " tokens agree\n";
    } catch (const std::exception &e) {
        std::cerr << "text_tokens_check: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
