// indel_tally_check.cpp -- basevar_amd/csrc/bv_indel_tally_core.h, the definition the kernels of bv_indel_tally.hip compile,
// held to host/vcf_emit.hpp's indel_string byte for byte.  A stand-alone program (tests/indel_tally_ref.py builds it, with
// ASan + UBSan for tests/test_indel_tally_cpu.py); every working array has exactly the size the core is promised.
//
//   indel_tally_check rows IN OUT   IN: u64 n_tokens, u64 text_bytes, u32 n_keys, tokens [n_tokens] (bv_pileup_token's layout,
//                                   ascending by pos), text, keys [n_keys].  Per key the core's flag, length and column against
//                                   indel_string over the row's tokens: inside the domain the same bytes ("." for the empty
//                                   column), outside it flagged, and flagged only then.  OUT, per key: u8 flag, u32 tokens of
//                                   the row, u32 classes, u32 greatest count, u32 column bytes, the column.
//   indel_tally_check time IN       the same IN: seconds of one host thread making the row's strings and indel_string for every
//                                   key (what bv_call did per row), best of five passes
//   indel_tally_check order         bv_it_cmp against std::string's order on pairs built for every edge of the key and of the
//                                   byte compare; prints the number of pairs
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../basevar_amd/csrc/bv_indel_tally_core.h"
#include "../../basevar_amd/host/vcf_emit.hpp"

static int fail(const std::string &m) {
    std::fprintf(stderr, "indel_tally_check: %s\n", m.c_str());
    return 1;
}

static int sign(int v) { return v < 0 ? -1 : v > 0 ? 1 : 0; }

// a text in a buffer of exactly its size
static std::unique_ptr<uint8_t[]> exact(const std::string &a) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[a.size()]);
    std::memcpy(p.get(), a.data(), a.size());
    return p;
}

static int run_order() {
    const unsigned char edge[] = {0x00, 0x01, '+', '-', 'A', 'a', 0x7f, 0x80, 0x81, 0xff};
    const size_t lens[] = {0, 1, 2, 3, 4, 5, 6, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 9000};
    std::vector<std::string> texts;
    for (size_t len : lens) {
        std::string base(len, 'G');
        for (size_t i = 0; i < len; ++i) base[i] = "ACGT"[(i * 7 + len) % 4];
        texts.push_back(base);
        // the deciding byte at every place near the key's edge and at the text's end, of every edge value
        for (size_t at : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)4, (size_t)5, len / 2, len - 2, len - 1})
            if (at < len)
                for (unsigned char v : edge) { std::string t = base; t[at] = (char)v; texts.push_back(t); }
        if (len) texts.push_back(base + std::string(1, '\0'));  // a proper prefix of a text that goes on with a zero byte
    }
    uint64_t pairs = 0;
    std::vector<std::unique_ptr<uint8_t[]>> held;
    for (const std::string &a : texts) held.push_back(exact(a));
    for (size_t i = 0; i < texts.size(); ++i)
        for (size_t j = 0; j < texts.size(); ++j) {
            const std::string &a = texts[i], &b = texts[j];
            const uint8_t *pa = held[i].get(), *pb = held[j].get();
            const int got = sign(bv_it_cmp(bv_it_key(pa, (uint32_t)a.size()), pa, (uint32_t)a.size(), bv_it_key(pb, (uint32_t)b.size()), pb, (uint32_t)b.size()));
            const int want = sign(a.compare(b));  // (char_traits<char>::compare: unsigned bytes)
            if (want != got) return fail("order: a text of " + std::to_string(a.size()) + " bytes against one of " + std::to_string(b.size()) + ": " + std::to_string(got) + ", std::string says " + std::to_string(want));
            if ((std::map<std::string, int>().key_comp()(a, b) ? -1 : 0) != (got < 0 ? -1 : 0)) return fail("order: std::map's order differs");
            ++pairs;
        }
    std::printf("order: %llu pairs\n", (unsigned long long)pairs);
    return 0;
}

template <class T>
static void put(std::string &o, T v) { o.append(reinterpret_cast<const char *>(&v), sizeof v); }

struct Input {
    uint64_t n_tokens = 0, text_bytes = 0;
    std::vector<bv_it_token> tok;
    std::unique_ptr<uint8_t[]> text;  // (exactly text_bytes: a read beyond the text is ASan's)
    std::vector<uint32_t> keys;
};

static bool read_input(const char *in_path, Input &in) {
    std::ifstream f(in_path, std::ios::binary);
    if (!f) return false;
    uint32_t n_keys = 0;
    f.read(reinterpret_cast<char *>(&in.n_tokens), 8); f.read(reinterpret_cast<char *>(&in.text_bytes), 8); f.read(reinterpret_cast<char *>(&n_keys), 4);
    if (!f) return false;
    in.tok.resize(in.n_tokens);
    in.text.reset(new uint8_t[in.text_bytes]);
    in.keys.resize(n_keys);
    f.read(reinterpret_cast<char *>(in.tok.data()), (std::streamsize)(sizeof(bv_it_token) * in.n_tokens));
    f.read(reinterpret_cast<char *>(in.text.get()), (std::streamsize)in.text_bytes);
    f.read(reinterpret_cast<char *>(in.keys.data()), 4ll * n_keys);
    return (bool)f;
}

static bool pos_below(const bv_it_token &x, const bv_it_token &y) { return x.pos < y.pos; }

static int run_time(const char *in_path) {
    Input in;
    if (!read_input(in_path, in)) return fail("cannot read the input");
    double best = 1e30;
    uint64_t bytes = 0, columns = 0;
    for (int pass = 0; pass < 5; ++pass) {
        const auto t0 = std::chrono::steady_clock::now();
        bytes = columns = 0;
        for (uint32_t key : in.keys) {
            const auto range = std::equal_range(in.tok.begin(), in.tok.end(), bv_it_token{key, 0, 0, 0, 0}, pos_below);
            if (range.first == range.second) continue;
            std::vector<std::string> strings;
            for (auto it = range.first; it != range.second; ++it) strings.emplace_back(reinterpret_cast<const char *>(in.text.get()) + it->text_off, it->text_len);
            const std::string column = bvamd::indel_string(strings);
            bytes += column.size(); ++columns;
        }
        best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    std::printf("time: %.6f s for %llu columns of %llu bytes from %llu tokens, %zu keys\n", best, (unsigned long long)columns, (unsigned long long)bytes,
                (unsigned long long)in.n_tokens, in.keys.size());
    return 0;
}

static int run_rows(const char *in_path, const char *out_path) {
    Input in;
    if (!read_input(in_path, in)) return fail("cannot read the input");
    const uint64_t text_bytes = in.text_bytes;
    const std::vector<bv_it_token> &tok = in.tok;
    const std::unique_ptr<uint8_t[]> &text = in.text;
    const std::vector<uint32_t> &keys = in.keys;
    const uint32_t n_keys = (uint32_t)keys.size();
    std::string out;
    for (uint32_t k = 0; k < n_keys; ++k) {
        const auto range = std::equal_range(tok.begin(), tok.end(), bv_it_token{keys[k], 0, 0, 0, 0}, pos_below);
        const uint32_t n = (uint32_t)(range.second - range.first);
        std::vector<std::string> strings;
        for (auto it = range.first; it != range.second; ++it) {
            if (!bv_it_token_ok(&*it, text_bytes)) return fail("a token of the input runs beyond the text");
            strings.emplace_back(reinterpret_cast<const char *>(text.get()) + it->text_off, it->text_len);
        }
        const std::string want = bvamd::indel_string(strings);
        std::map<std::string, uint32_t> tally;
        for (const std::string &s : strings)
            if (!s.empty() && s[0] != 'N' && s[0] != 'A' && s[0] != 'C' && s[0] != 'G' && s[0] != 'T') ++tally[s];
        uint32_t most = 0;
        for (const auto &kv : tally) most = std::max(most, kv.second);
        const bool inside = n <= BV_INDEL_ROW_TOKENS_MAX && (want == "." || want.size() <= BV_IT_COLUMN_MAX);
        // the core, over working arrays of exactly the promised sizes
        const uint32_t held = std::min(n, BV_INDEL_ROW_TOKENS_MAX), classes = std::min(held, BV_IT_CLASSES_MAX);
        std::unique_ptr<uint32_t[]> key(new uint32_t[held]);
        std::unique_ptr<uint16_t[]> cls(new uint16_t[held]), rep(new uint16_t[classes]), cnt(new uint16_t[classes]);
        bv_it_row r{n ? &*range.first : nullptr, text.get(), n, key.get(), cls.get(), rep.get(), cnt.get()};
        uint32_t n_cls = 0;
        const int flag = bv_it_classify(&r, text_bytes, &n_cls);
        if (flag == BV_IT_BAD) return fail("key " + std::to_string(k) + ": BV_IT_BAD on tokens inside the text");
        if ((flag == BV_IT_OK) != inside)
            return fail("key " + std::to_string(k) + ": flag " + std::to_string(flag) + " on a row of " + std::to_string(n) + " tokens whose column has " + std::to_string(want.size()) + " bytes");
        std::string column;
        if (flag == BV_IT_OK) {
            const uint32_t len = bv_it_column_len(&r, n_cls);
            std::unique_ptr<uint8_t[]> col(new uint8_t[len]);
            bv_it_column_put(&r, n_cls, col.get());
            column.assign(reinterpret_cast<const char *>(col.get()), len);
            if ((column.empty() ? std::string(".") : column) != want)
                return fail("key " + std::to_string(k) + ": the core's column of " + std::to_string(len) + " bytes is not indel_string's of " + std::to_string(want.size()));
            if (n_cls != tally.size()) return fail("key " + std::to_string(k) + ": " + std::to_string(n_cls) + " classes, the map has " + std::to_string(tally.size()));
        }
        put<uint8_t>(out, (uint8_t)flag); put<uint32_t>(out, n); put<uint32_t>(out, (uint32_t)tally.size()); put<uint32_t>(out, most);
        put<uint32_t>(out, (uint32_t)column.size());
        out += column;
    }
    std::ofstream o(out_path, std::ios::binary);
    o.write(out.data(), (std::streamsize)out.size());
    return o ? 0 : fail("cannot write the output");
}

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "order") return run_order();
    if (argc == 4 && std::string(argv[1]) == "rows") return run_rows(argv[2], argv[3]);
    if (argc == 3 && std::string(argv[1]) == "time") return run_time(argv[2]);
    return fail("usage: indel_tally_check rows IN OUT | time IN | order");
}
