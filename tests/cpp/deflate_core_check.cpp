// deflate_core_check -- the device DEFLATE encoder's shared cores (basevar_amd/csrc/bv_deflate_core.h and, for the small level,
// bv_deflate_small_core.h) as a plain host program, built under ASan + UBSan (make sanitize) and driven by
// tests/test_deflate_cpu.py and tests/test_deflate_small_cpu.py; the GPU tests compare the device's members with this
// program's, byte for byte.
//
//   deflate_core_check [--level fast|small] TEXT OUT [BLOCK_BYTES | @SIZES]
//
// cuts TEXT into blocks of BLOCK_BYTES (default 0xff00), or into the block lengths listed one per line in the file SIZES (which
// must add up to TEXT's size), codes every block at the level (default fast) as lane 0 of 1 and writes the BGZF members back to
// back to OUT.  Every member gets a buffer of exactly its worst case, text + 31 bytes, and at the small level every token run
// exactly BV_DEFS_TOK_ROOM, so that ASan sees a write behind either.
//
//   deflate_core_check --lengths VECTORS
//
// reads one count vector per line of VECTORS, `LIMIT N c0 c1 .. c(N-1)`, and prints per line `ROUNDS l0 l1 .. l(N-1)`: the
// code lengths of bv_defs_code_lengths and the rounds of halving it took.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../basevar_amd/csrc/bv_deflate_small_core.h"

static int lengths_mode(const char *path) {
    std::ifstream in(path);
    if (!in) { std::cerr << "cannot read " << path << "\n"; return 2; }
    std::unique_ptr<BvDefsHuff> H(new BvDefsHuff());
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        uint32_t limit = 0, n = 0;
        ls >> limit >> n;
        if (n < 2 || n > BV_DEFS_MAX_SYMS || limit < 1 || limit > 15 || n > (1u << limit)) { std::cerr << "a vector of " << n << " counts with limit " << limit << "\n"; return 2; }
        std::vector<uint32_t> counts(n);
        uint64_t sum = 0;
        for (uint32_t &c : counts) { ls >> c; sum += c; }
        if (!ls || sum >> 32) { std::cerr << "a short line, or counts that add up to 2^32 or more\n"; return 2; }
        std::vector<uint8_t> len(n);
        const uint32_t rounds = bv_defs_code_lengths(counts.data(), n, limit, len.data(), H.get(), 0, 1);
        std::cout << rounds;
        for (uint8_t l : len) std::cout << ' ' << (unsigned)l;
        std::cout << '\n';
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "--lengths")) return lengths_mode(argv[2]);
    bool small = false;
    if (argc > 2 && !std::strcmp(argv[1], "--level")) {
        small = !std::strcmp(argv[2], "small");
        if (!small && std::strcmp(argv[2], "fast")) { std::cerr << "the level is fast or small\n"; return 2; }
        argc -= 2; argv += 2;
    }
    if (argc < 3) { std::cerr << "usage: deflate_core_check [--level fast|small] TEXT OUT [BLOCK_BYTES | @SIZES]\n       deflate_core_check --lengths VECTORS\n"; return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { std::cerr << "cannot read " << argv[1] << "\n"; return 2; }
    const std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<size_t> sizes;
    if (argc > 3 && argv[3][0] == '@') {
        std::ifstream sf(argv[3] + 1);
        size_t v, sum = 0;
        while (sf >> v) { sizes.push_back(v); sum += v; }
        if (sum != raw.size()) { std::cerr << "the sizes add up to " << sum << ", the text has " << raw.size() << " bytes\n"; return 2; }
    } else {
        const size_t block = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : BV_DEF_MAX_BLOCK;
        if (block < 1) { std::cerr << "block bytes must be positive\n"; return 2; }
        for (size_t at = 0; at < raw.size(); at += block) sizes.push_back(raw.size() - at < block ? raw.size() - at : block);
    }
    std::vector<uint32_t> crc_tab(1024);
    bv_inf_crc_tables(crc_tab.data(), 0, 1);
    std::unique_ptr<BvDefState> S(small ? nullptr : new BvDefState());  // the state of the level that was asked for, and no other
    std::unique_ptr<BvDefSmallState> SS(small ? new BvDefSmallState() : nullptr);
    const auto same = [](uint32_t v) { return v; };
    std::ofstream out(argv[2], std::ios::binary);
    size_t at = 0;
    for (size_t n : sizes) {
        if (n < 1 || n > BV_DEF_MAX_BLOCK) { std::cerr << "a block of " << n << " bytes: 1 to 65280 are coded\n"; return 2; }
        // (a copy of exactly n bytes: a read behind the block is a finding too)
        const std::vector<uint8_t> text(raw.begin() + at, raw.begin() + at + n);
        std::vector<uint8_t> member(n + BV_DEF_MEMBER_EXTRA);
        std::vector<uint32_t> tok(small ? BV_DEFS_TOK_ROOM((uint32_t)n) : 0u);
        const uint32_t total = small ? bv_def_small_member(text.data(), (uint32_t)n, member.data(), SS.get(), tok.data(), crc_tab.data(), 0, 1, same)
                                     : bv_def_member(text.data(), (uint32_t)n, member.data(), S.get(), crc_tab.data(), 0, 1, same);
        if (total > member.size()) { std::cerr << "a member of " << total << " bytes for " << n << " bytes of text\n"; return 1; }
        out.write(reinterpret_cast<const char *>(member.data()), total);
        at += n;
    }
    out.close();
    if (!out) { std::cerr << "cannot write " << argv[2] << "\n"; return 2; }
    return 0;
}
