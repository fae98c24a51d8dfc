// deflate_core_check -- the device DEFLATE encoder's shared core (basevar_amd/csrc/bv_deflate_core.h) as a plain host program,
// built under ASan + UBSan (make sanitize) and driven by tests/test_deflate_cpu.py; the GPU test compares the device's members
// with this program's, byte for byte.
//
//   deflate_core_check TEXT OUT [BLOCK_BYTES | @SIZES]
//
// cuts TEXT into blocks of BLOCK_BYTES (default 0xff00), or into the block lengths listed one per line in the file SIZES (which
// must add up to TEXT's size), codes every block as lane 0 of 1 and writes the BGZF members back to back to OUT.  Every
// member gets a buffer of exactly its worst case, text + 31 bytes, so that ASan sees a write behind it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../basevar_amd/csrc/bv_deflate_core.h"

int main(int argc, char **argv) {
    if (argc < 3) { std::cerr << "usage: deflate_core_check TEXT OUT [BLOCK_BYTES | @SIZES]\n"; return 2; }
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
    std::unique_ptr<BvDefState> S(new BvDefState());
    std::ofstream out(argv[2], std::ios::binary);
    size_t at = 0;
    for (size_t n : sizes) {
        if (n < 1 || n > BV_DEF_MAX_BLOCK) { std::cerr << "a block of " << n << " bytes: 1 to 65280 are coded\n"; return 2; }
        // (a copy of exactly n bytes: a read behind the block is a finding too)
        const std::vector<uint8_t> text(raw.begin() + at, raw.begin() + at + n);
        std::vector<uint8_t> member(n + BV_DEF_MEMBER_EXTRA);
        const uint32_t total = bv_def_member(text.data(), (uint32_t)n, member.data(), S.get(), crc_tab.data(), 0, 1, [](uint32_t v) { return v; });
        if (total > member.size()) { std::cerr << "a member of " << total << " bytes for " << n << " bytes of text\n"; return 1; }
        out.write(reinterpret_cast<const char *>(member.data()), total);
        at += n;
    }
    out.close();
    if (!out) { std::cerr << "cannot write " << argv[2] << "\n"; return 2; }
    return 0;
}
