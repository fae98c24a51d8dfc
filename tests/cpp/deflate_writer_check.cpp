// deflate_writer_check -- the two ways of TextOut (basevar_amd/host/bgzf_tabix.hpp) to write the same lines, without a GPU:
// write_lines() as it is (zlib, a block at a time) and write_lines() with a BlockDeflater, here the CPU build of the device
// encoder's core (basevar_amd/csrc/bv_deflate_core.h).  tests/test_deflate_cpu.py compares the two files and their indexes.
//
//   deflate_writer_check LINES HOST.gz BATCH.gz SEED
//
// LINES: '#' header lines, then data lines (sequence name, position, ...).  The header goes through write_header(); the data
// lines go to both outputs in the same batches of whole lines, of seeded sizes from one line to a few hundred KiB, some empty.
// Prints the number of deflater calls and of blocks they were given.
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
#include "../../basevar_amd/host/bgzf_tabix.hpp"

int main(int argc, char **argv) {
    if (argc < 5) { std::cerr << "usage: deflate_writer_check LINES HOST.gz BATCH.gz SEED\n"; return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { std::cerr << "cannot read " << argv[1] << "\n"; return 2; }
    const std::string all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    uint64_t rng = std::strtoull(argv[4], nullptr, 10) * 2654435761ull + 12345;
    auto below = [&](uint32_t n) { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng >> 33) % n; };

    std::vector<uint32_t> crc_tab(1024);
    bv_inf_crc_tables(crc_tab.data(), 0, 1);
    std::unique_ptr<BvDefState> S(new BvDefState());
    size_t calls = 0, blocks = 0;
    const bvamd::BlockDeflater deflate = [&](const char *text, uint64_t text_bytes, const uint64_t *block_off, uint32_t n, uint8_t *dst, uint64_t *member_off) {
        ++calls; blocks += n;
        member_off[0] = 0;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t len = (uint32_t)(block_off[k + 1] - block_off[k]);
            // (a member through a buffer of its own worst case: the writer promised text_bytes + 31 * n in all)
            std::vector<uint8_t> m(len + BV_DEF_MEMBER_EXTRA);
            const std::vector<uint8_t> t(text + block_off[k], text + block_off[k + 1]);
            const uint32_t total = bv_def_member(t.data(), len, m.data(), S.get(), crc_tab.data(), 0, 1, [](uint32_t v) { return v; });
            if (member_off[k] + total > text_bytes + 31ull * n) std::abort();
            std::copy(m.begin(), m.begin() + total, dst + member_off[k]);
            member_off[k + 1] = member_off[k] + total;
        }
    };

    size_t p = 0;
    while (p < all.size() && all[p] == '#') p = all.find('\n', p) + 1;
    bvamd::TextOut host, batch;
    host.open(argv[2]);
    batch.open(argv[3]);
    host.write_header(all.substr(0, p));
    batch.write_header(all.substr(0, p));
    while (p < all.size()) {
        const uint32_t kind = below(8);
        size_t want = kind == 0 ? 0 : kind < 3 ? 1 : kind < 6 ? below(70000) : below(400000);
        size_t e = p;
        while (e < all.size() && (e - p < want || (e == p && kind != 0))) e = all.find('\n', e) + 1;
        const std::string lines = all.substr(p, e - p);
        host.write_lines(lines);
        batch.write_lines(lines, deflate);
        p = e;
    }
    host.close();
    batch.close();
    std::printf("%zu %zu\n", calls, blocks);
    return 0;
}
