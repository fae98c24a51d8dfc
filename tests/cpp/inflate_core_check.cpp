// inflate_core_check.cpp -- the CPU build of the device DEFLATE decoder (basevar_amd/csrc/bv_inflate_core.h) against zlib.
//
//   inflate_core_check CORPUS
//
// CORPUS: u32 n, then n x (u32 length, the bytes of one BGZF member), little endian (tests/bgzf_corpus.py writes it).
// zlib is the judge of every member: raw inflate() of the payload into exactly ISIZE bytes.  Where it ends with Z_STREAM_END,
// fills them and their crc32() is the member's, the core must say OK and give zlib's bytes; otherwise the core must not say OK.
// The category (header / deflate / size / crc) is compared too; where it differs the line says so and the run still passes.
// Guard bytes around the output range and around a private copy of the payload must stay as they were; the sanitizers
// (`make sanitize`: inflate_core_check.asan) watch every access.  One line per member on stdout:
//   index core_status zlib_status block_mask isize
// Exit status 0: every member agrees; 1: a disagreement (named on stderr).
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../basevar_amd/csrc/bv_inflate_core.h"

namespace {

constexpr size_t kGuard = 64;

int zlib_verdict(const uint8_t *payload, uint32_t payload_len, uint32_t isize, uint32_t crc, std::vector<uint8_t> &out) {
    out.assign(isize ? isize : 1, 0);
    z_stream s;
    std::memset(&s, 0, sizeof(s));
    if (inflateInit2(&s, -15) != Z_OK) std::abort();
    s.next_in = const_cast<Bytef *>(payload);
    s.avail_in = payload_len;
    s.next_out = out.data();
    s.avail_out = isize;
    int ret;
    for (;;) {
        const uLong before_in = s.total_in, before_out = s.total_out;
        ret = inflate(&s, Z_NO_FLUSH);
        if (ret != Z_OK || (s.total_in == before_in && s.total_out == before_out)) break;
    }
    const uLong total_out = s.total_out;
    inflateEnd(&s);
    if (ret == Z_DATA_ERROR) return BV_INF_BAD_DEFLATE;
    if (ret != Z_STREAM_END || total_out != isize) return BV_INF_BAD_SIZE;
    if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), out.data(), isize) != crc) return BV_INF_BAD_CRC;
    return BV_INF_OK;
}

uint32_t le32(FILE *f) {
    uint8_t b[4];
    if (std::fread(b, 1, 4, f) != 4) {
        std::fprintf(stderr, "inflate_core_check: truncated corpus\n");
        std::exit(2);
    }
    return bv_inf_le32(b);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: inflate_core_check CORPUS\n");
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    static uint32_t crc_tab[1024];
    bv_inf_crc_tables(crc_tab, 0, 1);
    static BvInfTables T;
    const uint32_t n = le32(f);
    int bad = 0, category = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t mlen = le32(f);
        // the member in an allocation of exactly its size: a read beyond it is the sanitizer's to report
        std::vector<uint8_t> m(mlen);
        if (mlen && std::fread(m.data(), 1, mlen, f) != mlen) {
            std::fprintf(stderr, "inflate_core_check: truncated corpus\n");
            return 2;
        }
        BvBgzfMember h;
        int core = bv_bgzf_member_parse(m.data(), mlen, &h), judge = core;
        uint32_t mask = 0;
        if (core == BV_INF_OK && h.isize > BV_INF_MAX_ISIZE) core = judge = BV_INF_BAD_SIZE;  // no BGZF member is that large
        if (core == BV_INF_OK) {
            std::vector<uint8_t> payload(m.begin() + h.payload_off, m.begin() + h.payload_off + h.payload_len);  // exact size again
            std::vector<uint8_t> expect;
            judge = zlib_verdict(payload.data(), h.payload_len, h.isize, h.crc, expect);
            std::vector<uint8_t> out(kGuard + h.isize + kGuard, 0xA5);
            core = bv_inf_stream(payload.data(), h.payload_len, out.data() + kGuard, h.isize, &T, 0, 1);
            mask = T.block_mask;
            if (core == BV_INF_OK) {
                uint32_t c = 0;
                for (uint32_t s = 0; s < 64; ++s) c ^= bv_inf_crc_share(out.data() + kGuard, h.isize, s, crc_tab);
                if (~c != h.crc) core = BV_INF_BAD_CRC;
                if ((~c) != (uint32_t)crc32(crc32(0L, Z_NULL, 0), out.data() + kGuard, h.isize)) {
                    std::fprintf(stderr, "member %u: the sliced CRC32 %08x is not zlib's\n", k, ~c);
                    ++bad;
                }
            }
            for (size_t g = 0; g < kGuard; ++g)
                if (out[g] != 0xA5 || out[kGuard + h.isize + g] != 0xA5) {
                    std::fprintf(stderr, "member %u: guard byte %zu damaged\n", k, g);
                    ++bad;
                    break;
                }
            if (judge == BV_INF_OK && core == BV_INF_OK && std::memcmp(out.data() + kGuard, expect.data(), h.isize) != 0) {
                std::fprintf(stderr, "member %u: inflated bytes differ from zlib's\n", k);
                ++bad;
            }
        }
        if ((core == BV_INF_OK) != (judge == BV_INF_OK)) {
            std::fprintf(stderr, "member %u: core status %d, zlib's verdict %d\n", k, core, judge);
            ++bad;
        } else if (core != judge) {
            std::fprintf(stderr, "member %u: category differs: core %d, zlib %d\n", k, core, judge);
            ++category;
        }
        std::printf("%u %d %d %u %u\n", k, core, judge, mask, h.isize);
    }
    std::fclose(f);
    std::fprintf(stderr, "inflate_core_check: %u members, %d disagreements, %d named differently\n", n, bad, category);
    return bad ? 1 : 0;
}
