// tabix_query.hpp -- a reader of tabix (.tbi) indexes with the one query a region call needs: where in the indexed file the
// lines of NAME:BEG-END may begin.
//
// The reference opens every batchfile's index and runs tbx_itr_querys(tbx, region) on it (src/basetype_caller.cpp:559-601).  No
// htslib here: the index's layout is the tabix paper's / bgzf_tabix.hpp's (this file reads what that one writes, and what htslib
// writes), and only the START of the iterator is taken from it -- the lines behind it are selected, and the region's end is
// found, where the inflated text lies (bv_engine_text_parse_bgzf_region, or the host reader).  So the query is:
//   * the bins that overlap [beg - 1, end) (0-based, half-open), the pseudo-bin 37450 left out;
//   * of their chunks, those whose END lies beyond the linear index's offset for window (beg - 1) >> 14 (htslib's rule: a
//     chunk that ends before the first line of that window cannot hold a line of the region);
//   * the smallest BEGIN among them.
// No such chunk: the file has no line there.  A name the index does not hold is for the caller to refuse.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bamio.hpp"  // BgzfReader: the index is itself a BGZF file

namespace bvamd {

class TabixReader {
public:
    struct Ref {
        std::vector<std::pair<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>>> bins;  // as they lie in the file
        std::vector<uint64_t> linear;
    };
    enum Hit { UNKNOWN_NAME, NOTHING, FOUND };

    // false: no file at `path`.  Throws on a file that is not a tabix index or ends early.
    bool load(const std::string &path) {
        std::FILE *probe = std::fopen(path.c_str(), "rb");
        if (!probe) return false;
        std::fclose(probe);
        path_ = path;
        BgzfReader bg(path);
        char magic[4];
        if (!bg.read(magic, 4) || std::memcmp(magic, "TBI\1", 4) != 0) throw std::runtime_error("[ERROR] not a tabix index: " + path);
        const uint32_t n_ref = count(bg);
        for (int i = 0; i < 6; ++i) conf_[i] = (int32_t)rd32(bg);
        const uint32_t l_nm = count(bg);
        std::string nm(l_nm, '\0');
        if (l_nm && !bg.read(&nm[0], l_nm)) truncated();
        names_.clear();
        for (size_t at = 0; at < nm.size();) {
            const size_t z = nm.find('\0', at);
            if (z == std::string::npos) throw std::runtime_error("[ERROR] damaged tabix index (names): " + path);
            names_.push_back(nm.substr(at, z - at));
            at = z + 1;
        }
        if (names_.size() != n_ref) throw std::runtime_error("[ERROR] damaged tabix index (names): " + path);
        refs_.assign(n_ref, Ref());
        for (Ref &r : refs_) {
            r.bins.resize(count(bg));
            for (auto &b : r.bins) {
                b.first = rd32(bg);
                b.second.resize(count(bg));
                for (auto &c : b.second) { c.first = rd64(bg); c.second = rd64(bg); }
            }
            r.linear.resize(count(bg));
            for (uint64_t &o : r.linear) o = rd64(bg);
        }
        return true;
    }
    const std::vector<std::string> &names() const { return names_; }
    const std::vector<Ref> &refs() const { return refs_; }
    const int32_t *conf() const { return conf_; }

    // Where the lines of name:beg-end (1-based, inclusive, 1 <= beg <= end) may begin: *voff is a virtual offset at or before
    // the first of them.  NOTHING: *has_window says whether the linear index has an entry to fall back on, and *voff is then its
    // offset for the region's first window -- a line at or behind which no line of the region lies in front (for a caller that
    // reads this file beside others whose indexes found something).
    Hit query(const std::string &name, int64_t beg, int64_t end, uint64_t *voff, bool *has_window = nullptr) const {
        size_t tid = 0;
        while (tid < names_.size() && names_[tid] != name) ++tid;
        if (tid == names_.size()) return UNKNOWN_NAME;
        const Ref &r = refs_[tid];
        int64_t b0 = beg - 1, e0 = std::min<int64_t>(end, (int64_t)1 << 29);  // [b0, e0)
        if (b0 < 0) b0 = 0;
        if (has_window) *has_window = false;
        if (b0 >= e0) return NOTHING;
        uint64_t min_off = 0;
        if (!r.linear.empty()) min_off = r.linear[std::min<size_t>((size_t)(b0 >> 14), r.linear.size() - 1)];
        const int64_t last = e0 - 1;
        bool any = false;
        uint64_t best = 0;
        for (const auto &bin : r.bins) {
            if (bin.first == 37450u || !overlaps(bin.first, b0, last)) continue;
            for (const auto &c : bin.second)
                if (c.second > min_off && (!any || c.first < best)) { any = true; best = c.first; }
        }
        if (!any) {
            if (has_window) *has_window = !r.linear.empty();
            *voff = min_off;
            return NOTHING;
        }
        *voff = best;
        return FOUND;
    }

private:
    // is `bin` one of the bins that may hold a line of [b0, last] (both 0-based, inclusive)?
    static bool overlaps(uint32_t bin, int64_t b0, int64_t last) {
        static const int shift[6] = {29, 26, 23, 20, 17, 14};
        static const uint32_t first[6] = {0, 1, 9, 73, 585, 4681};
        for (int l = 0; l < 6; ++l) {
            const uint32_t lo = first[l] + (uint32_t)(b0 >> shift[l]), hi = first[l] + (uint32_t)(last >> shift[l]);
            if (bin >= lo && bin <= hi) return true;
        }
        return false;
    }
    [[noreturn]] void truncated() const { throw std::runtime_error("[ERROR] truncated tabix index: " + path_); }
    uint32_t rd32(BgzfReader &bg) const {
        uint8_t b[4];
        if (!bg.read(b, 4)) truncated();
        return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    }
    uint64_t rd64(BgzfReader &bg) const {
        const uint64_t lo = rd32(bg), hi = rd32(bg);
        return lo | (hi << 32);
    }
    // a count of items that follow: at least 8 bytes each would have to be there, and no index of a 2^29-base contig comes near 2^24 of them
    uint32_t count(BgzfReader &bg) const {
        const uint32_t n = rd32(bg);
        if (n > (1u << 24)) throw std::runtime_error("[ERROR] damaged tabix index (a count of " + std::to_string(n) + "): " + path_);
        return n;
    }
    std::string path_;
    int32_t conf_[6] = {0, 0, 0, 0, 0, 0};
    std::vector<std::string> names_;
    std::vector<Ref> refs_;
};

}  // namespace bvamd
