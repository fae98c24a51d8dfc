// file_major.hpp -- reference-format batchfiles read FILE-MAJOR, a window of positions at a time (bv_call --files-per-pass K).
//
// BatchfileProducer (batch_producer.hpp) keeps a reader open on every batchfile for the whole run and interleaves their lines
// position by position.  A cohort of thousands of batchfiles has more files than a process may hold descriptors, so here the
// files are taken in GROUPS of K: within a window of P positions, group after group is opened at the place the window before
// left each file, its next P lines are read (the files of a group on the caller's threads), and it is closed again.  At no time
// are more than K batchfiles open (max_open() counts them), the header scan included.
//
// Where a file stands is a cursor: in a BGZF file (what the reference writes) the file offset of a member and the inflated
// bytes in front of the line inside it -- members are independent, so reading on from there costs no more than that member --,
// in anything else zlib reads (plain gzip, plain text) the offset in the inflated stream, reached with gzseek (direct in plain
// text; a plain gzip stream is inflated again from its start: correct, slow, and not what a cohort is written as).
//
// A window: begin(want) reads group 0 and fixes P = min(want, the lines every file of group 0 still has); group(g) reads the
// same P lines of group g's files -- a file that has fewer shortens the window (used()) and the run ends there, as the default
// route ends at the shortest file; end() moves every cursor used() lines on.  reread(p) brings one position's line of every
// file again, from the window's first cursors, one file open at a time: for the rare position the host reader takes.
#pragma once

#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "batch_producer.hpp"  // GzLineReader, bgzf_member_header, parse_sample_ids

namespace bvamd {

// The header scan of scan_batchfile_headers, file by file: each opened, read through its '#' lines and closed.
struct FileMajorHeaders {
    std::vector<std::string> sample_ids;
    std::vector<uint32_t> file_samples;
    std::vector<size_t> header_lines;
};
inline void scan_batchfile_headers_closing(const std::vector<std::string> &paths, FileMajorHeaders &h) {
    h.file_samples.assign(paths.size(), 0);
    h.header_lines.assign(paths.size(), 0);
    for (size_t b = 0; b < paths.size(); ++b) {
        GzLineReader rd;
        if (!rd.open(paths[b])) throw std::runtime_error("[ERROR] " + paths[b] + " open failure.");
        std::string line;
        while (rd.getline(line)) {
            if (line.empty() || line[0] != '#') { h.header_lines[b] += line.empty() ? 1 : 0; break; }
            const size_t before = h.sample_ids.size();
            parse_sample_ids(line, h.sample_ids);
            h.file_samples[b] += (uint32_t)(h.sample_ids.size() - before);
            ++h.header_lines[b];
        }
    }
}

class FileMajorReader {
public:
    struct Cursor { uint64_t pos = 0, skip = 0; };
    // The rows of one group for a window, packed position-major as bv_text_rows wants them: row (p, k) is line p of file
    // first_file + k; a position a file has no line for holds "\n" (such positions lie behind used()).
    struct Group {
        std::string text;
        std::vector<uint64_t> row_off;  // [n_positions * n_files + 1]
        size_t first_file = 0, n_files = 0, n_positions = 0;
    };

    FileMajorReader(std::vector<std::string> paths, const std::vector<size_t> &header_lines, size_t files_per_pass, int threads)
        : paths_(std::move(paths)), K_(std::max<size_t>(1, files_per_pass)), threads_(std::max(1, threads)), cur_(paths_.size()), bgzf_(paths_.size(), 0) {
        for (size_t f = 0; f < paths_.size(); ++f) {  // behind the header lines, one file open at a time
            std::FILE *fp = open_file(f);
            unsigned char h[18];
            bgzf_[f] = std::fread(h, 1, 18, fp) == 18 && bgzf_member_header(h);
            close_file(fp);
            Lines L;
            read_lines(f, cur_[f], f < header_lines.size() ? header_lines[f] : 0, L);
            cur_[f] = cursor_after(f, cur_[f], L, L.end.size());
        }
    }
    size_t files() const { return paths_.size(); }
    size_t groups() const { return (paths_.size() + K_ - 1) / K_; }
    size_t max_open() const { return (size_t)max_open_.load(); }
    size_t passes() const { return passes_; }  // groups read so far
    size_t used() const { return used_; }      // positions of the window that every file read so far has a line for

    // A new window of at most `want` positions: group 0 into `g`; returns P (0: a file of group 0 is through, and so is the run)
    size_t begin(size_t want, Group &g) {
        start_ = cur_;
        read_.assign(paths_.size(), Lines());
        P_ = want;
        const size_t got = read_group(0, want);
        P_ = used_ = got;
        pack(0, g);
        return P_;
    }
    // group gi >= 1 of the window; returns used()
    size_t group(size_t gi, Group &g) {
        used_ = std::min(used_, read_group(gi, P_));
        pack(gi, g);
        return used_;
    }
    void end() {
        for (size_t f = 0; f < paths_.size(); ++f) cur_[f] = cursor_after(f, start_[f], read_[f], std::min(used_, read_[f].end.size()));
        read_.clear();
    }
    // position p's line of every file, without the line breaks (p < used()); reread_at: of the window that began at `start`
    // (window_start()), from any thread, while this reader is at a later window
    std::vector<Cursor> window_start() const { return start_; }
    std::vector<std::string> reread(size_t p) { return reread_at(start_, p); }
    std::vector<std::string> reread_at(const std::vector<Cursor> &start, size_t p) {
        std::lock_guard<std::mutex> lk(io_);
        std::vector<std::string> out(paths_.size());
        for (size_t f = 0; f < paths_.size(); ++f) {
            Lines L;
            read_lines(f, start[f], p + 1, L);
            if (L.end.size() <= p) throw std::runtime_error("[ERROR] " + paths_[f] + ": a row of the window cannot be read again");
            out[f] = L.line(p);
        }
        return out;
    }

private:
    // Lines read from a cursor: `text` begins at the cursor's member (BGZF) or at the cursor (else); line k is
    // text[k ? end[k - 1] : first, end[k]) with its '\n' (a last line without one has none)
    struct Lines {
        std::string text;
        std::vector<uint64_t> end;
        std::vector<std::pair<uint64_t, uint64_t>> member;  // BGZF: (file offset, offset in text) of every member read, and of the byte behind the last
        uint64_t first = 0;
        std::string line(size_t k) const {
            const uint64_t a = k ? end[k - 1] : first, b = end[k];
            return text.substr(a, b - a - (text[b - 1] == '\n' ? 1 : 0));
        }
    };

    std::FILE *open_file(size_t f) {
        std::FILE *fp = std::fopen(paths_[f].c_str(), "rb");
        if (!fp) throw std::runtime_error("[ERROR] " + paths_[f] + " open failure.");
        count_open();
        return fp;
    }
    void close_file(std::FILE *fp) { std::fclose(fp); --open_; }
    void count_open() {
        const int n = ++open_;
        int m = max_open_.load();
        while (n > m && !max_open_.compare_exchange_weak(m, n)) {}
    }

    // up to n complete lines of file f from cursor c (a last line without a line break counts, as GzLineReader counts it)
    void read_lines(size_t f, const Cursor &c, size_t n, Lines &L) {
        L = Lines();
        if (bgzf_[f]) read_bgzf(f, c, n, L);
        else read_stream(f, c, n, L);
    }
    static void cut(Lines &L, uint64_t &scan, size_t n) {
        while (L.end.size() < n && scan < L.text.size()) {
            const char *nl = (const char *)std::memchr(L.text.data() + scan, '\n', L.text.size() - scan);
            if (!nl) { scan = L.text.size(); break; }
            scan = (uint64_t)(nl - L.text.data()) + 1;
            L.end.push_back(scan);
        }
    }
    void read_bgzf(size_t f, const Cursor &c, size_t n, Lines &L) {
        std::FILE *fp = open_file(f);
        struct Close { FileMajorReader *r; std::FILE *fp; ~Close() { r->close_file(fp); } } closer{this, fp};
        if (fseeko(fp, (off_t)c.pos, SEEK_SET) != 0) throw std::runtime_error("[ERROR] cannot seek in " + paths_[f]);
        L.first = c.skip;
        uint64_t at = c.pos, scan = c.skip;
        z_stream zs;
        std::memset(&zs, 0, sizeof zs);
        if (inflateInit2(&zs, -15) != Z_OK) throw std::runtime_error("[ERROR] inflateInit2 failed");
        struct End { z_stream *z; ~End() { inflateEnd(z); } } ender{&zs};
        std::vector<unsigned char> raw;
        bool eof = false;
        while (L.end.size() < n) {
            unsigned char h[18];
            const size_t got = std::fread(h, 1, 18, fp);
            if (got == 0) { eof = true; break; }
            if (got != 18 || !bgzf_member_header(h)) throw std::runtime_error("[ERROR] not a BGZF member where one was expected (truncated or damaged batchfile)");
            const size_t total = ((size_t)h[16] | ((size_t)h[17] << 8)) + 1, xlen = (size_t)h[10] | ((size_t)h[11] << 8);
            if (total < 12 + xlen + 8) throw std::runtime_error("[ERROR] damaged BGZF member");
            raw.resize(total);
            std::memcpy(raw.data(), h, 18);
            if (std::fread(&raw[18], 1, total - 18, fp) != total - 18) throw std::runtime_error("[ERROR] truncated BGZF member");
            const unsigned char *t = &raw[total - 4];
            const uint32_t isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
            L.member.push_back({at, (uint64_t)L.text.size()});
            at += total;
            if (isize) {
                const size_t o = L.text.size();
                L.text.resize(o + isize);
                inflateReset(&zs);
                zs.next_in = &raw[12 + xlen];
                zs.avail_in = (uInt)(total - 12 - xlen - 8);
                zs.next_out = reinterpret_cast<Bytef *>(&L.text[o]);
                zs.avail_out = isize;
                if (inflate(&zs, Z_FINISH) != Z_STREAM_END || zs.avail_out != 0) throw std::runtime_error("[ERROR] a BGZF member does not inflate to its recorded size");
            }
            if (L.text.size() > scan) cut(L, scan, n);
        }
        if (eof && L.end.size() < n && L.text.size() > (L.end.empty() ? L.first : L.end.back())) L.end.push_back(L.text.size());
        L.member.push_back({at, (uint64_t)L.text.size()});
    }
    void read_stream(size_t f, const Cursor &c, size_t n, Lines &L) {
        gzFile g = gzopen(paths_[f].c_str(), "rb");
        if (!g) throw std::runtime_error("[ERROR] " + paths_[f] + " open failure.");
        count_open();
        struct Close { FileMajorReader *r; gzFile g; ~Close() { gzclose(g); --r->open_; } } closer{this, g};
        gzbuffer(g, 1 << 20);
        if (c.pos && gzseek(g, (z_off_t)c.pos, SEEK_SET) < 0) throw std::runtime_error("[ERROR] cannot seek in " + paths_[f]);
        uint64_t scan = 0;
        bool eof = false;
        while (L.end.size() < n && !eof) {
            const size_t o = L.text.size();
            L.text.resize(o + ((size_t)1 << 20));
            const int got = gzread(g, &L.text[o], 1u << 20);
            if (got < 0) throw std::runtime_error("[ERROR] damaged or truncated gzip input: " + paths_[f]);
            L.text.resize(o + (size_t)got);
            eof = got == 0;
            cut(L, scan, n);
        }
        if (eof && L.end.size() < n && L.text.size() > (L.end.empty() ? 0 : L.end.back())) L.end.push_back(L.text.size());
    }
    // the cursor behind the first k lines of L, which was read from c
    Cursor cursor_after(size_t f, const Cursor &c, const Lines &L, size_t k) const {
        const uint64_t x = k ? L.end[k - 1] : L.first;
        if (!bgzf_[f]) return Cursor{c.pos + x, 0};
        if (L.member.empty()) return c;
        size_t m = 0;
        while (m + 1 < L.member.size() && L.member[m + 1].second <= x) ++m;  // the last member that begins at or before x
        return Cursor{L.member[m].first, x - L.member[m].second};
    }

    // the lines of group gi's files (at most n each), on the threads; returns the fewest any file has
    size_t read_group(size_t gi, size_t n) {
        std::lock_guard<std::mutex> lk(io_);
        const size_t lo = gi * K_, hi = std::min(paths_.size(), lo + K_);
        std::atomic<size_t> next{lo};
        std::exception_ptr err;
        std::mutex err_mu;
        auto work = [&]() {
            for (size_t f; (f = next++) < hi;) {
                try { read_lines(f, start_[f], n, read_[f]); }
                catch (...) { std::lock_guard<std::mutex> g(err_mu); if (!err) err = std::current_exception(); }
            }
        };
        std::vector<std::thread> th;
        for (size_t t = 1; t < std::min<size_t>((size_t)threads_, hi - lo); ++t) th.emplace_back(work);
        work();
        for (auto &t : th) t.join();
        ++passes_;
        if (err) std::rethrow_exception(err);
        size_t got = n;
        for (size_t f = lo; f < hi; ++f) got = std::min(got, read_[f].end.size());
        return got;
    }
    void pack(size_t gi, Group &g) {
        const size_t lo = gi * K_, hi = std::min(paths_.size(), lo + K_), K = hi - lo;
        g.first_file = lo; g.n_files = K; g.n_positions = P_;
        g.row_off.resize(P_ * K + 1);
        uint64_t at = 0;
        for (size_t p = 0; p < P_; ++p)
            for (size_t k = 0; k < K; ++k) {
                const Lines &L = read_[lo + k];
                g.row_off[p * K + k] = at;
                if (p < L.end.size()) {
                    const uint64_t a = p ? L.end[p - 1] : L.first, b = L.end[p];
                    at += b - a + (L.text[b - 1] == '\n' ? 0 : 1);
                } else {
                    at += 1;
                }
            }
        g.row_off[P_ * K] = at;
        g.text.resize(at);
        for (size_t p = 0; p < P_; ++p)
            for (size_t k = 0; k < K; ++k) {
                const Lines &L = read_[lo + k];
                char *d = &g.text[g.row_off[p * K + k]];
                const size_t n = (size_t)(g.row_off[p * K + k + 1] - g.row_off[p * K + k]);
                if (p < L.end.size()) std::memcpy(d, L.text.data() + (p ? L.end[p - 1] : L.first), std::min<size_t>(n, L.end[p] - (p ? L.end[p - 1] : L.first)));
                d[n - 1] = '\n';
            }
        for (size_t f = lo; f < hi; ++f) std::string().swap(read_[f].text);  // (the cursors need `end` and `member` only)
    }

    std::vector<std::string> paths_;
    size_t K_;
    int threads_;
    std::vector<Cursor> cur_, start_;
    std::vector<char> bgzf_;
    std::vector<Lines> read_;
    size_t P_ = 0, used_ = 0, passes_ = 0;
    std::atomic<int> open_{0}, max_open_{0};
    std::mutex io_;
};

}  // namespace bvamd
