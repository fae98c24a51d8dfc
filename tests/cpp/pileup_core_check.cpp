// pileup_core_check.cpp -- CPU harness (a program of its own, built with ASan + UBSan) for basevar_amd/csrc/bv_pileup_core.h,
// the definition of the device pileup (bv_pileup.hip compiles its record decode, filter and helpers, and restates its walk).
//
//   pileup_core_check bam <out> <fasta> <ref_id> <region_beg> <region_end> <beg> <end> <mapq_thd> <split> <a.bam> ...
//       reads the BAM files twice: through BamFile::next + pileup_tile (the host code as it is), and through BamFile::next_raw
//       runs + the core (split = 1: a run per record, else a run per sample).  The four planes, the depths and the tokens must be
//       equal byte for byte (exit 3 if not); the core's result and the runs are dumped to <out>.
//   pileup_core_check raw <out> <ref bytes file> <tid> <region_beg> <region_end> <beg> <end> <mapq_thd> <runs file>
//       the core alone over runs given as bytes (u32 n_runs, u32 n_samples, u64 run_off[n_runs + 1], u32 run_sample[n_runs], the
//       records): damaged input, which the host code is never shown.
//   pileup_core_check time ...   (tools/pileup_bench.py: seconds of the host pileup and of the raw read; see main)
// The first two print "status <BV_PILEUP_*> sample <s> run <r> at <offset>: <text>" and exit 0 when the core ended in a status or a
// clean result.  <out>, little endian: "PLUP", u32 status, fail sample, fail run, u64 fail at; u32 rows, n_samples, u64 pitch,
// u32 n_tokens, n_covered, u64 text_bytes, i32 tid, u32 n_runs, u64 record bytes; then (status 0 only) cell, qual, mapq
// [rows][pitch], rank u16 [rows][pitch], depth u32 [rows], the tokens sorted by (pos, sample) (24 bytes each), their text; then
// run_off, run_sample, the records.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <numeric>
#include <string>
#include <vector>

#include "../../basevar_amd/csrc/bv_pileup_core.h"
#include "../../basevar_amd/host/pileup.hpp"

using namespace bvamd;

namespace {

struct Runs {
    std::vector<uint8_t> records;
    std::vector<uint64_t> run_off{0};
    std::vector<uint32_t> run_sample;
    uint32_t n_samples = 0;
    int32_t tid = 0;
};

struct Result {
    uint32_t status = 0, fail_sample = 0, fail_run = 0;
    uint64_t fail_at = 0;
    uint32_t rows = 0, n_samples = 0, n_covered = 0;
    uint64_t pitch = 0;
    std::vector<uint8_t> cell, qual, mapq;
    std::vector<uint16_t> rank;
    std::vector<uint32_t> depth;
    std::vector<BvPileupToken> tokens;
    std::vector<uint8_t> text;
};

// The core over every sample: a counting pass, the tokens' places by a running sum in sample order, a writing pass
Result run_core(const Runs &R, const std::string &ref, uint32_t region_beg, uint32_t region_end, uint32_t beg, uint32_t end, int mapq_thd) {
    Result out;
    uint32_t gb = 0, ge = 0;
    if (!bv_pileup_step(region_beg, region_end, beg, end, &gb, &ge)) {
        std::fprintf(stderr, "pileup_core_check: [%u, %u] is no window of the step grid from %u\n", beg, end, region_beg);
        std::exit(2);
    }
    BvPileupQuery q;
    bv_pileup_query(R.tid, beg, end, gb, ge, mapq_thd, ref.size(), &q);
    const uint32_t n = R.n_samples, n_runs = (uint32_t)R.run_sample.size();
    out.rows = end - beg + 1; out.n_samples = n; out.pitch = ((uint64_t)n + 255) / 256 * 256;
    const size_t cells = (size_t)out.rows * out.pitch;
    std::vector<uint32_t> samp_run(n + 1, 0);
    for (uint32_t r = 0; r < n_runs; ++r) samp_run[R.run_sample[r] + 1] = r + 1;
    for (uint32_t s = 0; s < n; ++s) samp_run[s + 1] = std::max(samp_run[s + 1], samp_run[s]);
    std::vector<uint32_t> seen((out.rows + 31) / 32);
    std::vector<BvPileupSample> per(n);
    // a copy of the records of exactly their size, and of the reference: the sanitizer then sees every byte read beyond them
    std::vector<uint8_t> rec(R.records.begin(), R.records.end()), fa(ref.begin(), ref.end());
    for (int pass = 0; pass < 2; ++pass) {
        out.cell.assign(cells, BV_PU_CELL_N); out.qual.assign(cells, 0); out.mapq.assign(cells, 0); out.rank.assign(cells, 0);
        BvPileupSink k;
        k.cell = out.cell.data(); k.qual = out.qual.data(); k.mapq = out.mapq.data(); k.rank = out.rank.data(); k.pitch = out.pitch;
        k.seen = seen.data();
        k.tokens = pass ? out.tokens.data() : nullptr; k.text = out.text.data();
        k.text_at = 0; k.token_at = 0;
        for (uint32_t s = 0; s < n; ++s) {
            std::fill(seen.begin(), seen.end(), 0u);
            const uint32_t st = bv_pileup_sample(&q, rec.data(), 0, R.run_off.data(), samp_run[s], samp_run[s + 1], fa.data(), s, &k, &per[s]);
            if (st != BV_PILEUP_OK) {
                out.status = st; out.fail_sample = s; out.fail_run = per[s].run; out.fail_at = per[s].at;
                return out;
            }
        }
        if (pass == 0) {
            out.tokens.assign(k.token_at, BvPileupToken());
            out.text.assign(k.text_at, 0);
        }
    }
    out.depth.assign(out.rows, 0);
    for (uint32_t r = 0; r < out.rows; ++r) {
        for (uint64_t c = 0; c < out.pitch; ++c) out.depth[r] += out.rank[(size_t)r * out.pitch + c] != 0;
        out.n_covered += out.depth[r] != 0;
    }
    std::stable_sort(out.tokens.begin(), out.tokens.end(), [](const BvPileupToken &a, const BvPileupToken &b) {
        return a.pos != b.pos ? a.pos < b.pos : a.sample < b.sample;
    });
    return out;
}

template <class T>
void put(std::ofstream &f, const T &v) { f.write(reinterpret_cast<const char *>(&v), sizeof v); }
template <class T>
void put(std::ofstream &f, const std::vector<T> &v) { if (!v.empty()) f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(T))); }

void dump(const std::string &path, const Result &o, const Runs &R) {
    std::ofstream f(path, std::ios::binary);
    f.write("PLUP", 4);
    put(f, o.status); put(f, o.fail_sample); put(f, o.fail_run); put(f, o.fail_at);
    put(f, o.rows); put(f, o.n_samples); put(f, o.pitch);
    put(f, (uint32_t)o.tokens.size()); put(f, o.n_covered); put(f, (uint64_t)o.text.size());
    put(f, R.tid); put(f, (uint32_t)R.run_sample.size()); put(f, (uint64_t)R.records.size());
    if (o.status == BV_PILEUP_OK) {
        put(f, o.cell); put(f, o.qual); put(f, o.mapq); put(f, o.rank); put(f, o.depth);
        static_assert(sizeof(BvPileupToken) == 24, "a token descriptor is 24 bytes");
        put(f, o.tokens); put(f, o.text);
    }
    put(f, R.run_off); put(f, R.run_sample); put(f, R.records);
    if (!f) { std::fprintf(stderr, "pileup_core_check: cannot write %s\n", path.c_str()); std::exit(2); }
}

void report(const Result &o) {
    std::printf("status %u sample %u run %u at %llu: %s\n", o.status, o.fail_sample, o.fail_run, (unsigned long long)o.fail_at, bv_pileup_status_text(o.status));
}

int differ(const char *what) {
    std::printf("DIFFER: %s\n", what);
    return 3;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 12 && std::strcmp(argv[1], "bam") == 0) {
        const std::string out_path = argv[2], fasta = argv[3], ref_id = argv[4];
        const uint32_t region_beg = (uint32_t)std::strtoul(argv[5], nullptr, 10), region_end = (uint32_t)std::strtoul(argv[6], nullptr, 10);
        const uint32_t beg = (uint32_t)std::strtoul(argv[7], nullptr, 10), end = (uint32_t)std::strtoul(argv[8], nullptr, 10);
        const int mapq_thd = std::atoi(argv[9]);
        const bool split = std::atoi(argv[10]) != 0;
        std::vector<std::string> bams(argv + 11, argv + argc);
        const std::string fa = load_fasta_sequence(fasta, ref_id);
        // the raw way in: every sample's records of the fetch, undecoded
        Runs R;
        R.n_samples = (uint32_t)bams.size();
        R.tid = -1;
        const uint32_t lo = beg > PILEUP_PAD ? beg - PILEUP_PAD : 1, hi = end + PILEUP_PAD;
        for (size_t s = 0; s < bams.size(); ++s) {
            BamFile bf(bams[s]);
            const int tid = bf.tid_of(ref_id);
            if (tid < 0) continue;
            if (R.tid >= 0 && tid != R.tid) { std::fprintf(stderr, "pileup_core_check: %s numbers %s differently\n", bams[s].c_str(), ref_id.c_str()); return 2; }
            R.tid = tid;
            if (!bf.fetch(tid, (int64_t)lo - 1, (int64_t)hi)) continue;
            size_t before = R.records.size();
            while (bf.next_raw(R.records) >= 0) {
                if (split) { R.run_off.push_back(R.records.size()); R.run_sample.push_back((uint32_t)s); before = R.records.size(); }
            }
            if (!split && R.records.size() != before) { R.run_off.push_back(R.records.size()); R.run_sample.push_back((uint32_t)s); }
        }
        if (R.tid < 0) R.tid = 0;
        const Result o = run_core(R, fa, region_beg, region_end, beg, end, mapq_thd);
        // the host's way
        BamPool pool(bams, true);
        PileupTile t;
        std::string host_err;
        try {
            pileup_tile(pool, fa, ref_id, region_beg, region_end, beg, end, mapq_thd, 1, t);
        } catch (const std::exception &ex) {
            host_err = ex.what();
        }
        if (!host_err.empty()) {
            std::printf("host: %s\n", host_err.c_str());
            if (o.status != BV_PILEUP_BAD_BASE || host_err != bv_pileup_status_text(BV_PILEUP_BAD_BASE)) return differ("the host threw, the core did not say the same");
        } else {
            if (o.status != BV_PILEUP_OK) { report(o); return differ("the core refused what the host piled up"); }
            if (t.pitch != o.pitch || t.rows() != o.rows) return differ("shape");
            if (t.cell != o.cell) return differ("cell plane");
            if (t.qual != o.qual) return differ("qual plane");
            if (t.mapq != o.mapq) return differ("mapq plane");
            if (t.rank != o.rank) return differ("rank plane");
            if (t.depth != o.depth) return differ("depth");
            if (t.indels.size() != o.tokens.size()) return differ("token count");
            for (size_t i = 0; i < t.indels.size(); ++i) {
                const BvPileupToken &k = o.tokens[i];
                if (k.pos != t.indels[i].pos || k.sample != t.indels[i].sample || k.text_len != t.indels[i].text.size() ||
                    std::memcmp(o.text.data() + k.text_off, t.indels[i].text.data(), k.text_len) != 0)
                    return differ("token");
            }
        }
        dump(out_path, o, R);
        report(o);
        return 0;
    }
    if (argc == 11 && std::strcmp(argv[1], "raw") == 0) {
        auto slurp = [](const char *p) {
            std::ifstream f(p, std::ios::binary);
            if (!f) { std::fprintf(stderr, "pileup_core_check: cannot read %s\n", p); std::exit(2); }
            return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        };
        const std::string fa = slurp(argv[3]), raw = slurp(argv[10]);
        Runs R;
        R.tid = std::atoi(argv[4]);
        uint32_t n_runs = 0;
        if (raw.size() < 8) return 2;
        std::memcpy(&n_runs, raw.data(), 4);
        std::memcpy(&R.n_samples, raw.data() + 4, 4);
        const size_t head = 8 + 8ull * (n_runs + 1) + 4ull * n_runs;
        if (raw.size() < head) return 2;
        R.run_off.resize(n_runs + 1);
        R.run_sample.resize(n_runs);
        std::memcpy(R.run_off.data(), raw.data() + 8, 8ull * (n_runs + 1));
        if (n_runs) std::memcpy(R.run_sample.data(), raw.data() + 8 + 8ull * (n_runs + 1), 4ull * n_runs);
        R.records.assign(raw.begin() + (std::ptrdiff_t)head, raw.end());
        // what bv_engine_pileup checks on the host before any launch
        if (R.run_off[0] != 0 || R.run_off[n_runs] != R.records.size()) return 2;
        for (uint32_t r = 0; r < n_runs; ++r)
            if (R.run_off[r + 1] < R.run_off[r] || R.run_sample[r] >= R.n_samples || (r && R.run_sample[r] < R.run_sample[r - 1])) return 2;
        const Result o = run_core(R, fa, (uint32_t)std::strtoul(argv[5], nullptr, 10), (uint32_t)std::strtoul(argv[6], nullptr, 10),
                                  (uint32_t)std::strtoul(argv[7], nullptr, 10), (uint32_t)std::strtoul(argv[8], nullptr, 10), std::atoi(argv[9]));
        dump(argv[2], o, R);
        report(o);
        return 0;
    }
    if (argc >= 12 && std::strcmp(argv[1], "time") == 0) {
        // pileup_core_check time <runs out> <fasta> <ref_id> <region_beg> <region_end> <beg> <end> <mapq_thd> <threads> <a.bam> ...
        // (tools/pileup_bench.py) three passes over the window with the readers kept open, seconds each: the host pileup on
        // <threads> threads + the copy of the covered rows into a slab, and the raw read of the same fetches; the runs go to
        // <runs out> in the `raw` mode's format
        const std::string fa = load_fasta_sequence(argv[3], argv[4]), ref_id = argv[4];
        const uint32_t region_beg = (uint32_t)std::strtoul(argv[5], nullptr, 10), region_end = (uint32_t)std::strtoul(argv[6], nullptr, 10);
        const uint32_t beg = (uint32_t)std::strtoul(argv[7], nullptr, 10), end = (uint32_t)std::strtoul(argv[8], nullptr, 10);
        const int mapq_thd = std::atoi(argv[9]), threads = std::atoi(argv[10]);
        std::vector<std::string> bams(argv + 11, argv + argc);
        auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
        BamPool pool(bams, true);
        PileupTile t;
        for (int rep = 0; rep < 3; ++rep) {
            const double t0 = now();
            pileup_tile(pool, fa, ref_id, region_beg, region_end, beg, end, mapq_thd, threads, t);
            const double t1 = now();
            std::vector<uint8_t> cell, qual, mapq;
            std::vector<uint16_t> rank;
            size_t covered = 0;
            for (size_t r = 0; r < t.rows(); ++r) {
                if (!t.depth[r]) continue;
                ++covered;
                cell.insert(cell.end(), &t.cell[r * t.pitch], &t.cell[(r + 1) * t.pitch]);
                qual.insert(qual.end(), &t.qual[r * t.pitch], &t.qual[(r + 1) * t.pitch]);
                mapq.insert(mapq.end(), &t.mapq[r * t.pitch], &t.mapq[(r + 1) * t.pitch]);
                rank.insert(rank.end(), &t.rank[r * t.pitch], &t.rank[(r + 1) * t.pitch]);
            }
            const double t2 = now();
            std::printf("host threads %d pass %d: pileup_tile %.6f s, rows packed %.6f s, covered %zu, pitch %zu, tokens %zu\n", threads, rep, t1 - t0, t2 - t1,
                        covered, t.pitch, t.indels.size());
        }
        const uint32_t lo = beg > PILEUP_PAD ? beg - PILEUP_PAD : 1, hi = end + PILEUP_PAD;
        Runs R;
        for (int rep = 0; rep < 3; ++rep) {
            R = Runs();
            R.n_samples = (uint32_t)bams.size();
            std::vector<std::vector<uint8_t>> per(bams.size());
            const double t0 = now();
            std::vector<std::thread> th;
            std::atomic<size_t> next(0);
            for (int w = 0; w < std::max(1, threads); ++w)
                th.emplace_back([&] {
                    for (size_t s; (s = next.fetch_add(1)) < bams.size();) {
                        BamPool::Handle h = pool.get(s);
                        if (!h.bf->fetch(h.bf->tid_of(ref_id), (int64_t)lo - 1, (int64_t)hi)) continue;
                        while (h.bf->next_raw(per[s]) >= 0) {}
                    }
                });
            for (auto &x : th) x.join();
            for (size_t s = 0; s < bams.size(); ++s) {
                if (per[s].empty()) continue;
                R.records.insert(R.records.end(), per[s].begin(), per[s].end());
                R.run_off.push_back(R.records.size());
                R.run_sample.push_back((uint32_t)s);
            }
            std::printf("host threads %d pass %d: raw records read %.6f s, %zu bytes\n", threads, rep, now() - t0, R.records.size());
        }
        R.tid = BamFile(bams[0]).tid_of(ref_id);
        std::ofstream f(argv[2], std::ios::binary);
        put(f, (uint32_t)R.run_sample.size()); put(f, R.n_samples); put(f, R.run_off); put(f, R.run_sample); put(f, R.records);
        std::printf("tid %d\n", R.tid);
        return 0;
    }
    std::fprintf(stderr, "usage: pileup_core_check bam|raw|time ... (see the head of tests/cpp/pileup_core_check.cpp)\n");
    return 2;
}
