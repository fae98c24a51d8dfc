// raw_reads.hpp -- every sample's raw BAM records of one pileup window, undecoded, as bv_engine_pileup takes them
// (include/basevar_amd_pileup.h): what `bv_call --pileup device` and `bv_pileup --rows device` read before they hand a window to
// the engine.
#pragma once

#include <atomic>
#include <exception>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "pileup.hpp"

namespace bvamd {

struct WindowReads {
    std::vector<uint8_t> records;      // the runs back to back
    std::vector<uint64_t> run_off{0};  // [n_runs + 1]
    std::vector<uint32_t> run_sample;  // [n_runs], ascending: a sample without records has no run
    int tid = -1;                      // the contig's number in the BAM headers; -1: no run
};

// The records of the fetch of [wb - PILEUP_PAD, we + PILEUP_PAD] of every sample (BamFile::next_raw), read on `threads` threads
// that take the samples in turn; an exception on any thread is rethrown here once all have ended.  BAM files that number the
// contig differently cannot share one bv_pileup_reads.tid: refused.
inline void read_window_raw(BamPool &pool, const std::vector<std::string> &bams, const std::string &ref_id, uint32_t wb, uint32_t we, int threads,
                            WindowReads &out) {
    const size_t n = bams.size();
    const uint32_t lo = wb > PILEUP_PAD ? wb - PILEUP_PAD : 1, hi = we + PILEUP_PAD;
    std::vector<std::vector<uint8_t>> per(n);
    std::vector<int> tids(n, -1);
    std::atomic<size_t> next_sample(0);
    auto work = [&]() {
        for (size_t i; (i = next_sample.fetch_add(1)) < n;) {
            BamPool::Handle h = pool.get(i);
            tids[i] = h.bf->tid_of(ref_id);
            if (!h.bf->fetch(tids[i], (int64_t)lo - 1, (int64_t)hi)) continue;
            while (h.bf->next_raw(per[i]) >= 0) {}
        }
    };
    const size_t nt = (size_t)std::max(1, threads);
    std::vector<std::exception_ptr> errs(nt);
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; ++t)
        th.emplace_back([&, t]() { try { work(); } catch (...) { errs[t] = std::current_exception(); } });
    try { work(); } catch (...) { errs[0] = std::current_exception(); }
    for (auto &x : th) x.join();
    for (auto &e : errs) if (e) std::rethrow_exception(e);
    out = WindowReads();
    for (size_t i = 0; i < n; ++i) {
        if (tids[i] < 0 || per[i].empty()) continue;
        if (out.tid >= 0 && tids[i] != out.tid) throw std::runtime_error("[ERROR] --pileup device needs BAM files that number " + ref_id + " alike: " + bams[i]);
        out.tid = tids[i];
        out.records.insert(out.records.end(), per[i].begin(), per[i].end());
        out.run_off.push_back(out.records.size());
        out.run_sample.push_back((uint32_t)i);
    }
}

}  // namespace bvamd
