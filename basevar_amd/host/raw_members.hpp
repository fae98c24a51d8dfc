// raw_members.hpp -- every sample's BAM records of one pileup window as the COMPRESSED BGZF members that hold them plus the
// cut points, as bv_engine_pileup_bgzf takes them (include/basevar_amd_pileup_bgzf.h): the members-and-cut-points counterpart of
// BamFile::fetch + next_raw (host/raw_reads.hpp).  Nothing is inflated here: a host thread seeks, walks the members' BSIZE
// fields and reads their bytes.
//
// One RUN per merged BAI chunk (vb, ve) of the fetch: its first member lies at file offset vb >> 16 and the first record
// begins vb & 0xffff inflated bytes into it; if ve & 0xffff is not 0 the last member lies at ve >> 16 and ve & 0xffff of its bytes
// belong to the run, otherwise the last member is the one that ends at ve >> 16 and all its ISIZE bytes belong to it.  A file
// without an index has one run, from its first record to the last member before the end of the file.  A member that two
// chunks of one fetch share (they meet inside it) is read and handed over once: the second run starts at the first one's last.
#pragma once

#include <atomic>
#include <cstdio>
#include <exception>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "pileup.hpp"

namespace bvamd {

// bv_pileup_bgzf_run, field for field (the tools assert the size against the C header)
struct MemberRun {
    uint32_t sample, first_member, n_members, begin, end, reserved_;
};

// The members of one file's fetch, or of a whole window (WindowMembers): member k is data[member_off[k] .. member_off[k + 1])
struct MemberPlan {
    std::vector<uint8_t> data;
    std::vector<uint64_t> member_off{0};  // [members + 1]
    std::vector<uint64_t> member_pos;     // [members]: where each lies in its file
    std::vector<MemberRun> runs;
    void clear() { data.clear(); member_off.assign(1, 0); member_pos.clear(); runs.clear(); }
    uint32_t isize(size_t k) const {
        const uint8_t *t = &data[member_off[k + 1] - 4];
        return (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    }
};

// The one packing the device inflater takes (SAM specification 4.1 as every common writer lays it out): a gzip member whose
// extra field is the 6 bytes of the 'BC' subfield and nothing else
inline bool bam_member_header_ok(const uint8_t *h) {
    return h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C' && h[14] == 2 && h[15] == 0;
}

// Can this file's members go to the device as they lie?  Decided by its first member; a later one of another packing is an
// error of the read (member_read).
inline bool bam_members_supported(const std::string &path) {
    std::FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t h[18];
    const bool ok = std::fread(h, 1, 18, f) == 18 && bam_member_header_ok(h);
    std::fclose(f);
    return ok;
}

// The whole member at the file's current position, file offset `at`, appended to `p`: its bytes, 0 at the end of the file
inline size_t member_read(std::FILE *fp, const std::string &path, uint64_t at, MemberPlan &p) {
    uint8_t h[18];
    const size_t n = std::fread(h, 1, 18, fp);
    if (n == 0) return 0;
    if (n != 18 || !bam_member_header_ok(h))
        throw std::runtime_error("[ERROR] " + path + ": at offset " + std::to_string(at) + " lies no BGZF member of the XLEN = 6 packing (damaged file, or a member the device cannot take)");
    const size_t total = ((size_t)h[16] | ((size_t)h[17] << 8)) + 1;
    if (total < 26) throw std::runtime_error("[ERROR] " + path + ": damaged BGZF member at offset " + std::to_string(at));
    const size_t o = p.data.size();
    p.data.resize(o + total);
    std::memcpy(&p.data[o], h, 18);
    if (std::fread(&p.data[o + 18], 1, total - 18, fp) != total - 18) throw std::runtime_error("[ERROR] " + path + ": truncated BGZF member at offset " + std::to_string(at));
    p.member_off.push_back(p.data.size());
    p.member_pos.push_back(at);
    return total;
}

// The fetch of [beg, end) (0-based, as BamFile::fetch takes it) of `tid` as members and runs; run.sample is left 0.  False, and
// an empty plan, if the reference is not in this file.  Throws on a file that ends inside a member, on a member of another
// packing and on a chunk whose ends lie on no member (an index of another file).
inline bool plan_members(BamFile &bf, int tid, int64_t beg, int64_t end, MemberPlan &out) {
    out.clear();
    if (tid < 0 || (size_t)tid >= bf.refs().size()) return false;
    std::vector<std::pair<uint64_t, uint64_t>> chunks;
    const bool indexed = bf.has_index();
    if (indexed) chunks = bf.index().query(tid, beg, end);
    else chunks.push_back({bf.first_record(), ~0ull});
    std::FILE *fp = bf.raw_file();
    const std::string &path = bf.path();
    for (const auto &c : chunks) {
        const uint64_t vb = c.first, ve = c.second;
        if (vb >= ve) continue;  // an empty chunk
        const bool at_last = indexed && (ve & 0xffffu) != 0;  // the last member LIES at ve >> 16; else it ENDS there
        const uint64_t stop = indexed ? ve >> 16 : ~0ull;
        uint64_t at = vb >> 16;
        MemberRun run{0, (uint32_t)out.member_pos.size(), 0, (uint32_t)(vb & 0xffffu), 0, 0};
        bool seek = true;
        if (!out.member_pos.empty() && out.member_pos.back() == at) {  // the chunk before ended inside this member: share it
            run.first_member = (uint32_t)out.member_pos.size() - 1u;
            run.n_members = 1;
            if (at_last && at == stop) at = ~0ull;  // ... and this one ends inside it too
            else at += out.member_off[run.first_member + 1] - out.member_off[run.first_member];
        }
        while (at != ~0ull && (at_last || at < stop)) {
            if (at_last && at > stop) throw std::runtime_error("[ERROR] " + path + ": a chunk of its index ends at offset " + std::to_string(stop) + ", where no BGZF member begins");
            if (seek && std::fseek(fp, (long)at, SEEK_SET) != 0) throw std::runtime_error("[ERROR] seek failed in " + path);
            seek = false;
            const size_t total = member_read(fp, path, at, out);
            if (total == 0) {
                if (at_last) throw std::runtime_error("[ERROR] " + path + ": a chunk of its index ends behind the end of the file");
                break;
            }
            ++run.n_members;
            if (at_last && at == stop) break;
            at += total;
        }
        if (run.n_members == 0) continue;
        const uint32_t first_isize = out.isize(run.first_member), last_isize = out.isize(run.first_member + run.n_members - 1u);
        run.end = at_last ? (uint32_t)(ve & 0xffffu) : last_isize;
        if (run.begin > first_isize || run.end > last_isize || (run.n_members == 1 && run.begin > run.end))
            throw std::runtime_error("[ERROR] " + path + ": a chunk of its index points behind the text of its BGZF member");
        out.runs.push_back(run);
    }
    return true;
}

struct WindowMembers {
    MemberPlan plan;  // every sample's members, sample 0's first; the runs with their samples, ascending
    int tid = -1;     // the contig's number in the BAM headers; -1: no run
};

// The members of the fetch of [wb - PILEUP_PAD, we + PILEUP_PAD] of every sample (plan_members), read on `threads` threads
// that take the samples in turn; an exception on any thread is rethrown here once all have ended.  BAM files that number the
// contig differently cannot share one bv_pileup_bgzf.tid: refused, as read_window_raw refuses them.
inline void read_window_members(BamPool &pool, const std::vector<std::string> &bams, const std::string &ref_id, uint32_t wb, uint32_t we, int threads,
                                WindowMembers &out) {
    const size_t n = bams.size();
    const uint32_t lo = wb > PILEUP_PAD ? wb - PILEUP_PAD : 1, hi = we + PILEUP_PAD;
    std::vector<MemberPlan> per(n);
    std::vector<int> tids(n, -1);
    std::atomic<size_t> next_sample(0);
    auto work = [&]() {
        for (size_t i; (i = next_sample.fetch_add(1)) < n;) {
            BamPool::Handle h = pool.get(i);
            tids[i] = h.bf->tid_of(ref_id);
            plan_members(*h.bf, tids[i], (int64_t)lo - 1, (int64_t)hi, per[i]);
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
    out.plan.clear();
    out.tid = -1;
    size_t bytes = 0, members = 0;
    for (size_t i = 0; i < n; ++i) { bytes += per[i].data.size(); members += per[i].member_pos.size(); }
    out.plan.data.reserve(bytes);
    out.plan.member_off.reserve(members + 1);
    MemberPlan &w = out.plan;
    for (size_t i = 0; i < n; ++i) {
        if (tids[i] < 0 || per[i].runs.empty()) continue;
        if (out.tid >= 0 && tids[i] != out.tid) throw std::runtime_error("[ERROR] --pileup device needs BAM files that number " + ref_id + " alike: " + bams[i]);
        out.tid = tids[i];
        const uint32_t base = (uint32_t)w.member_pos.size();
        const uint64_t at = w.data.size();
        w.data.insert(w.data.end(), per[i].data.begin(), per[i].data.end());
        for (size_t k = 0; k < per[i].member_pos.size(); ++k) {
            w.member_off.push_back(at + per[i].member_off[k + 1]);
            w.member_pos.push_back(per[i].member_pos[k]);
        }
        for (MemberRun r : per[i].runs) {
            r.sample = (uint32_t)i;
            r.first_member += base;
            w.runs.push_back(r);
        }
    }
}

}  // namespace bvamd
