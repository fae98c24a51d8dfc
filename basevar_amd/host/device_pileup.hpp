// device_pileup.hpp -- one pileup window handed to the engine: what `bv_call --pileup device` and `bv_pileup --rows device` share
// between the window walk (for_each_pileup_window, pileup.hpp) and what each does with the piled-up planes.  The window comes as
// every sample's raw records (WindowReads, raw_reads.hpp -> bv_engine_pileup) or as the compressed BGZF members that hold them
// (WindowMembers, raw_members.hpp -> bv_engine_pileup_bgzf).  Declarations of the C ABI only: the entry points come in a table,
// filled with the linked symbols (bv_call) or with what dlsym returned (bv_pileup, which loads the library on demand).
#pragma once

#include <algorithm>
#include <stdexcept>

#include "../../include/basevar_amd_pileup_bgzf.h"
#include "raw_members.hpp"
#include "raw_reads.hpp"

namespace bvamd {

struct PileupEntryPoints {
    decltype(&bv_engine_pileup) pileup = nullptr;
    decltype(&bv_engine_pileup_bgzf) pileup_bgzf = nullptr;
    decltype(&bv_last_error) last_error = nullptr;  // what a failed call throws
};

// What every window of a region has in common, and the two ways in which the tools differ
struct PileupRegionCall {
    PileupEntryPoints entry;
    bv_engine *engine = nullptr;
    uint32_t n_samples = 0, region_beg = 0, region_end = 0;
    int mapq_thd = 0;
    bool skip_empty = false;  // bv_call: a window without any run has no site.  bv_pileup piles it up all the same: its rows are placeholders
    bool clamp_tid = false;   // bv_pileup: such a window has tid -1, handed over as 0
};

static_assert(sizeof(MemberRun) == sizeof(bv_pileup_bgzf_run), "one run layout");

inline bv_pileup_reads pileup_reads_of(const PileupRegionCall &c, const WindowReads &r, uint32_t wb, uint32_t we) {
    bv_pileup_reads in{};
    in.records = r.records.data(); in.run_off = r.run_off.data(); in.run_sample = r.run_sample.data();
    in.pitch = ((size_t)c.n_samples + 15) / 16 * 16; in.n_runs = (uint32_t)r.run_sample.size(); in.n_samples = c.n_samples;
    in.tid = c.clamp_tid ? std::max(r.tid, 0) : r.tid; in.region_beg = c.region_beg; in.region_end = c.region_end; in.beg = wb; in.end = we;
    in.mapq_thd = c.mapq_thd;
    in.mem_kind = BV_MEM_HOST;
    return in;
}

inline bv_pileup_bgzf pileup_bgzf_of(const PileupRegionCall &c, const WindowMembers &wm, uint32_t wb, uint32_t we) {
    bv_pileup_bgzf in{};
    in.members.data = wm.plan.data.data(); in.members.member_off = wm.plan.member_off.data(); in.members.data_bytes = wm.plan.data.size();
    in.members.n_members = (uint32_t)wm.plan.member_pos.size();
    in.runs = reinterpret_cast<const bv_pileup_bgzf_run *>(wm.plan.runs.data());
    in.pitch = ((size_t)c.n_samples + 15) / 16 * 16; in.n_runs = (uint32_t)wm.plan.runs.size(); in.n_samples = c.n_samples;
    in.tid = c.clamp_tid ? std::max(wm.tid, 0) : wm.tid; in.region_beg = c.region_beg; in.region_end = c.region_end; in.beg = wb; in.end = we;
    in.mapq_thd = c.mapq_thd;
    return in;
}

// Piles up window [wb, we]: *n_cov takes its covered positions.  false: the window has no run and skip_empty passes it by.
inline bool pileup_window_reads(const PileupRegionCall &c, const WindowReads &r, uint32_t wb, uint32_t we, uint32_t *n_cov) {
    if (c.skip_empty && r.run_sample.empty()) return false;
    const bv_pileup_reads in = pileup_reads_of(c, r, wb, we);
    if (c.entry.pileup(c.engine, &in, n_cov, nullptr) != BV_OK) throw std::runtime_error(c.entry.last_error(c.engine));
    return true;
}
inline bool pileup_window_members(const PileupRegionCall &c, const WindowMembers &wm, uint32_t wb, uint32_t we, uint32_t *n_cov) {
    if (c.skip_empty && wm.plan.runs.empty()) return false;
    const bv_pileup_bgzf in = pileup_bgzf_of(c, wm, wb, we);
    if (c.entry.pileup_bgzf(c.engine, &in, n_cov, nullptr) != BV_OK) throw std::runtime_error(c.entry.last_error(c.engine));
    return true;
}

}  // namespace bvamd
