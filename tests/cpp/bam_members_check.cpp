// bam_members_check.cpp -- CPU harness (a program of its own, built with ASan + UBSan) for basevar_amd/host/raw_members.hpp, the
// host planner behind bv_engine_pileup_bgzf: a fetch as whole compressed BGZF members plus cut points, nothing inflated.
//
//   bam_members_check plan <out> <fasta> <ref_id> <region_beg> <region_end> <beg> <end> <mapq_thd> <a.bam> ...
//       1. plans every file's fetch of the window -/+ 200 bases with read_window_members and inflates the planned members with zlib,
//          back to back as bv_engine_bgzf_inflate lays them out;
//       2. cuts the runs out of that text, each into a buffer of exactly its size;
//       3. requires that every run is a chain of whole records that ends exactly at the run's end (bv_pileup_record until
//          next_at == bytes);
//       4. requires that bv_pileup_core.h's pileup over these runs gives the planes, depths and tokens of the core over
//          BamFile::next_raw's bytes of the same fetch, byte for byte (exit 3 if not).  The run bytes themselves are not compared:
//          next_raw may read one record past a chunk that ends on a member boundary, which the core's filter makes harmless.
//       <out> receives the core's result and the next_raw runs in pileup_core_check's format, <out>.members the plan: "PMEM",
//       u32 n_members, u32 n_runs, i32 tid, u32 0, u64 data bytes, u64 member_off[n_members + 1], the runs (24 bytes each, the
//       layout of bv_pileup_bgzf_run), the members' bytes.  One line of counts says what the plan holds:
//       "plan members <n> runs <n> begin_gt0 <n> end_lt_isize <n> chunk_end_low0 <n> straddle <n> span3 <n> multi_run <n> shared <n>
//        no_run <n> isize0 <n>" -- runs with begin > 0, runs that end below their last member's ISIZE, chunk ends with a zero low
//       half, records across a member boundary, records across three or more members, samples of several runs, runs that share
//       their first member with the run before, samples without a run, members of ISIZE 0 inside a run.
#include <zlib.h>

#define main pileup_core_check_main  // its Runs, Result, run_core and dump; not its command line
#include "pileup_core_check.cpp"
#undef main

#include "../../basevar_amd/host/raw_members.hpp"
#include "../../basevar_amd/host/raw_reads.hpp"

namespace {

bool inflate_member(const uint8_t *m, size_t len, uint8_t *dst, uint32_t isize) {
    if (isize == 0) return true;
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<uint8_t *>(m) + 18; zs.avail_in = (uInt)(len - 18 - 8);
    zs.next_out = dst; zs.avail_out = isize;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == isize;
    inflateEnd(&zs);
    return ok;
}

bool same(const Result &a, const Result &b, const char **what) {
    *what = "status"; if (a.status != b.status) return false;
    *what = "cell plane"; if (a.cell != b.cell) return false;
    *what = "qual plane"; if (a.qual != b.qual) return false;
    *what = "mapq plane"; if (a.mapq != b.mapq) return false;
    *what = "rank plane"; if (a.rank != b.rank) return false;
    *what = "depth"; if (a.depth != b.depth || a.n_covered != b.n_covered) return false;
    *what = "tokens"; if (a.tokens.size() != b.tokens.size() || a.text != b.text) return false;
    return a.tokens.empty() || std::memcmp(a.tokens.data(), b.tokens.data(), a.tokens.size() * sizeof(BvPileupToken)) == 0;
}

}  // namespace

// bam_members_check time <runs out> <members out> <ref_id> <beg> <end> <threads> <a.bam> ...   (tools/pileup_bgzf_bench.py)
// three passes over the window with the readers kept open, seconds each: read_window_raw (the host reads and inflates) and
// read_window_members (the host only reads); the runs go to <runs out> in pileup_core_check's `raw` format, the plan to
// <members out> in the format above
static int time_reads(int argc, char **argv) {
    const std::string ref_id = argv[4];
    const uint32_t beg = (uint32_t)std::strtoul(argv[5], nullptr, 10), end = (uint32_t)std::strtoul(argv[6], nullptr, 10);
    const int threads = std::atoi(argv[7]);
    std::vector<std::string> bams(argv + 8, argv + argc);
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    BamPool pool(bams, true);
    WindowReads wr;
    WindowMembers wm;
    for (int rep = 0; rep < 3; ++rep) {
        const double t0 = now();
        read_window_raw(pool, bams, ref_id, beg, end, threads, wr);
        std::printf("host threads %d pass %d: raw records read %.6f s, %zu bytes\n", threads, rep, now() - t0, wr.records.size());
    }
    for (int rep = 0; rep < 3; ++rep) {
        const double t0 = now();
        read_window_members(pool, bams, ref_id, beg, end, threads, wm);
        std::printf("host threads %d pass %d: members read %.6f s, %zu members, %zu bytes, %zu runs\n", threads, rep, now() - t0, wm.plan.member_pos.size(),
                    wm.plan.data.size(), wm.plan.runs.size());
    }
    std::ofstream f(argv[2], std::ios::binary);
    put(f, (uint32_t)wr.run_sample.size()); put(f, (uint32_t)bams.size()); put(f, wr.run_off); put(f, wr.run_sample); put(f, wr.records);
    std::ofstream g(argv[3], std::ios::binary);
    g.write("PMEM", 4);
    put(g, (uint32_t)wm.plan.member_pos.size()); put(g, (uint32_t)wm.plan.runs.size()); put(g, (int32_t)wm.tid); put(g, (uint32_t)0); put(g, (uint64_t)wm.plan.data.size());
    put(g, wm.plan.member_off); put(g, wm.plan.runs); put(g, wm.plan.data);
    std::printf("tid %d\n", wr.tid);
    return f && g ? 0 : 2;
}

static int run(int argc, char **argv) {
    if (argc >= 9 && std::strcmp(argv[1], "time") == 0) return time_reads(argc, argv);
    if (argc < 11 || std::strcmp(argv[1], "plan") != 0) {
        std::fprintf(stderr, "usage: bam_members_check plan <out> <fasta> <ref_id> <region_beg> <region_end> <beg> <end> <mapq_thd> <a.bam> ...\n");
        return 2;
    }
    const std::string out_path = argv[2], fasta = argv[3], ref_id = argv[4];
    const uint32_t region_beg = (uint32_t)std::strtoul(argv[5], nullptr, 10), region_end = (uint32_t)std::strtoul(argv[6], nullptr, 10);
    const uint32_t beg = (uint32_t)std::strtoul(argv[7], nullptr, 10), end = (uint32_t)std::strtoul(argv[8], nullptr, 10);
    const int mapq_thd = std::atoi(argv[9]);
    std::vector<std::string> bams(argv + 10, argv + argc);
    const std::string fa = load_fasta_sequence(fasta, ref_id);
    const uint32_t lo = beg > PILEUP_PAD ? beg - PILEUP_PAD : 1, hi = end + PILEUP_PAD;
    // the parent's way in: next_raw's records of the same fetches, a run a sample
    BamPool pool(bams, true);
    WindowReads wr;
    read_window_raw(pool, bams, ref_id, beg, end, 2, wr);
    Runs R;
    R.n_samples = (uint32_t)bams.size();
    R.tid = wr.tid < 0 ? 0 : wr.tid;
    R.records = wr.records; R.run_off = wr.run_off; R.run_sample = wr.run_sample;
    const Result want = run_core(R, fa, region_beg, region_end, beg, end, mapq_thd);
    // the plan
    WindowMembers W;
    read_window_members(pool, bams, ref_id, beg, end, 2, W);
    const MemberPlan &P = W.plan;
    const size_t n_mem = P.member_pos.size();
    if (wr.tid >= 0 && W.tid >= 0 && wr.tid != W.tid) return differ("tid");
    std::vector<uint64_t> dst_off(n_mem + 1, 0);
    for (size_t k = 0; k < n_mem; ++k) dst_off[k + 1] = dst_off[k] + P.isize(k);
    std::vector<uint8_t> text(dst_off[n_mem]);
    for (size_t k = 0; k < n_mem; ++k)
        if (!inflate_member(&P.data[P.member_off[k]], P.member_off[k + 1] - P.member_off[k], text.data() + dst_off[k], P.isize(k))) return differ("a planned member does not inflate");
    Runs C;
    C.n_samples = R.n_samples; C.tid = R.tid;
    unsigned long long begin_gt0 = 0, end_lt = 0, straddle = 0, span3 = 0, multi = 0, shared = 0, no_run = 0, isize0 = 0, low0 = 0;
    std::vector<uint32_t> runs_of(bams.size(), 0);
    for (size_t r = 0; r < P.runs.size(); ++r) {
        const MemberRun &u = P.runs[r];
        const uint32_t last = u.first_member + u.n_members - 1;
        if (u.n_members == 0 || last >= n_mem || u.begin > P.isize(u.first_member) || u.end > P.isize(last) || u.sample >= bams.size() || u.reserved_ ||
            (r && u.sample < P.runs[r - 1].sample))
            return differ("a run the engine would refuse");
        const uint64_t a = dst_off[u.first_member] + u.begin, b = dst_off[last] + u.end;
        if (b < a) return differ("a run that ends before it begins");
        const std::vector<uint8_t> run(text.begin() + (std::ptrdiff_t)a, text.begin() + (std::ptrdiff_t)b);  // exactly its size: the sanitizer sees a read beyond it
        for (uint64_t at = 0; at < run.size();) {
            BvPileupRec rec;
            const uint32_t st = bv_pileup_record(run.data(), run.size(), at, &rec);
            if (st != BV_PILEUP_OK) {
                std::printf("run %zu of sample %u, byte %llu of %zu: %s\n", r, u.sample, (unsigned long long)at, run.size(), bv_pileup_status_text(st));
                return differ("a run is no chain of whole records");
            }
            uint32_t touched = 0;  // members with text that the record lies in
            for (uint32_t k = u.first_member; k <= last; ++k)
                touched += dst_off[k + 1] > dst_off[k] && a + at < dst_off[k + 1] && a + rec.next_at > dst_off[k];
            straddle += touched >= 2; span3 += touched >= 3;
            at = rec.next_at;
        }
        begin_gt0 += u.begin > 0; end_lt += u.end < P.isize(last);
        for (uint32_t k = u.first_member; k <= last; ++k) isize0 += P.isize(k) == 0;
        shared += r && P.runs[r - 1].sample == u.sample && P.runs[r - 1].first_member + P.runs[r - 1].n_members - 1 == u.first_member;
        ++runs_of[u.sample];
        C.records.insert(C.records.end(), run.begin(), run.end());
        C.run_off.push_back(C.records.size());
        C.run_sample.push_back(u.sample);
    }
    for (size_t s = 0; s < bams.size(); ++s) {
        multi += runs_of[s] >= 2; no_run += runs_of[s] == 0;
        BamPool::Handle h = pool.get(s);
        if (h.bf->has_index())
            for (const auto &c : h.bf->index().query(h.bf->tid_of(ref_id), (int64_t)lo - 1, (int64_t)hi)) low0 += c.first < c.second && (c.second & 0xffffu) == 0;
    }
    const Result got = run_core(C, fa, region_beg, region_end, beg, end, mapq_thd);
    const char *what = "";
    if (!same(want, got, &what)) { report(want); report(got); return differ(what); }
    dump(out_path, want, R);
    {
        std::ofstream f(out_path + ".members", std::ios::binary);
        f.write("PMEM", 4);
        put(f, (uint32_t)n_mem); put(f, (uint32_t)P.runs.size()); put(f, (int32_t)W.tid); put(f, (uint32_t)0); put(f, (uint64_t)P.data.size());
        put(f, P.member_off);
        static_assert(sizeof(MemberRun) == 24, "a run is 24 bytes");
        put(f, P.runs); put(f, P.data);
        if (!f) { std::fprintf(stderr, "bam_members_check: cannot write %s.members\n", out_path.c_str()); return 2; }
    }
    report(want);
    std::printf("plan members %zu runs %zu begin_gt0 %llu end_lt_isize %llu chunk_end_low0 %llu straddle %llu span3 %llu multi_run %llu shared %llu no_run %llu isize0 %llu\n",
                n_mem, P.runs.size(), begin_gt0, end_lt, low0, straddle, span3, multi, shared, no_run, isize0);
    return 0;
}

int main(int argc, char **argv) {
    try {
        return run(argc, argv);
    } catch (const std::exception &ex) {  // what the planner refuses about a file
        std::fprintf(stderr, "bam_members_check: %s\n", ex.what());
        return 4;
    }
}
