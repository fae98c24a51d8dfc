// call_pipeline_check.cpp -- the stages of bv_call below the whole tool, WITHOUT an engine (basevar_amd/host/call_pipeline.hpp,
// pileup.hpp, bgzf_tabix.hpp): the hand-off queue, the emitter's ordering rules, the pileup window walk, region parsing and the
// BGZF block table.
//   call_pipeline_check WORKDIR
// The records are made up from the rows themselves, the way host_fuzz.cpp makes them.  What the emitter writes into plain-text
// outputs is held to a single-threaded format_cvg_line / format_vcf_line loop over the batches in seq order.  Ends with
// "CALL_PIPELINE cases N FAILS 0" (exit 0) or lists what failed (exit 1).  tests/test_call_pipeline_cpu.py builds it plain, with
// ASan + UBSan and with TSan, and runs each as a program.
#include <atomic>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../basevar_amd/host/call_pipeline.hpp"

using namespace bvamd;

static int g_cases = 0, g_fails = 0;
#define CHECK(cond, what)                                                                  \
    do {                                                                                   \
        ++g_cases;                                                                         \
        if (!(cond)) { ++g_fails; std::cout << "FAIL line " << __LINE__ << ": " << what << std::endl; } \
    } while (0)

static const size_t N = 7;  // samples

static CallContext make_ctx(int threads) {
    CallContext ctx;
    for (size_t i = 0; i < N; ++i) ctx.sample_ids.push_back("s" + std::to_string(i));
    ctx.group_names = {"g1"};
    ctx.group_id.assign(N, 0);
    ctx.devices = {0};
    ctx.threads = threads;
    ctx.batch_sites = 64;
    return ctx;
}

// One site of batch `seq`: cells, phreds and a record made up from them
struct Site {
    uint8_t cell[N], phred[N], mapq[N];
    uint16_t rank[N];
    uint8_t ref;
    SiteText text;
    bv_site_result r;
    bv_group_result g;
};
static Site make_site(uint64_t seq, uint32_t k, uint32_t pos) {
    Site s{};
    uint32_t x = (uint32_t)(seq * 2654435761u + k * 40503u + 12345u);
    for (size_t i = 0; i < N; ++i) {
        x = x * 1664525u + 1013904223u;
        s.cell[i] = (uint8_t)((x >> 24) % 9);  // 0..7: base + strand, 8: no call
        if (s.cell[i] == 8) s.cell[i] = BV_CELL_N;
        s.phred[i] = (uint8_t)((x >> 16) % 41);
        s.mapq[i] = (uint8_t)((x >> 8) % 60);
        s.rank[i] = (uint16_t)(1 + x % 100);
    }
    s.ref = (uint8_t)(pos & 3);
    s.text.ref_id = "chrT"; s.text.ref_pos = pos; s.text.ref_base = std::string(1, "ACGT"[s.ref]);
    if (k % 3 == 1) s.text.indel_tokens = {"+AC", "-T"};
    bv_site_result &r = s.r;
    for (size_t i = 0; i < N; ++i)
        if (s.cell[i] < 8) { r.depth[s.cell[i] & 3] += 1; r.total_depth += 1; r.cvg_sb[(s.cell[i] >> 2) & 1] += 1; }
    r.status = r.total_depth ? BV_SITE_COVERED : 0;
    for (int b = 0; b < 4; ++b)
        if (b != s.ref && r.depth[b] && r.n_alt < BV_MAX_ALT) {
            r.alt[r.n_alt] = (uint8_t)b;
            r.af[r.n_alt] = (double)r.depth[b] / r.total_depth;
            r.caf[r.n_alt] = 0.25 * r.depth[b];
            ++r.n_alt;
        }
    if (r.n_alt && k % 4 != 3) r.status |= BV_SITE_VARIANT | BV_SITE_RANKSUM;
    r.qual = 100.0 + k; r.qd = 1.5; r.cvg_fs = 0.25; r.cvg_sor = 1.0; r.var_fs = 2.0; r.var_sor = 0.5;
    r.mq_ranksum = 1.25; r.rpr_ranksum = -2.5; r.bq_ranksum = 0.0;
    s.g.n_alt = r.n_alt; s.g.total_depth = r.total_depth;
    for (int a = 0; a < r.n_alt; ++a) { s.g.alt[a] = r.alt[a]; s.g.af[a] = 0.5; }
    return s;
}

// Batch `seq` with `n_sites` sites, as a slab batch or a text batch; its lines go to cvg / vcf when they are given
static BatchPtr make_batch(uint64_t seq, uint32_t n_sites, bool from_text, std::string *cvg, std::string *vcf, size_t *n_variant) {
    static const std::vector<std::string> groups = {"g1"};
    BatchPtr b(new Batch((uint32_t)N));
    b->seq = seq;
    b->from_text = from_text;
    b->result.n_groups = 1;
    for (uint32_t k = 0; k < n_sites; ++k) {
        const Site s = make_site(seq, k, (uint32_t)(1000 * seq + 10 * k + 1));
        if (from_text) {
            b->cell.insert(b->cell.end(), s.cell, s.cell + N);
            b->phred.insert(b->phred.end(), s.phred, s.phred + N);
        } else {
            b->slab.add_row(s.cell, s.phred, s.mapq, s.rank, s.ref);
        }
        b->text.push_back(s.text);
        b->result.sites.push_back(s.r);
        b->result.groups.push_back(s.g);
        if (cvg) *cvg += format_cvg_line(s.text, s.r);
        if (vcf && (s.r.status & BV_SITE_VARIANT)) {
            *vcf += format_vcf_line(s.text, s.cell, s.phred, N, s.r, &s.g, groups);
            if (n_variant) ++*n_variant;
        }
    }
    return b;
}

static std::string slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// The batches (sizes, kinds, errors by seq) through an emitter in the order `order`; returns what the two files hold
struct EmitRun {
    std::string cvg, vcf, error;
    size_t n_sites = 0, n_variants = 0;
};
static EmitRun emit(const std::string &dir, int threads, const std::vector<uint32_t> &sizes, const std::vector<bool> &from_text,
                    const std::vector<std::string> &errors_of, const std::vector<size_t> &order, const char *late_error = nullptr) {
    const CallContext ctx = make_ctx(threads);
    TextOut vcf, cvg;
    vcf.open(dir + "/out.vcf");
    cvg.open(dir + "/out.cvg");
    StageClock clk;
    ErrorSink errors;
    {
        OrderedEmitter em(ctx, vcf, cvg, clk, errors);
        for (size_t i : order) {
            BatchPtr b = make_batch(i, sizes[i], from_text[i], nullptr, nullptr, nullptr);
            b->error = errors_of[i];
            em.accept(std::move(b));
        }
        em.finish();
        if (late_error) errors.fail(late_error);
        EmitRun r;
        r.cvg = slurp(dir + "/out.cvg"); r.vcf = slurp(dir + "/out.vcf"); r.error = errors.first();
        r.n_sites = em.n_sites(); r.n_variants = em.n_variants();
        return r;
    }
}
// ... and what a single-threaded loop over batches [0, upto) in seq order writes
static EmitRun expected(const std::vector<uint32_t> &sizes, const std::vector<bool> &from_text, size_t upto) {
    EmitRun r;
    for (size_t i = 0; i < upto; ++i) {
        make_batch(i, sizes[i], from_text[i], &r.cvg, &r.vcf, &r.n_variants);
        r.n_sites += sizes[i];
    }
    return r;
}

static void check_queue() {
    const int P = 4, C = 3, per = 50;
    BatchQueue q(2);
    std::vector<std::atomic<int>> seen(P * per);
    for (auto &s : seen) s = 0;
    std::atomic<int> nulls(0);
    std::vector<std::thread> prod, cons;
    for (int c = 0; c < C; ++c)
        cons.emplace_back([&q, &seen, &nulls]() {
            for (BatchPtr b; (b = q.pop());) seen[(size_t)b->seq] += 1;
            nulls += 1;  // (pop() returned null: closed and drained)
        });
    for (int p = 0; p < P; ++p)
        prod.emplace_back([&q, p]() {
            for (int k = 0; k < per; ++k) {
                BatchPtr b(new Batch(1));
                b->seq = (uint64_t)(p * per + k);
                q.push(std::move(b));
            }
        });
    for (auto &t : prod) t.join();
    q.close();
    for (auto &t : cons) t.join();
    bool once = true;
    for (auto &s : seen) once = once && s == 1;
    CHECK(once, "BatchQueue: every batch delivered exactly once");
    CHECK(nulls == C, "BatchQueue: close() lets every consumer drain and return");
    CHECK(q.pop() == nullptr, "BatchQueue: a closed, empty queue gives null");
}

static void check_emitter(const std::string &dir) {
    // out of order: six batches of 1 to 5 sites, one empty, slab and text batches mixed
    const std::vector<uint32_t> sizes = {3, 1, 0, 5, 2, 4};
    const std::vector<bool> kinds = {false, true, true, false, true, false};
    const std::vector<std::string> none(6);
    const std::vector<std::vector<size_t>> orders = {{5, 4, 3, 2, 1, 0}, {2, 0, 5, 1, 4, 3}, {1, 3, 0, 2, 5, 4}};
    const EmitRun want = expected(sizes, kinds, 6);
    CHECK(!want.vcf.empty() && want.n_variants > 2 && want.n_variants < want.n_sites, "the made-up records have variant and other sites");
    for (int threads : {1, 3, 8})
        for (const auto &order : orders) {
            const EmitRun got = emit(dir, threads, sizes, kinds, none, order);
            CHECK(got.cvg == want.cvg, "out of order: the CVG bytes, threads " << threads);
            CHECK(got.vcf == want.vcf, "out of order: the VCF bytes, threads " << threads);
            CHECK(got.n_sites == want.n_sites && got.n_variants == want.n_variants && got.error.empty(), "out of order: counts, no error");
        }
    // a failed slab batch: batch 2 of 5 -- batches 0-1 are written, nothing of 2-4; a later error does not replace its message
    {
        const std::vector<uint32_t> sz = {2, 3, 4, 1, 2};
        const std::vector<bool> kd = {false, true, false, false, true};
        const std::vector<std::string> er = {"", "", "slab batch 2 failed", "", "batch 4 failed too"};
        const EmitRun w = expected(sz, kd, 2);
        for (const auto &order : std::vector<std::vector<size_t>>{{0, 1, 2, 3, 4}, {4, 3, 2, 1, 0}, {2, 4, 0, 3, 1}}) {
            const EmitRun got = emit(dir, 3, sz, kd, er, order, "a later error");
            CHECK(got.cvg == w.cvg && got.vcf == w.vcf, "failed slab batch: batches 0-1 and nothing else");
            CHECK(got.error == "slab batch 2 failed", "failed slab batch: the sink holds its message, got '" << got.error << "'");
            CHECK(got.n_sites == w.n_sites, "failed slab batch: sites counted");
        }
    }
    // a failed text batch: batch 2 has three records and an error -- its records are written, nothing behind it
    {
        const std::vector<uint32_t> sz = {2, 3, 3, 1, 2};
        const std::vector<bool> kd = {false, true, true, false, true};
        const std::vector<std::string> er = {"", "", "text batch 2: a position was refused", "", ""};
        const EmitRun w = expected(sz, kd, 3);
        for (const auto &order : std::vector<std::vector<size_t>>{{0, 1, 2, 3, 4}, {4, 3, 2, 1, 0}, {3, 2, 4, 1, 0}}) {
            const EmitRun got = emit(dir, 3, sz, kd, er, order, "a later error");
            CHECK(got.cvg == w.cvg && got.vcf == w.vcf, "failed text batch: batches 0-2 and nothing else");
            CHECK(got.error == "text batch 2: a position was refused", "failed text batch: the sink holds its message, got '" << got.error << "'");
            CHECK(got.n_sites == w.n_sites && got.n_variants == w.n_variants, "failed text batch: counts");
        }
    }
}

// The walk against a position-by-position enumeration: position p lies in step (p - beg) / PILEUP_STEP, counted from the
// region's first position, and in window ((p - beg) % PILEUP_STEP) / window of that step
static void check_walk(uint32_t beg, uint32_t end, uint32_t window, const char *what) {
    std::vector<std::pair<uint32_t, uint32_t>> naive, got;
    uint64_t cur_step = ~0ull, cur_win = ~0ull;
    for (uint64_t p = beg; p <= end; ++p) {
        const uint64_t step = (p - beg) / PILEUP_STEP, win = ((p - beg) % PILEUP_STEP) / window;
        if (step != cur_step || win != cur_win) { naive.emplace_back((uint32_t)p, (uint32_t)p); cur_step = step; cur_win = win; }
        naive.back().second = (uint32_t)p;
    }
    const size_t limit = naive.size() + 8;  // (a walk that does not end is cut off here)
    for_each_pileup_window(beg, end, window, [&](uint32_t wb, uint32_t we) {
        got.emplace_back(wb, we);
        return got.size() < limit;
    });
    CHECK(got == naive, "window walk, " << what << ": " << got.size() << " windows against " << naive.size());
    bool tiles = !got.empty() && got.front().first == beg && got.back().second == end, inside = true;
    for (size_t i = 0; i < got.size(); ++i) {
        const uint64_t wb = got[i].first, we = got[i].second;
        inside = inside && wb <= we && we - wb + 1 <= window && (wb - beg) / PILEUP_STEP == (we - beg) / PILEUP_STEP;
        if (i) tiles = tiles && wb == (uint64_t)got[i - 1].second + 1;
    }
    CHECK(tiles, "window walk, " << what << ": the windows tile the region without gap or overlap");
    CHECK(inside, "window walk, " << what << ": every window lies inside one step of the grid laid out from the region's first position");
    // stopping early: fn's false ends the walk
    size_t calls = 0;
    for_each_pileup_window(beg, end, window, [&](uint32_t, uint32_t) { ++calls; return false; });
    CHECK(calls == 1, "window walk, " << what << ": false stops it");
}

static void check_regions() {
    Region r;
    CHECK(parse_region("chrI:5-9", r) && r.ref_id == "chrI" && r.beg == 5 && r.end == 9, "chrI:5-9");
    CHECK(parse_region("HLA:A*01:3-8", r) && r.ref_id == "HLA:A*01" && r.beg == 3 && r.end == 8, "HLA:A*01:3-8: a name with colons");
    CHECK(!parse_region("chr1", r), "chr1 is refused");
    CHECK(!parse_region("chr1:9", r), "chr1:9 is refused");
    CHECK(!parse_region("chr1:9-", r), "chr1:9- is refused");
    CHECK(!parse_region("nonsense", r) && !parse_region("", r) && !parse_region("chr1:-9", r) && !parse_region("a-b:3", r), "other refusals");
}

static void check_block_table() {
    const uint64_t B = BgzfWriter::kBlock;
    CHECK(B == 0xff00, "kBlock");
    CHECK(bgzf_block_table(0) == std::vector<uint64_t>({0}), "block table, 0 bytes: no block");
    CHECK(bgzf_block_table(1) == std::vector<uint64_t>({0, 1}), "block table, 1 byte");
    CHECK(bgzf_block_table(B - 1) == std::vector<uint64_t>({0, B - 1}), "block table, 0xff00 - 1");
    CHECK(bgzf_block_table(B) == std::vector<uint64_t>({0, B}), "block table, 0xff00");
    CHECK(bgzf_block_table(B + 1) == std::vector<uint64_t>({0, B, B + 1}), "block table, 0xff00 + 1");
    CHECK(bgzf_block_table(3 * B) == std::vector<uint64_t>({0, B, 2 * B, 3 * B}), "block table, 3 x 0xff00");
    CHECK(ends_in_gz("a.vcf.gz") && !ends_in_gz("a.vcf") && !ends_in_gz(".gz") && !ends_in_gz("gz"), "ends_in_gz");
}

int main(int argc, char **argv) {
    if (argc < 2) { std::cerr << "usage: call_pipeline_check WORKDIR" << std::endl; return 2; }
    try {
        check_queue();
        check_emitter(argv[1]);
        check_walk(7, 7, 100, "a region of one position");
        check_walk(1, PILEUP_STEP + 1, 1u << 17, "a region ending one position past a step edge");
        check_walk(10, 10 + 2 * PILEUP_STEP + 5, PILEUP_STEP + 123, "a window wider than a step");
        check_walk(PILEUP_STEP - 300, PILEUP_STEP + 300, 1, "a window of 1");
        check_walk(UINT32_MAX - 1200000, UINT32_MAX, 65536, "a region ending at 4,294,967,295");
        check_regions();
        check_block_table();
    } catch (const std::exception &ex) {
        std::cout << "FAIL: " << ex.what() << std::endl;
        ++g_fails;
    }
    std::printf("CALL_PIPELINE cases %d FAILS %d\n", g_cases, g_fails);
    return g_fails ? 1 : 0;
}
