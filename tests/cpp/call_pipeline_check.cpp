// call_pipeline_check.cpp -- the stages of bv_call below the whole tool, WITHOUT an engine (basevar_amd/host/call_pipeline.hpp,
// pileup.hpp, bgzf_tabix.hpp, indel_tokens.hpp, device_emit.hpp): the hand-off queue, the emitter's ordering rules, the pileup
// window walk, region parsing, the BGZF block table, the host's lists of indel tokens (TokenList) and the plan step of
// --emit device (plan_record_lines, with csrc/bv_record_text_core.h's bv_rt_on_device as the predicate).
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

#include "../../basevar_amd/csrc/bv_record_text_core.h"
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

typedef std::vector<std::string> Strs;

static TokenList make_list(const std::vector<std::pair<uint32_t, std::string>> &toks) {
    TokenList l;
    for (const auto &t : toks) {
        l.tokens.push_back(bv_pileup_token{t.first, 0u, l.text.size(), (uint32_t)t.second.size(), 0u});
        l.text.insert(l.text.end(), t.second.begin(), t.second.end());
    }
    return l;
}
// the dealing walk over `keys` from `cursor` on: what every key's SiteText took
static std::vector<Strs> dealt(const TokenList &l, const std::vector<uint32_t> &keys, size_t &cursor) {
    std::vector<SiteText> st(keys.size());
    l.deal(keys.data(), keys.size(), st.data(), cursor);
    std::vector<Strs> out;
    for (const SiteText &s : st) out.push_back(s.indel_tokens);
    return out;
}

static void check_token_list() {
    {
        const TokenList none;
        size_t cur = 0;
        CHECK(dealt(none, {1, 2}, cur) == std::vector<Strs>({{}, {}}) && cur == 0, "TokenList, empty: nothing is dealt");
        CHECK(none.of(1).empty() && none.bytes() == 0, "TokenList, empty: of() and bytes()");
        const bv_indel_tokens t = none.as_indel_tokens();
        CHECK(t.n_tokens == 0 && t.text_bytes == 0 && t.mem_kind == BV_MEM_HOST && t.reserved_ == 0, "TokenList, empty: as_indel_tokens");
    }
    // positions 2 .. 11, eight tokens, three of them at 5
    const TokenList l = make_list({{2, "+A"}, {3, "-C"}, {5, "+GG"}, {5, "-T"}, {5, "+GG"}, {7, "+AC"}, {9, "-TT"}, {11, "+N"}});
    size_t cur = 0;
    CHECK(dealt(l, {4, 5, 6, 7}, cur) == std::vector<Strs>({{}, {"+GG", "-T", "+GG"}, {}, {"+AC"}}),
          "TokenList: tokens below the first key are passed over, a key without a token takes none, three tokens at one key");
    CHECK(cur == 6, "TokenList: the cursor stands behind the last key's tokens, got " << cur);
    CHECK(dealt(l, {8, 9, 10}, cur) == std::vector<Strs>({{}, {"-TT"}, {}}) && cur == 7, "TokenList: the next range of keys goes on with the same cursor");
    CHECK(dealt(l, {11, 12}, cur) == std::vector<Strs>({{"+N"}, {}}) && cur == 8, "TokenList: the last token, and a key behind the list's end");
    CHECK(dealt(l, {13}, cur) == std::vector<Strs>({{}}) && cur == 8, "TokenList: a walk from the list's end");
    cur = 0;
    CHECK(dealt(l, {2, 3}, cur) == std::vector<Strs>({{"+A"}, {"-C"}}) && cur == 2, "TokenList: tokens beyond the last key are left where they are");
    CHECK(l.of(2) == Strs({"+A"}) && l.of(11) == Strs({"+N"}) && l.of(6).empty() && l.of(1).empty() && l.of(12).empty(), "TokenList: of() on the first, the last and absent positions");
    CHECK(l.of(5) == Strs({"+GG", "-T", "+GG"}) && l.view(2) == "+GG" && l.view(7) == "+N", "TokenList: of() keeps the list's order; view()");
    CHECK(l.bytes() == 24 * 8 + 20, "TokenList: bytes() is descriptors and text, got " << l.bytes());
    const bv_indel_tokens t = l.as_indel_tokens();
    CHECK(t.tokens == l.tokens.data() && t.text == l.text.data() && t.n_tokens == 8 && t.text_bytes == 20 && t.mem_kind == BV_MEM_HOST && t.reserved_ == 0, "TokenList: as_indel_tokens");
    // from_site_texts: rows without tokens between rows with them
    const std::vector<Strs> rows = {{"+AC", "-T"}, {}, {}, {"+G"}, {}, {"-TTT", "+A", "+A"}, {}};
    std::vector<SiteText> texts(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) texts[i].indel_tokens = rows[i];
    const uint32_t want_pos[6] = {0, 0, 3, 5, 5, 5}, want_len[6] = {3, 2, 2, 4, 2, 2};
    const uint64_t want_off[6] = {0, 3, 5, 7, 11, 13};
    for (int threads : {1, 4, 16}) {
        const TokenList none = TokenList::from_site_texts(std::vector<SiteText>(), threads);
        CHECK(none.tokens.empty() && none.text.empty(), "from_site_texts, no row, threads " << threads);
        const TokenList got = TokenList::from_site_texts(texts, threads);
        bool same = got.tokens.size() == 6 && std::string(got.text.begin(), got.text.end()) == "+AC-T+G-TTT+A+A";
        for (size_t k = 0; same && k < 6; ++k) {
            const bv_pileup_token &d = got.tokens[k];
            same = d.pos == want_pos[k] && d.sample == 0 && d.text_off == want_off[k] && d.text_len == want_len[k] && d.reserved_ == 0;
        }
        CHECK(same, "from_site_texts: descriptors keyed by the row's index, text back to back, threads " << threads);
        bool round = true;
        for (size_t i = 0; i < rows.size(); ++i) round = round && got.of((uint32_t)i) == rows[i];
        CHECK(round, "from_site_texts: of(i) gives row i's strings in order, threads " << threads);
    }
    // a lazy list is fetched once, and only when asked
    int fetches = 0;
    LazyTokenList lazy{[&](TokenList &into) { ++fetches; into = make_list({{4, "+A"}}); }};
    CHECK(fetches == 0, "LazyTokenList: nothing is fetched before a row asks");
    CHECK(lazy.get().of(4) == Strs({"+A"}) && lazy.get().of(5).empty() && fetches == 1, "LazyTokenList: one fetch for any number of rows");
}

// One record of the plan step's batch: variant, covered, every number inside the device's formats
static Site plan_site(uint32_t k) {
    Site s = make_site(3, k, 5000 + 10 * k);
    s.text.indel_tokens.clear();
    bv_site_result &r = s.r;
    if (!r.total_depth) { r.total_depth = 1; r.depth[s.ref] = 1; }
    if (!r.n_alt) { r.n_alt = 1; r.alt[0] = (uint8_t)((s.ref + 1) & 3); r.af[0] = 0.125; r.caf[0] = 0.5; }
    r.status = BV_SITE_COVERED | BV_SITE_VARIANT | BV_SITE_RANKSUM;
    s.g.n_alt = r.n_alt;
    for (int a = 0; a < r.n_alt; ++a) { s.g.alt[a] = r.alt[a]; s.g.af[a] = 0.5; }
    return s;
}

static void check_plan() {
    const uint32_t n = 12, first_row = 40;
    std::vector<SiteText> text;
    BaseTypeBatch result;
    result.n_groups = 1;
    for (uint32_t k = 0; k < n; ++k) {
        const Site s = plan_site(k);
        text.push_back(s.text);
        result.sites.push_back(s.r);
        result.groups.push_back(s.g);
    }
    std::vector<uint8_t> flagged(n, 0), host_read(n, 0);
    result.sites[1].af[0] = std::nan("");                                     // refused by the predicate
    flagged[2] = 1; text[2].indel_tokens = {"+AC", "-T"};                     // left to the caller by the tally
    host_read[3] = 1; text[3].indel_tokens = {"+AC", "-T"};                   // host-read, with tokens
    host_read[4] = 1;                                                         // host-read, without
    text[5].ref_id = "chrU";                                                  // not the batch's first CHROM
    text[6].ref_base = "AC";                                                  // two REF characters
    result.sites[7].status = BV_SITE_COVERED;                                 // no variant
    result.sites[8].total_depth = 0; flagged[8] = 1;                          // flagged, and the reference writes no row
    CHECK(bv_rt_on_device(&result.sites[0], &result.groups[0], 1) && !bv_rt_on_device(&result.sites[1], &result.groups[1], 1), "plan: the predicate takes row 0 and refuses row 1");
    const Strs column = {"", "", "+AC|1,-T|1", "+AC|1,-T|1", "", ".", "-T|2", "", "+A|1", "", "", ""};  // what host_column hands out
    const std::vector<uint8_t> as_host = {0, 1, 1, 1, 0, 1, 1, 0, 1, 0, 0, 0}, off_device = {0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0};
    const auto fits = [](const bv_site_result &r, const bv_group_result *g, uint32_t G) { return bv_rt_on_device(&r, g, G); };
    for (int run = 0; run < 2; ++run) {
        // the second run: a group name beyond BV_RECORD_TEXT_NAME_MAX -- every line is host text
        const std::vector<std::string> groups = {run ? std::string(BV_RECORD_TEXT_NAME_MAX + 1, 'g') : std::string("g1")};
        std::vector<size_t> asked;
        const EmitPlan p = plan_record_lines(groups, text, result, first_row, flagged, &host_read, 3, fits, [&](size_t i) { asked.push_back(i); return column[i]; });
        std::string cvg, vcf;
        std::vector<uint64_t> cvg_off(1, 0), vcf_off(1, 0);
        std::vector<uint32_t> vidx, site;
        std::vector<size_t> want_asked;
        uint64_t n_off = 0, n_col = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const bool off = run || off_device[i];
            n_off += off;
            if (run || as_host[i]) {
                want_asked.push_back(i);
                const std::string row = format_cvg_line(text[i], result.sites[i], column[i]);
                cvg += row;
                n_col += !row.empty() && !column[i].empty() && column[i] != ".";
            }
            cvg_off.push_back(cvg.size());
            if (i == 7) continue;
            if (off) vcf += format_vcf_head(text[i], result.sites[i], &result.groups[i], groups);
            vcf_off.push_back(vcf.size());
            vidx.push_back(i);
            site.push_back(first_row + i);
        }
        CHECK(asked == want_asked, "plan, run " << run << ": host_column is asked for the host-text rows and no other");
        CHECK(p.cvg_host == cvg && p.cvg_host_off == cvg_off, "plan, run " << run << ": the CVG host text and its offsets");
        CHECK(p.vcf_host == vcf && p.vcf_host_off == vcf_off, "plan, run " << run << ": the VCF host text and its offsets");
        CHECK(p.vidx == vidx && p.site == site && p.vrec.size() == 11 && p.vgrp.size() == 11, "plan, run " << run << ": the variant subset, its records and rows");
        CHECK(p.lines_host_formatted == n_off && p.indel_columns_host == n_col && n_off == (run ? 12u : 3u) && n_col == 3u,
              "plan, run " << run << ": the counters, got " << p.lines_host_formatted << " and " << p.indel_columns_host);
        const bv_record_lines v = p.vcf_lines(nullptr), c = p.cvg_lines(result);
        CHECK(std::string(c.chrom, c.chrom_len) == (run ? "-" : "chrT") && c.n_groups == (run ? 0u : 1u) && v.n_groups == c.n_groups && (c.groups != nullptr) == !run,
              "plan, run " << run << ": CHROM and the groups of both calls");
        CHECK(c.n_lines == n && v.n_lines == 11 && c.records == result.sites.data() && v.records == p.vrec.data() && v.site == p.site.data() && !c.site && !c.slab &&
              c.host_text_off == p.cvg_host_off.data() && v.host_text_off == p.vcf_host_off.data() && c.mem_kind == BV_MEM_HOST && !c.reserved_, "plan, run " << run << ": both bv_record_lines");
        CHECK(std::string(c.ref_char, n) == std::string("") + text[0].ref_base + text[1].ref_base + text[2].ref_base + text[3].ref_base + text[4].ref_base + text[5].ref_base + "N" +
              text[7].ref_base + text[8].ref_base + text[9].ref_base + text[10].ref_base + text[11].ref_base && c.pos[3] == 5030 && v.pos[7] == 5080,
              "plan, run " << run << ": positions and REF characters ('N' for a REF of two)");
    }
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
        check_token_list();
        check_plan();
    } catch (const std::exception &ex) {
        std::cout << "FAIL: " << ex.what() << std::endl;
        ++g_fails;
    }
    std::printf("CALL_PIPELINE cases %d FAILS %d\n", g_cases, g_fails);
    return g_fails ? 1 : 0;
}
