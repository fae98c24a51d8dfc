// Test harness (tests/ only, needs a GPU): the device's batchfile row parser (bv_engine_text_parse / _submit, driven through
// BaseTypeEngine::lrt_text) against the host reader parse_site_rows_fast on the same bytes.
//
// Every case is a batch of three positions -- a clean row, the case, a clean row -- in the same files.  For the case the device
// must either parse it to exactly what the host reader writes (cell and phred planes, SiteText, records), or mark it "host";
// the batch as a whole must give the records, skips and error (message and position) of the host reader run position by
// position.  Cases: the row cases of host_formats_check.cpp's FAST_READER_CASES (restated here), and a seeded corpus of damaged
// valid rows.  Usage: text_rows_check [n_sites]; prints "TEXT_ROWS device <n> host <n> skipped <n> threw <n>" and "FAILS <n>".
//
// text_rows_check <n> lanes runs the positional corpus of row_lane_cases.hpp instead -- valid rows with every token start, tab and
// line break on every lane of the kernel's 64-byte steps, damage placed on the lanes at the step boundaries -- through the same
// comparison, many positions to a batch: a case the host reader does not throw on stands between clean positions, a case it
// throws on ends its batch.  Every row of the valid sweep and every clean position must be parsed on the device.
// text_rows_check <n> lanes-dump <file> writes the corpus's cases that can stand in a file of lines and that the host reader does
// not throw on ("CASE <valid> <samples per file, comma separated> <kind>", then one row per file), for the BGZF route
// (tests/test_gpu_bgzf_rows.py); it does not touch the GPU.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <random>

#include "../../basevar_amd/host/basetype_gpu.hpp"
#include "../../basevar_amd/host/batchfile_fast.hpp"
#include "row_lane_cases.hpp"

using namespace bvamd;

static int fails = 0;
#define CHECK(cond, msg) do { if (!(cond)) { std::cerr << "FAIL: " << msg << std::endl; ++fails; } } while (0)

struct HostRun {  // the host reader, position by position, as BatchfileProducer runs it
    SlabBuilder sb;
    std::vector<SiteText> text;
    std::vector<uint32_t> position;
    std::string error;
    uint32_t n_used = 0;
    explicit HostRun(uint32_t n) : sb(n) {}
};

static size_t n_device = 0, n_host = 0, n_skip = 0, n_threw = 0;

// what a position of a batch is: a clean row, a case, or a row of the valid sweep (a case that must be parsed on the device)
enum { CLEAN = 0, CASE = 1, VALID = 2 };

// `what` / `tags`: per position (default: clean, the case, clean -- all under `tag`)
static void run_case(BaseTypeEngine &eng, const std::vector<std::vector<std::string>> &batch, const std::vector<uint32_t> &fs,
                     const char *tag0, const std::vector<int> &what = {CLEAN, CASE, CLEAN}, const std::vector<std::string> *tags = nullptr) {
    const std::string all_tags = tags ? (*tags)[0] + " .. " + tags->back() : std::string(tag0);
    const char *tag = all_tags.c_str();
    auto tag_of = [&](size_t p) { return tags ? (*tags)[p] : std::string(tag0); };
    uint32_t N = 0;
    for (uint32_t v : fs) N += v;
    const size_t F = fs.size();
    std::string text;
    std::vector<uint64_t> off{0};
    for (const auto &pos : batch)
        for (const auto &r : pos) { text += r; text += '\n'; off.push_back(text.size()); }
    HostRun h(N);
    for (uint32_t p = 0; p < batch.size(); ++p, ++h.n_used) {
        SiteText st;
        try {
            if (!parse_site_rows_fast(batch[p], N, h.sb, st)) continue;
        } catch (const std::exception &e) { h.error = e.what(); break; }
        h.text.push_back(st);
        h.position.push_back(p);
    }
    const bv_text_rows rows{text.data(), off.data(), fs.data(), text.size(), (uint32_t)batch.size(), (uint32_t)F, 0};
    BaseTypeEngine::TextBatch tb;
    try {
        tb = eng.lrt_text(rows, [](const std::vector<std::string> &r, size_t n, SlabBuilder &sb, SiteText &st) {
            return parse_site_rows_fast(r, n, sb, st);
        });
    } catch (const std::exception &e) {
        CHECK(false, tag << ": lrt_text threw " << e.what());
        return;
    }
    std::string dev_error;
    if (tb.error) {
        try { std::rethrow_exception(tb.error); } catch (const std::exception &e) { dev_error = e.what(); }
    }
    for (uint32_t p = 0; p < batch.size(); ++p) {
        if (what[p] == CLEAN) continue;
        const uint8_t st1 = tb.row_state[p * F];
        (st1 & BV_TEXT_HOST ? n_host : st1 & BV_TEXT_SKIP ? n_skip : n_device)++;
    }
    if (!h.error.empty()) ++n_threw;
    CHECK(dev_error == h.error, tag << ": error [" << dev_error << "] vs host [" << h.error << "]");
    CHECK(tb.n_positions_used == h.n_used, tag << ": positions used " << tb.n_positions_used << " vs host " << h.n_used);
    CHECK(tb.position == h.position, tag << ": different positions kept");
    if (tb.position != h.position) return;
    // the clean positions are always the device's; the case is the device's only if the host reader wrote those same bytes
    for (uint32_t p = 0; p < batch.size(); ++p)
        if (what[p] != CASE)
            CHECK(!(tb.row_state[p * F] & (BV_TEXT_HOST | BV_TEXT_SKIP)), tag_of(p) << ": " << (what[p] == VALID ? "valid" : "clean") << " position " << p << " not parsed on the device");
    BaseTypeBatch ref;
    if (h.sb.n_sites()) ref = eng.lrt(h.sb);
    CHECK(ref.sites.size() == tb.batch.sites.size(), tag << ": record count");
    for (size_t i = 0; i < h.position.size() && i < tb.batch.sites.size(); ++i) {
        const std::string tag_i = tag_of(h.position[i]);
        const char *tag = tag_i.c_str();
        CHECK(std::memcmp(&ref.sites[i], &tb.batch.sites[i], sizeof(bv_site_result)) == 0, tag << ": record " << i << " differs");
        CHECK(std::memcmp(h.sb.cell_row(i), &tb.cell[i * N], N) == 0, tag << ": cell plane of record " << i);
        CHECK(std::memcmp(h.sb.phred_row(i), &tb.phred[i * N], N) == 0, tag << ": phred plane of record " << i);
        const SiteText &a = h.text[i], &b = tb.text[i];
        CHECK(a.ref_id == b.ref_id && a.ref_pos == b.ref_pos && a.ref_base == b.ref_base && a.indel_tokens == b.indel_tokens,
              tag << ": SiteText of record " << i);
    }
}

// one clean row of file f: n samples, a deterministic mix of calls, indels and uncovered cells
static std::string clean_row(uint32_t pos, uint32_t n, uint32_t salt, bool ref_a = true) {
    std::string mq, bs, q, rk, sd;
    uint32_t cov = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = (i * 7 + salt * 3 + pos) % 11;
        const char *b = k < 4 ? "ACGT" + k : k == 4 ? "+AC" : k == 5 ? "-G" : "N";
        const bool covered = k <= 5;
        cov += covered;
        auto add = [&](std::string &s, const std::string &t) { if (i) s += ' '; s += t; };
        add(mq, covered ? std::to_string(20 + (i * 13 + salt) % 41) : "0");
        add(bs, k < 4 ? std::string(1, b[0]) : std::string(b));
        add(q, covered ? std::string(1, (char)('!' + 5 + (i * 5 + salt) % 36)) : "!");
        add(rk, covered ? std::to_string(1 + (i * 11 + salt) % 150) : "0");
        add(sd, covered ? ((i + salt) % 2 ? "-" : "+") : ".");
    }
    return "chrT\t" + std::to_string(pos) + "\t" + (ref_a ? "A" : "c") + "\t" + std::to_string(cov) + "\t" + mq + "\t" + bs + "\t" +
           q + "\t" + rk + "\t" + sd;
}

// the positional corpus (row_lane_cases.hpp); `dump`: only write the cases for the BGZF route
static int run_lanes(const char *dump) {
    const std::vector<rowlane::Case> cases = rowlane::corpus();
    CHECK(rowlane::check_corpus(cases, std::cout) == 0, "the positional corpus does not reach the lanes / defects it must");
    // the host reader first: a case it throws on ends a batch
    std::vector<char> throws(cases.size(), 0);
    std::map<std::vector<uint32_t>, std::vector<size_t>> by_files;
    for (size_t i = 0; i < cases.size(); ++i) {
        uint32_t N = 0;
        for (uint32_t v : cases[i].fs) N += v;
        SlabBuilder sb(N);
        SiteText st;
        try { parse_site_rows_fast(cases[i].rows, N, sb, st); } catch (const std::exception &) { throws[i] = 1; }
        by_files[cases[i].fs].push_back(i);
    }
    if (dump) {
        std::ofstream out(dump, std::ios::binary);
        for (size_t i = 0; i < cases.size(); ++i) {
            if (throws[i] || cases[i].inner_newline) continue;
            out << "CASE " << (cases[i].valid ? 1 : 0) << " ";
            for (size_t f = 0; f < cases[i].fs.size(); ++f) out << (f ? "," : "") << cases[i].fs[f];
            out << " " << cases[i].kind << "\n";
            for (const std::string &r : cases[i].rows) out << r << "\n";
        }
        return fails ? 1 : 0;
    }
    const uint32_t kBatch = 64;  // positions per batch, and the engine's max_sites
    size_t n_batches = 0;
    for (const auto &group : by_files) {
        const std::vector<uint32_t> &fs = group.first;
        uint32_t N = 0;
        for (uint32_t v : fs) N += v;
        BaseTypeEngine eng(kBatch, N);
        std::vector<std::vector<std::string>> batch;
        std::vector<int> what;
        std::vector<std::string> tags;
        uint32_t clean_pos = 1;
        auto add_clean = [&]() {
            std::vector<std::string> rows;
            for (size_t f = 0; f < fs.size(); ++f) rows.push_back(rowlane::clean(clean_pos, fs[f], (uint32_t)f + 3).str());
            ++clean_pos;
            batch.push_back(rows); what.push_back(CLEAN); tags.push_back("clean");
        };
        auto flush = [&]() {
            if (batch.empty()) return;
            run_case(eng, batch, fs, "lanes", what, &tags);
            ++n_batches;
            batch.clear(); what.clear(); tags.clear();
        };
        for (size_t i : group.second) {
            const rowlane::Case &c = cases[i];
            if (!c.valid) add_clean();
            batch.push_back(c.rows); what.push_back(c.valid ? VALID : CASE); tags.push_back(c.kind);
            if (throws[i]) flush();  // the reader stops here: nothing behind it would be looked at
            else if (batch.size() + 3 > kBatch) { add_clean(); flush(); }
        }
        if (!batch.empty()) { add_clean(); flush(); }
    }
    std::cout << "TEXT_ROWS_LANES batches " << n_batches << " device " << n_device << " host " << n_host << " skipped " << n_skip << " threw " << n_threw << std::endl;
    CHECK(n_device > 0 && n_host > 0 && n_skip > 0 && n_threw > 0, "the positional corpus exercises every outcome");
    std::cout << "FAILS " << fails << std::endl;
    return fails ? 1 : 0;
}

int main(int argc, char **argv) {
    const int n_sites = argc > 1 ? std::atoi(argv[1]) : 40;
    if (argc > 2 && std::string(argv[2]) == "lanes") return run_lanes(nullptr);
    if (argc > 3 && std::string(argv[2]) == "lanes-dump") return run_lanes(argv[3]);
    BaseTypeEngine eng(8, 64);
    auto with_clean = [&](const std::vector<std::string> &rows, const std::vector<uint32_t> &fs, const char *tag) {
        std::vector<std::vector<std::string>> batch(3);
        for (size_t f = 0; f < fs.size(); ++f) {
            batch[0].push_back(clean_row(3, fs[f], (uint32_t)f));
            batch[2].push_back(clean_row(9, fs[f], (uint32_t)f + 5));
        }
        batch[1] = rows;
        run_case(eng, batch, fs, tag);
    };
    // ---- the row cases of host_formats_check.cpp (FAST_READER_CASES), restated
    with_clean({"chr1\t5\tA\t1\t60"}, {1}, "short row");
    with_clean({"chr1\t5\tA\t1\t60\tA\tI\t3\t+", "chr1\t6\tA\t1\t60\tA\tI\t3\t+"}, {1, 1}, "coordinate mismatch");
    with_clean({"chr1\t5\tA\t0\t60\tAC\tI\t3\tx"}, {1}, "depth 0 hides a bad token");
    with_clean({"chr1\t5\tA\t1\t60\tAC\tI\t3\tx"}, {1}, "base token of two characters");
    with_clean({"chr1\t5\tA\t1\t60\tR\tI\t3\t+"}, {1}, "base outside ACGT");
    with_clean({"chr1\t5\tA\t1\t60\tA\tI\t3\tx"}, {1}, "strange strand");
    with_clean({"chr1\t5\tA\t2\t60 \tA N\t I\t3 +4\t+ ."}, {2}, "empty tokens");
    with_clean({"chr1\t5\tA\t1\t60 60\tA \tI I\t3 3\t+ +"}, {2}, "empty base token");
    with_clean({"chr1\t5\ta\t1\t-3\t+AT\t\t70000\t-"}, {1}, "negative mapq, empty quality, rank past 16 bits");
    with_clean({"chr1\t5\tA\t1\t60\tA\tI\t3\t+\r"}, {1}, "CRLF line end");
    with_clean({"chr1\t5\tA\t1\t60\tA\tI\t3\t+\t"}, {1}, "trailing tab");
    with_clean({"chr1\t99999999999\tA\t1\t60\tA\tI\t3\t+"}, {1}, "position past int");
    with_clean({"chr1\tx5\tA\t1\t60\tA\tI\t3\t+"}, {1}, "position not a number");
    with_clean({"chr1\t5\tA\tone\t60\tA\tI\t3\t+"}, {1}, "depth not a number");
    with_clean({"chr1\t5\tA\t-1\t60\tA\tI\t3\t+", "chr1\t5\tA\t1\t60\tC\tI\t3\t-"}, {1, 1}, "depths summing to zero hide the row");
    with_clean({"chr1\t5\tA\t1\t 60\tA\tI\t3\t+"}, {1}, "leading blank in a column");
    with_clean({"chr1\t5\t\t1\t60\tA\tI\t3\t+"}, {1}, "empty reference base");
    with_clean({"chr1\t5\tAC\t1\t60\tA\tI\t3\t+"}, {1}, "two reference bases");
    with_clean({"chr1\t5\tA\t1\t60\ta\tI\t3\t+"}, {1}, "lower-case read base");
    with_clean({"chr1\t5\tA\t1\t6e1\tA\tI\t3.7\t+"}, {1}, "numbers the int reader stops inside");
    with_clean({"chr1\t5\tA\t2\t60 60\t+A -A\tI I\t3 4\t. ."}, {2}, "indels only, no strands");
    with_clean({"chr1\t5\tA\t2\t60 60\tA N\tI !\t3 0\t+ x"}, {2}, "a strange strand on an N call is never looked at");
    with_clean({"chr1\t5\tA\t1\t60\tA\tI\t3\t."}, {1}, "a covered call with strand '.'");
    with_clean({"chr1\t5\tA\t1\t60 7\tA N\tI !\t3 0\t+ .", "chr1\t5\tA\t0\t0\tN\t!\t0\t."}, {1, 2}, "ragged per-file counts");
    with_clean({"chr1\t5\tA\t1\t0060\tA\tI\t00003\t+"}, {1}, "leading zeros");
    with_clean({"chr1\t5\tA\t1\t255\tA\t~\t65535\t-"}, {1}, "largest strict values");
    with_clean({"chr1\t5\tA\t1\t256\tA\tI\t3\t+"}, {1}, "mapq past a byte");
    // ---- seeded damage of valid rows: 3 files of 2, 5 and 1 samples
    const std::vector<uint32_t> fs = {2, 5, 1};
    std::mt19937_64 rnd(20261015);
    for (int s = 0; s < n_sites; ++s) {
        std::vector<std::string> rows;
        for (size_t f = 0; f < fs.size(); ++f) rows.push_back(clean_row(100 + s, fs[f], (uint32_t)(s * 3 + f), s % 4 != 0));
        with_clean(rows, fs, "valid");
        for (int rep = 0; rep < 24; ++rep) {
            std::vector<std::string> bad = rows;
            const int hits = 1 + (int)(rnd() % 3);
            for (int k = 0; k < hits; ++k) {
                std::string &r = bad[rnd() % bad.size()];
                if (r.empty()) continue;
                const size_t at = rnd() % r.size();
                switch (rnd() % 14) {
                    case 0: r.erase(at, 1 + rnd() % 3); break;
                    case 1: r.insert(at, " "); break;
                    case 2: r.insert(at, "\t"); break;
                    case 3: r[at] = "ACGTN+-.!x5 \t-"[rnd() % 14]; break;
                    case 4: r.insert(at, "-7"); break;
                    case 5: r.insert(at, "99999999999"); break;
                    case 6: { const size_t sp = r.find(' ', at); if (sp != std::string::npos) r.erase(at, sp - at); break; }
                    case 7: { const size_t tb = r.rfind('\t'); if (tb != std::string::npos && (rnd() & 1)) r.erase(tb); break; }
                    case 8: r[at] = (char)(rnd() & 0xFF); break;           // byte flip
                    case 9: r.insert(at, "\r"); break;
                    case 10: {  // a 4-digit mapq in front of the first one
                        const size_t t4 = r.find('\t', r.find('\t', r.find('\t', r.find('\t') + 1) + 1) + 1);
                        if (t4 != std::string::npos) r.replace(t4 + 1, 0, "1000");
                        break;
                    }
                    case 11: {  // a 6-digit rank in front of the first one
                        const size_t t7 = r.rfind('\t');
                        const size_t t6 = t7 == std::string::npos || t7 == 0 ? std::string::npos : r.rfind('\t', t7 - 1);
                        if (t6 != std::string::npos) r.replace(t6 + 1, 0, "123456");
                        break;
                    }
                    case 12: r.append("\r"); break;
                    default: r.insert(at, "+ACG"); break;
                }
            }
            with_clean(bad, fs, "damaged");
        }
    }
    std::cout << "TEXT_ROWS device " << n_device << " host " << n_host << " skipped " << n_skip << " threw " << n_threw << std::endl;
    CHECK(n_device > 50 && n_host > 50 && n_threw > 20, "the corpus exercises every outcome");
    std::cout << "FAILS " << fails << std::endl;
    return fails ? 1 : 0;
}
