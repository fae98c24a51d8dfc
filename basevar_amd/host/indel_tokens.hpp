// indel_tokens.hpp -- the '+SEQ' / '-SEQ' tokens of a batch on the host, without an engine call: a position-keyed list of them
// however it came to the host -- the engine's list of the last parse, the tokens of a pileup window, or the SiteTexts' own
// strings laid out for bv_engine_indel_tally -- and the walk that takes them from a parsed batchfile row.
#pragma once

#include <algorithm>
#include <cstring>
#include <exception>
#include <functional>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include "../../include/basevar_amd_indel.h"  // bv_pileup_token (basevar_amd_pileup.h), bv_indel_tokens
#include "vcf_emit.hpp"                       // SiteText

namespace bvamd {

// fn(t, lo, hi) over [0, n) on up to `threads` threads (contiguous ranges; the caller's thread takes the first)
// An exception in any range (a malformed row, bad_alloc under large batches) is caught on its thread and the first one rethrown
// on the caller's thread once all ranges are done -- the tool's "[ERROR] ..." exit path, not std::terminate.
template <typename Fn>
void parallel_ranges(size_t n, int threads, Fn fn) {
    const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), n));
    if (nt <= 1) { fn(0, 0, n); return; }
    std::vector<std::thread> pool;
    std::vector<std::exception_ptr> errs(nt);
    for (size_t t = 1; t < nt; ++t)
        pool.emplace_back([&, t]() { try { fn(t, n * t / nt, n * (t + 1) / nt); } catch (...) { errs[t] = std::current_exception(); } });
    try { fn(0, 0, n / nt); } catch (...) { errs[0] = std::current_exception(); }
    for (auto &th : pool) th.join();
    for (auto &e : errs) if (e) std::rethrow_exception(e);
}

// The tokens of one parsed batchfile row that carries the BV_TEXT_INDEL mark, appended to `out` in sample order: to Readbases
// over five tabs (a parsed row has its 8 tabs), then token by token to the column's tab
inline void row_indel_tokens(const char *row, std::vector<std::string> &out) {
    const char *p = row;
    for (int k = 0; k < 5; ++k) { while (*p != '\t') ++p; ++p; }
    for (;;) {
        const char *q = p;
        while (*q != ' ' && *q != '\t') ++q;
        if (*p == '+' || *p == '-') out.emplace_back(p, (size_t)(q - p));
        if (*q == '\t') break;
        p = q + 1;
    }
}

struct TokenList {
    std::vector<bv_pileup_token> tokens;  // ascending by pos
    std::vector<uint8_t> text;

    std::string_view view(size_t k) const { return std::string_view(reinterpret_cast<const char *>(text.data()) + tokens[k].text_off, tokens[k].text_len); }
    uint64_t bytes() const { return sizeof(bv_pileup_token) * tokens.size() + text.size(); }  // what a fetch of the list brings over
    bv_indel_tokens as_indel_tokens() const { return bv_indel_tokens{tokens.data(), text.data(), tokens.size(), text.size(), BV_MEM_HOST, 0}; }

    // the tokens of one position, in list order
    std::vector<std::string> of(uint32_t pos) const {
        std::vector<std::string> out;
        auto it = std::lower_bound(tokens.begin(), tokens.end(), pos, [](const bv_pileup_token &t, uint32_t p) { return t.pos < p; });
        for (; it != tokens.end() && it->pos == pos; ++it) out.emplace_back(view((size_t)(it - tokens.begin())));
        return out;
    }
    // One forward pass over ascending keys: every token from `cursor` on whose pos is key[i] goes to texts[i].indel_tokens, the
    // tokens below a key belong to no record; `cursor` runs on, so the next call takes the keys that follow
    void deal(const uint32_t *key, size_t n, SiteText *texts, size_t &cursor) const {
        for (size_t i = 0; i < n && cursor < tokens.size(); ++i) {
            while (cursor < tokens.size() && tokens[cursor].pos < key[i]) ++cursor;
            for (; cursor < tokens.size() && tokens[cursor].pos == key[i]; ++cursor) texts[i].indel_tokens.emplace_back(view(cursor));
        }
    }
    // The SiteTexts' own strings as a list keyed by the row's index in `texts`
    // (a row of 10,000 samples brings hundreds of tokens: the descriptors are laid out on the run's host threads)
    static TokenList from_site_texts(const std::vector<SiteText> &texts, int threads) {
        const size_t n = texts.size();
        std::vector<uint64_t> token_at(n + 1, 0), text_at(n + 1, 0);
        parallel_ranges(n, threads, [&](size_t, size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i) {
                token_at[i + 1] = texts[i].indel_tokens.size();
                for (const std::string &t : texts[i].indel_tokens) text_at[i + 1] += t.size();
            }
        });
        for (size_t i = 0; i < n; ++i) { token_at[i + 1] += token_at[i]; text_at[i + 1] += text_at[i]; }
        TokenList list;
        list.tokens.resize(token_at[n]);
        list.text.resize(text_at[n]);
        parallel_ranges(n, threads, [&](size_t, size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; ++i) {
                uint64_t k = token_at[i], at = text_at[i];
                for (const std::string &t : texts[i].indel_tokens) {
                    list.tokens[k++] = bv_pileup_token{(uint32_t)i, 0u, at, (uint32_t)t.size(), 0u};
                    std::memcpy(list.text.data() + at, t.data(), t.size());
                    at += t.size();
                }
            }
        });
        return list;
    }
};

// A list that stays on the device until a row asks for it: fetch(list) runs at most once, at the first get()
struct LazyTokenList {
    std::function<void(TokenList &)> fetch;
    TokenList list;
    bool fetched = false;
    const TokenList &get() {
        if (!fetched) { fetch(list); fetched = true; }
        return list;
    }
};

}  // namespace bvamd
