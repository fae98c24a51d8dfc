// Test harness (tests/ only): bv_span_words of basevar_amd/csrc/bv_text_image.h, the cut of an image range [lo, hi) into lead
// bytes, whole 16-byte words and tail bytes behind the store of both device text writers (bv_vcf.hip, bv_pileup_text.hip).  A
// program of its own (tests/test_text_image_cpu.py builds it with ASan + UBSan and runs it); it includes nothing else of the engine.
//   text_image_check
//       every lo in 0 .. 47 -- a range that starts in, at and behind a word boundary -- with every hi in lo .. lo + 96 -- none to
//       six whole words: each byte of [lo, hi) has exactly one writer and no byte outside it has one, the word range is whole
//       aligned words, each edge is at most 15 bytes, and a range without a whole word has no word range.
#include <cstdio>
#include <vector>

#include "../../basevar_amd/csrc/bv_text_image.h"

int main() {
    unsigned cases = 0, fails = 0;
    for (uint32_t lo = 0; lo < 48u; ++lo)
        for (uint32_t hi = lo; hi <= lo + 96u; ++hi, ++cases) {
            const BvSpanWords s = bv_span_words(lo, hi);
            std::vector<int> writers(hi + 32u, 0);  // bytes [0, hi + 32): the stores below stay inside or the sanitizer says so
            for (uint32_t i = lo; i < s.lead_end; ++i) writers.at(i) += 1;
            for (uint32_t w = s.w_lo; w < s.w_hi; ++w)
                for (uint32_t i = 16u * w; i < 16u * w + 16u; ++i) writers.at(i) += 1;
            for (uint32_t i = s.tail_at; i < hi; ++i) writers.at(i) += 1;
            bool ok = true;
            for (uint32_t i = 0; i < writers.size(); ++i) ok = ok && writers[i] == (i >= lo && i < hi ? 1 : 0);  // disjoint, and their union is [lo, hi)
            const uint32_t lead = s.lead_end > lo ? s.lead_end - lo : 0u, tail = hi > s.tail_at ? hi - s.tail_at : 0u;
            ok = ok && lead <= 15u && tail <= 15u;
            ok = ok && s.lead_end >= lo && s.lead_end <= hi && s.tail_at >= s.lead_end && s.tail_at <= hi;
            if (s.w_lo < s.w_hi) ok = ok && 16u * s.w_lo == s.lead_end && 16u * s.w_hi == s.tail_at;  // the words lie between the edges
            const bool holds_word = (lo + 15u) / 16u * 16u + 16u <= hi;  // the first word boundary at or behind lo, and 16 bytes
            if (!holds_word) ok = ok && s.w_hi <= s.w_lo;
            if (!ok) {
                if (++fails <= 10) std::printf("lo %u hi %u: lead_end %u words [%u, %u) tail_at %u\n", lo, hi, s.lead_end, s.w_lo, s.w_hi, s.tail_at);
            }
        }
    std::printf("TEXT_IMAGE cases %u FAILS %u\n", cases, fails);
    return fails ? 1 : 0;
}
