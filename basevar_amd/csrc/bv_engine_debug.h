// bv_engine_debug.h -- the report printers of the instrumented builds (BV_TEAM_DEBUG, BV_PHASE_DEBUG): what bv_engine_wait
// prints from the stamps the kernels left in the counter blocks behind the first.  Included by bv_engine.hip under BV_TEAM_DEBUG only.
#pragma once

#include <algorithm>
#include <cstdio>
#include <vector>

#include "bv_kernels.h"

#ifdef BV_TEAM_DEBUG
// bv_p1s_stream_kernel (short rows): when each wave finished its static range of sites, per XCD
static void bv_stream_debug_report(const uint32_t *h) {
    const uint32_t *d = h + BV_CTR_WORDS;
    uint32_t t0 = 0; bool any = false;
    for (int b = 0; b < 512; ++b)
        if (d[4096 + b] && (!any || (int32_t)(d[4096 + b] - t0) < 0)) { t0 = d[4096 + b]; any = true; }
    if (!any) return;
    std::vector<double> v;
    struct Acc { double sum = 0; uint32_t n = 0; };
    Acc by_xcc[8], by_wave[4], by_simd[4], by_cu[16], by_se[8], by_slot[16];
    for (int w = 0; w < 2048; ++w) {
        if (!d[w] || !d[4096 + w / 4]) continue;
        const double t = (double)(int32_t)(d[w] - t0) * 0.01;
        const uint32_t hw = d[2048 + w];
        v.push_back(t);
        auto add = [&](Acc &a) { a.sum += t; a.n++; };
        add(by_xcc[d[4608 + w / 4] & 7u]); add(by_wave[w & 3]); add(by_simd[(hw >> 4) & 3u]); add(by_cu[(hw >> 8) & 15u]); add(by_se[(hw >> 13) & 7u]);
        add(by_slot[hw & 15u]);
    }
    if (v.empty()) return;
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    fprintf(stderr, "[stream debug] wave done min %.1f p10 %.1f p25 %.1f p50 %.1f p75 %.1f p90 %.1f max %.1f us (%zu waves)\n", v[0], v[n / 10], v[n / 4],
            v[n / 2], v[n * 3 / 4], v[n * 9 / 10], v[n - 1], n);
    auto show = [&](const char *nm, Acc *a, int k) {
        fprintf(stderr, "[stream debug] mean by %-12s:", nm);
        for (int i = 0; i < k; ++i) if (a[i].n) fprintf(stderr, " %d:%.0f(%u)", i, a[i].sum / a[i].n, a[i].n);
        fprintf(stderr, "\n");
    };
    show("XCD", by_xcc, 8); show("wave of group", by_wave, 4); show("SIMD", by_simd, 4); show("CU id", by_cu, 16); show("SE/SH bits", by_se, 8);
    show("wave slot", by_slot, 16);
}
#endif

#ifdef BV_TEAM_DEBUG
// bv_p1s_fused_kernel: per workgroup, when its streaming waves were done, what was left for the solvers then, when it ended
static void bv_fused_debug_report(const uint32_t *h) {
    const uint32_t *d = h + BV_CTR_WORDS;
    uint32_t t0 = 0; bool any = false;
    for (int b = 0; b < 512; ++b)
        if (d[b * 8] && (!any || (int32_t)(d[b * 8] - t0) < 0)) { t0 = d[b * 8]; any = true; }
    if (!any) return;
    const char *nm[5] = {"entry", "first streaming wave past its pass-1 rows", "last streaming wave past its pass-1 rows", "workgroup done", "last solver job done"};
    const int col[5] = {0, 1, 2, 3, 5};
    for (int j = 0; j < 5; ++j) {
        std::vector<double> v; double sum[8] = {}; uint32_t cnt[8] = {};
        for (int b = 0; b < 512; ++b) {
            if (!d[b * 8] || !d[b * 8 + col[j]]) continue;
            const double t = (double)(int32_t)(d[b * 8 + col[j]] - t0) * 0.01;
            v.push_back(t); sum[d[b * 8 + 7] & 7u] += t; cnt[d[b * 8 + 7] & 7u]++;
        }
        if (v.empty()) continue;
        std::sort(v.begin(), v.end());
        const size_t n = v.size();
        fprintf(stderr, "[fused debug] %-42s min %6.1f p10 %6.1f p50 %6.1f p90 %6.1f max %6.1f us | mean per XCD:", nm[j], v[0], v[n / 10], v[n / 2],
                v[n * 9 / 10], v[n - 1]);
        for (int x = 0; x < 8; ++x) fprintf(stderr, " %.1f", cnt[x] ? sum[x] / cnt[x] : 0.);
        fprintf(stderr, "\n");
    }
#ifdef BV_PHASE_DEBUG
    {
        const char *pn[12] = {"wait for the slot (vmcnt)", "slot -> registers (4 ds_read_b128)", "request the next slot: the 4 DMA pieces", "tally, pass-1 slot", "tally, pass-2 slot",
                              "row epilogue, pass 1", "row epilogue, pass 2", "slots", "leaving (drain)", "inside the streaming function", "request the next slot: draw a row", "slot requested -> found landed"};
        for (int part = 0; part < 2; ++part) {
            const uint32_t *c = d + 4220 + 12 * part;
            fprintf(stderr, "[fused phases] -- streaming waves, %s\n", part ? "past their last pass-1 row" : "while they have pass-1 rows");
            for (int i = 0; i < 12; ++i) {
                if (i == 7) fprintf(stderr, "[fused phases] %-38s %u\n", pn[i], c[i]);
                else if (i == 11) fprintf(stderr, "[fused phases] %-38s %12.0f cycles  (%.0f per timed slot, %u timed)\n", pn[i], 16.0 * c[i], d[4244 + part] ? 16.0 * c[i] / d[4244 + part] : 0., d[4244 + part]);
                else if (i != 9 || part == 0) fprintf(stderr, "[fused phases] %-38s %12.0f cycles  (%.0f per slot)\n", pn[i], 16.0 * c[i], c[7] ? 16.0 * c[i] / c[7] : 0.);
            }
        }
    }
#endif
#ifdef BV_PHASE_DEBUG
    for (int l = 0; l < 2; ++l) {
        const uint32_t *j = d + 4212 + 4 * l;
        fprintf(stderr, "[fused phases] 16-lane jobs %s: %u (of them from q3: %u), %.2f sites per job, mean %.0f cycles\n", l ? "after the last pass-1 row" : "while rows stream", j[1], j[3],
                j[1] ? (double)j[2] / j[1] : 0., j[1] ? 16.0 * j[0] / j[1] : 0.);
    }
#endif
#ifdef BV_PHASE_DEBUG
    {
        const char *jn[5] = {"the entry, the summary's and the bins' loads", "phase 1: LRT, the record's first version", "its stores complete, variant sites queued",
                             "phase 2's loads", "phase 2: rank sum, QUAL, strand-bias tests"};
        const uint32_t nj = d[4213] + d[4217];
        for (int i = 0; i < 5; ++i) fprintf(stderr, "[fused phases] a 16-lane job, %-48s %8.0f cycles\n", jn[i], nj ? 16.0 * d[4250 + i] / nj : 0.);
    }
#endif
    const char *qn[3] = {"q3 entries", "q2 entries", "variant rows (or blocks of 64)"};
    for (int j = 0; j < 3; ++j) {
        std::vector<uint32_t> v;
        for (int b = 0; b < 512; ++b) if (d[b * 8]) v.push_back(j == 0 ? (d[b * 8 + 4] & 0xFFFFu) : j == 1 ? (d[b * 8 + 4] >> 16) : d[b * 8 + 6]);
        std::sort(v.begin(), v.end());
        fprintf(stderr, "[fused debug] waiting when the last streaming wave was past its pass-1 rows, %-30s: min %u p50 %u p90 %u max %u\n", qn[j], v[0],
                v[v.size() / 2], v[v.size() * 9 / 10], v.back());
    }
}
#endif
#ifdef BV_TEAM_DEBUG
// the stamps of bv_pass1_kernel's team form (see BV_TEAM_STAMP in bv_pass1_team.h): distribution over the workgroups, and per XCD
static void bv_team_debug_report(const uint32_t *h) {
    fprintf(stderr, "[team debug] team jobs %u (mean %.0f cycles)  solo solves %u (mean %.0f cycles)\n", h[BV_CTR_CANDS],
            h[BV_CTR_CANDS] ? 64.0 * h[BV_CTR_CANDS + 1] / h[BV_CTR_CANDS] : 0., h[BV_CTR_EASY3],
            h[BV_CTR_EASY3] ? 64.0 * h[BV_CTR_EASY3 + 1] / h[BV_CTR_EASY3] : 0.);
    fprintf(stderr, "[team debug] tally waves waiting for a free ring slot: %.0f cycles per workgroup (sum over its rows)\n", 64.0 * h[BV_CTR_EASY] / 1024.0);
    const uint32_t *d = h + BV_CTR_WORDS;
    const char *nm[6] = {"entry", "start barrier passed", "first row begins", "tally waves done", "phred tables in LDS", "solver wave done"};
    uint32_t t0 = 0; bool any = false;
    for (int b = 0; b < 640; ++b)
        if (d[b * 8] && (!any || (int32_t)(d[b * 8] - t0) < 0)) { t0 = d[b * 8]; any = true; }
    if (!any) return;
    for (int j = 0; j < 6; ++j) {
        std::vector<double> v; double sum[8] = {}; uint32_t cnt[8] = {};
        for (int b = 0; b < 640; ++b) {
            if (!d[b * 8]) continue;
            const double t = (double)(int32_t)(d[b * 8 + j] - t0) * 0.01;
            v.push_back(t); sum[d[b * 8 + 7] & 7u] += t; cnt[d[b * 8 + 7] & 7u]++;
        }
        std::sort(v.begin(), v.end());
        const size_t n = v.size();
        fprintf(stderr, "[team debug] %-22s min %6.1f p10 %6.1f p50 %6.1f p90 %6.1f max %6.1f us | mean per XCD:", nm[j], v[0], v[n / 10], v[n / 2],
                v[n * 9 / 10], v[n - 1]);
        for (int x = 0; x < 8; ++x) fprintf(stderr, " %.1f", cnt[x] ? sum[x] / cnt[x] : 0.);
        fprintf(stderr, "\n");
    }
}
#endif
