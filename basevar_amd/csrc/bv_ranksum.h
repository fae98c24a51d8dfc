// bv_ranksum.h -- the Wilcoxon rank sum from value histograms: 64 values per window on a wave, 16 on a row, and the z -> phred tail.
// Included by bv_device.h, behind bv_wave.h and bv_kfunc.h (bv_kf_erfc).
#pragma once

// ------------------------------------------------------------------ Wilcoxon rank sum
// ref_vs_alt_ranksumtest -> wilcoxon_ranksum_test, src/basetype.cpp:201-233 and
// src/algorithm.h:76-136, evaluated from value histograms.  With descending order and
// average ranks for ties the rank of value v is above_v + (t_v + 1) / 2, i.e.
// n - below_v - t_v + (t_v + 1)/2; twice the ref rank sum is an exact integer:
//     2 R_ref = sum_v ref_v * (2 n - 2 below_v - t_v + 1)
// (bit-identical to the sort-based reference).
//
// Streaming form: feed values in ascending order, 64 per call (lane = value), carrying
// `below`.  Returns this window's contribution to 2 R_ref and updates below.
__device__ inline unsigned long long bv_ranksum_window(uint32_t ref_v, uint32_t alt_v, unsigned long long n,
                                                       unsigned long long &below, int lane) {
    uint32_t t = ref_v + alt_v;
    // (a window without a count adds nothing to the sum nor to `below`: mapq stops at 60, read-position ranks at the read length,
    // so most windows of most rows are empty, and a scan, a 64-bit product and a 64-bit wave sum are ~50 instructions)
    if (__ballot(t != 0u) == 0ull) return 0ull;
    uint32_t incl = bv_wave_incl_scan_u32(t);
    unsigned long long below_v = below + (incl - t);
    unsigned long long term = (unsigned long long)ref_v * (2ull * n - 2ull * below_v - t + 1ull);
    unsigned long long s = bv_wave_sum_u64(term);
    below += (unsigned long long)(uint32_t)bv_readlane63_i32((int)incl);
    return s;
}
// z statistic -> phred, algorithm.h:130-132 + basetype.cpp:222-231
__device__ inline double bv_ranksum_phred(unsigned long long twoR, unsigned long long n1, unsigned long long n2) {
    if (n1 == 0 || n2 == 0) return 10000;
    double r1 = (double)twoR / 2.0;
    double e = (double)(n1 * (n1 + n2 + 1)) / 2.0;
    double z = (r1 - e) / sqrt((double)(n1 * n2 * (n1 + n2 + 1)) / 12.0);
    double p = 2 * (bv_kf_erfc((double)(fabs(z) / sqrt(2.0))) / 2.0);
    double ph = -10 * log10(p);
    if (isinf(ph)) ph = 10000;
    return ph;
}

// ------------------------------------------------------------------ Wilcoxon rank sum, 16 values per window
__device__ inline unsigned long long bv_ranksum_window_g16(uint32_t ref_v, uint32_t alt_v, unsigned long long n,
                                                           unsigned long long &below) {
    const uint32_t t = ref_v + alt_v;
    const uint32_t incl = bv_g16_incl_scan_u32(t);
    const unsigned long long below_v = below + (incl - t);
    const unsigned long long term = (unsigned long long)ref_v * (2ull * n - 2ull * below_v - t + 1ull);
    const unsigned long long s = bv_g16_sum_u64(term);
    below += (unsigned long long)bv_g16_sum_u32(t);
    return s;
}
