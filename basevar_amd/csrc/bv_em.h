// bv_em.h -- the EM on weighted (base, phred) bins over a wave, in its general and its positive form, and the ordered replay
// of shallow sites in the reference's own sample order.
// Included by bv_device.h, behind bv_hostlog.h and bv_wave.h.
#pragma once

// ------------------------------------------------------------------ EM on weighted bins
// The compacted non-empty histogram bins live in LDS (bin i: code = base<<7 | phred, count);
// bin i is handled by lane i % 64 in slot i / 64.  Only the per-bin log-marginal of the
// previous iteration is carried in registers, so the solver stays light on VGPRs and the
// streaming phase of the same kernel keeps its occupancy.
struct BvBins {
    const uint32_t *code;  // LDS; bin i is at code[bv_bin_at(B, i)]
    const uint32_t *cnt;   // LDS
    uint32_t skip_mask;    // 0: dense arrays; ~127u: 128 entries, then 128 words skipped, ... (bins
                           // stored in the unused upper halves of the histogram rows, bv_pass1.hip)
    const double *hit;     // LDS copy of BvTables::hit  (1 - eps)
    const double *miss;    // LDS copy of BvTables::miss (eps / 3)
    const double *loghit;  // BvTables::loghit / logmiss (device memory, L2-resident), or NULL: single-base subsets then
    const double *logmiss; // run the iterative EM like every other subset
    int nb;                // number of bins (wave-uniform)
    const uint16_t *ord;   // LDS: the site's covered cells in SAMPLE ORDER (call << 8 | phred), or NULL.  When given (shallow
    int n_ord;             // sites), every EM of the LRT replays the reference's per-sample arithmetic literally (bv_em_ordered)
};

__device__ __forceinline__ int bv_bin_at(const BvBins &B, int i) { return i + (int)((uint32_t)i & B.skip_mask); }

// The reference's convergence term: algorithm.h:245 binds to int abs(int), so the double
// difference is truncated to int first (x86 cvttsd2si: NaN / out-of-range -> INT_MIN,
// and abs(INT_MIN) stays INT_MIN).
__device__ __forceinline__ double bv_int_abs_trunc(double d) {
    if (isnan(d) || fabs(d) >= 2147483648.0) return -2147483648.0;
    int t = (int)d;
    return (double)(t < 0 ? -t : t);
}

// log-likelihood sum at the marginals `pm` of an EM's last pass (algorithm.h:243, basetype.cpp:123-125)
__device__ __forceinline__ double bv_em_loglik(const BvBins &B, const double (&pm)[BV_SLOTS], int nslots, int lane) {
    double lr = 0.;
#pragma unroll
    for (int s = 0; s < BV_SLOTS; ++s) {
        if (s < nslots) {
            const int i = s * BV_WAVE + lane;
            if (i < B.nb) lr += (double)B.cnt[bv_bin_at(B, i)] * log(pm[s]);
        }
    }
    return bv_wave_sum(lr);
}

// EM, algorithm.h:210-255.  f: initial freqs in, final freqs out.  Returns loop iterations.
// Pass k = 0 is the reference's pre-loop e_step/m_step (algorithm.h:226-234); passes
// k = 1..100 are the `while (iter_num--)` body (algorithm.h:235-251).  Each pass is one
// fused sweep over the bins: e_step (algorithm.h:161-171), the m_step numerators
// (algorithm.h:190-193), log-marginals and the convergence sum (algorithm.h:243-247).
// Bin i lives in lane i % 64, slot i / 64; only the per-bin marginal of the previous pass
// is carried (in registers).  (A branch-free variant that kept three bins per lane in flight
// for ILP, with the log-marginals in LDS, was measured 13 % SLOWER end to end: the solver wave
// shares its SIMD with tally waves, so its instruction count matters more than its latency.)
__device__ __forceinline__ int bv_em_wave_generic(const BvBins &B, double f[4], double n_cov, double *lr_out, int lane) {
    const double epsilon = (double)0.001f;  // `const float epsilon=0.001`, algorithm.h:213
    const int nslots = (B.nb + BV_WAVE - 1) / BV_WAVE;
    // The reference takes log(marginal) of every sample in every pass, but uses the values only (a) in
    // the convergence term |int(llh_new - llh_old)| (algorithm.h:245, integer abs: zero unless the two logs
    // differ by >= 1) and (b) from the LAST pass, as the log-likelihood sum.  So the previous pass's
    // MARGINAL is carried instead of its log; a pass takes logs only for the bins whose marginal moved
    // by a factor outside (0.37, 2.7) -- |delta log| < 0.995 otherwise, which truncates to 0 whatever the
    // rounding of log() -- and the sum (b) is formed once after the loop.  NaN / 0 / inf marginals fail both
    // comparisons and take the exact path.
    double pm[BV_SLOTS];
#pragma unroll
    for (int s = 0; s < BV_SLOTS; ++s) pm[s] = 1.0;
    int iters = 0;
    for (int k = 0; k <= 100; ++k) {
        double pf0 = 0., pf1 = 0., pf2 = 0., pf3 = 0., delta = 0.;
#pragma unroll
        for (int s = 0; s < BV_SLOTS; ++s) {
            if (s < nslots) {
                const int i = s * BV_WAVE + lane;
                if (i < B.nb) {
                    const int at = bv_bin_at(B, i);
                    const uint32_t code = B.code[at];
                    const double c = (double)B.cnt[at];
                    const uint32_t b = code >> 7;
                    const double hit = B.hit[code & 127u], miss = B.miss[code & 127u];
                    double L0 = (b == 0 ? hit : miss) * f[0];
                    double L1 = (b == 1 ? hit : miss) * f[1];
                    double L2 = (b == 2 ? hit : miss) * f[2];
                    double L3 = (b == 3 ? hit : miss) * f[3];
                    double marg = L0;
                    marg += L1;
                    marg += L2;
                    marg += L3;
                    double r = 1.0 / marg;
                    pf0 += c * (L0 * r);
                    pf1 += c * (L1 * r);
                    pf2 += c * (L2 * r);
                    pf3 += c * (L3 * r);
                    const double old = pm[s];
                    if (k > 0 && !(marg < old * 2.7 && marg > old * 0.37))
                        delta += c * bv_int_abs_trunc(log(marg) - log(old));
                    pm[s] = marg;
                }
            }
        }
        f[0] = bv_wave_sum(pf0) / n_cov;
        f[1] = bv_wave_sum(pf1) / n_cov;
        f[2] = bv_wave_sum(pf2) / n_cov;
        f[3] = bv_wave_sum(pf3) / n_cov;
        if (k == 0) continue;
        delta = bv_wave_sum(delta);
        ++iters;
        if (delta < epsilon) break;
    }
    *lr_out = bv_em_loglik(B, pm, nslots, lane);
    return iters;
}

// The same EM when no call of the site has phred 0 and the start frequencies are not all zero (every
// likelihood and marginal is then a positive finite number).  Bases outside the subset keep
// frequency +0.0 through every pass in the reference as well (0 * x, 0 + x, 0 / n are exact), so their
// terms are skipped rather than computed; the per-base sums of a pass are reduced together
// (bv_wave_sum2/4); the convergence sum is only formed when some bin took the exact-log path; and
// sum / n_cov is sum * (1 / n_cov) (<= 1 ulp; the parity bar is 1e-6).  `in_set`: bit b = base b.
__device__ __forceinline__ int bv_em_wave(const BvBins &B, double f[4], unsigned in_set, double n_cov, double *lr_out,
                                          int lane) {
    const double epsilon = (double)0.001f;
    const int nslots = (B.nb + BV_WAVE - 1) / BV_WAVE;
    const double inv_n = 1.0 / n_cov;
    const bool s0 = in_set & 1u, s1 = in_set & 2u, s2 = in_set & 4u, s3 = in_set & 8u;
    const int nset = __popc(in_set);
    double pm[BV_SLOTS];
#pragma unroll
    for (int s = 0; s < BV_SLOTS; ++s) pm[s] = 1.0;
    int iters = 0;
    for (int k = 0; k <= 100; ++k) {
        double pf0 = 0., pf1 = 0., pf2 = 0., pf3 = 0., delta = 0.;
#pragma unroll
        for (int s = 0; s < BV_SLOTS; ++s) {
            if (s < nslots) {
                const int i = s * BV_WAVE + lane;
                if (i < B.nb) {
                    const int at = bv_bin_at(B, i);
                    const uint32_t code = B.code[at];
                    const double c = (double)B.cnt[at];
                    const uint32_t b = code >> 7;
                    const double hit = B.hit[code & 127u], miss = B.miss[code & 127u];
                    double L0 = 0., L1 = 0., L2 = 0., L3 = 0., marg = 0.;
                    if (s0) { L0 = (b == 0 ? hit : miss) * f[0]; marg += L0; }
                    if (s1) { L1 = (b == 1 ? hit : miss) * f[1]; marg += L1; }
                    if (s2) { L2 = (b == 2 ? hit : miss) * f[2]; marg += L2; }
                    if (s3) { L3 = (b == 3 ? hit : miss) * f[3]; marg += L3; }
                    const double r = c / marg;
                    if (s0) pf0 += L0 * r;
                    if (s1) pf1 += L1 * r;
                    if (s2) pf2 += L2 * r;
                    if (s3) pf3 += L3 * r;
                    const double old = pm[s];
                    if (k > 0 && !(marg < old * 2.7 && marg > old * 0.37))
                        delta += c * bv_int_abs_trunc(log(marg) - log(old));
                    pm[s] = marg;
                }
            }
        }
        if (nset == 1) {
            const double t = bv_wave_sum(s0 ? pf0 : (s1 ? pf1 : (s2 ? pf2 : pf3)));
            pf0 = pf1 = pf2 = pf3 = t;
        } else if (nset == 2) {
            // the two members, in base order
            const double x = s0 ? pf0 : (s1 ? pf1 : pf2);
            const double y = s3 ? pf3 : ((s2 && (s0 || s1)) ? pf2 : pf1);
            double tx, ty;
            bv_wave_sum2(x, y, tx, ty);
            pf0 = tx;                                  // only read when s0
            pf1 = s0 ? ty : tx;                        // s1: second member iff s0 is the first
            pf2 = (s0 || s1) ? ty : tx;                // s2: second member iff an earlier base is in the set
            pf3 = ty;                                  // s3 is always the second member
        } else {
            bv_wave_sum4(pf0, pf1, pf2, pf3, pf0, pf1, pf2, pf3);
        }
        f[0] = s0 ? pf0 * inv_n : 0.;
        f[1] = s1 ? pf1 * inv_n : 0.;
        f[2] = s2 ? pf2 * inv_n : 0.;
        f[3] = s3 ? pf3 * inv_n : 0.;
        if (k == 0) continue;
        ++iters;
        if (__ballot(delta != 0.) == 0ull) break;  // every bin's log-marginal moved by < 1: the sum is 0
        if (bv_wave_sum(delta) < epsilon) break;
    }
    *lr_out = bv_em_loglik(B, pm, nslots, lane);
    return iters;
}

// ------------------------------------------------------------------ shallow sites: the reference's own order
// A histogram cannot see the ORDER of the samples, and when two allele subsets have mathematically equal likelihood
// (two bases seen once each at the same phred ...) the reference's pick depends on it: its log-likelihood is a
// sequential sum of per-sample terms (algorithm.h:24-41, basetype.cpp:123).  All such ties sit at shallow sites, so
// sites with at most BV_ORD_MAX covered samples replay the reference literally: the covered cells are gathered in
// sample order, one sample per lane, e_step / m_step as algorithm.h:148-198 (per-sample products, the marginal summed
// over A, C, G, T in that order, four IEEE divisions, the m_step's sums taken over the samples in order, no fused
// multiply-add), the convergence term and the final sum in sample order, and log() as the host's libm computes it
// (bv_log_host; the device library's log only when the engine could not verify the host's table).
#define BV_ORD_MAX 64
// An ordered-cell buffer in LDS: BV_ORD_MAX cells (uint16_t) followed by the scratch of bv_em_ordered's in-order sums
// (BV_SEQ_N quantities x BV_SEQ_STRIDE doubles); declare it `alignas(8) uint16_t ord[BV_ORD_ALLOC]`.
#define BV_SEQ_N 5
#define BV_SEQ_STRIDE 65 /* 64 + 1: the BV_SEQ_N lanes that walk the rows read different banks */
#define BV_ORD_ALLOC (BV_ORD_MAX + 4 * BV_SEQ_N * BV_SEQ_STRIDE)

// covered cells of one row in sample order -> ord[] (at most BV_ORD_MAX); returns how many the row holds.  With `gid`:
// only the samples of pop-group `g` (gid: one byte per sample, readable in 16-byte chunks up to the row's last chunk).
__device__ __noinline__ uint32_t bv_gather_ordered(const uint8_t *bs_row, const uint8_t *q_row, uint32_t n_samples, uint16_t *ord,
                                                  int lane, const uint8_t *gid = nullptr, uint32_t g = 0) {
    const uint32_t n_chunks = (n_samples + 15u) >> 4;
    uint32_t count = 0;
    // a round is 64 chunks of 16 cells, one per lane: calls, phreds (and group ids) as 16-byte loads, the next round's issued
    // before this round's cells are placed -- the walk is one wave's, its latency is the whole cost
    bv_u32x4 nb_ = bv_u32x4{0x08080808u, 0x08080808u, 0x08080808u, 0x08080808u}, nq_ = bv_u32x4{0u, 0u, 0u, 0u}, ng_ = bv_u32x4{0u, 0u, 0u, 0u};
    auto fetch = [&](uint32_t c0) {
        const uint32_t chunk = c0 + (uint32_t)lane;
        nb_ = bv_u32x4{0x08080808u, 0x08080808u, 0x08080808u, 0x08080808u};
        if (chunk < n_chunks) {
            nb_ = *reinterpret_cast<const bv_u32x4 *>(bs_row + (size_t)chunk * 16u);
            nq_ = *reinterpret_cast<const bv_u32x4 *>(q_row + (size_t)chunk * 16u);
            if (gid) ng_ = *reinterpret_cast<const bv_u32x4 *>(gid + (size_t)chunk * 16u);
        }
    };
    fetch(0);
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += BV_WAVE) {
        const uint32_t chunk = c0 + (uint32_t)lane;
        const bv_u32x4 vb = nb_, vq = nq_, vg = ng_;
        if (c0 + BV_WAVE < n_chunks) fetch(c0 + BV_WAVE);
        uint32_t mask = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t wbk = (k >> 2) == 0 ? vb.x : (k >> 2) == 1 ? vb.y : (k >> 2) == 2 ? vb.z : vb.w;
            const uint32_t wgk = (k >> 2) == 0 ? vg.x : (k >> 2) == 1 ? vg.y : (k >> 2) == 2 ? vg.z : vg.w;
            const uint32_t c = (wbk >> (8 * (k & 3))) & 0xFFu;
            const bool mine = !gid || ((wgk >> (8 * (k & 3))) & 0xFFu) == g;
            if (c < 8u && mine && chunk * 16u + (uint32_t)k < n_samples) mask |= 1u << k;
        }
        const uint32_t cnt = (uint32_t)__popc(mask);
        const uint32_t incl = bv_wave_incl_scan_u32(cnt);
        uint32_t pos = count + incl - cnt;
        while (mask) {
            const int k = __builtin_ctz(mask);
            mask &= mask - 1u;
            if (pos < (uint32_t)BV_ORD_MAX) {
                const int wi = k >> 2, sh8 = 8 * (k & 3);
                const uint32_t wbk = wi == 0 ? vb.x : wi == 1 ? vb.y : wi == 2 ? vb.z : vb.w;
                const uint32_t wqk = wi == 0 ? vq.x : wi == 1 ? vq.y : wi == 2 ? vq.z : vq.w;
                ord[pos] = (uint16_t)((((wbk >> sh8) & 0xFFu) << 8) | ((wqk >> sh8) & 0xFFu));
            }
            ++pos;
        }
        count += (uint32_t)bv_readlane63_i32((int)incl);
    }
    return count;
}

// EM, algorithm.h:210-255, literally, on n <= BV_ORD_MAX samples (lane i = sample i).  f: initial freqs in, final out.
// hipcc contracts a * b + c into fused multiply-adds (-ffp-contract=fast: across statements, pragmas ignored) and
// __dmul_rn / __dadd_rn are plain * and + in its headers; the reference's marginal (algorithm.h:164-165) is a sum of
// ROUNDED products, so every product passes through an empty asm statement before it is added.
__device__ __noinline__ int bv_em_ordered(const uint16_t *ord, int n, const double *hit, const double *miss, double f[4],
                                          double *lr_out, int lane, const double *hostlog) {
    const double epsilon = (double)0.001f;
    const bool have = lane < n;
    const uint32_t w = have ? ord[lane] : 0u;
    const uint32_t b = (w >> 8) & 3u, qi = min(w & 0xFFu, 127u);
    const double hv = hit[qi], mv = miss[qi];
    const double lh0 = b == 0 ? hv : mv, lh1 = b == 1 ? hv : mv, lh2 = b == 2 ? hv : mv, lh3 = b == 3 ? hv : mv;
    double p0 = 0., p1 = 0., p2 = 0., p3 = 0., marg = 1.;
    auto e_step = [&]() {  // algorithm.h:161-171
        double L0 = __dmul_rn(lh0, f[0]), L1 = __dmul_rn(lh1, f[1]), L2 = __dmul_rn(lh2, f[2]), L3 = __dmul_rn(lh3, f[3]);
        asm volatile("" : "+v"(L0), "+v"(L1), "+v"(L2), "+v"(L3));  // rounded products: not to be fused into the sum
        marg = __dadd_rn(__dadd_rn(__dadd_rn(L0, L1), L2), L3);
        p0 = __ddiv_rn(L0, marg); p1 = __ddiv_rn(L1, marg); p2 = __ddiv_rn(L2, marg); p3 = __ddiv_rn(L3, marg);
    };
    // Sums over the samples IN SAMPLE ORDER, from 0.0 (algorithm.h:190-193, :29-33), of up to BV_SEQ_N quantities at once:
    // every lane parks its values in LDS, then lane k alone adds quantity k of samples 0 .. n-1 one after the other (the
    // loads do not depend on the running sum, so they pipeline; the k chains run side by side).  A loop of v_readlane +
    // add per quantity took five times the instructions, all of them on the critical path.
    typedef __attribute__((address_space(3))) double bv_lds_f64;
    bv_lds_f64 *seq = (bv_lds_f64 *)reinterpret_cast<double *>(const_cast<uint16_t *>(ord) + BV_ORD_MAX);  // `ord` is LDS
    double sums[BV_SEQ_N];
    auto wave_fence = [&]() {  // LDS operations of one wave execute in order: only the compiler has to be held back
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    auto seq_sums = [&](const double (&v)[BV_SEQ_N], int nq) {
#pragma unroll
        for (int k = 0; k < BV_SEQ_N; ++k)
            if (k < nq) seq[k * BV_SEQ_STRIDE + lane] = v[k];
        wave_fence();
        double acc = 0.;
        if (lane < nq) {
            const bv_lds_f64 *row = seq + lane * BV_SEQ_STRIDE;
            for (int i = 0; i < n; ++i) acc = __dadd_rn(acc, row[i]);
        }
#pragma unroll
        for (int k = 0; k < BV_SEQ_N; ++k) sums[k] = (k < nq) ? bv_readlane_f64(acc, k) : 0.;
        wave_fence();
    };
    const double dn = (double)n;
    auto ln = [&](double v) { return hostlog ? bv_log_host(v, hostlog) : log(v); };  // algorithm.h:243
    e_step();
    double llh = ln(marg);
    {
        const double v[BV_SEQ_N] = {p0, p1, p2, p3, 0.};
        seq_sums(v, 4);  // m_step, algorithm.h:184-198
        f[0] = __ddiv_rn(sums[0], dn); f[1] = __ddiv_rn(sums[1], dn); f[2] = __ddiv_rn(sums[2], dn); f[3] = __ddiv_rn(sums[3], dn);
    }
    int iters = 0;
    for (int it = 0; it < 100; ++it) {
        e_step();
        const double now = ln(marg);
        const double d = have ? bv_int_abs_trunc(now - llh) : 0.;
        llh = now;
        const double v[BV_SEQ_N] = {p0, p1, p2, p3, d};
        seq_sums(v, 5);  // the m_step's four sums and the convergence term, one walk
        f[0] = __ddiv_rn(sums[0], dn); f[1] = __ddiv_rn(sums[1], dn); f[2] = __ddiv_rn(sums[2], dn); f[3] = __ddiv_rn(sums[3], dn);
        ++iters;
        if (sums[4] < epsilon) break;
    }
    {
        const double v[BV_SEQ_N] = {have ? llh : 0., 0., 0., 0., 0.};
        seq_sums(v, 1);
    }
    *lr_out = sums[0];
    return iters;
}
