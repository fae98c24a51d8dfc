// bv_lrt.h -- BaseType::lrt over the wave EMs: the LRT's shared scratch and result, the team barrier, bv_lrt.
// Included by bv_device.h, behind bv_em.h.
#pragma once

// ------------------------------------------------------------------ LRT
// BaseType::lrt + _f, src/basetype.cpp:105-199.  The EM runs of one level (the n-subsets of
// the current active set, Combinations order: external/combinations.h:55-69) are independent.
//   NW >= 1: "team mode" -- the runs of a level are dealt to NW cooperating waves of a workgroup (NOT necessarily all of
//            its waves: no s_barrier); results meet in LDS behind a counting barrier in `sh` (which must then be a
//            BvLrtTeamShared shared by the team), every wave replays the cheap, uniform argmin / threshold decision.
//            Each run is the same one-wave arithmetic as in wave mode, so the outcome is bit-identical to it.
//            (Used at the tail of a long-row launch, bv_pass1_team.h: the idle tally waves join the solver wave.)
//   NW == 0: "wave mode"  -- the calling wave does every run itself (used for the pop-group
//            calls of pass 2, where each wave owns a different group); `sh` is wave-private.
struct BvLrtShared {
    double f[2][4][4];  // [level parity][combination][base]
    double lr[2][4];
    int iters[2][4];
    double single[4];   // closed-form log-likelihoods of the four single-base subsets (wave mode; kept here, not in
                        // registers: the solver runs at the 128-VGPR limit)
};

struct BvLrtOut {
    int n_alt;
    int alt_packed;  // alt base k in bits [2k, 2k+1], reference order
    double af[4];    // only ever indexed with compile-time constants (registers, no scratch)
    int m;           // final active-set size
    int first;       // active_bases[0]
    double chi2;     // last chi_sqrt_value
    int em_iters, n_em;
    bool zero_freq;
    bool tie_risk;   // bv_lrt_g16<true> only: two subsets of one level scored within BV_TIE_TOL of each other (see there)
};
__device__ __forceinline__ int bv_alt_at(const BvLrtOut &o, int k) { return (o.alt_packed >> (2 * k)) & 3; }

// 4-entry register files addressed by a run-time base code without touching scratch
__device__ __forceinline__ double bv_sel4(double v0, double v1, double v2, double v3, int i) {
    return i == 0 ? v0 : (i == 1 ? v1 : (i == 2 ? v2 : v3));
}
__device__ __forceinline__ uint32_t bv_sel4u(const uint32_t v[4], int i) {
    return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}

template <int NW>
__device__ __forceinline__ void bv_lrt_sync() {
    static_assert(NW == 0, "team mode synchronises through bv_team_barrier");
    // same wave writes (lane 0) then reads (all lanes): LDS is in-order per wave; just
    // stop the compiler from moving the accesses across this point
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Team mode: the LRT scratch plus a counting barrier for the NW waves of the team.  `bar` counts arrivals since the
// team's owner last zeroed it (before it hands out a site); every spin is bounded like the kernel's other hand-offs.
struct BvLrtTeamShared {
    BvLrtShared lrt;  // first member: bv_lrt() receives &team->lrt
    uint32_t bar;
    uint32_t *err;    // a.counters + BV_CTR_TIMEOUT
};
__device__ __forceinline__ void bv_team_barrier(BvLrtShared *sh, uint32_t target, int lane) {
    BvLrtTeamShared *t = reinterpret_cast<BvLrtTeamShared *>(sh);
    // one arrival per wave; its earlier LDS writes are ahead of the atomic in the wave's in-order LDS queue
    if (lane == 0) __hip_atomic_fetch_add(&t->bar, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    uint32_t spins = 0;
    while (__hip_atomic_load(&t->bar, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1u << 24)) {
            atomicOr(t->err, 0x10000000u);  // BV_TMO_RING (bv_kernels.h)
            break;
        }
    }
}

// [toupper(REF)] + alts (caller.cpp:750-753), the list a pop-group's LRT starts from, as bv_lrt / bv_lrt_g16 take it: 3 bits per
// entry, `nc` entries.  ref: the reference base, clamped to 4; n_alt, alt: the site record's.
__device__ __forceinline__ int bv_lrt_ref_alts(int ref, int n_alt, const uint8_t *alt, int &nc) {
    int comb = ref;
    nc = 1;
#pragma unroll
    for (int k = 0; k < BV_MAX_ALT; ++k) {
        if (k < n_alt) {
            comb |= (alt[k] & 3) << (3 * nc);
            ++nc;
        }
    }
    return comb;
}

// `specific_packed`: the candidate bases in reference order, 3 bits each (value 4 = a base
// that is not ACGT, never active); `nspec` of them.
template <int NW>
__device__ inline void bv_lrt(const BvBins &B, const uint32_t depth[4], uint32_t total, int specific_packed,
                              int nspec, int ref_code, double min_af, BvLrtShared *sh, int wave, int lane,
                              BvLrtOut &o, uint32_t q0_mask = 0xFu) {
    o.n_alt = 0; o.alt_packed = 0; o.af[0] = o.af[1] = o.af[2] = o.af[3] = 0.;
    o.m = 0; o.first = 0; o.chi2 = 0.; o.em_iters = 0; o.n_em = 0; o.zero_freq = false; o.tie_risk = false;
    // active_bases as a packed ordered list: position k in bits [2k, 2k+1]
    int act = 0, m = 0;
    for (int k = 0; k < nspec; ++k) {
        int b = (specific_packed >> (3 * k)) & 7;
        if (b < 4 && (double)bv_sel4u(depth, b) / (int)total >= min_af) {  // basetype.cpp:137
            act |= b << (2 * m);
            ++m;
        }
    }
    if (m == 0) return;
    if (m == 1 && !((q0_mask >> (act & 3)) & 1u)) {
        // One active base b and none of its calls has phred 0.  The reference's EM is then exact
        // and needs no arithmetic: every row's posterior for b is L_b / L_b == 1.0, the m_step
        // gives f_b == n/n == 1.0, the first delta is |int(-log(f_init))| == 0 because
        // f_init > 1 - 3*min_af, so the loop stops after one iteration; there is no smaller subset
        // to test (chi stays 0, basetype.cpp:146-151) and the log-likelihood sum is never read.
        const int b = act & 3;
        o.m = 1; o.first = b; o.chi2 = 0.; o.em_iters = 1; o.n_em = 1;
        if (b != ref_code) { o.n_alt = 1; o.alt_packed = b; o.af[0] = 1.0; }
        return;
    }
    const double n_cov = (double)total;
    const int m0 = m;
    const int first_c = (NW > 0) ? wave : 0, step_c = (NW > 0) ? NW : 1;
    // initial frequency of every base, depth/total (basetype.cpp:99)
    const double d0 = (double)depth[0] / n_cov, d1 = (double)depth[1] / n_cov, d2 = (double)depth[2] / n_cov,
                 d3 = (double)depth[3] / n_cov;

    double fr0 = 0., fr1 = 0., fr2 = 0., fr3 = 0.;  // active_bases_freq
    double lr_alt = 0., chi = 0.;
    bool have_single = false;  // sh->single[] holds the closed-form log-likelihoods of the single-base subsets
    int par = 0;
    uint32_t team_epoch = 0;  // team mode: barriers passed for this site
    // n == m0: F_m over the full active set (basetype.cpp:144); n < m0: the loop of :151-169,
    // whose bound is the ORIGINAL size while the subsets are drawn from the current set.
    for (int n = m0; n > 0; --n) {
        const bool top = (n == m0);
        const int ncomb = top ? 1 : m;  // the m subsets of size m-1; subset c drops position m-1-c
        for (int c = first_c; c < ncomb; c += step_c) {
            const int drop = top ? -1 : m - 1 - c;
            unsigned in_set = 0;  // bit b set <=> base b is in this subset
            for (int k = 0; k < m; ++k)
                if (k != drop) in_set |= 1u << ((act >> (2 * k)) & 3);
            double f[4];
            f[0] = (in_set & 1u) ? d0 : 0.;
            f[1] = (in_set & 2u) ? d1 : 0.;
            f[2] = (in_set & 4u) ? d2 : 0.;
            f[3] = (in_set & 8u) ? d3 : 0.;
            double s = 0.;
            s += f[0]; s += f[1]; s += f[2]; s += f[3];
            double lr;
            int it;
            if (B.ord != nullptr && s != 0.) {
                // (copies for the call: bv_em_ordered is not inlined, and an array whose address leaves the function lives in
                // scratch memory -- with f and lr handed over themselves, EVERY subset of every site paid memory trips for them,
                // also in the kernels that never replay)
                double fo[4] = {f[0], f[1], f[2], f[3]}, lro;
                it = bv_em_ordered(B.ord, B.n_ord, B.hit, B.miss, fo, &lro, lane, bv_hostlog_of(B.logmiss));
                f[0] = fo[0]; f[1] = fo[1]; f[2] = fo[2]; f[3] = fo[3];
                lr = lro;
            } else if (B.loghit != nullptr && q0_mask == 0u && s != 0. && (in_set & (in_set - 1u)) == 0u) {
                // A single-base subset {b} with every likelihood positive: the reference's EM needs no arithmetic.  Its
                // first e_step gives every sample the posterior L/L == 1.0 for b, the m_step f_b == n/n == 1.0, and from
                // then on every marginal is the likelihood itself (lh * 1.0), so the reported log-likelihood is
                //     sum_i log(lh_i[b]) = sum_bins c * (bin's base == b ? log(1 - eps_q) : log(eps_q / 3))
                // with the host's log() of the host's table values -- the reference's own per-sample terms.  One sweep
                // yields the sums of all four bases: lr_b = sum c * logmiss + sum_{bins of b} c * (loghit - logmiss).
                // The loop runs twice when the start frequency is below 1/e (the first delta is |int(-log f_init)|
                // per sample, algorithm.h:245), else once.
                if (!have_single) {
                    double a_ = 0., g0 = 0., g1 = 0., g2 = 0., g3 = 0.;
                    const int nslots = (B.nb + BV_WAVE - 1) / BV_WAVE;
#pragma unroll
                    for (int sl = 0; sl < BV_SLOTS; ++sl) {
                        if (sl < nslots) {
                            const int i = sl * BV_WAVE + lane;
                            if (i < B.nb) {
                                const int at = bv_bin_at(B, i);
                                const uint32_t code = B.code[at];
                                const double cc = (double)B.cnt[at];
                                const double lm = B.logmiss[code & 127u], dh = B.loghit[code & 127u] - lm;
                                const uint32_t bb = code >> 7;
                                a_ += cc * lm;
                                g0 += (bb == 0) ? cc * dh : 0.;
                                g1 += (bb == 1) ? cc * dh : 0.;
                                g2 += (bb == 2) ? cc * dh : 0.;
                                g3 += (bb == 3) ? cc * dh : 0.;
                            }
                        }
                    }
                    a_ = bv_wave_sum(a_);
                    bv_wave_sum4(g0, g1, g2, g3, g0, g1, g2, g3);
                    // (team mode: every wave that meets a single-base subset computes the four sums itself and reads back
                    // its own stores -- the other waves write the same values -- so no team barrier is needed here)
                    if (lane == 0) {
                        sh->single[0] = a_ + g0; sh->single[1] = a_ + g1;
                        sh->single[2] = a_ + g2; sh->single[3] = a_ + g3;
                    }
                    bv_lrt_sync<0>();
                    have_single = true;
                }
                const int b1 = __builtin_ctz(in_set);
                lr = sh->single[b1];
                const double f_init = bv_sel4(f[0], f[1], f[2], f[3], b1);
                it = (f_init < 0.36787944117144233) ? 2 : 1;
                f[0] = (b1 == 0) ? 1.0 : 0.; f[1] = (b1 == 1) ? 1.0 : 0.;
                f[2] = (b1 == 2) ? 1.0 : 0.; f[3] = (b1 == 3) ? 1.0 : 0.;
            } else {
                // phred-0 calls (1 - eps == 0) and all-zero starts make 0/0 in the reference: exact replay
                it = (q0_mask != 0u || s == 0.) ? bv_em_wave_generic(B, f, n_cov, &lr, lane)
                                                : bv_em_wave(B, f, in_set, n_cov, &lr, lane);
            }
            if (lane == 0) {
                sh->f[par][c][0] = f[0]; sh->f[par][c][1] = f[1];
                sh->f[par][c][2] = f[2]; sh->f[par][c][3] = f[3];
                sh->lr[par][c] = lr;
                sh->iters[par][c] = (s == 0.) ? -it - 1 : it;  // negative marks basetype.cpp:113-115
            }
        }
        if (NW > 0) bv_team_barrier(sh, (uint32_t)NW * (++team_epoch), lane);
        else bv_lrt_sync<0>();
        int i_min = 0;
        double chi_min = 0.;
        for (int c = 0; c < ncomb; ++c) {
            int it = sh->iters[par][c];
            if (it < 0) { o.zero_freq = true; it = -it - 1; }
            o.em_iters += it;
            o.n_em += 1;
            if (!top) {
                double v = 2 * (lr_alt - sh->lr[par][c]);
                if (c == 0 || v < chi_min) { chi_min = v; i_min = c; }  // first minimum, algorithm.h:24-27
            }
        }
        lr_alt = sh->lr[par][i_min];
        bool accept = top;
        if (!top) {
            chi = chi_min;
            accept = chi < 24;  // LRT_THRESHOLD, basetype.h:21
            if (accept) {
                const int drop = m - 1 - i_min;
                const int low = act & ((1 << (2 * drop)) - 1), high = act >> (2 * drop + 2);
                act = low | (high << (2 * drop));
                m = n;
            }
        }
        if (!accept) break;
        fr0 = sh->f[par][i_min][0]; fr1 = sh->f[par][i_min][1];
        fr2 = sh->f[par][i_min][2]; fr3 = sh->f[par][i_min][3];
        par ^= 1;
    }
    o.chi2 = chi;
    o.m = m;
    o.first = act & 3;
    double af0 = 0., af1 = 0., af2 = 0., af3 = 0.;
    int na = 0, packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < m) {
            const int b = (act >> (2 * k)) & 3;
            if (b != ref_code) {  // basetype.cpp:172-177
                const double v = bv_sel4(fr0, fr1, fr2, fr3, b);
                if (na == 0) af0 = v; else if (na == 1) af1 = v; else if (na == 2) af2 = v; else af3 = v;
                packed |= b << (2 * na);
                ++na;
            }
        }
    }
    o.n_alt = na;
    o.alt_packed = packed;
    o.af[0] = af0; o.af[1] = af1; o.af[2] = af2; o.af[3] = af3;
}
