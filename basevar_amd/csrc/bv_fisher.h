// bv_fisher.h -- kt_fisher_exact (two-sided) and the strand-bias tail around it, in the library's three forms: one family on
// the 64 lanes of a wave, one on the 16 lanes of a row (the 16-lane solver), one per lane (the reference's literal walk).
// Included by bv_device.h, behind bv_wave.h (the cross-lane primitives) and bv_kfunc.h (BvLnTab, bv_lnfact).
// BV_LNFACT_TABLE_ONLY, where a translation unit sets it, is defined before its first include.
#pragma once

// ------------------------------------------------------------------ Fisher exact test
// kt_fisher_exact (two-sided), htslib/kfunc.c:197-313, lane-parallel (the wave and the 16-lane form).
//
// The reference walks the hypergeometric pmf from both ends towards the observed table,
// updating p(i) multiplicatively and re-seeding it from lgamma() every 11 tables
// (hypergeo_acc, kfunc.c:220-243).  Here every table probability is evaluated on its own,
// one table per lane, from log-factorials:
//   p(i) = exp( lbinom(n1_, i) + lbinom(n - n1_, n_1 - i) - lbinom(n, n_1) )   (kfunc.c:197-212)
// log(n!) == lgamma(n + 1) is the only way kfunc.c:197-201 uses lgamma; the engine keeps a table of
// it in HBM (L2-resident), filled on the host with glibc's lgamma -- the reference's own values --
// for every n up to the largest possible depth.  Arguments beyond the table fall back to the
// Stirling series (7 terms, |error| < 1e-16 relative for n + 1 >= 17).  Values differ from the
// reference's multiplicative walk at the 1e-13 relative level (parity bar: 1e-6).

// One 2x2 table family: margins fixed, n11 = i varies over [imin, imax].
// lbinom(n, k) = lnfact(n) - lnfact(k) - lnfact(n - k); its k == 0 / k == n special case
// (kfunc.c:199) needs no branch here because lnfact(0) == 0 makes the difference exactly 0.
struct BvHyper {
    BvLnTab T;
    int n1_, n_1, n, n22off;
    double lf_n1;   // lnfact(n1_)
    double lf_n2;   // lnfact(n - n1_)
    double lb3;     // lbinom(n, n_1)
};
__device__ __forceinline__ double bv_hyper_logp(const BvHyper &h, int i) {
    double a = h.lf_n1 - bv_lnfact(h.T, i) - bv_lnfact(h.T, h.n1_ - i);
    double b = h.lf_n2 - bv_lnfact(h.T, h.n_1 - i) - bv_lnfact(h.T, i + h.n22off);
    return a + b - h.lb3;
}
__device__ __forceinline__ double bv_hyper_p(const BvHyper &h, int i) { return exp(bv_hyper_logp(h, i)); }
// p(i + 1) / p(i): the multiplicative step of the reference's own walk (hypergeo_acc, kfunc.c:226-231)
__device__ __forceinline__ double bv_hyper_ratio(const BvHyper &h, int i) {
    return ((double)(h.n1_ - i) * (double)(h.n_1 - i)) / ((double)(i + 1) * (double)(i + 1 + h.n22off));
}
__device__ __forceinline__ void bv_hyper_init(BvHyper &h, const BvLnTab &T, int n1_, int n_1, int n) {
    h.T = T;
    h.n1_ = n1_; h.n_1 = n_1; h.n = n; h.n22off = n - n1_ - n_1;
    h.lf_n1 = bv_lnfact(T, n1_);
    h.lf_n2 = bv_lnfact(T, n - n1_);
    h.lb3 = bv_lnfact(T, n) - bv_lnfact(T, n_1) - bv_lnfact(T, n - n_1);
}

// Tables of a family whose observed table has q < 2^-511 are carried scaled by 2^512: the walks below start where a tail
// falls under q * e^-60, and unscaled that first table's exp() is 0 from q ~ 1e-298 on -- a product of ratios that starts at 0
// stays 0 while the true terms rise past q.  Scaled, every table of at least q * e^-60 is a normal double (q >= 2^-1074 here,
// no table exceeds 1: nothing overflows); the two-sided sum is scaled back by the exact power of two.
#define BV_FISHER_SHIFT_LOG (-354.0)              /* just above ln 2^-511                */
#define BV_FISHER_SHIFT 354.89135644669199        /* 512 ln 2                            */
__device__ __forceinline__ double bv_fisher_shift(double logq) { return logq < BV_FISHER_SHIFT_LOG ? BV_FISHER_SHIFT : 0.; }
__device__ __forceinline__ double bv_fisher_unshift(double two, double shift) { return shift != 0. ? two * 0x1p-512 : two; }
// The same zero threatens wherever a walk STARTS below the double range and rises: the first table of a family with a steep end
// (log p(imin) of -1000 beside an ordinary q), the start of a tail window when one probe step spans hundreds of nats.  A walk
// whose first table has log p + shift < BV_FISHER_LIVE starts at the first table that reaches it instead: found by bisection
// on [lo, hi], hi at most the family's mode, over which log p rises.  The tables passed over are below 1e-304 of the scale on
// which q is at least 1e-169: nothing to a sum that is at least q.  (A walk that FALLS below the range may go to 0: so do its terms.)
#define BV_FISHER_LIVE (-700.0)
__device__ __forceinline__ int bv_fisher_mode(int n1_, int n_1, int n) {
    return (int)(((long long)(n1_ + 1) * (long long)(n_1 + 1)) / (long long)(n + 2));
}
__device__ inline int bv_fisher_first_live(const BvHyper &h, int lo, int hi, double shift) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (bv_hyper_logp(h, mid) + shift >= BV_FISHER_LIVE) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// kt_fisher_exact (two-sided), on the lanes of a group.  Semantics of the reference's two loops
// (kfunc.c:291-307): with lo = 0.99999999 q and hi = 1.00000001 q,
//   L* = first table from the left  with p >= lo,  left  = sum_{i < L*} p(i) + (p(L*) < hi ? p(L*) : 0)
//   R* = first table from the right with p >= lo,  right = sum_{i > R*} p(i) + (p(R*) < hi ? p(R*) : 0)
//   two = min(1, left + right)
// The pmf is unimodal, so the tables with p < lo are exactly those left of L* and right of R*:
//   two = sum_{p(i) < lo} p(i) + [p(L*) < hi] p(L*) + [p(R*) < hi] p(R*),
// with L* / R* the lowest / highest lane of a ballot.
// Regimes:
//   a row margin <= 12   product form, no log-factorials (the usual all-sites CVG case): the frame, bv_fisher_two_sided;
//   more tables          the group's walk, bv_fisher_walk: rounds of 64 tables with a prefix product on a wave, one block of
//                        tables per lane on a row -- they differ by design, each says why.  Beyond 256 (128) tables a probe of
//                        log p on either side first skips the far tails (bv_fisher_skip_tails).

// The lanes that share one table family: the whole wave, or one row of 16 (the 16-lane solver: control flow may diverge between the
// rows of a wave, so only row-local operations there).  idx: my place in the group; sum / sum16: a value summed over the group /
// over its first 16 lanes, known to every lane; ballot: the group's lanes as a mask, first / last: its lowest / highest set bit;
// bcast: the value held by lane k of the group; PROBES: the steps between the probe points of a tail, one point per lane.
struct BvWaveLanes {
    typedef unsigned long long Mask;
    static constexpr int PROBES = BV_WAVE - 1;
    static __device__ __forceinline__ int idx(int lane) { return lane; }
    static __device__ __forceinline__ double sum(double v) { return bv_wave_sum(v); }
    static __device__ __forceinline__ double sum16(double v) { BV_ROW_SCAN(v, BV_OP_ADD, BV_MV_F64); return bv_readlane_f64(v, 15); }
    static __device__ __forceinline__ Mask ballot(bool pred, int) { return __ballot(pred); }
    static __device__ __forceinline__ int first(Mask m) { return (int)__builtin_ctzll(m); }
    static __device__ __forceinline__ int last(Mask m) { return 63 - (int)__builtin_clzll(m); }
    static __device__ __forceinline__ double bcast(double v, int k, int) { return bv_readlane_f64(v, k); }
    static __device__ __forceinline__ int max_i32(int v) { return bv_wave_max_i32(v); }
    static __device__ __forceinline__ int min_i32(int v) { return bv_wave_min_i32(v); }
};
struct BvRowLanes {
    typedef uint32_t Mask;
    static constexpr int PROBES = 15;
    static __device__ __forceinline__ int idx(int lane) { return lane & 15; }
    static __device__ __forceinline__ double sum(double v) { return bv_g16_sum(v); }
    static __device__ __forceinline__ double sum16(double v) { return bv_g16_sum(v); }
    static __device__ __forceinline__ Mask ballot(bool pred, int lane) { return bv_g16_ballot(pred, lane); }
    static __device__ __forceinline__ int first(Mask m) { return __builtin_ctz(m); }
    static __device__ __forceinline__ int last(Mask m) { return 31 - __builtin_clz(m); }
    static __device__ __forceinline__ double bcast(double v, int k, int lane) { return bv_g16_bcast_f64(v, k, lane); }
    static __device__ __forceinline__ int max_i32(int v) { return bv_g16_max_i32(v); }
    static __device__ __forceinline__ int min_i32(int v) { return bv_g16_min_i32(v); }
};

// the end of every form: the two boundary tables join the sum of the tables below lo if they are below hi (`ends`: there are any)
__device__ __forceinline__ double bv_fisher_close(double two, double pL, double pR, double hi, double shift, bool ends = true) {
    if (ends) {
        if (pL < hi) two += pL;
        if (pR < hi) two += pR;
    }
    two = bv_fisher_unshift(two, shift);
    return two > 1. ? 1. : two;
}
// The whole decision when each lane of the group holds at most one table (`have`: it holds one, of probability p) and q is
// the observed table's.  FIRST16: the tables sit in the group's first 16 lanes.
template <class G, bool FIRST16>
__device__ __forceinline__ double bv_fisher_decide(double p, bool have, double q, int lane) {
    const double lo = 0.99999999 * q, hi = 1.00000001 * q;
    const bool viol = have && !(p < lo);
    const typename G::Mask vm = G::ballot(viol, lane);  // never empty: the observed table is in it
    const double two = FIRST16 ? G::sum16(viol ? 0. : p) : G::sum(viol ? 0. : p);
    const double pL = G::bcast(p, G::first(vm), lane), pR = G::bcast(p, G::last(vm), lane);
    return bv_fisher_close(two, pL, pR, hi, 0.);
}
// Many tables: skip the far tails whose terms are below q * 2^-86 (they cannot change a double-precision sum that is >= q).  One
// probe of log p per lane on either side of the observed table; [wl, wr] comes back as what is left to walk.
template <class G>
__device__ __forceinline__ void bv_fisher_skip_tails(const BvHyper &h, int n11, int imin, int imax, double logq, int lane, int &wl,
                                                     int &wr) {
    const int INF = 0x7fffffff, gl = G::idx(lane);
    const double cut = logq - 60.0;  // exp(-60) ~ 2^-86.6
    {
        // probes on [imin, n11]: tables before the last probe that is still below the cut are negligible
        // (rising side, or between mode and n11 where p >= q): a prefix by unimodality
        const int span = n11 - imin, step = span / G::PROBES + 1;
        const int i = imin + gl * step;
        const bool below = (i <= n11) && (bv_hyper_logp(h, min(i, n11)) < cut);
        const int last = G::max_i32(below ? i : -1);
        if (last >= 0) wl = last;
    }
    {
        const int span = imax - n11, step = span / G::PROBES + 1;
        const int i = imax - gl * step;
        const bool below = (i >= n11) && (bv_hyper_logp(h, max(i, n11)) < cut);
        const int first = G::min_i32(below ? i : INF);
        if (first != INF) wr = first;
    }
}

// The walk of a wave: R <= 64 tables, one per lane; more, rounds of 64 tables over [imin, imax] (beyond 256, the tails skipped).
__device__ __forceinline__ double bv_fisher_walk(BvWaveLanes, const BvHyper &h, int n11, int imin, int imax, int lane) {
    const int R = imax - imin + 1;

    if (R <= BV_WAVE) {
        // ---- one table per lane; q is the value of the lane that holds the observed table
        const int i = imin + lane;
        const bool have = i <= imax;
        const double pe = bv_hyper_p(h, have ? i : imax);
        const double p = have ? pe : 0.;
        const double q = bv_readlane_f64(p, n11 - imin);
        if (q == 0.0) return 0.0;  // kfunc.c:260-289
        return bv_fisher_decide<BvWaveLanes, false>(p, have, q, lane);
    }

    const double logq = bv_hyper_logp(h, n11);
    if (exp(logq) == 0.0) return 0.0;  // kfunc.c:260-289
    // (scaled where q is tiny, see bv_fisher_shift: unscaled, pbase = exp(log p(wl)) was 0 for q below ~1e-298 and with it every
    // table of every round -- two came out 0, FS 10000; found by tests/test_gpu_strand_tables.py, "probed R=max q300")
    const double shift = bv_fisher_shift(logq);
    const double q = exp(logq + shift);
    const double lo = 0.99999999 * q, hi = 1.00000001 * q;
    int wl = imin, wr = imax;
    if (R > 4 * BV_WAVE) bv_fisher_skip_tails<BvWaveLanes>(h, n11, imin, imax, logq, lane, wl, wr);
    // ---- rounds of 64 tables, ascending over [wl, wr].  Only the first table of the range comes from log-factorials
    // (four table lookups + exp, an L2 round trip); the others follow by the reference's own multiplicative step
    // p(i+1) = p(i) * ratio(i), as prefix products across the lanes -- no memory access inside the loop.  (~1e-16 per
    // step; the reference re-seeds every 11 tables, which matters at 1e-13, not at the 1e-6 bar.)
    double tail = 0., pL = 0., pR = 0.;
    bool seen = false;
    double lbase = bv_hyper_logp(h, wl) + shift;
    if (lbase < BV_FISHER_LIVE) {  // (uniform over the wave; rare)
        const int top = min(wr, bv_fisher_mode(h.n1_, h.n_1, h.n));
        if (wl < top) {
            wl = bv_fisher_first_live(h, wl + 1, top, shift);
            lbase = bv_hyper_logp(h, wl) + shift;
        }
    }
    double pbase = exp(lbase);
    for (int w = wl; w <= wr; w += BV_WAVE) {
        const int i = w + lane;
        const bool have = i <= wr;
        const double step = (lane == 0 || !have) ? 1.0 : bv_hyper_ratio(h, i - 1);
        const double pe = pbase * bv_wave_incl_scan_prod_f64(step);
        pbase = bv_readlane_f64(pe, 63) * bv_hyper_ratio(h, w + 63);  // first table of the next round (unused after the last)
        const double p = have ? pe : 0.;
        const bool viol = have && !(p < lo);
        tail += viol ? 0. : p;
        const unsigned long long vm = __ballot(viol);
        if (vm != 0ull) {
            if (!seen) pL = bv_readlane_f64(p, (int)__builtin_ctzll(vm));
            seen = true;
            pR = bv_readlane_f64(p, 63 - (int)__builtin_clzll(vm));
        }
    }
    return bv_fisher_close(bv_wave_sum(tail), pL, pR, hi, shift);
}

// The walk of a row of 16 lanes (control flow may diverge between the rows of a wave: row-local operations only).
__device__ __forceinline__ double bv_fisher_walk(BvRowLanes, const BvHyper &h, int n11, int imin, int imax, int lane) {
    const int gl = lane & 15;
    const int R = imax - imin + 1;
    // Up to 128 tables (no tails to skip: the blocks below are those of [imin, imax]): the lane's seed table is known here,
    // and its four log-factorials travel with those of q instead of making a memory trip of their own after it.
    const bool narrow = R <= 8 * 16;
    const int i0n = imin + gl * ((R + 15) >> 4);
    double seed_n = (narrow && i0n <= imax) ? bv_hyper_logp(h, i0n) : 0.;
    asm volatile("" : "+v"(seed_n));  // (read here, not where it is used)
    const double logq = bv_hyper_logp(h, n11);
    if (exp(logq) == 0.0) return 0.0;  // kfunc.c:260-289
    // q below 2^-511: every table is carried scaled by 2^512 (BV_FISHER_SHIFT) and the sum scaled back at the end.
    // Unscaled, a block that starts at a table of q * e^-60 (where a probed tail ends) is seeded with exp() == 0 once q nears
    // the smallest double, and stays 0 while the true terms rise past q: the tail's sum was lost, and with it the observed
    // table when it lay in that block (found by tests/test_gpu_strand_tables.py, "probed R=max q300": p came out halved).
    const double shift = bv_fisher_shift(logq);
    const double q = exp(logq + shift);
    const double lo = 0.99999999 * q, hi = 1.00000001 * q;
    int wl = imin, wr = imax;
    if (!narrow) bv_fisher_skip_tails<BvRowLanes>(h, n11, imin, imax, logq, lane, wl, wr);
    // The tables of [wl, wr] in 16 consecutive blocks, one per lane: the lane seeds its first table from log-factorials and
    // walks its block with the multiplicative step of the reference's own walk (hypergeo_acc, kfunc.c:226-231) -- at most
    // ~25 steps from an exact seed (the reference re-seeds every 11).  Per table: one division and a few multiplies on ONE
    // lane, against a 16-lane prefix product, two broadcasts and a ballot per 16 tables in the round form this replaces
    // (the Fisher tests were 45 % of the solver's instructions).
    const int Lb = (wr - wl + 16) >> 4;  // tables per lane
    int i0 = wl + gl * Lb;
    const int i1 = min(i0 + Lb - 1, wr);
    const bool mine = i0 <= wr;
    double ls = (narrow ? seed_n : bv_hyper_logp(h, mine ? i0 : wr)) + shift;
    if (mine && ls < BV_FISHER_LIVE) {
        // a block that starts below the double range and rises (bv_fisher_first_live): it starts where its tables do
        const int top = min(i1, bv_fisher_mode(h.n1_, h.n_1, h.n));
        if (i0 < top) {
            i0 = bv_fisher_first_live(h, i0 + 1, top, shift);
            ls = bv_hyper_logp(h, i0) + shift;
        }
    }
    double p = mine ? exp(ls) : 0.;
    double tail = 0., pfirst = 0., plast = 0.;
    bool seen = false;
    for (int t = 0; t < Lb; ++t) {
        const int i = i0 + t;
        const bool in = mine && i <= i1;
        const bool viol = in && !(p < lo);
        tail += (in && !viol) ? p : 0.;
        if (viol && !seen) pfirst = p;
        if (viol) { plast = p; seen = true; }
        p *= bv_hyper_ratio(h, i);
    }
    const uint32_t vm = bv_g16_ballot(seen, lane);  // never empty: the observed table lies inside [wl, wr]
    const double two = bv_g16_sum(tail);
    const double pL = bv_g16_bcast_f64(pfirst, __builtin_ctz(vm | 0x10000u), lane);
    const double pR = bv_g16_bcast_f64(plast, 31 - __builtin_clz(vm | 1u), lane);
    return bv_fisher_close(two, pL, pR, hi, shift, vm != 0u);
}

// The frame: margins, the product form, else the group's walk.  `T`: the log-factorial table.
template <class G>
__device__ __forceinline__ double bv_fisher_two_sided(int n11, int n12, int n21, int n22, int lane, const BvLnTab &T) {
    const int n1_ = n11 + n12, n_1 = n11 + n21, n = n11 + n12 + n21 + n22;
    const int imax = (n_1 < n1_) ? n_1 : n1_;
    int imin = n1_ + n_1 - n;
    if (imin < 0) imin = 0;
    if (imin == imax) return 1.;
    {
        // ---- a row margin of at most 12 reads (the usual case for the all-sites CVG test: a hom-ref
        // site carries only a handful of non-reference reads).  With m = that row's total and j = how
        // many of them sit in column 1, the table probability is a ratio of two products of m terms
        //     p(j) = C(m, j) * (n_1)_j * (n_2)_{m-j} / (n)_m        ((x)_k: falling factorial)
        // -- exact to ~1e-15.  The tables are walked in j instead of n11; the two-sided sum is
        // symmetric under that relabelling.  At most 13 tables: they sit in the first 16 lanes of the group.
        const int n2_ = n21 + n22, n_2 = n - n_1;
        const bool alt_row = n2_ <= n1_;
        const int m = alt_row ? n2_ : n1_, jobs = alt_row ? n21 : n11;
        if (m <= 12) {
            const int jmin = max(0, m - n_2), jmax = min(m, n_1);  // jmin < jmax because imin < imax
            const int j = jmin + G::idx(lane);
            const bool have = j <= jmax;
            double pn = 1.0, pd = 1.0;
            for (int t = 0; t < m; ++t) {
                const double num = (t < j) ? (double)(n_1 - t) * (double)(m - t) : (double)(n_2 - (t - j));
                const double den = (t < j) ? (double)(n - t) * (double)(t + 1) : (double)(n - t);
                pn *= num;
                pd *= den;
            }
            const double p = have ? pn / pd : 0.;
            const double q = G::bcast(p, jobs - jmin, lane);
            if (q == 0.0) return 0.0;
            return bv_fisher_decide<G, true>(p, have, q, lane);
        }
    }
    BvHyper h;
    bv_hyper_init(h, T, n1_, n_1, n);
    return bv_fisher_walk(G(), h, n11, imin, imax, lane);
}
__device__ inline double bv_fisher_two_sided_wave(int n11, int n12, int n21, int n22, int lane, const BvLnTab &T) {
    return bv_fisher_two_sided<BvWaveLanes>(n11, n12, n21, n22, lane, T);
}
__device__ inline double bv_fisher_two_sided_g16(int n11, int n12, int n21, int n22, int lane, const BvLnTab &T) {
    return bv_fisher_two_sided<BvRowLanes>(n11, n12, n21, n22, lane, T);
}

// strand_bias tail, src/basetype.cpp:277-286: FS and SOR from the two-sided p of the strand table and its four counts
__device__ __forceinline__ void bv_strand_bias_tail(double two, uint32_t ref_fwd, uint32_t ref_rev, uint32_t alt_fwd, uint32_t alt_rev,
                                                    double *fs_out, double *sor_out, uint32_t *flags) {
    double fs = -10 * log10(two);
    if (isinf(fs)) fs = 10000;
    else if (fs == 0) fs = 0.0;
    // basetype.cpp:286 multiplies `int`s; past 2^31 that is UB in the reference.  Its compiled
    // form (gcc -O3 x86-64, pinned by tests/golden/deep_sor.npz and sor_wrap.npz) divides the 32-bit
    // wrapped products and folds the guard `ref_rev * alt_fwd > 0` into "the wrapped product is not
    // zero": a denominator that wraps negative is divided by, one that is a multiple of 2^32
    // (65536 x 65536, 524288 x 8192) gives 10000 -- "both factors non-zero" divided by 0 there (inf, nan).
    // Reproduced exactly, and flagged so that a caller can tell such a value is not meaningful.
    int den = (int)(ref_rev * alt_fwd), num = (int)(ref_fwd * alt_rev);
    if ((unsigned long long)ref_rev * alt_fwd > 0x7fffffffull || (unsigned long long)ref_fwd * alt_rev > 0x7fffffffull)
        *flags |= BV_SITE_SOR_OVERFLOW;
    double sor = (den != 0) ? (double)num / (double)den : 10000;
    *fs_out = fs;
    *sor_out = sor;
}
__device__ inline void bv_strand_bias_wave(uint32_t ref_fwd, uint32_t ref_rev, uint32_t alt_fwd, uint32_t alt_rev,
                                           int lane, const BvLnTab &T, double *fs_out, double *sor_out, uint32_t *flags) {
    bv_strand_bias_tail(bv_fisher_two_sided_wave((int)ref_fwd, (int)ref_rev, (int)alt_fwd, (int)alt_rev, lane, T), ref_fwd, ref_rev,
                        alt_fwd, alt_rev, fs_out, sor_out, flags);
}
__device__ inline void bv_strand_bias_g16(uint32_t ref_fwd, uint32_t ref_rev, uint32_t alt_fwd, uint32_t alt_rev, int lane,
                                          const BvLnTab &T, double *fs_out, double *sor_out, uint32_t *flags) {
    bv_strand_bias_tail(bv_fisher_two_sided_g16((int)ref_fwd, (int)ref_rev, (int)alt_fwd, (int)alt_rev, lane, T), ref_fwd, ref_rev,
                        alt_fwd, alt_rev, fs_out, sor_out, flags);
}

// ------------------------------------------------------------------------------ per-lane Fisher test
// kt_fisher_exact (two-sided), htslib/kfunc.c:245-313, one table family per LANE: the walk of kfunc.c:291-307 with its
// incremental hypergeo_acc (kfunc.c:220-243: multiplicative update, re-seeded from log-factorials whenever n11 % 11 == 0
// or the table's n22 is 0).  log(k!) comes from the engine's table of the host's lgamma (the reference's own values).
struct BvHgAcc {
    int n11, n1_, n_1, n;
    double p;
};
__device__ __forceinline__ double bv_lbinom_lane(const BvLnTab &T, int n, int k) {
    if (k == 0 || n == k) return 0;
    return bv_lnfact(T, n) - bv_lnfact(T, k) - bv_lnfact(T, n - k);
}
__device__ __forceinline__ double bv_hypergeo_lane(const BvLnTab &T, int n11, int n1_, int n_1, int n) {
    return exp(bv_lbinom_lane(T, n1_, n11) + bv_lbinom_lane(T, n - n1_, n_1 - n11) - bv_lbinom_lane(T, n, n_1));
}
__device__ __forceinline__ double bv_hgacc_step(const BvLnTab &T, int n11, BvHgAcc &x) {  // hypergeo_acc(n11, 0, 0, 0, aux)
    if (n11 % 11 && n11 + x.n - x.n1_ - x.n_1) {
        if (n11 == x.n11 + 1) {
            x.p *= (double)(x.n1_ - x.n11) / n11 * (x.n_1 - x.n11) / (n11 + x.n - x.n1_ - x.n_1);
            x.n11 = n11;
            return x.p;
        }
        if (n11 == x.n11 - 1) {
            x.p *= (double)x.n11 / (x.n1_ - n11) * (x.n11 + x.n - x.n1_ - x.n_1) / (x.n_1 - n11);
            x.n11 = n11;
            return x.p;
        }
    }
    x.n11 = n11;
    x.p = bv_hypergeo_lane(T, x.n11, x.n1_, x.n_1, x.n);
    return x.p;
}
__device__ inline double bv_fisher_two_sided_lane(int n11, int n12, int n21, int n22, const BvLnTab &T) {
    const int n1_ = n11 + n12, n_1 = n11 + n21, n = n11 + n12 + n21 + n22;
    const int max = (n_1 < n1_) ? n_1 : n1_;
    int min = n1_ + n_1 - n;
    if (min < 0) min = 0;
    if (min == max) return 1.;
    BvHgAcc x;
    x.n11 = n11; x.n1_ = n1_; x.n_1 = n_1; x.n = n;
    x.p = bv_hypergeo_lane(T, n11, n1_, n_1, n);
    const double q = x.p;
    if (q == 0.0) return 0.0;  // kfunc.c:260-289: two = 0
    double p, left, right;
    int i, j;
    p = bv_hgacc_step(T, min, x);
    for (left = 0., i = min + 1; p < 0.99999999 * q && i <= max; ++i) { left += p; p = bv_hgacc_step(T, i, x); }
    if (p < 1.00000001 * q) left += p;
    p = bv_hgacc_step(T, max, x);
    for (right = 0., j = max - 1; p < 0.99999999 * q && j >= 0; --j) { right += p; p = bv_hgacc_step(T, j, x); }
    if (p < 1.00000001 * q) right += p;
    double two = left + right;
    if (two > 1.) two = 1.;
    return two;
}
