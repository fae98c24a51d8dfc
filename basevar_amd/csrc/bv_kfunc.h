// bv_kfunc.h -- device forms of htslib/kfunc.c's special functions, QUAL from a chi-square statistic, and log(n!).
// Included by bv_device.h.
#pragma once

// ------------------------------------------------------------------ special functions
// Device forms of htslib/kfunc.c as the reference calls them.  Same evaluation order as
// the reference so that only libm-vs-ocml ulp differences of exp/log remain.

// kf_lgamma, htslib/kfunc.c:39-52
__device__ inline double bv_kf_lgamma(double z) {
    double x = 0;
    x += 0.1659470187408462e-06 / (z + 7);
    x += 0.9934937113930748e-05 / (z + 6);
    x -= 0.1385710331296526 / (z + 5);
    x += 12.50734324009056 / (z + 4);
    x -= 176.6150291498386 / (z + 3);
    x += 771.3234287757674 / (z + 2);
    x -= 1259.139216722289 / (z + 1);
    x += 676.5203681218835 / z;
    x += 0.9999999999995183;
    return log(x) - 5.58106146679532777 - z + (z - 0.5) * log(z + 6.5);
}

// kf_erfc, htslib/kfunc.c:58-84
__device__ inline double bv_kf_erfc(double x) {
    const double SQRT2 = 1.41421356237309504880;
    double z = fabs(x) * SQRT2;
    if (z > 37.) return x > 0. ? 0. : 2.;
    double expntl = exp(z * z * -.5);
    double p;
    if (z < 10. / SQRT2) {
        double num = .03526249659989109;
        num = num * z + .7003830644436881;
        num = num * z + 6.37396220353165;
        num = num * z + 33.912866078383;
        num = num * z + 112.0792914978709;
        num = num * z + 221.2135961699311;
        num = num * z + 220.2068679123761;
        double den = .08838834764831844;
        den = den * z + 1.755667163182642;
        den = den * z + 16.06417757920695;
        den = den * z + 86.78073220294608;
        den = den * z + 296.5642487796737;
        den = den * z + 637.3336333788311;
        den = den * z + 793.8265125199484;
        den = den * z + 440.4137358247522;
        p = expntl * num / den;
    } else {
        p = expntl / 2.506628274631001 / (z + 1. / (z + 2. / (z + 3. / (z + 4. / (z + .65)))));
    }
    return x > 0. ? 2. * p : 2. * (1. - p);
}

// kf_gammaq, htslib/kfunc.c:103-143
__device__ inline double bv_kf_gammaq(double s, double z) {
    const double EPS = 1e-14, TINY = 1e-290;
    if (z <= 1. || z < s) {
        double sum = 1., x = 1.;
        for (int k = 1; k < 100; ++k) {
            x *= z / (s + k);
            sum += x;
            if (x / sum < EPS) break;
        }
        return 1. - exp(s * log(z) - z - bv_kf_lgamma(s + 1.) + log(sum));
    }
    double f = 1. + z - s, C = f, D = 0.;
    for (int j = 1; j < 100; ++j) {
        double a = j * (s - j), b = (j << 1) + 1 + z - s, d;
        D = b + a * D;
        if (D < TINY) D = TINY;
        C = b + a / C;
        if (C < TINY) C = TINY;
        D = 1. / D;
        d = C * D;
        f *= d;
        if (fabs(d - 1.) < EPS) break;
    }
    return exp(s * log(z) - z - bv_kf_lgamma(s) - log(f));
}

// QUAL from the last LRT statistic, src/basetype.cpp:186-195 (chi2_test: algorithm.h:44-46)
__device__ inline double bv_qual_from_chi2(double chi) {
    double p = bv_kf_gammaq(0.5, chi / 2.0);
    if (isnan(p)) p = 1.0;
    double q = (p != 0.0) ? -10 * log10(p) : 10000.0;
    if (q == 0.0) q = 0.0;  // -0.0 -> 0.0
    return q;
}

// log(n!) == lgamma(n + 1) from the engine's table of the host's values, the Stirling series beyond it: see bv_fisher.h
struct BvLnTab {
    const double *t;  // t[k] = lgamma(k + 1), k < n
    int n;
};
__device__ __forceinline__ double bv_lnfact_series(int n) {
    if (n < 16) {
        const double T0 = 0.0, T2 = 0.693147180559945, T3 = 1.7917594692280554, T4 = 3.178053830347945,
                     T5 = 4.787491742782047, T6 = 6.579251212010102, T7 = 8.525161361065415, T8 = 10.604602902745249,
                     T9 = 12.801827480081467, T10 = 15.104412573075514, T11 = 17.502307845873887,
                     T12 = 19.987214495661885, T13 = 22.55216385312342, T14 = 25.191221182738683,
                     T15 = 27.89927138384089;
        // select chain instead of a memory table: no scratch / constant-memory traffic
        double lo = n < 2 ? T0 : (n == 2 ? T2 : (n == 3 ? T3 : (n == 4 ? T4 : (n == 5 ? T5 : (n == 6 ? T6 : T7)))));
        double hi = n == 8 ? T8 : (n == 9 ? T9 : (n == 10 ? T10 : (n == 11 ? T11 : (n == 12 ? T12 : (n == 13 ? T13 : (n == 14 ? T14 : T15))))));
        return n < 8 ? lo : hi;
    }
    const double x = (double)n + 1.0;
    const double xi = 1.0 / x, x2 = xi * xi;
    double s = 1.0 / 156.0;
    s = s * x2 + (-691.0 / 360360.0);
    s = s * x2 + (1.0 / 1188.0);
    s = s * x2 + (-1.0 / 1680.0);
    s = s * x2 + (1.0 / 1260.0);
    s = s * x2 + (-1.0 / 360.0);
    s = s * x2 + (1.0 / 12.0);
    s *= xi;
    return (x - 0.5) * log(x) - x + 0.91893853320467274178 + s;
}
__device__ __forceinline__ double bv_lnfact(const BvLnTab &T, int n) {
#ifdef BV_LNFACT_TABLE_ONLY
    // short-row kernels: a depth is at most 65,535 there and the engine's table never has fewer than 65,536 entries
    // (bv_engine_create), so the series -- a log() and a select chain inlined at every one of ~60 call sites -- stays out
    return T.t[n < T.n ? n : T.n - 1];
#else
    if (n < T.n) return T.t[n];
    return bv_lnfact_series(n);
#endif
}
