// bv_hostlog.h -- log() as the host's libm computes it, restated for the device over BvTables::hostlog.
// Included by bv_device.h, behind BvTables.
#pragma once

// `logmiss` (BvTables::logmiss in device memory, or NULL) -> the host-log table, or NULL when the engine could not
// verify it (the ordered replay then uses the device library's log, ulps from the host's)
__device__ __forceinline__ const double *bv_hostlog_of(const double *logmiss) {
    if (!logmiss) return nullptr;
    const double *t = logmiss + BV_QBINS;
    return t[BV_HOSTLOG_N] != 0. ? t : nullptr;
}

// log(x) the way the host's glibc computes it on an FMA-capable x86-64 (sysdeps/ieee754/dbl-64/e_log.c, the variant
// its ifunc picks there): a 128-entry table of (1/c, log c), a degree-5 polynomial in r = z/c - 1, the near-1 branch
// with the split r = rhi + rlo, every fused multiply-add exactly where the compiled routine has one.  The reference's
// EM compares and truncates sums of such logs (algorithm.h:238-255), so at tie-prone shallow sites the last bit matters.
// T: BvTables::hostlog.  The same restatement runs on the host against log() before the table is accepted.
__device__ __forceinline__ double bv_log_host(double x, const double *__restrict__ T) {
    const double *A = T + 2, *Bc = T + 7, *tab = T + 18;
    uint64_t ix = (uint64_t)__double_as_longlong(x);
    const uint64_t LO = 0x3fee000000000000ull, HI = 0x3ff1090000000000ull;  // 1 - 2^-4, 1 + 0x1.09p-4
    if (ix - LO < HI - LO) {
        if (ix == 0x3ff0000000000000ull) return 0.;
        const double r = __dadd_rn(x, -1.0), r2 = __dmul_rn(r, r), r3 = __dmul_rn(r, r2);
        const double pA = __fma_rn(r2, Bc[3], __fma_rn(r, Bc[2], Bc[1]));
        const double pB = __fma_rn(r2, Bc[6], __fma_rn(r, Bc[5], Bc[4]));
        const double pC = __fma_rn(r3, Bc[10], __fma_rn(r2, Bc[9], __fma_rn(r, Bc[8], Bc[7])));
        const double p = __fma_rn(__fma_rn(pC, r3, pB), r3, pA);
        const double t = __fma_rn(r, 0x1p27, r), rhi = __fma_rn(-0x1p27, r, t), rlo = __dadd_rn(r, -rhi);
        const double s = __dmul_rn(rhi, rhi);
        const double hi = __fma_rn(s, Bc[0], r);
        const double lo = __fma_rn(s, Bc[0], __dadd_rn(r, -hi));
        const double lo2 = __fma_rn(__dmul_rn(Bc[0], rlo), __dadd_rn(rhi, r), lo);
        return __dadd_rn(__fma_rn(p, r3, lo2), hi);
    }
    const uint32_t top = (uint32_t)(ix >> 48);
    if (top - 0x0010u >= 0x7ff0u - 0x0010u) {
        if ((ix << 1) == 0ull) return -__longlong_as_double(0x7ff0000000000000ll);
        if (ix == 0x7ff0000000000000ull) return x;
        if ((top & 0x8000u) || (top & 0x7ff0u) == 0x7ff0u) return __longlong_as_double(0x7ff8000000000000ll);
        ix = (uint64_t)__double_as_longlong(__dmul_rn(x, 0x1p52));  // subnormal: scale up, take it off the exponent
        ix -= 52ull << 52;
    }
    const uint64_t tmp = ix - 0x3fe6000000000000ull;
    const uint32_t i = (uint32_t)(tmp >> 45) & 127u;
    const int k = (int)((int64_t)tmp >> 52);
    const double z = __longlong_as_double((long long)(ix - (tmp & (0xfffull << 52))));
    const double invc = tab[2u * i], logc = tab[2u * i + 1u], kd = (double)k;
    const double r = __fma_rn(z, invc, -1.0);
    const double w = __fma_rn(kd, T[0], logc), hi = __dadd_rn(r, w);
    const double lo = __fma_rn(kd, T[1], __dadd_rn(__dadd_rn(w, -hi), r));
    const double r2 = __dmul_rn(r, r), r3 = __dmul_rn(r, r2);
    const double p = __fma_rn(__fma_rn(r, A[4], A[3]), r2, __fma_rn(r, A[2], A[1]));
    return __dadd_rn(__fma_rn(r3, p, __fma_rn(r2, A[0], lo)), hi);
}
