// bv_wave.h -- every cross-lane primitive of the library: the DPP scans, sums and min / max over the 64 lanes of a wave, the
// permlane-folded packed sums, and the row-local all-reduces, scans, ballot and broadcast of the 16-lane solver.
// Included by bv_device.h.
#pragma once

// ------------------------------------------------------------------ wave reductions
// All cross-lane sums use DPP (data-parallel primitives: a VALU operand read from another
// lane), not ds_bpermute: a bpermute round trip costs an LDS latency per butterfly step,
// six dependent steps per reduction, and the solver does several reductions per EM pass.
// Pattern (gfx9 family): inclusive scan inside each row of 16 lanes by row_shr 1,2,4,8,
// then row_bcast15 / row_bcast31 carry the row totals across rows; lane 63 ends up holding
// the wave total, which v_readlane broadcasts.  Fixed order => deterministic FP sums, and
// every lane receives the bit-identical value.
#define BV_DPP_ROW_SHR(n) (0x110 + (n))
#define BV_DPP_ROW_ROR(n) (0x120 + (n))
#define BV_DPP_BCAST15 0x142
#define BV_DPP_BCAST31 0x143
#define BV_DPP_QUAD_XOR1 0xB1 /* quad_perm [1,0,3,2] */
#define BV_DPP_QUAD_XOR2 0x4E /* quad_perm [2,3,0,1] */
#define BV_DPP_ROW_MIRROR 0x140
#define BV_DPP_ROW_HALF_MIRROR 0x141

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int bv_dpp_i32(int ident, int v) {
    return __builtin_amdgcn_update_dpp(ident, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double bv_dpp_f64(double v) {  // identity 0.0
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = bv_dpp_i32<CTRL, ROW_MASK>(0, lo);
    hi = bv_dpp_i32<CTRL, ROW_MASK>(0, hi);
    return __hiloint2double(hi, lo);
}
// the same with identity 1.0 (for products): lanes without a source read 1.0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double bv_dpp_f64_one(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = bv_dpp_i32<CTRL, ROW_MASK>(0, lo);
    hi = bv_dpp_i32<CTRL, ROW_MASK>(0x3FF00000, hi);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long bv_dpp_u64(unsigned long long v) {
    int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    lo = bv_dpp_i32<CTRL, ROW_MASK>(0, lo);
    hi = bv_dpp_i32<CTRL, ROW_MASK>(0, hi);
    return ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ int bv_readlane63_i32(int v) { return __builtin_amdgcn_readlane(v, 63); }

// One skeleton under every scan and reduction below, as macros: OP(v, x) is the combine, a statement on the running value, and
// MV(CTRL, ROW_MASK, v) the lane move -- v as the DPP source lane holds it, and the combine's identity in a lane that has no source.
// (Not templates: the pieces of a template are functions of their own when the compiler's first clean-up passes run, and the u64
// and u32 forms then come out as other instructions -- 12 to 30 more in each pass-2 kernel, 20 in the short-row solve kernel.)
#define BV_OP_ADD(v, x) v += (x)
#define BV_OP_MUL(v, x) v *= (x)
#define BV_OP_MIN(v, x) v = min(v, (x))
#define BV_OP_MAX(v, x) v = max(v, (x))
#define BV_MV_F64(C, M, v) bv_dpp_f64<C, M>(v)
#define BV_MV_F64_ONE(C, M, v) bv_dpp_f64_one<C, M>(v)
#define BV_MV_U32(C, M, v) (uint32_t)bv_dpp_i32<C, M>(0, (int)v)
#define BV_MV_U64(C, M, v) bv_dpp_u64<C, M>(v)
#define BV_MV_I32_TOP(C, M, v) bv_dpp_i32<C, M>(0x7fffffff, v)       /* the identity of min */
#define BV_MV_I32_BOTTOM(C, M, v) bv_dpp_i32<C, M>((int)0x80000000, v) /* the identity of max */
#define BV_MV_I32_SELF(C, M, v) bv_dpp_i32<C, M>(v, v)               /* an all-reduce: every lane has a source */
// inclusive scan inside each row of 16 lanes (SCAN8: its first three steps, inside each aligned group of 8 lanes)
#define BV_ROW_SCAN8(v, OP, MV) \
    OP(v, MV(BV_DPP_ROW_SHR(1), 0xf, v)); OP(v, MV(BV_DPP_ROW_SHR(2), 0xf, v)); OP(v, MV(BV_DPP_ROW_SHR(4), 0xf, v))
#define BV_ROW_SCAN(v, OP, MV) BV_ROW_SCAN8(v, OP, MV); OP(v, MV(BV_DPP_ROW_SHR(8), 0xf, v))
// the same carried across the rows: lane l ends with the combine of lanes 0..l
#define BV_WAVE_SCAN(v, OP, MV) BV_ROW_SCAN(v, OP, MV); OP(v, MV(BV_DPP_BCAST15, 0xa, v)); OP(v, MV(BV_DPP_BCAST31, 0xc, v))
// symmetric all-reduce over the L = 16 / 8 / 4 lanes of a row that own an item, see bv_g16_sum
#define BV_ROW_ALLREDUCE(v, OP, MV, L) \
    OP(v, MV(BV_DPP_QUAD_XOR1, 0xf, v)); OP(v, MV(BV_DPP_QUAD_XOR2, 0xf, v)); \
    if (L >= 8) OP(v, MV(BV_DPP_ROW_HALF_MIRROR, 0xf, v)); \
    if (L >= 16) OP(v, MV(BV_DPP_ROW_MIRROR, 0xf, v))

// inclusive prefix sums, and prefix PRODUCTS, over the 64 lanes
__device__ __forceinline__ double bv_wave_incl_scan_f64(double v) { BV_WAVE_SCAN(v, BV_OP_ADD, BV_MV_F64); return v; }
__device__ __forceinline__ double bv_wave_incl_scan_prod_f64(double v) { BV_WAVE_SCAN(v, BV_OP_MUL, BV_MV_F64_ONE); return v; }
__device__ __forceinline__ uint32_t bv_wave_incl_scan_u32(uint32_t v) { BV_WAVE_SCAN(v, BV_OP_ADD, BV_MV_U32); return v; }
__device__ __forceinline__ unsigned long long bv_wave_incl_scan_u64(unsigned long long v) { BV_WAVE_SCAN(v, BV_OP_ADD, BV_MV_U64); return v; }
__device__ __forceinline__ double bv_wave_sum(double v) {
    v = bv_wave_incl_scan_f64(v);
    int lo = bv_readlane63_i32(__double2loint(v)), hi = bv_readlane63_i32(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ uint32_t bv_wave_sum_u32(uint32_t v) {
    return (uint32_t)bv_readlane63_i32((int)bv_wave_incl_scan_u32(v));
}
__device__ __forceinline__ unsigned long long bv_wave_sum_u64(unsigned long long v) {
    v = bv_wave_incl_scan_u64(v);
    uint32_t lo = (uint32_t)bv_readlane63_i32((int)(uint32_t)v), hi = (uint32_t)bv_readlane63_i32((int)(uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// Packed sums: gfx950's v_permlane32_swap / v_permlane16_swap fold two (four) per-lane values into
// one register whose halves (rows of 16 lanes) carry the partial sums of different values, so two
// (four) wave totals cost one scan instead of two (four).  Fixed order => deterministic.
__device__ __forceinline__ double bv_fold32_f64(double a, double b) {
    // lanes 0-31: a[l] + a[l+32];  lanes 32-63: b[l-32] + b[l]
    unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
    unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
    auto rl = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    auto rh = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    return __hiloint2double((int)rh[0], (int)rl[0]) + __hiloint2double((int)rh[1], (int)rl[1]);
}
__device__ __forceinline__ double bv_fold16_f64(double p, double q) {
    // rows of 16 lanes: [p0+p1, q0+q1, p2+p3, q2+q3]
    unsigned plo = (unsigned)__double2loint(p), phi = (unsigned)__double2hiint(p);
    unsigned qlo = (unsigned)__double2loint(q), qhi = (unsigned)__double2hiint(q);
    auto rl = __builtin_amdgcn_permlane16_swap(plo, qlo, false, false);
    auto rh = __builtin_amdgcn_permlane16_swap(phi, qhi, false, false);
    return __hiloint2double((int)rh[0], (int)rl[0]) + __hiloint2double((int)rh[1], (int)rl[1]);
}
__device__ __forceinline__ double bv_readlane_f64(double v, int srclane) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), srclane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), srclane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void bv_wave_sum2(double a, double b, double &sa, double &sb) {
    double v = bv_fold32_f64(a, b);
    BV_ROW_SCAN(v, BV_OP_ADD, BV_MV_F64);
    v += bv_dpp_f64<BV_DPP_BCAST15, 0xa>(v);
    sa = bv_readlane_f64(v, 31);
    sb = bv_readlane_f64(v, 63);
}
__device__ __forceinline__ void bv_wave_sum4(double a, double b, double c, double d, double &sa, double &sb, double &sc,
                                             double &sd) {
    double v = bv_fold16_f64(bv_fold32_f64(a, b), bv_fold32_f64(c, d));  // rows: [a, c, b, d]
    BV_ROW_SCAN(v, BV_OP_ADD, BV_MV_F64);
    sa = bv_readlane_f64(v, 15);
    sc = bv_readlane_f64(v, 31);
    sb = bv_readlane_f64(v, 47);
    sd = bv_readlane_f64(v, 63);
}
// Eight u32 wave totals with one scan: 32-lane fold, 16-lane fold, 8-lane fold, then a 3-step scan
// inside groups of 8 lanes (26 VALU instead of 8 x 13).
__device__ __forceinline__ uint32_t bv_fold32_u32(uint32_t a, uint32_t b) {
    auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    return r[0] + r[1];
}
__device__ __forceinline__ uint32_t bv_fold16_u32(uint32_t p, uint32_t q) {
    auto r = __builtin_amdgcn_permlane16_swap(p, q, false, false);
    return r[0] + r[1];
}
__device__ __forceinline__ void bv_wave_sum8_u32(const uint32_t v[8], uint32_t out[8], int lane) {
    uint32_t t0 = bv_fold16_u32(bv_fold32_u32(v[0], v[1]), bv_fold32_u32(v[2], v[3]));  // rows: v0, v2, v1, v3
    uint32_t t1 = bv_fold16_u32(bv_fold32_u32(v[4], v[5]), bv_fold32_u32(v[6], v[7]));  // rows: v4, v6, v5, v7
    t0 += (uint32_t)bv_dpp_i32<BV_DPP_ROW_ROR(8), 0xf>(0, (int)t0);  // both halves of a row: its 8 pair sums
    t1 += (uint32_t)bv_dpp_i32<BV_DPP_ROW_ROR(8), 0xf>(0, (int)t1);
    uint32_t w = (lane & 8) ? t1 : t0;
    BV_ROW_SCAN8(w, BV_OP_ADD, BV_MV_U32);
    out[0] = (uint32_t)__builtin_amdgcn_readlane((int)w, 7);
    out[4] = (uint32_t)__builtin_amdgcn_readlane((int)w, 15);
    out[2] = (uint32_t)__builtin_amdgcn_readlane((int)w, 23);
    out[6] = (uint32_t)__builtin_amdgcn_readlane((int)w, 31);
    out[1] = (uint32_t)__builtin_amdgcn_readlane((int)w, 39);
    out[5] = (uint32_t)__builtin_amdgcn_readlane((int)w, 47);
    out[3] = (uint32_t)__builtin_amdgcn_readlane((int)w, 55);
    out[7] = (uint32_t)__builtin_amdgcn_readlane((int)w, 63);
}
// min / max: same scan shape with the matching identity
__device__ __forceinline__ int bv_wave_min_i32(int v) { BV_WAVE_SCAN(v, BV_OP_MIN, BV_MV_I32_TOP); return bv_readlane63_i32(v); }
__device__ __forceinline__ int bv_wave_max_i32(int v) { BV_WAVE_SCAN(v, BV_OP_MAX, BV_MV_I32_BOTTOM); return bv_readlane63_i32(v); }

// ------------------------------------------------------------------ row-local primitives
// All-reduce over the 16 lanes of a row.  Every step pairs lanes symmetrically (i <-> i^1, i^2, 7-i, 15-i) and IEEE
// addition is commutative, so all 16 lanes end with the bit-identical sum -- no broadcast needed.
// L: the lanes that own the item -- 16 (a whole DPP row), or 8 / 4 (aligned parts of one: the pop-group solver for small groups,
// bv_p2g_solve_small_kernel): the first log2(L) steps of the same pairing.
template <int L = 16>
__device__ __forceinline__ double bv_g16_sum(double v) { BV_ROW_ALLREDUCE(v, BV_OP_ADD, BV_MV_F64, L); return v; }
__device__ __forceinline__ uint32_t bv_g16_sum_u32(uint32_t v) { BV_ROW_ALLREDUCE(v, BV_OP_ADD, BV_MV_U32, 16); return v; }
__device__ __forceinline__ unsigned long long bv_g16_sum_u64(unsigned long long v) { BV_ROW_ALLREDUCE(v, BV_OP_ADD, BV_MV_U64, 16); return v; }
__device__ __forceinline__ int bv_g16_max_i32(int v) { BV_ROW_ALLREDUCE(v, BV_OP_MAX, BV_MV_I32_SELF, 16); return v; }
__device__ __forceinline__ int bv_g16_min_i32(int v) { BV_ROW_ALLREDUCE(v, BV_OP_MIN, BV_MV_I32_SELF, 16); return v; }
// inclusive prefix PRODUCTS inside the row
__device__ __forceinline__ double bv_g16_incl_scan_prod_f64(double v) { BV_ROW_SCAN(v, BV_OP_MUL, BV_MV_F64_ONE); return v; }
// inclusive prefix sum inside the row (lane 15 of the row ends with the total)
__device__ __forceinline__ uint32_t bv_g16_incl_scan_u32(uint32_t v) { BV_ROW_SCAN(v, BV_OP_ADD, BV_MV_U32); return v; }
// the 16 ballot bits of this lane's group
__device__ __forceinline__ uint32_t bv_g16_ballot(bool pred, int lane) {
    return (uint32_t)(__ballot(pred) >> (lane & 48)) & 0xFFFFu;
}
// value held by lane `k` (0..15, uniform in the group) of this lane's group
__device__ __forceinline__ double bv_g16_bcast_f64(double v, int k, int lane) {
    const int src = ((lane & 48) | (k & 15)) << 2;
    const int lo = __builtin_amdgcn_ds_bpermute(src, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(v));
    return __hiloint2double(hi, lo);
}
