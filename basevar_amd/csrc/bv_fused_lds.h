// bv_fused_lds.h -- the fused short-row kernel's statements on LDS and memory: the four LDS-DMA forms of a ring slot (always four
// loads: the counted waits rely on it), the wave-level compare-and-swap / fetch-and-add, scalar reads, the pass-1 tally of a slot,
// the masks of a tagged pass-2 row's last slot.
// Included by bv_pass1_fused.hip alone, behind bv_fused_shared.h; the solver, stream and pass-2 pieces call into it.
#pragma once

// ---- LDS-DMA of one slot: four 1 KiB pieces (64 lanes x 16 bytes from p_i + v_i) to d0, d0 + 1 KiB, ..., always four (the
// counted waits rely on it).  M0 is written inside the statement; the s_add between the write and the load is the wait state.
__device__ __forceinline__ void bv_f_glds4(uint32_t d0, const uint8_t *p0, uint32_t v0, const uint8_t *p1, uint32_t v1,
                                           const uint8_t *p2, uint32_t v2, const uint8_t *p3, uint32_t v3) {
    uint32_t keep, t;
    asm volatile(
        "s_mov_b32 %[keep], m0\n\t"
        "s_mov_b32 m0, %[d0]\n\t"
        "s_add_u32 %[t], %[d0], 0x400\n\t"
        "global_load_lds_dwordx4 %[v0], %[p0] nt\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_add_u32 %[t], %[d0], 0x800\n\t"
        "global_load_lds_dwordx4 %[v1], %[p1] nt\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_add_u32 %[t], %[d0], 0xc00\n\t"
        "global_load_lds_dwordx4 %[v2], %[p2] nt\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %[v3], %[p3] nt\n\t"
        "s_mov_b32 m0, %[keep]"
        : [keep] "=&s"(keep), [t] "=&s"(t)
        : [d0] "s"(d0), [p0] "s"(p0), [p1] "s"(p1), [p2] "s"(p2), [p3] "s"(p3), [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2), [v3] "v"(v3)
        : "memory", "scc");
}
// A row's last slot: lanes past the row's end load nothing (mA: pieces 0 and 2, mB: pieces 1 and 3 -- never empty: a piece
// that lies wholly past the end is "loaded" by lane 0 alone from valid bytes of the slot; its cells are masked in the tally).
__device__ __forceinline__ void bv_f_glds4_masked(uint32_t d0, const uint8_t *p0, uint32_t v0, const uint8_t *p1, uint32_t v1,
                                                  const uint8_t *p2, uint32_t v2, const uint8_t *p3, uint32_t v3,
                                                  unsigned long long mA, unsigned long long mB) {
    uint32_t keep, t;
    unsigned long long sv;
    asm volatile(
        "s_mov_b32 %[keep], m0\n\t"
        "s_mov_b64 %[sv], exec\n\t"
        "s_mov_b64 exec, %[mA]\n\t"
        "s_mov_b32 m0, %[d0]\n\t"
        "s_add_u32 %[t], %[d0], 0x800\n\t"
        "global_load_lds_dwordx4 %[v0], %[p0] nt\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_add_u32 %[t], %[d0], 0x400\n\t"
        "global_load_lds_dwordx4 %[v2], %[p2] nt\n\t"
        "s_mov_b64 exec, %[mB]\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_add_u32 %[t], %[d0], 0xc00\n\t"
        "global_load_lds_dwordx4 %[v1], %[p1] nt\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %[v3], %[p3] nt\n\t"
        "s_mov_b64 exec, %[sv]\n\t"
        "s_mov_b32 m0, %[keep]"
        : [keep] "=&s"(keep), [t] "=&s"(t), [sv] "=&s"(sv)
        : [d0] "s"(d0), [p0] "s"(p0), [p1] "s"(p1), [p2] "s"(p2), [p3] "s"(p3), [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2), [v3] "v"(v3),
          [mA] "s"(mA), [mB] "s"(mB)
        : "memory", "scc");
}
// A pass-2 slot of the tagged rank layout (BV_SLAB_RPR_TAGGED): no call bytes -- 1 KiB of mapq and 2 KiB of ranks to the slot's
// second, third and fourth KiB.  Still FOUR loads, because the counted waits count four per slot whatever its kind: the first is
// lane 0 alone, 16 bytes of the mapq piece into the unused first KiB (the same line the second load fetches: no traffic of its own).
__device__ __forceinline__ void bv_f_glds4_tag(uint32_t d0, const uint8_t *p1, uint32_t v1, const uint8_t *p2, uint32_t v2, uint32_t v3) {
    uint32_t keep, t;
    unsigned long long sv;
    asm volatile(
        "s_mov_b32 %[keep], m0\n\t"
        "s_mov_b64 %[sv], exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "s_mov_b32 m0, %[d0]\n\t"
        "s_add_u32 %[t], %[d0], 0x400\n\t"
        "global_load_lds_dwordx4 %[v1], %[p1] nt\n\t"
        "s_mov_b64 exec, %[sv]\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_add_u32 %[t], %[d0], 0x800\n\t"
        "global_load_lds_dwordx4 %[v1], %[p1] nt\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_add_u32 %[t], %[d0], 0xc00\n\t"
        "global_load_lds_dwordx4 %[v2], %[p2] nt\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %[v3], %[p2] nt\n\t"
        "s_mov_b32 m0, %[keep]"
        : [keep] "=&s"(keep), [t] "=&s"(t), [sv] "=&s"(sv)
        : [d0] "s"(d0), [p1] "s"(p1), [p2] "s"(p2), [v1] "v"(v1), [v2] "v"(v2), [v3] "v"(v3)
        : "memory", "scc");
}
// Four pieces, each under a lane mask of its own (never empty): the last slot of a pass-2 row, whose 2 KiB of ranks end at twice the
// lane count of its 1 KiB of mapq.
__device__ __forceinline__ void bv_f_glds4_m4(uint32_t d0, const uint8_t *p0, uint32_t v0, unsigned long long m0, const uint8_t *p1, uint32_t v1,
                                              unsigned long long m1, const uint8_t *p2, uint32_t v2, unsigned long long m2, const uint8_t *p3,
                                              uint32_t v3, unsigned long long m3) {
    // (a row's last slot only: the operands are made scalar here, whatever the compiler believes about them at the call site)
    auto u32 = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
    auto u64 = [&](unsigned long long x) { return ((unsigned long long)u32((uint32_t)(x >> 32)) << 32) | u32((uint32_t)x); };
    d0 = u32(d0); m0 = u64(m0); m1 = u64(m1); m2 = u64(m2); m3 = u64(m3);
    p0 = (const uint8_t *)(uintptr_t)u64((uintptr_t)p0); p1 = (const uint8_t *)(uintptr_t)u64((uintptr_t)p1);
    p2 = (const uint8_t *)(uintptr_t)u64((uintptr_t)p2); p3 = (const uint8_t *)(uintptr_t)u64((uintptr_t)p3);
    uint32_t keep, t;
    unsigned long long sv;
    asm volatile(
        "s_mov_b32 %[keep], m0\n\t"
        "s_mov_b64 %[sv], exec\n\t"
        "s_mov_b32 m0, %[d0]\n\t"
        "s_mov_b64 exec, %[m0_]\n\t"
        "s_add_u32 %[t], %[d0], 0x400\n\t"
        "global_load_lds_dwordx4 %[v0], %[p0] nt\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_mov_b64 exec, %[m1_]\n\t"
        "s_add_u32 %[t], %[d0], 0x800\n\t"
        "global_load_lds_dwordx4 %[v1], %[p1] nt\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_mov_b64 exec, %[m2_]\n\t"
        "s_add_u32 %[t], %[d0], 0xc00\n\t"
        "global_load_lds_dwordx4 %[v2], %[p2] nt\n\t"
        "s_mov_b32 m0, %[t]\n\t"
        "s_mov_b64 exec, %[m3_]\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %[v3], %[p3] nt\n\t"
        "s_mov_b64 exec, %[sv]\n\t"
        "s_mov_b32 m0, %[keep]"
        : [keep] "=&s"(keep), [t] "=&s"(t), [sv] "=&s"(sv)
        : [d0] "s"(d0), [p0] "s"(p0), [p1] "s"(p1), [p2] "s"(p2), [p3] "s"(p3), [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2), [v3] "v"(v3),
          [m0_] "s"(m0), [m1_] "s"(m1), [m2_] "s"(m2), [m3_] "s"(m3)
        : "memory", "scc");
}
// One wave-level compare-and-swap on an LDS word by lane 0, the old value in an SGPR (no divergent branch, no vector-memory
// operation: see bv_lds_fetch_add_wave)
__device__ __forceinline__ uint32_t bv_f_lds_cas_wave(uint32_t lds_addr, uint32_t expect, uint32_t desired) {
    uint32_t r, tc, td;
    unsigned long long sv;
    asm volatile(
        "s_mov_b64 %[sv], exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "v_mov_b32 %[tc], %[cmp]\n\t"
        "v_mov_b32 %[td], %[val]\n\t"
        "ds_cmpst_rtn_b32 %[tc], %[adr], %[tc], %[td]\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_readfirstlane_b32 %[r], %[tc]\n\t"
        "s_mov_b64 exec, %[sv]"
        : [r] "=&s"(r), [tc] "=&v"(tc), [td] "=&v"(td), [sv] "=&s"(sv)
        : [adr] "v"(lds_addr), [cmp] "s"(expect), [val] "s"(desired)
        : "memory");
    return r;
}
// One wave-level fetch-and-add on a word of device memory by lane 0, the old value in an SGPR (as the compiler emits a returning
// agent-scope atomicAdd: `global_atomic_add ... sc0`), waited for inside the statement: the wave's LDS-DMA ring drains with it.
__device__ __forceinline__ uint32_t bv_f_global_fetch_add_wave(const uint32_t *p, uint32_t v) {
    uint32_t r, t, z;
    unsigned long long sv;
    asm volatile(
        "s_mov_b64 %[sv], exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "v_mov_b32 %[t], %[val]\n\t"
        "v_mov_b32 %[z], 0\n\t"
        "global_atomic_add %[t], %[z], %[t], %[base] sc0\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "v_readfirstlane_b32 %[r], %[t]\n\t"
        "s_mov_b64 exec, %[sv]"
        : [r] "=&s"(r), [t] "=&v"(t), [z] "=&v"(z), [sv] "=&s"(sv)
        : [val] "s"(v), [base] "s"(p)
        : "memory");
    return r;
}
// a reference base through the scalar cache (lgkmcnt: a vector load would sit in the vmcnt queue of the ring)
typedef const __attribute__((address_space(4))) uint32_t *bv_c32;
__device__ __forceinline__ uint32_t bv_f_ref_scalar(const uint8_t *ref_base, uint32_t site) {
    const uintptr_t p = (uintptr_t)ref_base + site;
    const uint32_t w = *(bv_c32)(p & ~(uintptr_t)3);
    return (w >> (8u * (uint32_t)(p & 3))) & 0xFFu;
}
__device__ __forceinline__ uint32_t bv_f_lds_read_u(const uint32_t *p) {  // p: a word of the kernel's __shared__ block
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)*(const volatile __attribute__((address_space(3))) uint32_t *)p);
}
__device__ __forceinline__ uint32_t bv_f_keep_mask(int kept) {  // dword mask of the first `kept` bytes
    return kept >= 4 ? 0xFFFFFFFFu : (kept <= 0 ? 0u : (1u << (8 * kept)) - 1u);
}

// the cells of two 16-byte chunks per lane (first and second KiB of a slot) -> the wave's histogram
// (The dense-row bank swizzle of the long-row kernel, bv_tally_chunk<.., SWZ>, was tried here too, per wave and row: at full
// coverage it gained nothing -- 120 against 122 M sites/s at 10,000 samples --, rows of coverage 0.3 lost 12 % to its VALU work and
// the un-swizzle, and its registers cost the sparse rows 3 %: not kept.)
__device__ __forceinline__ void bv_f_tally2(bv_u32x4 vbA, bv_u32x4 vqA, bv_u32x4 vbB, bv_u32x4 vqB, uint32_t *hist, uint32_t one) {
    // A phred byte >= 128 (invalid input) would carry into its neighbour under the shift below: such a slot takes the
    // exact cell-by-cell path (wave-uniform branch; never taken on valid data).
    const uint32_t hi = ((vqA.x | vqA.y | vqA.z) | (vqA.w | vqB.x | vqB.y) | (vqB.z | vqB.w)) & 0x80808080u;
    if (__builtin_expect(__ballot(hi != 0u) != 0ull, 0)) {
        const uint32_t wb[8] = {vbA.x, vbA.y, vbA.z, vbA.w, vbB.x, vbB.y, vbB.z, vbB.w};
        const uint32_t wq[8] = {vqA.x, vqA.y, vqA.z, vqA.w, vqB.x, vqB.y, vqB.z, vqB.w};
#pragma unroll 1
        for (int j = 0; j < 32; ++j) {
            const uint32_t c = (wb[j >> 2] >> (8 * (j & 3))) & 0xFFu, p = (wq[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            if (c < 8u) atomicAdd(p < 128u ? &hist[(c << 7) | p] : &hist[BV_S_HWORDS + c], 1u);
        }
        return;
    }
    // X = call << 8 | phred << 1 = twice the word index of the 8 x 128 histogram; call < 8 <=> X < 0x800
    vqA.x <<= 1; vqA.y <<= 1; vqA.z <<= 1; vqA.w <<= 1;
    vqB.x <<= 1; vqB.y <<= 1; vqB.z <<= 1; vqB.w <<= 1;
    bv_tally_chunk<1>(vbA, vqA, hist, one);
    bv_tally_chunk<1>(vbB, vqB, hist, one);
}
// A pass-2 slot or block of the tagged rank layout that is its row's last (last2: its chunks inside the row, tail = n_samples & 15):
// the rank words of a lane past the row's end were not loaded (stale bytes) and read as "no call", as do the cells of the row's last
// chunk at or beyond n_samples.  w2 / w3: the lane's ranks 0-7 / 8-15.
__device__ __forceinline__ void bv_f_p2t_last(bv_u32x4 &w2, bv_u32x4 &w3, int lane, uint32_t last2, int tail) {
    if ((uint32_t)lane >= last2) { w2 = bv_u32x4{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u}; w3 = w2; }
    else if (tail && (uint32_t)lane == last2 - 1u) bv_p2t_mask_tail16(w2, w3, tail);
}
