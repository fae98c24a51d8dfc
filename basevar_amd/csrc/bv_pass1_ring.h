// bv_pass1_ring.h -- the long-row kernel's workgroup state (BvPass1Shared: the ring of histograms and its sequence flags) and the
// LDS flag primitives through which its waves meet, each with a bounded spin.
// Included by bv_pass1.hip (bv_pass1_kernel) and, for the flags, by bv_pass1_team.h.
#pragma once

#include "bv_kernels.h"
#include "bv_solver.h"

#define BV_RING_EXTRA 2
template <int NBUF>
struct __attribute__((aligned(16))) BvPass1Shared {
    uint32_t hist[NBUF][BV_H2_WORDS];  // ring of histograms [(rev<<2)|base][phred byte]
    uint32_t published[NBUF];          // times a site has been assigned to the slot (lead tally wave)
    uint32_t filled[NBUF];             // tally-wave arrivals on the slot (NTALLY per fill)
    uint32_t drained[NBUF];            // times the slot has been solved and re-zeroed
    uint32_t site_of[NBUF];            // site held by the slot (0xFFFFFFFF = no more work)
    uint32_t swz_of[NBUF];             // 1: the slot's row is tallied with the dense-row swizzle (bv_tally_chunk<.., SWZ>); set with site_of
    uint32_t dense_hint;               // the solver's: the row it solved last was dense (a quarter of its cells covered)
    double tab_hit[BV_QBINS], tab_miss[BV_QBINS];  // LDS copy of BvTables
    BvSolverShared sv[1];              // the solver wave's bins and scratch, reached as sv[wave - NTALLY] (see bv_pass1_kernel)
};

// ------------------------------------------------------------------------------ kernel
// Every spin is bounded (~1 s): a protocol bug must end the kernel with counters[3] set
// (reported by bv_engine_wait) instead of hanging the GPU.
#define BV_SPIN_SLEEP 16 /* x64 cycles between polls of a hand-off flag (4, 16, 64 measured: 4.09, 4.05, 4.04 ms) */
__device__ __forceinline__ void bv_wait_flag(const uint32_t *flag, uint32_t want, uint32_t *err) {
    uint32_t spins = 0;
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != want) {
        __builtin_amdgcn_s_sleep(BV_SPIN_SLEEP);
        if (++spins > (1u << 22)) {  // ~2 s
            atomicOr(err, BV_TMO_RING);  // (or, not add: sixteen waves giving up must not wrap the word to 0)
            break;
        }
    }
}
__device__ __forceinline__ void bv_set_flag(uint32_t *flag, uint32_t v) {
    __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// one arrival per WAVE (lane 0 only; the wave's earlier LDS atomics are ahead of it in the
// in-order LDS queue)
__device__ __forceinline__ void bv_add_flag(uint32_t *flag, int lane) {
    if (lane == 0) __hip_atomic_fetch_add(flag, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
