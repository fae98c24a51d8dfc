// bv_device.h -- gfx950 device building blocks of the per-site basetype solver.
//
// Everything here operates on a per-site (base x phred) histogram that the tally loop
// builds in LDS.  The key identity: the reference's per-sample
// likelihood row depends only on (first base in ACGT, phred q) -- src/basetype.cpp:47-64 --
// so its n_cov x 4 EM collapses exactly onto <= 4 x 94 weighted bins.
//
// Execution model: wave64.  Every solver routine is a *wave-level* function: the 64 lanes
// of one wavefront cooperate through DPP scans (lane 63's total is broadcast with
// v_readlane, so every lane holds the bit-identical sum), and independent routines
// (the up-to-4 EM runs of one LRT level, Fisher tests, rank sums) are spread over the
// waves of the workgroup.  No MFMA: this is categorical-table arithmetic in FP64.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/basevar_amd.h"
#include "../../include/basevar_amd_diag.h"  // diagnostic / A-B flag bits the kernels honour

#define BV_WAVE 64
#define BV_QBINS 128                       /* phred axis of the LDS histogram          */
#define BV_ROWS 8                          /* (reverse << 2) | base                    */
#define BV_HIST_WORDS (BV_ROWS * BV_QBINS) /* 1024 x u32 = 4 KiB                       */
#define BV_NQ_VALID 94                     /* phred 0..93                              */
#define BV_MAX_BINS (4 * BV_NQ_VALID)      /* 376                                      */
#define BV_SLOTS 6                         /* ceil(376 / 64) bins per lane             */

// cell encoding used by the planes (include/basevar_amd.h):
//   bits 0-1 base, bit 2 reverse strand, bit 3 "not a base call" (N / + / -)
#ifndef BV_CELL_NOCALL
#define BV_CELL_NOCALL 0x08u
#endif
#define BV_HOSTLOG_N 274  // ln2hi, ln2lo, A[5], B[11], 128 x {invc, logc}: glibc's __log_data

// native 16-byte vector: one lane's share of a coalesced 1 KiB wave load
typedef uint32_t bv_u32x4 __attribute__((ext_vector_type(4)));

// (1 - eps_q) and eps_q / 3 for q = 0..127, filled on the host with glibc exp() so that
// eps is bit-identical to the reference's exp((qchar - 33) * MLN10TO10), basetype.cpp:47.
struct BvTables {
    double hit[BV_QBINS];
    double miss[BV_QBINS];
    const double *lnfact;  // lnfact[k] = lgamma(k + 1) (host glibc), k < lnfact_n; device memory
    uint32_t lnfact_n;
    uint32_t pad_;
    double loghit[BV_QBINS];   // log(hit[q]), log(miss[q]) with the host's log(): the per-sample log-marginals of a
    double logmiss[BV_QBINS];  // single-base subset (algorithm.h:243 with f == 1), see bv_lrt
    // The host libm's own log() data, found in the loaded libm at engine creation and accepted only after the
    // restated algorithm (bv_log_host below) reproduced the host's log() bit for bit on a few hundred thousand
    // arguments: ln2hi, ln2lo, A[5], B[11], then 128 x {invc, logc}.  hostlog[BV_HOSTLOG_N] != 0 <=> usable.
    // Must follow logmiss directly: the ordered replay finds it as logmiss + BV_QBINS (bv_hostlog_of).
    double hostlog[BV_HOSTLOG_N + 2];
};
static_assert(offsetof(BvTables, hostlog) == offsetof(BvTables, logmiss) + sizeof(double) * BV_QBINS, "hostlog follows logmiss");

// The building blocks themselves, in dependency order (each is included from here alone and relies on the ones before it):
#include "bv_hostlog.h"
#include "bv_wave.h"
#include "bv_kfunc.h"
#include "bv_fisher.h"
#include "bv_ranksum.h"
#include "bv_em.h"
#include "bv_lrt.h"
