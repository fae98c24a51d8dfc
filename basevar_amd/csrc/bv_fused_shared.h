// bv_fused_shared.h -- the fused short-row kernel (bv_pass1_fused.hip): its tunables, the counted waits of the LDS-DMA ring, the
// debug macro sets, the control words and flags, and the workgroup's LDS block (BvFusedRing, BvFusedShared).
// Included by bv_pass1_fused.hip alone, first of the bv_fused_*.h pieces and behind bv_short.h (BvP1sWaveScratch, BV_S_*);
// every other piece relies on it.
#pragma once

#ifndef BV_F_NS
#define BV_F_NS 8                         /* streaming waves per workgroup */
#endif
#ifndef BV_F_NV
#define BV_F_NV 4                         /* dedicated solver waves per workgroup (7 + 5 measured -1.2 %; round 5, lean solver: 8 + 3 -0.8 %, 8 + 2 -4 %) */
#endif
static_assert(BV_F_NV >= 1, "the streaming waves wait on a full queue: somebody must be emptying it");
#define BV_F_NW (BV_F_NS + BV_F_NV)
#ifndef BV_F_K
#define BV_F_K 3                          /* ring slots per streaming wave */
#endif
// the counted waits (every slot is four vector-memory operations): BV_F_W_ALL -- at most the K slots in flight are outstanding;
// BV_F_W_OLDEST -- the oldest of K slots has landed; _1 / _3 -- the same with one / three younger stores outstanding.
// (Round 6 tried counts kept per slot -- a slot of the tagged pass-2 rows then needs no fourth, one-lane load -- with the wait picked
// by a chain of scalar compares: the chain cost 4-5 % of the launch, the saved loads gained nothing measurable.  Not kept.)
#if BV_F_K == 3
#define BV_F_W_ALL "s_waitcnt vmcnt(12)"
#define BV_F_W_OLDEST "s_waitcnt vmcnt(8)"
#define BV_F_W_OLDEST_1 "s_waitcnt vmcnt(9)"
#define BV_F_W_OLDEST_3 "s_waitcnt vmcnt(11)"
#elif BV_F_K == 2
#define BV_F_W_ALL "s_waitcnt vmcnt(8)"
#define BV_F_W_OLDEST "s_waitcnt vmcnt(4)"
#define BV_F_W_OLDEST_1 "s_waitcnt vmcnt(5)"
#define BV_F_W_OLDEST_3 "s_waitcnt vmcnt(7)"
#elif BV_F_K == 4
#define BV_F_W_ALL "s_waitcnt vmcnt(16)"
#define BV_F_W_OLDEST "s_waitcnt vmcnt(12)"
#define BV_F_W_OLDEST_1 "s_waitcnt vmcnt(13)"
#define BV_F_W_OLDEST_3 "s_waitcnt vmcnt(15)"
#else
#error "BV_F_K: 2, 3 or 4 ring slots"
#endif
// -DBV_TEAM_DEBUG -DBV_PHASE_DEBUG: where the streaming waves' cycles go (s_memtime around the phases of a slot, summed over
// the launch's waves in units of 16 cycles; printed by bv_engine_wait with the [fused debug] lines)
#ifdef BV_PHASE_DEBUG
#define BV_PH_DECL uint32_t ph_[24]; for (int i_ = 0; i_ < 24; ++i_) ph_[i_] = 0u; uint32_t ph_t_ = (uint32_t)__builtin_amdgcn_s_memtime(); const uint32_t ph_t0_ = ph_t_; uint32_t ph_i0_ = 0, ph_i1_ = 0, ph_i2_ = 0, ph_n1_ = 0, ph_n2_ = 0
#define BV_PH(i) do { const uint32_t n_ = (uint32_t)__builtin_amdgcn_s_memtime(); ph_[(i) + ((st & BV_FS_P1_FIN) ? 12 : 0)] += n_ - ph_t_; ph_t_ = n_; } while (0)
#define BV_PH_COUNT(i) (++ph_[(i) + ((st & BV_FS_P1_FIN) ? 12 : 0)])
#define BV_PH_FLUSH(ctr, lane) do { ph_[9] = (uint32_t)__builtin_amdgcn_s_memtime() - ph_t0_; ph_[11] = ph_i1_; ph_[23] = ph_i2_; if ((lane) == 0) { atomicAdd(&(ctr)[BV_CTR_WORDS + 4244], ph_n1_); atomicAdd(&(ctr)[BV_CTR_WORDS + 4245], ph_n2_); } if ((lane) == 0) for (int i_ = 0; i_ < 24; ++i_) atomicAdd(&(ctr)[BV_CTR_WORDS + 4220 + i_], (i_ % 12) == 7 ? ph_[i_] : ph_[i_] >> 4); } while (0)
#else
#define BV_PH_DECL
#define BV_PH(i)
#define BV_PH_COUNT(i)
#define BV_PH_FLUSH(ctr, lane)
#endif
#define BV_F_SLOT_WORDS 1024              /* pass-1 rows: 2 KiB of calls, 2 KiB of phreds; pass-2 rows: 1 KiB of calls, 1 KiB of mapq, 2 KiB of ranks */
#define BV_F_QCAP 256                     /* entries per candidate queue (ring buffers) */
#define BV_F_QVCAP 128                    /* entries of the variant queue */
#define BV_F_EMPTY 0xFFFFFFFFu
// Every wait on another wave's LDS write is bounded (~1-2 s of s_sleep): a wave that gives up sets the sticky BV_CTR_TIMEOUT
// counter -- the submit then fails loudly in bv_engine_wait -- instead of hanging the GPU on a protocol error.
#define BV_F_SPIN_MAX (1u << 22)
// No issue priorities (s_setprio).  Round 4 ran the solver waves at priority 3: their chains of dependent FP64 operations lost
// 2-3 x beside two streaming waves per SIMD at equal priority (28 candidates waiting at the end of the pass-1 rows against 1).
// What they were really losing to was scratch memory -- reloads of hoisted loop invariants inside those chains, a memory trip
// each (round 5, see bv_f_stream_until_idle and the kernel's loop).  With those gone the priority COSTS: equal priorities
// measured +3 % at 100 k sites (187 against 181 M sites/s, eight interleaved pairs), +4 % at 524 k (200-207 against 192-201);
// streaming waves above the solvers (2 over 0) +2 %, (3 over 1) -1 %.
#define BV_F_MIN_JOB 4u                   /* sites per job of the 16-lane solver while rows are still streaming */
// control words in LDS
#define BV_FC_CURSOR 0                    /* sites of the workgroup's range handed out so far */
#define BV_FC_Q3_TAIL 1                   /* candidates with >= 3 active bases: reserved / claimed positions */
#define BV_FC_Q3_HEAD 2
#define BV_FC_Q2_TAIL 3                   /* candidates with <= 2 active bases */
#define BV_FC_Q2_HEAD 4
#define BV_FC_QH_TAIL 5                   /* candidates for the wave solver: entries of the workgroup's slice of cand_list (HBM) */
#define BV_FC_QH_HEAD 6
#define BV_FC_BLK_HEAD 7                  /* blocks of 64 sites (non-candidates) claimed */
#define BV_FC_NDONE 8                     /* streaming waves that have published their last pass-1 row */
#define BV_FC_QV_TAIL 9                   /* variant sites whose rank-sum rows (pass 2) are to be streamed */
#define BV_FC_QV_HEAD 10
#define BV_FC_BUSY 11                     /* solver jobs in flight (each may still add to the variant queue) */
#define BV_FC_OV_TAIL 12                  /* variant sites that did not fit the LDS queue: entries of the workgroup's overflow list (HBM) written */
#define BV_FC_OV_HEAD 13                  /* ... and claimed by streaming waves */
#define BV_FC_OV_LOCK 14                  /* one producer wave at a time appends to the list */
// (A workgroup owns a contiguous range of sites.  Dealing the launch's last eighth in 16-site chunks from a global counter --
// the XCDs stream at rates 7 % apart -- was built and measured in round 4: the pass-1 rows end within 21 us instead of 30, but
// the median moves up by as much and the launch ends with its last VARIANT rows, which stay local: 166-174 against 175-176 M
// sites/s.  docs/history/DESIGN_round4.md.)
// a streaming wave's flags that outlive a call of bv_f_stream_until_idle
#define BV_FS_P_DONE 1u                   /* no row will ever come again */
#define BV_FS_CUR_DONE 8u                 /* the cursor is exhausted */
#define BV_FS_P1_FIN 16u                  /* the wave's last pass-1 row is published, the wave counted in NDONE */
// kinds of rows in a streaming wave's ring
#define BV_FK_P1 1u                       /* calls + phreds of a site: the pass-1 tally */
#define BV_FK_P2 2u                       /* calls + mapq + ranks of a variant site: the two rank sums of pass 2 */

union __attribute__((aligned(16))) BvFusedRing {
    uint32_t slot[BV_F_K][BV_F_SLOT_WORDS];
    struct {                                  // while the wave has no row in flight
        BvP1sWaveScratch ws;
        uint32_t vl[64];
    } solve;
};
struct __attribute__((aligned(16))) BvFusedShared {
    uint32_t hist[BV_F_NS][BV_S_HWORDS + BV_S_OVF + 8];  // per streaming wave: [(rev<<2)|base][phred < 128], overflow rows; pass-2 rows: hm[2][256], hr[2][256]
    BvFusedRing ring[BV_F_NS];
    uint32_t grp[BV_F_NV][4][BV_G16_GRP_WORDS];          // the solver waves' group scratches
    uint32_t vl[BV_F_NV][64];                            // ... and their variant sites since the last flush
    double tab_hit[BV_QBINS], tab_miss[BV_QBINS];
    double tab_loghit[BV_QBINS], tab_logmiss[BV_QBINS];  // (from HBM these cost the 16-lane solver a memory trip per slot of bins)
    uint32_t stage[BV_F_NS][128];                        // a candidate's compacted bins on their way out
    uint32_t q3[BV_F_QCAP], q2[BV_F_QCAP];
    uint32_t qv[BV_F_QVCAP][4];                          // site, class table, n_ref | n_alt << 16, 2-bit lut
    uint32_t pub[BV_F_NS];                               // every pass-1 row of wave w below site pub[w] is published
    uint32_t ctl[16];
};
static_assert(sizeof(BvFusedShared) <= 160 * 1024, "one workgroup per CU must fit the LDS");
static_assert(4 * BV_G16_GRP_WORDS >= BV_S_HWORDS, "a solver wave's group scratch serves as its rank-sum histogram (bv_f_p2_rows)");
static_assert(BV_F_K < 3 || sizeof(BvFusedRing) == sizeof(uint32_t) * BV_F_K * BV_F_SLOT_WORDS, "the solver scratch must fit the ring");
