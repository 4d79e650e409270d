// ll_reg_solve_fast.h -- everything solve_fast3, the Mid-40 solver, is made of (device only, no kernel, no host code).
// Included by ll_reg_solve_kernels.hip (reg_solve_kernel; ll_reg_big_path.h and ll_reg_solve_general.h share SolveShared, the block
// sums, plane_table_reload and HASH_EMPTY / HT_* / hash64) and by ll_reg_maps_kernels.hip (reg_solve_maps_kernel).
//
// ONE workgroup per scan (a group of LL_GRP workgroups per scan for batches of <= 16 scans, group_barrier / group_reduce below)
// runs what the reference does between point_cloud_registration.hpp:460 and :531: the 2-iteration prerun solve, the loss-corrected
// L1 evaluation, the std::set-deduplicated 80-th percentile inlier threshold (:153-161), the prune, the final solve and the pose
// composition -- replacing ceres::Solve / Problem::Evaluate by a 28-value (21 H + 6 g + 1 cost) workgroup reduction and a
// Levenberg-Marquardt controller on the first wavefront.  No host round trip per iteration.  solve_fast3 holds every scan within
// FAST_MAX_BLOCKS without motion deblur: plane table in LDS, 18 B streamed per plane block, 64-bit activity masks and register
// tiles.  In order: evaluation-context and timing macros, SolveShared, the group barrier and reduction, block sums, capacities,
// inlier_threshold_regs, BlkRegs / load_blk, census_and_plane_table, plane_table_reload, solver_eval3, solver_lm3, inlier_phase3,
// solve_fast3, and the prologue both kernels share (SolveTicket, solve_fast_ticket, solve_fast_check, solve_fast_group_fields).
//
// No MFMA: 6x6 systems are reduced, not multiplied.  Line blocks live in HBM as 65 B; every cost evaluation streams the part of
// the blocks that does not fit the LDS record cache.
#pragma once
#include <hip/hip_runtime.h>

#include "ll_reg_query.h"
#include "ll_reg_solve_common.h"

namespace ll {

#define RS_WAVES (RS_THREADS / 64)

// Evaluation context as plain locals (R_inc / t_inc for the plain blocks, axis-angle for the motion-deblur ones);
// DEBLUR is a template constant, so the unused half disappears from each kernel instantiation.
#define LL_CTX_DECL(x)                                   \
    double R_[9], t_[3];                                  \
    MbRot mb_;                                            \
    {                                                     \
        const double q_[4] = {(x)[0], (x)[1], (x)[2], (x)[3]}; \
        quat_to_mat(q_, R_);                              \
        t_[0] = (x)[4];                                   \
        t_[1] = (x)[5];                                   \
        t_[2] = (x)[6];                                   \
        if (DEBLUR) mb_prepare(q_, mb_);                  \
    }
#define LL_CTX_ACCUM(kind, ff, a, v, huber_a, acc)                                                        \
    do {                                                                                                  \
        const double f_[3] = {(double)(ff).x, (double)(ff).y, (double)(ff).z};                            \
        if (DEBLUR)                                                                                       \
            block_accumulate_mb((kind), mb_, t_, (double)(ff).w, f_, (a), (v), (huber_a), (acc)); /* ICP:81-233 */ \
        else                                                                                              \
            block_accumulate((kind), R_, t_, f_, (a), (v), (huber_a), (acc)); /* ICP:238-380 */           \
    } while (0)
#define LL_CTX_L1(out, kind, ff, a, v, huber_a, q_last)                                                   \
    do {                                                                                                  \
        const double f_[3] = {(double)(ff).x, (double)(ff).y, (double)(ff).z};                            \
        if (DEBLUR)                                                                                       \
            (out) = block_l1_mb((kind), mb_, t_, (double)(ff).w, f_, (a), (v), (huber_a), (q_last));      \
        else                                                                                              \
            (out) = block_l1((kind), R_, t_, f_, (a), (v), (huber_a), (q_last));                          \
    } while (0)

// ---------------------------------------------------------------------------------------------------------
#ifdef LL_SOLVE_TIMING
#define LL_T0(var) long long var = clock64()
#define LL_TACC(slot, var)                                   \
    do {                                                     \
        if (threadIdx.x == 0) sh.tcyc[slot] += clock64() - var; \
    } while (0)
#else
#define LL_T0(var)
#define LL_TACC(slot, var)
#endif

struct SolveShared {
    long long tcyc[16];
    LmCtl ctl;
    double red[RS_WAVES][LL_NACC];
    double sum[LL_NACC];
    int need;
    int hist[256];
    int sel_bin, sel_cnt, n_cand;
    int isum[RS_WAVES];
    unsigned long long lsum[RS_WAVES];
    unsigned long long sel_prefix;
    int sel_rank;
    int n_active, n_corner_avail, n_surf_avail, n_unique;
    int l1_valid;  // compact path: blk_l1 holds the L1 values at the prerun result (written by its last evaluation)
    int pt_T, pt_Tl, pt_kc, pt_priv;  // plane-table path: distinct triples, table entries in LDS, record rounds cached in LDS, private entries
    double fit[10];                   // arguments of a line search's three-sample fit, from the controller lane to its wavefront
    int pt_nl;                        // ... line blocks of this workgroup's first rounds kept at the top of s_raw (solver_eval3)
    double thr;
    int grp_g, grp_G, grp_seq, grp_abort;  // grouped solver: this workgroup's rank in its scan's group, the group size, barriers passed
    int xch_seq, xch_epoch;                // ... exchanges of partial sums made in this launch, and the launch's number in its registration (granule tags)
    unsigned int xch[LL_GRP][2 * LL_NACC]; // ... the members' partial sums of one exchange, as 32-bit halves
};

// ---- grouped solver (small batches) ------------------------------------------------------------------------------------
// With one workgroup per scan a batch of B <= 16 scans keeps B of 256 CUs busy and every cost evaluation re-streams the 85 %
// of the scan's block records that do not fit one CU's LDS.  For such batches a scan is given to a GROUP of LL_GRP
// workgroups: every workgroup runs the whole control flow redundantly on the same numbers (census, LM controller, set
// de-duplication, rank select, prune: all deterministic), but a cost evaluation visits only the workgroup's 1/G share of the
// blocks -- which then fits its LDS record cache, so nothing is streamed after the first evaluation -- and the 28 partial sums
// are exchanged through global memory and added in rank order by every member (identical totals, identical decisions).
// Membership is by ticket (atomic counter, zeroed per launch): the G workgroups of a group are by construction running, so the
// flag barrier below cannot wait for a workgroup that has no CU; a partial group waits only for workgroups that start as CUs
// free up.  Spins are bounded: a barrier that does not complete aborts the scan's registration (RegState::aborted: the
// scan comes back rejected with its pose restored and ll_reg_collect reports the failure) instead of hanging the device.
#define LL_GRP_SPIN_LIMIT (1 << 22)
// FULL: every thread's plain global stores before the barrier (the L1 values) are visible to every member after it, and no
// member keeps stale lines -- an agent-scope release / acquire fence in every wavefront.  Otherwise only data moved with
// agent-scope atomics by the calling threads themselves is exchanged (the partial sums) and the barrier is just the counter.
template <bool FULL>
__device__ __forceinline__ void group_barrier(const RegDev &rd, int b, SolveShared &sh)
{
    if (FULL) __threadfence();
    __syncthreads();
    if (threadIdx.x == 0 && !sh.grp_abort) {
        const int target = (++sh.grp_seq) * sh.grp_G;
        int *bar = rd.grp_ctl + 1 + 2 * b, *abt = bar + 1;  // the scan's arrival counter and its abort word
        __hip_atomic_fetch_add(bar, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        int spins = 0;
        while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            // a member that gives up tells the others: they must not go on with its stale partial sums, nor wait out their own
            // limit for arrivals that will never come
            if (++spins > LL_GRP_SPIN_LIMIT || ((spins & 1023) == 0 && __hip_atomic_load(abt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                sh.grp_abort = 1;
                __hip_atomic_store(abt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
        if (!sh.grp_abort && __hip_atomic_load(abt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) sh.grp_abort = 1;
    }
    __syncthreads();  // (the partial sums are then read with agent-scope atomic loads, which no cache level may satisfy stale)
    if (FULL) __threadfence();
}

// sh.sum (this workgroup's share) -> sh.sum (the scan's totals), the same value in every member.
// FULL (the one evaluation per launch that also publishes the L1 values): partial sums through rd.grp_part behind the counter
// barrier with its fences.  Otherwise (every other evaluation, ~8 per launch) a fence-free exchange of self-validating
// GRANULES (MI355X_MICROARCH.md, hand-off price list: 8-byte {data, tag} written by one agent-scope store, polled with
// agent-scope loads -- about one memory round trip, against four for store / release / counter / poll / load): every double
// travels as two granules {32-bit half, tag}, tag = launch epoch << 12 | exchange number, so a reader that sees the tag has
// the data and nothing needs ordering.  Slots alternate by exchange parity: a member that posts exchange s + 2 has read all
// of s + 1, which every member posted only after reading all of s.  rd.grp_xch is zeroed per registration and the epoch is the
// ICP iteration, so no tag repeats while a stale granule could still be seen.  Bounded polling like the barrier: a member
// that gives up (or runs out of exchange numbers) raises the scan's abort word, the others see it.
template <bool FULL>
__device__ __forceinline__ void group_reduce(const RegDev &rd, int b, SolveShared &sh)
{
    const int tid = threadIdx.x, G = sh.grp_G;
    if (FULL) {
        double *part = rd.grp_part + ((size_t)b * 2 + (sh.grp_seq & 1)) * LL_GRP * LL_NACC;
        if (tid < LL_NACC) __hip_atomic_store(part + sh.grp_g * LL_NACC + tid, sh.sum[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        group_barrier<true>(rd, b, sh);
        if (tid < LL_NACC) {
            double t = 0.0;
            for (int k = 0; k < G; k++) t += __hip_atomic_load(part + k * LL_NACC + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sh.sum[tid] = t;
        }
        __syncthreads();
        return;
    }
    constexpr int NG = 2 * LL_NACC;  // granules per member
    static_assert(LL_GRP * NG <= RS_THREADS, "one polling thread per granule");
    if (tid == 0) sh.xch_seq++;
    __syncthreads();  // (sh.sum is complete; grp_abort as the last exchange left it)
    const int seq = sh.xch_seq;
    if (!sh.grp_abort && seq < 4096) {  // uniform
        const unsigned int tag = ((unsigned int)sh.xch_epoch << 12) | (unsigned int)seq;
        unsigned long long *slot = rd.grp_xch + ((size_t)b * 2 + (seq & 1)) * LL_GRP * NG;
        if (tid < NG) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(sh.sum[tid >> 1]);
            const unsigned int half = (tid & 1) ? (unsigned int)(bits >> 32) : (unsigned int)bits;
            __hip_atomic_store(slot + sh.grp_g * NG + tid, ((unsigned long long)tag << 32) | (unsigned long long)half, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        if (tid < G * NG) {
            const int *abt = rd.grp_ctl + 2 + 2 * b;
            unsigned long long v = __hip_atomic_load(slot + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int spins = 0;
            while ((unsigned int)(v >> 32) != tag) {
                if (++spins > LL_GRP_SPIN_LIMIT || ((spins & 1023) == 0 && __hip_atomic_load(abt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                    sh.grp_abort = 1;  // (any thread may raise it; read again behind the barrier below)
                    __hip_atomic_store(const_cast<int *>(abt), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
                v = __hip_atomic_load(slot + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            sh.xch[tid / NG][tid % NG] = (unsigned int)v;
        }
    } else if (tid == 0 && !sh.grp_abort) {  // out of exchange numbers: fail loudly rather than reuse a tag
        sh.grp_abort = 1;
        __hip_atomic_store(rd.grp_ctl + 2 + 2 * b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (tid < LL_NACC && !sh.grp_abort) {  // (after an abort the sums stay the member's own: nothing of this launch is kept)
        double t = 0.0;
        for (int k = 0; k < G; k++)
            t += __longlong_as_double((long long)(((unsigned long long)sh.xch[k][2 * tid + 1] << 32) | (unsigned long long)sh.xch[k][2 * tid]));
        sh.sum[tid] = t;
    }
    __syncthreads();
}

// three counts (each < 2^20) in one reduction: a | b << 20 | c << 40
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, SolveShared &sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_down((long long)v, off);
    if (lane == 0) sh.lsum[wave] = v;
    __syncthreads();
    unsigned long long s = 0;
    for (int w = 0; w < RS_WAVES; w++) s += sh.lsum[w];
    __syncthreads();
    return s;
}

__device__ int block_sum_int(int v, SolveShared &sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) sh.isum[wave] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < RS_WAVES; w++) s += sh.isum[w];
    __syncthreads();
    return s;
}

__device__ __forceinline__ unsigned long long hash64(unsigned long long k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}



// capacities shared by the solver paths (solve_fast3 here, solve_big; the plane table is described further down)
#define FAST_MAXK (FAST_MAX_BLOCKS / RS_THREADS)
#define HASH_EMPTY 0xffffffffffffffffull  // empty slot of the de-duplication hash tables (here, solve_big, solve_general)
#define HT_SIZE 16384
#define HT_PART 6144  // keys per de-duplication round (load factor <= 0.375)
// register-tile de-duplication (inlier_threshold_regs): 2-bit slot states, 64 KB + 32 KB, and a list of twice-contested keys
#define DD2_WORDS 16384
#define DD2_SLOTS (DD2_WORDS * 16)
#define DD2B_WORDS 8192
#define DD2B_SLOTS (DD2B_WORDS * 16)
#define DD2_LIST 2048  // twice-contested keys compared exactly; more (heavily duplicated input): hash every key instead
#define SEL_BINS 4096  // value-range bins of the rank select (must be a multiple of RS_THREADS)
#define SEL_CAND 1024  // keys of the selected bin ranked exactly; more -> radix-select fallback


// std::set de-duplication + rank select of the loss-corrected L1 values held in registers (l1r[k] = value of the
// thread's k-th block, < 0 for "no active block"): sets sh.thr = max(inliner_dis, element at int(ratio * n_distinct))
// (PCR:153-161, 484-485).  `total` only sizes the rounds of the heavily-duplicated fallback.
template <int NK>
__device__ __forceinline__ void inlier_threshold_regs(const double (&l1r)[NK], int total, unsigned long long *s_table, SolveShared &sh,
                                                      const RegConst &rc)
{
    static_assert(NK <= 64 && NK <= FAST_MAXK, "register tile of the fast paths (one bit per entry in the 64-bit masks)");
    const int tid = threadIdx.x;
    LL_T0(t_dd);
    // ---- std::set semantics (PCR:155-160): which values are distinct, and how many ---------------------------------
    // Exact duplicates among the residuals are rare, so the common case is made cheap (passes A - C below); heavily
    // duplicated inputs (more than DD2_LIST twice-contested keys) fall back to hashing every key, HT_PART keys per round.
    unsigned long long first_mask = 0;  // bit k: block k of this thread is the first occurrence of its L1 value
    {
        // Common case.  Three short, branch-light passes over the thread's keys instead of a
        // compare-and-swap probe per key (round 1: ~290 instructions per key once the compiler had unrolled the probe loop):
        //   A  every key marks a 2-bit slot state {bit 0: a key landed here, bit 1: a second key landed here} in a
        //      256 K-slot table (atomicOr): a key whose slot never gets bit 1 is distinct from every other key;
        //   B  the keys of contested slots (hash collisions and true duplicates, ~1100 of ~17 k) repeat that in a second
        //      table under an independent hash: distinct keys that merely collided in A almost surely separate here;
        //   C  what is contested twice -- true duplicates plus a stray pair -- is appended to a short list and compared
        //      exactly, each entry against the entries before it.
        // Slot hashes are two 32-bit multiplies.  Heavily duplicated inputs (list overflow) take the table path below.
        int my = 0;
        unsigned int *bmA = (unsigned int *)s_table;                       // [DD2_WORDS]  16 slots x 2 bits per word, 64 KB
        unsigned int *bmB = bmA + DD2_WORDS;                               // [DD2B_WORDS] second table, 32 KB
        unsigned long long *dl = (unsigned long long *)(bmB + DD2B_WORDS); // [DD2_LIST] twice-contested keys
        {
            uint4 *z = (uint4 *)s_table;
            for (int e = tid; e < (DD2_WORDS + DD2B_WORDS) / 4; e += RS_THREADS) z[e] = make_uint4(0u, 0u, 0u, 0u);
            if (tid == 0) sh.n_cand = 0;
        }
        __syncthreads();
        const int kt = (total + RS_THREADS - 1) / RS_THREADS;  // rounds that can hold a block (uniform)
        // slot hashes are recomputed in each pass (two 32-bit multiplies) rather than kept: with l1r[48] live, another 48
        // registers per thread made the compiler spill half of l1r to scratch, and every later pass paid for it
        auto slot_a = [](unsigned long long key) -> unsigned int {
            unsigned int h = (unsigned int)key * 0x9E3779B1u;
            h ^= h >> 15;
            h += (unsigned int)(key >> 32) * 0x85EBCA77u;
            h ^= h >> 13;
            return h & (DD2_SLOTS - 1);
        };
        auto slot_b = [](unsigned long long key) -> unsigned int {
            unsigned int h2 = ((unsigned int)(key >> 32) * 0xC2B2AE3Du) ^ ((unsigned int)key * 0x27D4EB2Fu);
            return (h2 ^ (h2 >> 16)) & (DD2B_SLOTS - 1);
        };
        unsigned long long valid_mask = 0, cont_mask = 0;
#pragma unroll
        for (int k = 0; k < NK; k++) {
            if (k >= kt) continue;  // not `break`: an early exit keeps the loop rolled and the register tile in scratch
            const double l1 = l1r[k];
            const bool valid = l1 >= 0.0;  // inactive slot or NaN (NaN never enters the set)
            const unsigned int slot = slot_a((unsigned long long)__double_as_longlong(l1));
            const unsigned int bit0 = valid ? (1u << ((slot & 15u) * 2u)) : 0u;  // 0: a harmless no-op for padding lanes
            const unsigned int old = atomicOr(&bmA[slot >> 4], bit0);
            atomicOr(&bmA[slot >> 4], (old & bit0) << 1);
            if (valid) valid_mask |= 1ull << k;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NK; k++) {
            if (k >= kt) continue;  // not `break`: an early exit keeps the loop rolled and the register tile in scratch
            const unsigned long long key = (unsigned long long)__double_as_longlong(l1r[k]);
            const unsigned int slot = slot_a(key);
            const bool contested = ((valid_mask >> k) & 1ull) && ((bmA[slot >> 4] >> ((slot & 15u) * 2u)) & 2u);
            const unsigned int h2 = slot_b(key);
            const unsigned int bit0 = contested ? (1u << ((h2 & 15u) * 2u)) : 0u;
            const unsigned int old = atomicOr(&bmB[h2 >> 4], bit0);
            atomicOr(&bmB[h2 >> 4], (old & bit0) << 1);
            if (contested) cont_mask |= 1ull << k;
        }
        __syncthreads();
        unsigned long long twice_mask = 0;
#pragma unroll
        for (int k = 0; k < NK; k++) {
            if (k >= kt) continue;  // not `break`: an early exit keeps the loop rolled and the register tile in scratch
            const unsigned int h2 = slot_b((unsigned long long)__double_as_longlong(l1r[k]));
            if (((cont_mask >> k) & 1ull) && ((bmB[h2 >> 4] >> ((h2 & 15u) * 2u)) & 2u)) twice_mask |= 1ull << k;
        }
        // every valid key that is not contested twice is distinct; the rest go through the exact list
        my = __popcll(valid_mask & ~twice_mask);
        first_mask = valid_mask & ~twice_mask;
        int my_pos[2] = {-1, -1};  // list positions of this thread's twice-contested keys (more than two: overflow)
        int n_twice = __popcll(twice_mask);
        if (twice_mask) {
            int got = 0;
#pragma unroll
            for (int k = 0; k < NK; k++) {
                if (!((twice_mask >> k) & 1ull)) continue;
                const int pos = atomicAdd(&sh.n_cand, 1);
                if (pos < DD2_LIST) dl[pos] = (unsigned long long)__double_as_longlong(l1r[k]);
                if (got < 2) my_pos[got] = pos;
                got++;
            }
        }
        const int over = block_sum_int(n_twice > 2 ? 1 : 0, sh);  // its barriers also publish the list
        const int n_list = sh.n_cand;
        if (n_list <= DD2_LIST && over == 0) {
            if (twice_mask) {
                int got = 0;
#pragma unroll
                for (int k = 0; k < NK; k++) {
                    if (!((twice_mask >> k) & 1ull)) continue;
                    const int pos = my_pos[got < 2 ? got : 1];
                    got++;
                    const unsigned long long key = (unsigned long long)__double_as_longlong(l1r[k]);
                    bool dup = false;
                    for (int j = 0; j < pos; j++) dup |= (dl[j] == key);
                    if (!dup) {
                        first_mask |= 1ull << k;
                        my++;
                    }
                }
            }
        } else {
            first_mask = 0;
            my = 0;
            const int rounds = (total + HT_PART - 1) / HT_PART;
            for (int rnd = 0; rnd < rounds; rnd++) {
                __syncthreads();
                for (int e = tid; e < HT_SIZE; e += RS_THREADS) s_table[e] = HASH_EMPTY;
                __syncthreads();
#pragma unroll
                for (int k = 0; k < NK; k++) {
                    const double l1 = l1r[k];
                    if (!(l1 >= 0.0)) continue;
                    const unsigned long long key = (unsigned long long)__double_as_longlong(l1);
                    const unsigned long long hk = hash64(key);
                    if ((int)((hk >> 40) % (unsigned long long)rounds) != rnd) continue;
                    unsigned int h = (unsigned int)hk & (HT_SIZE - 1);
                    for (;;) {
                        const unsigned long long old = atomicCAS(&s_table[h], HASH_EMPTY, key);
                        if (old == HASH_EMPTY) {
                            first_mask |= (1ull << k);
                            my++;
                            break;
                        }
                        if (old == key) break;
                        h = (h + 1u) & (HT_SIZE - 1);
                    }
                }
            }
        }
        const int nu = block_sum_int(my, sh);
        if (tid == 0) {
            sh.n_unique = nu;
            sh.sel_prefix = 0ull;
            int target = (int)(rc.inlier_ratio * (double)nu);  // PCR:160
            if (target > nu - 1) target = nu - 1;
            sh.sel_rank = target;
        }
        __syncthreads();
    }
    LL_TACC(3, t_dd);
    LL_T0(t_sel);
    if (sh.n_unique > 0) {
        // Rank select of the distinct values.  One histogram pass over SEL_BINS value-range bins (a monotone map, so
        // every key in a lower bin is smaller) finds the bin that holds the wanted rank; its few keys are ranked
        // exactly against each other.  An 8-bit radix select over the same keys is the fallback when that bin is
        // crowded (heavily clustered values).
        int *bins = (int *)s_table;                                      // [SEL_BINS]
        unsigned long long *cand = s_table + SEL_BINS / 2;               // [SEL_CAND] keys of the selected bin
        double kmin = INFINITY, kmax = -INFINITY;
#pragma unroll
        for (int k = 0; k < NK; k++)
            if (first_mask & (1ull << k)) {
                kmin = fmin(kmin, l1r[k]);
                kmax = fmax(kmax, l1r[k]);
            }
        for (int off = 32; off > 0; off >>= 1) {
            kmin = fmin(kmin, __shfl_down(kmin, off));
            kmax = fmax(kmax, __shfl_down(kmax, off));
        }
        if ((tid & 63) == 0) {
            sh.red[tid >> 6][0] = kmin;
            sh.red[tid >> 6][1] = kmax;
        }
        for (int e = tid; e < SEL_BINS; e += RS_THREADS) bins[e] = 0;
        __syncthreads();
        double lo = sh.red[0][0], hi = sh.red[0][1];
        for (int w = 1; w < RS_WAVES; w++) {
            lo = fmin(lo, sh.red[w][0]);
            hi = fmax(hi, sh.red[w][1]);
        }
        const double scale = (hi > lo) ? (double)(SEL_BINS - 1) / (hi - lo) : 0.0;
#pragma unroll
        for (int k = 0; k < NK; k++)
            if (first_mask & (1ull << k)) {
                int bi = (int)((l1r[k] - lo) * scale);
                bi = bi < 0 ? 0 : (bi > SEL_BINS - 1 ? SEL_BINS - 1 : bi);
                atomicAdd(&bins[bi], 1);
            }
        __syncthreads();
        // locate the bin of the wanted rank: every thread sums its SEL_BINS/RS_THREADS consecutive bins, a workgroup
        // prefix sum (wave scan + the eight wave totals) gives each thread the count below its first bin, and the one
        // thread whose range holds the rank walks its own few bins
        {
            const int per = SEL_BINS / RS_THREADS;
            const int lane = tid & 63, wave = tid >> 6;
            int part = 0;
            for (int e = 0; e < per; e++) part += bins[tid * per + e];
            int incl = part;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int y = __shfl_up(incl, off);
                if (lane >= off) incl += y;
            }
            if (lane == 63) sh.isum[wave] = incl;
            if (tid == 0) sh.n_cand = 0;
            __syncthreads();
            int below = incl - part;
            for (int w = 0; w < wave; w++) below += sh.isum[w];
            const int rank = sh.sel_rank;
            __syncthreads();  // everyone has read sel_rank / isum before the owner overwrites sel_rank
            const bool last_thread = tid == RS_THREADS - 1;
            if ((rank >= below && rank < below + part) || (last_thread && rank >= below + part)) {
                int cum = below, bi = tid * per;
                for (; bi < tid * per + per - 1; bi++) {
                    if (cum + bins[bi] > rank) break;
                    cum += bins[bi];
                }
                sh.sel_bin = bi;
                sh.sel_rank = rank - cum;  // rank inside the bin
                sh.sel_cnt = bins[bi];
            }
            __syncthreads();
        }
        if (sh.sel_cnt <= SEL_CAND) {
            const int sel_bin = sh.sel_bin;
#pragma unroll
            for (int k = 0; k < NK; k++)
                if (first_mask & (1ull << k)) {
                    int bi = (int)((l1r[k] - lo) * scale);
                    bi = bi < 0 ? 0 : (bi > SEL_BINS - 1 ? SEL_BINS - 1 : bi);
                    if (bi == sel_bin) cand[atomicAdd(&sh.n_cand, 1)] = (unsigned long long)__double_as_longlong(l1r[k]);
                }
            __syncthreads();
            const int m = sh.n_cand;  // == sel_cnt
            for (int i = tid; i < m; i += RS_THREADS) {
                const unsigned long long ki = cand[i];
                int rk = 0;
                for (int j = 0; j < m; j++) rk += (cand[j] < ki) ? 1 : 0;  // keys are distinct
                if (rk == sh.sel_rank) sh.sel_prefix = ki;
            }
            __syncthreads();
        } else {
            // crowded bin: MSB-first radix select (8 bits per pass) restricted to the keys of that bin
            const int sel_bin = sh.sel_bin;
            if (tid == 0) sh.sel_prefix = 0ull;
            __syncthreads();
            for (int pass = 0; pass < 8; pass++) {
                const int shift = 56 - 8 * pass;
                for (int e = tid; e < 256; e += RS_THREADS) sh.hist[e] = 0;
                __syncthreads();
                const unsigned long long prefix = sh.sel_prefix;
#pragma unroll
                for (int k = 0; k < NK; k++) {
                    if (!(first_mask & (1ull << k))) continue;
                    int bi = (int)((l1r[k] - lo) * scale);
                    bi = bi < 0 ? 0 : (bi > SEL_BINS - 1 ? SEL_BINS - 1 : bi);
                    if (bi != sel_bin) continue;
                    const unsigned long long key = (unsigned long long)__double_as_longlong(l1r[k]);
                    if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&sh.hist[(int)((key >> shift) & 255ull)], 1);
                }
                __syncthreads();
                if (tid == 0) {
                    int rank = sh.sel_rank, d = 0, cum = 0;
                    for (d = 0; d < 256; d++) {
                        if (cum + sh.hist[d] > rank) break;
                        cum += sh.hist[d];
                    }
                    if (d > 255) d = 255;
                    sh.sel_rank = rank - cum;
                    sh.sel_prefix = (prefix << 8) | (unsigned long long)d;
                }
                __syncthreads();
            }
        }
        if (tid == 0) sh.thr = fmax(rc.inliner_dis, __longlong_as_double((long long)sh.sel_prefix));  // PCR:485
    } else {
        if (tid == 0) sh.thr = rc.inliner_dis;  // empty set: defined deviation (PCR:160 would dereference end())
    }
    __syncthreads();
    LL_TACC(4, t_sel);
}

// a block's fp64 record as it lies in HBM: the line blocks (65 B) of solver_eval3, inlier_phase3 and solve_big; the plane blocks go
// through the plane table below
struct BlkRegs {
    float4 f;
    double a0, a1, a2, v0, v1, v2;
};

__device__ __forceinline__ void load_blk(const RegDev &rd, size_t sb, const double *av, int slot, BlkRegs &r)
{
    r.f = gload_f4(rd.blk_f + sb + slot);
    // surface slots hold plane blocks: a' is folded into the scalar a0 = n'.a' (ll_reg_core.h block_plane)
    av_load(av, rd.cap, slot, slot < rd.cap_c, r.a0, r.a1, r.a2, r.v0, r.v1, r.v2);
}


// ---------------------------------------------------------------------------------------------------------
// PLANE TABLE (every scan solve_fast3 holds).  A scan's ~17 k plane blocks are built from only 2.4 - 4.6 k
// distinct ordered (nn0, nn2, nn4) neighbour triples (the queries of a wall patch share their nearest map points), and every
// block with the same triple carries bit-identical {n', c} -- 32 of the 48 bytes a per-block record form re-streams on each of ~7 cost
// evaluations.  Here the solver workgroup de-duplicates the triples itself at the start of every launch:
//   1. census: block flags -> a 64-bit activity mask per thread (bit k <-> block tid + k * 512 in the planes / padding / lines
//      order; no flag array in LDS);
//   2. every active plane block's triple (rd.nn) goes into an LDS hash table of 8192 16-byte slots: the key is claimed with a
//      64-bit compare-and-swap on {p0, p1} and a 32-bit one on p2 -- whoever loses either moves on to the next slot, nobody
//      ever waits for another lane -- and the slot index stays in the thread's registers (a thread owns at most 48 blocks: 24
//      registers of two 16-bit slots, indexed by the trip number, which is a constant once the selects are unrolled);
//   3. the occupied slots are numbered densely (prefix sum in slot order); rd.blk_id[p] <- dense id of the block's slot, straight
//      from the registers (stores only); blocks that found no slot within PT_MAX_PROBE probes get a private entry at the top of
//      the table in HBM;
//   4. thread t pulls the triples of the ids t, t + 512, ... (at most 16) into registers -- the last reads of the hash table --
//      and, after one barrier, gathers their map points and computes {n', c} with block_plane() -- the arithmetic reg_build_kernel
//      used per block -- straight into the LDS entry of every id below PT_TCAP (4864), where the hash table was, and into the
//      scan's table in HBM (rd.pl_tab), which the slow evaluation form, the inlier phase and plane_table_reload read: nothing
//      is stored to HBM only to be loaded back;
//   5. a cost evaluation streams 18 bytes per block (the fp32 feature point straight from the extractor's cloud + the 16-bit
//      id) instead of 48 and reads the plane from LDS (ids beyond the LDS part: one 32-byte gather from the table in L2);
//      whatever LDS the table leaves free caches the first records {f, id} of the scan across the evaluations of a solve.
// Every block still evaluates the numbers the other paths evaluate ({n', c} from block_plane, bit for bit), in the same order;
// results agree with the general path's to rounding (pose 1e-12) and iteration for iteration with the oracle's (tests/test_gpu_reg.py).
#define PT_SLOTS 8192
#define PT_MAX_PROBE 192
#define PT_LDS_BYTES 155648           // s_raw of reg_solve_kernel: 152 KB
#define PT_TCAP (PT_LDS_BYTES / 32)   // table entries that fit LDS
#define LL_LINE_CACHE_MAX 1024        // line blocks of a scan kept in LDS (one workgroup per scan; a group member keeps its first round)
#define PT_EMPTY_A 0xffffffffffffffffull
#define PT_EMPTY_B 0xffffffffu
#define PT_PRIVATE 0xffffu   // a block's slot between the two passes: no slot found, the block gets a private table entry
#define PT_INACTIVE 0xfffeu  // ... not an active plane block
#define PT_NTRIP (FAST_MAX_BLOCKS / RS_THREADS / 8)  // trips of eight rounds a compact scan has at most (6)

struct PtSlot {
    unsigned long long a;  // (p0 << 32) | p1
    unsigned int b;        // p2
    unsigned int id;       // dense plane id (after the compaction)
};

__device__ __forceinline__ unsigned short gload_u16(const unsigned short *p) { return *(const LL_AS_GLOBAL unsigned short *)p; }

__device__ __forceinline__ unsigned int pt_hash(unsigned int p0, unsigned int p1, unsigned int p2)
{
    unsigned int h = p0 * 0x9E3779B1u;
    h ^= h >> 15;
    h += p1 * 0x85EBCA77u;
    h ^= h >> 13;
    h += p2 * 0xC2B2AE3Du;
    h ^= h >> 16;
    return h;
}

// slot of the triple (inserting it if new), or PT_PRIVATE.  Lock-free and wait-free per probe: a slot belongs to the first
// {p0, p1} that lands on its `a` word AND the first p2 that lands on its `b` word; a lane that loses either race (or finds
// another key) probes on, and every lane with the same triple walks the same probe sequence to the same slot.
template <int MAX_PROBE = PT_MAX_PROBE>
__device__ __forceinline__ unsigned int pt_insert(LL_AS_LDS PtSlot *ht, unsigned int p0, unsigned int p1, unsigned int p2)
{
    const unsigned long long A = ((unsigned long long)p0 << 32) | (unsigned long long)p1;
    const unsigned int hh = pt_hash(p0, p1, p2);
    unsigned int h = hh & (PT_SLOTS - 1);
    // double hashing (odd step, power-of-two table: a full cycle).  A wavefront waits for its slowest lane, and with linear
    // probing some lane of nearly every wavefront sat in one of the long clusters (2 - 3 k cycles per round of 64 inserts
    // at 43 % load)
    const unsigned int step = ((hh >> 13) | 1u) & (PT_SLOTS - 1);
    for (int probe = 0; probe < MAX_PROBE; probe++) {
        // two independent relaxed reads decide the common case (four of five blocks find their triple already there); each
        // word of a slot is written once, by an atomic, so a stale or half-claimed view only sends the lane through the
        // compare-and-swaps.  (Not `volatile`: the memory legalizer brackets a volatile access with waits for every outstanding
        // store, one HBM round trip per insert.)
        unsigned long long a = __hip_atomic_load(&ht[h].a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        unsigned int bb = __hip_atomic_load(&ht[h].b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (a == A && bb == p2) return h;
        if (a == PT_EMPTY_A) {  // (on failure the builtin leaves the value it found in `a`)
            if (__hip_atomic_compare_exchange_strong(&ht[h].a, &a, A, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) a = A;
        }
        if (a == A) {
            if (bb == PT_EMPTY_B) {
                if (__hip_atomic_compare_exchange_strong(&ht[h].b, &bb, p2, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) bb = p2;
            }
            if (bb == p2) return h;
        }
        h = (h + step) & (PT_SLOTS - 1);
    }
    return PT_PRIVATE;
}

// {n', c} of one neighbour triple -> two int4 (the arithmetic of reg_build_kernel's plane blocks: block_plane)
// SCALED: {m, beta} of ll_reg_core.h plane_scale (solve_fast3) instead of {n', c} (solve_big)
template <bool SCALED = false>
__device__ __forceinline__ void pt_plane(const f4 *map_pts, const double *pose_last, unsigned int i0, unsigned int i1, unsigned int i2, int4 &ob, int4 &oc)
{
    const f4 m0 = gload_pt(map_pts + i0), m1 = gload_pt(map_pts + i1), m2 = gload_pt(map_pts + i2);
    const double pa[3] = {(double)m0.x, (double)m0.y, (double)m0.z};
    const double pb[3] = {(double)m1.x, (double)m1.y, (double)m1.z};
    const double pc[3] = {(double)m2.x, (double)m2.y, (double)m2.z};
    double a_out[3] = {0.0, 0.0, 0.0}, v_out[3] = {0.0, 0.0, 0.0};
    (void)block_plane(pose_last, pa, pb, pc, a_out, v_out);  // degenerate triples never reach the table (build_one clears their flag)
    if (SCALED) {
        double m_[3], beta_;
        plane_scale(v_out, a_out[0], m_, &beta_);
        v_out[0] = m_[0], v_out[1] = m_[1], v_out[2] = m_[2], a_out[0] = beta_;
    }
    ob = make_int4(__double2loint(v_out[0]), __double2hiint(v_out[0]), __double2loint(v_out[1]), __double2hiint(v_out[1]));
    oc = make_int4(__double2loint(v_out[2]), __double2hiint(v_out[2]), __double2loint(a_out[0]), __double2hiint(a_out[0]));
}

__device__ __forceinline__ int4 *pt_table_global(const RegDev &rd, int b, int g, bool grouped)
{
    return rd.pl_tab + ((size_t)b * rd.tab_cap + (grouped ? (size_t)g * (rd.tab_cap / LL_GRP) : 0)) * 2;
}

// steps 1 - 4 above: the census of all blocks and the plane table of this workgroup's share of the plane blocks.  Returns the
// thread's activity mask.  Every loop that touches HBM keeps eight (four) independent loads in flight from clamped addresses.
#define PT_MAP_OFF (PT_SLOTS * 16)  // byte offset in s_raw of the id -> slot map (unsigned short[PT_SLOTS]) used during the build
template <bool GROUPED>
__device__ __noinline__ unsigned long long census_and_plane_table(const RegDev &rd, const RegConst &rc, const f4 *map_pts, int b, const RegState *st,
                                                                  int nC, int nS, uint4 *s_raw, SolveShared &sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int G = GROUPED ? LL_GRP : 1, GS = G * RS_THREADS;
    const int g = GROUPED ? sh.grp_g : 0;
    const int p0 = g * RS_THREADS + tid;
    const int kp = (nS + GS - 1) / GS;
    const int nSp = (nS + RS_THREADS - 1) / RS_THREADS * RS_THREADS;
    const int totp = nSp + nC;
    const size_t sb = (size_t)b * rd.cap;
    LL_AS_LDS PtSlot *ht = (LL_AS_LDS PtSlot *)s_raw;
    LL_AS_LDS unsigned short *slot_of_id = (LL_AS_LDS unsigned short *)((LL_AS_LDS char *)s_raw + PT_MAP_OFF);
    LL_T0(t_census);
    for (int e = tid; e < PT_SLOTS; e += RS_THREADS) lds_store_i4((int4 *)s_raw + e, make_int4(-1, -1, -1, -1));
    if (tid == 0) sh.pt_priv = 0;
    __syncthreads();
    const int4 *nn = rd.nn + sb + rd.cap_c;
    const unsigned char *flag0 = rd.blk_flag0 + sb;
    unsigned short *ids = rd.blk_id + (size_t)b * rd.cap_s;
    // ---- census (PCR:325,425) of all blocks + pass 1 of the own plane blocks: triples -> hash slots -----------------------
    unsigned long long act = 0;
    int na = 0, nca = 0, nsa = 0;
    // hash slot (or PT_PRIVATE / PT_INACTIVE) of every own plane block, two per register: a trip's eight (grouped: one) in
    // hreg[4 * trip ...] (grouped: half `trip & 1` of hreg[trip / 2])
    constexpr int NHREG = GROUPED ? PT_NTRIP / 2 : PT_NTRIP * 4;
    unsigned int hreg[NHREG];
#pragma unroll
    for (int i = 0; i < NHREG; i++) hreg[i] = PT_INACTIVE | (PT_INACTIVE << 16);
    for (int k0 = 0; k0 * RS_THREADS < totp; k0 += 8) {
        LL_T0(t_trip);
        unsigned char fl8[8];
        int4 t8[GROUPED ? 1 : 8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int j = tid + (k0 + u) * RS_THREADS;
            const int jc = j < totp ? j : 0;
            const size_t src = jc < nS ? (size_t)rd.cap_c + jc : (jc >= nSp ? (size_t)(jc - nSp) : (size_t)rd.cap_c);
            fl8[u] = gload_u8(flag0 + src);
            if (!GROUPED) t8[u] = gload_i4(nn + (j < nS ? j : 0));
        }
        if (GROUPED) {  // of eight consecutive rounds exactly one (round = g mod 8) is this member's
            const int j = tid + (k0 + g) * RS_THREADS;
            t8[0] = gload_i4(nn + (j < nS ? j : 0));
        }
        unsigned int h8[GROUPED ? 1 : 8];
#ifdef LL_SOLVE_TIMING
        if (fl8[0] == 255 && t8[0].x == -12345) act |= 1ull << 63;  // (forces the loads to have landed before the timer below)
        LL_TACC(10, t_trip);
        LL_T0(t_ins);
#endif
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int j = tid + (k0 + u) * RS_THREADS;
            const unsigned char fl = (j < totp && (j < nS || j >= nSp)) ? fl8[u] : (unsigned char)0;
            const bool active = (fl & BLK_ACTIVE) != 0;
            if (active) {
                act |= 1ull << (k0 + u);
                na++;
            }
            if (fl & 8) {
                if (j >= nSp) nca++; else nsa++;
            }
            if (!GROUPED || u == g) {
                const int4 t = t8[GROUPED ? 0 : u];
                const unsigned int h = (active && j < nS) ? pt_insert(ht, (unsigned int)t.x, (unsigned int)t.y, (unsigned int)t.z) : PT_INACTIVE;
                if (h == PT_PRIVATE) atomicAdd(&sh.pt_priv, 1);
                h8[GROUPED ? 0 : u] = h;
            }
        }
        // the slot indices stay in registers until pass 2 (no store between the inserts: the wait for the next flag byte would
        // become a wait for that store, one HBM round trip per block).  `k0 >> 3 == t` is uniform and t a constant after
        // unrolling, so hreg[] is never indexed at run time and stays out of scratch.
#pragma unroll
        for (int t = 0; t < PT_NTRIP; t++)
            if ((k0 >> 3) == t) {
                if constexpr (GROUPED) {
                    hreg[t / 2] = (t & 1) ? ((hreg[t / 2] & 0xffffu) | (h8[0] << 16)) : ((hreg[t / 2] & 0xffff0000u) | h8[0]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) hreg[4 * t + i] = h8[2 * i] | (h8[2 * i + 1] << 16);
                }
            }
#ifdef LL_SOLVE_TIMING
        LL_TACC(11, t_ins);
#endif
    }
    LL_T0(t_sums);
    {
        const unsigned long long tot = block_sum_u64((unsigned long long)na | ((unsigned long long)nca << 20) | ((unsigned long long)nsa << 40), sh);
        na = (int)(tot & 0xfffffull);
        nca = (int)((tot >> 20) & 0xfffffull);
        nsa = (int)((tot >> 40) & 0xfffffull);
    }
    if (rc.subsample_seed && na > rc.max_blocks) {  // a13 (PCR:438-458); the random stream is indexed by the block's
        int kept = 0;                               // position in the reference's order: corners, then surfaces
        for (int k = 0; k * RS_THREADS < totp; k++) {  // (a dropped block's triple stays in the table, unused)
            if (!((act >> k) & 1ull)) continue;
            const int j = tid + k * RS_THREADS;
            const int jref = j >= nSp ? j - nSp : nC + j;
            if (subsample_drop_block(rc.subsample_seed, st->icp_iters, jref, na, rc.max_blocks))
                act &= ~(1ull << k);
            else
                kept++;
        }
        na = block_sum_int(kept, sh);
    }
    if (tid == 0) {
        sh.n_active = na;
        sh.n_corner_avail = nca;
        sh.n_surf_avail = nsa;
    }
    __syncthreads();  // (also: every insert has landed)
    LL_TACC(12, t_sums);
    LL_TACC(6, t_census);
    LL_T0(t_tab);
    LL_T0(t_cmp);
    // ---- dense ids in slot order; id -> slot map --------------------------------------------------------------------------
    constexpr int SPT = PT_SLOTS / RS_THREADS;  // slots per thread: tid, tid + 512, ... (consecutive slots per thread would put
    unsigned int occ = 0;                       // all 64 lanes of a read on one LDS bank)
#pragma unroll
    for (int i = 0; i < SPT; i++)
        if (ht[tid + i * RS_THREADS].b != PT_EMPTY_B) occ |= 1u << i;
    const int cnt = __popc(occ);
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(incl, off);
        if (lane >= off) incl += y;
    }
    if (lane == 63) sh.isum[wave] = incl;
    __syncthreads();
    int base = incl - cnt, T = 0;
    for (int w = 0; w < RS_WAVES; w++) {
        if (w < wave) base += sh.isum[w];
        T += sh.isum[w];
    }
    {
        int rk = base;
#pragma unroll
        for (int i = 0; i < SPT; i++)
            if (occ & (1u << i)) {
                ht[tid + i * RS_THREADS].id = (unsigned int)rk;
                slot_of_id[rk] = (unsigned short)(tid + i * RS_THREADS);
                rk++;
            }
    }
    __syncthreads();
    LL_TACC(13, t_cmp);
    LL_T0(t_p2);
    int4 *tabG = pt_table_global(rd, b, g, GROUPED);
    double pose_last[7];
#pragma unroll
    for (int i = 0; i < 7; i++) pose_last[i] = gload_f64(st->pose_last + i);
    // ---- pass 2: slot (registers) -> dense id (LDS) -> rd.blk_id: stores only -----------------------------------------------
    const int region = GROUPED ? rd.tab_cap / LL_GRP : rd.tab_cap;
    if constexpr (GROUPED) {  // one block per trip: p0 + trip * GS (kp <= PT_NTRIP)
        unsigned int id8[PT_NTRIP];
#pragma unroll
        for (int u = 0; u < PT_NTRIP; u++) {
            const unsigned int h = (hreg[u / 2] >> ((u & 1) * 16)) & 0xffffu;
            const unsigned int sid = ht[h < PT_SLOTS ? h : 0u].id;
            id8[u] = h < PT_SLOTS ? sid : (h == PT_PRIVATE ? PT_PRIVATE : 0u);
        }
#pragma unroll
        for (int u = 0; u < PT_NTRIP; u++) {
            const int p = p0 + u * GS;
            if (p < nS) gstore_u16(ids + p, (unsigned short)id8[u]);
        }
    } else {
        for (int k0 = 0; k0 < kp; k0 += 8) {
            unsigned int w4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int t = 0; t < PT_NTRIP; t++)
                if ((k0 >> 3) == t) {
#pragma unroll
                    for (int i = 0; i < 4; i++) w4[i] = hreg[4 * t + i];
                }
            unsigned int id8[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const unsigned int h = (w4[u >> 1] >> ((u & 1) * 16)) & 0xffffu;
                const unsigned int sid = ht[h < PT_SLOTS ? h : 0u].id;
                id8[u] = h < PT_SLOTS ? sid : (h == PT_PRIVATE ? PT_PRIVATE : 0u);
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int p = p0 + (k0 + u) * GS;
                if (p < nS) gstore_u16(ids + p, (unsigned short)id8[u]);
            }
        }
    }
    if (sh.pt_priv > 0) {  // (uniform; rare: the hash table was too crowded around some triples -- those blocks get entries of
        int npriv = 0;     //  their own at the top of the table region, numbered per thread and then across the workgroup;
        for (int k = 0; k < kp; k++) {  // they live in HBM only)
            const int p = p0 + k * GS;
            if (p < nS && gload_u16(ids + p) == PT_PRIVATE) npriv++;
        }
        int incl2 = npriv;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl2, off);
            if (lane >= off) incl2 += y;
        }
        __syncthreads();
        if (lane == 63) sh.isum[wave] = incl2;
        __syncthreads();
        int pid = incl2 - npriv;
        for (int w = 0; w < wave; w++) pid += sh.isum[w];
        for (int k = 0; k < kp; k++) {
            const int p = p0 + k * GS;
            if (p >= nS || gload_u16(ids + p) != PT_PRIVATE) continue;
            const unsigned int id = (unsigned int)(region - 1 - pid);
            pid++;
            const int4 t = gload_i4(nn + p);
            int4 ob, oc;
            pt_plane<true>(map_pts, pose_last, (unsigned int)t.x, (unsigned int)t.y, (unsigned int)t.z, ob, oc);
            gstore_i4(tabG + 2 * id, ob);
            gstore_i4(tabG + 2 * id + 1, oc);
            gstore_u16(ids + p, (unsigned short)id);
        }
    }
    LL_TACC(15, t_p2);
    LL_T0(t_pl);
    // ---- the triples of the thread's ids t, t + 512, ... -> registers (the last readers of the hash table and the id -> slot
    //      map: after the barrier the planes overwrite them) ---------------------------------------------------------------------
    constexpr int IPT = PT_SLOTS / RS_THREADS;  // ids per thread at most
    const int Tu = __builtin_amdgcn_readfirstlane(T);
    unsigned long long ta[IPT];
    unsigned int tb[IPT];
#pragma unroll
    for (int i = 0; i < IPT; i++) ta[i] = 0ull, tb[i] = 0u;
#pragma unroll
    for (int q = 0; q < IPT / 4; q++)
        if (q * 4 * RS_THREADS < Tu) {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int id = tid + (4 * q + u) * RS_THREADS;
                const unsigned int sl = slot_of_id[id < T ? id : 0] & (PT_SLOTS - 1);
                ta[4 * q + u] = ht[sl].a;
                tb[4 * q + u] = ht[sl].b;
            }
        }
    const int Tl = T < PT_TCAP ? T : PT_TCAP;
    if (tid == 0) {
        // (T beyond the LDS part, or private entries: the evaluation takes its slower form, solver_eval3)
        // Line blocks (64 B each: sensor point + a', v' in fp64) are few in a Q-full scan and half of a voxel-filtered one; they are
        // not pipelined -- every evaluation that reads them from HBM waits a full memory latency at its end.  The first
        // LL_LINE_CACHE_MAX of them (this group member's first round) stay in LDS above the record cache, written by the
        // FILL evaluation like the plane records.
        int nl = 0;
        if (!rc.no_line_cache && T <= PT_TCAP && sh.pt_priv == 0) {
            int mine = GROUPED ? nC - g * RS_THREADS : nC;
            const int cap = GROUPED ? RS_THREADS : LL_LINE_CACHE_MAX;
            mine = mine < 0 ? 0 : (mine > cap ? cap : mine);
            const int room = (PT_LDS_BYTES / 16 - 2 * Tl) / 4;
            nl = mine < room ? mine : room;
        }
        const int kc = (PT_LDS_BYTES / 16 - 2 * Tl - 4 * nl) / RS_THREADS;
        sh.pt_T = sh.pt_priv > 0 ? PT_TCAP + 1 : T;
        sh.pt_Tl = Tl;
        sh.pt_kc = kc < kp ? kc : kp;
        sh.pt_nl = nl;
    }
    __syncthreads();  // the hash table is dead
    // ---- plane constants: ids below PT_TCAP straight into their LDS entries, every id into the table in HBM (which the slow
    //      evaluation form, the inlier phase and plane_table_reload read; nobody waits for these stores).  Four triples' gathers
    //      in flight -------------------------------------------------------------------------------------------------------------
    int4 *s_tab = (int4 *)s_raw;
#pragma unroll 1  // (one copy of the plane arithmetic: the selects below cost a few moves per trip)
    for (int q = 0; q * 4 * RS_THREADS < Tu; q++) {
        unsigned long long a4[4] = {0ull, 0ull, 0ull, 0ull};
        unsigned int b4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < IPT / 4; t++)
            if (q == t) {
#pragma unroll
                for (int u = 0; u < 4; u++) a4[u] = ta[4 * t + u], b4[u] = tb[4 * t + u];
            }
        const int i0 = tid + q * 4 * RS_THREADS;
        if (i0 < T) {
            f4 m[4][3];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int id = i0 + u * RS_THREADS;
                const unsigned long long sa = id < T ? a4[u] : a4[0];
                const unsigned int sb2 = id < T ? b4[u] : b4[0];
                m[u][0] = gload_pt(map_pts + (unsigned int)(sa >> 32));
                m[u][1] = gload_pt(map_pts + (unsigned int)sa);
                m[u][2] = gload_pt(map_pts + sb2);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int id = i0 + u * RS_THREADS;
                const double pa[3] = {(double)m[u][0].x, (double)m[u][0].y, (double)m[u][0].z};
                const double pb[3] = {(double)m[u][1].x, (double)m[u][1].y, (double)m[u][1].z};
                const double pc[3] = {(double)m[u][2].x, (double)m[u][2].y, (double)m[u][2].z};
                double a_out[3] = {0.0, 0.0, 0.0}, v_out[3] = {0.0, 0.0, 0.0};
                (void)block_plane(pose_last, pa, pb, pc, a_out, v_out);  // degenerate triples never reach the table (build_one clears their flag)
                {  // the table holds the SCALED plane {m = |n'| n', beta = |n'| c} (ll_reg_core.h plane_scale)
                    double m_[3], beta_;
                    plane_scale(v_out, a_out[0], m_, &beta_);
                    v_out[0] = m_[0], v_out[1] = m_[1], v_out[2] = m_[2], a_out[0] = beta_;
                }
                const int4 ob = make_int4(__double2loint(v_out[0]), __double2hiint(v_out[0]), __double2loint(v_out[1]), __double2hiint(v_out[1]));
                const int4 oc = make_int4(__double2loint(v_out[2]), __double2hiint(v_out[2]), __double2loint(a_out[0]), __double2hiint(a_out[0]));
                if (id < Tl) {
                    lds_store_i4(s_tab + 2 * id, ob);
                    lds_store_i4(s_tab + 2 * id + 1, oc);
                }
                if (id < T) {
                    gstore_i4(tabG + 2 * id, ob);
                    gstore_i4(tabG + 2 * id + 1, oc);
                }
            }
        }
    }
    __syncthreads();  // the LDS part of the table is complete
    LL_TACC(14, t_pl);
    LL_TACC(8, t_tab);
    return act;
}

// after the inlier phase has used s_raw for its tables
__device__ __forceinline__ void plane_table_reload(const RegDev &rd, int b, bool grouped, uint4 *s_raw, SolveShared &sh)
{
    const int4 *tabG = pt_table_global(rd, b, grouped ? sh.grp_g : 0, grouped);
    int4 *s_tab = (int4 *)s_raw;
    const int n = 2 * sh.pt_Tl;
    for (int e0 = threadIdx.x; e0 < n; e0 += 8 * RS_THREADS) {
        int4 v8[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int e = e0 + u * RS_THREADS;
            v8[u] = gload_i4(tabG + (e < n ? e : e0));
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int e = e0 + u * RS_THREADS;
            if (e < n) lds_store_i4(s_tab + e, v8[u]);
        }
    }
    __syncthreads();
}

struct Rec3 {
    int fx, fy, fz;  // bits of the fp32 feature point (sensor frame)
    unsigned int id;
};
struct Pl3 {
    int4 b, c;  // {n'.x, n'.y}, {n'.z, c}
};

// The plane loop of a cost evaluation, rounds [KB, KE) of this thread's blocks.  Everything the waitcnt pass has to see
// through is straight-line: loads are unconditional (clamped addresses), only arithmetic and LDS stores sit behind
// predicates -- a load behind a branch (a conditional global fallback for the plane, a cached / streamed switch inside the
// loop) made the compiler drain the whole pipeline with vmcnt(0) at every stage (first build of this path: 66 k cycles per
// evaluation against 25 k of fp64 issue).  Records are prefetched four rounds ahead (5 register sets rotating by name), the
// plane of the next record is fetched from the LDS table while the current one is evaluated.
//   FROM_CACHE: records from the LDS record cache (rounds < kc of an evaluation that does not FILL); else 18 B per lane and
//   record from HBM.  TAB_LDS: the scan's whole table is in LDS (T <= PT_TCAP) -- the fast form; otherwise a plane with
//   id >= Tl is gathered from the table in HBM behind a branch (correct, same summation order, not pipelined).
#define LL3_LOAD(R, K)                                                                             \
    {                                                                                              \
        if (FROM_CACHE_) {                                                                         \
            const int kc_ = (K) < kc ? (K) : kc - 1;                                               \
            const int4 c_ = lds_load_i4(cache + tid + kc_ * RS_THREADS);                           \
            R.fx = c_.x;                                                                           \
            R.fy = c_.y;                                                                           \
            R.fz = c_.z;                                                                           \
            R.id = (unsigned int)c_.w;                                                             \
        } else {                                                                                   \
            const int pp_ = p0 + (K) * GS;                                                         \
            const int pc_ = pp_ < nS ? pp_ : 0;                                                    \
            float fx_, fy_, fz_;                                                                   \
            gload_f3(feat + pc_, fx_, fy_, fz_);                                                   \
            R.id = gload_u16(ids + pc_);                                                           \
            R.fx = __float_as_int(fx_);                                                            \
            R.fy = __float_as_int(fy_);                                                            \
            R.fz = __float_as_int(fz_);                                                            \
        }                                                                                          \
    }
#define LL3_PLANE(Q, R)                                                                            \
    {                                                                                              \
        if (TAB_LDS || R.id < (unsigned int)Tl) {                                                  \
            Q.b = lds_load_i4(tabL + 2 * R.id);                                                    \
            Q.c = lds_load_i4(tabL + 2 * R.id + 1);                                                \
        } else {                                                                                   \
            Q.b = gload_i4(tabG + 2 * R.id);                                                       \
            Q.c = gload_i4(tabG + 2 * R.id + 1);                                                   \
        }                                                                                          \
    }
#define LL3_USE(R, Q, K)                                                                                   \
    if ((K) < KE_) {                                                                                       \
        const int pp_ = p0 + (K) * GS;                                                                     \
        if (FILL && (K) < kc) lds_store_i4(cache + tid + (K) * RS_THREADS, make_int4(R.fx, R.fy, R.fz, (int)R.id)); \
        if (pp_ < nS && ((act >> (g + G * (K))) & 1ull)) { /* (a group member's last round may reach into the lines' bits) */ \
            const double f[3] = {(double)__int_as_float(R.fx), (double)__int_as_float(R.fy), (double)__int_as_float(R.fz)}; \
            const double v[3] = {__hiloint2double(Q.b.y, Q.b.x), __hiloint2double(Q.b.w, Q.b.z), __hiloint2double(Q.c.y, Q.c.x)}; \
            const double beta_ = __hiloint2double(Q.c.w, Q.c.z);                                           \
            plane_accumulate_scaled(R_, t_, f, v, beta_, huber_a, acc);                                    \
            if (L1OUT) gstore_f64(l1_planes + pp_, plane_l1_scaled(R_, t_, f, v, beta_, huber_a, q_last)); \
        }                                                                                                  \
    }
#define LL3_PIPE(FROM_CACHE, KB, KE)                                   \
    {                                                                  \
        constexpr bool FROM_CACHE_ = FROM_CACHE;                       \
        const int KB_ = (KB), KE_ = (KE);                              \
        if (KB_ < KE_) {                                               \
            Rec3 r0, r1, r2, r3, r4;                                   \
            Pl3 q0, q1, q2, q3, q4;                                    \
            LL3_LOAD(r0, KB_)                                          \
            LL3_LOAD(r1, KB_ + 1)                                      \
            LL3_LOAD(r2, KB_ + 2)                                      \
            LL3_LOAD(r3, KB_ + 3)                                      \
            LL3_PLANE(q0, r0)                                          \
            for (int k = KB_; k < KE_; k += 5) {                       \
                LL3_LOAD(r4, k + 4)                                    \
                LL3_PLANE(q1, r1)                                      \
                LL3_USE(r0, q0, k)                                     \
                LL3_LOAD(r0, k + 5)                                    \
                LL3_PLANE(q2, r2)                                      \
                LL3_USE(r1, q1, k + 1)                                 \
                LL3_LOAD(r1, k + 6)                                    \
                LL3_PLANE(q3, r3)                                      \
                LL3_USE(r2, q2, k + 2)                                 \
                LL3_LOAD(r2, k + 7)                                    \
                LL3_PLANE(q4, r4)                                      \
                LL3_USE(r3, q3, k + 3)                                 \
                LL3_LOAD(r3, k + 8)                                    \
                LL3_PLANE(q0, r0)                                      \
                LL3_USE(r4, q4, k + 4)                                 \
            }                                                          \
        }                                                              \
    }

// workgroup evaluation of cost / g / H at x over the active blocks -> sh.sum (FILL: this evaluation writes the LDS record cache; L1OUT: it also leaves the L1 values; GROUPED: a group member's share)
template <bool FILL, bool L1OUT, bool GROUPED>
__device__ __noinline__ void solver_eval3(const RegDev &rd, int b, int nC, int nS, const double *x, double huber_a, unsigned long long act,
                                          uint4 *s_raw, const double *q_last_g, SolveShared &sh)
{
    constexpr int DEBLUR = 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double q_last[4] = {0.0, 0.0, 0.0, 1.0};
    if (L1OUT) {
        q_last[0] = q_last_g[0];
        q_last[1] = q_last_g[1];
        q_last[2] = q_last_g[2];
        q_last[3] = q_last_g[3];
    }
    double *l1_planes = rd.blk_l1 + (size_t)b * rd.cap + rd.cap_c;
    double *l1_lines = rd.blk_l1 + (size_t)b * rd.cap;
    LL_CTX_DECL(x)
    double acc[LL_NACC];
#pragma unroll
    for (int i = 0; i < LL_NACC; i++) acc[i] = 0.0;
    constexpr int G = GROUPED ? LL_GRP : 1, GS = G * RS_THREADS;
    const int g = GROUPED ? sh.grp_g : 0;
    const int p0 = g * RS_THREADS + tid;
    const int Tl = sh.pt_Tl, kc = sh.pt_kc;
    const int kp = (nS + GS - 1) / GS;
    const int4 *tabL = (const int4 *)s_raw;
    int4 *cache = (int4 *)s_raw + 2 * Tl;
    const int4 *tabG = pt_table_global(rd, b, g, GROUPED);
    const unsigned short *ids = rd.blk_id + (size_t)b * rd.cap_s;
    const float4 *feat = rd.surf_feat + (size_t)b * rd.feat_stride_s;
    if (sh.pt_T <= PT_TCAP) {  // uniform: the whole table is in LDS (every C2 scan)
        constexpr bool TAB_LDS = true;
        if (!FILL) LL3_PIPE(true, 0, kc)
        LL3_PIPE(false, FILL ? 0 : kc, kp)
    } else {
        constexpr bool TAB_LDS = false;
        if (!FILL) LL3_PIPE(true, 0, kc)
        LL3_PIPE(false, FILL ? 0 : kc, kp)
    }
    plane_unfold2(acc);  // the factors 2 of the planes' rotation rows and columns (plane_accumulate_scaled leaves them out), before the lines are added
    {
        // line blocks (a few hundred per Mid-40 scan): the 65-byte fp64 form
        const size_t sb = (size_t)b * rd.cap;
        const double *av = rd.blk_av + (size_t)b * 6 * rd.cap;
        const int kpl = (nS + RS_THREADS - 1) / RS_THREADS;  // the lines' first round in the activity mask
        const int nl = sh.pt_nl;
        int4 *lc = (int4 *)s_raw + (PT_LDS_BYTES / 16 - 4 * nl);  // four planes of nl entries: {f}, {a0, v0}, {v1, v2}, {a1, a2}
        int k = 0;
        for (int l = p0; l < nC; l += GS, k++) {
            if (!((act >> (kpl + g + G * k)) & 1ull)) continue;
            BlkRegs br;
            const int j = GROUPED ? (k == 0 ? tid : nl) : l;  // its place in the LDS copy (>= nl: none)
            if (!FILL && j < nl) {
                const int4 c0 = lds_load_i4(lc + j), c1 = lds_load_i4(lc + nl + j), c2 = lds_load_i4(lc + 2 * nl + j), c3 = lds_load_i4(lc + 3 * nl + j);
                br.f = make_float4(__int_as_float(c0.x), __int_as_float(c0.y), __int_as_float(c0.z), __int_as_float(c0.w));
                br.a0 = __hiloint2double(c1.y, c1.x);
                br.v0 = __hiloint2double(c1.w, c1.z);
                br.v1 = __hiloint2double(c2.y, c2.x);
                br.v2 = __hiloint2double(c2.w, c2.z);
                br.a1 = __hiloint2double(c3.y, c3.x);
                br.a2 = __hiloint2double(c3.w, c3.z);
            } else {
                load_blk(rd, sb, av, l, br);
                if (FILL && j < nl) {
                    lds_store_i4(lc + j, make_int4(__float_as_int(br.f.x), __float_as_int(br.f.y), __float_as_int(br.f.z), __float_as_int(br.f.w)));
                    lds_store_i4(lc + nl + j, make_int4(__double2loint(br.a0), __double2hiint(br.a0), __double2loint(br.v0), __double2hiint(br.v0)));
                    lds_store_i4(lc + 2 * nl + j, make_int4(__double2loint(br.v1), __double2hiint(br.v1), __double2loint(br.v2), __double2hiint(br.v2)));
                    lds_store_i4(lc + 3 * nl + j, make_int4(__double2loint(br.a1), __double2hiint(br.a1), __double2loint(br.a2), __double2hiint(br.a2)));
                }
            }
            const double a[3] = {br.a0, br.a1, br.a2};
            const double v[3] = {br.v0, br.v1, br.v2};
            LL_CTX_ACCUM(BLK_LINE, br.f, a, v, huber_a, acc);
            if (L1OUT) {
                double l1;
                LL_CTX_L1(l1, BLK_LINE, br.f, a, v, huber_a, q_last);
                l1_lines[l] = l1;
            }
        }
    }
    // A wavefront none of whose threads owns an active block (voxel-filtered scans of a few hundred blocks: half of the eight)
    // has nothing but +0.0 to add: it writes the zeros instead of running 28 six-step reductions beside the wavefront that
    // shares its SIMD (the 504 data-parallel moves and adds are half of such an evaluation's cycles).  Same sums, bit for bit.
    if (__ballot(act != 0ull) != 0ull) {
        wave_sum_acc(acc, sh.red[wave], lane);
    } else if (lane < LL_NACC) {
        sh.red[wave][lane] = 0.0;
    }
    __syncthreads();
    if (tid < LL_NACC) {
        double s = 0.0;
        for (int w = 0; w < RS_WAVES; w++) s += sh.red[w][tid];
        sh.sum[tid] = s;
    }
    __syncthreads();
    if (GROUPED) {
        LL_T0(t_grp);
        group_reduce<L1OUT>(rd, b, sh);
        LL_TACC(9, t_grp);
    }
}
#undef LL3_LOAD
#undef LL3_PLANE
#undef LL3_USE
#undef LL3_PIPE

// one ceres::Solve on the plane-table layout: starts at x0, leaves the result in sh.ctl
template <bool WANT_L1, bool GROUPED>
__device__ __forceinline__ void solver_lm3(const RegDev &rd, const RegConst &rc, int b, int nC, int nS, const double *x0, int max_iter,
                                           int n_active, unsigned long long act, uint4 *s_raw, const double *q_last, SolveShared &sh)
{
    const int tid = threadIdx.x;
    if (tid == 0) {
        lm_begin(sh.ctl, x0, max_iter, rc.bound);
        sh.l1_valid = 0;
    }
    __syncthreads();
    {
        LL_T0(t0);
        solver_eval3<true, false, GROUPED>(rd, b, nC, nS, sh.ctl.x, rc.huber_a, act, s_raw, q_last, sh);
        LL_TACC(0, t0);
    }
    {
        LL_T0(t1);
        if (tid < 64) {  // the controller's wavefront
            const int need = lm_init_wave(sh.ctl, sh.sum, n_active, tid);
            if (tid == 0) sh.need = need;
        }
        __syncthreads();
        LL_TACC(1, t1);
    }
    while (sh.need) {
        const bool spec = WANT_L1 && sh.ctl.iteration >= max_iter;  // if this candidate is accepted it is the solve's result
        LL_T0(t0);
        if (spec)
            solver_eval3<false, true, GROUPED>(rd, b, nC, nS, sh.ctl.cand, rc.huber_a, act, s_raw, q_last, sh);
        else
            solver_eval3<false, false, GROUPED>(rd, b, nC, nS, sh.ctl.cand, rc.huber_a, act, s_raw, q_last, sh);
        LL_TACC(0, t0);
        LL_T0(t1);
        if (tid < 64) {  // the controller's wavefront steps the controller (ll_lm_wave.h); lane 0 has the answer
            const int need = lm_update_wave(sh.ctl, sh.sum, sh.fit, tid, sh.tcyc + 14);
            if (tid == 0) {
                sh.need = need;
                sh.l1_valid = (spec && !need && sh.ctl.last_accept == 1) ? 1 : 0;
            }
        }
        __syncthreads();
        LL_TACC(1, t1);
    }
}

// L1 values at the prerun result -> inlier threshold -> prune (PCR:476-499), the activity mask in place of LDS flags.
// Returns the pruned mask.
template <int NK, bool GROUPED>
__device__ __noinline__ unsigned long long inlier_phase3(const RegDev &rd, const RegConst &rc, int b, RegState *st, SolveShared &sh, uint4 *s_raw,
                                                         unsigned long long act, int nC, int nS)
{
    constexpr int DEBLUR = 0;
    const int tid = threadIdx.x;
    const int nSp = (nS + RS_THREADS - 1) / RS_THREADS * RS_THREADS;
    const int totp = nSp + nC;
    const size_t sb = (size_t)b * rd.cap;
    LL_T0(t_l1);
    double *l1g = rd.blk_l1 + sb;
    if (!sh.l1_valid) {
        // rare: the prerun ended on a rejected step (or converged early).  Every workgroup evaluates its own share, from the
        // table in HBM (a plain rolled loop)
        LL_CTX_DECL(sh.ctl.x)
        constexpr int G = GROUPED ? LL_GRP : 1, GS = G * RS_THREADS;
        const int g = GROUPED ? sh.grp_g : 0;
        const int p0 = g * RS_THREADS + tid;
        const int4 *tabG = pt_table_global(rd, b, g, GROUPED);
        const unsigned short *ids = rd.blk_id + (size_t)b * rd.cap_s;
        const float4 *feat = rd.surf_feat + (size_t)b * rd.feat_stride_s;
        const double *av = rd.blk_av + (size_t)b * 6 * rd.cap;
        int k = 0;
        for (int p = p0; p < nS; p += GS, k++) {
            if (!((act >> (g + G * k)) & 1ull)) continue;
            const float4 ff = gload_f4(feat + p);
            const unsigned int id = gload_u16(ids + p);
            const int4 qb = gload_i4(tabG + 2 * id), qc = gload_i4(tabG + 2 * id + 1);
            const double f[3] = {(double)ff.x, (double)ff.y, (double)ff.z};
            const double v[3] = {__hiloint2double(qb.y, qb.x), __hiloint2double(qb.w, qb.z), __hiloint2double(qc.y, qc.x)};
            l1g[rd.cap_c + p] = plane_l1_scaled(R_, t_, f, v, __hiloint2double(qc.w, qc.z), rc.huber_a, st->pose_last);  // (the table holds scaled planes)
        }
        const int kpl = nSp / RS_THREADS;
        k = 0;
        for (int l = p0; l < nC; l += GS, k++) {
            if (!((act >> (kpl + g + G * k)) & 1ull)) continue;
            BlkRegs br;
            load_blk(rd, sb, av, l, br);
            const double a[3] = {br.a0, br.a1, br.a2};
            const double v[3] = {br.v0, br.v1, br.v2};
            double l1;
            LL_CTX_L1(l1, BLK_LINE, br.f, a, v, rc.huber_a, st->pose_last);
            l1g[l] = l1;
        }
        if (GROUPED)
            group_barrier<true>(rd, b, sh);  // the other members' shares
        else
            __syncthreads();
    } else if (tid == 0) {
        sh.tcyc[9] += 1;  // LL_SOLVE_TIMING: how often the shortcut was taken
    }
    double l1r[NK];  // the thread's register tile: block j = tid + k * RS_THREADS
    {
        const int kt = (totp + RS_THREADS - 1) / RS_THREADS;
#pragma unroll
        for (int k = 0; k < NK; k++) {  // unconditional loads from clamped addresses: all in flight together
            const int j = tid + k * RS_THREADS;
            double v = -1.0;
            if (k < kt) {
                const int jc = j < totp ? j : 0;
                const size_t src = jc < nS ? (size_t)rd.cap_c + jc : (jc >= nSp ? (size_t)(jc - nSp) : (size_t)rd.cap_c);
                v = gload_f64(l1g + src);
            }
            l1r[k] = v;
        }
#pragma unroll
        for (int k = 0; k < NK; k++) l1r[k] = ((act >> k) & 1ull) ? l1r[k] : -1.0;
    }
    __syncthreads();
    LL_TACC(2, t_l1);

    inlier_threshold_regs<NK>(l1r, totp, (unsigned long long *)s_raw, sh, rc);  // overwrites the LDS plane table and record cache

    // ---- prune (PCR:487-499) ---------------------------------------------------------------------------------
    LL_T0(t_prune);
    {
        const double thr = sh.thr;
        int na = 0;
#pragma unroll
        for (int k = 0; k < NK; k++) {
            if (!((act >> k) & 1ull)) continue;
            if (l1r[k] > thr)
                act &= ~(1ull << k);
            else
                na++;
        }
        na = block_sum_int(na, sh);
        if (tid == 0) sh.n_active = na;
        __syncthreads();
    }
    LL_TACC(7, t_prune);
    return act;
}

// (inlined into its kernel by force: left to the inliner's size estimate, the one-workgroup form became a call when the controller grew)
template <bool GROUPED>
__device__ __forceinline__ void solve_fast3(const RegDev &rd, const RegConst &rc, const f4 *map_pts, int b, RegState *st, SolveShared &sh, uint4 *s_raw)
{
    constexpr int DEBLUR = 0;
    const int tid = threadIdx.x;
    const int nC = rd.n_corner[b], nS = rd.n_surf[b];
    const int nSp = (nS + RS_THREADS - 1) / RS_THREADS * RS_THREADS;  // lines start at a whole round
    const int totp = nSp + nC;                                        // <= FAST_MAX_BLOCKS (scan_is_compact)
    const size_t sb = (size_t)b * rd.cap;
    if (tid < 16) sh.tcyc[tid] = 0;
    __syncthreads();
    LL_T0(t_total);

    // ---- flags -> the thread's activity mask (bit k: block tid + k * RS_THREADS in the order planes, padding, lines), census
    //      (PCR:325,425), and the scan's plane table (this workgroup's share of it) ------------------------------------------
    unsigned long long act = census_and_plane_table<GROUPED>(rd, rc, map_pts, b, st, nC, nS, s_raw, sh);

    // ---- prerun solve (PCR:463-474); its last evaluation also leaves the per-block L1 values in blk_l1 ------------
    solver_lm3<true, GROUPED>(rd, rc, b, nC, nS, st->inc, rc.ceres_prerun_times, sh.n_active, act, s_raw, st->pose_last, sh);
    int lm_iters = sh.ctl.iteration;

    if (totp <= 36 * RS_THREADS)  // the Mid-40 configurations: a 36-entry register tile per thread
        act = inlier_phase3<36, GROUPED>(rd, rc, b, st, sh, s_raw, act, nC, nS);
    else
        act = inlier_phase3<FAST_MAXK, GROUPED>(rd, rc, b, st, sh, s_raw, act, nC, nS);

    // ---- final solve (PCR:501-508) -----------------------------------------------------------------------------
    {
        __shared__ double x_start_3[7];
        if (tid < 7) x_start_3[tid] = sh.ctl.x[tid];
        plane_table_reload(rd, b, GROUPED, s_raw, sh);  // (its barrier also publishes x_start_3)
        solver_lm3<false, GROUPED>(rd, rc, b, nC, nS, x_start_3, rc.ceres_max_iterations, sh.n_active, act, s_raw, st->pose_last, sh);
    }
    lm_iters += sh.ctl.iteration;
    if (GROUPED) {
        group_barrier<false>(rd, b, sh);  // nobody reads st->inc / st->pose_last any more
        if (sh.grp_g != 0) return;
        if (sh.grp_abort) {  // a barrier timed out: nothing this group computed can be trusted (reg_finalize_kernel rejects the scan)
            if (tid == 0) {
                st->aborted = 1;
                st->done = 1;
                st->icp_iters += 1;
            }
            return;
        }
    }
    solve_epilogue(rc, st, sh, lm_iters);
#if defined(LL_SOLVE_TIMING) || defined(LL_LM_COUNTS)
    LL_TACC(5, t_total);
    if (tid == 0)
        for (int i = 0; i < 16; i++) st->dbg_cycles[i] += sh.tcyc[i];
#endif
}

// ---- the prologue of the kernels built on solve_fast3 (reg_solve_kernel, reg_solve_maps_kernel) -------------------------------------
// Which scan this workgroup works on, and as which member: blockIdx.x, or in a grouped launch (n_scans * G workgroups) scan and rank
// by ticket, see group_barrier.  (Returned by value: with three reference parameters reg_solve_maps_kernel's registers moved.)
struct SolveTicket {
    int b, g, G;  // scan, rank in its group, group size
};
__device__ __forceinline__ SolveTicket solve_fast_ticket(const RegDev &rd, const RegConst &rc, SolveShared &sh)
{
    SolveTicket t = {(int)blockIdx.x, 0, 1};
    if (rc.solve_group > 1) {
        if (threadIdx.x == 0) sh.grp_seq = atomicAdd(rd.grp_ctl, 1);
        __syncthreads();
        t.G = rc.solve_group;
        t.b = sh.grp_seq / t.G;
        t.g = sh.grp_seq - t.b * t.G;
        __syncthreads();
    }
    return t;
}
// false: the scan is beyond solve_fast3.  Cannot happen (the host launches these kernels only for batches they hold): fail loudly --
// rejected and reported -- instead of answering.
__device__ __forceinline__ bool solve_fast_check(const RegDev &rd, const RegConst &rc, int b, int g, int nC, int nS, RegState *st)
{
    if (padded_block_count(nC, nS) > FAST_MAX_BLOCKS || !scan_is_compact(rd, rc, b)) {
        if (g == 0 && threadIdx.x == 0) {
            st->aborted = 1;
            st->done = 1;
            st->icp_iters += 1;
        }
        return false;
    }
    return true;
}
__device__ __forceinline__ void solve_fast_group_fields(const RegConst &rc, int g, int G, SolveShared &sh)
{
    if (threadIdx.x == 0) {
        sh.grp_g = g;
        sh.grp_G = G;
        sh.grp_seq = 0;
        sh.xch_seq = 0;
        sh.xch_epoch = rc.xch_epoch;
        sh.grp_abort = (rc.test_group_abort && G > 1) ? 1 : 0;  // test switch: behave as if the first barrier had timed out
    }
    __syncthreads();
}

}  // namespace ll
