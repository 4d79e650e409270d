// ll_reg_small_solve.h -- the text of reg_solve_small_kernel (ll_reg_small_kernels.hip), included once per form of the kernel:
//   LL_SMALL_KERNEL      the kernel's name
//   LL_SMALL_MORE_ARGS   parameters behind (SmallArgs rd, RegConst rc)
//   LL_SMALL_BIND_MAP    statement(s) run once the workgroup knows its scan b: empty for the single-map form, the look-up of the
//                        scan's surface map in the map table for the map-per-slot form
// Text inclusion rather than a shared device function: the single-map kernels then compile from the same tokens as before the
// map-per-slot form existed, and keep their registers, spills and scratch exactly (a body shared through a function moved them).
template <int W, int M>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(W == 4 ? 1 : 2, 8)))
void LL_SMALL_KERNEL(SmallArgs rd, RegConst rc LL_SMALL_MORE_ARGS)
{
    const int cap = rd.cap, capl = rd.capl;
    const f4 *map_surf = rd.map_surf;
    constexpr int NT = 64 * W;
    constexpr int K = W <= 2 ? M * W : 1;  // W <= 2: keys per lane of the sorting wavefront (register sort); W >= 4: the sort runs in LDS
    constexpr int NS = W <= 2 ? 1 : (M * NT <= 256 ? 256 : (M * NT <= 512 ? 512 : (M * NT <= 1024 ? 1024 : 2048)));  // ... over this many keys
    static_assert(M <= 16 && K <= 16 && M * NT <= 2048, "census rounds / sort keys per lane / LDS sort size");
    __shared__ SmallShared sh;
    extern __shared__ double s_dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = rd.order ? rd.order[blockIdx.x] : (int)blockIdx.x;
    RegState *st = rd.state + b;
    if (st->done) return;
    LL_SMALL_BIND_MAP  // (map-per-slot form: map_surf = the surface map of scan b)
    SmallBlocks B;
    {
        LL_AS_LDS double *p = (LL_AS_LDS double *)s_dyn;
        B.v0 = p, B.v1 = p + cap, B.v2 = p + 2 * cap, B.a0 = p + 3 * cap;
        B.a1 = p + 4 * cap, B.a2 = p + 4 * cap + capl;
        LL_AS_LDS float *q = (LL_AS_LDS float *)(p + 4 * cap + 2 * capl + (W >= 4 ? 2 * NS : 0));
        B.fx = q, B.fy = q + cap, B.fz = q + 2 * cap;
    }
    const int nC = rd.n_corner[b], nS = rd.n_surf[b];
    const int ncand = nC + nS;  // <= NT * M (the host chose M)
    if (ncand > NT * M) {       // (a launch that does not hold the scan must not answer for it: rejected and reported, ll_reg_collect)
        if (tid == 0) {
            st->aborted = 1;
            st->done = 1;
            st->icp_iters += 1;
        }
        return;
    }
    const size_t sb = (size_t)b * rd.cap_all;
    const unsigned char *flag0 = rd.blk_flag0 + sb;
#if defined(LL_SOLVE_TIMING) || defined(LL_LM_COUNTS)
    if (tid < 16) sh.tcyc[tid] = 0;
    __syncthreads();
#endif
    SM_T0(t_total);
    SM_T0(t_census);

    // ---- census (PCR:325, 425) in the reference's order: candidate c < nC is corner query c, else surface query c - nC -------------
    unsigned int act = 0;  // bit r: candidate r * NT + tid is a kept block
    int na = 0, nca = 0, nsa = 0;
#pragma unroll
    for (int r = 0; r < M; r++) {
        const int c = r * NT + tid;
        const int cc = c < ncand ? c : 0;
        const size_t slot = cc < nC ? (size_t)cc : (size_t)rd.cap_c + (cc - nC);
        const unsigned char fl = (c < ncand) ? gload_u8(flag0 + slot) : (unsigned char)0;
        if (fl & BLK_ACTIVE) {
            act |= 1u << r;
            na++;
        }
        if (fl & 8) {
            if (c < nC) nca++; else nsa++;
        }
    }
    {
        const unsigned long long tot = small_sum_u64<W>((unsigned long long)na | ((unsigned long long)nca << 20) | ((unsigned long long)nsa << 40), sh);
        na = (int)(tot & 0xfffffull);
        nca = (int)((tot >> 20) & 0xfffffull);
        nsa = (int)((tot >> 40) & 0xfffffull);
    }
    if (rc.subsample_seed && na > rc.max_blocks) {  // a13 (PCR:438-458): the random stream is indexed by the block's position in the reference's order
#pragma unroll
        for (int r = 0; r < M; r++) {
            if (!((act >> r) & 1u)) continue;
            if (subsample_drop_block(rc.subsample_seed, st->icp_iters, r * NT + tid, na, rc.max_blocks)) act &= ~(1u << r);
        }
    }
    // dense numbering of the kept blocks in candidate order: position = kept blocks of the earlier rounds + of the earlier wavefronts of
    // this round + of the lower lanes
    int pos[M];
    {
        int mine[M];
#pragma unroll
        for (int r = 0; r < M; r++) {
            const unsigned long long bal = __ballot((act >> r) & 1u);
            mine[r] = __popcll(bal & ((1ull << lane) - 1ull));
            if (lane == 0) sh.cnt[r][wave] = __popcll(bal);
        }
        __syncthreads();
        int base = 0, kept_lines = 0;
#pragma unroll
        for (int r = 0; r < M; r++) {
            int before = 0, round_total = 0;
#pragma unroll
            for (int w = 0; w < W; w++) {
                const int c = sh.cnt[r][w];
                if (w < wave) before += c;
                round_total += c;
            }
            pos[r] = base + before + mine[r];
            base += round_total;
        }
        // kept line blocks: kept candidates below nC (the lines come first in candidate order)
        {
            int kl = 0;
#pragma unroll
            for (int r = 0; r < M; r++)
                if (((act >> r) & 1u) && r * NT + tid < nC) kl++;
            kept_lines = (int)small_sum_u64<W>((unsigned long long)kl, sh);
        }
        if (tid == 0) {
            sh.n_eval = 0;
            sh.n_active = base;
            sh.nA = base;
            sh.nL = kept_lines;
            sh.n_corner_avail = nca;
            sh.n_surf_avail = nsa;
        }
    }
    SM_TACC(6, t_census);
    SM_T0(t_build);
    // ---- build: the kept blocks' constants -> LDS -------------------------------------------------------------------------------------
    {
        double pose_last[7];
#pragma unroll
        for (int i = 0; i < 7; i++) pose_last[i] = gload_f64(st->pose_last + i);
        const double *av = rd.blk_av + (size_t)b * 6 * rd.cap_all;
        const float4 *sfeat = rd.surf_feat + (size_t)b * rd.feat_stride_s;
#pragma unroll
        for (int r = 0; r < M; r++) {
            const int c = r * NT + tid;
            if (!((act >> r) & 1u)) continue;
            const int p = pos[r];
            if (c < nC) {
                const float4 f = gload_f4(rd.blk_f + sb + c);
                double a0, a1, a2, v0, v1, v2;
                av_load(av, rd.cap_all, c, true, a0, a1, a2, v0, v1, v2);
                B.fx[p] = f.x, B.fy[p] = f.y, B.fz[p] = f.z;
                B.v0[p] = v0, B.v1[p] = v1, B.v2[p] = v2;
                B.a0[p] = a0, B.a1[p] = a1, B.a2[p] = a2;
            } else {
                const int q = c - nC;
                const int4 t = gload_i4(rd.nn + sb + rd.cap_c + q);
                const f4 m0 = gload_pt(map_surf + (unsigned int)t.x), m1 = gload_pt(map_surf + (unsigned int)t.y), m2 = gload_pt(map_surf + (unsigned int)t.z);
                float fx, fy, fz;
                gload_f3(sfeat + q, fx, fy, fz);
                const double pa[3] = {(double)m0.x, (double)m0.y, (double)m0.z};
                const double pb[3] = {(double)m1.x, (double)m1.y, (double)m1.z};
                const double pc[3] = {(double)m2.x, (double)m2.y, (double)m2.z};
                double a_out[3] = {0.0, 0.0, 0.0}, v_out[3] = {0.0, 0.0, 0.0};
                (void)block_plane(pose_last, pa, pb, pc, a_out, v_out);  // (degenerate triples were never flagged active: build_one / the tile kernel)
                B.fx[p] = fx, B.fy[p] = fy, B.fz[p] = fz;
                B.v0[p] = v_out[0], B.v1[p] = v_out[1], B.v2[p] = v_out[2];
                B.a0[p] = a_out[0];
            }
        }
    }
    __syncthreads();
    SM_TACC(8, t_build);
    const int nA = sh.nA, nL = sh.nL;
    // from here on a thread's blocks are the DENSE ones r * NT + tid
    unsigned int live = 0;
#pragma unroll
    for (int r = 0; r < M; r++)
        if (r * NT + tid < nA) live |= 1u << r;

    // ---- prerun solve (PCR:463-474) ---------------------------------------------------------------------------------------------------
    small_lm<W>(B, rc, st->inc, rc.ceres_prerun_times, live, sh);
    int lm_iters = sh.ctl.iteration;

    // ---- loss-corrected L1 values at the prerun result (PCR:476-485), in registers -----------------------------------------------------
    double l1[M];
    SM_T0(t_l1);
    {
        constexpr int DEBLUR = 0;
        LL_CTX_DECL_SMALL(sh.ctl.x)
        double q_last[4];
#pragma unroll
        for (int i = 0; i < 4; i++) q_last[i] = gload_f64(st->pose_last + i);
#pragma unroll
        for (int r = 0; r < M; r++) {
            const int idx = r * NT + tid;
            double v1 = -1.0;
            if ((live >> r) & 1u) {
                const double f[3] = {(double)B.fx[idx], (double)B.fy[idx], (double)B.fz[idx]};
                const double v[3] = {B.v0[idx], B.v1[idx], B.v2[idx]};
                if (idx < nL) {
                    const double a[3] = {B.a0[idx], B.a1[idx], B.a2[idx]};
                    v1 = block_l1(BLK_LINE, R_, t_, f, a, v, rc.huber_a, q_last);
                } else {
                    const double a[3] = {B.a0[idx], 0.0, 0.0};
                    v1 = block_l1(BLK_PLANE, R_, t_, f, a, v, rc.huber_a, q_last);
                }
            }
            l1[r] = v1;
        }
    }
    SM_TACC(2, t_l1);
    SM_T0(t_sort);
    // ---- std::set de-duplication + rank select (PCR:153-161): one bitonic sort on the first wavefront --------------------------------
    if (W <= 2) {
        unsigned long long key[K];  // (the first wavefront's: its own M values per lane, then the other wavefront's)
#pragma unroll
        for (int k = 0; k < K; k++) {
            const double v = l1[k < M ? k : 0];
            key[k] = (k < M && v >= 0.0) ? (unsigned long long)__double_as_longlong(v) : 0xffffffffffffffffull;  // inactive slot or NaN (NaN never enters the set)
        }
        if (W > 1) {
            // the other wavefront hands its keys to the first one, 64 at a time through the 512 bytes of one wavefront's partial sums
            // (nothing is being summed now): which lane ends up with which key does not matter to a sort
            unsigned long long *xch = (unsigned long long *)&sh.red[0][0];
            static_assert(sizeof(sh.red) >= 64 * sizeof(unsigned long long), "exchange buffer");
#pragma unroll
            for (int w = 1; w < (W <= 2 ? W : 1); w++) {
#pragma unroll
                for (int r = 0; r < M; r++) {
                    if (wave == w) xch[lane] = key[r];
                    __syncthreads();
                    if (wave == 0) key[(w * M + r) < K ? (w * M + r) : 0] = xch[lane];
                    __syncthreads();
                }
            }
        }
        if (wave == 0) {
            wave_bitonic_sort<K>(key, lane);
            // element g = lane * K + k is the first of its value iff it differs from element g - 1
            const unsigned long long prev_last = (unsigned long long)__shfl_up((long long)key[K - 1], 1);
            unsigned int first = 0;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const unsigned long long pv = k == 0 ? prev_last : key[k - 1];
                const bool valid = key[k] != 0xffffffffffffffffull;
                if (valid && ((k == 0 && lane == 0) || key[k] != pv)) first |= 1u << k;
            }
            const int cnt = __popc(first);
            int incl = cnt;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int y = __shfl_up(incl, off);
                if (lane >= off) incl += y;
            }
            const int nu = __shfl(incl, 63);
            int target = (int)(rc.inlier_ratio * (double)nu);  // PCR:160
            if (target > nu - 1) target = nu - 1;
            if (nu == 0) {
                if (lane == 0) sh.thr = rc.inliner_dis;  // empty set: defined deviation (PCR:160 would dereference end())
            } else if (target >= incl - cnt && target < incl) {
                int rk = incl - cnt;
                unsigned long long sel = 0;
#pragma unroll
                for (int k = 0; k < K; k++) {
                    if ((first >> k) & 1u) {
                        if (rk == target) sel = key[k];
                        rk++;
                    }
                }
                sh.thr = fmax(rc.inliner_dis, __longlong_as_double((long long)sel));  // PCR:485
            }
        }
    } else {
        // four / eight wavefronts: no sort.  (A bitonic sort of the keys in LDS -- 66 barrier steps for 2 048 keys -- was a third of a
        // launch of the mapping loop's scans: 44 k of 149 k cycles.)  std::set semantics by an exact LDS hash table -- a key is inserted
        // with one 64-bit compare-and-swap; whoever finds its own key already there is a duplicate, exactly one lane per distinct value is
        // not, whatever the order of the atomics -- then a most-significant-digit-first radix select over the distinct keys, 8 bits per
        // pass: a 256-bin LDS histogram, one wavefront finds the digit that holds the wanted rank.
        LL_AS_LDS unsigned long long *tab = (LL_AS_LDS unsigned long long *)(B.a2 + capl);  // [2 * NS] slots, behind the line arrays
        constexpr unsigned int TS = 2u * NS;
        for (int e = tid; e < (int)TS; e += NT) tab[e] = 0xffffffffffffffffull;
        __syncthreads();
        unsigned int uniq = 0;  // bit r: l1[r] is the first of its value
#pragma unroll
        for (int r = 0; r < M; r++) {
            const double v = l1[r];
            if (!(v >= 0.0)) continue;  // inactive slot or NaN (NaN never enters the set)
            const unsigned long long key = (unsigned long long)__double_as_longlong(v);
            unsigned int hsh = (unsigned int)key * 0x9E3779B1u;
            hsh ^= hsh >> 15;
            hsh += (unsigned int)(key >> 32) * 0x85EBCA77u;
            hsh ^= hsh >> 13;
            unsigned int slot = hsh & (TS - 1u);
            for (;;) {  // (at most half of the slots are ever taken: the probe ends)
                const unsigned long long old = atomicCAS((unsigned long long *)&tab[slot], 0xffffffffffffffffull, key);
                if (old == 0xffffffffffffffffull) {
                    uniq |= 1u << r;
                    break;
                }
                if (old == key) break;
                slot = (slot + 1u) & (TS - 1u);
            }
        }
        const int nu = (int)small_sum_u64<W>((unsigned long long)__popc(uniq), sh);  // (its barriers: every insert has landed)
        int target = (int)(rc.inlier_ratio * (double)nu);  // PCR:160
        if (target > nu - 1) target = nu - 1;
        if (nu == 0) {
            if (tid == 0) sh.thr = rc.inliner_dis;  // empty set: defined deviation (PCR:160 would dereference end())
        } else {
            unsigned long long prefix = 0ull;
            int rank = target;
            for (int pass = 0; pass < 8; pass++) {
                const int shift = 56 - 8 * pass;
                if (tid < 256) sh.hist[tid] = 0;
                __syncthreads();
#pragma unroll
                for (int r = 0; r < M; r++) {
                    if (!((uniq >> r) & 1u)) continue;
                    const unsigned long long key = (unsigned long long)__double_as_longlong(l1[r]);
                    if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&sh.hist[(int)((key >> shift) & 255ull)], 1);
                }
                __syncthreads();
                if (wave == 0) {  // lane l sums bins 4 l .. 4 l + 3; the lane whose range holds the rank walks its four bins
                    const int b0 = sh.hist[4 * lane], b1 = sh.hist[4 * lane + 1], b2 = sh.hist[4 * lane + 2], b3 = sh.hist[4 * lane + 3];
                    const int part = b0 + b1 + b2 + b3;
                    int incl = part;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const int y = __shfl_up(incl, off);
                        if (lane >= off) incl += y;
                    }
                    const int below = incl - part;
                    if (rank >= below && rank < incl) {
                        int d = 4 * lane, cum = below;
                        if (cum + b0 <= rank) {
                            cum += b0;
                            d++;
                            if (cum + b1 <= rank) {
                                cum += b1;
                                d++;
                                if (cum + b2 <= rank) {
                                    cum += b2;
                                    d++;
                                }
                            }
                        }
                        sh.sel_digit = d;
                        sh.sel_rank = rank - cum;
                    }
                }
                __syncthreads();
                prefix = (prefix << 8) | (unsigned long long)sh.sel_digit;
                rank = sh.sel_rank;
            }
            if (tid == 0) sh.thr = fmax(rc.inliner_dis, __longlong_as_double((long long)prefix));  // PCR:485
        }
    }
    __syncthreads();
    SM_TACC(3, t_sort);
    SM_T0(t_prune);
    // ---- prune (PCR:487-499) -----------------------------------------------------------------------------------------------------------
    {
        const double thr = sh.thr;
        int keep = 0;
#pragma unroll
        for (int r = 0; r < M; r++) {
            if (!((live >> r) & 1u)) continue;
            if (l1[r] > thr)
                live &= ~(1u << r);
            else
                keep++;
        }
        keep = (int)small_sum_u64<W>((unsigned long long)keep, sh);
        if (tid == 0) sh.n_active = keep;
        if (tid < 7) sh.x_start[tid] = sh.ctl.x[tid];
        __syncthreads();
    }
    SM_TACC(7, t_prune);
    // ---- final solve (PCR:501-508) -------------------------------------------------------------------------------------------------------
    small_lm<W>(B, rc, sh.x_start, rc.ceres_max_iterations, live, sh);
    lm_iters += sh.ctl.iteration;
    solve_epilogue(rc, st, sh, lm_iters);
    if (tid == 0) st->last_work = sh.n_eval;  // next launch: the scans that worked longest start first
#if defined(LL_SOLVE_TIMING) || defined(LL_LM_COUNTS)
    SM_TACC(5, t_total);
    if (tid == 0)
        for (int i = 0; i < 16; i++) st->dbg_cycles[i] += sh.tcyc[i];
#endif
}

