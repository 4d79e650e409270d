// ll_api_reg.hip -- the registrar handle (ll_reg_*) of the C ABI: every ll_reg_enqueue_* form and the two drivers behind them,
// ll_reg_collect, the debug taps, ll_cloud_transform*.  This file owns the ordering of the registrar's stream behind the feature
// producers and the map-snapshot pins of the solve in flight.
#include "ll_api_internal.h"
#include "ll_reg_query.h"  // padded_block_count, LL_TABLE_MAX_BLOCKS: the host's refusal and the solver kernels count a scan's blocks alike

extern "C" void ll_reg_default_params(ll_reg_params *p)
{
    memset(p, 0, sizeof(*p));
    p->if_motion_deblur = 0;              // PCR:60
    p->icp_max_iterations = 20;           // PCR:89
    p->ceres_max_iterations = 100;        // PCR:90
    p->ceres_prerun_times = 2;            // PCR:91
    p->icp_line = 1;                      // PCR:50
    p->icp_plane = 1;                     // PCR:49
    p->if_line_feature_check = 0;         // PCR:46
    p->if_plane_feature_check = 0;        // PCR:48
    p->subsample_seed = 0;                // strict: no sub-sampling, too many features is an error
    p->current_frame_index = 101;
    p->mapping_init_accumulate_frames = 100;  // PCR:84
    p->maximum_allow_residual_block = 100000; // PCR:103
    p->force_all_iterations = 0;
    p->maximum_dis_line_for_match = 2.0;  // PCR:65
    p->maximum_dis_plane_for_match = 50.0; // PCR:64
    p->huber_a = 0.1;                     // PCR:220
    p->inliner_dis = 0.02;                // PCR:97
    p->inlier_ratio = 0.80;               // PCR:98
    p->minimum_icp_R_diff = 0.01;         // PCR:94
    p->minimum_icp_T_diff = 0.01;         // PCR:95
    p->para_max_angular_rate = 200.0f / 50.0f; // PCR:86
    p->para_max_speed = 100.0f / 50.0f;   // PCR:87
    p->max_final_cost = 100.0f;           // PCR:88
    p->minimum_pt_time_stamp = 0.f;       // PCR:92
    p->maximum_pt_time_stamp = 1.0f;      // PCR:93
}

extern "C" void ll_reg_destroy(ll_reg *r);
static int reg_create_impl(int32_t device, int32_t max_scans, int32_t max_features_per_scan, ll_reg *r)
{
    r->device = device;
    r->max_scans = max_scans;
    r->max_feat = max_features_per_scan;
    HC(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
    HC(hipEventCreateWithFlags(&r->ev_wait, hipEventDisableTiming));
    RegDev &d = r->dev;
    memset(&d, 0, sizeof(d));
    const size_t B = max_scans, F = max_features_per_scan;
    d.cap_c = (int)F;
    d.cap_s = (int)F;
    d.cap = d.cap_c + d.cap_s;
    int hc = 1;
    while (hc < 2 * d.cap) hc <<= 1;
    d.hash_cap = hc;
    DM(d.state, B);
    DM(d.blk_f, B * d.cap);
    DM(d.blk_av, B * 6 * d.cap);
    DM(d.blk_id, B * d.cap_s);
    {
        const int lim = d.cap_s < 61440 ? d.cap_s : 61440;  // LL_TABLE_MAX_BLOCKS: larger scans never take a plane-table path
        d.tab_cap = (lim + 4095) / 4096 * 4096;             // (<= 61440: private entries count down from tab_cap - 1, below the 16-bit sentinels)
    }
    DM(d.pl_tab, B * (size_t)d.tab_cap * 2);
    DM(d.blk_flag, B * d.cap);
    DM(d.nn, B * d.cap);
    DM(d.qperm, B * d.cap_s);
    DM(d.qsorted, B * d.cap_s);
    DM(d.qperm_c, B * LL_QSORT_CORNER_MAX);
    DM(d.qw, B * d.cap);
    DM(d.ref_q, B * d.cap);
    DM(d.ref_p, B * d.cap);
    DM(d.ref_s, B * d.cap);
    DM(d.blk_flag0, B * d.cap);
    DM(d.work_search, B * d.cap);
    DM(d.work_build, B * d.cap);
    d.n_chunks = (int)((F + 255) / 256);  // must match RQ_THREADS in ll_reg_query_kernels.hip
    DM(d.work_cnt, B * 4);
    DM(d.work_off, 3 * 2049);  // 3 prefix tables x (RL_MAX_SEG + 1), ll_reg_query_kernels.hip
    DM(d.grp_ctl, 2 * B + 1);
    DM(d.solve_order, B);
    DM(d.grp_part, B * 2 * LL_GRP * 28);
    DM(d.grp_xch, B * 2 * LL_GRP * 56);
    DM(d.blk_l1, B * d.cap);
    DM(d.hash, B * (size_t)d.hash_cap);
    DM(r->d_corner, B * F);
    DM(r->d_surf, B * F);
    DM(r->d_nc, B);
    DM(r->d_ns, B);
    DM(r->d_pose_tmp, 8);
    DM(r->d_map_tab, 2 * B);
    r->h_map_tab.resize(2 * B);
    HC(hipMemsetAsync(d.blk_flag, 0, B * d.cap, r->stream));  // (on the registrar's stream: a null-stream memset is not ordered with it)
    r->h_state.resize(B);
    r->h_nc.assign(B, 0);
    r->h_ns.assign(B, 0);
    return 0;
}

extern "C" int ll_reg_create(int32_t device, int32_t max_scans, int32_t max_features_per_scan, ll_reg **out)
{
    if (!out) return set_err("ll_reg_create", "null argument");
    if (max_scans < 1 || max_features_per_scan < 1) return set_err("ll_reg_create", "bad capacity");
    if ((int64_t)max_scans * 2 * max_features_per_scan >= 0x7fffffffLL)
        return set_err("ll_reg_create", "max_scans x 2 x max_features_per_scan must stay below 2^31 (work-list entries are 32-bit)");
    if (check_device(device)) return -1;
    ll_reg *r = new ll_reg();
    if (reg_create_impl(device, max_scans, max_features_per_scan, r)) {
        ll_reg_destroy(r);
        return -1;
    }
    *out = r;
    return 0;
}

extern "C" void ll_reg_destroy(ll_reg *r)
{
    if (!r) return;
    (void)hipSetDevice(r->device);
    RegDev &d = r->dev;
    void *ptrs[] = {d.state, d.blk_f, d.blk_av, d.blk_id, d.pl_tab, d.blk_flag, d.nn, d.qperm, d.qsorted, d.qperm_c, d.qw, d.ref_q, d.ref_p, d.ref_s, d.blk_flag0, d.work_search, d.work_build, d.work_cnt, d.work_off, d.grp_ctl, d.solve_order, d.grp_part, d.grp_xch, d.blk_l1, d.hash, d.dbg_idx, d.dbg_d2,
                    r->d_corner, r->d_surf, r->d_nc, r->d_ns, r->d_pose_tmp, r->d_map_tab, r->d_info, r->d_und, r->d_und_jobs, r->d_ts};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (r->hp_ts) (void)hipHostFree(r->hp_ts);
    for (hipEvent_t e : r->ev) (void)hipEventDestroy(e);
    if (r->ev_wait) (void)hipEventDestroy(r->ev_wait);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
}

extern "C" void *ll_reg_stream(ll_reg *r) { return r ? (void *)r->stream : nullptr; }

extern "C" int ll_reg_set_debug(ll_reg *r, int32_t enable)
{
    if (!r) return set_err("ll_reg_set_debug", "null handle");
    HC(hipSetDevice(r->device));
    if (enable & (16 | 64))
        return set_err("ll_reg_set_debug", "bits 4 and 6 selected the round-1 / round-2 solver forms, which were retired in round 6 (the plane-table and the "
                                           "general path are the only solver forms)");
    r->debug = enable;
    if ((enable & 1) && !r->dev.dbg_idx) {
        DM(r->dev.dbg_idx, (size_t)r->max_scans * r->dev.cap * 5);
        DM(r->dev.dbg_d2, (size_t)r->max_scans * r->dev.cap * 5);
    }
    return 0;
}

extern "C" int ll_reg_set_debug_knn_iteration(ll_reg *r, int32_t icp_iteration)
{
    if (!r) return set_err("ll_reg_set_debug_knn_iteration", "null handle");
    if (icp_iteration < 0) return set_err("ll_reg_set_debug_knn_iteration", "negative ICP iteration");
    r->debug_knn_iter = icp_iteration;
    return 0;
}

extern "C" int ll_reg_set_profiling(ll_reg *r, int32_t enable)
{
    if (!r) return set_err("ll_reg_set_profiling", "null handle");
    r->profiling = enable ? 1 : 0;
    return 0;
}

extern "C" int ll_reg_set_information(ll_reg *r, int32_t enable)
{
    if (!r) return set_err("ll_reg_set_information", "null handle");
    if (enable && !r->d_info) {  // (the first time the switch goes on: a registrar that never asks pays nothing)
        HC(hipSetDevice(r->device));
        DM(r->d_info, (size_t)r->max_scans);
        r->h_info.resize((size_t)r->max_scans);
    }
    r->info_enable = enable ? 1 : 0;  // read by the next enqueue
    return 0;
}

extern "C" int ll_reg_information(ll_reg *r, int32_t n_scans, ll_reg_information_record *out)
{
    static_assert(sizeof(ll_reg_information_record) == sizeof(InfoRecord), "ll_reg_information_record is the device record");
    if (!r) return set_err("ll_reg_information", "null handle");
    if (!out) return set_err("ll_reg_information", "null output");
    if (!r->info_collected) return set_err("ll_reg_information", "no registration has been collected since the last enqueue (call ll_reg_collect first)");
    if (!r->info_enqueued) return set_err("ll_reg_information", "the last enqueue was made with the information switch off (ll_reg_set_information)");
    if (n_scans != r->last_n_scans) return set_err("ll_reg_information", "n_scans differs from the last enqueue's");
    memcpy(out, r->h_info.data(), (size_t)n_scans * sizeof(InfoRecord));
    return 0;
}

extern "C" int ll_reg_information_time(ll_reg *r, float *ms)
{
    if (!r) return set_err("ll_reg_information_time", "null handle");
    if (!ms) return set_err("ll_reg_information_time", "null output");
    *ms = r->prof_ms[3];  // (0 without ll_reg_set_profiling, or when the last collected enqueue had the switch off)
    return 0;
}

// A time range per scan for the next enqueue with a map per slot (lock-step sequences: every slot runs from its own previous frame's
// last stamp to this frame's, laser_mapping.hpp:1336-1347).  One-shot like ll_history_set_gate_pose: the next ll_reg_enqueue_fe_maps /
// ll_reg_enqueue_fe_downsampled_maps takes the table, whether it succeeds or is refused.  The pairs wait in pinned memory and go up
// with that enqueue's other per-scan data.
extern "C" int ll_reg_set_time_ranges(ll_reg *r, const float *minimum_pt_time_stamp, const float *maximum_pt_time_stamp, int32_t n_scans)
{
    static const char *where = "ll_reg_set_time_ranges";
    if (!r) return set_err(where, "null handle");
    if (!minimum_pt_time_stamp || !maximum_pt_time_stamp) return set_err(where, "null argument");
    if (n_scans < 1 || n_scans > r->max_scans) return set_err(where, "n_scans out of range");
    if (!r->hp_ts) {
        HC(hipSetDevice(r->device));
        HC(hipHostMalloc((void **)&r->hp_ts, (size_t)r->max_scans * sizeof(float2), hipHostMallocDefault));
        DM(r->d_ts, (size_t)r->max_scans);
    }
    // (the staging is free: the enqueue that read it last has drained the stream behind its copy, reg_exchange_counts)
    for (int b = 0; b < n_scans; b++) r->hp_ts[b] = make_float2(minimum_pt_time_stamp[b], maximum_pt_time_stamp[b]);
    r->ts_pending = n_scans;
    return 0;
}

static int make_reg_const(const ll_reg_params *p, int debug, RegConst *c)
{
    debug &= ~(16 | 64);  // (retired solver forms; LL_DEBUG_OR cannot ask for them either)
    memset(c, 0, sizeof(*c));
    c->if_motion_deblur = p->if_motion_deblur;
    c->icp_max_iterations = p->icp_max_iterations;
    c->ceres_max_iterations = p->ceres_max_iterations;
    c->ceres_prerun_times = p->ceres_prerun_times;
    c->icp_line = p->icp_line;
    c->icp_plane = p->icp_plane;
    c->check_line_pca = p->if_line_feature_check;
    c->check_plane_pca = p->if_plane_feature_check;
    c->subsample_seed = (unsigned int)p->subsample_seed;
    c->max_blocks = p->maximum_allow_residual_block;
    c->force_all_iterations = p->force_all_iterations;
    c->debug_knn = debug & 1;
    c->force_general = (debug & 2) ? 1 : 0;
    c->knn_reuse = (debug & 4) ? 0 : 1;
    c->knn_reuse_from = (debug & 8) ? 1 : 2;  // bit 3: also try reuse at ICP iteration 1 (test coverage)
    c->solve_group = (debug & 32) ? 1 : 0;    // bit 5: never spread a scan over a group of workgroups (A/B); 0 = decide per batch size
    c->test_group_abort = (debug & 128) ? 1 : 0;  // bit 7: the grouped solver gives up at once (exercises the abort / reject path)
    c->knn_coop = (debug & 256) ? 0 : 1;  // bit 8: corner searches per lane everywhere instead of per wavefront where few (A/B, ll_knn_coop.h)
    c->knn_tile_last_sort = (debug & 8192) ? 0 : ((debug & 16384) ? 2 : 1);  // bits 13 / 14: A/B of the re-sort schedule (sort at iteration 0 only / at 0, 1, 2)
    c->no_solve_order = (debug & 262144) ? 1 : 0;  // bit 18: the small solver's workgroups in scan order (A/B)
    c->no_small_solver = (debug & 32768) ? 1 : 0;  // bit 15: small scans on the 512-thread solver too (A/B)
    c->small_waves = ((debug & 65536) && (debug & 131072)) ? 2 : ((debug & 65536) ? 1 : ((debug & 131072) ? 4 : 0));  // bits 16 / 17: the small solver with one / four wavefronts per scan whatever the batch size (tests)
    c->no_line_cache = (debug & 4096) ? 1 : 0;  // bit 12: no LDS copy of the line blocks in the solver (A/B)
    c->knn_tile = (debug & 512) ? 0 : ((debug & 1024) ? 1 : 2);  // bit 9: no tile search of the surface queries (A/B, ll_knn_tile.h); bit 10: tile
                                                                 // search only where all queries are searched, the reuse machinery for the rest
    c->max_d2_line_d = p->maximum_dis_line_for_match;
    c->max_d2_plane_d = p->maximum_dis_plane_for_match;
    // fp32 distances are compared against the double thresholds (PCR:254,353): d2 < thr  <=>  d2 < ceil_f32(thr)
    float fl = (float)p->maximum_dis_line_for_match, fp = (float)p->maximum_dis_plane_for_match;
    if ((double)fl < p->maximum_dis_line_for_match) fl = nextafterf(fl, INFINITY);
    if ((double)fp < p->maximum_dis_plane_for_match) fp = nextafterf(fp, INFINITY);
    c->max_d2_line = fl;
    c->max_d2_plane = fp;
    c->huber_a = p->huber_a;
    c->inliner_dis = p->inliner_dis;
    c->inlier_ratio = p->inlier_ratio;
    c->minimum_icp_R_diff = p->minimum_icp_R_diff;
    c->minimum_icp_T_diff = p->minimum_icp_T_diff;
    c->bound = (double)p->para_max_speed;
    c->para_max_angular_rate = p->para_max_angular_rate;
    c->max_final_cost = p->max_final_cost;
    c->min_ts = p->minimum_pt_time_stamp;
    c->max_ts = p->maximum_pt_time_stamp;
    return 0;
}

static void prof_begin(ll_reg *r, int cls)
{
    if (!r->profiling) return;
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    (void)hipEventRecord(a, r->stream);
    r->ev.push_back(a);
    r->ev.push_back(b);
    r->ev_class.push_back(cls);
}
static void prof_end(ll_reg *r)
{
    if (!r->profiling) return;
    (void)hipEventRecord(r->ev.back(), r->stream);
}

// ---- feature sources ---------------------------------------------------------------------------------------------------------------
// the registrar's stream behind the view's producers (work on its own stream is ordered already)
static int reg_wait(ll_reg *r, const FeatView &v)
{
    for (int i = 0; i < 2; i++) {
        if (!v.producer[i] || v.producer[i] == r->stream || (i == 1 && v.producer[1] == v.producer[0])) continue;
        HC(hipEventRecord(r->ev_wait, v.producer[i]));
        HC(hipStreamWaitEvent(r->stream, r->ev_wait, 0));
    }
    return 0;
}

// the one place that points the registrar at its features, ordered after their producers
static int reg_bind(ll_reg *r, const FeatView &v)
{
    if (reg_wait(r, v)) return -1;
    r->dev.corner_feat = v.corner;
    r->dev.surf_feat = v.surf;
    r->dev.n_corner = v.n_corner;
    r->dev.n_surf = v.n_surf;
    r->dev.feat_stride_c = v.stride_c;
    r->dev.feat_stride_s = v.stride_s;
    return 0;
}

// ---- what the two drivers share ----------------------------------------------------------------------------------------------------
static int reg_params_check(const char *where, const ll_reg *r, int n_scans, const ll_reg_params *prm, const double *poses_last,
                            const double *poses_curr)
{
    if (!prm || !poses_last || !poses_curr) return set_err(where, "null argument");
    if (n_scans < 1 || n_scans > r->max_scans) return set_err(where, "n_scans out of range");
    if (prm->icp_max_iterations < 0 || prm->ceres_max_iterations < 0 || prm->ceres_prerun_times < 0)
        return set_err(where, "negative iteration count");
    if (prm->icp_max_iterations > (1 << 19)) return set_err(where, "icp_max_iterations above 524288");  // (the grouped solver tags its exchanges with the launch number in 20 bits)
    return 0;
}

struct PinGuard {  // an enqueue that fails after reg_begin must not leave its pins behind
    ll_reg *r;
    bool keep = false;
    ~PinGuard()
    {
        if (!keep) {
            // kernels of this enqueue may already be in flight on the snapshots (a failure inside the ICP loop): they must
            // have drained before the pins go and ll_map_upload / a refresh may recycle the buffers
            (void)hipStreamSynchronize(r->stream);
            r->pinned[0].reset();
            r->pinned[1].reset();
            r->pinned_maps.clear();
        }
    }
};

// the solver constants of this enqueue (*debug, if asked for: the debug bits they were made from), and no pin left from an earlier one
static int reg_begin(ll_reg *r, const ll_reg_params *prm, int *debug = nullptr)
{
    static const int debug_or = getenv("LL_DEBUG_OR") ? atoi(getenv("LL_DEBUG_OR")) : 0;  // (A/B runs of unmodified drivers: bits of ll_reg_set_debug)
    if (debug) *debug = r->debug | debug_or;
    make_reg_const(prm, r->debug | debug_or, &r->rc);
    r->rc.debug_knn_iter = r->debug_knn_iter;
    // A solve enqueued earlier on this handle and never collected still reads its snapshots: let it finish before its pins are
    // replaced (the snapshots could otherwise be recycled and rebuilt under its kernels by a concurrent ll_map_upload / refresh).
    if (r->pinned[0] || r->pinned[1] || !r->pinned_maps.empty()) HC(hipStreamSynchronize(r->stream));
    r->pinned[0].reset();
    r->pinned[1].reset();
    r->pinned_maps.clear();
    r->info_enqueued = 0;
    r->info_collected = 0;
    r->collected_scans = 0;
    r->und_valid = 0;
    r->ts_last = 0;
    return 0;
}

static void reg_init_state(RegState &s, int b, const double *poses_last, const double *poses_curr, const double *poses_incre, bool run)
{
    memset(&s, 0, sizeof(s));
    for (int i = 0; i < 7; i++) {
        s.pose_last[i] = poses_last[7 * b + i];
        s.pose_curr[i] = poses_curr[7 * b + i];
        s.inc[i] = poses_incre ? poses_incre[7 * b + i] : (i == 3 ? 1.0 : 0.0);
    }
    s.prev_q[3] = 1.0;  // q_last_optimize(1,0,0,0), PCR:204
    s.gated = run ? 0 : 1;
    s.done = run ? 0 : 1;
    s.result = 1;
    s.accepted = 1;
}

// States (and, for a map per slot, the grid table the driver filled) to the device, the feature counts to r->h_nc / r->h_ns;
// returns with the stream drained -- or, for one scan whose counts the caller knows (`known`), without waiting at all
static int reg_exchange_counts(ll_reg *r, int n_scans, bool map_tab, const int *known = nullptr)
{
    for (hipEvent_t e : r->ev) (void)hipEventDestroy(e);
    r->ev.clear();
    r->ev_class.clear();
    HC(hipMemcpyAsync(r->dev.state, r->h_state.data(), (size_t)n_scans * sizeof(RegState), hipMemcpyHostToDevice, r->stream));
    if (map_tab) HC(hipMemcpyAsync(r->d_map_tab, r->h_map_tab.data(), (size_t)n_scans * 2 * sizeof(Grid), hipMemcpyHostToDevice, r->stream));
    // feature counts on the host: launch geometry, and the sub-sampling precondition (the reference's random
    // drop, PCR:232-238,339-345,438-458, is not reproduced)
    if (known) {  // (one scan whose {corner, surface} counts the caller has on the host already: nothing to wait for)
        r->h_nc[0] = known[0];
        r->h_ns[0] = known[1];
        return 0;
    }
    HC(hipMemcpyAsync(r->h_nc.data(), r->dev.n_corner, (size_t)n_scans * sizeof(int), hipMemcpyDeviceToHost, r->stream));
    HC(hipMemcpyAsync(r->h_ns.data(), r->dev.n_surf, (size_t)n_scans * sizeof(int), hipMemcpyDeviceToHost, r->stream));
    HC(hipStreamSynchronize(r->stream));
    return 0;
}

// the two size refusals (`cite`: what the entry point's message says about the reference's sub-sampling, in its own words)
static int reg_size_check(const char *where, const ll_reg *r, const ll_reg_params *prm, int max_nc, int max_ns, const char *cite)
{
    if (max_nc > r->dev.cap_c || max_ns > r->dev.cap_s) return set_err(where, "feature count exceeds the registrar capacity");
    if (!prm->subsample_seed && (max_nc > prm->maximum_allow_residual_block || max_ns > prm->maximum_allow_residual_block))
        return set_err(where, (std::string("feature count exceeds maximum_allow_residual_block and subsample_seed is 0 (strict mode): raise the "
                                           "limit, or set a seed to get the reference's sub-sampling ") + cite + "with a reproducible random stream").c_str());
    return 0;
}

// gc / gs: the grids every scan ran against, or map_tab: the device table of a map per slot (then gc / gs are not read)
// ts_tab: the device table of a time range per scan (a map per slot with motion deblur), else nullptr
static int reg_finish(ll_reg *r, int n_scans, PinGuard &pin_guard, const Grid &gc, const Grid &gs, const Grid *map_tab, const float2 *ts_tab = nullptr)
{
    if (r->info_enable) {
        // here the states still hold the last iteration's increment and pose_last, and the map snapshots are pinned
        prof_begin(r, 3);
        launch_reg_information(r->dev, r->rc, gc, gs, map_tab, r->d_info, n_scans, r->stream, ts_tab);
        prof_end(r);
        r->info_enqueued = 1;
    }
    prof_begin(r, 2);
    launch_reg_finalize(r->dev, r->rc, n_scans, r->stream);
    prof_end(r);
    HC(hipGetLastError());
    pin_guard.keep = true;  // released by ll_reg_collect
    return 0;
}

// ---- one map for the batch -----------------------------------------------------------------------------------------------------------
// The first thing every single-map entry point does with its handle: a table of time ranges that is pending (ll_reg_set_time_ranges)
// is dropped and the call refused, whatever else the call would have been refused for -- not silently ignored, and never left for a
// later enqueue: a caller that set a range per scan expects a map per slot behind it.
static int reg_refuse_pending_ranges(const char *where, ll_reg *r)
{
    if (!r || !r->ts_pending) return 0;
    r->ts_pending = 0;
    return set_err(where, "a table of time ranges is pending (ll_reg_set_time_ranges): it applies to the entry points with a map per slot "
                          "only and has been dropped");
}

// common launch sequence; reg_bind has set the feature pointers in r->dev
static int reg_enqueue(const char *where, ll_reg *r, const ll_map *map, int n_scans, const ll_reg_params *prm, const double *poses_last,
                       const double *poses_curr, const double *poses_incre, const int *known_counts = nullptr)
{
    if (!map) return set_err(where, "null argument");
    if (reg_params_check(where, r, n_scans, prm, poses_last, poses_curr)) return -1;
    if (map->device != r->device) return set_err(where, "map lives on another device");
    int debug = 0;
    if (reg_begin(r, prm, &debug)) return -1;
    PinGuard pin_guard{r};
    // PCR:199 gate
    // the snapshots this solve runs against, whatever ll_map_upload / ll_history_refresh* publish meanwhile
    r->pinned[0] = map_pin(map, 0);
    r->pinned[1] = map_pin(map, 1);
    const MapKind empty_kind{};
    const MapKind &mk0 = r->pinned[0] ? r->pinned[0]->mk : empty_kind, &mk1 = r->pinned[1] ? r->pinned[1]->mk : empty_kind;
    const bool run = mk0.n > 0 && mk1.n > 50 && prm->current_frame_index > prm->mapping_init_accumulate_frames;
    r->last_gated = run ? 0 : 1;
    r->last_n_scans = n_scans;
    for (int b = 0; b < n_scans; b++) reg_init_state(r->h_state[b], b, poses_last, poses_curr, poses_incre, run);
    if (reg_exchange_counts(r, n_scans, false, n_scans == 1 ? known_counts : nullptr)) return -1;
    int max_nc = 0, max_ns = 0;
    for (int b = 0; b < n_scans; b++) {
        max_nc = r->h_nc[b] > max_nc ? r->h_nc[b] : max_nc;
        max_ns = r->h_ns[b] > max_ns ? r->h_ns[b] : max_ns;
    }
    if (reg_size_check(where, r, prm, max_nc, max_ns, "(point_cloud_registration.hpp:232-238,339-345,438-458) ")) return -1;
    if (prm->subsample_seed && (max_nc > 2 * prm->maximum_allow_residual_block || max_ns > 2 * prm->maximum_allow_residual_block))
        r->rc.knn_reuse = 0;  // skipped features change from iteration to iteration: every iteration searches
    // Scans of thousands of surface queries: the tile search (ll_knn_kernels.hip) takes them, in every ICP iteration -- searching
    // all of them costs less than classifying them against reuse records and searching the lists that leaves
    // (small batches are latency chains, not issue-bound: the wavefront-per-query searches and the short work lists serve them better --
    //  single scan 2.24 ms against 2.49 with a tile launch per iteration; debug bit 11 forces the tile search for tests)
    if (max_ns < LL_KNN_TILE_MIN_SURF || max_ns > LL_KNN_TILE_MAX_SURF || (n_scans <= LL_KNN_COOP_MAX_SCANS && !(debug & 2048))) r->rc.knn_tile = 0;
    // Scans sorted in segments (more than LL_KNN_TILE_SEG surface queries: Mid-100) keep the reuse machinery behind the tile search of ICP
    // iterations 0 / 1: measured on C3 (bench_c3.py, k-NN class per step) 6.7 ms against 10.3 ms with a tile search in every iteration and
    // 7.2 ms without the tile search
    if (r->rc.knn_tile == 2 && max_ns > LL_KNN_TILE_SEG) r->rc.knn_tile = 1;
    if (r->rc.knn_tile == 2) r->rc.knn_reuse = 0;
    // ... until the late iterations, where most lists provably hold (profiles/knn_sparse_gate.json: 23 % of the C2 batch's surface queries
    // have left their order budget at ICP iteration 4, 4 % at iteration 9): from LL_KNN_SPARSE_FROM on, one streaming pass compares every query with
    // the 16-byte record its last search left and the tile search takes the rest, compacted into whole wavefronts in cell order
    // (ll_knn_kernels.hip; the round-3 form that lost against searching everything sent them to per-lane ring searches).  The records
    // lie in the cell order, so they start once it is final (knn_tile_last_sort).  Not where a query changes without moving
    // (sub-sampling), where the block is more than the list (PCA checks) or where the tile kernel does not transform (motion deblur);
    // debug bit 19 restores the search of everything (A/B, tests).
    r->rc.knn_sparse_from = 0;
    if (r->rc.knn_tile == 2 && !(debug & 524288) && !prm->subsample_seed && !r->rc.check_line_pca && !r->rc.check_plane_pca && !r->rc.if_motion_deblur) {
        static const int from_env = getenv("LL_KNN_SPARSE_FROM") ? atoi(getenv("LL_KNN_SPARSE_FROM")) : 0;  // (A/B runs of unmodified drivers)
        const int from = from_env > 0 ? from_env : LL_KNN_SPARSE_FROM;
        r->rc.knn_sparse_from = from > r->rc.knn_tile_last_sort + 1 ? from : r->rc.knn_tile_last_sort + 1;
    }
    // Small batches leave most of the chip idle with one workgroup per scan: spread each scan's cost evaluations over a
    // group of LL_GRP workgroups (ll_reg_solve_fast.h, group_*).  Compact scans only; the others run on the group's first.
    // A scan whose records (nearly) fit one CU's LDS cache gains nothing from it and pays ~3.5 us per exchange: voxel-filtered
    // clouds of a few thousand features (the mapping loop, Q-pipe) stay on one workgroup.
    r->rc.solve_group = (r->rc.solve_group == 1 || n_scans > LL_GRP_MAX_SCANS || r->rc.if_motion_deblur || r->rc.force_general ||
                         max_nc + max_ns < LL_GRP_MIN_BLOCKS) ? 1 : LL_GRP;
    if (run) {
        if (!mk0.pts || !mk1.pts) return set_err(where, "map not uploaded (or converted to fp16 points: the registrar needs the fp32 records)");
        // the searches of a registration that reuses neighbours prune with a guard band (ll_knn_core.h Grid::guard): ~8 % more
        // candidates per search, displacement budgets set by the true 6th neighbour, a third fewer searches in the late iterations
        Grid g0 = mk0.grid, g1 = mk1.grid;
        g0.guard = g1.guard = r->rc.knn_reuse ? 0.05f : 0.0f;
        if (r->rc.solve_group > 1)  // the exchange granules carry (launch number, exchange number) tags: none may survive from an earlier registration
            HC(hipMemsetAsync(r->dev.grp_xch, 0, (size_t)n_scans * 2 * LL_GRP * 56 * sizeof(unsigned long long), r->stream));
        for (int it = 0; it < prm->icp_max_iterations; it++) {
            r->rc.xch_epoch = it + 1;
            prof_begin(r, 0);
            launch_reg_knn_build(r->dev, r->rc, g0, g1, n_scans, it, max_nc, max_ns, r->stream);
            prof_end(r);
            prof_begin(r, 1);
            if (r->rc.solve_group > 1) HC(hipMemsetAsync(r->dev.grp_ctl, 0, (size_t)(2 * n_scans + 1) * sizeof(int), r->stream));
            launch_reg_solve(r->dev, r->rc, mk1.grid, n_scans, max_nc, max_ns, it, r->stream);
            prof_end(r);
        }
    }
    return reg_finish(r, n_scans, pin_guard, mk0.grid, mk1.grid, nullptr);
}

extern "C" int ll_reg_collect(ll_reg *r, int32_t n_scans, double *poses_curr, double *poses_incre, ll_reg_report *reports,
                              int32_t *results)
{
    if (!r) return set_err("ll_reg_collect", "null handle");
    if (n_scans < 1 || n_scans > r->max_scans) return set_err("ll_reg_collect", "n_scans out of range");
    HC(hipSetDevice(r->device));
    HC(hipMemcpyAsync(r->h_state.data(), r->dev.state, (size_t)n_scans * sizeof(RegState), hipMemcpyDeviceToHost, r->stream));
    if (r->info_enqueued)  // the records ride in the same wait
        HC(hipMemcpyAsync(r->h_info.data(), r->d_info, (size_t)r->last_n_scans * sizeof(InfoRecord), hipMemcpyDeviceToHost, r->stream));
    HC(hipStreamSynchronize(r->stream));
    r->info_collected = 1;
    r->collected_scans = n_scans < r->last_n_scans ? n_scans : r->last_n_scans;
    r->pinned[0].reset();  // the solve has left the device: its map snapshots may be recycled
    r->pinned[1].reset();
    r->pinned_maps.clear();
    int n_aborted = 0;
    for (int b = 0; b < n_scans; b++) {
        const RegState &s = r->h_state[b];
        n_aborted += s.aborted ? 1 : 0;
        for (int i = 0; i < 7; i++) {
            if (poses_curr) poses_curr[7 * b + i] = s.pose_curr[i];
            if (poses_incre) poses_incre[7 * b + i] = s.inc[i];
        }
        if (results) results[b] = s.result;
        if (reports) {
            ll_reg_report &rp = reports[b];
            rp.final_cost = s.final_cost;
            rp.initial_cost = s.initial_cost;
            rp.inlier_threshold = s.inlier_thr;
            rp.angular_diff_deg = s.angular_diff;
            rp.t_diff = s.t_diff;
            rp.icp_iterations = s.icp_iters;
            rp.n_blocks_last = s.n_blocks_last;
            rp.corner_avail = s.corner_avail;
            rp.surf_avail = s.surf_avail;
            rp.lm_iterations_total = s.lm_total;
            rp.accepted = s.accepted;
            rp.gated = s.gated;
            rp.aborted = s.aborted ? 1 : 0;
        }
    }
    if (r->profiling) {
        for (int k = 0; k < 4; k++) {
            r->prof_ms[k] = 0.f;
            r->prof_launches[k] = 0;
        }
        for (size_t i = 0; i < r->ev_class.size(); i++) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, r->ev[2 * i], r->ev[2 * i + 1]) == hipSuccess) {
                r->prof_ms[r->ev_class[i]] += ms;
                r->prof_launches[r->ev_class[i]]++;
            }
        }
    }
    if (n_aborted) {
        // Not an error of the call: every output is filled in, the affected scans come back rejected (result 0, report.aborted 1,
        // pose restored) like any registration the reference rejects, the others are valid.  The count is the return value and
        // ll_last_error() says what happened.
        (void)set_err("ll_reg_collect", "a group barrier of the small-batch solver timed out (device oversubscribed?): the affected scans were rejected");
        return n_aborted;
    }
    return 0;
}

extern "C" int ll_debug_quintic(int32_t device, const double *args10, int32_t n, double *out_sequential, double *out_wavefront)
{
    if (!args10 || !out_sequential || !out_wavefront || n < 0) return set_err("ll_debug_quintic", "bad argument");
    if (check_device(device)) return -1;
    double *d_a = nullptr, *d_s = nullptr, *d_w = nullptr;
    const size_t m = (size_t)(n > 0 ? n : 1);
    HC(hipMalloc((void **)&d_a, m * 10 * sizeof(double)));
    HC(hipMalloc((void **)&d_s, m * sizeof(double)));
    HC(hipMalloc((void **)&d_w, m * sizeof(double)));
    int rc = 0;
    if (hipMemcpy(d_a, args10, (size_t)n * 10 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    if (!rc) {
        launch_debug_quintic(d_a, n, d_s, d_w, nullptr);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out_sequential, d_s, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_wavefront, d_w, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
            rc = -1;
    }
    (void)hipFree(d_a);
    (void)hipFree(d_s);
    (void)hipFree(d_w);
    return rc ? set_err("ll_debug_quintic", "device error") : 0;
}

extern "C" int ll_debug_lm_sequence(int32_t device, const double *hdr12, const double *evals28, int32_t n, int32_t max_calls, void *out_lane0,
                                    void *out_wavefront, int32_t *ret_lane0, int32_t *ret_wavefront, int32_t *ctl_bytes)
{
    if (!ctl_bytes || n < 0 || max_calls < 0) return set_err("ll_debug_lm_sequence", "bad argument");
    *ctl_bytes = debug_lm_ctl_bytes();
    if (n == 0 || max_calls == 0) return 0;  // (the size alone)
    if (!hdr12 || !evals28 || !out_lane0 || !out_wavefront || !ret_lane0 || !ret_wavefront) return set_err("ll_debug_lm_sequence", "bad argument");
    if (check_device(device)) return -1;
    const size_t slots = (size_t)n * (size_t)max_calls, img = slots * (size_t)*ctl_bytes;
    double *d_h = nullptr, *d_e = nullptr;
    unsigned int *d_s = nullptr, *d_w = nullptr;
    int *d_rs = nullptr, *d_rw = nullptr;
    HC(hipMalloc((void **)&d_h, (size_t)n * 12 * sizeof(double)));
    HC(hipMalloc((void **)&d_e, slots * 28 * sizeof(double)));
    HC(hipMalloc((void **)&d_s, img));
    HC(hipMalloc((void **)&d_w, img));
    HC(hipMalloc((void **)&d_rs, slots * sizeof(int)));
    HC(hipMalloc((void **)&d_rw, slots * sizeof(int)));
    int rc = 0;
    if (hipMemcpy(d_h, hdr12, (size_t)n * 12 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_e, evals28, slots * 28 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_s, 0, img) != hipSuccess ||
        hipMemset(d_w, 0, img) != hipSuccess || hipMemset(d_rs, 0xff, slots * sizeof(int)) != hipSuccess ||
        hipMemset(d_rw, 0xff, slots * sizeof(int)) != hipSuccess)
        rc = -1;
    if (!rc) {
        launch_debug_lm_sequence(d_h, d_e, n, max_calls, d_s, d_w, d_rs, d_rw, nullptr);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out_lane0, d_s, img, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_wavefront, d_w, img, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(ret_lane0, d_rs, slots * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(ret_wavefront, d_rw, slots * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
            rc = -1;
    }
    (void)hipFree(d_h);
    (void)hipFree(d_e);
    (void)hipFree(d_s);
    (void)hipFree(d_w);
    (void)hipFree(d_rs);
    (void)hipFree(d_rw);
    return rc ? set_err("ll_debug_lm_sequence", "device error") : 0;
}

extern "C" int ll_reg_debug_cycles(ll_reg *r, int32_t scan, long long out[16])
{
    if (!r || scan < 0 || scan >= r->max_scans) return set_err("ll_reg_debug_cycles", "bad argument");
    for (int i = 0; i < 16; i++) out[i] = r->h_state[scan].dbg_cycles[i];
    return 0;
}

extern "C" int ll_reg_debug_worklists(ll_reg *r, int32_t n_scans, int64_t out[4])
{
    if (!r || !out || n_scans < 1 || n_scans > r->max_scans) return set_err("ll_reg_debug_worklists", "bad argument");
    HC(hipSetDevice(r->device));
    const size_t n = (size_t)n_scans * 4;  // work_cnt: [scan][kind][searched, re-sorted] of the last re-query launch
    std::vector<int> h(n);
    HC(hipStreamSynchronize(r->stream));
    HC(hipMemcpy(h.data(), r->dev.work_cnt, n * sizeof(int), hipMemcpyDeviceToHost));
    out[0] = out[1] = out[2] = out[3] = 0;
    for (size_t i = 0; i < n; i++) out[i & 3] += h[i];
    return 0;
}

extern "C" int ll_reg_kernel_times(ll_reg *r, float ms[3], int32_t launches[3])
{
    if (!r) return set_err("ll_reg_kernel_times", "null handle");
    for (int k = 0; k < 3; k++) {
        if (ms) ms[k] = r->prof_ms[k];
        if (launches) launches[k] = r->prof_launches[k];
    }
    return 0;
}

// the extractor's capacities against the registrar's (the four _fe forms)
static int reg_fe_fits(const char *where, const ll_reg *r, const ll_fe *fe, int n_scans)
{
    if (n_scans > fe->prm.max_scans) return set_err(where, "n_scans exceeds the extractor capacity");
    if (fe->prm.max_points > r->max_feat) return set_err(where, "registrar feature capacity < extractor max_points");
    return 0;
}

extern "C" int ll_reg_enqueue_fe(ll_reg *r, const ll_map *map, ll_fe *fe, int32_t n_scans, const ll_reg_params *prm,
                                 const double *poses_last, const double *poses_curr, const double *poses_incre)
{
    static const char *where = "ll_reg_enqueue_fe";
    if (reg_refuse_pending_ranges(where, r)) return -1;
    if (!r || !fe) return set_err(where, "null handle");
    if (fe->prm.device != r->device) return set_err(where, "extractor lives on another device");
    if (reg_fe_fits(where, r, fe, n_scans)) return -1;
    HC(hipSetDevice(r->device));
    if (reg_bind(r, feat_view(fe))) return -1;  // order after the extractor's stream
    return reg_enqueue(where, r, map, n_scans, prm, poses_last, poses_curr, poses_incre);
}

// ---- a map per slot ---------------------------------------------------------------------------------------------------------------
// what can be refused before anything is launched
// the pending table of time ranges, taken by this enqueue whatever becomes of it (one-shot): its n_scans, or 0 when none was set
static int reg_take_time_ranges(ll_reg *r)
{
    const int n = r->ts_pending;
    r->ts_pending = 0;
    return n;
}

// ts_n: what reg_take_time_ranges answered
static int reg_maps_check(const char *where, ll_reg *r, const ll_map *const *maps, int n_scans, const ll_reg_params *prm, const double *poses_last,
                          const double *poses_curr, int ts_n)
{
    if (!r || !maps) return set_err(where, "null argument");
    if (reg_params_check(where, r, n_scans, prm, poses_last, poses_curr)) return -1;
    if (ts_n && ts_n != n_scans) return set_err(where, "the table of time ranges was set for another n_scans (ll_reg_set_time_ranges): dropped");
    if (prm->if_motion_deblur && !ts_n)
        return set_err(where, "motion deblur is not supported with a map per slot without a time range per scan (if_motion_deblur must be 0, or "
                              "ll_reg_set_time_ranges in front of this call): the params' range is one pair for the batch");
    for (int b = 0; b < n_scans; b++)
        if (maps[b] && maps[b]->device != r->device) return set_err(where, "map lives on another device");
    return 0;
}

// reg_enqueue with a map per slot; reg_bind has set the feature pointers in r->dev and reg_maps_check passed.  The gate of PCR:199 is
// decided per slot from that slot's map and frame index; maps[b] == nullptr is an idle slot (comes back gated).
// deblur (reg_maps_check: only with a table of time ranges taken, r->hp_ts[0 .. n_scans)): the reference's *_mb problem per slot, slot b
// over its own range -- the searches as below, the transform and the block constants with the slot's range, and solve_big<1> for every
// running slot (ll_reg_big_maps_kernels.hip), which is what the single-map entry points give a deblur scan of any size.
static int reg_enqueue_maps(const char *where, ll_reg *r, const ll_map *const *maps, int n_scans, const ll_reg_params *prm, const int32_t *frame_index,
                            const double *poses_last, const double *poses_curr, const double *poses_incre)
{
    const bool deblur = prm->if_motion_deblur != 0;
    if (reg_begin(r, prm)) return -1;
    PinGuard pin_guard{r};
    r->rc.knn_tile = 0;   // (no table form: their work items are not bound to one scan per workgroup; the lists are the same bit for bit)
    r->rc.knn_reuse = 0;
    // every distinct map is pinned once: slots that name the same handle see the same pair of snapshots
    std::vector<const ll_map *> seen;
    std::vector<int> pin_of(n_scans, -1);
    for (int b = 0; b < n_scans; b++) {
        if (!maps[b]) continue;
        size_t k = 0;
        while (k < seen.size() && seen[k] != maps[b]) k++;
        if (k == seen.size()) {
            seen.push_back(maps[b]);
            r->pinned_maps.push_back(map_pin(maps[b], 0));
            r->pinned_maps.push_back(map_pin(maps[b], 1));
        }
        pin_of[b] = (int)k;
    }
    const MapKind empty_kind{};
    int n_run = 0;
    for (int b = 0; b < n_scans; b++) {
        const MapSnap *s0 = pin_of[b] >= 0 ? r->pinned_maps[2 * pin_of[b]].get() : nullptr, *s1 = pin_of[b] >= 0 ? r->pinned_maps[2 * pin_of[b] + 1].get() : nullptr;
        const MapKind &mk0 = s0 ? s0->mk : empty_kind, &mk1 = s1 ? s1->mk : empty_kind;
        const int fi = frame_index ? frame_index[b] : prm->current_frame_index;
        const bool run = mk0.n > 0 && mk1.n > 50 && fi > prm->mapping_init_accumulate_frames;  // PCR:199, per slot
        if (run && (!mk0.pts || !mk1.pts)) return set_err(where, "map not uploaded (or converted to fp16 points: the registrar needs the fp32 records)");
        Grid g0{}, g1{};
        if (run) g0 = mk0.grid, g1 = mk1.grid;  // (guard 0: nothing reuses neighbours here)
        g0.guard = g1.guard = 0.0f;
        r->h_map_tab[2 * b] = g0;
        r->h_map_tab[2 * b + 1] = g1;
        n_run += run ? 1 : 0;
        reg_init_state(r->h_state[b], b, poses_last, poses_curr, poses_incre, run);
    }
    r->last_gated = n_run ? 0 : 1;
    r->last_n_scans = n_scans;
    if (deblur) {  // the ranges go up with the states and the grid table, ahead of the one wait reg_exchange_counts makes anyway
        HC(hipMemcpyAsync(r->d_ts, r->hp_ts, (size_t)n_scans * sizeof(float2), hipMemcpyHostToDevice, r->stream));
        // d_ts is rewritten HERE, behind reg_begin, and nowhere else: reg_undistort_records reads it lazily after the collect, and reg_begin
        // has just cleared und_valid / collected_scans -- an upload inside ll_reg_set_time_ranges could change the ranges under the records
        // of a registration that is still being read (a setter followed by a refused enqueue)
        r->ts_last = 1;
    }
    if (reg_exchange_counts(r, n_scans, true)) return -1;
    int max_nc = 0, max_ns = 0;  // over the slots that run: the others launch nothing
    RegMapsClasses cls{};        // ... and per solver form (reg_maps_class: the form each scan would get alone)
    int max_tot[4] = {0, 0, 0, 0};
    cls.grp_min = r->rc.solve_group == 1 ? 0x7fffffff : LL_GRP_MIN_BLOCKS;  // (debug bit 5: no groups)
    for (int b = 0; b < n_scans; b++) {
        if (r->h_state[b].done) continue;
        const int nc = r->h_nc[b], ns = r->h_ns[b], c = reg_maps_class(r->rc, nc, ns, cls.grp_min);
        max_nc = nc > max_nc ? nc : max_nc;
        max_ns = ns > max_ns ? ns : max_ns;
        cls.n[c]++;
        cls.max_nc[c] = nc > cls.max_nc[c] ? nc : cls.max_nc[c];
        cls.max_ns[c] = ns > cls.max_ns[c] ? ns : cls.max_ns[c];
        max_tot[c] = nc + ns > max_tot[c] ? nc + ns : max_tot[c];
    }
    // The small solver sizes itself (wavefronts, rounds, LDS) by max_nc + max_ns.  The two maxima may come from different scans and add up to
    // more than any scan has -- beyond 1024 for a class whose scans all stay below, which would select the eight-wavefront form for scans that
    // take the four-wavefront form alone.  Hand it the largest scan's total instead (only the sum and max_nc are read).
    for (int c = 0; c < 2; c++) cls.max_ns[c] = max_tot[c] - cls.max_nc[c];
    if (reg_size_check(where, r, prm, max_nc, max_ns, "")) return -1;
    r->rc.solve_group = cls.n[3] ? LL_GRP : 1;  // (here: whether the grouped solver's bookkeeping is needed; the launcher sets it per launch)
    if (deblur) {  // no size classes: every running slot takes solve_big<1> on one workgroup
        r->rc.solve_group = 1;
        for (int b = 0; b < n_scans; b++)  // scan_is_compact (ll_reg_query.h) on the host's counts, through the definitions the kernel reads
            if (!r->h_state[b].done && (r->rc.force_general || padded_block_count(r->h_nc[b], r->h_ns[b]) > LL_TABLE_MAX_BLOCKS))
                return set_err(where, "a scan of this batch is beyond the compact solver's size (or the general solver was forced): not supported with a map "
                                      "per slot, register such scans through the single-map entry points");
        for (int it = 0; n_run && it < prm->icp_max_iterations; it++) {
            r->rc.xch_epoch = it + 1;
            prof_begin(r, 0);
            launch_reg_knn_build_maps(r->dev, r->rc, r->d_map_tab, n_scans, it, max_nc, max_ns, r->stream, r->d_ts);
            prof_end(r);
            prof_begin(r, 1);
            launch_reg_solve_big_maps(r->dev, r->rc, r->d_map_tab, r->d_ts, n_scans, r->stream);
            prof_end(r);
        }
    } else if (n_run) {
        if ((cls.n[2] && !reg_solve_fast_eligible(r->rc, cls.max_nc[2], cls.max_ns[2])) || (cls.n[3] && !reg_solve_fast_eligible(r->rc, cls.max_nc[3], cls.max_ns[3])))
            return set_err(where, "a scan of this batch is beyond the compact solver's size (or the general solver was forced): not supported with a map "
                                  "per slot, register such scans through the single-map entry points");
        if (r->rc.solve_group > 1)
            HC(hipMemsetAsync(r->dev.grp_xch, 0, (size_t)n_scans * 2 * LL_GRP * 56 * sizeof(unsigned long long), r->stream));
        for (int it = 0; it < prm->icp_max_iterations; it++) {
            r->rc.xch_epoch = it + 1;
            prof_begin(r, 0);
            launch_reg_knn_build_maps(r->dev, r->rc, r->d_map_tab, n_scans, it, max_nc, max_ns, r->stream);
            prof_end(r);
            prof_begin(r, 1);
            if (r->rc.solve_group > 1) HC(hipMemsetAsync(r->dev.grp_ctl, 0, (size_t)(2 * n_scans + 1) * sizeof(int), r->stream));
            launch_reg_solve_maps(r->dev, r->rc, r->d_map_tab, n_scans, cls, it, r->stream);
            prof_end(r);
        }
    }
    const Grid none{};
    return reg_finish(r, n_scans, pin_guard, none, none, r->d_map_tab, deblur ? r->d_ts : nullptr);
}

extern "C" int ll_reg_enqueue_fe_maps(ll_reg *r, const ll_map *const *maps, ll_fe *fe, int32_t n_scans, const ll_reg_params *prm,
                                      const int32_t *frame_index, const double *poses_last, const double *poses_curr, const double *poses_incre)
{
    static const char *where = "ll_reg_enqueue_fe_maps";
    const int ts_n = r ? reg_take_time_ranges(r) : 0;
    if (!r || !fe) return set_err(where, "null handle");
    if (reg_maps_check(where, r, maps, n_scans, prm, poses_last, poses_curr, ts_n)) return -1;
    if (fe->prm.device != r->device) return set_err(where, "extractor lives on another device");
    if (reg_fe_fits(where, r, fe, n_scans)) return -1;
    HC(hipSetDevice(r->device));
    if (reg_bind(r, feat_view(fe))) return -1;
    return reg_enqueue_maps(where, r, maps, n_scans, prm, frame_index, poses_last, poses_curr, poses_incre);
}

// ---- voxel filters in front of the registrar ---------------------------------------------------------------------------------------
// what every downsampled form asks of its pair of filters (their capacities: each form's own checks, they differ)
static int reg_voxel_check(const char *where, const ll_reg *r, const ll_voxel *vc, const ll_voxel *vs)
{
    if (vc->device != r->device || vs->device != r->device) return set_err(where, "handles live on different devices");
    if (vc == vs) return set_err(where, "corner and surface need their own voxel filter handle");
    return 0;
}

// producer -> (voxel filters, on the registrar's stream) -> registrar: *out is what the registrar binds
static int reg_downsample(const char *where, ll_reg *r, const FeatView &in, ll_voxel *vc, ll_voxel *vs, float line_res, float plane_res, int n_scans,
                          FeatView *out)
{
    if (reg_wait(r, in)) return -1;
    const char *err = nullptr;
    const float lc[3] = {line_res, line_res, line_res}, ls[3] = {plane_res, plane_res, plane_res};
    if (voxel_filter(vc->dev, in.corner, in.n_corner, in.stride_c, n_scans, lc, r->stream, &err)) return set_err(where, err);
    if (voxel_filter(vs->dev, in.surf, in.n_surf, in.stride_s, n_scans, ls, r->stream, &err)) return set_err(where, err);
    vc->last_stream = vs->last_stream = r->stream;
    *out = feat_view(vc, vs);
    return 0;
}

// One scan whose corner and surface cloud lie on the device, written on the registrar's own stream, with their sizes on the device
// (where the kernels read them) AND on the host (n_corner, n_surf: the caller has read them back already), so the enqueue does not wait
// for them (ll_api_scene_align.hip).  Collect with ll_reg_collect.
int ll::reg_enqueue_device_clouds(const char *where, ll_reg *r, const ll_map *map, const float4 *d_corner, const int *d_n_corner, int n_corner,
                                  const float4 *d_surf, const int *d_n_surf, int n_surf, const ll_reg_params *prm, const double pose_last[7],
                                  const double pose_curr[7], const double pose_incre[7])
{
    if (reg_refuse_pending_ranges(where, r)) return -1;
    HC(hipSetDevice(r->device));
    const FeatView v{d_corner, d_surf, d_n_corner, d_n_surf, n_corner > 0 ? n_corner : 1, n_surf > 0 ? n_surf : 1, {nullptr, nullptr}};
    if (reg_bind(r, v)) return -1;
    const int known[2] = {n_corner, n_surf};
    return reg_enqueue(where, r, map, 1, prm, pose_last, pose_curr, pose_incre, known);
}

extern "C" int ll_reg_enqueue_fe_downsampled(ll_reg *r, const ll_map *map, ll_fe *fe, ll_voxel *vc, ll_voxel *vs, float line_res,
                                             float plane_res, int32_t n_scans, const ll_reg_params *prm, const double *poses_last,
                                             const double *poses_curr, const double *poses_incre)
{
    static const char *where = "ll_reg_enqueue_fe_downsampled";
    if (reg_refuse_pending_ranges(where, r)) return -1;
    if (!r || !fe || !vc || !vs) return set_err(where, "null handle");
    if (fe->prm.device != r->device) return set_err(where, "handles live on different devices");
    if (reg_voxel_check(where, r, vc, vs)) return -1;
    if (n_scans < 1) return set_err(where, "n_scans exceeds the extractor capacity");
    if (reg_fe_fits(where, r, fe, n_scans)) return -1;
    HC(hipSetDevice(r->device));
    FeatView v;
    if (reg_downsample(where, r, feat_view(fe), vc, vs, line_res, plane_res, n_scans, &v) || reg_bind(r, v)) return -1;
    return reg_enqueue(where, r, map, n_scans, prm, poses_last, poses_curr, poses_incre);
}

extern "C" int ll_reg_enqueue_fe_downsampled_maps(ll_reg *r, const ll_map *const *maps, ll_fe *fe, ll_voxel *vc, ll_voxel *vs, float line_res,
                                                  float plane_res, int32_t n_scans, const ll_reg_params *prm, const int32_t *frame_index,
                                                  const double *poses_last, const double *poses_curr, const double *poses_incre)
{
    static const char *where = "ll_reg_enqueue_fe_downsampled_maps";
    const int ts_n = r ? reg_take_time_ranges(r) : 0;
    if (!r || !fe || !vc || !vs) return set_err(where, "null handle");
    if (reg_maps_check(where, r, maps, n_scans, prm, poses_last, poses_curr, ts_n)) return -1;
    if (fe->prm.device != r->device) return set_err(where, "handles live on different devices");
    if (reg_voxel_check(where, r, vc, vs)) return -1;
    if (n_scans > vc->dev.max_clouds || n_scans > vs->dev.max_clouds) return set_err(where, "n_scans exceeds the voxel filters' max_clouds");
    if (reg_fe_fits(where, r, fe, n_scans)) return -1;
    HC(hipSetDevice(r->device));
    FeatView v;
    if (reg_downsample(where, r, feat_view(fe), vc, vs, line_res, plane_res, n_scans, &v) || reg_bind(r, v)) return -1;
    return reg_enqueue_maps(where, r, maps, n_scans, prm, frame_index, poses_last, poses_curr, poses_incre);
}

extern "C" int ll_reg_solve_batch_fe(ll_reg *r, const ll_map *map, ll_fe *fe, int32_t n_scans, const ll_reg_params *prm,
                                     const double *poses_last, double *poses_curr, double *poses_incre, ll_reg_report *reports,
                                     int32_t *results)
{
    if (ll_reg_enqueue_fe(r, map, fe, n_scans, prm, poses_last, poses_curr, poses_incre)) return -1;
    return ll_reg_collect(r, n_scans, poses_curr, poses_incre, reports, results);
}

extern "C" int ll_reg_upload_features(ll_reg *r, int32_t n_scans, const float *corner_xyzi, const int32_t *n_corner, int32_t stride_corner,
                                      const float *surf_xyzi, const int32_t *n_surf, int32_t stride_surf)
{
    if (!r || !n_corner || !n_surf) return set_err("ll_reg_upload_features", "null argument");
    if (n_scans < 1 || n_scans > r->max_scans) return set_err("ll_reg_upload_features", "n_scans out of range");
    if (stride_corner < 0 || stride_surf < 0) return set_err("ll_reg_upload_features", "negative stride");
    for (int b = 0; b < n_scans; b++) {  // validate everything before the first copy: a caller mistake must not become a host over-read
        if (n_corner[b] < 0 || n_corner[b] > r->max_feat || n_surf[b] < 0 || n_surf[b] > r->max_feat)
            return set_err("ll_reg_upload_features", "feature count exceeds capacity");
        if ((n_corner[b] > 0 && !corner_xyzi) || (n_surf[b] > 0 && !surf_xyzi))
            return set_err("ll_reg_upload_features", "null feature array with a non-zero count");
        if (n_scans > 1 && (n_corner[b] > stride_corner || n_surf[b] > stride_surf))
            return set_err("ll_reg_upload_features", "feature count exceeds the per-scan stride");
    }
    HC(hipSetDevice(r->device));
    const size_t F = r->max_feat;
    for (int b = 0; b < n_scans; b++) {
        if (n_corner[b] > 0)
            HC(hipMemcpyAsync(r->d_corner + b * F, corner_xyzi + (size_t)b * stride_corner * 4, (size_t)n_corner[b] * sizeof(float4),
                              hipMemcpyHostToDevice, r->stream));
        if (n_surf[b] > 0)
            HC(hipMemcpyAsync(r->d_surf + b * F, surf_xyzi + (size_t)b * stride_surf * 4, (size_t)n_surf[b] * sizeof(float4),
                              hipMemcpyHostToDevice, r->stream));
    }
    HC(hipMemcpyAsync(r->d_nc, n_corner, n_scans * sizeof(int), hipMemcpyHostToDevice, r->stream));
    HC(hipMemcpyAsync(r->d_ns, n_surf, n_scans * sizeof(int), hipMemcpyHostToDevice, r->stream));
    HC(hipStreamSynchronize(r->stream));
    r->uploaded_scans = n_scans;
    return 0;
}

extern "C" int ll_reg_enqueue_fe_merged(ll_reg *r, const ll_map *map, ll_fe *fe, int32_t n_scans, int32_t heads, const ll_reg_params *prm,
                                        const double *poses_last, const double *poses_curr, const double *poses_incre)
{
    static const char *where = "ll_reg_enqueue_fe_merged";
    if (reg_refuse_pending_ranges(where, r)) return -1;
    if (!r || !fe) return set_err(where, "null handle");
    if (fe->prm.device != r->device) return set_err(where, "extractor lives on another device");
    if (heads < 1 || n_scans < 1 || n_scans > r->max_scans || (int64_t)n_scans * heads > fe->prm.max_scans)
        return set_err(where, "n_scans * heads exceeds the extractor capacity (or n_scans the registrar's)");
    HC(hipSetDevice(r->device));
    const FeatView in = feat_view(fe);
    if (reg_wait(r, in)) return -1;
    launch_reg_merge_heads(in.corner, in.surf, in.n_corner, in.n_surf, in.stride_c, heads, r->d_corner, r->d_surf, r->d_nc, r->d_ns, r->max_feat,
                           n_scans, r->stream);
    HC(hipGetLastError());
    r->uploaded_scans = n_scans;
    if (reg_bind(r, feat_view(r))) return -1;
    // a merged cloud larger than the registrar's capacity shows in the counts: reg_enqueue refuses it
    return reg_enqueue(where, r, map, n_scans, prm, poses_last, poses_curr, poses_incre);
}

extern "C" int ll_reg_enqueue_uploaded(ll_reg *r, const ll_map *map, int32_t n_scans, const ll_reg_params *prm, const double *poses_last,
                                       const double *poses_curr, const double *poses_incre)
{
    static const char *where = "ll_reg_enqueue_uploaded";
    if (reg_refuse_pending_ranges(where, r)) return -1;
    if (!r) return set_err(where, "null handle");
    if (n_scans < 1 || n_scans > r->uploaded_scans) return set_err(where, "no features uploaded for that many scans");
    HC(hipSetDevice(r->device));
    if (reg_bind(r, feat_view(r))) return -1;
    return reg_enqueue(where, r, map, n_scans, prm, poses_last, poses_curr, poses_incre);
}

extern "C" int ll_reg_solve_batch(ll_reg *r, const ll_map *map, int32_t n_scans, const float *corner_xyzi, const int32_t *n_corner,
                                  int32_t stride_corner, const float *surf_xyzi, const int32_t *n_surf, int32_t stride_surf,
                                  const ll_reg_params *prm, const double *poses_last, double *poses_curr, double *poses_incre,
                                  ll_reg_report *reports, int32_t *results)
{
    if (reg_refuse_pending_ranges("ll_reg_solve_batch", r)) return -1;  // (before the upload: the enqueue behind it would refuse anyway)
    if (ll_reg_upload_features(r, n_scans, corner_xyzi, n_corner, stride_corner, surf_xyzi, n_surf, stride_surf)) return -1;
    if (ll_reg_enqueue_uploaded(r, map, n_scans, prm, poses_last, poses_curr, poses_incre)) return -1;
    return ll_reg_collect(r, n_scans, poses_curr, poses_incre, reports, results);
}

extern "C" int ll_reg_solve(ll_reg *r, const ll_map *map, const float *scan_corner_xyzi, int32_t n_corner,
                            const float *scan_surf_xyzi, int32_t n_surf, const ll_reg_params *prm, const double pose_last[7],
                            double pose_curr[7], double pose_incre[7], ll_reg_report *rep)
{
    int32_t res = 1;
    double inc_local[7] = {0, 0, 0, 1, 0, 0, 0};
    double *inc = pose_incre ? pose_incre : inc_local;
    const int rc = ll_reg_solve_batch(r, map, 1, scan_corner_xyzi, &n_corner, n_corner, scan_surf_xyzi, &n_surf, n_surf, prm,
                                      pose_last, pose_curr, inc, rep, &res);
    if (rc < 0) return rc;
    return res;
}

extern "C" int ll_reg_debug_knn(ll_reg *r, int32_t scan, int32_t *corner_idx5, float *corner_d25, int32_t *surf_idx5, float *surf_d25)
{
    if (!r) return set_err("ll_reg_debug_knn", "null handle");
    if (!r->dev.dbg_idx) return set_err("ll_reg_debug_knn", "debug taps not enabled (ll_reg_set_debug)");
    if (scan < 0 || scan >= r->max_scans) return set_err("ll_reg_debug_knn", "scan out of range");
    HC(hipSetDevice(r->device));
    HC(hipStreamSynchronize(r->stream));
    int nc = 0, ns = 0;
    HC(hipMemcpy(&nc, r->dev.n_corner + scan, sizeof(int), hipMemcpyDeviceToHost));
    HC(hipMemcpy(&ns, r->dev.n_surf + scan, sizeof(int), hipMemcpyDeviceToHost));
    const size_t base = (size_t)scan * r->dev.cap * 5;
    D2H_OPT(corner_idx5, r->dev.dbg_idx + base, (size_t)nc * 5, int);
    D2H_OPT(corner_d25, r->dev.dbg_d2 + base, (size_t)nc * 5, float);
    D2H_OPT(surf_idx5, r->dev.dbg_idx + base + (size_t)r->dev.cap_c * 5, (size_t)ns * 5, int);
    D2H_OPT(surf_d25, r->dev.dbg_d2 + base + (size_t)r->dev.cap_c * 5, (size_t)ns * 5, float);
    return 0;
}

extern "C" int ll_reg_debug_blocks(ll_reg *r, int32_t scan, int32_t *corner_nn4, uint8_t *corner_flag, int32_t *surf_nn4, uint8_t *surf_flag)
{
    if (!r) return set_err("ll_reg_debug_blocks", "null handle");
    if (scan < 0 || scan >= r->max_scans) return set_err("ll_reg_debug_blocks", "scan out of range");
    HC(hipSetDevice(r->device));
    HC(hipStreamSynchronize(r->stream));
    int nc = 0, ns = 0;
    HC(hipMemcpy(&nc, r->dev.n_corner + scan, sizeof(int), hipMemcpyDeviceToHost));
    HC(hipMemcpy(&ns, r->dev.n_surf + scan, sizeof(int), hipMemcpyDeviceToHost));
    const size_t base = (size_t)scan * r->dev.cap;
    D2H_OPT(corner_nn4, reinterpret_cast<const int *>(r->dev.nn + base), (size_t)nc * 4, int);
    D2H_OPT(corner_flag, r->dev.blk_flag0 + base, (size_t)nc, unsigned char);
    D2H_OPT(surf_nn4, reinterpret_cast<const int *>(r->dev.nn + base + r->dev.cap_c), (size_t)ns * 4, int);
    D2H_OPT(surf_flag, r->dev.blk_flag0 + base + r->dev.cap_c, (size_t)ns, unsigned char);
    return 0;
}

// The clouds of the accepted scans (src is [n_scans][stride] on the device, counts[] on the host, the producer waited for), each through its
// pose, appended to dev_out_xyzi from *n_points on
static int cloud_transform_accepted(const char *where, ll_reg *r, const float4 *src, int stride, const int *counts, int n_scans, const int32_t *accept,
                                    const double *poses7, float *dev_out_xyzi, int64_t capacity_points, int64_t *n_points)
{
    int64_t total = *n_points;
    for (int b = 0; b < n_scans; b++)
        if (accept[b]) total += counts[b];
    if (total > capacity_points) return set_err(where, "device buffer too small");
    double *d_poses = nullptr;
    DM(d_poses, (size_t)n_scans * 7);
    hipError_t e = hipMemcpyAsync(d_poses, poses7, (size_t)n_scans * 7 * sizeof(double), hipMemcpyHostToDevice, r->stream);
    int64_t at = *n_points;
    for (int b = 0; b < n_scans && e == hipSuccess; b++) {
        if (!accept[b] || counts[b] == 0) continue;
        launch_cloud_transform(src + (size_t)b * stride, (float4 *)dev_out_xyzi + at, counts[b], d_poses + (size_t)b * 7, r->stream);
        at += counts[b];
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    (void)hipFree(d_poses);
    if (e != hipSuccess) return set_err(where, hipGetErrorString(e));
    *n_points = total;
    return 0;
}

extern "C" int ll_cloud_transform_fe_device(ll_reg *r, ll_fe *fe, int32_t n_scans, int32_t kind, const int32_t *accept, const double *poses7,
                                            float *dev_out_xyzi, int64_t capacity_points, int64_t *n_points)
{
    static const char *where = "ll_cloud_transform_fe_device";
    if (!r || !fe || !accept || !poses7 || !dev_out_xyzi || !n_points) return set_err(where, "null argument");
    if (fe->prm.device != r->device) return set_err(where, "extractor lives on another device");
    if (n_scans < 0 || n_scans > fe->prm.max_scans || kind < 0 || kind > 1 || *n_points < 0) return set_err(where, "bad argument");
    if (n_scans == 0) return 0;
    HC(hipSetDevice(r->device));
    HC(hipStreamSynchronize(fe->stream));
    std::vector<int> cnt((size_t)n_scans);
    HC(hipMemcpy(cnt.data(), kind == 0 ? fe->dev.n_corner : fe->dev.n_surf, (size_t)n_scans * sizeof(int), hipMemcpyDeviceToHost));
    return cloud_transform_accepted(where, r, kind == 0 ? fe->dev.corner_feat : fe->dev.surf_feat, fe->dev.stride, cnt.data(), n_scans, accept, poses7,
                                    dev_out_xyzi, capacity_points, n_points);
}

// ---------------------------------------------------------------------------------------------------- spinning-lidar hand-off
// The registrar's inputs out of a spin handle (ll_spin_api.hip), device to device: corner stack = LL_SPIN_LESS_SHARP (packed by
// spin_pack_kernel), surface stack = LL_SPIN_LESS_FLAT.  The forms mirror the _fe ones above.
static const char *kSpinDeblur =
    "if_motion_deblur must be 0: the spinning extractor writes intensity = scanID + scanPeriod * relTime "
    "(laser_feature_extractor.hpp:502), which refine_blur (point_cloud_registration.hpp:128-141) would misread as a time stamp";

// the argument checks ll_reg_enqueue_spin and ll_reg_enqueue_spin_downsampled share (nothing is launched before they all pass)
static int reg_spin_check(const char *where, ll_reg *r, ll_spin *sp, int n_scans, const ll_reg_params *prm, SpinView *v)
{
    if (!r || !sp) return set_err(where, "null handle");
    if (!prm) return set_err(where, "null argument");
    spin_view(sp, v);
    if (v->device != r->device) return set_err(where, "extractor lives on another device");
    if (n_scans < 1) return set_err(where, "n_scans must be at least 1");
    if (n_scans > v->max_scans) return set_err(where, "n_scans exceeds the extractor capacity");
    if (n_scans > r->max_scans) return set_err(where, "n_scans exceeds the registrar capacity");
    if (v->max_points > r->max_feat) return set_err(where, "registrar feature capacity < extractor max_points");
    if (prm->if_motion_deblur != 0) return set_err(where, kSpinDeblur);
    return 0;
}

extern "C" int ll_reg_enqueue_spin(ll_reg *r, const ll_map *map, ll_spin *sp, int32_t n_scans, const ll_reg_params *prm,
                                   const double *poses_last, const double *poses_curr, const double *poses_incre)
{
    static const char *where = "ll_reg_enqueue_spin";
    if (reg_refuse_pending_ranges(where, r)) return -1;
    SpinView v;
    if (reg_spin_check(where, r, sp, n_scans, prm, &v)) return -1;
    if (spin_handoff(sp, n_scans, &v)) return -1;
    HC(hipSetDevice(r->device));
    if (reg_bind(r, feat_view(v))) return -1;  // order after the extractor's stream (the extraction and the pack kernel behind it)
    return reg_enqueue(where, r, map, n_scans, prm, poses_last, poses_curr, poses_incre);
}

extern "C" int ll_reg_enqueue_spin_downsampled(ll_reg *r, const ll_map *map, ll_spin *sp, ll_voxel *vc, ll_voxel *vs, float line_res,
                                               float plane_res, int32_t n_scans, const ll_reg_params *prm, const double *poses_last,
                                               const double *poses_curr, const double *poses_incre)
{
    static const char *where = "ll_reg_enqueue_spin_downsampled";
    if (reg_refuse_pending_ranges(where, r)) return -1;
    if (!vc || !vs) return set_err(where, "null handle");
    SpinView v;
    if (reg_spin_check(where, r, sp, n_scans, prm, &v)) return -1;
    if (reg_voxel_check(where, r, vc, vs)) return -1;
    if (n_scans > vc->dev.max_clouds || n_scans > vs->dev.max_clouds || v.pack_stride > vc->dev.stride || v.max_points > vs->dev.stride)
        return set_err(where, "voxel filter capacity too small: the corner filter needs n_scans clouds of min(max_points, 1200 * scan_line) "
                              "points, the surface filter n_scans clouds of max_points points");
    if (spin_handoff(sp, n_scans, &v)) return -1;
    HC(hipSetDevice(r->device));
    FeatView f;  // extractor (+ pack) -> voxel filters -> registrar
    if (reg_downsample(where, r, feat_view(v), vc, vs, line_res, plane_res, n_scans, &f) || reg_bind(r, f)) return -1;
    return reg_enqueue(where, r, map, n_scans, prm, poses_last, poses_curr, poses_incre);
}

extern "C" int ll_cloud_transform_spin_device(ll_reg *r, ll_spin *sp, int32_t n_scans, int32_t which, const int32_t *accept,
                                              const double *poses7, float *dev_out_xyzi, int64_t capacity_points, int64_t *n_points)
{
    static const char *where = "ll_cloud_transform_spin_device";
    if (!r || !sp || !accept || !poses7 || !dev_out_xyzi || !n_points) return set_err(where, "null argument");
    SpinView v;
    spin_view(sp, &v);
    if (v.device != r->device) return set_err(where, "extractor lives on another device");
    if (which == LL_SPIN_LESS_FLAT_PRE) return set_err(where, "LL_SPIN_LESS_FLAT_PRE is a list of positions, not a cloud the reference publishes");
    if (which < LL_SPIN_FULL || which > LL_SPIN_LESS_FLAT) return set_err(where, "unknown cloud");
    if (n_scans < 0 || n_scans > v.max_scans) return set_err(where, "n_scans exceeds the extractor capacity");
    if (*n_points < 0) return set_err(where, "bad argument");
    if (n_scans == 0) return 0;
    const float4 *src = nullptr;
    int stride = 0;
    std::vector<int> cnt((size_t)n_scans);
    if (spin_device_cloud(sp, n_scans, which, &src, &stride, cnt.data())) return -1;  // (synchronises the extractor's stream)
    HC(hipSetDevice(r->device));
    return cloud_transform_accepted(where, r, src, stride, cnt.data(), n_scans, accept, poses7, dev_out_xyzi, capacity_points, n_points);
}

extern "C" int ll_cloud_transform(ll_reg *r, const float *in_xyzi, float *out_xyzi, int32_t n, const double pose[7])
{
    if (!r || !pose || (n > 0 && (!in_xyzi || !out_xyzi))) return set_err("ll_cloud_transform", "null argument");
    if (n <= 0) return 0;
    HC(hipSetDevice(r->device));
    float4 *d_in = nullptr, *d_out = nullptr;
    DM(d_in, (size_t)n);
    DM(d_out, (size_t)n);
    HC(hipMemcpyAsync(d_in, in_xyzi, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, r->stream));
    HC(hipMemcpyAsync(r->d_pose_tmp, pose, 7 * sizeof(double), hipMemcpyHostToDevice, r->stream));
    launch_cloud_transform(d_in, d_out, n, r->d_pose_tmp, r->stream);
    HC(hipGetLastError());
    HC(hipMemcpyAsync(out_xyzi, d_out, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, r->stream));
    HC(hipStreamSynchronize(r->stream));
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return 0;
}

// ---------------------------------------------------------------------------------------------------- deskewed clouds
// pointAssociateToMap / pointcloudAssociateToMap with if_undistore = 1 (point_cloud_registration.hpp:622-661, 673-685) after the
// registration has been collected.  The solver states are the next enqueue's to overwrite, so the first call after a collect copies
// what the formula needs into records of this handle (undistort_snapshot_kernel, on the registrar's stream: ordered behind the
// registration and ahead of the next upload); every later call until the next enqueue reuses them.
int ll::reg_undistort_records(const char *where, ll_reg *r, int n_slots)
{
    if (!r->collected_scans) return set_err(where, "no registration has been collected since the last enqueue (call ll_reg_collect first)");
    if (n_slots < 1 || n_slots > r->last_n_scans) return set_err(where, "slot beyond the last registration's n_scans");
    HC(hipSetDevice(r->device));
    if (!r->d_und) {
        DM(r->d_und, (size_t)r->max_scans);
        DM(r->d_und_jobs, (size_t)r->max_scans);
    }
    if (!r->und_valid) {
        launch_undistort_snapshot(r->dev.state, 0, r->last_n_scans, r->rc, r->d_und, r->stream, r->ts_last ? r->d_ts : nullptr);
        HC(hipGetLastError());
        r->und_valid = 1;
    }
    return 0;
}

extern "C" int ll_reg_interpolation(ll_reg *r, int32_t n_scans, double *theta, double *omega_hat9, double *pose_last7, double *pose_incre7)
{
    static const char *where = "ll_reg_interpolation";
    if (!r) return set_err(where, "null handle");
    if (!r->collected_scans) return set_err(where, "no registration has been collected since the last enqueue (call ll_reg_collect first)");
    if (n_scans < 1 || n_scans > r->collected_scans) return set_err(where, "n_scans beyond the last collected registration's");
    for (int b = 0; b < n_scans; b++) {
        const RegState &s = r->h_state[b];
        const bool gated = s.gated != 0;  // no increment was estimated (PCR:199): identity
        if (theta) theta[b] = gated ? 0.0 : s.interp_theta;
        for (int i = 0; i < 9 && omega_hat9; i++) omega_hat9[9 * b + i] = gated ? 0.0 : s.hat[i];
        for (int i = 0; i < 7 && pose_last7; i++) pose_last7[7 * b + i] = s.pose_last[i];
        for (int i = 0; i < 7 && pose_incre7; i++) pose_incre7[7 * b + i] = gated ? (i == 3 ? 1.0 : 0.0) : s.inc[i];
    }
    return 0;
}

extern "C" int ll_cloud_undistort(ll_reg *r, int32_t slot, const float *in_xyzi, float *out_xyzi, int32_t n)
{
    static const char *where = "ll_cloud_undistort";
    if (!r || (n > 0 && (!in_xyzi || !out_xyzi))) return set_err(where, "null argument");
    if (slot < 0) return set_err(where, "negative slot");
    if (reg_undistort_records(where, r, slot + 1)) return -1;
    if (n <= 0) return 0;
    float4 *d_in = nullptr, *d_out = nullptr;
    DM(d_in, (size_t)n);
    DM(d_out, (size_t)n);
    hipError_t e = hipMemcpyAsync(d_in, in_xyzi, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess) {
        const UndistortJob one{slot, n, 0, 0};
        launch_cloud_undistort(r->d_und, nullptr, one, 1, n, d_in, nullptr, nullptr, d_out, r->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_xyzi, d_out, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (e != hipSuccess) return set_err(where, hipGetErrorString(e));
    return 0;
}

extern "C" int ll_cloud_undistort_fe_device(ll_reg *r, ll_fe *fe, int32_t n_scans, int32_t kind, const int32_t *accept, float *dev_out_xyzi,
                                            int64_t capacity_points, int64_t *n_points)
{
    static const char *where = "ll_cloud_undistort_fe_device";
    if (!r || !fe || !accept || !dev_out_xyzi || !n_points) return set_err(where, "null argument");
    if (fe->prm.device != r->device) return set_err(where, "extractor lives on another device");
    if (n_scans < 0 || n_scans > fe->prm.max_scans || kind < 0 || kind > 2 || *n_points < 0) return set_err(where, "bad argument");
    if (n_scans == 0) return 0;
    if (kind == 2 && !fe->dev.full_idx) return set_err(where, "the extractor keeps no full selection");
    if (reg_undistort_records(where, r, n_scans)) return -1;
    HC(hipStreamSynchronize(fe->stream));
    std::vector<int> cnt((size_t)n_scans);
    HC(hipMemcpy(cnt.data(), kind == 0 ? fe->dev.n_corner : kind == 1 ? fe->dev.n_surf : fe->dev.n_full, (size_t)n_scans * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<UndistortJob> jobs;
    int64_t at = *n_points;
    int max_n = 0;
    for (int b = 0; b < n_scans; b++) {
        if (!accept[b] || cnt[b] <= 0) continue;
        if (cnt[b] > fe->dev.stride) return set_err(where, "selection count exceeds the extractor stride");
        jobs.push_back(UndistortJob{b, cnt[b], (long long)b * fe->dev.stride, (long long)at});
        at += cnt[b];
        max_n = cnt[b] > max_n ? cnt[b] : max_n;
    }
    if (at > capacity_points) return set_err(where, "device buffer too small");
    if (!jobs.empty()) {
        HC(hipMemcpyAsync(r->d_und_jobs, jobs.data(), jobs.size() * sizeof(UndistortJob), hipMemcpyHostToDevice, r->stream));
        const UndistortJob none{0, 0, 0, 0};
        if (kind == 2)
            launch_cloud_undistort(r->d_und, r->d_und_jobs, none, (int)jobs.size(), max_n, fe->dev.xyzi, fe->dev.full_idx, fe->dev.tstamp, (float4 *)dev_out_xyzi, r->stream);
        else
            launch_cloud_undistort(r->d_und, r->d_und_jobs, none, (int)jobs.size(), max_n, kind == 0 ? fe->dev.corner_feat : fe->dev.surf_feat, nullptr, nullptr,
                                   (float4 *)dev_out_xyzi, r->stream);
        HC(hipGetLastError());
        HC(hipStreamSynchronize(r->stream));  // (the job table is host memory of this call; the caller reads the buffer on a stream of its own)
    }
    *n_points = at;
    return 0;
}
