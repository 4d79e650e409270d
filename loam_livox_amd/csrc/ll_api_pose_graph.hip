// ll_api_pose_graph.hip -- the pose-graph optimiser of the C ABI (ll_pose_graph_*): G independent graphs in, one copy to the device,
// one launch (ll_pose_graph_kernels.hip: a workgroup per graph, the whole minimisation inside), one copy back, one host wait.  The
// call is checked and planned on the host (ll_pose_graph.h: incidence lists, block envelope, information factors) before anything is
// enqueued.
#include "ll_api_internal.h"
#include "ll_pose_graph.h"

struct ll_pose_graph {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t max_graphs = 0, max_poses = 0, max_edges = 0, max_blocks = 0;
    // what a call sends and brings back, in one piece: page-locked on the host, mirrored on the device (PgArena below)
    char *hp_io = nullptr, *d_io = nullptr;
    size_t io_bytes = 0;
    double *d_work = nullptr;  // cand, r, J, ecost, scale, diag, g, rhs, y, ps0, ps1
    double *d_H = nullptr;     // 36 * max_blocks
    int64_t work[4] = {0, 0, 0, 0};
};

namespace {

// where the pieces of a call lie in the exchange buffer: poses and summaries first (they come back), then the inputs
struct PgArena {
    size_t x, summary, meas, info_l, strip, graphs, edge_ab, has_l, inc_start, inc, first, end;
    PgArena(int64_t G, int64_t P, int64_t E)
    {
        size_t at = 0;
        auto take = [&](size_t bytes) {
            const size_t here = at;
            at += (bytes + 7) & ~(size_t)7;
            return here;
        };
        x = take(7 * P * sizeof(double));
        summary = take(G * sizeof(ll_pose_graph_summary));
        meas = take(7 * E * sizeof(double));
        info_l = take(36 * E * sizeof(double));
        strip = take(P * sizeof(int64_t));
        graphs = take(G * sizeof(PgGraph));
        edge_ab = take(2 * E * sizeof(int32_t));
        has_l = take(E * sizeof(int32_t));
        inc_start = take((P + 1) * sizeof(int32_t));
        inc = take(2 * E * sizeof(int32_t));
        first = take(P * sizeof(int32_t));
        end = at;
    }
};

size_t work_doubles(int64_t P, int64_t E) { return (size_t)(7 * P + 6 * E + 72 * E + E + 5 * 6 * P + 2 * P); }

const int64_t kMaxGraphs = 1 << 20;
const int64_t kMaxBlocks = (int64_t)1 << 32;  // 36 doubles each

}  // namespace

extern "C" void ll_pose_graph_default_params(ll_pose_graph_params *p)
{
    if (!p) return;
    p->max_num_iterations = 200;
    p->max_num_consecutive_invalid_steps = 5;
    p->initial_trust_region_radius = 1e4;
    p->max_trust_region_radius = 1e16;
    p->min_trust_region_radius = 1e-32;
    p->min_relative_decrease = 1e-3;
    p->min_lm_diagonal = 1e-6;
    p->max_lm_diagonal = 1e32;
    p->function_tolerance = 1e-6;
    p->gradient_tolerance = 1e-10;
    p->parameter_tolerance = 1e-8;
}

extern "C" void ll_pose_graph_destroy(ll_pose_graph *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->d_io) (void)hipFree(h->d_io);
    if (h->d_work) (void)hipFree(h->d_work);
    if (h->d_H) (void)hipFree(h->d_H);
    if (h->hp_io) (void)hipHostFree(h->hp_io);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

extern "C" int ll_pose_graph_create(int32_t device, int64_t max_graphs, int64_t max_poses_total, int64_t max_edges_total, int64_t max_envelope_blocks,
                                    ll_pose_graph **out)
{
    const char *fn = "ll_pose_graph_create";
    if (!out) return set_err(fn, "null argument");
    if (max_graphs < 1 || max_graphs > kMaxGraphs) return set_err(fn, "max_graphs out of range");
    if (max_poses_total < 1 || max_poses_total > kPgMaxCount) return set_err(fn, "max_poses_total out of range");
    if (max_edges_total < 1 || max_edges_total > kPgMaxCount) return set_err(fn, "max_edges_total out of range");
    if (max_envelope_blocks < 1 || max_envelope_blocks > kMaxBlocks) return set_err(fn, "max_envelope_blocks out of range");
    if (check_device(device)) return -1;
    ll_pose_graph *h = new ll_pose_graph();
    h->device = device;
    h->max_graphs = max_graphs, h->max_poses = max_poses_total, h->max_edges = max_edges_total, h->max_blocks = max_envelope_blocks;
    h->io_bytes = PgArena(max_graphs, max_poses_total, max_edges_total).end;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&h->d_io, h->io_bytes) != hipSuccess ||
        hipHostMalloc((void **)&h->hp_io, h->io_bytes, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void **)&h->d_work, work_doubles(max_poses_total, max_edges_total) * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&h->d_H, (size_t)max_envelope_blocks * 36 * sizeof(double)) != hipSuccess) {
        ll_pose_graph_destroy(h);
        return set_err(fn, "allocation failed");
    }
    *out = h;
    return 0;
}

extern "C" int ll_pose_graph_solve(ll_pose_graph *h, const ll_pose_graph_params *p, int64_t n_graphs, const int64_t *pose_offsets, double *poses7,
                                   const int64_t *edge_offsets, const int32_t *edge_ab, const double *edge_meas7, const double *edge_information,
                                   ll_pose_graph_summary *summary)
{
    const char *fn = "ll_pose_graph_solve";
    if (!h) return set_err(fn, "null argument");
    if (n_graphs > 0 && !summary) return set_err(fn, "null argument");
    ll_pose_graph_params prm;
    ll_pose_graph_default_params(&prm);
    if (p) prm = *p;
    if (prm.max_num_iterations < 0 || prm.max_num_consecutive_invalid_steps < 1 || !(prm.initial_trust_region_radius > 0.0))
        return set_err(fn, "parameters out of range");
    PgPlan plan;
    const std::string why = pg_plan(n_graphs, pose_offsets, poses7, edge_offsets, edge_ab, edge_meas7, edge_information, &plan);
    if (!why.empty()) return set_err(fn, why.c_str());
    const int64_t G = n_graphs, P = plan.n_poses, E = plan.n_edges, B = plan.envelope_blocks;
    if (G > h->max_graphs || P > h->max_poses || E > h->max_edges || B > h->max_blocks) {
        char text[256];
        snprintf(text, sizeof text, "capacity exceeded: the call needs %lld graphs, %lld poses, %lld edges and %lld envelope blocks (the handle has %lld, %lld, %lld, %lld)",
                 (long long)G, (long long)P, (long long)E, (long long)B, (long long)h->max_graphs, (long long)h->max_poses, (long long)h->max_edges,
                 (long long)h->max_blocks);
        return set_err(fn, text);
    }
    h->work[0] = h->work[1] = 0;
    h->work[2] = B, h->work[3] = G;
    if (G == 0) return 0;
    HC(hipSetDevice(h->device));
    const PgArena a(G, P, E);
    char *hp = h->hp_io, *d = h->d_io;
    memcpy(hp + a.x, poses7, 7 * P * sizeof(double));
    memset(hp + a.summary, 0, G * sizeof(ll_pose_graph_summary));
    if (E > 0) {
        memcpy(hp + a.meas, edge_meas7, 7 * E * sizeof(double));
        if (plan.any_information) memcpy(hp + a.info_l, plan.info_l.data(), 36 * E * sizeof(double));
        memcpy(hp + a.edge_ab, edge_ab, 2 * E * sizeof(int32_t));
        memcpy(hp + a.has_l, plan.edge_has_l.data(), E * sizeof(int32_t));
        memcpy(hp + a.inc, plan.inc.data(), 2 * E * sizeof(int32_t));
    }
    memcpy(hp + a.strip, plan.strip.data(), P * sizeof(int64_t));
    memcpy(hp + a.graphs, plan.graphs.data(), G * sizeof(PgGraph));
    memcpy(hp + a.inc_start, plan.inc_start.data(), (P + 1) * sizeof(int32_t));
    memcpy(hp + a.first, plan.first.data(), P * sizeof(int32_t));

    PgView v{};
    v.graphs = (const PgGraph *)(d + a.graphs);
    v.x = (double *)(d + a.x);
    v.edge_ab = (const int32_t *)(d + a.edge_ab);
    v.meas = (const double *)(d + a.meas);
    v.info_l = (const double *)(d + a.info_l);
    v.edge_has_l = (const int32_t *)(d + a.has_l);
    v.inc_start = (const int32_t *)(d + a.inc_start);
    v.inc = (const int32_t *)(d + a.inc);
    v.first = (const int32_t *)(d + a.first);
    v.strip = (const int64_t *)(d + a.strip);
    v.summary = (ll_pose_graph_summary *)(d + a.summary);
    double *w = h->d_work;
    v.cand = w, w += 7 * P;
    v.r = w, w += 6 * E;
    v.J = w, w += 72 * E;
    v.ecost = w, w += E;
    v.scale = w, w += 6 * P;
    v.diag = w, w += 6 * P;
    v.g = w, w += 6 * P;
    v.rhs = w, w += 6 * P;
    v.y = w, w += 6 * P;
    v.ps0 = w, w += P;
    v.ps1 = w, w += P;
    v.H = h->d_H;
    v.prm = prm;

    const char *err = nullptr;
    HC(hipMemcpyAsync(d, hp, a.end, hipMemcpyHostToDevice, h->stream));
    if (pose_graph_launch(v, (int)G, h->stream, &err)) return set_err(fn, err);
    HC(hipMemcpyAsync(hp, d, a.meas, hipMemcpyDeviceToHost, h->stream));  // the poses and the summaries
    h->work[0] = 3;  // the call in, the launch, the results out
    HC(hipStreamSynchronize(h->stream));  // the one wait
    h->work[1] = 1;
    memcpy(poses7, hp + a.x, 7 * P * sizeof(double));
    memcpy(summary, hp + a.summary, G * sizeof(ll_pose_graph_summary));
    return 0;
}

extern "C" int ll_pose_graph_work(ll_pose_graph *h, int64_t out[4])
{
    if (!h || !out) return set_err("ll_pose_graph_work", "null argument");
    for (int i = 0; i < 4; i++) out[i] = h->work[i];
    return 0;
}
