// ll_map_refine.h -- the host side of the key-frame map refinement: the check and the plan of a run (plain C++, shared by
// ll_api_map_refine.hip and tests/map_refine_host.cpp) and the entry points of ll_map_refine_kernels.hip.
//
// The structure of a run is host knowledge: the sizes of the stored clouds are known where they were added, so the selections'
// places in the work index space and the (selection, chunk) work list come from them without a device round trip.
#pragma once
#include <cmath>

#include <string>
#include <vector>

#include "ll_map_refine_core.h"

namespace ll {

struct MrWork {
    int sel, first;  // points first .. first + MR_CHUNK of selection sel
};

struct MrPlan {
    std::vector<MrSel> sel;
    std::vector<MrWork> work;
    int64_t total = 0;  // points of the run = the sum of the selections' sizes
};

// The check and the plan of a run over the clouds whose first points and sizes are cloud_off[0 .. n_clouds] (ascending).  Returns the
// refusal's text, or "" with *plan filled.  poses may be null for MR_FILTER_ONLY.
inline std::string mr_plan(int mode, int64_t n_sel, const int64_t *ids, const double *poses_ori7, const double *poses_opm7, float leaf,
                           const std::vector<int64_t> &cloud_off, MrPlan *plan)
{
    if (mode != MR_FILTER_THEN_MOVE && mode != MR_MOVE_THEN_FILTER && mode != MR_FILTER_ONLY) return "mode must be 0 (filter, then move) or 1 (move, then filter)";
    if (n_sel < 0) return "negative count";
    if (n_sel > MR_MAX_SEL) return "a run holds at most 2^20 selections";
    if (!(leaf > 0.f) || !std::isfinite(leaf)) return "the leaf must be positive and finite";
    const bool moves = mode != MR_FILTER_ONLY;
    if (n_sel > 0 && (!ids || (moves && (!poses_ori7 || !poses_opm7)))) return "null argument";
    const int64_t n_clouds = (int64_t)cloud_off.size() - 1;
    int64_t total = 0, n_work = 0;
    for (int64_t s = 0; s < n_sel; s++) {
        if (ids[s] < 0 || ids[s] >= n_clouds) return "id out of range";
        const int64_t n = cloud_off[ids[s] + 1] - cloud_off[ids[s]];
        total += n;
        n_work += (n + MR_CHUNK - 1) / MR_CHUNK;
        if (total >= 0x7fffffffLL) return "a run holds fewer than 2^31 points";
    }
    if (moves)
        for (int64_t i = 0; i < 7 * n_sel; i++)
            if (!std::isfinite(poses_ori7[i]) || !std::isfinite(poses_opm7[i])) return "a pose is not finite";
    plan->sel.assign((size_t)n_sel, MrSel());
    plan->work.clear();
    plan->work.reserve((size_t)n_work);
    plan->total = total;
    int64_t at = 0;
    for (int64_t s = 0; s < n_sel; s++) {
        MrSel &e = plan->sel[(size_t)s];
        e.src_off = cloud_off[ids[s]];
        e.n = (int)(cloud_off[ids[s] + 1] - cloud_off[ids[s]]);
        e.in_off = (int)at;
        at += e.n;
        if (moves)
            mr_affine(poses_ori7 + 7 * s, poses_opm7 + 7 * s, e.aff.R, e.aff.T);
        else
            for (int i = 0; i < 12; i++) (i < 9 ? e.aff.R[i] : e.aff.T[i - 9]) = (i == 0 || i == 4 || i == 8) ? 1.f : 0.f;
        for (int first = 0; first < e.n; first += MR_CHUNK) plan->work.push_back(MrWork{(int)s, first});
    }
    return "";
}

#ifdef __HIPCC__
// scratch of a chain: grown, never shrunk, content not kept between chains
struct MrDev {
    int64_t pt_cap = 0, sel_cap = 0, work_cap = 0;
    unsigned long long *keys = nullptr, *keys2 = nullptr;  // [pt_cap]
    unsigned int *vals = nullptr, *vals2 = nullptr, *is_head = nullptr, *rank = nullptr, *head_pos = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    MrSel *sel = nullptr;          // [sel_cap]
    MrWork *work = nullptr;        // [work_cap]
    unsigned int *mm = nullptr;    // [sel_cap][8] bounding box (ordered encoding) + finite count
    VoxelParams *prm = nullptr;    // [sel_cap]
    int *n_vox = nullptr, *vox_off = nullptr;  // [sel_cap]
    int *result = nullptr;         // [sel_cap + 1] output offsets, then [sel_cap] status: what the host waits for, in one piece
    int *n_vox_total = nullptr;
};

// the enqueue calls of one chain, whatever the number of selections: nine kernels of this unit, the sort and the scan counted as one
// call each (how many kernels hipcub launches inside them depends on the points and the key bits); the copies around it are the caller's
#define MR_CHAIN_LAUNCHES 11

int map_refine_room(MrDev &d, int64_t points, int64_t n_sel, int64_t n_work, const char **err);
void map_refine_free(MrDev &d);
// One chain over src, whose selections and work list are in d.sel / d.work already: the outputs packed ragged in selection order at
// out[0 ..], their offsets at d.result[0 .. n_sel] and the status values at d.result[n_sel + 1 ..].  Enqueues only.
int map_refine_chain(MrDev &d, const float4 *src, int mode, int n_sel, int n_work, int total, float leaf, float4 *out, hipStream_t s,
                     const char **err);
#endif

}  // namespace ll
