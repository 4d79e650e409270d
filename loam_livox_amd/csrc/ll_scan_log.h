// ll_scan_log.h -- the host side of the scan log of the batched match buffer (ll_history_batch_enable_scan_log): its bookkeeping in
// plain C++, shared by ll_api_history_batch_scanlog.hip, ll_api_map_refine.hip and tests/scan_log_host.cpp, and the entry points of
// ll_scan_log_kernels.hip.
//
// Storage is a pool of fixed-size blocks, one scan per block (max_points_per_frame float4), allocated in chunks that never move: the
// pool grows by another chunk and nothing is copied.  Everything about a block's life is decided on the host -- which scans are
// logged, when a FIFO is trimmed, handed over, dropped or consumed -- so the free list, the slots' FIFOs and the groups live here, and
// the device only ever sees block addresses.
//   FIFO    per slot, of (block, n): m_laser_cloud_full_history (laser_mapping.hpp:1456), trimmed to maximum_history_size (:1480-1486).
//   group   what one hand-over took (:1550-1553, 1558): the slot's whole FIFO in order, under a 64-bit id that is never reused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <deque>
#include <string>
#include <unordered_map>
#include <vector>

#include "ll_scan_log_core.h"

namespace ll {

typedef SlSlotT<float4> SlSlot;
typedef SlCopyT<float4> SlCopy;

struct SlScan {
    int block, n;
};

struct SlBook {
    int S = 0, max_hist = 0, chunk_blocks = 0;  // blocks of one chunk
    int n_blocks = 0, in_use = 0;               // blocks allocated / held by a FIFO or a group
    std::vector<int> free_list;                 // taken from the back
    std::vector<std::deque<SlScan>> fifo;       // [S]
    std::unordered_map<int64_t, std::vector<SlScan>> groups;
    int64_t next_id = 1;
};

inline void sl_init(SlBook &b, int S, int max_hist, int chunk_blocks)
{
    b = SlBook();
    b.S = S, b.max_hist = max_hist, b.chunk_blocks = chunk_blocks;
    b.fifo.assign((size_t)S, std::deque<SlScan>());
}

// chunks the pool lacks for `want` free blocks
inline int sl_chunks_short(const SlBook &b, int want)
{
    const int lack = want - (int)b.free_list.size();
    return lack <= 0 ? 0 : (lack + b.chunk_blocks - 1) / b.chunk_blocks;
}

// another chunk has been allocated: its blocks join the free list, lowest taken first
inline void sl_add_chunk(SlBook &b)
{
    for (int k = b.chunk_blocks - 1; k >= 0; k--) b.free_list.push_back(b.n_blocks + k);
    b.n_blocks += b.chunk_blocks;
}

inline int sl_take(SlBook &b)
{
    const int block = b.free_list.back();
    b.free_list.pop_back();
    b.in_use++;
    return block;
}

inline void sl_release(SlBook &b, int block)
{
    b.free_list.push_back(block);
    b.in_use--;
}

// :1456 for slot s
inline void sl_push(SlBook &b, int s, int block, int n) { b.fifo[(size_t)s].push_back(SlScan{block, n}); }

// :1480-1486 for slot s: one scan leaves when the FIFO is longer than maximum_history_size
inline void sl_trim(SlBook &b, int s)
{
    std::deque<SlScan> &f = b.fifo[(size_t)s];
    if ((int)f.size() > b.max_hist) {
        sl_release(b, f.front().block);
        f.pop_front();
    }
}

// :1550-1553, 1558: the slot's whole FIFO becomes a group (an empty one gives an empty group) and the FIFO is empty afterwards
inline int64_t sl_hand_over(SlBook &b, int s)
{
    const int64_t id = b.next_id++;
    std::deque<SlScan> &f = b.fifo[(size_t)s];
    b.groups.emplace(id, std::vector<SlScan>(f.begin(), f.end()));
    f.clear();
    return id;
}

inline const std::vector<SlScan> *sl_group(const SlBook &b, int64_t id)
{
    const auto it = b.groups.find(id);
    return it == b.groups.end() ? nullptr : &it->second;
}

// the group's blocks back to the free list; false for an id that names no group (unknown, dropped or consumed)
inline bool sl_drop(SlBook &b, int64_t id)
{
    const auto it = b.groups.find(id);
    if (it == b.groups.end()) return false;
    for (const SlScan &e : it->second) sl_release(b, e.block);
    b.groups.erase(it);
    return true;
}

// "" when every id names a group and none is named twice, else the refusal's text
inline std::string sl_check_groups(const SlBook &b, int64_t n, const int64_t *ids)
{
    std::unordered_map<int64_t, int> seen;
    for (int64_t i = 0; i < n; i++) {
        if (!sl_group(b, ids[i])) return "unknown or consumed group";
        if (seen[ids[i]]++) return "a group is named twice";
    }
    return "";
}

// one piece of a gather: points first .. first + n of `block` to staging index dst, for request req
struct SlItem {
    int req, block, first, n;
    long long dst;
};

struct SlPlan {
    std::vector<SlItem> items;       // (request, block, chunk)
    std::vector<int64_t> req_off;    // [n_req + 1] first staging point of every request
};

// The gather of n_req requests: request r is the concatenation, in order, of the scans of the groups group_ids[group_off[r] ..
// group_off[r + 1]] (m_accumulated_point_cloud, :943-946).  The ids have passed sl_check_groups.
inline void sl_gather_plan(const SlBook &b, int64_t n_req, const int64_t *group_off, const int64_t *group_ids, SlPlan *plan)
{
    plan->items.clear();
    plan->req_off.assign((size_t)n_req + 1, 0);
    long long at = 0;
    for (int64_t r = 0; r < n_req; r++) {
        for (int64_t g = group_off[r]; g < group_off[r + 1]; g++)
            for (const SlScan &e : *sl_group(b, group_ids[g])) {
                for (int first = 0; first < e.n; first += SL_CHUNK) {
                    const int n = e.n - first < SL_CHUNK ? e.n - first : SL_CHUNK;
                    plan->items.push_back(SlItem{(int)r, e.block, first, n, at + first});
                }
                at += e.n;
            }
        plan->req_off[(size_t)r + 1] = at;
    }
}

// ---- ll_scan_log_kernels.hip
// One launch for all slots: slot s with tab[s].dst writes tab[s].n points there -- x, y, z from xf[s][i], the intensity from the scan
// through full_idx (sl_logged_point).  tab is on the device; max_n bounds the n.  Enqueues only.
int sl_log(const SlSlot *tab, const float4 *xf, int max_pts, const float4 *xyzi, const int *full_idx, int stride, int S, int max_n, hipStream_t s,
           const char **err);
// One launch for all requests: work item w copies work[w].n points from work[w].src to dst[work[w].dst ..].  work is on the device.
int sl_gather(const SlCopy *work, int n_work, float4 *dst, hipStream_t s, const char **err);

}  // namespace ll
