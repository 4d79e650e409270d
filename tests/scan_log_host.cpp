// Test-only: the scan log of the batched match buffer on the CPU (tests/test_scan_log_host.py).  The two kernels of
// ll_scan_log_kernels.hip, compiled from their own unit against tests/cellmap_batch_shim, and the bookkeeping of ll_scan_log.h --
// the text ll_api_history_batch_scanlog.hip and ll_api_map_refine.hip drive them with -- replay a schedule of log calls, hand-overs
// and drops, then one gather.  Also built with -fsanitize=address,undefined and run as it is: every block lies in a chunk of exactly
// chunk_blocks * max_pts points, so a write past a block's end or a read of a freed chunk is the sanitizer's to report.
//
//   scan_log_host IN OUT
// IN : int32 S, T, max_hist, max_pts, chunk_blocks; per step, per slot: int32 n (-1: not in the step's append), int32 named, then
//      (n >= 0) n x 4 float xf, max_pts x 4 float scan, n int32 full_idx; after the slots int32 n_hand, n_hand x int32 slot; int32
//      n_drop, n_drop x int32 group ordinal (0 = the first group handed over).  Last: int32 n_req, (n_req + 1) x int32 group_off,
//      group_off[n_req] x int32 group ordinal.
// OUT: per step int32 in_use, n_blocks, enqueued; then int32 n_groups; per group handed over int32 alive, n, n x 4 float (bits);
//      then (n_req + 1) x int64 req_off, req_off[n_req] x 4 float; then int32 each: a consumed group is refused as unknown, a group
//      named twice is refused, blocks in use once the gather's groups are consumed.
#include <hip/hip_runtime.h>

#include <stdio.h>

#include "../loam_livox_amd/csrc/ll_scan_log_kernels.hip"
using namespace ll;

static void rd(void *p, size_t size, size_t n, FILE *f)
{
    if (n && fread(p, size, n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}
static int rd_i(FILE *f) { int v; rd(&v, 4, 1, f); return v; }
static void put_i(FILE *f, int v) { fwrite(&v, 4, 1, f); }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const int S = rd_i(in), T = rd_i(in), max_hist = rd_i(in), max_pts = rd_i(in), chunk_blocks = rd_i(in);
    SlBook book;
    sl_init(book, S, max_hist, chunk_blocks);
    std::vector<float4 *> chunks;
    auto block_at = [&](int b) { return chunks[(size_t)(b / chunk_blocks)] + (size_t)(b % chunk_blocks) * (size_t)max_pts; };
    auto room = [&](int want) {
        for (int c = sl_chunks_short(book, want); c > 0; c--) {
            chunks.push_back(new float4[(size_t)chunk_blocks * (size_t)max_pts]);
            sl_add_chunk(book);
        }
    };
    room(chunk_blocks);
    std::vector<float4> xf((size_t)S * max_pts), scan((size_t)S * max_pts);
    std::vector<int> full_idx((size_t)S * max_pts), n(S), named(S);
    std::vector<SlSlot> tab(S);
    std::vector<int64_t> ids;  // ordinal -> group id
    const char *err = nullptr;
    for (int step = 0; step < T; step++) {
        int want = 0, max_n = 0;
        for (int s = 0; s < S; s++) {
            n[s] = rd_i(in);
            named[s] = rd_i(in) && n[s] >= 0;
            if (n[s] < 0) continue;
            if (n[s] > max_pts) return 3;
            rd(&xf[(size_t)s * max_pts], 16, (size_t)n[s], in);
            rd(&scan[(size_t)s * max_pts], 16, (size_t)max_pts, in);
            rd(&full_idx[(size_t)s * max_pts], 4, (size_t)n[s], in);
            if (named[s]) want++, max_n = std::max(max_n, n[s]);
        }
        room(want);
        std::vector<int> block(S, -1);
        for (int s = 0; s < S; s++) {
            if (named[s]) block[s] = sl_take(book);
            tab[s] = SlSlot{named[s] ? block_at(block[s]) : nullptr, named[s] ? n[s] : 0, 0};
        }
        if (sl_log(tab.data(), xf.data(), max_pts, scan.data(), full_idx.data(), max_pts, S, max_n, nullptr, &err)) return 4;
        for (int s = 0; s < S; s++) {
            if (n[s] < 0) continue;
            if (named[s]) sl_push(book, s, block[s], n[s]);
            sl_trim(book, s);
        }
        for (int k = rd_i(in); k > 0; k--) ids.push_back(sl_hand_over(book, rd_i(in)));
        for (int k = rd_i(in); k > 0; k--)
            if (!sl_drop(book, ids[(size_t)rd_i(in)])) return 5;
        put_i(out, book.in_use);
        put_i(out, book.n_blocks);
        put_i(out, max_n > 0 ? 1 : 0);
    }
    put_i(out, (int)ids.size());
    for (int64_t id : ids) {
        const std::vector<SlScan> *g = sl_group(book, id);
        put_i(out, g ? 1 : 0);
        int total = 0;
        for (size_t k = 0; g && k < g->size(); k++) total += (*g)[k].n;
        put_i(out, total);
        for (size_t k = 0; g && k < g->size(); k++) fwrite(block_at((*g)[k].block), 16, (size_t)(*g)[k].n, out);
    }
    // the gather of ll_map_refine_add_logged
    const int n_req = rd_i(in);
    std::vector<int64_t> group_off((size_t)n_req + 1), group_ids;
    for (int r = 0; r <= n_req; r++) group_off[(size_t)r] = rd_i(in);
    for (int64_t g = 0; g < group_off[(size_t)n_req]; g++) group_ids.push_back(ids[(size_t)rd_i(in)]);
    if (!sl_check_groups(book, (int64_t)group_ids.size(), group_ids.data()).empty()) return 6;
    SlPlan plan;
    sl_gather_plan(book, n_req, group_off.data(), group_ids.data(), &plan);
    std::vector<SlCopy> work;
    for (const SlItem &it : plan.items) work.push_back(SlCopy{block_at(it.block) + it.first, it.dst, it.n, it.req});
    std::vector<float4> stage((size_t)plan.req_off[(size_t)n_req] + 1);
    if (sl_gather(work.data(), (int)work.size(), stage.data(), nullptr, &err)) return 7;
    fwrite(plan.req_off.data(), 8, plan.req_off.size(), out);
    fwrite(stage.data(), 16, (size_t)plan.req_off[(size_t)n_req], out);
    // consumed afterwards; then the refusals: a consumed group is unknown, a group named twice
    std::vector<int64_t> twice;
    if (!group_ids.empty()) twice = {group_ids[0], group_ids[0]};
    const bool twice_refused = twice.empty() || sl_check_groups(book, 2, twice.data()) == "a group is named twice";
    for (int64_t id : group_ids) sl_drop(book, id);
    const bool unknown_refused = group_ids.empty() || sl_check_groups(book, 1, group_ids.data()) == "unknown or consumed group";
    put_i(out, unknown_refused ? 1 : 0);
    put_i(out, twice_refused ? 1 : 0);
    put_i(out, book.in_use);
    for (float4 *p : chunks) delete[] p;
    fclose(in);
    fclose(out);
    return 0;
}
