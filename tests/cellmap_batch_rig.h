// Test-only: what the CPU drivers of the batched stores' launch chains share (tests/cellmap_batch_kernels_host.cpp,
// fullmap_batch_host.cpp, cellmatch_batch_host.cpp, cellmap_batch_extract_host.cpp).  Include it behind the kernel units.  A Store is a
// CbDev at a fixed capacity, allocated through the array enumeration of ll_cellmap_batch.h, with the host side the API keeps beside it
// (frame counters, cell offsets); an append and a materialisation go through the host functions of ll_cellmap_batch_core.h, the ones
// ll_api_history_batch_stores.hip calls.  Everything a Store or an Owned allocates is freed with it.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ll_cellmap_batch.h"

namespace rig {
using namespace ll;

inline void put_i(FILE *f, int v) { fwrite(&v, 4, 1, f); }
inline void rd(void *p, size_t size, size_t n, FILE *f)
{
    if (n && fread(p, size, n, f) != n) exit(3);
}

struct Owned {
    std::vector<void *> all;
    template <typename T> void al(T *&p, size_t n)
    {
        p = (T *)calloc(n + 8, sizeof(T));
        all.push_back(p);
    }
    Owned() {}
    Owned(const Owned &) = delete;
    ~Owned()
    {
        for (void *p : all) free(p);
    }
};

struct Store {
    CbDev m;
    std::vector<int> frame, coff, n;  // [S] frame counters, [S + 1] cell offsets at the last append, [S] the clouds of this step
    float4 *src;                      // [S][maxp] the clouds of this step
    size_t maxp;
    Owned own;
    int launches = 0;
    const char *err = nullptr;

    Store(int S, float res, int threshold, size_t cap, size_t max_points) : frame(S, 0), coff(S + 1, 0), n(S, -1), maxp(max_points)
    {
        memset(&m, 0, sizeof(m));
        m.S = S;
        m.geom = cell_geom(res);
        m.threshold = threshold;
        auto a = [&](auto *&p, size_t count, bool) { own.al(p, count); return 0; };
        cb_each_log(m, cap, a);
        cb_each_table(m, cap, a);
        cb_each_append(m, cap, a);
        cb_each_mat(m, cap, a);
        cb_each_fixed(m, a);
        m.cap = m.ccap = m.acap = m.mcap = cap;
        char *tmp;
        own.al(tmp, 64);
        m.tmp = tmp;
        m.tmp_bytes = 64;
        own.al(src, S * maxp);
    }
    // one step's clouds: per slot int32 n (-1: the slot sits the step out) and n x {x, y, z} float
    void read_clouds(FILE *in)
    {
        for (int s = 0; s < m.S; s++) {
            rd(&n[s], 4, 1, in);
            if (n[s] > (int)maxp) exit(2);  // (a cloud the step's stack cannot hold: a malformed IN file, like a wrong argument)
            for (int i = 0; i < n[s]; i++) {
                float p[3];
                rd(p, 4, 3, in);
                src[s * maxp + i] = make_float4(p[0], p[1], p[2], 7.f);
            }
        }
    }
    bool active(int s) const { return n[s] >= 0; }
    // the two host halves of an append, around the chains of the caller
    long long begin_append(int *max_n)
    {
        return cb_fill_slots(m.tab, m.S, [&](int s) { return n[s]; }, frame.data(), m.n_log, max_n);
    }
    void end_append(bool appended)
    {
        if (appended) m.n_cells = m.counts[1];
        cb_after_append(frame.data(), coff.data(), m.S, [&](int s) { return active(s); }, appended ? m.coff : nullptr);
    }
    // the clouds of this step behind the log; returns the new points, -1 on an error
    long long append()
    {
        int max_n = 0;
        const long long n_new = begin_append(&max_n);
        if (n_new > 0 && cb_append(m, src, (int)maxp, max_n, n_new, nullptr, &launches, &err)) {
            printf("append: %s\n", err);
            return -1;
        }
        end_append(n_new > 0);
        return n_new;
    }
    int materialise()
    {
        if (cb_materialise(m, nullptr, &launches, &err)) {
            printf("mat: %s\n", err);
            return -1;
        }
        m.n_log = m.poff[m.S];
        return 0;
    }
    // per slot: int32 frame, n_cells, n_points; n_cells x 3 int32 cell indices; n_cells + 1 int32 cell_start; n_cells int32 stamps;
    // n_points x 3 float
    void dump(FILE *out) const
    {
        for (int s = 0; s < m.S; s++) {
            const int c0 = m.coff[s], nc = m.coff[s + 1] - c0, p0 = m.poff[s], np = m.poff[s + 1] - p0;
            put_i(out, frame[s]); put_i(out, nc); put_i(out, np);
            for (int c = 0; c < nc; c++) { int k[3]; cell_unpack(m.ckey[c0 + c], k); fwrite(k, 4, 3, out); }
            for (int c = 0; c <= nc; c++) put_i(out, nc > 0 ? m.cstart[c0 + s + c] : 0);
            for (int c = 0; c < nc; c++) put_i(out, m.clast[c0 + c]);
            for (int i = 0; i < np; i++) fwrite(&m.pts[p0 + i].x, 4, 3, out);
        }
    }
};

}  // namespace rig
