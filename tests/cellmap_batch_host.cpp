// Test-only host build of the batched cell maps' deferred store (tests/test_cellmap_batch_host.py): the log, the epochs and the
// materialisation of ll_cellmap_batch_kernels.hip restated on the CPU with the SAME per-point decisions, those of
// loam_livox_amd/csrc/ll_cellmap_batch_core.h.  Each kernel of the two chains is one loop here; a loop reads what its kernel reads
// (the classification sees the table as it was before the cloud, never a cell the cloud itself opens).
//
//   cellmap_batch_host IN OUT
// IN : int32 n_maps, n_steps, threshold; float resolution; per step: int32 read; per map: int32 n (-1: the map sits the step out),
//      n x 3 float.
// OUT: after every step with read != 0, per map: int32 frame, n_cells, n_points; n_cells x 3 int32 cell indices; n_cells + 1
//      int32 cell_start; n_cells int32 last-update stamps; n_points x 3 float.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../loam_livox_amd/csrc/ll_cellmap_batch_core.h"

using namespace ll;
typedef unsigned long long u64;

struct Pt {
    float x, y, z;
    u64 key;
    int slot, epoch;
};
struct Cell {
    u64 key;
    int slot, last, epoch;
};

struct Store {
    int S = 0, thr = 0;
    CellGeom g;
    std::vector<Pt> log;
    std::vector<Cell> table;  // by (slot, key)
    std::vector<int> coff, poff, frame;
    std::vector<int> cstart;  // slot s's entries start at coff[s] + s
    bool dirty = false;
    long sorted_in_add = 0, appended = 0, materialisations = 0;

    void init(int n_maps, int threshold, float resolution)
    {
        S = n_maps;
        thr = threshold;
        g = cell_geom(resolution);
        coff.assign(S + 1, 0);
        poff.assign(S + 1, 0);
        frame.assign(S, 0);
        cstart.assign(S + 1, 0);
    }

    void keys_of_table(std::vector<u64> &k, std::vector<int> &s) const
    {
        k.resize(table.size());
        s.resize(table.size());
        for (size_t i = 0; i < table.size(); i++) k[i] = table[i].key, s[i] = table[i].slot;
    }

    // clouds[s]: nullptr = inactive
    void append(const std::vector<const std::vector<float> *> &clouds)
    {
        std::vector<u64> ckey;
        std::vector<int> cslot;
        keys_of_table(ckey, cslot);
        const size_t base = log.size();
        struct Cand {
            u64 key;
            int slot;
        };
        std::vector<Cand> cand;
        // cb_classify_kernel
        for (int s = 0; s < S; s++) {
            if (!clouds[s]) continue;
            const std::vector<float> &c = *clouds[s];
            for (size_t i = 0; i < c.size() / 3; i++) {
                Pt p{c[3 * i], c[3 * i + 1], c[3 * i + 2], 0, s, 0};
                p.key = cb_point_key(p.x, p.y, p.z, g);
                Cand cd{LL_CELL_KEY_NONE, S};
                if (p.key != LL_CELL_KEY_NONE) {
                    const int ci = cb_find(ckey.data(), coff[s], coff[s + 1], p.key);
                    if (ci >= 0) {
                        const int before = table[ci].last;
                        table[ci].last = frame[s];
                        if (cb_first_touch(before, frame[s]) && cb_stale(frame[s], before, thr)) table[ci].epoch = cb_epoch_after_reset(table[ci].epoch);
                    } else {
                        cd.key = p.key;
                        cd.slot = s;
                    }
                }
                log.push_back(p);
                cand.push_back(cd);
            }
        }
        const size_t n_new = cand.size();
        appended += (long)n_new;
        if (n_new > 0) {
            // the two sorts: by key, then stably by slot
            std::stable_sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) { return a.key < b.key; });
            std::stable_sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) { return a.slot < b.slot; });
            sorted_in_add += (long)n_new;
            // cb_newcell_flag_kernel + the merge
            std::vector<Cell> opened;
            for (size_t a = 0; a < n_new; a++)
                if (cand[a].slot < S && (a == 0 || cand[a - 1].slot != cand[a].slot || cand[a - 1].key != cand[a].key))
                    opened.push_back(Cell{cand[a].key, cand[a].slot, frame[cand[a].slot], 0});
            std::vector<Cell> merged(table.size() + opened.size());
            std::merge(table.begin(), table.end(), opened.begin(), opened.end(), merged.begin(),
                       [](const Cell &a, const Cell &b) { return cb_less(a.slot, a.key, b.slot, b.key); });
            table.swap(merged);
            keys_of_table(ckey, cslot);
            for (int s = 0; s <= S; s++) coff[s] = cb_lower_bound_slot(cslot.data(), (int)cslot.size(), s);  // cb_coff_kernel
            // cb_epoch_kernel
            for (size_t j = base; j < log.size(); j++) {
                Pt &p = log[j];
                if (p.key == LL_CELL_KEY_NONE) continue;
                const int ci = cb_find(ckey.data(), coff[p.slot], coff[p.slot + 1], p.key);
                if (ci >= 0) p.epoch = table[ci].epoch;
            }
        }
        for (int s = 0; s < S; s++)
            if (clouds[s]) frame[s] += cb_frame_step(cells_before[s] == 0);
        dirty = true;
    }
    std::vector<int> cells_before;
    void note_cells()
    {
        cells_before.resize(S);
        for (int s = 0; s < S; s++) cells_before[s] = coff[s + 1] - coff[s];
    }

    void materialise()
    {
        if (!dirty) return;
        std::vector<u64> ckey;
        std::vector<int> cslot;
        keys_of_table(ckey, cslot);
        // cb_live_kernel
        struct Ord {
            u64 key;
            int slot, pos;
        };
        std::vector<Ord> o(log.size());
        for (size_t j = 0; j < log.size(); j++) {
            const Pt &p = log[j];
            bool live = false;
            if (p.key != LL_CELL_KEY_NONE) {
                const int ci = cb_find(ckey.data(), coff[p.slot], coff[p.slot + 1], p.key);
                live = ci >= 0 && cb_live(p.epoch, table[ci].epoch);
            }
            o[j] = Ord{live ? p.key : LL_CELL_KEY_NONE, live ? p.slot : S, (int)j};
        }
        std::stable_sort(o.begin(), o.end(), [](const Ord &a, const Ord &b) { return a.key < b.key; });
        std::stable_sort(o.begin(), o.end(), [](const Ord &a, const Ord &b) { return a.slot < b.slot; });
        // cb_gather_kernel, cb_poff_kernel, cb_cstart_kernel
        std::vector<Pt> store;
        std::vector<int> sslot;
        std::vector<u64> skey;
        for (const Ord &e : o) {
            sslot.push_back(e.slot);
            if (e.slot >= S) continue;
            store.push_back(log[e.pos]);
            skey.push_back(e.key);
        }
        for (int s = 0; s <= S; s++) poff[s] = cb_lower_bound_slot(sslot.data(), (int)sslot.size(), s);
        cstart.assign(table.size() + S + 1, 0);
        for (size_t t = 0; t < table.size(); t++) {
            const int s = table[t].slot;
            cstart[t + s] = cb_lower_bound(skey.data(), poff[s], poff[s + 1], table[t].key) - poff[s];
        }
        for (int s = 0; s < S; s++) cstart[coff[s + 1] + s] = poff[s + 1] - poff[s];
        log.swap(store);
        dirty = false;
        materialisations++;
    }
};

static void put_i(FILE *f, int v) { fwrite(&v, sizeof(int), 1, f); }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int n_maps = 0, n_steps = 0, thr = 0;
    float res = 0.f;
    if (fread(&n_maps, 4, 1, in) != 1 || fread(&n_steps, 4, 1, in) != 1 || fread(&thr, 4, 1, in) != 1 || fread(&res, 4, 1, in) != 1) return 3;
    Store st;
    st.init(n_maps, thr, res);
    for (int step = 0; step < n_steps; step++) {
        int read = 0;
        if (fread(&read, 4, 1, in) != 1) return 3;
        std::vector<std::vector<float>> data(n_maps);
        std::vector<const std::vector<float> *> clouds(n_maps, nullptr);
        for (int s = 0; s < n_maps; s++) {
            int n = 0;
            if (fread(&n, 4, 1, in) != 1) return 3;
            if (n < 0) continue;
            data[s].resize((size_t)n * 3);
            if (n > 0 && fread(data[s].data(), sizeof(float), (size_t)n * 3, in) != (size_t)n * 3) return 3;
            clouds[s] = &data[s];
        }
        st.note_cells();
        st.append(clouds);
        if (st.sorted_in_add > st.appended) return 4;  // an add sorts the new points at most
        if (!read) continue;
        st.materialise();
        st.materialise();  // (a second read costs nothing)
        for (int s = 0; s < n_maps; s++) {
            const int c0 = st.coff[s], nc = st.coff[s + 1] - c0, p0 = st.poff[s], np = st.poff[s + 1] - p0;
            put_i(out, st.frame[s]);
            put_i(out, nc);
            put_i(out, np);
            for (int c = 0; c < nc; c++) {
                int k[3];
                cell_unpack(st.table[c0 + c].key, k);
                fwrite(k, sizeof(int), 3, out);
            }
            for (int c = 0; c <= nc; c++) put_i(out, nc > 0 ? st.cstart[c0 + s + c] : 0);
            for (int c = 0; c < nc; c++) put_i(out, st.table[c0 + c].last);
            for (int i = 0; i < np; i++) fwrite(&st.log[p0 + i].x, sizeof(float), 3, out);
        }
    }
    put_i(out, (int)st.materialisations);
    fclose(in);
    fclose(out);
    return 0;
}
