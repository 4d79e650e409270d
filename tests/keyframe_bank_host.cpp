// The key-frame bank's arithmetic on the CPU (tests/test_keyframe_bank_host.py, tests/test_gpu_keyframe_bank.py): the tile body of
// loam_livox_amd/csrc/ll_keyframe_bank_core.h -- the very text kb_corr_kernel runs -- beside the straight double loop of
// cm_kf_similarity_kernel's definition.
// argv: <in.bin> <out.bin>.  in: int32 n_pairs, then per pair a[3600], b[3600] float32.  out, per pair, as float64: the 3600 sums of
// the tiled body [Y * 60 + X], the 3600 sums of the straight loop, the maximum over 60 x 60 shifts (tiled), the maximum over 61 x 61
// shifts (straight), the norms A and B in the device's summation order, and the similarity (a float, widened).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ll_keyframe_bank_core.h"

using namespace ll;

// num( Y, X ) as cm_kf_similarity_kernel writes it; Y, X in 0 .. 60
static double straight(const float *a, const float *b, int Y, int X)
{
    const int half = LL_KB_RES / 2;
    double num = 0.0;
    for (int i = 0; i < LL_KB_RES; i++) {
        const int bi = (Y + i - half + LL_KB_RES) % LL_KB_RES;
        for (int j = 0; j < LL_KB_RES; j++) num += (double)a[i * LL_KB_RES + j] * (double)b[bi * LL_KB_RES + (X + j - half + LL_KB_RES) % LL_KB_RES];
    }
    return num;
}

// sum of squares in the device's order: 1 024 thread-strided partial sums, the shuffle-down tree of every wavefront of 64 (a lane
// whose partner lies beyond the wavefront reads itself), then wavefronts 0 .. 15 in sequence
static double device_order_norm(const float *img)
{
    double part[1024];
    for (int t = 0; t < 1024; t++) {
        double n = 0.0;
        for (int e = t; e < LL_KB_BINS; e += 1024) n += (double)img[e] * (double)img[e];
        part[t] = n;
    }
    double A = 0.0;
    for (int w = 0; w < 16; w++) {
        double x[64], y[64];
        for (int l = 0; l < 64; l++) x[l] = part[64 * w + l];
        for (int off = 32; off > 0; off >>= 1) {
            for (int l = 0; l < 64; l++) y[l] = x[l] + (l + off < 64 ? x[l + off] : x[l]);
            for (int l = 0; l < 64; l++) x[l] = y[l];
        }
        A += x[0];
    }
    return A;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n_pairs = 0;
    if (fread(&n_pairs, sizeof(int), 1, f) != 1 || n_pairs < 0 || n_pairs > 4096) return 3;
    std::vector<float> img((size_t)n_pairs * 2 * LL_KB_BINS);
    if (!img.empty() && fread(img.data(), sizeof(float), img.size(), f) != img.size()) return 3;
    fclose(f);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    std::vector<float> pad(LL_KB_PAD_FLOATS);
    std::vector<double> rec(2 * LL_KB_BINS + 5);
    for (int p = 0; p < n_pairs; p++) {
        const float *a = &img[(size_t)p * 2 * LL_KB_BINS], *b = a + LL_KB_BINS;
        double *tiled = rec.data(), *plain = tiled + LL_KB_BINS;
        double best60 = -1.0e300, best61 = -1.0e300;
        for (int tile = 0; tile < LL_KB_TILES; tile++) {
            // (every float of the padded rows that a tile reads is written: every column below LL_KB_PAD_COLS of all sixty rows; the rest is never read)
            for (int e = 0; e < LL_KB_BINS; e++) kb_pad_element(b[e], e, tile, pad.data());
            for (int t = 0; t < LL_KB_THREADS; t++) {
                if ((t & 63) >= LL_KB_RES) continue;
                double acc[LL_KB_R];
                const int Y = kb_item_y(t), x0 = kb_item_x0(t);
                kb_item(a, pad.data(), Y, x0, acc);
                for (int r = 0; r < LL_KB_R; r++) {
                    tiled[Y * LL_KB_RES + tile * LL_KB_TILE_X + x0 + r] = acc[r];
                    best60 = acc[r] > best60 ? acc[r] : best60;
                }
            }
        }
        for (int Y = 0; Y <= LL_KB_RES; Y++)
            for (int X = 0; X <= LL_KB_RES; X++) {
                const double num = straight(a, b, Y, X);
                if (Y < LL_KB_RES && X < LL_KB_RES) plain[Y * LL_KB_RES + X] = num;
                best61 = num > best61 ? num : best61;
            }
        const double A = device_order_norm(a), B = device_order_norm(b);
        double *tail = plain + LL_KB_BINS;
        tail[0] = best60;
        tail[1] = best61;
        tail[2] = A;
        tail[3] = B;
        tail[4] = (double)kb_quotient(A, B, best60);
        if (fwrite(rec.data(), sizeof(double), rec.size(), out) != rec.size()) return 4;
    }
    fclose(out);
    return 0;
}
