// ll_keyframe_bank.h -- host entry points of ll_keyframe_bank_kernels.hip (the key-frame descriptor bank, ll_api_keyframe_bank.hip).
// Every function only enqueues on s.  d_img: the bank's entries, [entries][2 kinds][3600] floats (line image, plane image); d_norm:
// [entries][2] sums of squares; d_pairs: {a = the new key frame's entry, b = the old one's}, validated by the caller.
#pragma once
#include <hip/hip_runtime.h>

namespace ll {

// the two norms of one entry, in cm_kf_similarity_kernel's summation order: d_norm2[0] line, [1] plane.  One launch.
int keyframe_bank_norms(const float *d_entry, double *d_norm2, hipStream_t s, const char **err);
// d_sim[0 .. n_pairs) line similarities, [n_pairs .. 2 n_pairs) plane similarities; d_partial: 6 doubles per pair.  Two launches.
int keyframe_bank_match(const float *d_img, const double *d_norm, const int2 *d_pairs, int n_pairs, double *d_partial, float *d_sim,
                        hipStream_t s, const char **err);
// all 3600 sums num( Y, X ), Y, X < 60, of d_pair[0] and one kind into d_surface[Y * 60 + X].  One launch.
int keyframe_bank_surface(const float *d_img, const int2 *d_pair, int kind, double *d_surface, hipStream_t s, const char **err);

}  // namespace ll
