// ll_api_voxel.hip -- the voxel filter handle (ll_voxel_*) of the C ABI (ll_voxel_kernels.hip).  The forms that run a pair of
// filters in front of the registrar are in ll_api_reg.hip.
#include "ll_api_internal.h"

extern "C" int ll_voxel_create(int32_t device, int32_t max_clouds, int32_t max_points_per_cloud, ll_voxel **out)
{
    if (!out) return set_err("ll_voxel_create", "null argument");
    if (max_clouds < 1 || max_points_per_cloud < 1) return set_err("ll_voxel_create", "bad capacity");
    if (check_device(device)) return -1;
    ll_voxel *v = new ll_voxel();
    v->device = device;
    HC(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
    HC(hipEventCreateWithFlags(&v->ev, hipEventDisableTiming));
    const char *err = nullptr;
    if (voxel_alloc(v->dev, max_clouds, max_points_per_cloud, &err)) {
        voxel_free(v->dev);
        (void)hipStreamDestroy(v->stream);
        (void)hipEventDestroy(v->ev);
        delete v;
        return set_err("ll_voxel_create", err);
    }
    *out = v;
    return 0;
}

extern "C" void ll_voxel_destroy(ll_voxel *v)
{
    if (!v) return;
    (void)hipSetDevice(v->device);
    voxel_free(v->dev);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    if (v->ev) (void)hipEventDestroy(v->ev);
    delete v;
}

extern "C" int ll_voxel_filter(ll_voxel *v, int32_t n_clouds, const float *xyzi, const int32_t *n_points, int32_t stride_points,
                               const float leaf[3], float *out_xyzi, int32_t *n_out, int32_t *status)
{
    if (!v || !xyzi || !n_points || !leaf || !out_xyzi || !n_out) return set_err("ll_voxel_filter", "null argument");
    if (n_clouds < 1 || n_clouds > v->dev.max_clouds) return set_err("ll_voxel_filter", "n_clouds out of range");
    if (stride_points < 1 || stride_points > v->dev.stride) return set_err("ll_voxel_filter", "stride exceeds max_points_per_cloud");
    for (int b = 0; b < n_clouds; b++)
        if (n_points[b] < 0 || n_points[b] > stride_points) return set_err("ll_voxel_filter", "n_points out of range");
    HC(hipSetDevice(v->device));
    const size_t total = (size_t)n_clouds * stride_points;
    HC(hipMemcpyAsync(v->dev.in, xyzi, total * sizeof(float4), hipMemcpyHostToDevice, v->stream));
    HC(hipMemcpyAsync(v->dev.n, n_points, (size_t)n_clouds * sizeof(int), hipMemcpyHostToDevice, v->stream));
    const char *err = nullptr;
    if (voxel_filter(v->dev, v->dev.in, v->dev.n, stride_points, n_clouds, leaf, v->stream, &err)) return set_err("ll_voxel_filter", err);
    v->last_stream = v->stream;
    HC(hipMemcpyAsync(out_xyzi, v->dev.out, total * sizeof(float4), hipMemcpyDeviceToHost, v->stream));
    HC(hipMemcpyAsync(n_out, v->dev.n_out, (size_t)n_clouds * sizeof(int), hipMemcpyDeviceToHost, v->stream));
    std::vector<int> st(n_clouds);
    HC(hipMemcpyAsync(st.data(), v->dev.status, (size_t)n_clouds * sizeof(int), hipMemcpyDeviceToHost, v->stream));
    HC(hipStreamSynchronize(v->stream));
    if (status)
        for (int b = 0; b < n_clouds; b++) status[b] = st[b];
    return 0;
}

extern "C" int ll_voxel_counts(ll_voxel *v, int32_t n_clouds, int32_t *n_out, int32_t *status)
{
    if (!v || n_clouds < 1 || n_clouds > v->dev.max_clouds) return set_err("ll_voxel_counts", "bad argument");
    HC(hipSetDevice(v->device));
    HC(hipStreamSynchronize(v->stream));
    if (v->last_stream && v->last_stream != v->stream) HC(hipStreamSynchronize(v->last_stream));
    if (n_out) HC(hipMemcpy(n_out, v->dev.n_out, (size_t)n_clouds * sizeof(int), hipMemcpyDeviceToHost));
    if (status) HC(hipMemcpy(status, v->dev.status, (size_t)n_clouds * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}
