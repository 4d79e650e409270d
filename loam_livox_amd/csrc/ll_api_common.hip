// ll_api_common.hip -- what every handle of the C ABI declared in include/loam_livox_hip.h reports through: the error text, the
// version, the hardware-queue hint.  The host layer (ll_api_*.hip, ll_spin_api.hip) owns device memory, HIP streams and launch order;
// all arithmetic of the hot path runs in the *_kernels.hip files.  There is no CPU fallback: every entry point fails with an error
// string when HIP reports no usable device.
#include "ll_api_internal.h"

thread_local std::string ll::g_err;
int ll::set_err(const char *where, const char *what)
{
    g_err = std::string(where) + ": " + what;
    return -1;
}
int ll::check_device(int device)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return set_err("hipGetDeviceCount", "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= count) return set_err("device", "ordinal out of range");
    HC(hipSetDevice(device));
    return 0;
}

extern "C" const char *ll_last_error(void) { return g_err.c_str(); }
extern "C" const char *ll_version(void) { return "loam_livox_hip 0.1 (gfx950)"; }

extern "C" int ll_runtime_hint_hw_queues(int32_t n)
{
    if (n < 1 || n > 64) return set_err("ll_runtime_hint_hw_queues", "n must be in 1 .. 64");
    if (getenv("GPU_MAX_HW_QUEUES")) return 0;  // the caller's environment wins
    char buf[16];
    snprintf(buf, sizeof(buf), "%d", (int)n);
    if (setenv("GPU_MAX_HW_QUEUES", buf, 0) != 0) return set_err("ll_runtime_hint_hw_queues", "setenv failed");
    return 1;
}
