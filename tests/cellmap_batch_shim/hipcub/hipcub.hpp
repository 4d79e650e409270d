// Test-only stand-in for <hipcub/hipcub.hpp>: a stable sort of pairs by a bit range of the key, and an exclusive sum.
#pragma once
#include <numeric>
namespace hipcub {
struct DeviceRadixSort {
    template <typename K, typename V>
    static int SortPairs(void *tmp, size_t &bytes, const K *kin, K *kout, const V *vin, V *vout, int n, int b0 = 0, int b1 = sizeof(K) * 8, hipStream_t = nullptr)
    {
        if (!tmp) { bytes = 64; return 0; }
        std::vector<int> idx(n);
        std::iota(idx.begin(), idx.end(), 0);
        typedef unsigned long long U;
        const U mask = b1 - b0 >= 64 ? ~0ull : (((1ull << (b1 - b0)) - 1ull) << b0);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return ((U)kin[a] & mask) < ((U)kin[b] & mask); });
        for (int i = 0; i < n; i++) kout[i] = kin[idx[i]], vout[i] = vin[idx[i]];
        return 0;
    }
};
struct DeviceScan {
    template <typename T>
    static int ExclusiveSum(void *tmp, size_t &bytes, const T *in, T *out, int n, hipStream_t = nullptr)
    {
        if (!tmp) { bytes = 64; return 0; }
        T acc = 0;
        for (int i = 0; i < n; i++) { T v = in[i]; out[i] = acc; acc += v; }
        return 0;
    }
};
}
