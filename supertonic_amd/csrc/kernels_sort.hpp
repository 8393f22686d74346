// kernels_sort.hpp — the ascending bitonic sort of P keys in LDS (P a power of two) by one workgroup of kThreads, shared by
// loudness_range_kernel (kernels_loudness.hip: the short-term window powers) and f0_stats_kernel (kernels_f0.hip: the voiced frames).
// Every compare-exchange of a stage owns its two elements and the stages are separated by barriers: nothing depends on thread timing.
// The caller orders its own writes of key before the call (a barrier); the last stage's barrier orders the result before its reads.
#pragma once
#include <hip/hip_runtime.h>

namespace stn {

template <int kThreads, typename T>
__device__ __forceinline__ void lds_bitonic_sort(T* key, int P) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += kThreads) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const T a = key[i], b = key[p];
                if ((a > b) == ((i & k) == 0)) { key[i] = b; key[p] = a; }
            }
            __syncthreads();
        }
}

}  // namespace stn
