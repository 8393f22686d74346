// loudness_range.hpp — the arithmetic of the loudness report (include/stn.h "loudness range") that the host rule
// (stn_loudness_range_rule, loudness_range.cpp) and the kernel (loudness_range_kernel, kernels_loudness.hip) share: a block's and a
// window's power from a row's 100 ms segment sums, the level of a power, the index of an order statistic.  Double throughout; every sum
// in the order written here.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define STN_LR_HD __host__ __device__
#else
#define STN_LR_HD
#endif

namespace stn {

constexpr int LR_BLOCK = 4;    // segments of a 400 ms momentary block
constexpr int LR_WINDOW = 30;  // segments of a 3 s short-term window
constexpr double LR_ABS_GATE = -70.0, LR_REL_GATE = -20.0, LR_LOW = 0.10, LR_HIGH = 0.95;

// mean square of block j (seg points at its first segment): the integrated measurement's block, sum and all
STN_LR_HD inline double lr_block_power(const double* seg, int hop) {
    return ((seg[0] + seg[1]) + (seg[2] + seg[3])) * (1.0 / (4.0 * hop));
}

// mean square of window j (seg points at its first segment): the 30 segments added left to right
STN_LR_HD inline double lr_window_power(const double* seg, int hop) {
    double a = seg[0];
    for (int i = 1; i < LR_WINDOW; ++i) a += seg[i];
    return a / (30.0 * hop);
}

STN_LR_HD inline double lr_level(double z) { return -0.691 + 10.0 * log10(z); }

// EBU Tech 3342's reference code: the q-quantile of n ascending values is element floor((n - 1) q + 0.5)
STN_LR_HD inline int64_t lr_index(int64_t n, double q) { return (int64_t)((double)(n - 1) * q + 0.5); }

}  // namespace stn
