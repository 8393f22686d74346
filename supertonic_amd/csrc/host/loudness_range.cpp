// loudness_range.cpp — stn_loudness_range_rule: maximum momentary loudness, maximum short-term loudness and loudness range (EBU Tech
// 3342) of one row from its 100 ms segment sums, in double and without a device.  It is the definition in include/stn.h "loudness
// range" written out; loudness_range_kernel's decisions are tested against it.
#include "loudness_range.hpp"

#include <algorithm>
#include <limits>
#include <vector>

#include "stn.h"

extern "C" {

int stn_loudness_range_rule(int hop, int64_t nseg, const double* seg, double* m_max, double* s_max, double* lra, int32_t* n_st) {
    using namespace stn;
    if (hop < 1 || nseg < 0 || (nseg > 0 && !seg)) return STN_ERR_INVALID;
    const double ninf = -std::numeric_limits<double>::infinity();
    double zm = -1.0, zs = -1.0;
    for (int64_t j = 0; j + LR_BLOCK <= nseg; ++j) zm = std::max(zm, lr_block_power(seg + j, hop));
    std::vector<double> z;
    for (int64_t j = 0; j + LR_WINDOW <= nseg; ++j) z.push_back(lr_window_power(seg + j, hop));
    double sum = 0.0;
    int64_t cnt = 0;
    for (double v : z) {
        zs = std::max(zs, v);
        if (lr_level(v) > LR_ABS_GATE) { sum += v; ++cnt; }
    }
    std::vector<double> kept;
    if (cnt > 0) {
        const double rel = lr_level(sum / (double)cnt) + LR_REL_GATE;
        for (double v : z) {
            const double l = lr_level(v);
            if (l > LR_ABS_GATE && l > rel) kept.push_back(v);
        }
    }
    std::sort(kept.begin(), kept.end());
    const int64_t n = (int64_t)kept.size();
    if (m_max) *m_max = zm < 0.0 ? ninf : lr_level(zm);
    if (s_max) *s_max = zs < 0.0 ? ninf : lr_level(zs);
    if (lra) *lra = n < 2 ? 0.0 : lr_level(kept[(size_t)lr_index(n, LR_HIGH)]) - lr_level(kept[(size_t)lr_index(n, LR_LOW)]);
    if (n_st) *n_st = (int32_t)n;
    return STN_OK;
}

}  // extern "C"
