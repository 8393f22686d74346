// f0.hpp — the geometry of the pitch report (include/stn.h "f0") that the host rule (stn_f0_rule, f0.cpp), the
// engine (engine_f0.cpp) and the kernels' launcher (kernels_f0.hip) share: the decimation, the hop, the lag range and the frame count
// of a span, and the parameter limits with their messages.  Host only; double throughout.
#pragma once
#include <cstdint>
#include <string>

#include "stn.h"

namespace stn {

constexpr int F0_MIN_HZ = 8000, F0_MAX_HZ = 192000;  // the rates of the output stage

// What a rate and a parameter set fix: the box average's length k, the analysis rate ha = hz / k (below 32000), the hop in analysis
// samples, the lag range [tau_min, tau_max) of the search (the difference function runs to tau_max itself), the gate as a mean square
struct F0Geometry {
    int k = 1, hop = 0, tau_min = 0, tau_max = 0;
    double ha = 0.0, gate_ms = 0.0;
};

// why (hz, p) is refused, or "" (p null: the defaults)
std::string f0_check(int hz, const stn_f0_params* p);
// the geometry of a checked (hz, p)
F0Geometry f0_geometry(int hz, const stn_f0_params& p);
// whole frames inside a span of n samples
inline int64_t f0_frames(const F0Geometry& g, int64_t n) {
    const int64_t na = n / g.k;
    return na < 2 * (int64_t)g.tau_max ? 0 : (na - 2 * (int64_t)g.tau_max) / g.hop + 1;
}

}  // namespace stn
