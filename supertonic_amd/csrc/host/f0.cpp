// f0.cpp — the pitch report's host arithmetic (f0.hpp) and its C entry points: stn_f0_defaults, stn_f0_error, stn_f0_plan, stn_f0_rule,
// stn_f0_rule_lags and stn_f0_stats_rule.  Host only: no device, no handle.  stn_f0_rule is the definition in include/stn.h "f0" written
// out in double (the direct squared difference, every sum left to right); the kernels (kernels_f0.hip) are tested against it.
#include "f0.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace stn {

std::string f0_check(int hz, const stn_f0_params* pp) {
    if (hz < F0_MIN_HZ || hz > F0_MAX_HZ)
        return "f0: sample rate must be in [" + std::to_string(F0_MIN_HZ) + ", " + std::to_string(F0_MAX_HZ) + "] Hz (got " + std::to_string(hz) + ")";
    stn_f0_params p;
    if (pp) p = *pp; else stn_f0_defaults(&p);
    if (!(p.fmin_hz >= 30.0f && p.fmin_hz < p.fmax_hz && p.fmax_hz <= 1000.0f))
        return "f0 range [" + std::to_string(p.fmin_hz) + ", " + std::to_string(p.fmax_hz) + "] Hz: must satisfy 30 <= fmin < fmax <= 1000";
    if (!(p.threshold > 0.0f && p.threshold < 1.0f)) return "f0 threshold " + std::to_string(p.threshold) + ": must be inside (0, 1)";
    if (!(p.gate_db >= -120.0f && p.gate_db <= 0.0f)) return "f0 gate " + std::to_string(p.gate_db) + " dB: must be in [-120, 0]";
    const F0Geometry g = f0_geometry(hz, p);
    if (g.tau_min < 2)
        return "f0 fmax " + std::to_string(p.fmax_hz) + " Hz at " + std::to_string(hz) + " Hz: the shortest lag is " + std::to_string(g.tau_min) +
               " analysis samples, and the refinement needs at least 2";
    return "";
}

F0Geometry f0_geometry(int hz, const stn_f0_params& p) {
    F0Geometry g;
    g.k = std::max(1, hz / 16000);
    g.ha = (double)hz / (double)g.k;
    g.hop = (int)std::floor(g.ha / 100.0 + 0.5);
    g.tau_max = (int)std::ceil(g.ha / (double)p.fmin_hz);
    g.tau_min = (int)std::floor(g.ha / (double)p.fmax_hz);
    g.gate_ms = std::pow(10.0, (double)p.gate_db / 10.0);
    return g;
}

namespace {

// One frame of the definition: w points at the frame's 2 tau_max analysis samples.  Returns the chosen lag (0: unvoiced) and fills
// f0 / ap; dp is scratch of tau_max + 1.
int f0_frame(const double* w, const F0Geometry& g, double threshold, std::vector<double>& dp, double& f0, double& ap) {
    const int T = g.tau_max;
    f0 = 0.0;
    ap = 1.0;
    double e = 0.0;
    for (int j = 0; j < T; ++j) e += w[j] * w[j];
    if (e / (double)T < g.gate_ms) return 0;
    dp[0] = 1.0;
    double run = 0.0;
    for (int tau = 1; tau <= T; ++tau) {
        double d = 0.0;
        for (int j = 0; j < T; ++j) { const double v = w[j] - w[j + tau]; d += v * v; }
        run += d;
        dp[(size_t)tau] = run > 0.0 ? d * (double)tau / run : 1.0;
    }
    int lag = 0;
    for (int tau = g.tau_min; tau < T; ++tau)
        if (dp[(size_t)tau] < threshold) { lag = tau; break; }
    if (!lag) return 0;
    while (lag + 1 < T && dp[(size_t)lag + 1] < dp[(size_t)lag]) ++lag;
    const double a = dp[(size_t)lag - 1], b = dp[(size_t)lag], c = dp[(size_t)lag + 1], den = a - 2.0 * b + c;
    double off = 0.0;
    if (den > 0.0) off = std::min(1.0, std::max(-1.0, 0.5 * (a - c) / den));
    f0 = g.ha / ((double)lag + off);
    ap = b;
    return lag;
}

int f0_rule(int hz, int64_t n, const float* x, const stn_f0_params* pp, int64_t cap, double* f0, double* ap, int32_t* lags, int64_t* frames) {
    if (n < 0 || (n > 0 && !x) || cap < 0 || !f0_check(hz, pp).empty()) return STN_ERR_INVALID;
    stn_f0_params p;
    if (pp) p = *pp; else stn_f0_defaults(&p);
    const F0Geometry g = f0_geometry(hz, p);
    const int64_t F = f0_frames(g, n);
    if (frames) *frames = F;
    if (F > cap && (f0 || ap || lags)) return STN_ERR_INVALID;
    const int64_t na = n / g.k;
    std::vector<double> u((size_t)na), dp((size_t)g.tau_max + 1);
    for (int64_t j = 0; j < na; ++j) {
        double a = 0.0;
        for (int i = 0; i < g.k; ++i) a += (double)x[j * g.k + i];
        u[(size_t)j] = a / (double)g.k;
    }
    for (int64_t t = 0; t < F; ++t) {
        double f = 0.0, a = 1.0;
        const int lag = f0_frame(u.data() + t * g.hop, g, (double)p.threshold, dp, f, a);
        if (f0) f0[t] = f;
        if (ap) ap[t] = a;
        if (lags) lags[t] = lag;
    }
    return STN_OK;
}

}  // namespace
}  // namespace stn

extern "C" {

void stn_f0_defaults(stn_f0_params* p) {
    if (!p) return;
    p->fmin_hz = 60.0f;
    p->fmax_hz = 500.0f;
    p->threshold = 0.15f;
    p->gate_db = -60.0f;
}

const char* stn_f0_error(int hz, const stn_f0_params* params_or_null) {
    static thread_local std::string why;
    why = stn::f0_check(hz, params_or_null);
    return why.c_str();
}

int stn_f0_plan(int hz, int64_t n, const stn_f0_params* params_or_null, int* k, int* hop, int* tau_min, int* tau_max, int64_t* frames) {
    if (n < 0 || !stn::f0_check(hz, params_or_null).empty()) return STN_ERR_INVALID;
    stn_f0_params p;
    if (params_or_null) p = *params_or_null; else stn_f0_defaults(&p);
    const stn::F0Geometry g = stn::f0_geometry(hz, p);
    if (k) *k = g.k;
    if (hop) *hop = g.hop;
    if (tau_min) *tau_min = g.tau_min;
    if (tau_max) *tau_max = g.tau_max;
    if (frames) *frames = stn::f0_frames(g, n);
    return STN_OK;
}

int stn_f0_rule(int hz, int64_t n, const float* x, const stn_f0_params* params_or_null, int64_t cap, double* f0, double* ap, int64_t* frames) {
    return stn::f0_rule(hz, n, x, params_or_null, cap, f0, ap, nullptr, frames);
}

int stn_f0_rule_lags(int hz, int64_t n, const float* x, const stn_f0_params* params_or_null, int64_t cap, int32_t* lag, int64_t* frames) {
    return stn::f0_rule(hz, n, x, params_or_null, cap, nullptr, nullptr, lag, frames);
}

int stn_f0_stats_rule(const float* f0, int64_t frames, stn_f0_stats* out) {
    if (frames < 0 || (frames > 0 && !f0) || !out || frames > INT32_MAX) return STN_ERR_INVALID;
    std::vector<float> v;
    double lg = 0.0;
    for (int64_t t = 0; t < frames; ++t)
        if (f0[t] > 0.0f) { v.push_back(f0[t]); lg += std::log2((double)f0[t]); }
    std::sort(v.begin(), v.end());
    out->frames = (int32_t)frames;
    out->voiced = (int32_t)v.size();
    out->median_hz = out->mean_hz = out->min_hz = out->max_hz = 0.0f;
    if (!v.empty()) {
        out->median_hz = v[(v.size() - 1) / 2];
        out->mean_hz = (float)std::exp2(lg / (double)v.size());
        out->min_hz = v.front();
        out->max_hz = v.back();
    }
    return STN_OK;
}

}  // extern "C"
