// pause_plan.cpp — see pause_plan.hpp.
#include "pause_plan.hpp"

#include <algorithm>
#include <cmath>

#include "../../../include/stn.h"

namespace stn {

std::string pause_check(float max_pause_ms) {
    if (!(max_pause_ms >= 20.0f && max_pause_ms <= 5000.0f)) return "pause limit " + std::to_string(max_pause_ms) + " ms: must be in [20, 5000]";
    return "";
}

int64_t pause_samples(int hz, float max_pause_ms) { return (int64_t)((double)max_pause_ms * (double)hz / 1000.0 + 0.5); }

int pause_stride(int64_t W, int hz, int64_t Mp) {
    const int64_t F = (hz + 50) / 100;
    const int64_t K = (W + F - 1) / F;
    const int64_t pf = Mp / F + 1;  // frames of the shortest pause that is cut: P = pf F > Mp
    // active, (pf inactive, active) per cut
    const int64_t cuts = K > 0 ? (K - 1) / (pf + 1) : 0;
    return (int)std::min<int64_t>(cuts, PAUSE_MAX_CUTS) + 1;
}

PausePlan pause_plan(int hz, int64_t n, const double* level, int64_t K, double top_db, int64_t keep, int64_t Mp) {
    const int64_t F = (hz + 50) / 100;
    PausePlan p;
    p.start = 0; p.end = n; p.len = n;
    double mx = 0.0;
    for (int64_t k = 0; k < K; ++k) mx = std::fmax(mx, level[k]);
    if (!(n > 0 && mx > 1e-7)) return p;  // no speech: untouched
    const double thr = mx * std::pow(10.0, -top_db / 10.0);
    int64_t f0 = K, f1 = -1;
    for (int64_t k = 0; k < K; ++k)
        if (level[k] >= thr) {
            if (k < f0) f0 = k;
            f1 = k;
        }
    if (f1 < f0) return p;
    p.start = std::max<int64_t>(0, f0 * F - keep);
    p.end = std::min<int64_t>(n, (f1 + 1) * F + keep);
    const int64_t hr = Mp / 2, hl = Mp - hr;
    int64_t dropped = 0, last = f0;  // last: the last active frame seen
    for (int64_t b = f0 + 1; b <= f1; ++b) {
        if (!(level[b] >= thr)) continue;
        const int64_t a = last + 1;  // frames a .. b - 1 are inactive between two active ones
        last = b;
        const int64_t P = (b - a) * F;
        if (P > Mp && (int)p.cuts.size() < PAUSE_MAX_CUTS) {
            p.cuts.push_back({a * F + hl, b * F - hr});
            dropped += P - Mp;
        }
    }
    p.len = p.end - p.start - dropped;
    return p;
}

std::vector<PausePiece> pause_pieces(int64_t start, int64_t end, int64_t n, const int64_t* cuts, int m, int64_t fd) {
    std::vector<PausePiece> v((size_t)m + 1);
    int64_t at = 0;
    for (int j = 0; j <= m; ++j) {
        const int64_t src = j == 0 ? start : cuts[2 * (j - 1) + 1], stop = j == m ? end : cuts[2 * j];
        const int64_t len = stop - src, fl = std::min(fd, len);
        v[(size_t)j] = {at, len, src, (j > 0 || start > 0) ? (int32_t)fl : 0, (j < m || end < n) ? (int32_t)fl : 0};
        at += len;
    }
    return v;
}

}  // namespace stn

static thread_local std::string g_pause_err;

extern "C" {

const char* stn_pause_plan_error(void) { return g_pause_err.c_str(); }

int stn_pause_plan(int hz, int64_t n, const double* level, int64_t K, float top_db, float keep_ms, float max_pause_ms, int64_t* start, int64_t* end,
                   int64_t* cuts, int cap_pairs, int32_t* n_cuts) {
    try {
        g_pause_err.clear();
        const int64_t F = ((int64_t)hz + 50) / 100;
        if (hz < 8000 || hz > 192000) g_pause_err = "pause plan: rate " + std::to_string(hz) + " Hz outside [8000, 192000]";
        else if (n < 0 || K != (n + F - 1) / F) g_pause_err = "pause plan: K must be ceil(n / F) frames of F = " + std::to_string(F) + " samples, n >= 0";
        else if (K > 0 && !level) g_pause_err = "pause plan: level is null";
        else if (!(top_db >= 1.0f && top_db <= 120.0f)) g_pause_err = "pause plan: top_db " + std::to_string(top_db) + " dB: must be in [1, 120]";
        else if (!(keep_ms >= 0.0f && keep_ms <= 1000.0f)) g_pause_err = "pause plan: keep " + std::to_string(keep_ms) + " ms: must be in [0, 1000]";
        else if (cap_pairs < 0 || (cap_pairs > 0 && !cuts)) g_pause_err = "pause plan: cap_pairs without cuts";
        else g_pause_err = stn::pause_check(max_pause_ms);
        if (!g_pause_err.empty()) return STN_ERR_INVALID;
        const int64_t keep = (int64_t)((double)keep_ms * (double)hz / 1000.0 + 0.5);
        const stn::PausePlan p = stn::pause_plan(hz, n, level, K, (double)top_db, keep, stn::pause_samples(hz, max_pause_ms));
        if (start) *start = p.start;
        if (end) *end = p.end;
        if (n_cuts) *n_cuts = (int32_t)p.cuts.size();
        for (size_t c = 0; c < p.cuts.size() && c < (size_t)cap_pairs; ++c) {
            cuts[2 * c] = p.cuts[c].lo;
            cuts[2 * c + 1] = p.cuts[c].hi;
        }
        return STN_OK;
    } catch (const std::exception& e) {
        g_pause_err = e.what();
        return STN_ERR_INVALID;
    }
}

}  // extern "C"
