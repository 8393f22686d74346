// pitch.cpp — the pitch shift's host arithmetic (pitch.hpp) and its C entry points: stn_pitch_ratio, stn_pitch_error, stn_pitch_plan,
// stn_pitch_window.  Host only: no device, no handle.
#include "pitch.hpp"

#include <cmath>

#include "../../../include/stn.h"

namespace stn {

std::string pitch_check(float semitones) {
    if (std::isfinite(semitones) && semitones >= -12.0f && semitones <= 12.0f) return "";
    return "pitch " + (std::isfinite(semitones) ? std::to_string(semitones) : std::string(std::isnan(semitones) ? "nan" : (semitones > 0 ? "inf" : "-inf"))) +
           " semitones: must be a finite number in [-12, 12] (0: off)";
}

bool pitch_ratio(float semitones, int& a, int& b) {
    if (!pitch_check(semitones).empty()) return false;
    const double r = std::pow(2.0, (double)semitones / 12.0);
    double best = INFINITY;
    for (int d = 1; d <= PITCH_MAX_TERM; ++d) {
        // the two numerators around r d: nothing else over this denominator can be closer
        const int lo = (int)std::floor(r * d);
        for (int n = lo; n <= lo + 1; ++n) {
            if (n < 1 || n > PITCH_MAX_TERM) continue;
            const double q = (double)n / (double)d, e = q > r ? q / r : r / q;
            if (e < best) { best = e; a = n; b = d; }  // (strictly: a tie stays with the smaller denominator)
        }
    }
    return true;
}

int pitch_hop(int hz) {
    int H = 1;
    while ((int64_t)128 * H < hz) H *= 2;
    return H;
}

std::string pitch_plan(int hz, int64_t W, int a, int b, PitchPlan& p) {
    if (hz < 8000 || hz > 192000) return "pitch: sample rate " + std::to_string(hz) + " Hz outside [8000, 192000]";
    if (W < 0 || W > ((int64_t)1 << 40)) return "pitch: row length " + std::to_string(W) + " outside [0, 2^40]";
    if (a < 1 || a > PITCH_MAX_TERM || b < 1 || b > PITCH_MAX_TERM)
        return "pitch: ratio " + std::to_string(a) + "/" + std::to_string(b) + ": both terms must be in [1, " + std::to_string(PITCH_MAX_TERM) + "]";
    p.H = pitch_hop(hz);
    p.delta = 3 * p.H / 4;
    p.Ws = (W * a + b - 1) / b;
    p.M = p.Ws / p.H + 2;
    return "";
}

std::vector<float> pitch_window(int hz) {
    const int N = 2 * pitch_hop(hz);
    std::vector<float> w((size_t)N);
    for (int i = 0; i < N; ++i) w[(size_t)i] = (float)(0.5 * (1.0 - std::cos(2.0 * M_PI * (double)i / (double)N)));
    return w;
}

}  // namespace stn

extern "C" {

int stn_pitch_ratio(float semitones, int* a, int* b) {
    int n = 1, d = 1;
    if (!stn::pitch_ratio(semitones, n, d)) return STN_ERR_INVALID;
    if (a) *a = n;
    if (b) *b = d;
    return STN_OK;
}

const char* stn_pitch_error(float semitones) {
    static thread_local std::string why;
    why = stn::pitch_check(semitones);
    return why.c_str();
}

int stn_pitch_plan(int hz, int64_t W, int a, int b, int* H, int* delta, int64_t* M, int64_t* Ws) {
    stn::PitchPlan p;
    if (!stn::pitch_plan(hz, W, a, b, p).empty()) return STN_ERR_INVALID;
    if (H) *H = p.H;
    if (delta) *delta = p.delta;
    if (M) *M = p.M;
    if (Ws) *Ws = p.Ws;
    return STN_OK;
}

int stn_pitch_window(int hz, float* w, size_t cap, int* n) {
    if (hz < 8000 || hz > 192000) return STN_ERR_INVALID;
    const std::vector<float> v = stn::pitch_window(hz);
    if (n) *n = (int)v.size();
    if (w) for (size_t i = 0; i < v.size() && i < cap; ++i) w[i] = v[i];
    return STN_OK;
}

}  // extern "C"
