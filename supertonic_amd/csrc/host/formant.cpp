// formant.cpp — the formant correction's host arithmetic (formant.hpp) and its C entry points: stn_formant_plan, stn_formant_lpc.
// Host only: no device, no handle.
#include "formant.hpp"

#include <algorithm>
#include <cmath>

#include "../../../include/stn.h"
#include "pitch.hpp"

namespace stn {

std::string formant_plan(int hz, int64_t W, FormantPlan& f) {
    if (hz < 8000 || hz > 192000) return "formant: sample rate " + std::to_string(hz) + " Hz outside [8000, 192000]";
    if (W < 0 || W > ((int64_t)1 << 40)) return "formant: row length " + std::to_string(W) + " outside [0, 2^40]";
    f.H = pitch_hop(hz);
    f.p = std::min(FORMANT_MAX_ORDER, std::max(10, 2 * ((hz + 1999) / 2000) + 2));
    f.frames = (W + f.H - 1) / f.H + 1;
    return "";
}

std::vector<double> formant_lag_window(int hz, int p) {
    std::vector<double> w((size_t)p + 1);
    for (int k = 0; k <= p; ++k) {
        const double t = 2.0 * M_PI * 60.0 * (double)k / (double)hz;
        w[(size_t)k] = std::exp(-0.5 * t * t);
    }
    return w;
}

void formant_lpc(const double* r, const double* lagw, int p, double* a, double* err, double* refl) {
    double rc[FORMANT_MAX_ORDER + 1], t[FORMANT_MAX_ORDER + 1];
    rc[0] = 1.0001 * r[0] + 1e-9;
    for (int k = 1; k <= p; ++k) rc[k] = r[k] * lagw[k];
    a[0] = 1.0;
    for (int k = 1; k <= p; ++k) a[k] = 0.0;
    double E = rc[0];
    for (int i = 1; i <= p; ++i) {
        double acc = rc[i];
        for (int j = 1; j < i; ++j) acc += a[j] * rc[i - j];
        const double k = -acc / E;
        for (int j = 1; j < i; ++j) t[j] = a[j] + k * a[i - j];
        for (int j = 1; j < i; ++j) a[j] = t[j];
        a[i] = k;
        E *= 1.0 - k * k;
        if (refl) refl[i - 1] = k;
    }
    *err = E;
}

}  // namespace stn

extern "C" {

int stn_formant_plan(int hz, int64_t W, int* H, int* p, int64_t* frames, double* lag_or_null, size_t cap) {
    stn::FormantPlan f;
    if (!stn::formant_plan(hz, W, f).empty()) return STN_ERR_INVALID;
    if (H) *H = f.H;
    if (p) *p = f.p;
    if (frames) *frames = f.frames;
    if (lag_or_null) {
        const std::vector<double> w = stn::formant_lag_window(hz, f.p);
        for (size_t i = 0; i < w.size() && i < cap; ++i) lag_or_null[i] = w[i];
    }
    return STN_OK;
}

int stn_formant_lpc(int hz, const double* r, int p, double* a, double* err, double* refl_or_null) {
    if (hz < 8000 || hz > 192000 || !r || !a || !err || p < 1 || p > stn::FORMANT_MAX_ORDER) return STN_ERR_INVALID;
    const std::vector<double> w = stn::formant_lag_window(hz, p);
    stn::formant_lpc(r, w.data(), p, a, err, refl_or_null);
    return STN_OK;
}

}  // extern "C"
