// engine_expander.cpp — the fetch-time downward expander / noise gate of a handle: its limits, coefficients and static curve (host
// only), the scan tables and the scratch, the sequence of launches and the op-level entry.  The kernels are kernels_dynamics.hip; the
// hook is Engine::out_source (engine_batch.cpp); DESIGN.md section 25 has the contract.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace stn {

namespace {

// the fp32 values the kernels compute with (and the float64 reference is given): T, S = ratio - 1, K, R
ExpCoef static_coef(const stn_expander& c) {
    ExpCoef f{};
    f.T = c.threshold_db;
    f.S = (float)((double)c.ratio - 1.0);
    f.K = c.knee_db;
    f.R = c.range_db;
    return f;
}

}  // namespace

std::array<Lim, 7> limits(const stn_expander& c) {
    return {{{"threshold_db", c.threshold_db, -90.0f, -10.0f}, {"ratio", c.ratio, 1.0f, 20.0f},       {"knee_db", c.knee_db, 0.0f, 24.0f},
             {"range_db", c.range_db, 1.0f, 80.0f},            {"attack_ms", c.attack_ms, 0.1f, 300.0f}, {"hold_ms", c.hold_ms, 0.0f, 500.0f},
             {"release_ms", c.release_ms, 10.0f, 3000.0f}}};
}

std::string expander_check(const stn_expander* c) { return c ? range_check("expander", limits(*c)) : "expander: c is null"; }

double expander_curve(const stn_expander& c, double in_db) {
    const ExpCoef f = static_coef(c);
    const double T = f.T, S = f.S, K = f.K, d = T - in_db;
    double z;
    if (2.0 * d < -K) z = 0.0;
    else if (K > 0.0 && 2.0 * std::fabs(d) <= K) z = S * (d + 0.5 * K) * (d + 0.5 * K) / (2.0 * K);
    else z = S * d;
    return in_db - std::min(z, (double)f.R);
}

void expander_table(int hz, const stn_expander& c, ExpTable& t) {
    refuse(expander_check(&c));
    refuse(rate_check("expander", hz));
    t.hz = hz;
    t.coef = static_coef(c);
    t.coef.kA = (float)compressor_k(c.attack_ms, hz);
    // release_ms is the time a fully open gate takes to close through the whole range: delta dB per sample
    t.coef.delta = (float)((double)c.range_db * 1000.0 / ((double)c.release_ms * (double)hz));
    t.hold = (int64_t)std::floor((double)c.hold_ms * (double)hz / 1000.0 + 0.5);
    t.coef.Bh = (float)((double)t.coef.delta * (double)t.hold);
    // what i + 1 chunks of LO_CHUNK samples subtract from a start value of stage 1, and multiply one of stage 2 by, from the fp32
    // delta and k the kernels run on
    const double c1 = (double)LO_CHUNK * (double)t.coef.delta, E = std::pow(1.0 - (double)t.coef.kA, LO_CHUNK);
    t.pw.assign((size_t)2 * LO_SCAN, 0.0);
    double e = E;
    for (int i = 0; i < LO_SCAN; ++i) {
        t.pw[(size_t)i] = (double)(i + 1) * c1;
        t.pw[(size_t)LO_SCAN + i] = e;
        e *= E;
    }
}

void Engine::set_expander(bool on, const stn_expander* c) { dyn_set(xp_, on, c, on ? expander_check(c) : ""); }

Engine::XpScratch Engine::xp_layout(char* base, int64_t rows, int64_t W) {
    const size_t nc = (size_t)rows * (size_t)lo_chunks(W);
    Carve c{base};
    XpScratch sc{};
    sc.s1 = c.take<float>(nc);
    sc.s2 = c.take<float>(nc);
    sc.cmin = c.take<float>(nc);
    sc.ccnt = c.take<int32_t>(nc);
    sc.rmin = c.take<float>((size_t)rows);
    sc.rcnt = c.take<int64_t>((size_t)rows);
    sc.bytes = c.off;
    return sc;
}

void Engine::xp_enqueue(const ExpTable& t, const float* x, int64_t rows, int64_t W, const int64_t* n, const XpScratch& sc, float* y, float* open, XpProbe* probe) {
    // per sample: log10 (about 20), the gain computer (11), the detector (2), the clamp and the smoothing (3), the gain 10^x and its product (about 22)
    static constexpr DynSeq seq{"expander", "rows", {33.0, 36.0, 60.0}, {4, 8, 16}, 2, 8, 12};
    dyn_enqueue(seq, t, rows, W, sc, open ? 1 : 0, probe, nullptr,
                [&](int pass) { launch_expander_chunks(s_, pass, x, rows, W, n, t, sc.s1, sc.s2, y, open, sc.cmin, sc.ccnt); },
                [&] { launch_expander_rows(s_, rows, W, t, sc.cmin, sc.ccnt, sc.rmin, sc.rcnt); });
}

void Engine::xp_batch(const float* x, int64_t Wo, float* y) {
    dyn_batch(xp_, ST_EXPANDER, Wo, expander_table, xp_layout, [&](const XpScratch& sc, const RowSpans& n) { xp_enqueue(xp_.tab.t, x, bt_.B, Wo, n.n, sc, y, nullptr, nullptr); });
}

void Engine::batch_expander(float* min_attenuation_db, int64_t* closed_samples) {
    dyn_report(xp_, ST_EXPANDER, xp_layout, min_attenuation_db || closed_samples, [&](const XpScratch* sc) {
        read_rows(min_attenuation_db, sc ? sc->rmin : nullptr);
        read_rows(closed_samples, sc ? sc->rcnt : nullptr);
    });
}

void Engine::op_expander(int hz, int rows, int W, const float* x, const stn_expander& c, float* y, XpProbe* probe) {
    dyn_op(xp_, hz, rows, W, x, c, y, probe, expander_table, xp_layout, {probe ? probe->open : nullptr},
           [&](const ExpTable& t, const XpScratch& sc, RowSpans n, const float* dx, float* dy, float* const* tap) { xp_enqueue(t, dx, rows, W, n.n, sc, dy, tap[0], probe); });
}

}  // namespace stn
