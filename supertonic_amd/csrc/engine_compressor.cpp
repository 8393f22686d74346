// engine_compressor.cpp — the fetch-time dynamic range compressor of a handle: its limits, coefficients and static curve (host only),
// the scan tables and the scratch, the sequence of launches and the op-level entry.  The kernels are kernels_dynamics.hip; the hook
// is Engine::out_source (engine_batch.cpp); DESIGN.md section 20 has the contract.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace stn {

namespace {

// the fp32 values the kernels compute with (and the float64 reference is given): T, S = 1 / ratio - 1, K, makeup
CompCoef static_coef(const stn_compressor& c) {
    CompCoef f{};
    f.T = c.threshold_db;
    f.S = (float)(1.0 / (double)c.ratio - 1.0);
    f.K = c.knee_db;
    f.makeup = c.makeup_db;
    return f;
}

}  // namespace

std::array<Lim, 6> limits(const stn_compressor& c) {
    return {{{"threshold_db", c.threshold_db, -60.0f, 0.0f}, {"ratio", c.ratio, 1.0f, 20.0f},       {"knee_db", c.knee_db, 0.0f, 24.0f},
             {"attack_ms", c.attack_ms, 0.1f, 300.0f},       {"release_ms", c.release_ms, 10.0f, 3000.0f}, {"makeup_db", c.makeup_db, -12.0f, 24.0f}}};
}

std::string compressor_check(const stn_compressor* c) { return c ? range_check("compressor", limits(*c)) : "compressor: c is null"; }

double compressor_k(float ms, int rate_hz) { return -std::expm1(-1000.0 / ((double)ms * (double)rate_hz)); }

double compressor_curve(const stn_compressor& c, double in_db) {
    const CompCoef f = static_coef(c);
    const double T = f.T, S = f.S, K = f.K, d = in_db - T;
    double z;
    if (2.0 * d < -K) z = 0.0;
    else if (K > 0.0 && 2.0 * std::fabs(d) <= K) z = -S * (d + 0.5 * K) * (d + 0.5 * K) / (2.0 * K);
    else z = -S * d;
    return in_db - z + (double)f.makeup;
}

void compressor_table(int hz, const stn_compressor& c, CompTable& t) {
    refuse(compressor_check(&c));
    refuse(rate_check("compressor", hz));
    t.hz = hz;
    t.coef = static_coef(c);
    t.coef.kA = (float)compressor_k(c.attack_ms, hz);
    t.coef.kR = (float)compressor_k(c.release_ms, hz);
    // what a chunk of LO_CHUNK samples multiplies a start value by, from the fp32 k the kernels run on, and its powers
    const double D = std::pow(1.0 - (double)t.coef.kR, LO_CHUNK), E = std::pow(1.0 - (double)t.coef.kA, LO_CHUNK);
    t.pw.assign((size_t)2 * LO_SCAN, 0.0);
    double d = D, e = E;
    for (int i = 0; i < LO_SCAN; ++i) {
        t.pw[(size_t)i] = d;
        t.pw[(size_t)LO_SCAN + i] = e;
        d *= D;
        e *= E;
    }
}

void Engine::set_compressor(bool on, const stn_compressor* c) { dyn_set(cp_, on, c, on ? compressor_check(c) : ""); }

Engine::CpScratch Engine::cp_layout(char* base, int64_t rows, int64_t W) {
    const size_t nc = (size_t)rows * (size_t)lo_chunks(W);
    Carve c{base};
    CpScratch sc{};
    sc.s1 = c.take<float>(nc);
    sc.s2 = c.take<float>(nc);
    sc.cmax = c.take<float>(nc);
    sc.rmax = c.take<float>((size_t)rows);
    sc.bytes = c.off;
    return sc;
}

void Engine::cp_enqueue(const CompTable& t, const float* x, int64_t rows, int64_t W, const int64_t* n, const CpScratch& sc, float* y, float* gr, CpProbe* probe) {
    // per sample: log10 (about 20), the gain computer (8), the detector (3), the smoothing (2), the gain 10^x and its product (about 22)
    static constexpr DynSeq seq{"compressor", "rowmax", {31.0, 33.0, 56.0}, {4, 8, 12}, 1, 4, 4};
    dyn_enqueue(seq, t, rows, W, sc, gr ? 1 : 0, probe, nullptr,
                [&](int pass) { launch_compressor_chunks(s_, pass, x, rows, W, n, t, sc.s1, sc.s2, y, gr, sc.cmax); },
                [&] { launch_compressor_rowmax(s_, rows, W, sc.cmax, sc.rmax); });
}

void Engine::cp_batch(const float* x, int64_t Wo, float* y) {
    dyn_batch(cp_, ST_COMPRESSOR, Wo, compressor_table, cp_layout, [&](const CpScratch& sc, const RowSpans& n) { cp_enqueue(cp_.tab.t, x, bt_.B, Wo, n.n, sc, y, nullptr, nullptr); });
}

void Engine::batch_compressor(float* max_reduction_db) {
    dyn_report(cp_, ST_COMPRESSOR, cp_layout, max_reduction_db != nullptr, [&](const CpScratch* sc) { read_rows(max_reduction_db, sc ? sc->rmax : nullptr); });
}

void Engine::op_compressor(int hz, int rows, int W, const float* x, const stn_compressor& c, float* y, CpProbe* probe) {
    dyn_op(cp_, hz, rows, W, x, c, y, probe, compressor_table, cp_layout, {probe ? probe->gr : nullptr},
           [&](const CompTable& t, const CpScratch& sc, RowSpans n, const float* dx, float* dy, float* const* tap) { cp_enqueue(t, dx, rows, W, n.n, sc, dy, tap[0], probe); });
}

}  // namespace stn
