// engine_deesser.cpp — the fetch-time de-esser of a handle: its limits, band and coefficients (host only), the tables and the scratch,
// the sequence of eight launches and the op-level entry.  The band's first two launches are the loudness measurement's
// (kernels_loudness.hip), the six behind them the shared sequence (Engine::dyn_enqueue) on kernels_dynamics.hip; the
// hook is Engine::out_source (engine_batch.cpp); DESIGN.md section 21 has the contract.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace stn {

namespace {

// the Butterworth pair's q: 1 / (2 cos(pi / 8)) and 1 / (2 cos(3 pi / 8)), as the fp32 values the contract names
constexpr float kQ[2] = {0.54119610f, 1.30656296f};

}  // namespace

void deesser_band(const stn_deesser& c, stn_filter f[2]) {
    for (int i = 0; i < 2; ++i) f[i] = stn_filter{STN_FILT_HIGHPASS, c.freq_hz, kQ[i], 0.0f};
}

std::array<Lim, 7> limits(const stn_deesser& c) {
    return {{{"freq_hz", c.freq_hz, 2000.0f, 12000.0f}, {"threshold_db", c.threshold_db, -60.0f, 0.0f}, {"ratio", c.ratio, 1.0f, 20.0f},
             {"knee_db", c.knee_db, 0.0f, 24.0f},       {"attack_ms", c.attack_ms, 0.1f, 300.0f},       {"release_ms", c.release_ms, 10.0f, 3000.0f},
             {"range_db", c.range_db, 1.0f, 24.0f}}};
}

std::string deesser_check(const stn_deesser* c, int rate_hz) {
    if (!c) return "deesser: c is null";
    const std::string out = range_check("deesser", limits(*c));
    if (!out.empty()) return out;
    if (c->mode != STN_DEESS_SPLIT && c->mode != STN_DEESS_WIDE) return "deesser: mode " + std::to_string(c->mode) + " is not STN_DEESS_SPLIT (0) or STN_DEESS_WIDE (1)";
    if (rate_hz <= 0) return "";  // (no model loaded yet: the corners are checked when the band is first designed)
    const std::string why = rate_check("deesser", rate_hz);
    if (!why.empty()) return why;
    // the chain's corners for a high-pass with q in [0.5, 1.5] (section 18), worded for this setting
    const double fr = c->freq_hz, rate = rate_hz;
    if (fr > 0.45 * rate) return "deesser: freq_hz " + num(fr) + " is above 0.45 x the output rate (" + num(0.45 * rate) + " Hz at " + std::to_string(rate_hz) + " Hz)";
    if (fr < rate / 2400) return "deesser: freq_hz " + num(fr) + " is below the output rate / 2400 (" + num(rate / 2400) + " Hz at " + std::to_string(rate_hz) + " Hz)";
    return "";
}

void deesser_table(int hz, const stn_deesser& c, DeessTable& t) {
    refuse(deesser_check(&c, hz));
    refuse(rate_check("deesser", hz));
    t.hz = hz;
    t.split = c.mode == STN_DEESS_SPLIT;
    // the band: one section pass of the chain, designed and rounded as stn_filter_coefs does
    stn_filter f[2];
    deesser_band(c, f);
    t.band = LoudTable{};
    t.band.hz = hz;
    t.band.hop = 1;  // (the measurement's launches want a table with a hop; nothing here reads it)
    for (int h = 0; h < 2; ++h) {
        double d[5];
        filter_design(f[h], hz, d);
        for (int j = 0; j < 5; ++j) t.band.coef.c[h * 5 + j] = (float)d[j];
    }
    cascade_powers(t.band.coef, t.band.mpow);
    // the detector: the compressor's T, S, K and k from the same fields, and the powers its scans read
    compressor_table(hz, stn_compressor{c.threshold_db, c.ratio, c.knee_db, c.attack_ms, c.release_ms, 0.0f}, t.det);
    t.coef.band = t.band.coef;
    t.coef.T = t.det.coef.T;
    t.coef.S = t.det.coef.S;
    t.coef.K = t.det.coef.K;
    t.coef.kA = t.det.coef.kA;
    t.coef.kR = t.det.coef.kR;
    t.coef.range = c.range_db;
}

void Engine::set_deesser(bool on, const stn_deesser* c) { dyn_set(ds_, on, c, on ? deesser_check(c, loaded_ ? output_rate() : 0) : ""); }

Engine::DsScratch Engine::ds_layout(char* base, int64_t rows, int64_t W) {
    const size_t nc = (size_t)rows * (size_t)lo_chunks(W);
    Carve c{base};
    DsScratch sc{};
    sc.st = c.take<float>(nc * 4);
    sc.pk = c.take<float>(nc);
    sc.s1 = c.take<float>(nc);
    sc.s2 = c.take<float>(nc);
    sc.cmax = c.take<float>(nc);
    sc.rmax = c.take<float>((size_t)rows);
    sc.bytes = c.off;
    return sc;
}

void Engine::ds_enqueue(const DeessTable& t, const float* x, int64_t rows, int64_t W, const RowSpans& n, const DsScratch& sc, float* y, DsProbe* probe,
                        float* band, float* gr) {
    const double samples = (double)rows * W, chunks = (double)rows * lo_chunks(W);
    const size_t nc = (size_t)rows * (size_t)lo_chunks(W);
    auto out = [&](float* dst, const float* src, size_t per) { if (dst) STN_HIP(hipMemcpyAsync(dst, src, nc * per * 4, hipMemcpyDeviceToHost, s_)); };
    // the band's state at every chunk's start: the first two launches of a section pass (section 18)
    StageSpan span(*this, "out", "deesser_band_chunks", 11.0 * samples, samples * 4 + chunks * 20);
    launch_loudness_chunks(s_, false, x, rows, W, n.full, t.band, sc.st, sc.pk, nullptr, nullptr);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->st_end, sc.st, 4);
    span.next("deesser_band_scan", chunks * 32.0 * 11, chunks * 32);
    launch_loudness_scan(s_, rows, W, n.full, t.band, sc.st);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->st_start, sc.st, 4);
    // per sample: the two sections (11), log10 (about 20), the gain computer and its cap (9), the detector (3), the smoothing (2), the
    // gain 10^x and its use (about 23)
    static constexpr DynSeq seq{"deesser", "rowmax", {43.0, 45.0, 68.0}, {20, 24, 28}, 1, 4, 4};
    dyn_enqueue(seq, t.det, rows, W, sc, (band ? 1 : 0) + (gr ? 1 : 0), probe, &span,
                [&](int pass) { launch_deesser_chunks(s_, pass, x, rows, W, n.n, t, sc.st, sc.s1, sc.s2, y, band, gr, sc.cmax); },
                [&] { launch_compressor_rowmax(s_, rows, W, sc.cmax, sc.rmax); });
}

void Engine::ds_batch(const float* x, int64_t Wo, float* y) {
    dyn_batch(ds_, ST_DEESSER, Wo, deesser_table, ds_layout, [&](const DsScratch& sc, const RowSpans& n) { ds_enqueue(ds_.tab.t, x, bt_.B, Wo, n, sc, y, nullptr, nullptr, nullptr); });
}

void Engine::batch_deesser(float* max_reduction_db) {
    dyn_report(ds_, ST_DEESSER, ds_layout, max_reduction_db != nullptr, [&](const DsScratch* sc) { read_rows(max_reduction_db, sc ? sc->rmax : nullptr); });
}

void Engine::op_deesser(int hz, int rows, int W, const float* x, const stn_deesser& c, float* y, DsProbe* probe) {
    dyn_op(ds_, hz, rows, W, x, c, y, probe, deesser_table, ds_layout, {probe ? probe->band : nullptr, probe ? probe->gr : nullptr},
           [&](const DeessTable& t, const DsScratch& sc, RowSpans n, const float* dx, float* dy, float* const* tap) { ds_enqueue(t, dx, rows, W, n, sc, dy, probe, tap[0], tap[1]); });
}

}  // namespace stn
