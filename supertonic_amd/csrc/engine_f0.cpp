// engine_f0.cpp — the pitch report of a handle's finished batch and of host rows: the parameter and length checks (host/f0.hpp), the
// report's scratch and its two launches behind the output stage's rows.  The kernels are kernels_f0.hip; include/stn.h "f0" has the
// contract and DESIGN.md section 27 the decomposition.
#include "engine_internal.hpp"
#include "host/f0.hpp"

#include <algorithm>

namespace stn {

namespace {

stn_f0_params f0_params(const stn_f0_params* p) {
    stn_f0_params v;
    if (p) v = *p; else stn_f0_defaults(&v);
    return v;
}

// The longest row's frame count.  Refuses, before anything is uploaded or launched, a row of more frames than the report takes, and
// one of more than the caller's arrays hold.
int64_t f0_longest(const F0Geometry& g, const int64_t* n, size_t rows, int64_t cap, bool arrays) {
    if (cap < 0) throw std::invalid_argument("f0: cap must not be negative");
    int64_t m = 0;
    for (size_t r = 0; r < rows; ++r) {
        const int64_t F = f0_frames(g, n[r]);
        refuse(f0_frames_check((int64_t)r, F));
        if (arrays && F > cap)
            throw std::invalid_argument("f0: row " + std::to_string(r) + " holds " + std::to_string(F) + " frames, and the arrays given hold " +
                                        std::to_string(cap) + " per row");
        m = std::max(m, F);
    }
    return m;
}

}  // namespace

void Engine::f0_report(int hz, const stn_f0_params& p, const float* x, int64_t rows, int64_t W, const int64_t* n, const int64_t* nh, int64_t cap,
                       float* f0, float* ap, stn_f0_stats* stats) {
    const F0Geometry g = f0_geometry(hz, p);
    const int64_t maxF = f0_longest(g, nh, (size_t)rows, cap, f0 || ap);
    F0Launch l;
    l.k = g.k; l.hop = g.hop; l.tau_min = g.tau_min; l.tau_max = g.tau_max; l.threshold = p.threshold; l.ha = g.ha; l.gate_ms = g.gate_ms;
    const size_t nr = (size_t)rows, nf = nr * (size_t)maxF;
    Carve sz{nullptr};
    sz.take<float>(nf);
    sz.take<float>(nf);
    sz.take<stn_f0_stats>(nr);
    Carve c{f0_buf_.reserve(*this, sz.off)};
    float* df = c.take<float>(nf);
    float* da = c.take<float>(nf);
    stn_f0_stats* ds = c.take<stn_f0_stats>(nr);
    const double frames = (double)nf, T = (double)g.tau_max, samples = (double)rows * (double)W;
    if (maxF > 0) {  // (a span carries its events on a launch: none without one)
        StageSpan span(*this, "out", "f0", frames * T * (T + 1.0) * 3.0, samples * 4 + frames * 8);
        launch_f0_track(s_, x, rows, W, n, l, maxF, maxF, df, da);
    }
    STN_HIP(hipGetLastError());
    {
        StageSpan span(*this, "out", "f0", frames * 20.0, frames * 4 + (double)rows * 24);
        launch_f0_stats(s_, df, rows, W, n, l, maxF, maxF, ds);
    }
    STN_HIP(hipGetLastError());
    // the columns no frame of any row reaches are filled here; the kernel fills a shorter row's up to the longest row's count
    if (f0) std::fill(f0, f0 + nr * (size_t)cap, 0.0f);
    if (ap) std::fill(ap, ap + nr * (size_t)cap, 1.0f);
    if (maxF > 0) {
        if (f0) STN_HIP(hipMemcpy2DAsync(f0, (size_t)cap * 4, df, (size_t)maxF * 4, (size_t)maxF * 4, nr, hipMemcpyDeviceToHost, s_));
        if (ap) STN_HIP(hipMemcpy2DAsync(ap, (size_t)cap * 4, da, (size_t)maxF * 4, (size_t)maxF * 4, nr, hipMemcpyDeviceToHost, s_));
    }
    if (stats) STN_HIP(hipMemcpyAsync(stats, ds, nr * sizeof(stn_f0_stats), hipMemcpyDeviceToHost, s_));
}

int64_t Engine::batch_f0_frames(const stn_f0_params* pp) {
    const int64_t Wo = out_row_len();
    const int hz = output_rate();
    refuse(f0_check(hz, pp));
    const std::vector<int64_t> n = out_spans(Wo, hz);
    return f0_longest(f0_geometry(hz, f0_params(pp)), n.data(), n.size(), 0, false);
}

void Engine::batch_f0(const stn_f0_params* pp, int64_t cap, float* f0, float* ap, stn_f0_stats* stats) {
    const int64_t Wo = out_row_len();
    const int hz = output_rate();
    refuse(f0_check(hz, pp));
    const stn_f0_params p = f0_params(pp);
    {  // (the refusals come before the output stage runs)
        const std::vector<int64_t> n = out_spans(Wo, hz);
        (void)f0_longest(f0_geometry(hz, p), n.data(), n.size(), cap, f0 || ap);
    }
    const float* x = out_source(Wo);
    const BatchSpans& sp = batch_spans(hz, Wo);
    f0_report(hz, p, x, bt_.B, Wo, sp.dev.n, sp.host.data(), cap, f0, ap, stats);
    sync();
}

void Engine::op_f0(int hz, int rows, int W, const float* x, const int64_t* n, const stn_f0_params* pp, int64_t cap, float* f0, float* ap,
                   stn_f0_stats* stats) {
    OpScope op(*this);
    refuse(f0_check(hz, pp));
    const stn_f0_params p = f0_params(pp);
    const std::vector<int64_t> nn = spans("op_f0", rows, W, n);
    (void)f0_longest(f0_geometry(hz, p), nn.data(), nn.size(), cap, f0 || ap);  // (before the upload)
    const float* dx = op.up(x, (size_t)rows * (size_t)W);
    const int64_t* dn = op.spans(rows, W, nn).n;
    f0_report(hz, p, dx, rows, W, dn, nn.data(), cap, f0, ap, stats);
    sync();
}

}  // namespace stn
