// engine_limiter.cpp — the look-ahead peak limiter behind the loudness gain: the setting, the Hann weights (host only), the fetch
// scratch that holds the limited fp32 rows, and the step the output stage (engine_batch.cpp) and batch_limiter share.  The kernels are
// kernels_limiter.hip; DESIGN.md section 15 has the contract.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>

namespace stn {

std::string limiter_check(int hz, float lookahead_ms) {
    if (!(lookahead_ms >= 0.5f && lookahead_ms <= 10.0f)) return "limiter look-ahead " + std::to_string(lookahead_ms) + " ms: must be in [0.5, 10]";
    return rate_check("limiter", hz);
}
int64_t limiter_samples(int hz, float lookahead_ms) { return (int64_t)((double)lookahead_ms * (double)hz / 1000.0 + 0.5); }

std::vector<float> limiter_window(int hz, float lookahead_ms) {
    const int64_t A = limiter_samples(hz, lookahead_ms);
    std::vector<double> h((size_t)A + 1);
    double sum = 0.0;
    for (int64_t k = 0; k <= A; ++k) {
        h[(size_t)k] = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)(k + 1) / (double)(A + 2));
        sum += h[(size_t)k];
    }
    std::vector<float> w((size_t)A + 1);
    for (int64_t k = 0; k <= A; ++k) w[(size_t)k] = (float)(h[(size_t)k] / sum);
    return w;
}

void Engine::set_limiter(bool on, float lookahead_ms) {
    refuse(limiter_check(LO_MIN_HZ, lookahead_ms));  // (the rate is the fetch's: checked there)
    lm_on_ = on;
    lm_ms_ = lookahead_ms;
}

void Engine::get_limiter(int* on, float* lookahead_ms) const {
    if (on) *on = lm_on_ ? 1 : 0;
    if (lookahead_ms) *lookahead_ms = lm_ms_;
}

// uploaded once per (rate, look-ahead)
const float* Engine::lm_window(int hz) {
    if (lm_win_.get() && lm_win_hz_ == hz && lm_win_ms_ == lm_ms_) return static_cast<const float*>(lm_win_.get());
    refuse(limiter_check(hz, lm_ms_));
    const std::vector<float> w = limiter_window(hz, lm_ms_);
    float* d = reinterpret_cast<float*>(lm_win_.reserve(*this, w.size() * sizeof(float)));
    sync();  // a fetch may still be reading the old weights
    STN_HIP(hipMemcpy(d, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    lm_win_hz_ = hz; lm_win_ms_ = lm_ms_;
    return d;
}

Engine::LmScratch Engine::lm_layout(char* base, int64_t rows, int64_t W) {
    const size_t nt = (size_t)rows * (size_t)lm_tiles(W);
    Carve c{base};
    LmScratch sc{};
    sc.y = c.take<float>((size_t)rows * (size_t)W);
    sc.pcnt = c.take<int>(nt);
    sc.pmin = c.take<float>(nt);
    sc.limited = c.take<int64_t>((size_t)rows);
    sc.red = c.take<float>((size_t)rows);
    sc.bytes = c.off;
    return sc;
}

Engine::LmScratch Engine::lm_scratch(int64_t rows, int64_t W) {
    return lm_layout(lm_buf_.reserve(*this, lm_layout(nullptr, rows, W).bytes), rows, W);
}

void Engine::lm_enqueue(const float* x, int64_t rows, int64_t W, const int64_t* n, const float* g, float c, int64_t A, const float* w, const LmScratch& sc,
                        float* s, const TpScratch* tp) {
    const double samples = (double)rows * W, chunks = (double)rows * lo_chunks(W);
    if (tp) {  // section 16: the envelope of x * g drives the curve
        StageSpan span(*this, "out", "true_peak", 97.0 * samples, samples * 8 + chunks * 4);
        launch_truepeak(s_, x, rows, W, n, g, tp->pk, tp->env);
        STN_HIP(hipGetLastError());
    }
    {
        const double tiles = (double)rows * lm_tiles(W);
        StageSpan span(*this, "out", "limiter", 4.0 * samples, samples * (tp ? 12 : 8) + tiles * 8);
        launch_limiter(s_, x, rows, W, n, g, c, (int)A, w, sc.y, s, sc.pcnt, sc.pmin, tp ? tp->env : nullptr);
        STN_HIP(hipGetLastError());
        span.next("limiter_rows", tiles, tiles * 8 + (double)rows * 12);
        launch_limiter_rows(s_, rows, W, sc.pcnt, sc.pmin, sc.limited, sc.red);
    }
    STN_HIP(hipGetLastError());
    // the curve moves inter-sample peaks a little: one scalar per row then holds the ceiling, and is reported
    if (tp) tp_rows(sc.y, rows, W, n, nullptr, tp->pk, nullptr, c, tp->tp_y, tp->trim);
}

Engine::LmScratch Engine::lm_rows(const float* x, int64_t rows, int64_t W, const int64_t* n, const float* g) {
    const int hz = output_rate();
    const float* w = lm_window(hz);
    LmScratch sc = lm_scratch(rows, W);
    const TpScratch tp = pk_true_ ? tp_scratch(rows, W, true) : TpScratch{};
    lm_enqueue(x, rows, W, n, g, (float)std::pow(10.0, (double)lo_ceiling_ / 20.0), limiter_samples(hz, lm_ms_), w, sc, nullptr, pk_true_ ? &tp : nullptr);
    sc.trim = tp.trim;
    return sc;
}

void Engine::batch_limiter(float* reduction_db, int64_t* limited) {
    const int64_t Wo = out_row_len();  // (throws without a finished batch)
    const size_t B = (size_t)bt_.B;
    if (!limiter_active()) {
        if (reduction_db) std::fill(reduction_db, reduction_db + B, 0.0f);
        if (limited) std::fill(limited, limited + B, (int64_t)0);
        return;
    }
    // a reporting call: the whole stage runs again (the limited rows stay in the scratch, unused) and 12 bytes per row are read
    // back, as batch_loudness runs the measurement again; a fetch keeps no results on the host, so that _begin stays asynchronous
    const float* src = out_source(Wo);
    const LoRes m = lo_batch(src, Wo, true);
    const LmScratch sc = lm_rows(src, (int64_t)B, Wo, m.n, m.gain);
    if (reduction_db) STN_HIP(hipMemcpyAsync(reduction_db, sc.red, B * sizeof(float), hipMemcpyDeviceToHost, s_));
    if (limited) STN_HIP(hipMemcpyAsync(limited, sc.limited, B * sizeof(int64_t), hipMemcpyDeviceToHost, s_));
    sync();
}

void Engine::op_limiter(int hz, int rows, int W, const float* x, const int64_t* n, const float* gain, float ceiling_dbfs, float lookahead_ms, float* y,
                        float* s, float* reduction_db, int64_t* limited) {
    op_limiter_ex(hz, rows, W, x, n, gain, ceiling_dbfs, lookahead_ms, y, s, reduction_db, limited, STN_PEAK_SAMPLE, nullptr, nullptr);
}

void Engine::op_limiter_ex(int hz, int rows, int W, const float* x, const int64_t* n, const float* gain, float ceiling_dbfs, float lookahead_ms, float* y,
                           float* s, float* reduction_db, int64_t* limited, int peak_mode, float* env, float* trim) {
    OpScope op(*this);
    if (peak_mode != STN_PEAK_SAMPLE && peak_mode != STN_PEAK_TRUE)
        throw std::invalid_argument("peak mode " + std::to_string(peak_mode) + ": must be STN_PEAK_SAMPLE (0) or STN_PEAK_TRUE (1)");
    const bool tpm = peak_mode == STN_PEAK_TRUE;
    refuse(limiter_check(hz, lookahead_ms));
    refuse(loudness_check(nullptr, ceiling_dbfs));
    const std::vector<int64_t> nn = spans("op_limiter", rows, W, n);
    const std::vector<float> w = limiter_window(hz, lookahead_ms);
    const LmScratch sc = op.carve(lm_layout, rows, W);
    const TpScratch tp = tpm ? op.carve(tp_layout, rows, W, true) : TpScratch{};
    const size_t nx = (size_t)rows * W;
    const float* dx = op.up(x, nx);
    float* ds = s ? op.buf<float>(nx) : nullptr;
    const int64_t* dn = op.spans(rows, W, nn).n;
    const float* dw = op.up(w);
    const float* dg = op.up(gain, (size_t)rows);
    lm_enqueue(dx, rows, W, dn, dg, (float)std::pow(10.0, (double)ceiling_dbfs / 20.0), limiter_samples(hz, lookahead_ms), dw, sc, ds, tpm ? &tp : nullptr);
    op.down(y, sc.y, nx);
    op.down(s, ds, nx);
    op.down(reduction_db, sc.red, (size_t)rows);
    op.down(limited, sc.limited, (size_t)rows);
    if (tpm) op.down(env, tp.env, nx);
    if (tpm) op.down(trim, tp.trim, (size_t)rows);
    if (!tpm && trim) std::fill(trim, trim + rows, 1.0f);
    sync();  // (w is read by the copy above until here)
}

}  // namespace stn
