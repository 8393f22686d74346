// engine_truepeak.cpp — the true-peak mode of the loudness ceiling: the 4x oversampling filter (host only), the setting, the fetch
// scratch, the reporting call and the op-level entries.  The kernels are kernels_truepeak.hip; the measurement (engine_loudness.cpp) and
// the limiter (engine_limiter.cpp) are its consumers; DESIGN.md section 16 has the contract.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>

namespace stn {

// resample_design's formula with P = 4, Q = 1, the cutoff at the input Nyquist and T = 16 given: tap j of phase p sits
// d = p - (j - off) * 4 fine samples from the output instant, h = sinc(d / 4) * I0(beta * sqrt(1 - (d / 32)^2)) / I0(beta), every phase
// normalized in double to a gain of 1 at DC.  sinc is exactly 0 at the non-zero integers, so phase 0 is the unit tap.  The filter lives
// in normalized frequency: the same taps serve every rate.
void truepeak_design(float* taps) {
    constexpr int P = TP_PHASES, T = TP_TAPS;
    const double half = (double)T * P / 2.0, i0b = bessel_i0(TP_BETA);
    for (int p = 0; p < P; ++p) {
        double h[T], sum = 0.0;
        for (int j = 0; j < T; ++j) {
            const int d = p - (j - TP_OFF) * P;
            const double x = (double)d / P;
            const double sinc = d == 0 ? 1.0 : (d % P == 0 ? 0.0 : std::sin(M_PI * x) / (M_PI * x));
            const double r = (double)d / half;
            const double w = r * r < 1.0 ? bessel_i0(TP_BETA * std::sqrt(1.0 - r * r)) / i0b : 0.0;
            h[j] = sinc * w;
            sum += h[j];
        }
        for (int j = 0; j < T; ++j) taps[p * T + j] = (float)(h[j] / sum);
    }
}

TpCoef truepeak_coef() {
    float taps[TP_PHASES * TP_TAPS];
    truepeak_design(taps);
    TpCoef c;
    for (int p = 1; p < TP_PHASES; ++p)
        for (int j = 0; j < TP_TAPS; ++j) c.h[p - 1][j] = taps[p * TP_TAPS + j];
    return c;
}

void Engine::set_peak_mode(int mode) {
    if (mode != STN_PEAK_SAMPLE && mode != STN_PEAK_TRUE)
        throw std::invalid_argument("peak mode " + std::to_string(mode) + ": must be STN_PEAK_SAMPLE (0) or STN_PEAK_TRUE (1)");
    pk_true_ = mode == STN_PEAK_TRUE;
}

Engine::TpScratch Engine::tp_layout(char* base, int64_t rows, int64_t W, bool with_env) {
    Carve c{base};
    TpScratch sc{};
    sc.pk = c.take<float>((size_t)rows * (size_t)lo_chunks(W));
    sc.tp_in = c.take<float>((size_t)rows);
    sc.tp_out = c.take<float>((size_t)rows);
    sc.tp_y = c.take<float>((size_t)rows);
    sc.trim = c.take<float>((size_t)rows);
    if (with_env) sc.env = c.take<float>((size_t)rows * (size_t)W);
    sc.bytes = c.off;
    return sc;
}

Engine::TpScratch Engine::tp_scratch(int64_t rows, int64_t W, bool with_env) {
    return tp_layout(tp_buf_.reserve(*this, tp_layout(nullptr, rows, W, with_env).bytes), rows, W, with_env);
}

void Engine::tp_rows(const float* x, int64_t rows, int64_t W, const int64_t* n, const float* g, float* pk, float* env, float c, float* tp, float* trim) {
    const double samples = (double)rows * W, chunks = (double)rows * lo_chunks(W);
    {
        StageSpan span(*this, "out", "true_peak", 97.0 * samples, samples * (env ? 8 : 4) + chunks * 4);
        launch_truepeak(s_, x, rows, W, n, g, pk, env);
        STN_HIP(hipGetLastError());
        span.next("true_peak_rows", chunks, chunks * 4 + (double)rows * 8);
        launch_truepeak_rows(s_, rows, W, n, pk, c, tp, trim);
    }
    STN_HIP(hipGetLastError());
}

void Engine::batch_true_peak(float* tp_in, float* tp_out, float* trim) {
    const int64_t Wo = out_row_len();  // (throws without a finished batch)
    const int64_t B = bt_.B;
    const float c = (float)std::pow(10.0, (double)lo_ceiling_ / 20.0);
    // a reporting call, as batch_limiter is: the stage runs again and 12 bytes per row are read back
    const float* src = out_source(Wo);
    const LoRes m = lo_batch(src, Wo, lo_on_);
    const bool lim_true = limiter_active() && pk_true_;
    const TpScratch sc = tp_scratch(B, Wo, lim_true);   // (sized for the limiter's use below: it moves no more)
    tp_rows(src, B, Wo, m.n, nullptr, sc.pk, nullptr, c, sc.tp_in, nullptr);
    const float* d_out = sc.tp_in;
    const float* d_trim = nullptr;
    if (lo_on_) {
        if (limiter_active()) {
            const LmScratch lm = lm_rows(src, B, Wo, m.n, m.gain);
            d_trim = lm.trim;
            tp_rows(lm.y, B, Wo, m.n, lm.trim, sc.pk, nullptr, c, sc.tp_out, nullptr);
        } else {
            tp_rows(src, B, Wo, m.n, m.gain, sc.pk, nullptr, c, sc.tp_out, nullptr);
        }
        d_out = sc.tp_out;
    }
    if (tp_in) STN_HIP(hipMemcpyAsync(tp_in, sc.tp_in, (size_t)B * 4, hipMemcpyDeviceToHost, s_));
    if (tp_out) STN_HIP(hipMemcpyAsync(tp_out, d_out, (size_t)B * 4, hipMemcpyDeviceToHost, s_));
    if (trim) {
        if (d_trim) STN_HIP(hipMemcpyAsync(trim, d_trim, (size_t)B * 4, hipMemcpyDeviceToHost, s_));
        else std::fill(trim, trim + B, 1.0f);
    }
    sync();
}

const char* Engine::op_true_peak(int hz, int rows, int W, const float* x, const int64_t* n, const float* gain, int x_misalign, float* tp, float* env,
                                 float* pk) {
    OpScope op(*this);
    refuse(rate_check("true peak", hz));
    const std::vector<int64_t> nn = spans("op_true_peak", rows, W, n);
    const size_t nx = (size_t)rows * W, nc = (size_t)rows * (size_t)lo_chunks(W);
    const float* dx = op.up(x, nx, x_misalign ? 1 : 0);
    const TpScratch sc = op.carve(tp_layout, rows, W, env != nullptr);
    const int64_t* dn = op.spans(rows, W, nn).n;
    const float* dg = op.up(gain, (size_t)rows);
    if (sc.env) op.poison(sc.env, nx);
    op.poison(sc.pk, nc);
    op.poison(sc.tp_in, (size_t)rows);
    tp_rows(dx, rows, W, dn, dg, sc.pk, sc.env, 1.0f, sc.tp_in, nullptr);
    op.down(tp, sc.tp_in, (size_t)rows);
    op.down(env, sc.env, nx);
    op.down(pk, sc.pk, nc);
    sync();
    return truepeak_staging_form(dx, W, sc.env);
}

}  // namespace stn
