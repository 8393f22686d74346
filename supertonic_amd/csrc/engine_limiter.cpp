// engine_limiter.cpp — the look-ahead peak limiter behind the loudness gain: the setting, the Hann weights (host only), the fetch
// scratch that holds the limited fp32 rows, and the step the output stage (engine_batch.cpp) and batch_limiter share.  The kernels are
// kernels_limiter.hip; DESIGN.md section 15 has the contract.
#include "engine.hpp"

#include <algorithm>
#include <cmath>

namespace stn {

std::string limiter_check(int hz, float lookahead_ms) {
    if (!(lookahead_ms >= 0.5f && lookahead_ms <= 10.0f)) return "limiter look-ahead " + std::to_string(lookahead_ms) + " ms: must be in [0.5, 10]";
    if (hz < LO_MIN_HZ || hz > LO_MAX_HZ)
        return "limiter: sample rate must be in [" + std::to_string(LO_MIN_HZ) + ", " + std::to_string(LO_MAX_HZ) + "] Hz (got " + std::to_string(hz) + ")";
    return "";
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
    const std::string why = limiter_check(LO_MIN_HZ, lookahead_ms);  // (the rate is the fetch's: checked there)
    if (!why.empty()) throw std::invalid_argument(why);
    lm_on_ = on;
    lm_ms_ = lookahead_ms;
}

void Engine::get_limiter(int* on, float* lookahead_ms) const {
    if (on) *on = lm_on_ ? 1 : 0;
    if (lookahead_ms) *lookahead_ms = lm_ms_;
}

void Engine::lm_release() {
    if (lm_buf_) (void)hipFree(lm_buf_);
    if (lm_win_) (void)hipFree(lm_win_);
    lm_buf_ = nullptr; lm_buf_cap_ = 0;
    lm_win_ = nullptr; lm_win_cap_ = 0; lm_win_hz_ = 0; lm_win_ms_ = -1.0f;
}

// uploaded once per (rate, look-ahead)
const float* Engine::lm_window(int hz) {
    if (lm_win_ && lm_win_hz_ == hz && lm_win_ms_ == lm_ms_) return lm_win_;
    const std::string why = limiter_check(hz, lm_ms_);
    if (!why.empty()) throw std::invalid_argument(why);
    const std::vector<float> w = limiter_window(hz, lm_ms_);
    sync();  // a fetch may still be reading the old weights
    if (!lm_win_ || w.size() > lm_win_cap_) {
        if (lm_win_) (void)hipFree(lm_win_);
        lm_win_ = nullptr; lm_win_cap_ = 0;
        STN_HIP(hipMalloc(reinterpret_cast<void**>(&lm_win_), w.size() * sizeof(float)));
        lm_win_cap_ = w.size();
    }
    STN_HIP(hipMemcpy(lm_win_, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    lm_win_hz_ = hz; lm_win_ms_ = lm_ms_;
    return lm_win_;
}

// grow-only scratch (not part of the resident batch: growing it re-keys no captured graph): the limited rows, per tile the two
// partial results, per row the two results
static size_t lm_up(size_t b) { return (b + 255) / 256 * 256; }
size_t Engine::lm_layout(int64_t rows, int64_t W, size_t* o) {
    const size_t nt = (size_t)rows * (size_t)lm_tiles(W);
    o[0] = 0;                                          // y
    o[1] = o[0] + lm_up((size_t)rows * (size_t)W * 4);  // pcnt
    o[2] = o[1] + lm_up(nt * 4);                       // pmin
    o[3] = o[2] + lm_up(nt * 4);                       // limited
    o[4] = o[3] + lm_up((size_t)rows * 8);             // red
    return o[4] + lm_up((size_t)rows * 4);
}
Engine::LmScratch Engine::lm_at(char* base, const size_t* o) {
    return {reinterpret_cast<float*>(base + o[0]), reinterpret_cast<int*>(base + o[1]), reinterpret_cast<float*>(base + o[2]),
            reinterpret_cast<int64_t*>(base + o[3]), reinterpret_cast<float*>(base + o[4])};
}

Engine::LmScratch Engine::lm_scratch(int64_t rows, int64_t W) {
    size_t o[5];
    const size_t need = lm_layout(rows, W, o);
    if (!lm_buf_ || need > lm_buf_cap_) {
        sync();  // the previous fetch may still be reading it
        if (lm_buf_) (void)hipFree(lm_buf_);
        lm_buf_ = nullptr; lm_buf_cap_ = 0;
        STN_HIP(hipMalloc(reinterpret_cast<void**>(&lm_buf_), need + need / 4));
        lm_buf_cap_ = need + need / 4;
    }
    return lm_at(lm_buf_, o);
}

Engine::LmScratch Engine::lm_rows(const float* x, int64_t rows, int64_t W, const float* g) {
    const int hz = output_rate();
    const float* w = lm_window(hz);
    LmScratch sc = lm_scratch(rows, W);
    const float c = (float)std::pow(10.0, (double)lo_ceiling_ / 20.0);
    const double samples = (double)rows * W, chunks = (double)rows * lo_chunks(W);
    const TpScratch tp = pk_true_ ? tp_scratch(rows, W, true) : TpScratch{};
    if (pk_true_) {  // section 16: the envelope of x * g drives the curve
        StageSpan span(*this, "out", "true_peak", 97.0 * samples, samples * 8 + chunks * 4);
        launch_truepeak(s_, x, rows, W, lo_n_ptr_, g, tp.pk, tp.env);
        STN_HIP(hipGetLastError());
    }
    {
        const double tiles = (double)rows * lm_tiles(W);
        StageSpan span(*this, "out", "limiter", 4.0 * samples, samples * (pk_true_ ? 12 : 8) + tiles * 8);
        launch_limiter(s_, x, rows, W, lo_n_ptr_, g, c, (int)limiter_samples(hz, lm_ms_), w, sc.y, nullptr, sc.pcnt, sc.pmin, tp.env);
        STN_HIP(hipGetLastError());
        span.next("limiter_rows", tiles, tiles * 8 + (double)rows * 12);
        launch_limiter_rows(s_, rows, W, sc.pcnt, sc.pmin, sc.limited, sc.red);
    }
    STN_HIP(hipGetLastError());
    if (pk_true_) {  // the curve moves inter-sample peaks a little: one scalar per row then holds the ceiling, and is reported
        tp_rows(sc.y, rows, W, lo_n_ptr_, nullptr, tp.pk, c, tp.tp_y, tp.trim);
        sc.trim = tp.trim;
    }
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
    const float* g = lo_batch(src, Wo, true) + 2 * (int64_t)B;
    const LmScratch sc = lm_rows(src, (int64_t)B, Wo, g);
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
    STN_HIP(hipSetDevice(device_));
    if (peak_mode != STN_PEAK_SAMPLE && peak_mode != STN_PEAK_TRUE)
        throw std::invalid_argument("peak mode " + std::to_string(peak_mode) + ": must be STN_PEAK_SAMPLE (0) or STN_PEAK_TRUE (1)");
    const bool tpm = peak_mode == STN_PEAK_TRUE;
    const std::string why = limiter_check(hz, lookahead_ms);
    if (!why.empty()) throw std::invalid_argument(why);
    if (!(ceiling_dbfs >= -30.0f && ceiling_dbfs <= 0.0f))
        throw std::invalid_argument("loudness peak ceiling " + std::to_string(ceiling_dbfs) + " dBFS: must be in [-30, 0]");
    std::vector<int64_t> nn((size_t)rows, (int64_t)W);
    for (int r = 0; r < rows && n; ++r) {
        if (n[r] < 0 || n[r] > W) throw std::invalid_argument("op_limiter: n[" + std::to_string(r) + "] = " + std::to_string(n[r]) + " outside [0, W]");
        nn[(size_t)r] = n[r];
    }
    const std::vector<float> w = limiter_window(hz, lookahead_ms);
    ar_.reset();
    size_t o[5];
    const size_t need = lm_layout(rows, W, o);
    const LmScratch sc = lm_at(static_cast<char*>(ar_.alloc(need)), o);
    const size_t nx = (size_t)rows * W;
    float* dx = static_cast<float*>(ar_.alloc(nx * 4));
    float* ds = s ? static_cast<float*>(ar_.alloc(nx * 4)) : nullptr;
    int64_t* dn = static_cast<int64_t*>(ar_.alloc((size_t)rows * 8));
    float* dw = static_cast<float*>(ar_.alloc(w.size() * 4));
    float* dg = gain ? static_cast<float*>(ar_.alloc((size_t)rows * 4)) : nullptr;
    float* denv = tpm ? static_cast<float*>(ar_.alloc(nx * 4)) : nullptr;
    float* dpk = tpm ? static_cast<float*>(ar_.alloc((size_t)rows * (size_t)lo_chunks(W) * 4)) : nullptr;
    float* dtp = tpm ? static_cast<float*>(ar_.alloc((size_t)rows * 8)) : nullptr;  // [rows] true peak of y, [rows] trim
    STN_HIP(hipMemcpyAsync(dx, x, nx * 4, hipMemcpyHostToDevice, s_));
    STN_HIP(hipMemcpyAsync(dn, nn.data(), nn.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
    STN_HIP(hipMemcpyAsync(dw, w.data(), w.size() * 4, hipMemcpyHostToDevice, s_));
    if (dg) STN_HIP(hipMemcpyAsync(dg, gain, (size_t)rows * 4, hipMemcpyHostToDevice, s_));
    const float c = (float)std::pow(10.0, (double)ceiling_dbfs / 20.0);
    if (tpm) {
        launch_truepeak(s_, dx, rows, W, dn, dg, dpk, denv);
        STN_HIP(hipGetLastError());
    }
    launch_limiter(s_, dx, rows, W, dn, dg, c, (int)limiter_samples(hz, lookahead_ms), dw, sc.y, ds, sc.pcnt, sc.pmin, denv);
    STN_HIP(hipGetLastError());
    launch_limiter_rows(s_, rows, W, sc.pcnt, sc.pmin, sc.limited, sc.red);
    STN_HIP(hipGetLastError());
    if (y) STN_HIP(hipMemcpyAsync(y, sc.y, nx * 4, hipMemcpyDeviceToHost, s_));
    if (s) STN_HIP(hipMemcpyAsync(s, ds, nx * 4, hipMemcpyDeviceToHost, s_));
    if (reduction_db) STN_HIP(hipMemcpyAsync(reduction_db, sc.red, (size_t)rows * 4, hipMemcpyDeviceToHost, s_));
    if (limited) STN_HIP(hipMemcpyAsync(limited, sc.limited, (size_t)rows * 8, hipMemcpyDeviceToHost, s_));
    if (tpm) {
        launch_truepeak(s_, sc.y, rows, W, dn, nullptr, dpk, nullptr);
        STN_HIP(hipGetLastError());
        launch_truepeak_rows(s_, rows, W, dn, dpk, c, dtp, dtp + rows);
        STN_HIP(hipGetLastError());
        if (env) STN_HIP(hipMemcpyAsync(env, denv, nx * 4, hipMemcpyDeviceToHost, s_));
        if (trim) STN_HIP(hipMemcpyAsync(trim, dtp + rows, (size_t)rows * 4, hipMemcpyDeviceToHost, s_));
    } else if (trim) {
        std::fill(trim, trim + rows, 1.0f);
    }
    sync();  // (nn and w are read by the copies above until here)
}

}  // namespace stn
