// engine_resample.cpp — the output rate of a handle: the resampler's filter design (host only), its device table, and the launch
// the output stage makes when the rate is on (engine_batch.cpp).  The kernel is kernels_resample.hip.
#include "engine_internal.hpp"

#include <cmath>
#include <numeric>

namespace stn {

// Zeroth-order modified Bessel function of the first kind (power series; the Kaiser window's shape)
double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < sum * 1e-17) break;
    }
    return sum;
}

// Kaiser-windowed sinc designed at the common rate in_hz * P.  Passband edge 0.85 * min(in, out) / 2, stopband
// edge min(in, out) / 2, cutoff between the two, attenuation target 90 dB (the spec asks for 80 dB of rejection and +-0.05 dB of
// ripple; the margin keeps a passband tone's error near -90 dB).  The length comes from Kaiser's formula, rounded up to whole taps per
// phase and to a multiple of 8 (the kernel's FMA chains).  Tap j of phase p sits (p - (j - off) * P) fine samples from the output
// instant; every phase is normalised to a gain of exactly 1 at DC.
std::string resample_design(int in_hz, int out_hz, ResampleTable& f) {
    auto bad_rate = [](int hz) { return hz < RESAMPLE_MIN_HZ || hz > RESAMPLE_MAX_HZ; };
    if (bad_rate(in_hz) || bad_rate(out_hz))
        return "sample rates must be in [" + std::to_string(RESAMPLE_MIN_HZ) + ", " + std::to_string(RESAMPLE_MAX_HZ) + "] Hz (got " +
               std::to_string(in_hz) + " -> " + std::to_string(out_hz) + "); supported output rates include 8000, 11025, 16000, 22050, 24000, "
               "32000, 44100, 48000, 88200 and 96000";
    const int g = std::gcd(in_hz, out_hz);
    const int P = out_hz / g, Q = in_hz / g;
    if (P > RESAMPLE_MAX_P)
        return "output rate " + std::to_string(out_hz) + " Hz against " + std::to_string(in_hz) + " Hz reduces to P/Q = " + std::to_string(P) + "/" +
               std::to_string(Q) + ": P must be <= " + std::to_string(RESAMPLE_MAX_P);
    resample_design_pq(P, Q, in_hz, out_hz, f);
    return "";
}

void resample_design_pq(int P, int Q, int in_hz, int out_hz, ResampleTable& f) {
    f.in_hz = in_hz; f.out_hz = out_hz; f.P = P; f.Q = Q;
    if (P == Q) {  // the same rate: one centred unit tap (a copy)
        f.T = 8; f.off = 3;
        f.taps.assign(8, 0.f);
        f.taps[3] = 1.f;
        return;
    }
    constexpr double A = 90.0;
    const double beta = 0.1102 * (A - 8.7);
    const double fmin = std::min(in_hz, out_hz), f_pass = 0.85 * fmin / 2, f_stop = fmin / 2, fc = (f_pass + f_stop) / 2;
    const double fine = (double)in_hz * P;
    const double dw = 2.0 * M_PI * (f_stop - f_pass) / fine;
    const int64_t N = (int64_t)std::ceil((A - 7.95) / (2.285 * dw)) + 1;
    int64_t T = (N + P - 1) / P;
    T = (T + 7) / 8 * 8;
    f.T = (int)T;
    f.off = f.T / 2 - 1;
    const double half = (double)T * P / 2.0, i0b = bessel_i0(beta);
    f.taps.assign((size_t)P * T, 0.f);
    std::vector<double> h((size_t)T);
    for (int p = 0; p < P; ++p) {
        double sum = 0.0;
        for (int j = 0; j < f.T; ++j) {
            const double d = (double)p - (double)(j - f.off) * P;  // fine samples between the tap and the output instant
            const double x = 2.0 * fc * d / fine;
            const double sinc = x == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
            const double r = d / half;
            const double w = r * r < 1.0 ? bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b : 0.0;
            h[j] = sinc * w;
            sum += h[j];
        }
        for (int j = 0; j < f.T; ++j) f.taps[(size_t)p * T + j] = (float)(h[j] / sum);
    }
}

void Engine::rs_prepare(RsTable& m, int in_hz, int out_hz) {
    if (m.t.dev && m.t.in_hz == in_hz && m.t.out_hz == out_hz) return;
    ResampleTable n;
    const std::string why = resample_design(in_hz, out_hz, n);
    if (!why.empty()) throw std::invalid_argument(why);
    n.dev = m.dev[0].put(*this, n.taps);
    m.t = std::move(n);
}

void Engine::set_output_rate(int hz) {
    if (hz < 0 || (hz != 0 && (hz < RESAMPLE_MIN_HZ || hz > RESAMPLE_MAX_HZ)))
        throw std::invalid_argument("output rate " + std::to_string(hz) + " Hz: 0 (the model's rate) or a rate in [" + std::to_string(RESAMPLE_MIN_HZ) + ", " +
                                    std::to_string(RESAMPLE_MAX_HZ) + "] Hz");
    // (section 18) a chain in force must stay inside its limits at the new rate
    if (loaded_) refuse(filter_check((int)fl_set_.size(), fl_set_.data(), hz == 0 ? a_.sample_rate : hz));
    // (section 21) and so must a de-esser in force
    if (loaded_ && ds_.on) refuse(deesser_check(&ds_.set, hz == 0 ? a_.sample_rate : hz));
    STN_HIP(hipSetDevice(device_));
    // with a model loaded the pair is designed now (a refused pair leaves the previous rate in force); otherwise at the first fetch
    if (loaded_ && hz != 0 && hz != a_.sample_rate) rs_prepare(rs_, a_.sample_rate, hz);
    out_hz_ = hz;
}

const ResampleTable& Engine::rs_table() {
    rs_prepare(rs_, a_.sample_rate, out_hz_);  // (re)designed when the rate or the model's rate changed
    return rs_.t;
}

int64_t Engine::out_len(int64_t W) const {
    if (!resample_on()) return W;
    const int g = std::gcd(a_.sample_rate, out_hz_);
    return resample_out_len(W, out_hz_ / g, a_.sample_rate / g);
}

void Engine::resample_enqueue(const ResampleTable& t, const float* x, int64_t rows, int64_t W, int enc, void* y, int64_t dst_stride) {
    static const char* const names[] = {"resample", "resample_pcm16", "resample_pcm24", "resample_mulaw", "resample_alaw"};
    {
        const double n_out = (double)rows * resample_out_len(W, t.P, t.Q);
        StageSpan span(*this, "out", names[enc >= ENC_F32 && enc <= ENC_ALAW ? enc : 0], 2.0 * n_out * t.T, (double)rows * W * 4 + n_out * enc_bytes(enc));
        launch_resample(s_, x, rows, W, t, enc, y, dst_stride);
    }
    STN_HIP(hipGetLastError());
}

void Engine::op_resample(int in_hz, int out_hz, int rows, int W, const float* x, float* y, int16_t* pcm) {
    OpScope op(*this);
    rs_prepare(op_rs_, in_hz, out_hz);
    const int64_t W_out = resample_out_len(W, op_rs_.t.P, op_rs_.t.Q);
    const size_t ny = (size_t)rows * W_out;
    const float* dx = op.up(x, (size_t)rows * W);
    if (y) {
        float* dy = op.buf<float>(ny);
        resample_enqueue(op_rs_.t, dx, rows, W, ENC_F32, dy, W_out);
        op.down(y, dy, ny);
    }
    if (pcm) {
        int16_t* dp = op.buf<int16_t>(ny);
        resample_enqueue(op_rs_.t, dx, rows, W, ENC_PCM16, dp, W_out);
        op.down(pcm, dp, ny);
    }
    sync();
}

}  // namespace stn
