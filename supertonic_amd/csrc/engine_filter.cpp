// engine_filter.cpp — the fetch-time biquad chain of a handle: the designer and its limits (host only), the section passes' tables and
// scratch, the passes themselves and the op-level entry.  The write kernel is kernels_filter.hip, the other two launches of a pass are
// the loudness measurement's (kernels_loudness.hip); the hook is Engine::out_source (engine_batch.cpp); DESIGN.md section 18 has the
// contract.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>

namespace stn {

namespace {

const char* const kTypeNames[] = {"highpass", "lowpass", "notch", "peak", "lowshelf", "highshelf"};

bool same_chain(const std::vector<stn_filter>& a, int n, const stn_filter* f) {
    if ((int)a.size() != n) return false;
    for (int i = 0; i < n; ++i)
        if (a[(size_t)i].type != f[i].type || a[(size_t)i].freq_hz != f[i].freq_hz || a[(size_t)i].q != f[i].q || a[(size_t)i].gain_db != f[i].gain_db) return false;
    return true;
}

}  // namespace

std::string filter_check(int n, const stn_filter* f, int rate_hz) {
    if (n < 0 || n > STN_MAX_FILTERS) return "filters: n = " + std::to_string(n) + " must be in [0, " + std::to_string(STN_MAX_FILTERS) + "]";
    if (n > 0 && !f) return "filters: f is null";
    if (n > 0 && rate_hz > 0) {
        const std::string why = rate_check("filters", rate_hz);
        if (!why.empty()) return why;
    }
    for (int i = 0; i < n; ++i) {
        const stn_filter& s = f[i];
        const std::string who = "filter " + std::to_string(i);
        if (s.type < STN_FILT_HIGHPASS || s.type > STN_FILT_HIGHSHELF) return who + ": type " + std::to_string(s.type) + " is not one of STN_FILT_* (0 .. 5)";
        const std::string name = who + " (" + kTypeNames[s.type] + ")";
        if (!(s.q >= 0.3f && s.q <= 8.0f)) return name + ": q " + num(s.q) + " must be in [0.3, 8]";
        if (!(std::fabs(s.gain_db) <= 18.0f)) return name + ": gain_db " + num(s.gain_db) + " must be in [-18, 18]";
        if (!(s.freq_hz > 0.0f)) return name + ": freq_hz " + num(s.freq_hz) + " must be positive";
        if (rate_hz <= 0) continue;  // (no model loaded yet: the corner limits are checked when the chain is first designed)
        const double fr = s.freq_hz, rate = rate_hz;
        if (fr > 0.45 * rate) return name + ": freq_hz " + num(fr) + " is above 0.45 x the output rate (" + num(0.45 * rate) + " Hz at " + std::to_string(rate_hz) + " Hz)";
        // below these corners the fp32 rounding of the coefficients moves the response by more than 0.1 dB
        const bool butter = (s.type == STN_FILT_HIGHPASS || s.type == STN_FILT_LOWPASS) && s.q >= 0.5f && s.q <= 1.5f;
        const int div = butter ? 2400 : 800;
        if (fr < rate / div)
            return name + ": freq_hz " + num(fr) + " is below the output rate / " + std::to_string(div) + " (" + num(rate / div) + " Hz at " + std::to_string(rate_hz) + " Hz)";
    }
    return "";
}

// RBJ Audio-EQ-Cookbook, normalized by a0.  1 - cos w0 is formed as 2 sin^2(w0 / 2): at a 20 Hz corner the difference would cancel
// eleven digits.
void filter_design(const stn_filter& f, int rate_hz, double c[5]) {
    const double w0 = 2.0 * M_PI * (double)f.freq_hz / (double)rate_hz;
    const double cs = std::cos(w0), sn = std::sin(w0), sh = std::sin(0.5 * w0);
    const double omc = 2.0 * sh * sh, opc = 1.0 + cs;  // 1 - cos, 1 + cos
    const double alpha = sn / (2.0 * (double)f.q);
    const double A = std::pow(10.0, (double)f.gain_db / 40.0);
    double b0 = 1, b1 = 0, b2 = 0, a0 = 1, a1 = 0, a2 = 0;
    switch (f.type) {
        case STN_FILT_HIGHPASS: b0 = 0.5 * opc; b1 = -opc; b2 = 0.5 * opc; a0 = 1 + alpha; a1 = -2 * cs; a2 = 1 - alpha; break;
        case STN_FILT_LOWPASS: b0 = 0.5 * omc; b1 = omc; b2 = 0.5 * omc; a0 = 1 + alpha; a1 = -2 * cs; a2 = 1 - alpha; break;
        case STN_FILT_NOTCH: b0 = 1; b1 = -2 * cs; b2 = 1; a0 = 1 + alpha; a1 = -2 * cs; a2 = 1 - alpha; break;
        case STN_FILT_PEAK: b0 = 1 + alpha * A; b1 = -2 * cs; b2 = 1 - alpha * A; a0 = 1 + alpha / A; a1 = -2 * cs; a2 = 1 - alpha / A; break;
        case STN_FILT_LOWSHELF: {
            const double r = 2.0 * std::sqrt(A) * alpha;
            b0 = A * ((A + 1) - (A - 1) * cs + r); b1 = 2 * A * ((A - 1) - (A + 1) * cs); b2 = A * ((A + 1) - (A - 1) * cs - r);
            a0 = (A + 1) + (A - 1) * cs + r; a1 = -2 * ((A - 1) + (A + 1) * cs); a2 = (A + 1) + (A - 1) * cs - r;
            break;
        }
        default: {  // STN_FILT_HIGHSHELF
            const double r = 2.0 * std::sqrt(A) * alpha;
            b0 = A * ((A + 1) + (A - 1) * cs + r); b1 = -2 * A * ((A - 1) + (A + 1) * cs); b2 = A * ((A + 1) + (A - 1) * cs - r);
            a0 = (A + 1) - (A - 1) * cs + r; a1 = 2 * ((A - 1) - (A + 1) * cs); a2 = (A + 1) - (A - 1) * cs - r;
            break;
        }
    }
    c[0] = b0 / a0; c[1] = b1 / a0; c[2] = b2 / a0; c[3] = a1 / a0; c[4] = a2 / a0;
}

void filter_table(int hz, int n, const stn_filter* f, FilterTable& t) {
    refuse(filter_check(n, f, hz));
    if (n > 0) refuse(rate_check("filters", hz));
    t.hz = hz;
    t.f.assign(f, f + n);
    t.pass.assign((size_t)(n + 1) / 2, LoudTable{});
    for (size_t p = 0; p < t.pass.size(); ++p) {
        LoudTable& T = t.pass[p];
        T.hz = hz;
        T.hop = 1;  // (the measurement's launches want a table with a hop; nothing here reads it)
        const float identity[5] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int h = 0; h < 2; ++h) {
            const int i = (int)p * 2 + h;
            if (i < n) {
                double c[5];
                filter_design(f[i], hz, c);
                for (int j = 0; j < 5; ++j) T.coef.c[h * 5 + j] = (float)c[j];
            } else {
                std::copy(identity, identity + 5, T.coef.c + h * 5);
            }
        }
        cascade_powers(T.coef, T.mpow);
    }
}

void Engine::fl_prepare(FlTable& m, int hz, int n, const stn_filter* f) {
    if (m.t.hz == hz && same_chain(m.t.f, n, f)) return;  // (a table of n >= 1 sections is up once it is here: a fresh one has none)
    FilterTable nt;
    filter_table(hz, n, f, nt);
    m.t = FilterTable();  // (no chain's table while its device copies change hands)
    for (size_t p = 0; p < nt.pass.size(); ++p) nt.pass[p].dev = m.dev[p].put(*this, nt.pass[p].mpow);
    m.t = std::move(nt);
}

void Engine::set_filters(int n, const stn_filter* f) {
    refuse(filter_check(n, f, loaded_ ? output_rate() : 0));
    if (same_chain(fl_set_, n, f)) return;
    fl_set_.assign(f, f + n);
    ++fl_gen_;
}

Engine::FlScratch Engine::fl_layout(char* base, int64_t rows, int64_t W) {
    const size_t nc = (size_t)rows * (size_t)lo_chunks(W);
    Carve c{base};
    FlScratch sc{};
    sc.st = c.take<float>(nc * 4);
    sc.pk = c.take<float>(nc);
    sc.bytes = c.off;
    return sc;
}

void Engine::fl_enqueue(const FilterTable& t, const float* x, int64_t rows, int64_t W, const int64_t* full, const FlScratch& sc, float* y, FlProbe* probe) {
    const double samples = (double)rows * W, chunks = (double)rows * lo_chunks(W);
    const size_t st_bytes = (size_t)rows * (size_t)lo_chunks(W) * 16;
    for (size_t p = 0; p < t.pass.size(); ++p) {
        const LoudTable& T = t.pass[p];
        const float* src = p == 0 ? x : y;
        if (probe) OpScope::poison(s_, sc.st, st_bytes / 4);
        StageSpan span(*this, "out", "filter_chunks", 11.0 * samples, samples * 4 + chunks * 20);
        launch_loudness_chunks(s_, false, src, rows, W, full, T, sc.st, sc.pk, nullptr, nullptr);
        STN_HIP(hipGetLastError());
        if (probe && probe->st_end) STN_HIP(hipMemcpyAsync(probe->st_end + p * (st_bytes / 4), sc.st, st_bytes, hipMemcpyDeviceToHost, s_));
        span.next("filter_scan", chunks * 32.0 * 11, chunks * 32);
        launch_loudness_scan(s_, rows, W, full, T, sc.st);
        STN_HIP(hipGetLastError());
        span.next("filter_write", 11.0 * samples, samples * 8 + chunks * 16);
        launch_filter_write(s_, src, rows, W, T, sc.st, y);
        STN_HIP(hipGetLastError());
        if (probe && probe->st_start) STN_HIP(hipMemcpyAsync(probe->st_start + p * (st_bytes / 4), sc.st, st_bytes, hipMemcpyDeviceToHost, s_));
    }
}

// the hook of every fetch path: the finished batch's rows at the output rate (x: b.wav, or the resampled rows already in y) through the
// chain in force into y, the fetch scratch
void Engine::fl_batch(const float* x, int64_t Wo, float* y) {
    const Batch& b = bt_;
    fl_prepare(fl_, output_rate(), (int)fl_set_.size(), fl_set_.data());
    const FlScratch sc = fl_layout(fl_buf_.reserve(*this, fl_layout(nullptr, b.B, Wo).bytes), b.B, Wo);
    fl_enqueue(fl_.t, x, b.B, Wo, batch_spans(output_rate(), Wo).dev.full, sc, y, nullptr);
}

void Engine::op_filter(int hz, int rows, int W, const float* x, int n, const stn_filter* f, float* y, FlProbe* probe) {
    OpScope op(*this);
    if (n < 1) throw std::invalid_argument("op_filter: n = " + std::to_string(n) + " must be in [1, " + std::to_string(STN_MAX_FILTERS) + "]");
    fl_prepare(op_fl_, hz, n, f);
    const size_t nx = (size_t)rows * W, off = probe && probe->x_misalign ? 1 : 0;
    float* dx = op.guarded(nx, off, probe);
    float* dy = op.guarded(nx, off, probe);
    op.put(dx, x, nx);
    const FlScratch sc = op.carve(fl_layout, rows, W);
    fl_enqueue(op_fl_.t, dx, rows, W, op.full_spans(rows, W).full, sc, dy, probe);
    op.down(y, dy, nx);
    if (probe) {
        probe->guard_ok = op.guards_ok();
        probe->form = chunk_staging_form(dx, dy, W);
    }
    sync();
}

}  // namespace stn
