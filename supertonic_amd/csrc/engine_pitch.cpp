// engine_pitch.cpp — the pitch of a handle: a shift of s semitones is a time stretch by a / b ~ 2^(s/12) at the
// model's rate (WSOLA, kernels_pitch.hip) and a resample by b / a back to the row length (kernels_resample.hip), in front of every other
// stage of the output stage.  The ratio, the geometry and the window are host/pitch.cpp.
#include "engine_internal.hpp"

#include "host/pitch.hpp"

namespace stn {

// the rates the a / b table is designed at: a k -> b k Hz with the smallest k that puts both in the resampler's range (max / min <= 2,
// so a k with min k >= 8000 has max k <= 17280).  stn_op_resample(a k, b k) designs the same table.
static int ps_rate_scale(int a, int b) { return (RESAMPLE_MIN_HZ + std::min(a, b) - 1) / std::min(a, b); }

void Engine::ps_table(RsTable& m, int a, int b) {
    const int k = ps_rate_scale(a, b);
    if (m.t.dev && m.t.in_hz == a * k && m.t.out_hz == b * k) return;
    ResampleTable n;
    resample_design_pq(b, a, a * k, b * k, n);
    n.dev = m.dev[0].put(*this, n.taps);
    m.t = std::move(n);
}

void Engine::set_pitch(float semitones) {
    int a = 1, b = 1;
    if (!pitch_ratio(semitones, a, b)) throw std::invalid_argument(pitch_check(semitones));
    ps_semi_ = semitones; ps_a_ = a; ps_b_ = b;
    ++ps_gen_;  // (rows that went through another shift: nothing measured on them holds)
}

Engine::PsScratch Engine::ps_layout(char* base, int64_t rows, int64_t W, const PitchPlan& p) {
    Carve c{base};
    PsScratch sc;
    sc.win = c.take<float>((size_t)2 * p.H);
    sc.delta = c.take<int>((size_t)rows * p.M);
    sc.score = c.take<float>((size_t)rows * p.M);
    sc.ys = c.take<float>((size_t)rows * p.Ws);
    sc.y = c.take<float>((size_t)rows * W);
    sc.bytes = c.off;
    return sc;
}

void Engine::ps_enqueue(const float* x, int64_t rows, int64_t W, const int64_t* n, int a, int b, const PitchPlan& p, const float* win, int* delta,
                        float* score, float* ys) {
    {
        const double N = 2.0 * p.H, cand = 2.0 * p.delta + 1.0;
        StageSpan span(*this, "out", "pitch_search", (double)rows * p.M * cand * N * 4.0, (double)rows * p.M * (2.0 * N + 2.0 * p.delta) * 4);
        launch_pitch_search(s_, x, rows, W, n, p.H, p.M, a, b, delta, score);
        span.next("pitch_ola", 3.0 * rows * p.Ws, (double)rows * p.Ws * 12);
        launch_pitch_ola(s_, x, rows, W, n, p.H, p.M, p.Ws, a, b, delta, win, ys);
    }
    STN_HIP(hipGetLastError());
}

void Engine::ps_resample(const ResampleTable& t, const float* ys, int64_t rows, int64_t Ws, int64_t W, float* y) {
    {
        const double n_out = (double)rows * W;
        StageSpan span(*this, "out", "pitch_resample", 2.0 * n_out * t.T, (double)rows * Ws * 4 + n_out * 4);
        launch_resample(s_, ys, rows, Ws, t, ENC_F32, y, W, W);  // (ceil(Ws b / a) >= W: the first W are the row)
    }
    STN_HIP(hipGetLastError());
}

const float* Engine::ps_batch() {
    const Batch& b = bt_;
    const int hz = a_.sample_rate;
    const int64_t W = native_row_len();
    PitchPlan p;
    refuse(pitch_plan(hz, W, ps_a_, ps_b_, p));
    // section 26: under STN_PITCH_FORMANT the correction's scratch lies behind the shift's, and its rows are the stage's result
    const bool formant = ps_mode_ == STN_PITCH_FORMANT;
    FormantPlan f;
    if (formant) refuse(formant_plan(hz, W, f));
    const size_t ps_bytes = ps_layout(nullptr, b.B, W, p).bytes;
    bool moved = false;
    char* base = ps_buf_.reserve(*this, ps_bytes + (formant ? fm_layout(nullptr, b.B, W, f).bytes : 0), &moved);
    const PsScratch sc = ps_layout(base, b.B, W, p);
    const FmScratch fm = formant ? fm_layout(base + ps_bytes, b.B, W, f) : FmScratch{};
    const float* res = formant ? fm.out : sc.y;
    const PsKey key{ed_seq_, ps_gen_, W, b.B, base};
    if (!moved && ps_valid_ && key == ps_key_) return res;  // later fetches of the same batch under the same shift and mode reuse the rows
    const int64_t* n = batch_spans(hz, W).dev.n;  // (the spans at the model's rate: the span table's own entry)
    ps_win_ = pitch_window(hz);
    STN_HIP(hipMemcpyAsync(sc.win, ps_win_.data(), ps_win_.size() * sizeof(float), hipMemcpyHostToDevice, s_));
    if (formant) {
        fm_lagw_ = formant_lag_window(hz, f.p);
        STN_HIP(hipMemcpyAsync(fm.lagw, fm_lagw_.data(), fm_lagw_.size() * sizeof(double), hipMemcpyHostToDevice, s_));
    }
    sync();  // (the uploads read ps_win_ and fm_lagw_, which the next batch or setting replaces; once per finished batch and setting)
    ps_table(ps_rs_, ps_a_, ps_b_);
    ps_enqueue(b.wav, b.B, W, n, ps_a_, ps_b_, p, sc.win, sc.delta, sc.score, sc.ys);
    ps_resample(ps_rs_.t, sc.ys, b.B, p.Ws, W, sc.y);
    if (formant) fm_enqueue(b.wav, sc.y, b.B, W, n, f, sc.win, fm);
    ps_key_ = key;
    ps_valid_ = true;
    return res;
}

// the stretch (and, with y, the resample behind it) on the caller's rows: the launches of ps_batch on arena buffers
void Engine::ps_op(int hz, int rows, int W, const float* x, const int64_t* n, int a, int b, float* ys_out, int* delta_out, float* score_out, float* y_out,
                   int mode) {
    OpScope op(*this);
    PitchPlan p;
    refuse(pitch_plan(hz, W, a, b, p));
    if (W < 1) throw std::invalid_argument("pitch: W must be >= 1");
    if (mode != STN_PITCH_RESAMPLE && mode != STN_PITCH_FORMANT) throw std::invalid_argument("pitch mode: STN_PITCH_RESAMPLE or STN_PITCH_FORMANT");
    const bool formant = mode == STN_PITCH_FORMANT && y_out;
    FormantPlan f;
    if (formant) refuse(formant_plan(hz, W, f));
    const std::vector<int64_t> nn = spans("op_pitch", rows, W, n);
    const std::vector<float> win = pitch_window(hz);
    const std::vector<double> lagw = formant ? formant_lag_window(hz, f.p) : std::vector<double>();
    const PsScratch sc = op.carve(ps_layout, rows, W, p);
    const size_t nx = (size_t)rows * W;
    const float* dx = op.up(x, nx);
    const int64_t* dn = op.spans(rows, W, nn).n;
    op.put(sc.win, win.data(), win.size());
    if (y_out) ps_table(op_ps_rs_, a, b);
    ps_enqueue(dx, rows, W, dn, a, b, p, sc.win, sc.delta, sc.score, sc.ys);
    if (y_out) {
        ps_resample(op_ps_rs_.t, sc.ys, rows, p.Ws, W, sc.y);
        const float* res = sc.y;
        if (formant) {
            const FmScratch fm = op.carve(fm_layout, rows, W, f);
            op.put(fm.lagw, lagw.data(), lagw.size());
            fm_enqueue(dx, sc.y, rows, W, dn, f, sc.win, fm);
            res = fm.out;
        }
        op.down(y_out, res, nx);
    }
    op.down(ys_out, sc.ys, (size_t)rows * p.Ws);
    op.down(delta_out, sc.delta, (size_t)rows * p.M);
    op.down(score_out, sc.score, (size_t)rows * p.M);
    sync();  // (win and lagw are read by the copies above until here)
}

void Engine::op_time_stretch(int hz, int rows, int W, const float* x, const int64_t* n, int a, int b, float* y, int* delta, float* score) {
    ps_op(hz, rows, W, x, n, a, b, y, delta, score, nullptr);
}

void Engine::op_pitch(int hz, int rows, int W, const float* x, const int64_t* n, float semitones, float* y) {
    int a = 1, b = 1;
    if (!pitch_ratio(semitones, a, b)) throw std::invalid_argument(pitch_check(semitones));
    ps_op(hz, rows, W, x, n, a, b, nullptr, nullptr, nullptr, y);
}

void Engine::op_pitch_ex(int hz, int rows, int W, const float* x, const int64_t* n, float semitones, int mode, float* y) {
    int a = 1, b = 1;
    if (!pitch_ratio(semitones, a, b)) throw std::invalid_argument(pitch_check(semitones));
    ps_op(hz, rows, W, x, n, a, b, nullptr, nullptr, nullptr, y, mode);
}

}  // namespace stn
