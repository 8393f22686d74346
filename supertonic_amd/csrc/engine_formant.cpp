// engine_formant.cpp — the pitch mode of a handle and the formant correction: under STN_PITCH_FORMANT the pitch
// stage (engine_pitch.cpp) ends with two launches (kernels_formant.hip) that read the rows before the shift and the shifted rows and
// write the rows every later stage starts from.  The geometry, the lag window and the recursion's host statement are host/formant.cpp.
#include "engine_internal.hpp"

namespace stn {

void Engine::set_pitch_mode(int mode) {
    if (mode != STN_PITCH_RESAMPLE && mode != STN_PITCH_FORMANT)
        throw std::invalid_argument("pitch mode " + std::to_string(mode) + ": STN_PITCH_RESAMPLE (0) or STN_PITCH_FORMANT (1)");
    if (mode == ps_mode_) return;
    ps_mode_ = mode;
    ++ps_gen_;  // (rows that went through another mode: nothing measured on them holds)
}

Engine::FmScratch Engine::fm_layout(char* base, int64_t rows, int64_t W, const FormantPlan& f) {
    Carve c{base};
    FmScratch sc;
    const size_t cells = (size_t)rows * (size_t)f.frames;
    sc.lagw = c.take<double>((size_t)f.p + 1);
    sc.ax = c.take<float>(cells * (f.p + 1));
    sc.cy = c.take<float>(cells * (f.p + 1));
    sc.g = c.take<double>(cells);
    sc.ex = c.take<double>(cells);
    sc.ey = c.take<double>(cells);
    sc.out = c.take<float>((size_t)rows * W);
    sc.bytes = c.off;
    return sc;
}

void Engine::fm_enqueue(const float* x, const float* y, int64_t rows, int64_t W, const int64_t* n, const FormantPlan& f, const float* win,
                        const FmScratch& sc) {
    {
        const double N = 2.0 * f.H, cells = (double)rows * f.frames;
        StageSpan span(*this, "out", "formant_lpc", cells * 2.0 * (f.p + 1) * N * 2.0, cells * (2.0 * N * 4 + 2.0 * (f.p + 1) * 4 + 24));
        launch_formant_lpc(s_, x, y, rows, W, n, f.H, f.frames, f.p, win, sc.lagw, sc.ax, sc.cy, sc.g, sc.ex, sc.ey);
        span.next("formant_filter", cells * 2.0 * 4.0 * f.H * (2.0 * f.p + 1) * 2.0, cells * (4.0 * f.H * 4 + 2.0 * (f.p + 1) * 4) + (double)rows * W * 4);
        launch_formant_filter(s_, y, rows, W, n, f.H, f.frames, f.p, win, sc.ax, sc.cy, sc.out);
    }
    STN_HIP(hipGetLastError());
}

void Engine::op_formant(int hz, int rows, int W, const float* x, const float* y, const int64_t* n, float* out, FormantProbe* probe) {
    OpScope op(*this);
    FormantPlan f;
    refuse(formant_plan(hz, W, f));
    if (W < 1) throw std::invalid_argument("formant: W must be >= 1");
    const std::vector<int64_t> nn = spans("op_formant", rows, W, n);
    const std::vector<float> win = pitch_window(hz);
    const std::vector<double> lagw = formant_lag_window(hz, f.p);
    // [guard][x][guard], [guard][y][guard] and [guard][out][guard] (the scratch's own rows stay unused here)
    const size_t nx = (size_t)rows * W;
    float* dx = op.guarded(nx, 0, probe);
    float* dy = op.guarded(nx, 0, probe);
    float* dout = op.guarded(nx, 0, probe);
    const int64_t* dn = op.spans(rows, W, nn).n;
    float* dwin = op.buf<float>(win.size());
    FmScratch sc = op.carve_poisoned(probe, fm_layout, rows, W, f);
    sc.out = dout;
    op.put(dx, x, nx);
    op.put(dy, y, nx);
    op.put(dwin, win.data(), win.size());
    op.put(sc.lagw, lagw.data(), lagw.size());
    fm_enqueue(dx, dy, rows, W, dn, f, dwin, sc);
    op.down(out, sc.out, nx);
    if (probe) {
        const size_t cells = (size_t)rows * (size_t)f.frames;
        op.down(probe->ax, sc.ax, cells * (f.p + 1));
        op.down(probe->cy, sc.cy, cells * (f.p + 1));
        op.down(probe->g, sc.g, cells);
        op.down(probe->ex, sc.ex, cells);
        op.down(probe->ey, sc.ey, cells);
        probe->guard_ok = op.guards_ok();
    }
    sync();  // (win and lagw are read by the copies above until here)
}

}  // namespace stn
