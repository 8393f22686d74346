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
    STN_HIP(hipSetDevice(device_));
    FormantPlan f;
    refuse(formant_plan(hz, W, f));
    if (W < 1) throw std::invalid_argument("formant: W must be >= 1");
    const std::vector<int64_t> nn = spans("op_formant", rows, W, n);
    const std::vector<float> win = pitch_window(hz);
    const std::vector<double> lagw = formant_lag_window(hz, f.p);
    ar_.reset();
    // [guard][x][guard], [guard][y][guard] and [guard][out][guard] (the scratch's own rows stay unused here)
    constexpr size_t G = GuardedRows::G;
    const size_t nx = (size_t)rows * W;
    float* blk[3];
    for (float*& b : blk) b = static_cast<float*>(ar_.alloc((nx + 2 * G) * 4));
    const int64_t* dn = op_spans(rows, W, nn).n;
    float* dwin = static_cast<float*>(ar_.alloc(win.size() * sizeof(float)));
    const size_t sc_bytes = fm_layout(nullptr, rows, W, f).bytes;
    char* sb = static_cast<char*>(ar_.alloc(sc_bytes));
    FmScratch sc = fm_layout(sb, rows, W, f);
    sc.out = blk[2] + G;
    if (probe) {
        for (float* b : blk) STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b), 0x7FC00000, nx + 2 * G, s_));
        STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sb), 0x7FC00000, sc_bytes / 4, s_));
    }
    STN_HIP(hipMemcpyAsync(blk[0] + G, x, nx * 4, hipMemcpyHostToDevice, s_));
    STN_HIP(hipMemcpyAsync(blk[1] + G, y, nx * 4, hipMemcpyHostToDevice, s_));
    STN_HIP(hipMemcpyAsync(dwin, win.data(), win.size() * sizeof(float), hipMemcpyHostToDevice, s_));
    STN_HIP(hipMemcpyAsync(sc.lagw, lagw.data(), lagw.size() * sizeof(double), hipMemcpyHostToDevice, s_));
    fm_enqueue(blk[0] + G, blk[1] + G, rows, W, dn, f, dwin, sc);
    STN_HIP(hipMemcpyAsync(out, sc.out, nx * 4, hipMemcpyDeviceToHost, s_));
    std::vector<uint32_t> guards(6 * G);
    if (probe) {
        const size_t cells = (size_t)rows * (size_t)f.frames;
        if (probe->ax) STN_HIP(hipMemcpyAsync(probe->ax, sc.ax, cells * (f.p + 1) * 4, hipMemcpyDeviceToHost, s_));
        if (probe->cy) STN_HIP(hipMemcpyAsync(probe->cy, sc.cy, cells * (f.p + 1) * 4, hipMemcpyDeviceToHost, s_));
        if (probe->g) STN_HIP(hipMemcpyAsync(probe->g, sc.g, cells * 8, hipMemcpyDeviceToHost, s_));
        if (probe->ex) STN_HIP(hipMemcpyAsync(probe->ex, sc.ex, cells * 8, hipMemcpyDeviceToHost, s_));
        if (probe->ey) STN_HIP(hipMemcpyAsync(probe->ey, sc.ey, cells * 8, hipMemcpyDeviceToHost, s_));
        for (int i = 0; i < 3; ++i) {
            STN_HIP(hipMemcpyAsync(guards.data() + 2 * i * G, blk[i], G * 4, hipMemcpyDeviceToHost, s_));
            STN_HIP(hipMemcpyAsync(guards.data() + (2 * i + 1) * G, blk[i] + G + nx, G * 4, hipMemcpyDeviceToHost, s_));
        }
    }
    sync();  // (win, lagw and guards are read or written by the copies above until here)
    if (probe) probe->guard_ok = std::all_of(guards.begin(), guards.end(), [](uint32_t v) { return v == 0x7FC00000u; });
}

}  // namespace stn
