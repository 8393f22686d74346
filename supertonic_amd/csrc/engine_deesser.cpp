// engine_deesser.cpp — the fetch-time de-esser of a handle: its limits, band and coefficients (host only), the tables and the scratch,
// the sequence of eight launches and the op-level entry.  The chunk passes are kernels_deesser.hip, the band's first two launches the
// loudness measurement's (kernels_loudness.hip), the detector's scans and the row maxima the compressor's (kernels_compressor.hip); the
// hook is Engine::out_source (engine_batch.cpp); DESIGN.md section 21 has the contract.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace stn {

namespace {

void fields(const stn_deesser& c, float out[7]) {
    const float v[7] = {c.freq_hz, c.threshold_db, c.ratio, c.knee_db, c.attack_ms, c.release_ms, c.range_db};
    std::copy(v, v + 7, out);
}

bool same_setting(const float a[7], int mode, const stn_deesser& c) {
    float b[7];
    fields(c, b);
    return mode == c.mode && std::equal(a, a + 7, b);
}

// the Butterworth pair's q: 1 / (2 cos(pi / 8)) and 1 / (2 cos(3 pi / 8)), as the fp32 values the contract names
constexpr float kQ[2] = {0.54119610f, 1.30656296f};

}  // namespace

void deesser_band(const stn_deesser& c, stn_filter f[2]) {
    for (int i = 0; i < 2; ++i) f[i] = stn_filter{STN_FILT_HIGHPASS, c.freq_hz, kQ[i], 0.0f};
}

std::string deesser_check(const stn_deesser* c, int rate_hz) {
    if (!c) return "deesser: c is null";
    const Lim lim[7] = {{"freq_hz", c->freq_hz, 2000.0f, 12000.0f}, {"threshold_db", c->threshold_db, -60.0f, 0.0f}, {"ratio", c->ratio, 1.0f, 20.0f},
                        {"knee_db", c->knee_db, 0.0f, 24.0f},       {"attack_ms", c->attack_ms, 0.1f, 300.0f},       {"release_ms", c->release_ms, 10.0f, 3000.0f},
                        {"range_db", c->range_db, 1.0f, 24.0f}};
    const std::string out = range_check("deesser", lim);
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
    fields(c, t.set);
    t.mode = c.mode;
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

void Engine::ds_prepare(DeessTable& t, int hz, const stn_deesser& c) {
    if (t.hz == hz && t.band.dev && t.det.dev && same_setting(t.set, t.mode, c)) return;
    DeessTable nt;
    deesser_table(hz, c, nt);
    STN_HIP(hipSetDevice(device_));
    STN_HIP(hipMalloc(reinterpret_cast<void**>(&nt.band.dev), nt.band.mpow.size() * sizeof(double)));
    STN_HIP(hipMemcpyAsync(nt.band.dev, nt.band.mpow.data(), nt.band.mpow.size() * sizeof(double), hipMemcpyHostToDevice, s_));
    STN_HIP(hipMalloc(reinterpret_cast<void**>(&nt.det.dev), nt.det.pw.size() * sizeof(double)));
    STN_HIP(hipMemcpyAsync(nt.det.dev, nt.det.pw.data(), nt.det.pw.size() * sizeof(double), hipMemcpyHostToDevice, s_));
    sync();  // (the uploads read nt's host copies, and a fetch may still be reading the old tables)
    if (t.band.dev) (void)hipFree(t.band.dev);
    if (t.det.dev) (void)hipFree(t.det.dev);
    t = std::move(nt);
}

void Engine::ds_release() {
    for (DeessTable* t : {&ds_, &op_ds_}) {
        if (t->band.dev) { (void)hipFree(t->band.dev); t->band.dev = nullptr; }
        if (t->det.dev) { (void)hipFree(t->det.dev); t->det.dev = nullptr; }
    }
}

void Engine::set_deesser(bool on, const stn_deesser* c) {
    if (!on) {
        if (ds_on_) ++ds_gen_;
        ds_on_ = false;
        return;
    }
    refuse(deesser_check(c, loaded_ ? output_rate() : 0));
    float now[7];
    fields(ds_set_, now);
    if (ds_on_ && same_setting(now, ds_set_.mode, *c)) return;
    ds_set_ = *c;
    ds_on_ = true;
    ++ds_gen_;
}

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
    sc.nw = c.take<int64_t>((size_t)rows);
    sc.n = c.take<int64_t>((size_t)rows);
    sc.bytes = c.off;
    return sc;
}

void Engine::ds_enqueue(const DeessTable& t, const float* x, int64_t rows, int64_t W, const DsScratch& sc, float* y, DsProbe* probe, float* band, float* gr) {
    const double samples = (double)rows * W, chunks = (double)rows * lo_chunks(W);
    const size_t nc = (size_t)rows * (size_t)lo_chunks(W);
    auto out = [&](float* dst, const float* src, size_t per) { if (dst) STN_HIP(hipMemcpyAsync(dst, src, nc * per * 4, hipMemcpyDeviceToHost, s_)); };
    // the band's state at every chunk's start: the first two launches of a section pass (section 18)
    StageSpan span(*this, "out", "deesser_band_chunks", 11.0 * samples, samples * 4 + chunks * 20);
    launch_loudness_chunks(s_, false, x, rows, W, sc.nw, t.band, sc.st, sc.pk, nullptr, nullptr);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->st_end, sc.st, 4);
    span.next("deesser_band_scan", chunks * 32.0 * 11, chunks * 32);
    launch_loudness_scan(s_, rows, W, sc.nw, t.band, sc.st);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->st_start, sc.st, 4);
    // per sample: the two sections (11), log10 (about 20), the gain computer and its cap (9), the detector (3), the smoothing (2), the
    // gain 10^x and its use (about 23)
    span.next("deesser_chunks1", 43.0 * samples, samples * 4 + chunks * 20);
    launch_deesser_chunks(s_, 1, x, rows, W, sc.n, t, sc.st, sc.s1, sc.s2, y, nullptr, nullptr, sc.cmax);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s1_end, sc.s1, 1);
    span.next("deesser_scan1", chunks * 11 * 2, chunks * 8);
    launch_compressor_scan(s_, 1, rows, W, t.det, sc.s1);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s1_start, sc.s1, 1);
    span.next("deesser_chunks2", 45.0 * samples, samples * 4 + chunks * 24);
    launch_deesser_chunks(s_, 2, x, rows, W, sc.n, t, sc.st, sc.s1, sc.s2, y, nullptr, nullptr, sc.cmax);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s2_end, sc.s2, 1);
    span.next("deesser_scan2", chunks * 11 * 2, chunks * 8);
    launch_compressor_scan(s_, 2, rows, W, t.det, sc.s2);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s2_start, sc.s2, 1);
    span.next("deesser_write", 68.0 * samples, samples * (8 + (band ? 4 : 0) + (gr ? 4 : 0)) + chunks * 28);
    launch_deesser_chunks(s_, 3, x, rows, W, sc.n, t, sc.st, sc.s1, sc.s2, y, band, gr, sc.cmax);
    STN_HIP(hipGetLastError());
    span.next("deesser_rowmax", chunks, chunks * 4 + (double)rows * 4);
    launch_compressor_rowmax(s_, rows, W, sc.cmax, sc.rmax);
    STN_HIP(hipGetLastError());
}

// the hook of every fetch path: the finished batch's rows at the output rate (x: b.wav, or the rows already in y) de-essed into y, the
// fetch scratch
Engine::DsScratch Engine::ds_batch(const float* x, int64_t Wo, float* y) {
    const Batch& b = bt_;
    const int hz = output_rate();
    ds_prepare(ds_, hz, ds_set_);
    bool moved = false;
    char* base = ds_buf_.reserve(*this, ds_layout(nullptr, b.B, Wo).bytes, &moved);
    const DsScratch sc = ds_layout(base, b.B, Wo);
    // row b's valid samples: section 11's span, its reported duration at the output rate; uploaded once per finished batch, with the
    // width the band's two launches take as every row's length
    std::vector<int64_t> n = out_spans(Wo, hz);
    if (moved || n != ds_n_ || ds_n_ptr_ != sc.n || ds_n_W_ != Wo) {
        ds_n_ = std::move(n);
        ds_n_ptr_ = sc.n;
        ds_n_W_ = Wo;
        const std::vector<int64_t> nw((size_t)b.B, Wo);
        STN_HIP(hipMemcpyAsync(sc.n, ds_n_.data(), ds_n_.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
        STN_HIP(hipMemcpyAsync(sc.nw, nw.data(), nw.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
        sync();  // (the uploads read ds_n_, which the next batch's lengths replace, and nw, this frame's; once per finished batch, as cp_batch)
    }
    ds_enqueue(ds_, x, b.B, Wo, sc, y, nullptr, nullptr, nullptr);
    ds_key_ = DsKey{ed_seq_, hz, fl_gen_, ds_gen_, Wo, ds_buf_.get(), ps_gen_, xp_gen_};
    ds_valid_ = true;
    return sc;
}

void Engine::batch_deesser(float* max_reduction_db) {
    const int64_t Wo = out_row_len();
    if (!max_reduction_db) return;
    if (!deesser_on()) {  // nothing is turned down
        std::fill(max_reduction_db, max_reduction_db + bt_.B, 0.0f);
        return;
    }
    // the row maxima a fetch of this batch under this rate, chain and setting left in ds_buf_ are the report; otherwise the sequence runs
    const DsKey key{ed_seq_, output_rate(), fl_gen_, ds_gen_, Wo, ds_buf_.get(), ps_gen_, xp_gen_};
    if (!(ds_valid_ && key == ds_key_)) (void)out_source(Wo);
    const DsScratch sc = ds_layout(ds_buf_.reserve(*this, ds_layout(nullptr, bt_.B, Wo).bytes), bt_.B, Wo);
    STN_HIP(hipMemcpyAsync(max_reduction_db, sc.rmax, (size_t)bt_.B * 4, hipMemcpyDeviceToHost, s_));
    sync();
}

void Engine::op_deesser(int hz, int rows, int W, const float* x, const stn_deesser& c, float* y, DsProbe* probe) {
    STN_HIP(hipSetDevice(device_));
    ds_prepare(op_ds_, hz, c);
    ar_.reset();
    const size_t nx = (size_t)rows * W;
    GuardedRows r(*this, nx, x, probe, probe && probe->x_misalign, probe && probe->in_place);
    float* dband = probe && probe->band ? static_cast<float*>(ar_.alloc(nx * 4)) : nullptr;
    float* dgr = probe && probe->gr ? static_cast<float*>(ar_.alloc(nx * 4)) : nullptr;
    const size_t sc_bytes = ds_layout(nullptr, rows, W).bytes;
    char* sb = static_cast<char*>(ar_.alloc(sc_bytes));
    const DsScratch sc = ds_layout(sb, rows, W);
    if (probe) {
        for (float* b : {dband, dgr})
            if (b) STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b), 0x7FC00000, nx, s_));
        STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sb), 0x7FC00000, sc_bytes / 4, s_));
    }
    const std::vector<int64_t> nn((size_t)rows, (int64_t)W);
    STN_HIP(hipMemcpyAsync(sc.n, nn.data(), nn.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
    STN_HIP(hipMemcpyAsync(sc.nw, nn.data(), nn.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
    ds_enqueue(op_ds_, r.dx, rows, W, sc, r.dy, probe, dband, dgr);
    r.download(y);
    if (dband) STN_HIP(hipMemcpyAsync(probe->band, dband, nx * 4, hipMemcpyDeviceToHost, s_));
    if (dgr) STN_HIP(hipMemcpyAsync(probe->gr, dgr, nx * 4, hipMemcpyDeviceToHost, s_));
    if (probe) {
        probe->guard_ok = r.guards_ok();
        probe->form = deesser_staging_form(r.dx, r.dy, W);
    }
    sync();
}

}  // namespace stn
