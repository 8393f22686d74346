// engine_expander.cpp — the fetch-time downward expander / noise gate of a handle: its limits, coefficients and static curve (host
// only), the scan tables and the scratch, the sequence of launches and the op-level entry.  The kernels are kernels_expander.hip; the
// hook is Engine::out_source (engine_batch.cpp); DESIGN.md section 25 has the contract.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace stn {

namespace {

void fields(const stn_expander& c, float out[7]) {
    const float v[7] = {c.threshold_db, c.ratio, c.knee_db, c.range_db, c.attack_ms, c.hold_ms, c.release_ms};
    std::copy(v, v + 7, out);
}

bool same_setting(const float a[7], const stn_expander& c) {
    float b[7];
    fields(c, b);
    return std::equal(a, a + 7, b);
}

// the fp32 values the kernels compute with (and the float64 reference is given): T, S = ratio - 1, K, R
ExpCoef static_coef(const stn_expander& c) {
    ExpCoef f{};
    f.T = c.threshold_db;
    f.S = (float)((double)c.ratio - 1.0);
    f.K = c.knee_db;
    f.R = c.range_db;
    return f;
}

}  // namespace

std::string expander_check(const stn_expander* c) {
    if (!c) return "expander: c is null";
    const Lim lim[7] = {{"threshold_db", c->threshold_db, -90.0f, -10.0f}, {"ratio", c->ratio, 1.0f, 20.0f},       {"knee_db", c->knee_db, 0.0f, 24.0f},
                        {"range_db", c->range_db, 1.0f, 80.0f},            {"attack_ms", c->attack_ms, 0.1f, 300.0f}, {"hold_ms", c->hold_ms, 0.0f, 500.0f},
                        {"release_ms", c->release_ms, 10.0f, 3000.0f}};
    return range_check("expander", lim);
}

double expander_curve(const stn_expander& c, double in_db) {
    const ExpCoef f = static_coef(c);
    const double T = f.T, S = f.S, K = f.K, d = T - in_db;
    double z;
    if (2.0 * d < -K) z = 0.0;
    else if (K > 0.0 && 2.0 * std::fabs(d) <= K) z = S * (d + 0.5 * K) * (d + 0.5 * K) / (2.0 * K);
    else z = S * d;
    return in_db - std::min(z, (double)f.R);
}

void expander_table(int hz, const stn_expander& c, ExpTable& t) {
    refuse(expander_check(&c));
    refuse(rate_check("expander", hz));
    t.hz = hz;
    fields(c, t.set);
    t.coef = static_coef(c);
    t.coef.kA = (float)compressor_k(c.attack_ms, hz);
    // release_ms is the time a fully open gate takes to close through the whole range: delta dB per sample
    t.coef.delta = (float)((double)c.range_db * 1000.0 / ((double)c.release_ms * (double)hz));
    t.hold = (int64_t)std::floor((double)c.hold_ms * (double)hz / 1000.0 + 0.5);
    t.coef.Bh = (float)((double)t.coef.delta * (double)t.hold);
    // what i + 1 chunks of LO_CHUNK samples subtract from a start value of stage 1, and multiply one of stage 2 by, from the fp32
    // delta and k the kernels run on
    const double c1 = (double)LO_CHUNK * (double)t.coef.delta, E = std::pow(1.0 - (double)t.coef.kA, LO_CHUNK);
    t.pw.assign((size_t)2 * LO_SCAN, 0.0);
    double e = E;
    for (int i = 0; i < LO_SCAN; ++i) {
        t.pw[(size_t)i] = (double)(i + 1) * c1;
        t.pw[(size_t)LO_SCAN + i] = e;
        e *= E;
    }
}

void Engine::xp_prepare(ExpTable& t, int hz, const stn_expander& c) {
    if (t.hz == hz && t.dev && same_setting(t.set, c)) return;
    ExpTable nt;
    expander_table(hz, c, nt);
    STN_HIP(hipSetDevice(device_));
    STN_HIP(hipMalloc(reinterpret_cast<void**>(&nt.dev), nt.pw.size() * sizeof(double)));
    STN_HIP(hipMemcpyAsync(nt.dev, nt.pw.data(), nt.pw.size() * sizeof(double), hipMemcpyHostToDevice, s_));
    sync();  // (the upload reads nt's host copy, and a fetch may still be reading the old table)
    if (t.dev) (void)hipFree(t.dev);
    t = std::move(nt);
}

void Engine::xp_release() {
    for (ExpTable* t : {&xp_, &op_xp_})
        if (t->dev) { (void)hipFree(t->dev); t->dev = nullptr; }
}

void Engine::set_expander(bool on, const stn_expander* c) {
    if (!on) {
        if (xp_on_) ++xp_gen_;
        xp_on_ = false;
        return;
    }
    refuse(expander_check(c));
    float now[7];
    fields(xp_set_, now);
    if (xp_on_ && same_setting(now, *c)) return;
    xp_set_ = *c;
    xp_on_ = true;
    ++xp_gen_;
}

Engine::XpScratch Engine::xp_layout(char* base, int64_t rows, int64_t W) {
    const size_t nc = (size_t)rows * (size_t)lo_chunks(W);
    Carve c{base};
    XpScratch sc{};
    sc.s1 = c.take<float>(nc);
    sc.s2 = c.take<float>(nc);
    sc.cmin = c.take<float>(nc);
    sc.ccnt = c.take<int32_t>(nc);
    sc.rmin = c.take<float>((size_t)rows);
    sc.rcnt = c.take<int64_t>((size_t)rows);
    sc.n = c.take<int64_t>((size_t)rows);
    sc.bytes = c.off;
    return sc;
}

void Engine::xp_enqueue(const ExpTable& t, const float* x, int64_t rows, int64_t W, const XpScratch& sc, float* y, float* open, XpProbe* probe) {
    const double samples = (double)rows * W, chunks = (double)rows * lo_chunks(W);
    const size_t st_bytes = (size_t)rows * (size_t)lo_chunks(W) * 4;
    auto out = [&](float* dst, const float* src) { if (dst) STN_HIP(hipMemcpyAsync(dst, src, st_bytes, hipMemcpyDeviceToHost, s_)); };
    // per sample: log10 (about 20), the gain computer (11), the detector (2), the clamp and the smoothing (3), the gain 10^x and its product (about 22)
    StageSpan span(*this, "out", "expander_chunks1", 33.0 * samples, samples * 4 + chunks * 4);
    launch_expander_chunks(s_, 1, x, rows, W, sc.n, t, sc.s1, sc.s2, y, nullptr, sc.cmin, sc.ccnt);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s1_end, sc.s1);
    span.next("expander_scan1", chunks * 11 * 2, chunks * 8);
    launch_expander_scan(s_, 1, rows, W, t, sc.s1);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s1_start, sc.s1);
    span.next("expander_chunks2", 36.0 * samples, samples * 4 + chunks * 8);
    launch_expander_chunks(s_, 2, x, rows, W, sc.n, t, sc.s1, sc.s2, y, nullptr, sc.cmin, sc.ccnt);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s2_end, sc.s2);
    span.next("expander_scan2", chunks * 11 * 2, chunks * 8);
    launch_expander_scan(s_, 2, rows, W, t, sc.s2);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s2_start, sc.s2);
    span.next("expander_write", 60.0 * samples, samples * (open ? 12 : 8) + chunks * 16);
    launch_expander_chunks(s_, 3, x, rows, W, sc.n, t, sc.s1, sc.s2, y, open, sc.cmin, sc.ccnt);
    STN_HIP(hipGetLastError());
    span.next("expander_rows", chunks * 2, chunks * 8 + (double)rows * 12);
    launch_expander_rows(s_, rows, W, t, sc.cmin, sc.ccnt, sc.rmin, sc.rcnt);
    STN_HIP(hipGetLastError());
}

// the hook of every fetch path: the finished batch's rows at the output rate (x: the rows the stage starts from, or the rows already in
// y) expanded into y, the fetch scratch
Engine::XpScratch Engine::xp_batch(const float* x, int64_t Wo, float* y) {
    const Batch& b = bt_;
    const int hz = output_rate();
    xp_prepare(xp_, hz, xp_set_);
    bool moved = false;
    char* base = xp_buf_.reserve(*this, xp_layout(nullptr, b.B, Wo).bytes, &moved);
    const XpScratch sc = xp_layout(base, b.B, Wo);
    // row b's valid samples: section 11's span, its reported duration at the output rate; uploaded once per finished batch
    std::vector<int64_t> n = out_spans(Wo, hz);
    if (moved || n != xp_n_ || xp_n_ptr_ != sc.n) {
        xp_n_ = std::move(n);
        xp_n_ptr_ = sc.n;
        STN_HIP(hipMemcpyAsync(sc.n, xp_n_.data(), xp_n_.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
        sync();  // (the upload reads xp_n_, which the next batch's lengths replace; once per finished batch, as cp_batch)
    }
    xp_enqueue(xp_, x, b.B, Wo, sc, y, nullptr, nullptr);
    xp_key_ = XpKey{ed_seq_, hz, fl_gen_, xp_gen_, Wo, xp_buf_.get(), ps_gen_};
    xp_valid_ = true;
    return sc;
}

void Engine::batch_expander(float* min_attenuation_db, int64_t* closed_samples) {
    const int64_t Wo = out_row_len();
    if (!min_attenuation_db && !closed_samples) return;
    if (!expander_on()) {  // nothing is turned down
        if (min_attenuation_db) std::fill(min_attenuation_db, min_attenuation_db + bt_.B, 0.0f);
        if (closed_samples) std::fill(closed_samples, closed_samples + bt_.B, (int64_t)0);
        return;
    }
    // the row results a fetch of this batch under this rate, chain and setting left in xp_buf_ are the report; otherwise the sequence runs
    const XpKey key{ed_seq_, output_rate(), fl_gen_, xp_gen_, Wo, xp_buf_.get(), ps_gen_};
    if (!(xp_valid_ && key == xp_key_)) (void)out_source(Wo);
    const XpScratch sc = xp_layout(xp_buf_.reserve(*this, xp_layout(nullptr, bt_.B, Wo).bytes), bt_.B, Wo);
    if (min_attenuation_db) STN_HIP(hipMemcpyAsync(min_attenuation_db, sc.rmin, (size_t)bt_.B * 4, hipMemcpyDeviceToHost, s_));
    if (closed_samples) STN_HIP(hipMemcpyAsync(closed_samples, sc.rcnt, (size_t)bt_.B * 8, hipMemcpyDeviceToHost, s_));
    sync();
}

void Engine::op_expander(int hz, int rows, int W, const float* x, const stn_expander& c, float* y, XpProbe* probe) {
    STN_HIP(hipSetDevice(device_));
    xp_prepare(op_xp_, hz, c);
    ar_.reset();
    const size_t nx = (size_t)rows * W;
    GuardedRows r(*this, nx, x, probe, probe && probe->x_misalign, probe && probe->in_place);
    float* dop = probe && probe->open ? static_cast<float*>(ar_.alloc(nx * 4)) : nullptr;
    const size_t sc_bytes = xp_layout(nullptr, rows, W).bytes;
    char* sb = static_cast<char*>(ar_.alloc(sc_bytes));
    const XpScratch sc = xp_layout(sb, rows, W);
    if (probe) {
        if (dop) STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dop), 0x7FC00000, nx, s_));
        STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sb), 0x7FC00000, sc_bytes / 4, s_));
    }
    const std::vector<int64_t> nn((size_t)rows, (int64_t)W);
    STN_HIP(hipMemcpyAsync(sc.n, nn.data(), nn.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
    xp_enqueue(op_xp_, r.dx, rows, W, sc, r.dy, dop, probe);
    r.download(y);
    if (dop) STN_HIP(hipMemcpyAsync(probe->open, dop, nx * 4, hipMemcpyDeviceToHost, s_));
    if (probe) {
        probe->guard_ok = r.guards_ok();
        probe->form = expander_staging_form(r.dx, r.dy, W);
    }
    sync();
}

}  // namespace stn
