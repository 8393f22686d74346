// engine_compressor.cpp — the fetch-time dynamic range compressor of a handle: its limits, coefficients and static curve (host only),
// the scan tables and the scratch, the sequence of launches and the op-level entry.  The kernels are kernels_compressor.hip; the hook
// is Engine::out_source (engine_batch.cpp); DESIGN.md section 20 has the contract.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace stn {

namespace {

void fields(const stn_compressor& c, float out[6]) {
    const float v[6] = {c.threshold_db, c.ratio, c.knee_db, c.attack_ms, c.release_ms, c.makeup_db};
    std::copy(v, v + 6, out);
}

bool same_setting(const float a[6], const stn_compressor& c) {
    float b[6];
    fields(c, b);
    return std::equal(a, a + 6, b);
}

// the fp32 values the kernels compute with (and the float64 reference is given): T, S = 1 / ratio - 1, K, makeup
CompCoef static_coef(const stn_compressor& c) {
    CompCoef f{};
    f.T = c.threshold_db;
    f.S = (float)(1.0 / (double)c.ratio - 1.0);
    f.K = c.knee_db;
    f.makeup = c.makeup_db;
    return f;
}

}  // namespace

std::string compressor_check(const stn_compressor* c) {
    if (!c) return "compressor: c is null";
    const Lim lim[6] = {{"threshold_db", c->threshold_db, -60.0f, 0.0f}, {"ratio", c->ratio, 1.0f, 20.0f},       {"knee_db", c->knee_db, 0.0f, 24.0f},
                        {"attack_ms", c->attack_ms, 0.1f, 300.0f},       {"release_ms", c->release_ms, 10.0f, 3000.0f}, {"makeup_db", c->makeup_db, -12.0f, 24.0f}};
    return range_check("compressor", lim);
}

double compressor_k(float ms, int rate_hz) { return -std::expm1(-1000.0 / ((double)ms * (double)rate_hz)); }

double compressor_curve(const stn_compressor& c, double in_db) {
    const CompCoef f = static_coef(c);
    const double T = f.T, S = f.S, K = f.K, d = in_db - T;
    double z;
    if (2.0 * d < -K) z = 0.0;
    else if (K > 0.0 && 2.0 * std::fabs(d) <= K) z = -S * (d + 0.5 * K) * (d + 0.5 * K) / (2.0 * K);
    else z = -S * d;
    return in_db - z + (double)f.makeup;
}

void compressor_table(int hz, const stn_compressor& c, CompTable& t) {
    refuse(compressor_check(&c));
    refuse(rate_check("compressor", hz));
    t.hz = hz;
    fields(c, t.set);
    t.coef = static_coef(c);
    t.coef.kA = (float)compressor_k(c.attack_ms, hz);
    t.coef.kR = (float)compressor_k(c.release_ms, hz);
    // what a chunk of LO_CHUNK samples multiplies a start value by, from the fp32 k the kernels run on, and its powers
    const double D = std::pow(1.0 - (double)t.coef.kR, LO_CHUNK), E = std::pow(1.0 - (double)t.coef.kA, LO_CHUNK);
    t.pw.assign((size_t)2 * LO_SCAN, 0.0);
    double d = D, e = E;
    for (int i = 0; i < LO_SCAN; ++i) {
        t.pw[(size_t)i] = d;
        t.pw[(size_t)LO_SCAN + i] = e;
        d *= D;
        e *= E;
    }
}

void Engine::cp_prepare(CompTable& t, int hz, const stn_compressor& c) {
    if (t.hz == hz && t.dev && same_setting(t.set, c)) return;
    CompTable nt;
    compressor_table(hz, c, nt);
    STN_HIP(hipSetDevice(device_));
    STN_HIP(hipMalloc(reinterpret_cast<void**>(&nt.dev), nt.pw.size() * sizeof(double)));
    STN_HIP(hipMemcpyAsync(nt.dev, nt.pw.data(), nt.pw.size() * sizeof(double), hipMemcpyHostToDevice, s_));
    sync();  // (the upload reads nt's host copy, and a fetch may still be reading the old table)
    if (t.dev) (void)hipFree(t.dev);
    t = std::move(nt);
}

void Engine::cp_release() {
    for (CompTable* t : {&cp_, &op_cp_})
        if (t->dev) { (void)hipFree(t->dev); t->dev = nullptr; }
}

void Engine::set_compressor(bool on, const stn_compressor* c) {
    if (!on) {
        if (cp_on_) ++cp_gen_;
        cp_on_ = false;
        return;
    }
    refuse(compressor_check(c));
    float now[6];
    fields(cp_set_, now);
    if (cp_on_ && same_setting(now, *c)) return;
    cp_set_ = *c;
    cp_on_ = true;
    ++cp_gen_;
}

Engine::CpScratch Engine::cp_layout(char* base, int64_t rows, int64_t W) {
    const size_t nc = (size_t)rows * (size_t)lo_chunks(W);
    Carve c{base};
    CpScratch sc{};
    sc.s1 = c.take<float>(nc);
    sc.s2 = c.take<float>(nc);
    sc.cmax = c.take<float>(nc);
    sc.rmax = c.take<float>((size_t)rows);
    sc.n = c.take<int64_t>((size_t)rows);
    sc.bytes = c.off;
    return sc;
}

void Engine::cp_enqueue(const CompTable& t, const float* x, int64_t rows, int64_t W, const CpScratch& sc, float* y, float* gr, CpProbe* probe) {
    const double samples = (double)rows * W, chunks = (double)rows * lo_chunks(W);
    const size_t st_bytes = (size_t)rows * (size_t)lo_chunks(W) * 4;
    auto out = [&](float* dst, const float* src) { if (dst) STN_HIP(hipMemcpyAsync(dst, src, st_bytes, hipMemcpyDeviceToHost, s_)); };
    // per sample: log10 (about 20), the gain computer (8), the detector (3), the smoothing (2), the gain 10^x and its product (about 22)
    StageSpan span(*this, "out", "compressor_chunks1", 31.0 * samples, samples * 4 + chunks * 4);
    launch_compressor_chunks(s_, 1, x, rows, W, sc.n, t, sc.s1, sc.s2, y, nullptr, sc.cmax);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s1_end, sc.s1);
    span.next("compressor_scan1", chunks * 11 * 2, chunks * 8);
    launch_compressor_scan(s_, 1, rows, W, t, sc.s1);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s1_start, sc.s1);
    span.next("compressor_chunks2", 33.0 * samples, samples * 4 + chunks * 8);
    launch_compressor_chunks(s_, 2, x, rows, W, sc.n, t, sc.s1, sc.s2, y, nullptr, sc.cmax);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s2_end, sc.s2);
    span.next("compressor_scan2", chunks * 11 * 2, chunks * 8);
    launch_compressor_scan(s_, 2, rows, W, t, sc.s2);
    STN_HIP(hipGetLastError());
    if (probe) out(probe->s2_start, sc.s2);
    span.next("compressor_write", 56.0 * samples, samples * (gr ? 12 : 8) + chunks * 12);
    launch_compressor_chunks(s_, 3, x, rows, W, sc.n, t, sc.s1, sc.s2, y, gr, sc.cmax);
    STN_HIP(hipGetLastError());
    span.next("compressor_rowmax", chunks, chunks * 4 + (double)rows * 4);
    launch_compressor_rowmax(s_, rows, W, sc.cmax, sc.rmax);
    STN_HIP(hipGetLastError());
}

// the hook of every fetch path: the finished batch's rows at the output rate (x: b.wav, or the rows already in y) compressed into y, the
// fetch scratch
Engine::CpScratch Engine::cp_batch(const float* x, int64_t Wo, float* y) {
    const Batch& b = bt_;
    const int hz = output_rate();
    cp_prepare(cp_, hz, cp_set_);
    bool moved = false;
    char* base = cp_buf_.reserve(*this, cp_layout(nullptr, b.B, Wo).bytes, &moved);
    const CpScratch sc = cp_layout(base, b.B, Wo);
    // row b's valid samples: section 11's span, its reported duration at the output rate; uploaded once per finished batch
    std::vector<int64_t> n = out_spans(Wo, hz);
    if (moved || n != cp_n_ || cp_n_ptr_ != sc.n) {
        cp_n_ = std::move(n);
        cp_n_ptr_ = sc.n;
        STN_HIP(hipMemcpyAsync(sc.n, cp_n_.data(), cp_n_.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
        sync();  // (the upload reads cp_n_, which the next batch's lengths replace; once per finished batch, as fl_batch)
    }
    cp_enqueue(cp_, x, b.B, Wo, sc, y, nullptr, nullptr);
    cp_key_ = CpKey{ed_seq_, hz, fl_gen_, cp_gen_, Wo, cp_buf_.get(), ds_gen_, ps_gen_, xp_gen_};
    cp_valid_ = true;
    return sc;
}

void Engine::batch_compressor(float* max_reduction_db) {
    const int64_t Wo = out_row_len();
    if (!max_reduction_db) return;
    if (!compressor_on()) {  // nothing is turned down
        std::fill(max_reduction_db, max_reduction_db + bt_.B, 0.0f);
        return;
    }
    // the row maxima a fetch of this batch under this rate, chain and setting left in cp_buf_ are the report; otherwise the sequence runs
    const CpKey key{ed_seq_, output_rate(), fl_gen_, cp_gen_, Wo, cp_buf_.get(), ds_gen_, ps_gen_, xp_gen_};
    if (!(cp_valid_ && key == cp_key_)) (void)out_source(Wo);
    const CpScratch sc = cp_layout(cp_buf_.reserve(*this, cp_layout(nullptr, bt_.B, Wo).bytes), bt_.B, Wo);
    STN_HIP(hipMemcpyAsync(max_reduction_db, sc.rmax, (size_t)bt_.B * 4, hipMemcpyDeviceToHost, s_));
    sync();
}

void Engine::op_compressor(int hz, int rows, int W, const float* x, const stn_compressor& c, float* y, CpProbe* probe) {
    STN_HIP(hipSetDevice(device_));
    cp_prepare(op_cp_, hz, c);
    ar_.reset();
    const size_t nx = (size_t)rows * W;
    GuardedRows r(*this, nx, x, probe, probe && probe->x_misalign, probe && probe->in_place);
    float* dgr = probe && probe->gr ? static_cast<float*>(ar_.alloc(nx * 4)) : nullptr;
    const size_t sc_bytes = cp_layout(nullptr, rows, W).bytes;
    char* sb = static_cast<char*>(ar_.alloc(sc_bytes));
    const CpScratch sc = cp_layout(sb, rows, W);
    if (probe) {
        if (dgr) STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(dgr), 0x7FC00000, nx, s_));
        STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sb), 0x7FC00000, sc_bytes / 4, s_));
    }
    const std::vector<int64_t> nn((size_t)rows, (int64_t)W);
    STN_HIP(hipMemcpyAsync(sc.n, nn.data(), nn.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
    cp_enqueue(op_cp_, r.dx, rows, W, sc, r.dy, dgr, probe);
    r.download(y);
    if (dgr) STN_HIP(hipMemcpyAsync(probe->gr, dgr, nx * 4, hipMemcpyDeviceToHost, s_));
    if (probe) {
        probe->guard_ok = r.guards_ok();
        probe->form = compressor_staging_form(r.dx, r.dy, W);
    }
    sync();
}

}  // namespace stn
