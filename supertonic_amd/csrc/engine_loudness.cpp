// engine_loudness.cpp — loudness normalization of a handle's fetches: the K-weighting design (host only), the scan's power table, the
// measurement's scratch, and the measurement the output stage (engine_batch.cpp) and batch_loudness share.  The kernels are
// kernels_loudness.hip; DESIGN.md section 11 has the contract.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace stn {

std::string rate_check(const char* what, int hz) {
    if (hz < LO_MIN_HZ || hz > LO_MAX_HZ)
        return std::string(what) + ": sample rate must be in [" + std::to_string(LO_MIN_HZ) + ", " + std::to_string(LO_MAX_HZ) + "] Hz (got " + std::to_string(hz) + ")";
    return "";
}

std::string loudness_check(const float* target, float ceiling) {
    if (target && !(*target >= -60.0f && *target <= 0.0f)) return "loudness target " + std::to_string(*target) + " LUFS: must be in [-60, 0]";
    if (!(ceiling >= -30.0f && ceiling <= 0.0f)) return "loudness peak ceiling " + std::to_string(ceiling) + " dBFS: must be in [-30, 0]";
    return "";
}

std::vector<int64_t> spans(const char* who, int rows, int W, const int64_t* n) {
    std::vector<int64_t> nn((size_t)rows, (int64_t)W);
    for (int r = 0; r < rows && n; ++r) {
        if (n[r] < 0 || n[r] > W) throw std::invalid_argument(std::string(who) + ": n[" + std::to_string(r) + "] = " + std::to_string(n[r]) + " outside [0, W]");
        nn[(size_t)r] = n[r];
    }
    return nn;
}

// BS.1770-4 K-weighting at any rate: the analog prototypes of the standard's 48 kHz table (libebur128's derivation), bilinear-transformed
// at hz.  At 48 kHz this is the published table to 1e-15.
std::string kweighting_design(int hz, KWeighting& k) {
    const std::string why = rate_check("loudness", hz);
    if (!why.empty()) return why;
    const double fs = hz;
    {  // high shelf, +4 dB above ~1.7 kHz (the head's acoustic effect)
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(M_PI * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        k.shelf_b[0] = (Vh + Vb * K / Q + K * K) / a0;
        k.shelf_b[1] = 2.0 * (K * K - Vh) / a0;
        k.shelf_b[2] = (Vh - Vb * K / Q + K * K) / a0;
        k.shelf_a[0] = 1.0;
        k.shelf_a[1] = 2.0 * (K * K - 1.0) / a0;
        k.shelf_a[2] = (1.0 - K / Q + K * K) / a0;
    }
    {  // RLB high-pass at ~38 Hz
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(M_PI * f0 / fs), a0 = 1.0 + K / Q + K * K;
        k.hp_b[0] = 1.0; k.hp_b[1] = -2.0; k.hp_b[2] = 1.0;
        k.hp_a[0] = 1.0;
        k.hp_a[1] = 2.0 * (K * K - 1.0) / a0;
        k.hp_a[2] = (1.0 - K / Q + K * K) / a0;
    }
    return "";
}

// M = A^LO_CHUNK of the state transition A the fp32 coefficients define (state s1 s2 t1 t2 of the two transposed direct form II
// sections, zero input), with its powers M^1 .. M^LO_SCAN, in double: the scan reads them as they are.
void cascade_powers(const LoudCoef& coef, std::vector<double>& mpow) {
    double c[10];
    for (int i = 0; i < 10; ++i) c[i] = coef.c[i];
    // v = s1; s1' = -a1 v + s2; s2' = -a2 v; y = c0 v + t1; t1' = c1 v - d1 y + t2; t2' = c2 v - d2 y
    const double A[16] = {-c[3], 1, 0, 0,
                          -c[4], 0, 0, 0,
                          c[6] - c[8] * c[5], 0, -c[8], 1,
                          c[7] - c[9] * c[5], 0, -c[9], 0};
    auto mul = [](const double* X, const double* Y, double* Z) {
        for (int r = 0; r < 4; ++r)
            for (int q = 0; q < 4; ++q) {
                double s = 0.0;
                for (int j = 0; j < 4; ++j) s += X[r * 4 + j] * Y[j * 4 + q];
                Z[r * 4 + q] = s;
            }
    };
    double M[16], T[16];
    std::memcpy(M, A, sizeof(M));
    for (int i = 1; i < LO_CHUNK; ++i) { mul(M, A, T); std::memcpy(M, T, sizeof(M)); }
    mpow.assign((size_t)LO_SCAN * 16, 0.0);
    double P[16];
    std::memcpy(P, M, sizeof(P));
    for (int i = 0; i < LO_SCAN; ++i) {
        for (int j = 0; j < 16; ++j) mpow[(size_t)i * 16 + j] = P[j];
        mul(P, M, T);
        std::memcpy(P, T, sizeof(P));
    }
}

// The kernels' fp32 coefficients and the scan's powers for them
std::string loudness_design(int hz, LoudTable& t) {
    KWeighting k;
    const std::string why = kweighting_design(hz, k);
    if (!why.empty()) return why;
    t.hz = hz;
    t.hop = (hz + 5) / 10;
    const double src[10] = {k.shelf_b[0], k.shelf_b[1], k.shelf_b[2], k.shelf_a[1], k.shelf_a[2], k.hp_b[0], k.hp_b[1], k.hp_b[2], k.hp_a[1], k.hp_a[2]};
    for (int i = 0; i < 10; ++i) t.coef.c[i] = (float)src[i];
    cascade_powers(t.coef, t.mpow);
    return "";
}

void Engine::lo_prepare(OnDevice<LoudTable>& m, int hz) {
    if (m.t.dev && m.t.hz == hz) return;
    LoudTable n;
    refuse(loudness_design(hz, n));
    n.dev = m.dev[0].put(*this, n.mpow);
    m.t = std::move(n);
}

void Engine::set_loudness(bool on, float target, float ceiling) {
    refuse(loudness_check(&target, ceiling));
    lo_on_ = on;
    lo_target_ = target;
    lo_ceiling_ = ceiling;
}

void Engine::get_loudness(int* on, float* target, float* ceiling) const {
    if (on) *on = lo_on_ ? 1 : 0;
    if (target) *target = lo_target_;
    if (ceiling) *ceiling = lo_ceiling_;
}

Engine::LoScratch Engine::lo_layout(char* base, int64_t rows, int64_t W) {
    const size_t nc = (size_t)rows * (size_t)lo_chunks(W);
    Carve c{base};
    LoScratch sc{};
    sc.st = c.take<float>(nc * 4);
    sc.pk = c.take<float>(nc);
    sc.pa = c.take<float>(nc);
    sc.pb = c.take<float>(nc);
    sc.res = c.take<float>((size_t)rows * 3);
    if (base) sc.out = {sc.res, sc.res + rows, sc.res + 2 * rows, nullptr};
    sc.bytes = c.off;
    return sc;
}

void Engine::lo_measure(const LoudTable& t, const float* x, int64_t rows, int64_t W, const int64_t* n, const LoScratch& sc, int64_t max_seg, bool on,
                        float target, float ceiling, float* st_end, bool true_peak) {
    const double samples = (double)rows * W, chunks = (double)rows * lo_chunks(W);
    StageSpan span(*this, "out", "loudness", 20.0 * samples, samples * 4 + chunks * 20);
    auto next = [&](double flops, double bytes) { STN_HIP(hipGetLastError()); span.next("loudness", flops, bytes); };  // (the launch before it is checked)
    launch_loudness_chunks(s_, false, x, rows, W, n, t, sc.st, sc.pk, sc.pa, sc.pb);
    if (st_end) STN_HIP(hipMemcpyAsync(st_end, sc.st, (size_t)rows * (size_t)lo_chunks(W) * 16, hipMemcpyDeviceToHost, s_));
    next(chunks * 32.0 * 11, chunks * 32);
    launch_loudness_scan(s_, rows, W, n, t, sc.st);
    next(22.0 * samples, samples * 4 + chunks * 24);
    launch_loudness_chunks(s_, true, x, rows, W, n, t, sc.st, sc.pk, sc.pa, sc.pb);
    if (true_peak) {  // section 16: pk becomes the per-chunk true peaks, and the gate, untouched, caps the gain by the row's true peak
        STN_HIP(hipGetLastError());
        span.next("true_peak", 97.0 * samples, samples * 4 + chunks * 4);
        launch_truepeak(s_, x, rows, W, n, nullptr, sc.pk, nullptr);
    }
    next(chunks * 2, chunks * 12 + (double)rows * 12);
    launch_loudness_gate(s_, rows, W, n, t, sc.pk, sc.pa, sc.pb, max_seg, on, target, ceiling, sc.res);
    STN_HIP(hipGetLastError());
}

void Engine::lo_read_back(const LoRes& m, size_t n, float* lufs, float* peak, float* gain) {
    if (lufs) STN_HIP(hipMemcpyAsync(lufs, m.lufs, n * 4, hipMemcpyDeviceToHost, s_));
    if (peak) STN_HIP(hipMemcpyAsync(peak, m.peak, n * 4, hipMemcpyDeviceToHost, s_));
    if (gain) STN_HIP(hipMemcpyAsync(gain, m.gain, n * 4, hipMemcpyDeviceToHost, s_));
}

// row b's span: its reported duration (after /speed) at hz, as the reference's hosts cut the file, inside [0, W]
std::vector<int64_t> Engine::out_spans(int64_t W, int hz) const {
    std::vector<int64_t> n((size_t)bt_.B);
    for (int i = 0; i < bt_.B; ++i) n[(size_t)i] = std::max<int64_t>(0, std::min<int64_t>(W, (int64_t)(reported_dur_[(size_t)i] * (float)hz)));
    return n;
}

// The upload rule of the span table, stated once:
//  - how often: once per finished batch (ed_seq_) and per (hz, W); the fetches, reports and stages in between find the entry and
//    upload nothing.  Two entries, so that a fetch with pitch and a rate set finds both of its keys.  A block that moved (more rows
//    than ever) holds nothing, and another row count puts the entries elsewhere in it.
//  - no host wait on the way: the upload is enqueued and the fetch goes on (fetch_*_begin stays asynchronous).
//  - the host copy an upload reads is e.host, an engine member, replaced only behind a drained stream: the batch_upload of a new
//    batch has drained it since, and a replacement nothing has drained for (another rate within the same batch) waits first.
const Engine::BatchSpans& Engine::batch_spans(int hz, int64_t W) {
    const size_t B = (size_t)bt_.B;
    Carve size{nullptr};
    for (size_t k = 0; k < std::size(sp_); ++k) size.take<int64_t>(2 * B);
    bool moved = false;
    Carve c{sp_buf_.reserve(*this, size.off, &moved)};
    if (moved) for (BatchSpans& e : sp_) e.dev = RowSpans();
    int64_t* d = nullptr;
    const size_t slot = hz == a_.sample_rate && W == native_row_len() ? 0 : 1;
    for (size_t k = 0; k <= slot; ++k) d = c.take<int64_t>(2 * B);
    BatchSpans& e = sp_[slot];
    if (e.seq == ed_seq_ && e.hz == hz && e.W == W && e.host.size() == 2 * B && e.dev.n == d) return e;
    if (e.drains == drains_) sync();
    e.host = out_spans(W, hz);
    e.host.resize(2 * B, W);
    STN_HIP(hipMemcpyAsync(d, e.host.data(), e.host.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
    ++sp_uploads_;
    e.dev = {d, d + B};
    e.seq = ed_seq_; e.hz = hz; e.W = W; e.drains = drains_;
    return e;
}

Engine::LoRes Engine::lo_batch(const float* x, int64_t Wo, bool on) {
    const Batch& b = bt_;
    const int hz = output_rate();
    lo_prepare(lo_, hz);
    const BatchSpans& sp = batch_spans(hz, Wo);
    // (the limiter, when active, enforces the ceiling: DESIGN.md section 15)
    return lo_rows(lo_.t, x, b.B, Wo, sp.dev.n, lr_max_seg(lo_.t, sp.host.data(), (size_t)b.B), on, lo_target_, lo_cap(), lo_true_peak());
}

Engine::LoRes Engine::lo_rows(const LoudTable& t, const float* x, int64_t rows, int64_t W, const int64_t* n, int64_t max_seg, bool on, float target,
                              float ceiling, bool true_peak) {
    const LoScratch sc = lo_scratch(rows, W);
    lo_measure(t, x, rows, W, n, sc, max_seg, on, target, ceiling, nullptr, true_peak);
    LoRes m = sc.out;
    m.n = n;
    return m;
}

void Engine::batch_loudness(float* lufs, float* peak, float* gain) {
    const int64_t Wo = out_row_len();
    lo_read_back(lo_batch(out_source(Wo), Wo, lo_on_), (size_t)bt_.B, lufs, peak, gain);
    sync();
}

const int64_t* Engine::lo_op(int hz, int rows, int W, const float* x, const int64_t* n, bool on, float target, float ceiling, LoProbe* probe, float* lufs,
                             float* peak, float* gain) {
    OpScope op(*this);
    lo_prepare(op_lo_, hz);
    const std::vector<int64_t> nn = spans("op_loudness", rows, W, n);
    const int64_t max_seg = lr_max_seg(op_lo_.t, nn.data(), nn.size());
    const float* dx = op.up(x, (size_t)rows * W, probe && probe->x_misalign ? 1 : 0);
    const LoScratch sc = lo_scratch(rows, W);
    if (probe) op.poison(sc.st, sc.bytes / 4);  // every per-chunk array and the results
    const int64_t* dn = op.spans(rows, W, nn).n;
    lo_measure(op_lo_.t, dx, rows, W, dn, sc, max_seg, on, target, ceiling, probe ? probe->st_end : nullptr);
    lo_read_back(sc.out, (size_t)rows, lufs, peak, gain);
    if (probe) {
        const size_t nc = (size_t)rows * (size_t)lo_chunks(W);
        op.down(probe->st_start, sc.st, nc * 4);
        op.down(probe->pk, sc.pk, nc);
        op.down(probe->pa, sc.pa, nc);
        op.down(probe->pb, sc.pb, nc);
        probe->form = chunk_staging_form(dx, nullptr, W);
    }
    sync();
    return dn;
}

void Engine::op_loudness(int hz, int rows, int W, const float* x, const int64_t* n, float* lufs, float* peak) {
    lo_op(hz, rows, W, x, n, false, lo_target_, lo_ceiling_, nullptr, lufs, peak, nullptr);
}

// ---- the loudness report

int64_t Engine::lr_max_seg(const LoudTable& t, const int64_t* n, size_t rows) {
    int64_t m = 0;
    for (size_t r = 0; r < rows; ++r) m = std::max<int64_t>(m, n[r] / t.hop);
    return m;
}

void Engine::lr_report(const LoudTable& t, int64_t rows, int64_t W, const int64_t* n, int64_t max_seg, float* m_max, float* s_max, float* lra, int32_t* n_st) {
    refuse(loudness_range_check(max_seg));
    const LoScratch sc = lo_scratch(rows, W);  // (as the measurement carved it: the same size moves nothing)
    Carve sz{nullptr};
    sz.take<float>((size_t)rows * 3);
    sz.take<int32_t>((size_t)rows);
    Carve c{lr_buf_.reserve(*this, sz.off)};
    float* res = c.take<float>((size_t)rows * 3);
    int32_t* nst = c.take<int32_t>((size_t)rows);
    {
        const double chunks = (double)rows * lo_chunks(W);
        StageSpan span(*this, "out", "loudness_range", chunks * 2, chunks * 8 + (double)rows * 16);
        launch_loudness_range(s_, rows, W, n, t, sc.pa, sc.pb, max_seg, res, nst);
    }
    STN_HIP(hipGetLastError());
    const size_t nr = (size_t)rows;
    if (m_max) STN_HIP(hipMemcpyAsync(m_max, res, nr * 4, hipMemcpyDeviceToHost, s_));
    if (s_max) STN_HIP(hipMemcpyAsync(s_max, res + nr, nr * 4, hipMemcpyDeviceToHost, s_));
    if (lra) STN_HIP(hipMemcpyAsync(lra, res + 2 * nr, nr * 4, hipMemcpyDeviceToHost, s_));
    if (n_st) STN_HIP(hipMemcpyAsync(n_st, nst, nr * 4, hipMemcpyDeviceToHost, s_));
}

void Engine::batch_loudness_range(float* m_max, float* s_max, float* lra, int32_t* n_st) {
    const int64_t Wo = out_row_len();
    const LoRes m = lo_batch(out_source(Wo), Wo, lo_on_);
    lr_report(lo_.t, bt_.B, Wo, m.n, lr_max_seg(lo_.t, batch_spans(output_rate(), Wo).host.data(), (size_t)bt_.B), m_max, s_max, lra, n_st);
    sync();
}

void Engine::op_loudness_range(int hz, int rows, int W, const float* x, const int64_t* n, float* m_max, float* s_max, float* lra, int32_t* n_st) {
    refuse(rate_check("loudness", hz));
    int64_t max_seg = 0;
    for (int64_t v : spans("op_loudness_range", rows, W, n)) max_seg = std::max<int64_t>(max_seg, v / ((hz + 5) / 10));
    refuse(loudness_range_check(max_seg));  // (before the upload and the measurement, which a longer row passes)
    const int64_t* dn = lo_op(hz, rows, W, x, n, false, lo_target_, lo_ceiling_, nullptr, nullptr, nullptr, nullptr);
    lr_report(op_lo_.t, rows, W, dn, max_seg, m_max, s_max, lra, n_st);
    sync();
}

void Engine::op_loudness_ex(int hz, int rows, int W, const float* x, const int64_t* n, bool on, float target, float ceiling, LoProbe& probe,
                            float* lufs, float* peak, float* gain) {
    lo_op(hz, rows, W, x, n, on, target, ceiling, &probe, lufs, peak, gain);
}

}  // namespace stn
