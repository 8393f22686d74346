// engine_edges.cpp — trimming leading and trailing silence by level at fetch time: the setting, the fade window (host only), the
// detection's scratch, and the edges cached per finished batch and (rate, parameters) that the output stage (engine_batch.cpp),
// batch_silence_edges and the join plan share.  The kernels are kernels_edges.hip and join_trim_rows_kernel (kernels_output.hip);
// DESIGN.md section 14 has the contract.
#include "engine.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace stn {

std::string silence_check(float top_db, float keep_ms, float fade_ms) {
    if (!(top_db >= 1.0f && top_db <= 120.0f)) return "silence trim top_db " + std::to_string(top_db) + " dB: must be in [1, 120]";
    if (!(keep_ms >= 0.0f && keep_ms <= 1000.0f)) return "silence trim keep " + std::to_string(keep_ms) + " ms: must be in [0, 1000]";
    if (!(fade_ms >= 0.0f && fade_ms <= 50.0f)) return "silence trim fade " + std::to_string(fade_ms) + " ms: must be in [0, 50]";
    return "";
}
// (int64)(ms * hz / 1000 + 0.5), in double: the keep and the fade length in samples
int64_t silence_samples(int hz, float ms) { return (int64_t)((double)ms * (double)hz / 1000.0 + 0.5); }

// w[j] = float32(0.5 - 0.5 cos(pi (j + 0.5) / Fd)), j < Fd
std::vector<float> silence_fade_window(int hz, float fade_ms) {
    const int64_t fd = silence_samples(hz, fade_ms);
    std::vector<float> w((size_t)fd);
    for (int64_t j = 0; j < fd; ++j) w[(size_t)j] = (float)(0.5 - 0.5 * std::cos(M_PI * ((double)j + 0.5) / (double)fd));
    return w;
}

static std::string silence_rate_check(int hz) {
    if (hz < LO_MIN_HZ || hz > LO_MAX_HZ)
        return "silence trim: sample rate must be in [" + std::to_string(LO_MIN_HZ) + ", " + std::to_string(LO_MAX_HZ) + "] Hz (got " + std::to_string(hz) + ")";
    return "";
}

void Engine::set_silence_trim(bool on, float top_db, float keep_ms, float fade_ms) {
    const std::string why = silence_check(top_db, keep_ms, fade_ms);
    if (!why.empty()) throw std::invalid_argument(why);
    st_on_ = on;
    st_db_ = top_db;
    st_keep_ = keep_ms;
    st_fade_ = fade_ms;
}

void Engine::get_silence_trim(int* on, float* top_db, float* keep_ms, float* fade_ms) const {
    if (on) *on = st_on_ ? 1 : 0;
    if (top_db) *top_db = st_db_;
    if (keep_ms) *keep_ms = st_keep_;
    if (fade_ms) *fade_ms = st_fade_;
}

void Engine::ed_release() {
    if (ed_buf_) (void)hipFree(ed_buf_);
    if (st_win_) (void)hipFree(st_win_);
    ed_buf_ = nullptr; ed_buf_cap_ = 0;
    st_win_ = nullptr; st_win_cap_ = 0; st_win_hz_ = 0; st_win_ms_ = -1.0f;
    ed_valid_ = ed_host_valid_ = false;
}

// uploaded once per (rate, fade_ms); at least one float, so that the kernel's pointer is never null
const float* Engine::st_window(int hz) {
    if (st_win_ && st_win_hz_ == hz && st_win_ms_ == st_fade_) return st_win_;
    const std::vector<float> w = silence_fade_window(hz, st_fade_);
    const size_t need = std::max<size_t>(w.size(), 1);
    if (!st_win_ || need > st_win_cap_) {
        sync();  // a fetch may still be reading the old window
        if (st_win_) (void)hipFree(st_win_);
        st_win_ = nullptr; st_win_cap_ = 0;
        STN_HIP(hipMalloc(reinterpret_cast<void**>(&st_win_), need * sizeof(float)));
        st_win_cap_ = need;
    } else {
        sync();
    }
    if (!w.empty()) STN_HIP(hipMemcpy(st_win_, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    st_win_hz_ = hz; st_win_ms_ = st_fade_;
    return st_win_;
}

// grow-only scratch (not part of the resident batch: growing it re-keys no captured graph): per chunk the two frame shares, per frame
// the level, per row the edges, the span and the one-member programme of the per-row trimmed fetch
static size_t ed_up(size_t b) { return (b + 255) / 256 * 256; }
static size_t ed_layout(int64_t rows, int64_t W, int hz, size_t* o) {
    const size_t nc = (size_t)rows * (size_t)ed_chunks(W), nf = (size_t)rows * (size_t)edges_frames(W, hz);
    o[0] = 0;                                  // pa
    o[1] = o[0] + ed_up(nc * 4);               // pb
    o[2] = o[1] + ed_up(nc * 4);               // lev
    o[3] = o[2] + ed_up(nf * 8);               // edges
    o[4] = o[3] + ed_up((size_t)rows * 16);    // n
    o[5] = o[4] + ed_up((size_t)rows * 8);     // seg
    o[6] = o[5] + ed_up((size_t)rows * sizeof(JoinSegT));  // prog
    return o[6] + ed_up((size_t)rows * sizeof(JoinProg));
}

Engine::EdScratch Engine::ed_scratch(int64_t rows, int64_t W, int hz) {
    size_t o[7];
    const size_t need = ed_layout(rows, W, hz, o);
    if (!ed_buf_ || need > ed_buf_cap_) {
        sync();  // the previous fetch may still be reading it
        if (ed_buf_) (void)hipFree(ed_buf_);
        ed_buf_ = nullptr; ed_buf_cap_ = 0;
        ed_valid_ = ed_host_valid_ = false;
        STN_HIP(hipMalloc(reinterpret_cast<void**>(&ed_buf_), need + need / 4));
        ed_buf_cap_ = need + need / 4;
    }
    EdScratch sc;
    sc.pa = reinterpret_cast<float*>(ed_buf_ + o[0]);
    sc.pb = reinterpret_cast<float*>(ed_buf_ + o[1]);
    sc.lev = reinterpret_cast<double*>(ed_buf_ + o[2]);
    sc.edges = reinterpret_cast<int64_t*>(ed_buf_ + o[3]);
    sc.n = reinterpret_cast<int64_t*>(ed_buf_ + o[4]);
    sc.seg = reinterpret_cast<JoinSegT*>(ed_buf_ + o[5]);
    sc.prog = reinterpret_cast<JoinProg*>(ed_buf_ + o[6]);
    return sc;
}

Engine::EdScratch Engine::ed_batch(const float* x, int64_t Wo) {
    const Batch& b = bt_;
    const int hz = output_rate();
    const std::string why = silence_rate_check(hz);
    if (!why.empty()) throw std::invalid_argument(why);
    const EdScratch sc = ed_scratch(b.B, Wo, hz);
    const EdKey key{ed_seq_, hz, st_db_, st_keep_, st_fade_, Wo, ed_buf_};
    if (ed_valid_ && key == ed_key_) return sc;
    // row b's span: section 11's, its reported duration at the output rate
    ed_n_.resize((size_t)b.B);
    for (int i = 0; i < b.B; ++i) ed_n_[(size_t)i] = std::max<int64_t>(0, std::min<int64_t>(Wo, (int64_t)(reported_dur_[(size_t)i] * (float)hz)));
    STN_HIP(hipMemcpyAsync(sc.n, ed_n_.data(), ed_n_.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
    {
        const double samples = (double)b.B * Wo;
        const double chunks = (double)b.B * ed_chunks(Wo);
        StageSpan span(*this, "out", "edges_frames", 2.0 * samples, samples * 4 + chunks * 8);
        launch_edges_frames(s_, x, b.B, Wo, sc.n, hz, sc.pa, sc.pb);
        span.next("edges_rows", chunks, chunks * 8 + (double)b.B * edges_frames(Wo, hz) * 16);
        launch_edges_rows(s_, b.B, Wo, sc.n, hz, (double)st_db_, silence_samples(hz, st_keep_), silence_samples(hz, st_fade_), sc.pa, sc.pb, sc.lev,
                          sc.edges, sc.seg, sc.prog);
    }
    STN_HIP(hipGetLastError());
    ed_key_ = key;
    ed_valid_ = true;
    ed_host_valid_ = false;
    return sc;
}

const std::vector<int64_t>& Engine::ed_batch_host() {
    const int64_t Wo = out_row_len();
    const EdKey key{ed_seq_, output_rate(), st_db_, st_keep_, st_fade_, Wo, ed_buf_};
    if (ed_valid_ && ed_host_valid_ && key == ed_key_) return ed_host_;
    const EdScratch sc = (ed_valid_ && key == ed_key_) ? ed_scratch(bt_.B, Wo, output_rate()) : ed_batch(out_source(Wo), Wo);
    ed_host_.resize((size_t)bt_.B * 2);
    STN_HIP(hipMemcpyAsync(ed_host_.data(), sc.edges, ed_host_.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s_));
    sync();
    ed_host_valid_ = true;
    return ed_host_;
}

void Engine::batch_silence_edges(int64_t* start, int64_t* end) {
    const std::vector<int64_t>& e = ed_batch_host();
    for (int i = 0; i < bt_.B; ++i) {
        if (start) start[i] = e[(size_t)i * 2];
        if (end) end[i] = e[(size_t)i * 2 + 1];
    }
}

void Engine::op_silence_edges(int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, int64_t* start, int64_t* end) {
    op_silence_trim(hz, rows, W, x, n, top_db, keep_ms, 0.0f, nullptr, ENC_F32, nullptr, start, end);
}

void Engine::op_silence_trim(int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, float fade_ms, const float* gain,
                             int enc, void* y, int64_t* start, int64_t* end) {
    STN_HIP(hipSetDevice(device_));
    std::string why = silence_check(top_db, keep_ms, fade_ms);
    if (why.empty()) why = silence_rate_check(hz);
    if (!why.empty()) throw std::invalid_argument(why);
    const int eb = enc_bytes(enc);
    if (eb == 0) throw std::invalid_argument("unknown sample encoding " + std::to_string(enc));
    std::vector<int64_t> nn((size_t)rows, (int64_t)W);
    for (int r = 0; r < rows && n; ++r) {
        if (n[r] < 0 || n[r] > W) throw std::invalid_argument("op_silence: n[" + std::to_string(r) + "] = " + std::to_string(n[r]) + " outside [0, W]");
        nn[(size_t)r] = n[r];
    }
    ar_.reset();
    size_t o[7];
    const size_t need = ed_layout(rows, W, hz, o);
    char* base = static_cast<char*>(ar_.alloc(need));
    const size_t nx = (size_t)rows * W;
    float* dx = static_cast<float*>(ar_.alloc(nx * 4));
    int64_t* dn = reinterpret_cast<int64_t*>(base + o[4]);
    int64_t* de = reinterpret_cast<int64_t*>(base + o[3]);
    JoinSegT* seg = reinterpret_cast<JoinSegT*>(base + o[5]);
    JoinProg* prog = reinterpret_cast<JoinProg*>(base + o[6]);
    STN_HIP(hipMemcpyAsync(dx, x, nx * 4, hipMemcpyHostToDevice, s_));
    STN_HIP(hipMemcpyAsync(dn, nn.data(), nn.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
    const int64_t fd = silence_samples(hz, fade_ms);
    float* pa = reinterpret_cast<float*>(base + o[0]);
    float* pb = reinterpret_cast<float*>(base + o[1]);
    launch_edges_frames(s_, dx, rows, W, dn, hz, pa, pb);
    launch_edges_rows(s_, rows, W, dn, hz, (double)top_db, silence_samples(hz, keep_ms), fd, pa, pb, reinterpret_cast<double*>(base + o[2]), de, seg, prog);
    STN_HIP(hipGetLastError());
    std::vector<int64_t> e((size_t)rows * 2);
    STN_HIP(hipMemcpyAsync(e.data(), de, e.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s_));
    if (y) {
        const std::vector<float> w = silence_fade_window(hz, fade_ms);
        float* dw = static_cast<float*>(ar_.alloc(std::max<size_t>(w.size(), 1) * 4));
        if (!w.empty()) STN_HIP(hipMemcpyAsync(dw, w.data(), w.size() * 4, hipMemcpyHostToDevice, s_));
        float* dg = nullptr;
        if (gain) {
            dg = static_cast<float*>(ar_.alloc((size_t)rows * 4));
            STN_HIP(hipMemcpyAsync(dg, gain, (size_t)rows * 4, hipMemcpyHostToDevice, s_));
        }
        const int64_t Ws = ((int64_t)W + 15) / 16 * 16;  // rows 16-byte aligned in every encoding: the store runs full width
        void* dy = ar_.alloc((size_t)rows * Ws * eb);
        launch_join_trim_rows(s_, dx, W, seg, prog, rows, W, dg, dw, enc, dy, Ws);
        STN_HIP(hipGetLastError());
        STN_HIP(hipMemcpy2DAsync(y, (size_t)W * eb, dy, (size_t)Ws * eb, (size_t)W * eb, (size_t)rows, hipMemcpyDeviceToHost, s_));
    }
    sync();  // (w, nn and e are read or written by the copies above until here)
    for (int r = 0; r < rows; ++r) {
        if (start) start[r] = e[(size_t)r * 2];
        if (end) end[r] = e[(size_t)r * 2 + 1];
    }
}

void Engine::dbg_batch_set_wav(const float* wav) {
    const int64_t Wo = out_row_len();  // (throws without a finished batch)
    (void)Wo;
    const Batch& b = bt_;
    const size_t n = (size_t)b.B * native_row_len();
    sync();
    STN_HIP(hipMemcpy(b.wav, wav, n * sizeof(float), hipMemcpyHostToDevice));
    ++ed_seq_;
    ed_valid_ = ed_host_valid_ = false;
}

}  // namespace stn
