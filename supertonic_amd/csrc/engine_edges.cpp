// engine_edges.cpp — trimming leading and trailing silence by level at fetch time: the setting, the fade window (host only), the
// detection's scratch, and the edges cached per finished batch and (rate, parameters) that the output stage (engine_batch.cpp),
// batch_silence_edges and the join plan share.  The kernels are kernels_edges.hip and join_trim_rows_kernel (kernels_output.hip);
// DESIGN.md section 14 has the contract.
// The pause limit lives here too: its setting, its launch behind the detection, and the cuts cached beside the edges.
#include "engine_internal.hpp"

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

void Engine::set_silence_trim(bool on, float top_db, float keep_ms, float fade_ms) {
    refuse(silence_check(top_db, keep_ms, fade_ms));
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

// uploaded once per (rate, fade_ms); at least one float, so that the kernel's pointer is never null
const float* Engine::st_window(int hz) {
    if (st_win_.get() && st_win_hz_ == hz && st_win_ms_ == st_fade_) return static_cast<const float*>(st_win_.get());
    const std::vector<float> w = silence_fade_window(hz, st_fade_);
    float* d = reinterpret_cast<float*>(st_win_.reserve(*this, std::max<size_t>(w.size(), 1) * sizeof(float)));
    sync();  // a fetch may still be reading the old window
    if (!w.empty()) STN_HIP(hipMemcpy(d, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    st_win_hz_ = hz; st_win_ms_ = st_fade_;
    return d;
}

Engine::EdScratch Engine::ed_layout(char* base, int64_t rows, int64_t W, int hz, int S) {
    const size_t nc = (size_t)rows * (size_t)ed_chunks(W), nf = (size_t)rows * (size_t)edges_frames(W, hz);
    Carve c{base};
    EdScratch sc{};
    sc.pa = c.take<float>(nc);
    sc.pb = c.take<float>(nc);
    sc.lev = c.take<double>(nf);
    sc.edges = c.take<int64_t>((size_t)rows * 2);
    sc.seg = c.take<JoinSegT>((size_t)rows);
    sc.prog = c.take<JoinProg>((size_t)rows);
    if (S > 0) {  // the pause limit's tables (section 17)
        sc.pseg = c.take<JoinSegT>((size_t)rows * S);
        sc.pprog = c.take<JoinProg>((size_t)rows);
        sc.pcut = c.take<int64_t>((size_t)rows * 2 * S);
        sc.S = S;
    }
    sc.bytes = c.off;
    return sc;
}

Engine::EdScratch Engine::ed_scratch(int64_t rows, int64_t W, int hz, int S) {
    bool moved = false;
    char* base = ed_buf_.reserve(*this, ed_layout(nullptr, rows, W, hz, S).bytes, &moved);
    if (moved) ed_valid_ = ed_host_valid_ = false;
    return ed_layout(base, rows, W, hz, S);
}

void Engine::ed_enqueue(const float* x, int64_t rows, int64_t W, const int64_t* n, int hz, float top_db, float keep_ms, float fade_ms, const EdScratch& sc, int64_t Mp) {
    const double samples = (double)rows * W, chunks = (double)rows * ed_chunks(W);
    {
        StageSpan span(*this, "out", "edges_frames", 2.0 * samples, samples * 4 + chunks * 8);
        launch_edges_frames(s_, x, rows, W, n, hz, sc.pa, sc.pb);
        span.next("edges_rows", chunks, chunks * 8 + (double)rows * edges_frames(W, hz) * 16);
        launch_edges_rows(s_, rows, W, n, hz, (double)top_db, silence_samples(hz, keep_ms), silence_samples(hz, fade_ms), sc.pa, sc.pb, sc.lev,
                          sc.edges, sc.seg, sc.prog);
        if (sc.S > 0) {
            const double frames = (double)rows * edges_frames(W, hz);
            span.next("pause_rows", frames, frames * 8 + (double)rows * sc.S * (sizeof(JoinSegT) + 16));
            launch_pause_rows(s_, rows, W, n, hz, (double)top_db, silence_samples(hz, fade_ms), Mp, sc.S, sc.lev, sc.edges, sc.pseg, sc.pprog, sc.pcut);
        }
    }
    STN_HIP(hipGetLastError());
}

Engine::EdScratch Engine::ed_batch(const float* x, int64_t Wo, bool pauses) {
    const Batch& b = bt_;
    const int hz = output_rate();
    refuse(rate_check("silence trim", hz));
    const EdScratch sc = ed_scratch(b.B, Wo, hz, pl_stride(pauses, Wo, hz));
    const EdKey key = ed_key(Wo, pauses);
    if (ed_valid_ && key == ed_key_) return sc;
    ed_enqueue(x, b.B, Wo, batch_spans(hz, Wo).dev.n, hz, st_db_, st_keep_, st_fade_, sc, pauses ? pause_samples(hz, pl_ms_) : 0);
    ed_key_ = key;
    ed_valid_ = true;
    ed_host_valid_ = false;
    return sc;
}

const std::vector<int64_t>& Engine::ed_batch_host(bool pauses) {
    const int64_t Wo = out_row_len();
    const EdKey key = ed_key(Wo, pauses);
    if (ed_valid_ && ed_host_valid_ && key == ed_key_) return ed_host_;
    const EdScratch sc = (ed_valid_ && key == ed_key_) ? ed_scratch(bt_.B, Wo, output_rate(), pl_stride(pauses, Wo, output_rate()))
                                                       : ed_batch(out_source(Wo), Wo, pauses);
    ed_host_.resize((size_t)bt_.B * 2);
    STN_HIP(hipMemcpyAsync(ed_host_.data(), sc.edges, ed_host_.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s_));
    if (sc.S > 0) {  // the rows' cut lists: one read per finished batch and setting
        pz_host_.resize((size_t)bt_.B * 2 * sc.S);
        pz_S_ = sc.S;
        STN_HIP(hipMemcpyAsync(pz_host_.data(), sc.pcut, pz_host_.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s_));
    }
    sync();
    ed_host_valid_ = true;
    return ed_host_;
}

// row r's words {start, end} of an edge table read back -> the caller's arrays
static void edges_copy_out(const int64_t* e, int rows, int64_t* start, int64_t* end) {
    for (int r = 0; r < rows; ++r) {
        if (start) start[r] = e[(size_t)r * 2];
        if (end) end[r] = e[(size_t)r * 2 + 1];
    }
}

void Engine::batch_silence_edges(int64_t* start, int64_t* end) { edges_copy_out(ed_batch_host(pause_limit_active()).data(), bt_.B, start, end); }

void Engine::op_silence_edges(int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, int64_t* start, int64_t* end) {
    op_silence_trim(hz, rows, W, x, n, top_db, keep_ms, 0.0f, nullptr, ENC_F32, nullptr, start, end);
}

void Engine::op_silence_trim(int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, float fade_ms, const float* gain,
                             int enc, void* y, int64_t* start, int64_t* end) {
    ed_op("op_silence_trim", "op_silence", false, hz, rows, W, x, n, top_db, keep_ms, fade_ms, 0.0f, gain, enc, y, nullptr, start, end, nullptr, nullptr, nullptr, 0);
}

// ---- pause limit

void Engine::set_pause_limit(bool on, float max_pause_ms) {
    refuse(pause_check(max_pause_ms));
    pl_on_ = on;
    pl_ms_ = max_pause_ms;
}

void Engine::get_pause_limit(int* on, float* max_pause_ms) const {
    if (on) *on = pl_on_ ? 1 : 0;
    if (max_pause_ms) *max_pause_ms = pl_ms_;
}

// row r's words {cuts, len, lo, hi, ...} of a cut list read back -> the caller's arrays
static void pause_copy_out(const int64_t* w, int S, int rows, int64_t* len, int32_t* n_cuts, int64_t* cuts, int cap_pairs) {
    for (int r = 0; r < rows; ++r) {
        const int64_t* wr = w + (size_t)r * 2 * S;
        if (n_cuts) n_cuts[r] = (int32_t)wr[0];
        if (len) len[r] = wr[1];
        if (cuts)
            for (int c = 0; c < (int)wr[0] && c < cap_pairs; ++c) {
                cuts[((size_t)r * cap_pairs + c) * 2] = wr[2 + 2 * c];
                cuts[((size_t)r * cap_pairs + c) * 2 + 1] = wr[3 + 2 * c];
            }
    }
}

void Engine::batch_pauses(int64_t* len, int32_t* n_cuts, int64_t* cuts, int cap_pairs) {
    if (cap_pairs < 0 || (cuts && cap_pairs == 0)) throw std::invalid_argument("batch_pauses: cuts needs cap_pairs >= 1");
    ed_batch_host(true);
    pause_copy_out(pz_host_.data(), pz_S_, bt_.B, len, n_cuts, cuts, cap_pairs);
}

void Engine::op_pause_trim(int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, float fade_ms, float max_pause_ms,
                           const float* gain, int enc, void* y, int64_t* start, int64_t* end, int64_t* len, int32_t* n_cuts, int64_t* cuts, int cap_pairs) {
    ed_op("op_pause_trim", "op_pause", true, hz, rows, W, x, n, top_db, keep_ms, fade_ms, max_pause_ms, gain, enc, y, nullptr, start, end, len, n_cuts, cuts, cap_pairs);
}

void Engine::op_silence_edges_ex(int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, float fade_ms, float max_pause_ms,
                                 EdProbe& probe, int64_t* start, int64_t* end, int64_t* len, int32_t* n_cuts, int64_t* cuts, int cap_pairs) {
    ed_op("op_silence_edges_ex", "op_silence", max_pause_ms != 0.0f, hz, rows, W, x, n, top_db, keep_ms, fade_ms, max_pause_ms, nullptr, ENC_F32, nullptr, &probe,
          start, end, len, n_cuts, cuts, cap_pairs);
}

// The one body of the three entries above: the detection (with the pause pass when `pauses`), then, with y, the rows cut, faded and
// stored as enc.  entry and who name the caller in the refusals.  With a probe the rows sit as it asks, the whole scratch (the shares,
// the levels, the edges and the tables) holds the poison before the first launch, and the shares and levels are read out.
void Engine::ed_op(const char* entry, const char* who, bool pauses, int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms,
                   float fade_ms, float max_pause_ms, const float* gain, int enc, void* y, EdProbe* probe, int64_t* start, int64_t* end, int64_t* len,
                   int32_t* n_cuts, int64_t* cuts, int cap_pairs) {
    OpScope op(*this);
    refuse(silence_check(top_db, keep_ms, fade_ms));
    if (pauses) refuse(pause_check(max_pause_ms));
    refuse(rate_check(pauses ? "pause limit" : "silence trim", hz));
    if (cap_pairs < 0 || (cuts && cap_pairs == 0)) throw std::invalid_argument(std::string(entry) + ": cuts needs cap_pairs >= 1");
    const int eb = enc_bytes(enc);
    if (eb == 0) throw std::invalid_argument("unknown sample encoding " + std::to_string(enc));
    const std::vector<int64_t> nn = spans(who, rows, W, n);
    const int64_t Mp = pauses ? pause_samples(hz, max_pause_ms) : 0;
    const int S = pauses ? pause_stride(W, hz, Mp) : 0;
    const EdScratch sc = op.carve_poisoned(probe, ed_layout, rows, W, hz, S);
    const float* dx = op.up(x, (size_t)rows * W, probe && probe->x_misalign ? 1 : 0);
    ed_enqueue(dx, rows, W, op.spans(rows, W, nn).n, hz, top_db, keep_ms, fade_ms, sc, Mp);
    std::vector<int64_t> e((size_t)rows * 2), pz((size_t)rows * 2 * S);
    op.down(e.data(), sc.edges, e.size());
    if (S > 0) op.down(pz.data(), sc.pcut, pz.size());
    const std::vector<float> w = silence_fade_window(hz, fade_ms);
    if (y) {
        const float* dw = w.empty() ? op.buf<float>(1) : op.up(w);  // (never null: the kernel's pointer)
        const float* dg = op.up(gain, (size_t)rows);
        const int64_t Ws = ((int64_t)W + 15) / 16 * 16;  // rows 16-byte aligned in every encoding: the store runs full width
        void* dy = op.buf<char>((size_t)rows * Ws * eb);
        launch_join_trim_rows(s_, dx, W, pauses ? sc.pseg : sc.seg, pauses ? sc.pprog : sc.prog, rows, W, dg, dw, enc, dy, Ws);
        STN_HIP(hipGetLastError());
        op.down_rows(y, dy, (size_t)W * eb, (size_t)Ws * eb, (size_t)rows);
    }
    if (probe) {
        const size_t nc = (size_t)rows * (size_t)ed_chunks(W), nf = (size_t)rows * (size_t)edges_frames(W, hz);
        op.down(probe->pa, sc.pa, nc);
        op.down(probe->pb, sc.pb, nc);
        op.down(probe->lev, sc.lev, nf);
        probe->form = chunk_staging_form(dx, nullptr, W);
    }
    sync();  // (w, e and pz are read or written by the copies above until here)
    edges_copy_out(e.data(), rows, start, end);
    if (S > 0) return pause_copy_out(pz.data(), S, rows, len, n_cuts, cuts, cap_pairs);
    for (int r = 0; r < rows; ++r) {
        if (len) len[r] = e[(size_t)r * 2 + 1] - e[(size_t)r * 2];
        if (n_cuts) n_cuts[r] = 0;
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
