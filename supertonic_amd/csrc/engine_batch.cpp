// engine_batch.cpp — the resident-batch pipeline (stn_batch_*): upload, the one duration read, the captured latent pipeline and its
// graph cache, the output stage and the fetches that run it (see engine.hpp).
#include "engine.hpp"
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace stn {
using detail::up;

// =================================================================================================
// resident batch
// =================================================================================================

// Grow-only device buffer of the resident batch.  A reallocation retires the old block (freed at the next upload, once the
// stream has drained) and bumps the generation that is part of the graph key: a captured graph holds raw pointers.
template <typename T>
void Engine::ensure(T*& p, size_t& cap, size_t need) {
    if (p && need <= cap) return;
    const size_t n = std::max<size_t>(need + need / 4, 64);  // headroom: ragged request streams settle after a few uploads
    T* q = nullptr;
    STN_HIP(hipMalloc(reinterpret_cast<void**>(&q), n * sizeof(T)));
    if (p) {
        batch_owned_.erase(std::find(batch_owned_.begin(), batch_owned_.end(), static_cast<void*>(p)));
        batch_retired_.push_back(p);
    }
    batch_owned_.push_back(q);
    p = q;
    cap = n;
    ++bt_.gen;
}

void Engine::batch_upload(int B, int Lt, const int64_t* ids, const float* text_mask, const float* style_ttl,
                          const float* style_dp, const float* duration_override, const int64_t* utt_ids) {
    STN_HIP(hipSetDevice(device_));
    if (!loaded_) throw std::runtime_error("no model loaded");
    if (B <= 0 || Lt <= 0) throw std::runtime_error("empty batch");
    sync();
    for (void* p : batch_retired_) (void)hipFree(p);
    batch_retired_.clear();
    Batch& b = bt_;
    const int Lt_in = Lt;  // the caller's row stride of ids / text_mask
    if (shape_buckets_) Lt = (int)bucket_up(Lt, 32);  // token rows padded with id 0 / mask 0: the lengths come from the mask, not from Lt
    b.B = B; b.Lt = Lt; b.L = 0; b.noise_L = 0; b.total_step = 0;
    b.have_override = false; b.have_noise = false;
    b.h_dur.clear(); b.h_llen.clear();
    const size_t n_ttl = (size_t)B * a_.n_style_ttl * a_.d_style_ttl, n_dp = (size_t)B * a_.n_style_dp * a_.d_style_dp;
    ensure(b.ids, b.ids_cap, (size_t)B * Lt);
    ensure(b.tlen, b.tlen_cap, (size_t)B);
    ensure(b.style_ttl, b.ttl_cap, n_ttl);
    ensure(b.style_dp, b.dp_cap, n_dp);
    ensure(b.dur, b.dur_cap, (size_t)B);
    ensure(b.utt_ids, b.utt_cap, (size_t)B);
    if (Lt != Lt_in) {
        STN_HIP(hipMemsetAsync(b.ids, 0, sizeof(int64_t) * B * Lt, s_));
        STN_HIP(hipMemcpy2DAsync(b.ids, sizeof(int64_t) * Lt, ids, sizeof(int64_t) * Lt_in, sizeof(int64_t) * Lt_in, (size_t)B, hipMemcpyHostToDevice, s_));
    } else {
        STN_HIP(hipMemcpyAsync(b.ids, ids, sizeof(int64_t) * B * Lt, hipMemcpyHostToDevice, s_));
    }
    STN_HIP(hipMemcpyAsync(b.style_ttl, style_ttl, sizeof(float) * n_ttl, hipMemcpyHostToDevice, s_));
    STN_HIP(hipMemcpyAsync(b.style_dp, style_dp, sizeof(float) * n_dp, hipMemcpyHostToDevice, s_));
    std::vector<int64_t> uid(B);
    for (int i = 0; i < B; ++i) uid[i] = utt_ids ? utt_ids[i] : i;
    STN_HIP(hipMemcpyAsync(b.utt_ids, uid.data(), sizeof(int64_t) * B, hipMemcpyHostToDevice, s_));
    ar_.reset();
    float* d_mask = up(ar_, s_, text_mask, (size_t)B * Lt_in);
    launch_mask_to_len(s_, d_mask, B, Lt_in, b.tlen);
    // packed text rows: first row of each utterance (fixed for the life of this upload) and their total
    ensure(b.toff, b.toff_cap, (size_t)B + 1);
    b.trows = 0;
    for (int i = 0; i < B; ++i) {
        int n = 0;
        for (int t = 0; t < Lt_in; ++t) n += text_mask[(size_t)i * Lt_in + t] > 0.5f ? 1 : 0;  // as mask_to_len_kernel counts
        b.trows += n;
    }
    if (shape_buckets_) b.trows = (int)bucket_up(b.trows, 64);  // dead text rows behind the last utterance (toff[B] keeps the exact sum)
    if (B <= 1024) launch_row_map(s_, b.tlen, B, b.toff, nullptr);
    b.have_override = duration_override != nullptr;
    if (duration_override) b.h_dur.assign(duration_override, duration_override + B);
    sync();
}

void Engine::batch_set_noise(const float* noise, int L) {
    STN_HIP(hipSetDevice(device_));
    Batch& b = bt_;
    if (b.B == 0) throw std::runtime_error("batch_set_noise: no batch uploaded");
    if (L < 1) throw std::runtime_error("batch_set_noise: L must be >= 1");
    const int D = a_.latent_dim * a_.chunk_compress_factor;
    sync();
    ensure(b.noise, b.noise_cap, (size_t)b.B * D * L);
    STN_HIP(hipMemcpyAsync(b.noise, noise, sizeof(float) * b.B * D * L, hipMemcpyHostToDevice, s_));
    b.have_noise = true;
    b.noise_L = L;  // checked against the durations in batch_run
    sync();
}

// Latent geometry exactly as TextToSpeech::sampleNoisyLatent (/root/reference/cpp/helper.cpp:424-440,457,764-768):
// float32 products, truncation to integers.
static void latent_geometry(const stn_arch& a, const std::vector<float>& dur, int& L, std::vector<int>& llen) {
    const int cs = a.base_chunk_size * a.chunk_compress_factor;
    float mx = dur[0];
    for (float d : dur) mx = std::max(mx, d);
    const float wav_len_max = mx * (float)a.sample_rate;
    L = (int)((wav_len_max + (float)cs - 1.0f) / (float)cs);
    llen.resize(dur.size());
    for (size_t i = 0; i < dur.size(); ++i) {
        const int64_t wl = (int64_t)(dur[i] * (float)a.sample_rate);
        llen[i] = (int)((wl + cs - 1) / cs);
    }
}

void Engine::batch_run(int total_step, float speed, uint64_t noise_seed) {
    STN_HIP(hipSetDevice(device_));
    Batch& b = bt_;
    if (b.B == 0) throw std::runtime_error("batch_run: no batch uploaded");
    if (total_step < 1) throw std::runtime_error("total_step must be >= 1");
    if (!(speed > 0.f)) throw std::runtime_error("speed must be > 0");
    const stn_arch& a = a_;
    const int B = b.B, Lt = b.Lt, D = a.latent_dim * a.chunk_compress_factor;
    b.total_step = total_step; b.speed = speed; b.noise_seed = noise_seed;
    ar_.reset();
    // 1. duration predictor (always executed; its output may be overridden for shape control)
    Ragged trg;
    const bool tpk = packed_text_ok(B) && b.trows > 0;
    if (tpk) { trg.off = b.toff; trg.rows = b.trows; }
    std::vector<float> dur(B);
    // the text rows: persistent, grow-only buffers (a reallocation bumps b.gen, which every graph key holds)
    const size_t text_bytes = (size_t)(tpk ? (int64_t)b.trows : (int64_t)B * Lt) * a.te_out_dim * (is_half(dt_) ? 2 : 4);
    ensure(b.text_side, b.text_side_cap, text_bytes);
    ensure(b.text_rows, b.text_cap, text_bytes);
    {
        // on the side streams, each with its own workspace (see dp_s_): swapped in for the duration of a text stage
        struct Side {
            Engine& e; hipStream_t& s; Arena& ar; bool on;
            Side(Engine& e_, hipStream_t& s_, Arena& ar_) : e(e_), s(s_), ar(ar_), on(s_ != nullptr) { if (on) { std::swap(e.s_, s); e.ar_.swap(ar); e.ar_.reset(); } }
            ~Side() { if (on) { std::swap(e.s_, s); e.ar_.swap(ar); } }
        };
        {   // 2. text encoder -> context rows (act dtype), once the previous run has taken its copy of them
            Side side(*this, te_s_, te_ar_);
            if (side.on && copied_valid_) STN_HIP(hipStreamWaitEvent(s_, ev_copied_, 0));
            text_enc_dev(B, Lt, b.ids, b.style_ttl, b.tlen, nullptr, b.text_side, tpk ? &trg : nullptr);
            STN_HIP(hipEventRecord(ev_te_, s_));
        }
        {   // 1. duration predictor (always executed; its output may be overridden for shape control), beside the encoder
            Side side(*this, dp_s_, dp_ar_);
            duration_dev(B, Lt, b.ids, b.style_dp, b.tlen, b.dur, tpk ? &trg : nullptr);
            if (!b.have_override || dur_read_always_) {
                STN_HIP(hipMemcpyAsync(dur.data(), b.dur, sizeof(float) * B, hipMemcpyDeviceToHost, s_));
                STN_HIP(hipEventRecord(ev_dp_, s_));
            }
        }
        if (!b.have_override || dur_read_always_) STN_HIP(hipEventSynchronize(ev_dp_));  // the one host round trip (the predictor only): L = f(max duration) sizes every later buffer
        if (b.have_override) dur = b.h_dur;  // known on the host: no device->host read, no sync (unless the measurement switch asks for the read: the
                                             // critical path of a predicted-duration run on the controlled shapes of a forced one)
    }
    // Hand-over of this run's text rows to the main pipeline (everything captured below reads b.text_rows).  It happens where the
    // rows are first needed — in front of the text K/V GEMM of the first text cross-attention — so the noise, the style K/V, the time
    // conditioning and the first ConvNeXt blocks of the estimator run beside the encoder; a captured pipeline is therefore TWO
    // graphs with this hand-over between them.
    auto take_text_rows = [this, &b, text_bytes]() {
        if (te_s_) STN_HIP(hipStreamWaitEvent(s_, ev_te_, 0));
        STN_HIP(hipMemcpyAsync(b.text_rows, b.text_side, text_bytes, hipMemcpyDeviceToDevice, s_));
        STN_HIP(hipEventRecord(ev_copied_, s_));
        copied_valid_ = true;
    };
    for (float& d : dur) d /= speed;  // cpp/helper.cpp:529-531
    int L = 0;
    latent_geometry(a, dur, L, b.h_llen);
    if (L < 1) throw std::runtime_error("predicted duration too short: zero latent frames");
    if (shape_buckets_ && !b.have_noise) L = (int)bucket_up(L, 16);  // (injected noise has the caller's exact [B, D, L] layout)
    if (b.have_noise && b.noise_L != L)
        throw std::runtime_error("injected noise has L=" + std::to_string(b.noise_L) + " but the durations imply L=" + std::to_string(L));
    b.L = L;
    reported_dur_ = dur;  // durations after /speed: what the reference returns (cpp/helper.cpp:680)
    ++ed_seq_;            // (what was measured on the previous waveform at fetch time no longer holds)
    const size_t nx = (size_t)B * D * L, nw = (size_t)B * L * a.base_chunk_size * a.chunk_compress_factor;
    ensure(b.xt[0], b.xt_cap[0], nx);
    ensure(b.xt[1], b.xt_cap[1], nx);
    ensure(b.wav, b.wav_cap, nw);
    // Everything the pipeline derives from the lengths alone — the estimator's row map, the cross-attention's pairing, the vocoder's extents
    // and offsets — is built here, on the host that already holds the lengths, and rides up with them and the seed in ONE copy node at the
    // head of the chain (host/len_tables.hpp): four single-workgroup kernels leave every replay.
    int ve_rows = 0;
    if (packed_rows_ok(B)) for (int v : b.h_llen) ve_rows += v;
    if (shape_buckets_) ve_rows = (int)bucket_up(ve_rows, 64);  // dead rows behind the last utterance
    int vform = VO_DENSE;
    const int tr_rows = vocoder_rows(B, L, &vform);  // (two forms with equal row counts must not share a capture)
    const int tab_vo = vo_ragged_ ? LEN_VO_SCALED : !tr_rows ? LEN_VO_NONE : vform == VO_TRIM_TAIL ? LEN_VO_TAIL : LEN_VO_2RF;
    const bool tab_pairs = ve_rows > 0 && fused_xattn_ && is_half(dt_) && B >= 2;
    b.tl = len_tables_layout(B, ve_rows, tab_pairs, tab_vo);
    h_tab_.assign((size_t)b.tl.total, 0);
    len_tables_build(b.tl, b.h_llen.data(), B, ve_rows, tab_pairs, tab_vo, a.chunk_compress_factor, L * a.chunk_compress_factor, vo_rf_, h_tab_.data());
    const unsigned long long seed64 = (unsigned long long)noise_seed;
    std::memcpy(h_tab_.data() + b.tl.seed, &seed64, sizeof seed64);
    ensure(b.tab, b.tab_cap, (size_t)b.tl.total);  // (a reallocation bumps b.gen: no graph keeps the old block)
    b.llen = b.tab + b.tl.llen;
    seed_dev_ = reinterpret_cast<unsigned long long*>(b.tab + b.tl.seed);
    // per-call data of the captured region lives in pinned host memory (the graph's memcpy node re-reads it at replay).
    // Sized for 1024 utterances of 64 latent frames up front so that it is not reallocated under cached graphs; should it ever have to grow,
    // its address is part of the graph key and the graphs that point at the old block are dropped before it is freed.
    if ((size_t)b.tl.total > pin_tab_cap_) {
        if (pin_tab_) { sync(); drop_graphs(); (void)hipHostFree(pin_tab_); pin_tab_ = nullptr; }
        const size_t cap = std::max<size_t>((size_t)b.tl.total + (size_t)b.tl.total / 4, (size_t)1024 * (64 + 8));
        STN_HIP(hipHostMalloc(reinterpret_cast<void**>(&pin_tab_), sizeof(int) * cap, hipHostMallocDefault));
        pin_tab_cap_ = cap;
        pin_valid_ = false;
    }
    // a previous run's copy node may still be reading the staging: rewrite it only when the content changes, and then
    // only after the stream has drained (steady-state replays of an unchanged batch never wait here)
    if (!pin_valid_ || pin_tab_n_ != h_tab_.size() || !std::equal(h_tab_.begin(), h_tab_.end(), pin_tab_)) {
        sync();
        std::copy(h_tab_.begin(), h_tab_.end(), pin_tab_);
        pin_tab_n_ = h_tab_.size();
        pin_valid_ = true;
    }

    ensure_time_cond(total_step, B);  // eager, on s_, ahead of whatever is replayed or captured below (same stream: ordered)
    GraphKey key;
    key.B = B; key.Lt = Lt; key.L = L; key.steps = total_step; key.noise = b.have_noise; key.ragged = vo_ragged_; key.xattn = fused_xattn_;
    key.ffn = fused_ffn_; key.gen = b.gen; key.wgen = wgen_; key.pin = pin_tab_;
    key.rows = ve_rows;
    last_ve_rows_ = key.rows ? key.rows : (int64_t)B * L;
    key.vrows = tr_rows; key.vform = vform;
    if (shape_buckets_) key.vrows = (int)bucket_up(key.vrows, 64 * a.chunk_compress_factor);
    key.trows = tpk ? b.trows : 0;
    last_vo_rows_ = (int64_t)B * L * a.chunk_compress_factor;
    if (vo_ragged_ && packed_ve_ && is_half(dt_)) {
        last_vo_rows_ = 0;
        for (int v : b.h_llen) last_vo_rows_ += (int64_t)v * a.chunk_compress_factor;
        if (shape_buckets_) last_vo_rows_ = bucket_up(last_vo_rows_, 64 * a.chunk_compress_factor);
        key.vrows = (int)last_vo_rows_;  // (the length-aware vocoder's packed rows are baked into the pipeline like the others)
    }
    else if (key.vrows) last_vo_rows_ = key.vrows;
    key.p0 = b.xt[0]; key.p1 = b.wav; key.s = s_;
    // event timing forces eager launches: hipEventRecord captured into a graph returns garbage spans on ROCm 7.2 (measured)
    const bool graphable = graph_on_ && !prof_on_;
    if (graphable) {
        for (auto& g : graphs_)
            if (g.key == key) {
                g.last_use = ++graph_clock_;
                STN_HIP(hipGraphLaunch(g.exec, s_));
                take_text_rows();
                STN_HIP(hipGraphLaunch(g.exec2, s_));
                ++graph_replays_;
                return;
            }
    }
    const auto warm = std::find(warm_keys_.begin(), warm_keys_.end(), key);
    if (graphable && warm != warm_keys_.end()) {  // second sighting of this shape: the arena is warm, allocation order is fixed
        const Arena::Mark cap0 = ar_.mark();
        const size_t cap_before = ar_.capacity();
        STN_HIP(hipStreamBeginCapture(s_, hipStreamCaptureModeThreadLocal));
        bool ok = true;
        std::string why;
        hipGraph_t g = nullptr, g2 = nullptr;
        hipError_t ec1 = hipErrorUnknown;
        bool split = false;
        // at the hand-over the first graph ends and the second begins (the hand-over itself is issued between their launches)
        auto split_capture = [&]() {
            ec1 = hipStreamEndCapture(s_, &g);
            split = true;
            STN_HIP(hipStreamBeginCapture(s_, hipStreamCaptureModeThreadLocal));
        };
        try { enqueue_after_duration(total_step, split_capture); } catch (const std::exception& e) { ok = false; why = e.what(); }
        const hipError_t ec = hipStreamEndCapture(s_, &g2);
        text_gate_ = nullptr;
        ar_.release(cap0);
        hipGraphExec_t ex = nullptr, ex2 = nullptr;
        if (ok && split && ec1 == hipSuccess && ec == hipSuccess && g && g2 && ar_.capacity() == cap_before &&
            hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) == hipSuccess && hipGraphInstantiate(&ex2, g2, nullptr, nullptr, 0) == hipSuccess) {
            if (graphs_.size() >= kGraphCache) {  // evict the least recently used entry
                auto lru = std::min_element(graphs_.begin(), graphs_.end(), [](const GraphEntry& x, const GraphEntry& y) { return x.last_use < y.last_use; });
                sync();  // its last replay may still be running
                (void)hipGraphExecDestroy(lru->exec);
                (void)hipGraphDestroy(lru->graph);
                if (lru->exec2) (void)hipGraphExecDestroy(lru->exec2);
                if (lru->graph2) (void)hipGraphDestroy(lru->graph2);
                graphs_.erase(lru);
            }
            GraphEntry e;
            e.key = key; e.graph = g; e.exec = ex; e.graph2 = g2; e.exec2 = ex2; e.last_use = ++graph_clock_;
            graphs_.push_back(e);
            warm_keys_.erase(warm);
            STN_HIP(hipGraphLaunch(ex, s_));
            take_text_rows();
            STN_HIP(hipGraphLaunch(ex2, s_));
            ++graph_replays_;
            return;
        }
        if (ex) (void)hipGraphExecDestroy(ex);
        if (ex2) (void)hipGraphExecDestroy(ex2);
        if (g2) (void)hipGraphDestroy(g2);
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        if (!ok) throw std::runtime_error("graph capture failed: " + why);
        // fall through to an eager run
    }
    if (warm == warm_keys_.end()) {
        if (warm_keys_.size() >= kWarmKeys) warm_keys_.erase(warm_keys_.begin());
        warm_keys_.push_back(key);
    }
    enqueue_after_duration(total_step, take_text_rows);
}

// Everything after the duration read: lengths to the device, text encoder, initial latent, Euler loop, vocoder.
void Engine::ensure_time_cond(int total_step, int B) {
    TimeCond& t = tcond_;
    if (t.steps == total_step && t.B == B && t.wgen == wgen_ && t.buf) return;
    const stn_arch& a = a_;
    const size_t n_cnt = (size_t)2 * total_step * B + (size_t)B, n_tb = (size_t)total_step * B * a.ve_main_blocks * a.ve_dim;
    const size_t need = (n_cnt + 3) / 4 * 4 + n_tb;  // (tb 16-byte aligned behind the counters)
    if (need > t.cap) {
        sync();
        drop_graphs();  // captured pipelines read the old buffer
        if (t.buf) (void)hipFree(t.buf);
        t.buf = nullptr; t.cap = 0;
        STN_HIP(hipMalloc(reinterpret_cast<void**>(&t.buf), need * sizeof(float)));
        t.cap = need;
    }
    t.tot = t.buf; t.cur = t.tot + (size_t)total_step * B; t.dt = t.cur + (size_t)total_step * B; t.tb = t.buf + (n_cnt + 3) / 4 * 4;
    t.steps = 0;  // (invalid until the launches below are enqueued)
    const Arena::Mark mk = ar_.mark();
    launch_step_counters(s_, t.tot, t.cur, t.dt, B, total_step);
    (void)ve_time_cond_dev(total_step * B, t.tot, t.cur, t.tb);
    ar_.release(mk);
    t.steps = total_step; t.B = B; t.wgen = wgen_;
}

void Engine::enqueue_after_duration(int total_step, const std::function<void()>& take_text_rows) {
    Batch& b = bt_;
    const stn_arch& a = a_;
    const int B = b.B, Lt = b.Lt, L = b.L, D = a.latent_dim * a.chunk_compress_factor;
    const size_t nx = (size_t)B * D * L;
    // the lengths, the seed and every table derived from the lengths (batch_run built them): one copy; its size follows from the graph key
    STN_HIP(hipMemcpyAsync(b.tab, pin_tab_, sizeof(int) * (size_t)b.tl.total, hipMemcpyHostToDevice, s_));
    // 2. (the text encoder ran on the side stream: batch_run) its rows
    Ragged trg;
    const bool tpk = packed_text_ok(B) && b.trows > 0;
    if (tpk) { trg.off = b.toff; trg.rows = b.trows; }
    const Ragged* trgp = tpk ? &trg : nullptr;
    void* text_rows = b.text_rows;
    // 3. initial latent
    if (b.have_noise) {
        STN_HIP(hipMemcpyAsync(b.xt[0], b.noise, nx * 4, hipMemcpyDeviceToDevice, s_));
        launch_mask_ncl(s_, b.xt[0], B, D, L, b.llen);
    } else {
        stage_ = "ve";
        if (prof_on_) prof_begin("noise", 0.0, (double)nx * 4.0);
        launch_randn_masked(s_, 0, b.utt_ids, B, D, L, b.llen, b.xt[0], seed_dev_);
        if (prof_on_) prof_end();
    }
    // 4. Euler loop: step-invariant K/V once, the time conditioning of every step in one pass, then total_step passes
    VeCtx c = ve_prepare_dev(B, Lt, text_rows, b.style_ttl, b.tlen, trgp, /*defer_text=*/true);
    // armed here, fired by the first text cross-attention of the first Euler step (ve_step_dev): hand-over of the rows, then the text K/V
    text_gate_ = [this, &c, &b, &take_text_rows, B, Lt, text_rows, trgp]() {
        take_text_rows();
        ve_text_kv_dev(c, B, Lt, text_rows, b.tlen, trgp);
    };
    struct Disarm { std::function<void()>& g; ~Disarm() { g = nullptr; } } disarm{text_gate_};  // it refers to this frame: never outlives it
    if (a.ve_main_blocks == 0) { auto fire = std::move(text_gate_); text_gate_ = nullptr; fire(); }  // (no cross-attention would ever fire it)
    // (step counters and time conditioning: computed once per (total_step, B, weights) by ensure_time_cond, ahead of the captured pipeline)
    if (tcond_.steps != total_step || tcond_.B != B || tcond_.wgen != wgen_) throw std::runtime_error("time conditioning not prepared for this run");
    const float* tot_all = tcond_.tot;
    const float* cur_all = tcond_.cur;
    const float* dt_all = tcond_.dt;
    const float* tb_all = tcond_.tb;
    const size_t tb_stride = (size_t)B * a.ve_main_blocks * a.ve_dim;
    Ragged rg;
    const Ragged* rgp = nullptr;
    if (packed_rows_ok(B)) {  // the estimator works on the frames the utterances own and nothing else
        rg.rows = 0;
        for (int v : b.h_llen) rg.rows += v;
        if (shape_buckets_) rg.rows = (int)bucket_up(rg.rows, 64);  // dead rows behind the last utterance (as in the graph key)
        if (b.tl.ve_off < 0 || b.tl.ve_row_b + rg.rows > b.tl.total) throw std::logic_error("batch_run: no row map in the length tables");
        const int* off = b.tab + b.tl.ve_off;
        const int* row_b = b.tab + b.tl.ve_row_b;
        rg.off = off; rg.row_b = row_b;
        // one 1024-thread workgroup of fold_dwconv_ln fits a CU: 271 runs of <= 32 frames (this bench's lengths) are two rounds, 256 runs of <= 40 one
        rg.fold_run = fold_run_frames(b.h_llen.data(), B, n_cu_);
        if (fused_xattn_ && is_half(dt_) && B >= 2) {  // the head-split cross-attention's pairing, once per synthesis (the lengths are the run's)
            if (b.tl.pairs < 0) throw std::logic_error("batch_run: no pairing in the length tables");
            const int* pairs = b.tab + b.tl.pairs;
            rg.hs_pairs = pairs;
        }
        rgp = &rg;
    }
    int cur = 0;
    // the latent as rows (the input projection's operand) lives across the steps: every step's Euler update writes it beside the [B][D][L] layout, so only
    // the first step converts (ncl_to_rows: 11 us of strided reads per step otherwise)
    const int Dz = (a.latent_dim * a.chunk_compress_factor + 63) / 64 * 64;
    const int64_t Mz = rgp ? (int64_t)rg.rows : (int64_t)B * L;
    void* z_rows = act_alloc(Mz * Dz);
    for (int st = 0; st < total_step; ++st) {
        ve_step_dev(B, L, c, b.xt[cur], b.tlen, b.llen, tot_all + (size_t)st * B, cur_all + (size_t)st * B, b.xt[cur ^ 1],
                    tb_all + (size_t)st * tb_stride, rgp, dt_all, z_rows, st > 0, st + 1 < total_step);
        cur ^= 1;
    }
    final_xt_ = cur;
    // 5. vocoder
    const int* vlen = nullptr;
    if (vo_ragged_) vlen = b.tab + b.tl.vo_n;  // len * ccf
    int vrows = 0;
    const int* valid = nullptr;
    bool tails = false;
    if (vo_ragged_ && packed_ve_) {
        for (int v : b.h_llen) vrows += v * a.chunk_compress_factor;
        if (shape_buckets_) vrows = (int)bucket_up(vrows, 64 * a.chunk_compress_factor);
    } else if (int vform = VO_DENSE; int tr = vocoder_rows(B, L, &vform)) {
        if (shape_buckets_) tr = (int)bucket_up(tr, 64 * a.chunk_compress_factor);
        // reference (dense) semantics at the cost of the frames that are not position-independent
        vlen = b.tab + b.tl.vo_n; valid = b.tab + b.tl.vo_valid; vrows = tr; tails = vform == VO_TRIM_TAIL;
    }
    if (vlen && b.tl.vo_n < 0) throw std::logic_error("batch_run: no vocoder extents in the length tables");
    vocoder_dev(B, L, b.xt[cur], b.wav, vlen, vrows, valid, tails, vlen ? b.tab + b.tl.vo_off : nullptr);
    STN_HIP(hipGetLastError());  // a kernel launch that was rejected (bad configuration) must not pass silently
}

// =================================================================================================
// output stage: the finished batch -> what a fetch delivers
// =================================================================================================

// the fetch scratch: the one place where it grows (engine.hpp has the rule for the pointers handed out)
char* DevBuf::reserve(Engine& e, size_t bytes, bool* moved) {
    const bool grow = !p_ || bytes > cap_;
    if (moved) *moved = grow;
    if (!grow) return p_;
    e.sync();  // the previous fetch may still be reading it
    if (p_) (void)hipFree(p_);
    p_ = nullptr; cap_ = 0;
    STN_HIP(hipMalloc(reinterpret_cast<void**>(&p_), bytes + bytes / 4));
    cap_ = bytes + bytes / 4;
    return p_;
}

// a constant table's device copy: the one place where one is replaced (engine.hpp has the rule; the caller has set the device)
void* DeviceTable::put(Engine& e, const void* host, size_t bytes) {
    void* p = nullptr;
    STN_HIP(hipMalloc(&p, bytes));
    STN_HIP(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, e.stream()));
    e.sync();
    if (p_) (void)hipFree(p_);
    return p_ = p;
}

int64_t Engine::out_row_len() {
    STN_HIP(hipSetDevice(device_));
    const Batch& b = bt_;
    if (!b.wav || b.L == 0) throw std::runtime_error("no finished batch");
    return out_len(native_row_len());
}

bool Engine::out_native() const { return !pitch_on() && !loudness_on() && !out_in_scratch(); }

const float* Engine::out_source(int64_t Wo) {
    const Batch& b = bt_;
    // section 24: with pitch on every stage starts from the shifted rows (pitch scratch, row stride W) instead of b.wav
    const float* wav = wav_rows();
    if (!out_in_scratch()) return wav;
    float* d = out_f32_buf((size_t)b.B * Wo);
    // the chain in the order of Stage, behind the pitch: the first stage that is on reads the rows it starts from (left as they are) and
    // writes the scratch, every later one runs in place there (sections 18, 25, 21 and 20)
    const float* cur = wav;
    if (resample_on()) { resample_enqueue(rs_table(), cur, b.B, native_row_len(), ENC_F32, d, Wo); cur = d; }
    if (filter_on()) { fl_batch(cur, Wo, d); cur = d; }
    if (expander_on()) { xp_batch(cur, Wo, d); cur = d; }
    if (deesser_on()) { ds_batch(cur, Wo, d); cur = d; }
    if (compressor_on()) { cp_batch(cur, Wo, d); cur = d; }
    return d;
}

RowsId Engine::rows_id(Stage stage, int64_t Wo) const {
    // the generation of every stage, in the order of Stage (the rate's is hz itself): the one list of what rows depend on
    const uint64_t gen[] = {ps_gen_, 0, fl_gen_, xp_.gen, ds_.gen, cp_.gen};
    static_assert(sizeof(gen) / sizeof(gen[0]) == N_STAGES, "one generation per stage of the chain");
    RowsId id{ed_seq_, output_rate(), Wo, {}};
    std::copy(gen, gen + stage + 1, id.gen);
    return id;
}

// section 15: with the limiter active the store, the cut and the join run on the limited rows
Engine::GainedRows Engine::gain_step(const float* src, int64_t rows, int64_t W, int64_t stride, const LoRes& m) {
    if (!limiter_active()) return {src, m.gain, stride};
    const LmScratch lm = lm_rows(src, rows, W, m.n, m.gain);
    return {lm.y, lm.trim, W};
}

static int64_t join_stride(const JoinPlan& p);
static size_t join_f32_offset(size_t n_rows);
static int need_enc(int enc) {
    const int eb = enc_bytes(enc);
    if (eb == 0) throw std::invalid_argument("unknown sample encoding " + std::to_string(enc));
    return eb;
}

// Loudness on: the rows at the output rate are measured, then stored with the gain in the encoding.  Off: resampled straight into the
// destination in the encoding when a rate is set; at the native rate encoded by the store kernel, or (fp32) copied.
void Engine::enqueue_output(const OutRows& o) {
    if (o.join) { enqueue_joined(o); return; }
    const Batch& b = bt_;
    const int eb = need_enc(o.enc);
    const int64_t Wo = out_row_len(), W = native_row_len();
    if (o.stride < Wo)
        throw std::invalid_argument(resample_on() ? "dst_stride smaller than the waveform length at the output rate" : "dst_stride smaller than the waveform length");
    if (silence_trim_on()) {
        // section 14: the rows at the output rate (resampled into the fetch scratch first when a rate is set), their edges and per-row
        // programmes from the detection (cached per batch and setting), the gains as measured over the untrimmed spans, and the join's
        // store with one member per programme: row b's segment from column 0, zero codewords behind it
        const float* src = out_source(Wo);
        if (src == o.dst) throw std::logic_error("trimmed fetch: source and destination rows are the same");
        const EdScratch sc = ed_batch(src, Wo, pause_limit_active());  // (section 17: with the pause limit, the rows' several segments)
        const LoRes m = loudness_on() ? lo_batch(src, Wo, true) : LoRes{};
        const float* fade = st_window(output_rate());
        const GainedRows r = gain_step(src, b.B, Wo, out_in_scratch() ? Wo : W, m);  // (the untrimmed rows limited, then cut)
        StageSpan span(*this, "out", "trim_rows", (double)b.B * Wo, (double)b.B * Wo * (4 + eb));
        launch_join_trim_rows(s_, r.src, r.stride, sc.S > 0 ? sc.pseg : sc.seg, sc.S > 0 ? sc.pprog : sc.prog, b.B, Wo, r.g, fade, o.enc, o.dst, o.stride,
                              out_dither(DITHER_ROW));
    } else if (loudness_on()) {
        const float* src = out_source(Wo);  // (with an fp32 fetch at a set rate, the scratch is src and o.dst alike: scaled in place)
        const GainedRows r = gain_step(src, b.B, Wo, Wo, lo_batch(src, Wo, true));
        StageSpan span(*this, "out", "loudness_gain", (double)b.B * Wo, (double)b.B * Wo * (4 + eb));
        launch_store_rows(s_, r.src, b.B, Wo, r.g, o.enc, o.dst, o.stride, out_dither(DITHER_ROW));
    } else if (shapes_rows()) {
        // sections 18, 20, 21 and 25: the filtered, expanded, de-essed and / or compressed rows are in the fetch scratch; an fp32 fetch that was handed that scratch as its destination is done
        const float* src = out_source(Wo);
        if (src != o.dst) {
            StageSpan span(*this, "out", "store_rows", (double)b.B * Wo, (double)b.B * Wo * (4 + eb));
            launch_store_rows(s_, src, b.B, Wo, nullptr, o.enc, o.dst, o.stride, out_dither(DITHER_ROW));
        }
    } else if (resample_on() && dithers(o.enc)) {
        // section 23: the resampler's fused store truncates; a dithered fetch resamples into the fp32 scratch and ends in the one store
        // (one definition of the quantizer, one more pass over the rows)
        float* d = out_f32_buf((size_t)b.B * Wo);
        resample_enqueue(rs_table(), wav_rows(), b.B, W, ENC_F32, d, Wo);
        StageSpan span(*this, "out", "store_rows", (double)b.B * Wo, (double)b.B * Wo * (4 + eb));
        launch_store_rows(s_, d, b.B, Wo, nullptr, o.enc, o.dst, o.stride, out_dither(DITHER_ROW));
    } else if (resample_on()) {
        resample_enqueue(rs_table(), wav_rows(), b.B, W, o.enc, o.dst, o.stride);
    } else if (o.enc != ENC_F32) {
        const float* src = wav_rows();
        StageSpan span(*this, "out", "store_rows", (double)b.B * W, (double)b.B * W * (4 + eb));
        launch_store_rows(s_, src, b.B, W, nullptr, o.enc, o.dst, o.stride, out_dither(DITHER_ROW));
    } else {
        STN_HIP(hipMemcpy2DAsync(o.dst, (size_t)o.stride * 4, wav_rows(), (size_t)W * 4, (size_t)W * 4, (size_t)b.B, hipMemcpyDeviceToDevice, s_));
    }
    STN_HIP(hipGetLastError());
}

static void copy_durations(const std::vector<float>& dur, float* duration) {
    if (duration) std::copy(dur.begin(), dur.end(), duration);
}

void Engine::batch_fetch(float* wav, size_t wav_capacity, float* duration) {
    if (wav) {
        const size_t n = (size_t)bt_.B * out_row_len();
        if (wav_capacity < n) throw std::runtime_error("wav buffer too small: need " + std::to_string(n) + " floats");
    }
    batch_fetch_encoded(ENC_F32, wav, wav_capacity * 4, duration);
}
void Engine::batch_fetch_pcm16(int16_t* pcm, size_t capacity, float* duration) {
    const size_t n = (size_t)bt_.B * out_row_len();
    if (capacity < n) throw std::runtime_error("pcm buffer too small: need " + std::to_string(n) + " samples");
    batch_fetch_encoded(ENC_PCM16, pcm, capacity * 2, duration);
}
void Engine::batch_fetch_encoded(int enc, void* dst, size_t capacity_bytes, float* duration) {
    const int eb = need_enc(enc);
    if (dst) {
        const int64_t Wo = out_row_len();
        const size_t n = (size_t)bt_.B * Wo, bytes = n * eb;
        if (capacity_bytes < bytes) throw std::runtime_error("buffer too small: need " + std::to_string(bytes) + " bytes");
        const void* src = bt_.wav;  // fp32 at the native rate: the batch's own rows, no device copy
        if (enc != ENC_F32 || !out_native() || silence_trim_on()) {
            // (a trimmed fp32 fetch of rows in the scratch moves samples within their rows: its destination lies behind those rows)
            const size_t off = enc == ENC_F32 && silence_trim_on() && out_in_scratch() ? join_f32_offset(n) : 0;
            void* d = enc == ENC_F32 ? static_cast<void*>(out_f32_buf(off + n) + off) : static_cast<void*>(out_enc_buf(bytes));
            enqueue_output({d, enc, Wo});
            src = d;
        }
        STN_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s_));
    }
    sync();
    copy_durations(reported_dur_, duration);
}
void Engine::batch_fetch_encoded_begin(int slot, int enc) {
    if (slot < 0 || slot > 1) throw std::invalid_argument("fetch slot must be 0 or 1");
    need_enc(enc);
    const int64_t Wo = out_row_len();
    slot_begin(slot, {nullptr, enc, Wo}, bt_.B, Wo, reported_dur_);
}
void Engine::batch_fetch_joined_begin(int slot, const stn_join* j, int enc) {
    if (slot < 0 || slot > 1) throw std::invalid_argument("fetch slot must be 0 or 1");
    need_enc(enc);
    const JoinPlan p = batch_join_plan(j);
    slot_begin(slot, {nullptr, enc, join_stride(p), &p, j->gain_scope}, p.G, p.W_join, p.prog_dur);  // (the slot hands out G rows of W_join: fetch_slot_dims)
}
// rows of `width` samples through the output stage into the slot's device buffer, o.stride >= width samples apart (o.dst is set here), then
// packed into its pinned buffer on the copy stream
void Engine::slot_begin(int slot, OutRows o, int64_t rows, int64_t width, const std::vector<float>& dur) {
    const size_t eb = (size_t)enc_bytes(o.enc), nw = (size_t)rows * width, bytes = (size_t)rows * o.stride * eb;
    const int enc = o.enc;
    FetchSlot& f = fetch_[slot];
    if (!copy_s_) STN_HIP(hipStreamCreateWithFlags(&copy_s_, hipStreamNonBlocking));
    if (!f.ready) { STN_HIP(hipEventCreateWithFlags(&f.ready, hipEventDisableTiming)); STN_HIP(hipEventCreateWithFlags(&f.done, hipEventDisableTiming)); }
    if (f.busy) STN_HIP(hipEventSynchronize(f.done));  // the slot's previous copy (two batches ago) must be out before it is refilled
    if (bytes > f.cap) {
        if (f.dev) (void)hipFree(f.dev);
        if (f.pin) (void)hipHostFree(f.pin);
        f.dev = nullptr; f.pin = nullptr; f.cap = 0;
        const size_t cap = bytes + bytes / 4;
        STN_HIP(hipMalloc(reinterpret_cast<void**>(&f.dev), cap));
        STN_HIP(hipHostMalloc(reinterpret_cast<void**>(&f.pin), cap, hipHostMallocDefault));
        f.cap = cap;
    }
    o.dst = f.dev;
    enqueue_output(o);
    STN_HIP(hipEventRecord(f.ready, s_));
    STN_HIP(hipStreamWaitEvent(copy_s_, f.ready, 0));
    if (o.stride == width || rows == 1) STN_HIP(hipMemcpyAsync(f.pin, f.dev, nw * eb, hipMemcpyDeviceToHost, copy_s_));
    else STN_HIP(hipMemcpy2DAsync(f.pin, (size_t)width * eb, f.dev, (size_t)o.stride * eb, (size_t)width * eb, (size_t)rows, hipMemcpyDeviceToHost, copy_s_));
    STN_HIP(hipEventRecord(f.done, copy_s_));
    f.n = nw;
    f.enc = enc;
    f.dur = dur;
    f.busy = true;
}
void Engine::batch_fetch_encoded_end(int slot, const void** data, size_t* n_bytes, float* duration) {
    if (slot < 0 || slot > 1) throw std::invalid_argument("fetch slot must be 0 or 1");
    FetchSlot& f = fetch_[slot];
    if (!f.busy) throw std::runtime_error("no fetch in flight on this slot");
    STN_HIP(hipEventSynchronize(f.done));
    if (data) *data = f.pin;
    if (n_bytes) *n_bytes = f.n * enc_bytes(f.enc);
    copy_durations(f.dur, duration);
}
void Engine::batch_fetch_pcm16_begin(int slot) { batch_fetch_encoded_begin(slot, ENC_PCM16); }
void Engine::batch_fetch_pcm16_end(int slot, const int16_t** pcm, size_t* n, float* duration) {
    if (slot >= 0 && slot <= 1 && fetch_[slot].busy && fetch_[slot].enc != ENC_PCM16)
        throw std::runtime_error("the fetch on this slot is not 16-bit PCM (use stn_batch_fetch_encoded_end)");
    const void* d = nullptr;
    batch_fetch_encoded_end(slot, &d, nullptr, duration);
    if (pcm) *pcm = static_cast<const int16_t*>(d);
    if (n) *n = fetch_[slot].n;
}
void Engine::batch_copy_wav_device(float* dst, int64_t dst_stride) { enqueue_output({dst, ENC_F32, dst_stride}); }
void Engine::batch_copy_pcm16_device(int16_t* dst, int64_t dst_stride) { enqueue_output({dst, ENC_PCM16, dst_stride}); }
void Engine::batch_copy_encoded_device(int enc, void* dst, int64_t dst_stride) { enqueue_output({dst, enc, dst_stride}); }
void Engine::set_dither(int mode, uint64_t seed) {
    if (mode != DITHER_OFF && mode != DITHER_ROUND && mode != DITHER_TPDF && mode != DITHER_TPDF_HP)
        throw std::invalid_argument("dither mode " + std::to_string(mode) + ": must be STN_DITHER_OFF (0), _ROUND (1), _TPDF (2) or _TPDF_HP (3)");
    dither_.mode = mode;
    dither_.seed = seed;
}
void Engine::op_encode_ex(int enc, int rows, int W, const float* x, int x_misalign, const float* gain, const int64_t* row_id, int mode, uint64_t seed,
                          int64_t dst_stride, void* y) {
    const int eb = need_enc(enc);
    if (mode < DITHER_OFF || mode > DITHER_TPDF_HP) throw std::invalid_argument("dither mode " + std::to_string(mode) + ": must be 0 .. 3");
    if (x_misalign < 0 || x_misalign > 3) throw std::invalid_argument("x_misalign must be 0 .. 3 floats");
    if (dst_stride < W) throw std::invalid_argument("dst_stride smaller than the row length");
    OpScope op(*this);
    const size_t n = (size_t)rows * W, ny = (size_t)rows * dst_stride * eb;
    float* dx = op.buf<float>(n + 4) + x_misalign;  // (room for every offset, so that the block behind it never moves with it)
    op.put(dx, x, n);
    char* dy = op.up(static_cast<const char*>(y), ny);
    const float* dg = op.up(gain, (size_t)rows);
    const int64_t* di = op.up(row_id, (size_t)rows);
    launch_store_rows(s_, dx, rows, W, dg, enc, dy, dst_stride, Dither{mode, seed, DITHER_ROW, di});
    STN_HIP(hipGetLastError());
    op.down(static_cast<char*>(y), dy, ny);
    sync();
}
void Engine::op_encode(int enc, int rows, int W, const float* x, void* y) {
    const int eb = need_enc(enc);
    OpScope op(*this);
    const size_t n = (size_t)rows * W;
    const float* dx = op.up(x, n);
    char* dy = op.buf<char>(n * eb);
    launch_store_rows(s_, dx, rows, W, nullptr, enc, dy, W);
    STN_HIP(hipGetLastError());
    op.down(static_cast<char*>(y), dy, n * eb);
    sync();
}
// =================================================================================================
// join: the output stage's joined form
// =================================================================================================

JoinPlan Engine::batch_join_plan(const stn_join* j) {
    const int64_t Wo = out_row_len();  // (throws without a finished batch)
    const Batch& b = bt_;
    const int64_t cs = (int64_t)a_.base_chunk_size * a_.chunk_compress_factor;
    // member i's whole wave: what its own run would return, L_i * chunk samples at the output rate (cpp/helper.cpp:706-715)
    std::vector<int64_t> len((size_t)b.B);
    for (int i = 0; i < b.B; ++i) len[(size_t)i] = std::min<int64_t>(Wo, out_len((int64_t)b.h_llen[(size_t)i] * cs));
    JoinPlan p;
    if (silence_trim_on() && j && (j->mode == STN_JOIN_WHOLE || j->mode == STN_JOIN_TRIM)) {
        // section 14: a member's segment is [start_b, end_b) under either mode, its duration (float)len_b / (float)hz; the edges come
        // from the device (one read of 2 B integers per finished batch and setting)
        // (section 17: with the pause limit its length is len_b, what the cuts leave, and the rows' cut lists come with the edges)
        const bool pauses = pause_limit_active();
        const std::vector<int64_t>& e = ed_batch_host(pauses);
        const int hz = output_rate();
        const int64_t* n = batch_spans(hz, Wo).host.data();  // the rows' spans: a segment that ends before its row's does is faded out
        const int64_t fd = silence_samples(hz, st_fade_);
        std::vector<float> dur((size_t)b.B);
        for (int i = 0; i < b.B; ++i) {
            len[(size_t)i] = pauses ? pz_host_[(size_t)i * 2 * pz_S_ + 1] : e[(size_t)i * 2 + 1] - e[(size_t)i * 2];
            dur[(size_t)i] = (float)len[(size_t)i] / (float)hz;
        }
        stn_join jj = *j;
        jj.mode = STN_JOIN_WHOLE;  // (the lengths are the edges')
        const std::string why = join_plan(&jj, b.B, Wo, hz, len.data(), dur.data(), p);
        if (!why.empty()) throw std::invalid_argument(why);
        p.seg_src.resize((size_t)b.B); p.seg_fin.resize((size_t)b.B); p.seg_fout.resize((size_t)b.B);
        for (int i = 0; i < b.B; ++i) {
            const int64_t st = e[(size_t)i * 2], en = e[(size_t)i * 2 + 1], fl = std::min<int64_t>(fd, en - st);
            p.seg_src[(size_t)i] = st;
            p.seg_fin[(size_t)i] = st > 0 ? (int32_t)fl : 0;
            p.seg_fout[(size_t)i] = en < n[(size_t)i] ? (int32_t)fl : 0;
        }
        if (pauses) {  // member i's pieces: its row's segments in order, from the member's place in the programme
            p.piece_first.assign(1, 0);
            for (int i = 0; i < b.B; ++i) {
                const int64_t* wr = &pz_host_[(size_t)i * 2 * pz_S_];
                for (const PausePiece& q : pause_pieces(e[(size_t)i * 2], e[(size_t)i * 2 + 1], n[(size_t)i], wr + 2, (int)wr[0], fd)) {
                    p.piece_dst.push_back(p.seg_dst[(size_t)i] + q.dst); p.piece_len.push_back(q.len); p.piece_src.push_back(q.src);
                    p.piece_fin.push_back(q.fin); p.piece_fout.push_back(q.fout);
                }
                p.piece_first.push_back((int32_t)p.piece_dst.size());
            }
        }
    } else {
        const std::string why = join_plan(j, b.B, Wo, output_rate(), len.data(), reported_dur_.data(), p);
        if (!why.empty()) throw std::invalid_argument(why);
    }
    if (p.G > 65535) throw std::invalid_argument("join: more than 65535 programmes");
    return p;
}

// [B] members, then [G] programmes {len, first | count << 32}, then the [G] spans of the programmes, as int64 words: a member is {dst,
// len, source row}, the words of JoinSeg, or, from trimmed sources (p.seg_src set), {dst, len, source row, src, fin | fout << 32}, the
// words of JoinSegT
std::vector<int64_t> Engine::join_table_words(const JoinPlan& p, const std::vector<int64_t>& span) {
    static_assert(sizeof(JoinSeg) == 24 && sizeof(JoinSegT) == 40 && sizeof(JoinProg) == 16, "the join tables are uploaded as int64 words");
    const bool trim = !p.seg_src.empty(), pieces = !p.piece_first.empty();
    const size_t mw = trim ? 5 : 3, nm = p.pieces();
    std::vector<int64_t> w(nm * mw + (size_t)p.G * 3);
    for (int i = 0; i < p.B; ++i) {
        if (pieces) {  // (the pause limit: several words of the member's row)
            for (int32_t q = p.piece_first[(size_t)i]; q < p.piece_first[(size_t)i + 1]; ++q) {
                const JoinSegT sg{p.piece_dst[(size_t)q], p.piece_len[(size_t)q], i, p.piece_src[(size_t)q], p.piece_fin[(size_t)q], p.piece_fout[(size_t)q]};
                std::memcpy(&w[(size_t)q * mw], &sg, sizeof(sg));
            }
        } else if (trim) {
            const JoinSegT sg{p.seg_dst[(size_t)i], p.seg_len[(size_t)i], i, p.seg_src[(size_t)i], p.seg_fin[(size_t)i], p.seg_fout[(size_t)i]};
            std::memcpy(&w[(size_t)i * mw], &sg, sizeof(sg));
        } else {
            const JoinSeg sg{p.seg_dst[(size_t)i], p.seg_len[(size_t)i], i};
            std::memcpy(&w[(size_t)i * mw], &sg, sizeof(sg));
        }
    }
    for (int g = 0; g < p.G; ++g) {
        int32_t first = p.first[(size_t)g], last = g + 1 < p.G ? p.first[(size_t)g + 1] : p.B;
        if (pieces) { first = p.piece_first[(size_t)first]; last = p.piece_first[(size_t)last]; }
        const JoinProg pg{p.prog_len[(size_t)g], first, last - first};
        std::memcpy(&w[nm * mw + (size_t)g * 2], &pg, sizeof(pg));
    }
    std::copy(span.begin(), span.end(), w.end() - p.G);
    return w;
}

Engine::JoinTables Engine::join_tables_at(const int64_t* d, const JoinPlan& p) {
    const int64_t* prog = d + p.pieces() * (p.seg_src.empty() ? 3 : 5);
    if (p.seg_src.empty()) return {reinterpret_cast<const JoinSeg*>(d), reinterpret_cast<const JoinProg*>(prog), prog + (size_t)p.G * 2};
    return {nullptr, reinterpret_cast<const JoinProg*>(prog), prog + (size_t)p.G * 2, reinterpret_cast<const JoinSegT*>(d), st_window(output_rate())};
}

Engine::JoinTables Engine::join_tables(const JoinPlan& p) {
    std::vector<int64_t> w = join_table_words(p, join_spans(p));
    bool moved = false;
    int64_t* d = reinterpret_cast<int64_t*>(join_tab_.reserve(*this, w.size() * sizeof(int64_t), &moved));
    if (moved || w != join_tab_host_) {  // later fetches of the same batch under the same join reuse the upload
        join_tab_host_ = std::move(w);
        STN_HIP(hipMemcpyAsync(d, join_tab_host_.data(), join_tab_host_.size() * sizeof(int64_t), hipMemcpyHostToDevice, s_));
    }
    return join_tables_at(d, p);
}

void Engine::join_enqueue(const float* x, int64_t src_stride, const JoinTables& t, const JoinPlan& p, const float* g, int enc, void* y, int64_t dst_stride,
                          const Dither& d) {
    {
        StageSpan span(*this, "out", "join", (double)p.G * p.W_join, (double)p.G * p.W_join * (4 + enc_bytes(enc)));
        if (t.tseg) launch_join_trim_rows(s_, x, src_stride, t.tseg, t.prog, p.G, p.W_join, g, t.fade, enc, y, dst_stride, d);
        else launch_join_rows(s_, x, src_stride, t.seg, t.prog, p.G, p.W_join, g, enc, y, dst_stride, d);
    }
    STN_HIP(hipGetLastError());
}

// the fetch scratch of a joined fetch: the resampled and / or filtered rows (when there are any) in front, the joined fp32 rows
// (per-programme gain) behind
static size_t join_f32_offset(size_t n_rows) { return (n_rows + 3) / 4 * 4; }

const float* Engine::join_f32(const JoinPlan& p) {
    const Batch& b = bt_;
    const int64_t Wo = out_row_len();
    const size_t off = out_in_scratch() ? join_f32_offset((size_t)b.B * Wo) : 0;
    float* base = out_f32_buf(off + (size_t)p.G * p.W_join);  // (sized once: out_source below then finds room and moves nothing)
    const float* src = out_source(Wo);
    join_enqueue(src, out_in_scratch() ? Wo : native_row_len(), join_tables(p), p, nullptr, ENC_F32, base + off, p.W_join);
    return base + off;
}

std::vector<int64_t> Engine::join_spans(const JoinPlan& p) const {
    const int hz = output_rate();
    std::vector<int64_t> n((size_t)p.G);
    for (int g = 0; g < p.G; ++g)
        n[(size_t)g] = std::max<int64_t>(0, std::min<int64_t>(p.prog_len[(size_t)g], (int64_t)(p.prog_dur[(size_t)g] * (float)hz)));
    return n;
}

// (the programmes' spans ride in the plan's tables: whoever joined the rows, join_f32, has uploaded them, and join_tables finds them)
Engine::LoRes Engine::join_measure(const JoinPlan& p, const float* joined, bool on) {
    lo_prepare(lo_, output_rate());
    const std::vector<int64_t> n = join_spans(p);
    return lo_rows(lo_.t, joined, p.G, p.W_join, join_tables(p).span, lr_max_seg(lo_.t, n.data(), n.size()), on, lo_target_, lo_cap(), lo_true_peak());
}

// Loudness off: one join launch behind the optional resample.  On, per member row: the rows measured as every fetch measures them, then
// the join with g_b.  On, per programme: joined as fp32, measured as G rows, stored with g_g by the store kernel.
void Engine::enqueue_joined(const OutRows& o) {
    const Batch& b = bt_;
    const JoinPlan& p = *o.join;
    const int eb = need_enc(o.enc);
    const int64_t Wo = out_row_len(), W = native_row_len();
    if (o.stride < p.W_join) throw std::invalid_argument("dst_stride smaller than the joined length W_join = " + std::to_string(p.W_join));
    if (p.W_join == 0) return;
    if (loudness_on() && o.scope == STN_JOIN_GAIN_PROG) {
        const float* joined = join_f32(p);
        const GainedRows r = gain_step(joined, p.G, p.W_join, p.W_join, join_measure(p, joined, true));  // (G rows, each its programme's gain and span)
        Dither d = out_dither(DITHER_PROG);
        // (section 23: a programme's stream ends at its length; the lengths are the words of the plan's table, which join_f32 left on the device)
        if (dithers(o.enc)) { d.lim = &join_tables(p).prog->len; d.lim_stride = sizeof(JoinProg) / sizeof(int64_t); }
        {
            StageSpan span(*this, "out", "loudness_gain", (double)p.G * p.W_join, (double)p.G * p.W_join * (4 + eb));
            launch_store_rows(s_, r.src, p.G, p.W_join, r.g, o.enc, o.dst, o.stride, d);
        }
        STN_HIP(hipGetLastError());
        return;
    }
    const float* src = out_source(Wo);
    const GainedRows r = gain_step(src, b.B, Wo, out_in_scratch() ? Wo : W, loudness_on() ? lo_batch(src, Wo, true) : LoRes{});  // (the segments are the limited rows)
    join_enqueue(r.src, r.stride, join_tables(p), p, r.g, o.enc, o.dst, o.stride, out_dither(DITHER_PROG));
}

static int64_t join_stride(const JoinPlan& p) { return (p.W_join + 15) / 16 * 16; }  // a multiple of every encoding's vector

static void copy_plan(const JoinPlan& p, int64_t* prog_len, float* prog_dur) {
    if (prog_len) std::copy(p.prog_len.begin(), p.prog_len.end(), prog_len);
    if (prog_dur) std::copy(p.prog_dur.begin(), p.prog_dur.end(), prog_dur);
}

void Engine::batch_fetch_joined(const stn_join* j, int enc, void* dst, size_t capacity_bytes, int64_t* prog_len, float* prog_dur) {
    const int eb = need_enc(enc);
    const JoinPlan p = batch_join_plan(j);
    if (dst) {
        const size_t bytes = (size_t)p.G * p.W_join * eb;
        if (capacity_bytes < bytes) throw std::invalid_argument("joined buffer too small: need " + std::to_string(bytes) + " bytes");
        if (bytes) {
            // on the device the rows lie join_stride samples apart, so that every row starts 16-byte aligned and the join stores full
            // width whatever W_join is; the copy packs them
            const int64_t Ws = join_stride(p);
            void* d = out_enc_buf((size_t)p.G * Ws * eb);
            enqueue_output({d, enc, Ws, &p, j->gain_scope});
            if (Ws == p.W_join || p.G == 1) STN_HIP(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, s_));
            else STN_HIP(hipMemcpy2DAsync(dst, (size_t)p.W_join * eb, d, (size_t)Ws * eb, (size_t)p.W_join * eb, (size_t)p.G, hipMemcpyDeviceToHost, s_));
        }
    }
    sync();
    copy_plan(p, prog_len, prog_dur);
}

void Engine::batch_copy_joined_device(const stn_join* j, int enc, void* dst, int64_t dst_stride) {
    need_enc(enc);
    const JoinPlan p = batch_join_plan(j);
    enqueue_output({dst, enc, dst_stride, &p, j->gain_scope});
}

void Engine::batch_join_loudness(const stn_join* j, float* lufs, float* peak, float* gain) {
    const JoinPlan p = batch_join_plan(j);
    if (p.W_join == 0) throw std::invalid_argument("join: every programme is empty");
    lo_read_back(join_measure(p, join_f32(p), lo_on_), (size_t)p.G, lufs, peak, gain);
    sync();
}

void Engine::batch_join_loudness_range(const stn_join* j, float* m_max, float* s_max, float* lra, int32_t* n_st) {
    const JoinPlan p = batch_join_plan(j);
    if (p.W_join == 0) throw std::invalid_argument("join: every programme is empty");
    const LoRes m = join_measure(p, join_f32(p), lo_on_);
    const std::vector<int64_t> n = join_spans(p);
    lr_report(lo_.t, p.G, p.W_join, m.n, lr_max_seg(lo_.t, n.data(), n.size()), m_max, s_max, lra, n_st);
    sync();
}

void Engine::op_join(int hz, int rows, int W, const float* x, const int64_t* n, const stn_join* j, int enc, bool loudness_on, float target_lufs,
                     float ceiling_dbfs, void* y, float* prog_lufs, float* prog_peak, float* prog_gain) {
    const int eb = need_enc(enc);
    OpScope op(*this);
    JoinPlan p;
    stn_join jj = *j;
    jj.mode = STN_JOIN_WHOLE;  // (the lengths are the caller's)
    if (j->mode != STN_JOIN_WHOLE && j->mode != STN_JOIN_TRIM) throw std::invalid_argument("join: unknown mode " + std::to_string(j->mode));
    const std::string why = join_plan(&jj, rows, W, hz, n, nullptr, p);
    if (!why.empty()) throw std::invalid_argument(why);
    if (p.G > 65535) throw std::invalid_argument("join: more than 65535 programmes");
    const bool measure = loudness_on || prog_lufs || prog_peak || prog_gain;
    if (measure) {
        refuse(loudness_check(&target_lufs, ceiling_dbfs));
        lo_prepare(op_lo_, hz);
    }
    if (p.W_join == 0) throw std::invalid_argument("join: every programme is empty");
    const size_t ny = (size_t)p.G * p.W_join;
    const float* dx = op.up(x, (size_t)rows * W);
    char* dy = op.buf<char>(ny * eb);
    const std::vector<int64_t> words = join_table_words(p, p.prog_len);  // (a programme is measured over its whole length)
    const JoinTables t = join_tables_at(op.up(words), p);
    if (!measure) {
        join_enqueue(dx, W, t, p, nullptr, enc, dy, p.W_join);
    } else {
        float* dj = op.buf<float>(ny);
        join_enqueue(dx, W, t, p, nullptr, ENC_F32, dj, p.W_join);
        const LoRes res = lo_rows(op_lo_.t, dj, p.G, p.W_join, t.span, lr_max_seg(op_lo_.t, p.prog_len.data(), p.prog_len.size()), loudness_on, target_lufs,
                                  ceiling_dbfs);
        launch_store_rows(s_, dj, p.G, p.W_join, res.gain, enc, dy, p.W_join);
        STN_HIP(hipGetLastError());
        lo_read_back(res, (size_t)p.G, prog_lufs, prog_peak, prog_gain);
    }
    op.down(static_cast<char*>(y), dy, ny * eb);
    sync();
}
void Engine::batch_fetch_latent(float* latent) {
    Batch& b = bt_;
    const size_t nx = (size_t)b.B * a_.latent_dim * a_.chunk_compress_factor * b.L;
    STN_HIP(hipMemcpyAsync(latent, b.xt[final_xt_], nx * 4, hipMemcpyDeviceToHost, s_));
    sync();
}

}  // namespace stn
