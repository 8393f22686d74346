// engine.hpp — MI355X-native executor of the four Supertonic graphs.
//
// Replaces what the reference does with four `Ort::Session`s (/root/reference/cpp/helper.cpp:776-795) and
// their `Run` calls (:519, :552, :643, :668).  One Engine = one GPU + one HIP stream; all stages are
// enqueued on that stream with no host round trip except the single read of the predicted durations that
// sizes the latent (cpp/helper.cpp:430-438 needs max(duration) on the host too).
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <initializer_list>
#include <iterator>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/stn_arch.h"
#include "host/len_tables.hpp"
#include "host/join_plan.hpp"
#include "host/pause_plan.hpp"
#include "host/formant.hpp"
#include "host/pitch.hpp"
#include "kernels.hpp"

namespace stn {

#define STN_HIP(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr);       \
    } while (0)

struct DevTensor {
    float* f32 = nullptr;      // canonical fp32 copy (layout noted per tensor)
    uint16_t* bf16 = nullptr;  // 16-bit copy for GEMM operands (matrices only) in the engine's format: bf16, or IEEE half for F16 engines
    int rows = 0, cols = 0;
    const void* as(int dt) const { return is_half(dt) ? static_cast<const void*>(bf16) : static_cast<const void*>(f32); }
};

struct Linear { DevTensor w; const float* b = nullptr; int N = 0, K = 0; };
struct LNorm { const float* g = nullptr; const float* b = nullptr; };
struct ConvNeXt { const float* dw_t = nullptr; const float* dw_b = nullptr; LNorm ln; Linear pw1, pw2; const float* gamma = nullptr; };
struct Attn { LNorm ln; Linear q, kv, qkv, o; };  // kv = [Wk; Wv] rows, qkv = [Wq; Wk; Wv] rows

// Grow-only chunked device workspace.  Stage code takes mark()/release() pairs; all work is stream-ordered,
// chunks are never freed before the Engine dies, so pointers handed out stay valid while kernels run.
// New chunks are hipMalloc'ed only the first time a shape needs them (warm-up), never afterwards.
class Arena {
   public:
    struct Mark { size_t chunk, off; };
    Arena() = default;
    Arena(const Arena&) = delete;             // owns device memory: a copy would free it twice
    Arena& operator=(const Arena&) = delete;
    ~Arena();
    void swap(Arena& o) { chunks_.swap(o.chunks_); std::swap(cur_, o.cur_); std::swap(off_, o.off_); }
    void* alloc(size_t bytes);
    Mark mark() const { return {cur_, off_}; }
    void release(Mark m) { cur_ = m.chunk; off_ = m.off; }
    void reset() { cur_ = 0; off_ = 0; }
    size_t capacity() const;

   private:
    struct Chunk { char* p; size_t cap; };
    std::vector<Chunk> chunks_;
    size_t cur_ = 0, off_ = 0;
};

// Silence trimming's host arithmetic (engine_edges.cpp): why (top_db, keep_ms, fade_ms) is refused, or ""; a length in ms as samples at
// hz, (int64)(ms * hz / 1000 + 0.5) in double; the raised-cosine fade of that many samples, float32(0.5 - 0.5 cos(pi (j + 0.5) / Fd))
std::string silence_check(float top_db, float keep_ms, float fade_ms);
int64_t silence_samples(int hz, float ms);
std::vector<float> silence_fade_window(int hz, float fade_ms);
// The limiter's host arithmetic (engine_limiter.cpp): why (hz, lookahead_ms) is refused, or ""; the look-ahead A in samples at hz,
// (int64)(ms * hz / 1000 + 0.5) in double; the A + 1 Hann weights 0.5 - 0.5 cos(2 pi (k + 1) / (A + 2)), normalized to sum 1 in
// double, as float32
std::string limiter_check(int hz, float lookahead_ms);
int64_t limiter_samples(int hz, float lookahead_ms);
std::vector<float> limiter_window(int hz, float lookahead_ms);

// Argument checks the settings and the op entries share (engine_loudness.cpp).  rate_check: why hz is refused for the feature named
// `what`, or ""; loudness_check: why a target (not checked when null) or a ceiling is refused, or ""; refuse: throws a reason that is
// not ""; spans: row r's span n[r] (W when n is null) of rows x W, or throws "<who>: n[r] = ... outside [0, W]"
std::string rate_check(const char* what, int hz);
std::string loudness_check(const float* target_lufs, float ceiling_dbfs);
inline void refuse(const std::string& why) { if (!why.empty()) throw std::invalid_argument(why); }
std::vector<int64_t> spans(const char* who, int rows, int W, const int64_t* n);
// The filter chain's host arithmetic (engine_filter.cpp).  filter_check: why f[0 .. n) is refused at rate_hz, naming the field, or "";
// filter_design: one section's b0 b1 b2 a1 a2 in double (RBJ cookbook, a0 = 1); FilterTable: the chain at hz as section passes of two
// biquads (an odd count padded with the identity), each a LoudTable of fp32 coefficients and scan powers (hop = 1, unused)
std::string filter_check(int n, const stn_filter* f, int rate_hz);
void filter_design(const stn_filter& f, int rate_hz, double c[5]);
struct FilterTable {
    int hz = 0;
    std::vector<stn_filter> f;
    std::vector<LoudTable> pass;
};
void filter_table(int hz, int n, const stn_filter* f, FilterTable& t);  // fills t (no device copies); throws what filter_check refuses
// The compressor's host arithmetic (engine_compressor.cpp).  compressor_check: why c is refused, naming the field, or "" (no limit
// depends on the rate); compressor_k: k = -expm1(-1000 / (ms rate)) in double; compressor_curve: the static curve in double on the
// fp32-rounded T, S, K and makeup; compressor_table: coefficients and scan powers at hz (no device copy), throws what the check refuses
std::string compressor_check(const stn_compressor* c);
double compressor_k(float ms, int rate_hz);
double compressor_curve(const stn_compressor& c, double in_db);
void compressor_table(int hz, const stn_compressor& c, CompTable& t);
// The de-esser's host arithmetic (engine_deesser.cpp).  deesser_check: why c is refused at rate_hz (0: the limits that need no rate
// only), naming the field, or ""; deesser_band: the two Butterworth high-pass sections at c.freq_hz, as filter_check takes them;
// deesser_table: band, detector coefficients and the scans' powers at hz (no device copies), throws what the check refuses
std::string deesser_check(const stn_deesser* c, int rate_hz);
void deesser_band(const stn_deesser& c, stn_filter f[2]);
void deesser_table(int hz, const stn_deesser& c, DeessTable& t);
// The expander's host arithmetic (engine_expander.cpp).  expander_check: why c is refused, naming the field, or "" (no limit depends on
// the rate); expander_curve: the static curve in double on the fp32-rounded T, S, K and R; expander_table: coefficients (kA, delta, Bh
// and the hold in samples) and scan tables at hz (no device copy), throws what the check refuses
std::string expander_check(const stn_expander* c);
double expander_curve(const stn_expander& c, double in_db);
void expander_table(int hz, const stn_expander& c, ExpTable& t);

class Engine;
class OpScope;
// One grow-only device buffer of the output stage's fetch scratch (not part of the resident batch: growing it re-keys no captured
// graph).  reserve returns the block, of at least `bytes`; a block too small is replaced, behind a sync of the engine (a fetch in
// flight may still read it), by one a quarter larger than asked, and *moved (when given) says so: what the old block held is gone.
// A pointer from reserve is valid until the next larger reserve on the same buffer: a caller that hands one out sizes the buffer up
// front for every use that follows.  Freed with the engine, after its streams are drained.
class DevBuf {
   public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p_) (void)hipFree(p_); }
    char* reserve(Engine& e, size_t bytes, bool* moved = nullptr);
    const void* get() const { return p_; }

   private:
    char* p_ = nullptr;
    size_t cap_ = 0;
};

// The device copy of a constant host table, owned: freed with its owner (an engine member: after the destructor's body has drained the
// streams, as DevBuf).  put replaces the contents from host memory and returns the new block: allocate, upload, wait, free the old one.
// It always waits, because the upload reads the caller's host array and a fetch in flight may still read the old block: one wait per
// handle and setting (a table is designed when its rate or setting changes), never one per fetch.
class DeviceTable {
   public:
    DeviceTable() = default;
    DeviceTable(const DeviceTable&) = delete;
    DeviceTable& operator=(const DeviceTable&) = delete;
    ~DeviceTable() { if (p_) (void)hipFree(p_); }
    void* put(Engine& e, const void* host, size_t bytes);
    template <typename T> T* put(Engine& e, const std::vector<T>& host) { return static_cast<T*>(put(e, host.data(), host.size() * sizeof(T))); }
    explicit operator bool() const { return p_ != nullptr; }

   private:
    void* p_ = nullptr;
};
// A constant table as the launchers take it (t; its `dev` pointers point into dev) with the N device copies it needs
template <typename Table, size_t N = 1>
struct OnDevice { Table t; DeviceTable dev[N]; };

// Row spans on the device, [rows] each: n[r] the valid samples of row r, full[r] the row width (the lengths of a launch over whole rows)
struct RowSpans { const int64_t* n = nullptr; const int64_t* full = nullptr; };

// Consecutive arrays from a block, each on a 256-byte boundary of it.  Without a block (null) no pointer is formed: off, the bytes
// taken so far, is then the size the same sequence of take calls needs.
struct Carve {
    char* base = nullptr;
    size_t off = 0;
    template <typename T> T* take(size_t count) {
        const size_t o = off;
        off += (count * sizeof(T) + 255) / 256 * 256;
        return base ? reinterpret_cast<T*>(base + o) : nullptr;
    }
};

// The output stage's chain: the stages that shape the rows a fetch delivers, in the order Engine::out_source runs them.  A stage sees
// the rows of every stage in front of it and of none behind it.
enum Stage : int { ST_PITCH, ST_RATE, ST_FILTER, ST_EXPANDER, ST_DEESSER, ST_COMPRESSOR, N_STAGES };
// The rows at one point of the chain (Engine::rows_id): the finished batch's waveform, the output rate, the row length and the
// generation of every stage up to and including that point; the later ones stay 0.  Whatever is kept of such rows holds one as its key.
struct RowsId {
    uint64_t seq = 0; int hz = 0; int64_t Wo = 0; uint64_t gen[N_STAGES] = {};
    bool operator==(const RowsId& o) const { return seq == o.seq && hz == o.hz && Wo == o.Wo && std::equal(gen, gen + N_STAGES, o.gen); }
};
// One dynamics stage of the chain (expander, de-esser, compressor): what the shared host skeleton (engine_internal.hpp) works on.  The
// limits, the curve, the table, the scratch layout and the launches are the stage's own (engine_<stage>.cpp).
template <typename Set, typename Table>
struct DynStage {
    bool on = false;
    Set set;                       // the setting in force (the "speech" default until one is set)
    uint64_t gen = 0;              // bumped by every change of the setting
    struct Made { Table t; Set from{}; DeviceTable dev[2]; };  // a table, the setting it was made from and its device copies
    Made tab, op_tab;              // at the output rate, and of the op entry
    DevBuf buf;                    // fetch-time scratch of the launches: exists only once a fetch ran with the stage on
    RowsId key; const void* key_buf = nullptr; bool valid = false;            // what the row results in buf belong to, and the scratch
};

struct KernelStat { double ms = 0; long launches = 0; double flops = 0; double bytes = 0; };

class Engine {
   public:
    Engine(int device, int dtype);
    ~Engine();
    Engine(const Engine&) = delete;

    void load_synthetic(const stn_arch& a, uint64_t seed);
    // canonical tensors by name from any source (ONNX initializers through a manifest, ...): fn(name, rows, cols) must return
    // rows*cols floats in the canonical layout (Linear [N][K]; depthwise [C][k]; vocoder input conv [Cout][Cin][k]; 1-D as [1][n])
    using TensorSource = std::function<std::vector<float>(const std::string& name, int rows, int cols)>;
    void load_tensors(const stn_arch& a, const TensorSource& src);
    std::vector<std::string> tensor_names(const stn_arch& a);  // every canonical tensor the descriptor implies (no device work)
    bool loaded() const { return loaded_; }
    const stn_arch& arch() const { return a_; }
    int64_t param_count() const { return params_; }
    int dtype() const { return dt_; }
    hipStream_t stream() const { return s_; }
    void sync() { STN_HIP(hipStreamSynchronize(s_)); if (dp_s_) STN_HIP(hipStreamSynchronize(dp_s_)); if (te_s_) STN_HIP(hipStreamSynchronize(te_s_)); ++drains_; }
    // run on a caller-owned stream (e.g. torch's current stream, so RCCL ops order after the engine's kernels);
    // nullptr returns to the engine's own stream
    void set_stream(hipStream_t s);

    // ---- device-level stages (all pointers device, enqueued on stream()) -------------------------
    // lengths are int32 [B] on device.
    struct Ragged;  // packed rows (defined below)
    // trg (optional): the text positions as packed rows (sum of tlen rows, off[b] = first row of utterance b)
    void duration_dev(int B, int Lt, const int64_t* ids, const float* style_dp, const int* tlen, float* dur, const Ragged* trg = nullptr);
    // emits text_emb as NCL fp32 [B,Ce,Lt] (if ncl) and/or as rows [B*Lt][Ce] in the act dtype (if rows)
    void text_enc_dev(int B, int Lt, const int64_t* ids, const float* style_ttl, const int* tlen, float* ncl, void* rows,
                      const Ragged* trg = nullptr);
    struct VeCtx { void* text_kv = nullptr; void* style_kv = nullptr; int Lt = 0; const int* text_off = nullptr; };  // step-invariant K/V
    // tlen: text lengths (the text keys are rotated here, once, with their length-aware positions)
    // defer_text: allocate the text K/V but leave them to ve_text_kv_dev (batch_run computes them behind the text-row hand-over)
    VeCtx ve_prepare_dev(int B, int Lt, const void* text_rows, const float* style_ttl, const int* tlen, const Ragged* trg = nullptr, bool defer_text = false);
    void ve_text_kv_dev(const VeCtx& c, int B, int Lt, const void* text_rows, const int* tlen, const Ragged* trg);
    // time conditioning of `rows` (= B x steps) (current, total) pairs -> tb [rows][main_blocks * C] (fp32, arena)
    float* ve_time_cond_dev(int rows, const float* total_step, const float* current_step, float* tb_out = nullptr /* else: from the arena */);
    // The resident batch's time conditioning depends on (total_step, B, weights) and on nothing the caller uploads — every utterance of a run has the same
    // step counters — so it is computed once per such triple into a persistent buffer, eagerly and outside the captured pipeline, instead of by every
    // synthesis (time embedding + three exact-fp32 GEMMs + the step counters: ~75 us of a 10.8 ms batch, five launches)
    struct TimeCond { int steps = 0, B = 0; uint64_t wgen = ~0ull; float* buf = nullptr; size_t cap = 0; float *tot = nullptr, *cur = nullptr, *dt = nullptr, *tb = nullptr; };
    TimeCond tcond_;
    void ensure_time_cond(int total_step, int B);
    // tb: rows of this step's time conditioning ([B][main_blocks*C]); nullptr -> computed here from the step counters
    // Packed ("ragged") latent rows: utterance b owns rows off[b] .. off[b] + llen[b] and no padding rows exist; `rows` is
    // their total.  The masked stages are row-independent, so this is an exact optimisation of the padded [b*L + t] layout.
    struct Ragged { const int* off = nullptr; const int* row_b = nullptr; int rows = 0;
                    const int* hs_pairs = nullptr;  // (latent rows) which two utterances share a workgroup of the head-split cross-attention
                    int fold_run = 0; };            // (latent rows) run length of fold_dwconv_ln's workgroups for these lengths (fold_run_frames; 0: default)
    void ve_step_dev(int B, int L, const VeCtx& c, const float* noisy, const int* tlen, const int* llen,
                     const float* total_step, const float* current_step, float* denoised, const float* tb = nullptr,
                     const Ragged* rg = nullptr, const float* dt = nullptr /* 1/total_step per utterance, if precomputed */,
                     void* z_rows = nullptr /* [rows][D padded to 64] act, columns >= D zero: persistent across the steps of one synthesis */,
                     bool z_ready = false /* z_rows already holds `noisy` as rows (the step before wrote it) */,
                     bool z_next = false /* write `denoised` into z_rows as rows for the step after */);
    // vlen (optional, device [B]): valid vocoder frames per utterance — the length-aware mode (see set_vocoder_mode)
    // vrows > 0 (with vlen): run the vocoder on packed rows — vrows = sum of vlen — and unpack into the padded wav at the end
    // valid (with vlen, vrows): the exact trimmed DENSE mode — rows are computed on vlen[b] frames, exact below valid[b], and
    // the rest of each row is the cached zero-latent response (quiet chunk + edge tail)
    // tails (with valid): the blocks' conv taps beyond vlen[b] read the cached per-layer tails instead of zero (VO_TRIM_TAIL)
    // voff (packed rows): the row offsets [B + 1] of vlen where the caller already holds them (the length tables); null: launch_row_map computes them
    void vocoder_dev(int B, int L, const float* latent, float* wav, const int* vlen = nullptr, int vrows = 0,
                     const int* valid = nullptr, bool tails = false, const int* voff = nullptr);
    int vocoder_receptive_field() const;  // frames on either side that one output frame depends on
    void prepare_xattn_weights();         // fragment-ordered copies of the estimator's cross-attention Wq / Wo (kernels_xattn_hs.hip)
    std::unordered_map<const void*, const void*> frag_w_;  // row-major 16-bit matrix -> its fragment-ordered copy
    // diagnostics: stamps of the head-split cross-attention launches (stn_dbg_xattn_hs_*)
    void hs_stamps_enable(bool on);
    int64_t hs_stamps_fetch(unsigned long long* out, size_t cap);
    unsigned long long* hs_ts_ = nullptr;  // 8 values per workgroup, HS_TS_WG workgroups
    int hs_ts_wgs_ = 0;                    // workgroups of the last stamped launch
    static constexpr int HS_TS_WG = 8192;
    const float* unit_vec_ = nullptr;  // 1024 ones, then 1024 zeros: layer scale / bias of a fold that has none (the head-split block's output: gamma = 1)
    std::unordered_map<const void*, const void*> frag_acc_w_;  // ... -> its copy in accumulator-operand k order (Wo of the head-split block, kernels_xattn_hs.hip)
    void prepare_vocoder_constants();     // zero-latent response of the loaded model: quiet chunk, edge tail and the per-layer tails
    void prepare_ffn_weights();           // fragment-ordered copies of every ConvNeXt block's pw1 / pw2 (kernels_ffn.hip, K4)
    struct FfnW { const void *wseq = nullptr, *wsplit[std::size(FFN_SPLITS)] = {}; };  // wsplit: the estimator's K4-split streams, one per FFN_SPLITS entry
    std::unordered_map<const void*, FfnW> ffn_w_;  // key: the block's row-major 16-bit pw1 matrix

    // ---- host-pointer stages: 1:1 with the reference's four Run sites ------------------------------
    void duration(int B, int Lt, const int64_t* ids, const float* style_dp, const float* text_mask, float* dur);
    void text_enc(int B, int Lt, const int64_t* ids, const float* style_ttl, const float* text_mask, float* text_emb);
    void vector_est(int B, int L, int Lt, const float* noisy, const float* text_emb, const float* style_ttl,
                    const float* text_mask, const float* latent_mask, const float* total_step,
                    const float* current_step, float* denoised);
    void vocoder(int B, int L, const float* latent, float* wav);

    // ---- resident batch: upload once, run on device, fetch --------------------------------------------
    struct Batch {
        int B = 0, Lt = 0, L = 0, noise_L = 0, total_step = 0;
        float speed = 1.f;
        bool have_override = false, have_noise = false;
        uint64_t noise_seed = 0;
        // device buffers persist across uploads and only ever grow (no hipFree/hipMalloc per request; a captured graph
        // stays valid while `gen` — bumped by every reallocation — is unchanged)
        int64_t* ids = nullptr; size_t ids_cap = 0;
        int* tlen = nullptr; size_t tlen_cap = 0;
        float* style_ttl = nullptr; size_t ttl_cap = 0;
        float* style_dp = nullptr; size_t dp_cap = 0;
        float* dur = nullptr; size_t dur_cap = 0;
        int* llen = nullptr;                      // the latent lengths: tab + LenTables::llen (set by batch_run)
        int* tab = nullptr; size_t tab_cap = 0;   // the length tables of the run (host/len_tables.hpp), uploaded by the pipeline's one copy node
        LenTables tl;                             // their layout
        int64_t* utt_ids = nullptr; size_t utt_cap = 0;
        float* noise = nullptr; size_t noise_cap = 0;   // injected noise [B,D,L] (optional)
        float* xt[2] = {nullptr, nullptr}; size_t xt_cap[2] = {0, 0};
        float* wav = nullptr; size_t wav_cap = 0;        // [B, L*cs]
        // text-encoder output rows: written on the side stream (text_side), copied at the head of the main pipeline into the
        // buffer the captured graphs read (text_rows) — so the encoder of run i+1 can work while run i still reads its rows
        unsigned char* text_side = nullptr; size_t text_side_cap = 0;
        unsigned char* text_rows = nullptr; size_t text_cap = 0;
        int* toff = nullptr; size_t toff_cap = 0;       // packed text rows: first row of each utterance [B+1]
        int trows = 0;                                   // sum of the text lengths
        uint64_t gen = 0;
        std::vector<float> h_dur; std::vector<int> h_llen;
    };
    void batch_upload(int B, int Lt, const int64_t* ids, const float* text_mask, const float* style_ttl,
                      const float* style_dp, const float* duration_override, const int64_t* utt_ids);
    void batch_set_noise(const float* noise, int L);  // injected xt for the L the durations imply
    void batch_run(int total_step, float speed, uint64_t noise_seed);
    // hipGraph replay of the post-duration pipeline (text encoder, noise, Euler loop, vocoder): captured the second time
    // a shape is seen, replayed afterwards; per-call data (latent lengths, noise seed) travel through pinned host buffers.
    void set_graph_mode(bool on) { graph_on_ = on; }
    // length-aware vocoder in batch_run: every utterance's frames end at its own length, as in a batch-of-one run
    void set_vocoder_mode(bool length_aware) { vo_ragged_ = length_aware; }
    // vector-estimator row layout in batch_run: packed rows (default) or the padded [b*L + t] rows (tests compare the two)
    void set_packed_rows(bool on) { packed_ve_ = on; }
    // GELU form of the loaded model: 0 = erf (the default: torch.nn.GELU()), 1 = the tanh approximation.  stn_load_dir sets it from how the
    // graphs spell the activation (graph_bind Result::gelu); fp32 and f16 results follow it exactly, bf16 stores take the tanh-form
    // shortcut for both (|difference to erf| <= 5e-4, below half a bf16 ulp where it matters), and the fused K4 kernels compute the
    // exp2 (= tanh) form in both 16-bit modes.
    void set_gelu_form(int tanh_form) { if ((tanh_form != 0) != (gelu_act_ == ACT_GELU_TANH)) { sync(); drop_graphs(); } gelu_act_ = tanh_form ? ACT_GELU_TANH : ACT_GELU; }
    int gelu_form() const { return gelu_act_ == ACT_GELU_TANH ? 1 : 0; }
    // Shape buckets for the graph cache (the service path: requests of unlike lengths).  A captured pipeline has every size baked in:
    // B, Lt, L and the packed row counts (sum of the latent lengths, of the token counts, the vocoder's rows).  With buckets on, Lt, L and
    // the three row counts are rounded UP to a bucket boundary (bucket_up: four buckets per octave, <= 25 % padding) — the utterances'
    // own lengths stay exact and travel through device memory, so two requests that fall into the same buckets replay ONE graph.  Rows
    // behind the last sequence are dead: the row-independent kernels compute garbage there that nothing reads, the per-sequence kernels
    // never touch them, and every utterance's result over its own frames is bit-identical to the unbucketed run.  What changes for the
    // caller: stn_batch_dims reports the bucketed L (and W = L * chunk samples) and the fetched rows are that long.  B stays exact.
    // (No cached graph is dropped by the switch: a graph is fully described by the sizes in its key, bucketed or not.)
    void set_shape_buckets(bool on) { shape_buckets_ = on; }
    static int64_t bucket_up(int64_t x, int64_t min_gran) {
        if (x <= 0) return x;
        int64_t g = min_gran;
        while (g * 8 <= x) g *= 2;  // granularity = a quarter .. an eighth of x, at least min_gran: 4 - 8 buckets per octave
        return (x + g - 1) / g * g;
    }
    // measurement aid (bench.py `lone_batch_predicted_path`): with durations forced for shape control the predictor's device->host read
    // is skipped; this switch performs the read and the wait anyway, so the timed critical path is that of a predicted-duration run
    void set_duration_read(bool always) { dur_read_always_ = always; }
    // cross-attention blocks of the estimator head-split (kernels_xattn_hs.hip) instead of four launches
    void set_fused_xattn(int mode) { fused_xattn_ = mode ? 1 : 0; }  // 0: four launches; otherwise head-split (fold_ln + one launch, kernels_xattn_hs.hip)
    // K4: the pointwise pair of a ConvNeXt block as one launch.  Bit mask over the stages: 1 = vocoder, 2 = vector estimator,
    // 4 = text encoder / duration predictor.  16-bit engines, widths 384 / 512 (ffn_fused_supported)
    // 8 = the estimator's blocks as K4-split (hidden dimension cut over 4, 8 or 12 workgroups per 128-row slab, 16-bit partial sums folded
    // by the next reader of x: fold_dwconv_ln / fold_ln); packed rows, from ffn_split_min_rows() rows on
    void set_fused_ffn(int mask) { fused_ffn_ = mask; }
    void set_fused_ffn_min_rows(int64_t k4_rows, int64_t split_rows) {
        sync(); drop_graphs();  // a captured pipeline has the kernel choice baked in
        if (k4_rows >= 0) ffn_min_rows_ = k4_rows;
        if (split_rows >= 0) ffn_split_min_rows_ = split_rows;
    }
    int fused_ffn() const { return fused_ffn_; }
    int64_t last_ve_rows() const { return last_ve_rows_; }
    int64_t last_vo_rows() const { return last_vo_rows_; }  // frames the vocoder computed in the last batch_run  // rows the estimator worked on in the last batch_run
    bool packed_text_ok(int B) const {
        return packed_ve_ && B <= 1024 && dwconv_ln_supports_packed(a_.te_dim, a_.te_kernel) && dwconv_ln_supports_packed(a_.dp_dim, a_.dp_kernel);
    }
    bool packed_rows_ok(int B) const { return packed_ve_ && B <= 1024 && a_.ve_dilated > 0 && dwconv_ln_supports_packed(a_.ve_dim, a_.ve_kernel); }
    long graph_replays() const { return graph_replays_; }
    size_t graphs_cached() const { return graphs_.size(); }
    const Batch& batch() const { return bt_; }
    void batch_fetch(float* wav, size_t wav_capacity, float* duration);
    // waveform as 16-bit PCM (clamp, *32767, truncate: cpp/helper.cpp:986-987) converted on the GPU: half the D2H bytes
    void batch_fetch_pcm16(int16_t* pcm, size_t capacity, float* duration);
    // The same, pipelined: _begin converts into the device slot and starts its device->host copy on a second stream (the next
    // stn_batch_upload / stn_batch_run proceed meanwhile: the copy of batch i overlaps the synthesis of batch i+1); _end waits
    // for that copy and hands out the slot's pinned host buffer (valid until the slot's next _begin).  Two slots.
    bool fetch_slot_dims(int slot, int* B, int64_t* W) const {
        const FetchSlot& f = fetch_[slot];
        if (!f.busy || f.dur.empty()) return false;
        *B = (int)f.dur.size(); *W = (int64_t)(f.n / f.dur.size());
        return true;
    }
    void batch_fetch_pcm16_begin(int slot);
    void batch_fetch_pcm16_end(int slot, const int16_t** pcm, size_t* n, float* duration);
    void batch_fetch_latent(float* latent);  // final denoised latent [B,D,L] (tests)
    // device->device: wav rows [B][W] into dst rows of stride dst_stride floats (>= W), on the engine's stream
    void batch_copy_wav_device(float* dst, int64_t dst_stride);
    // the finished batch as int16 PCM (writeWavFile's conversion) straight into a device buffer, rows dst_stride apart
    void batch_copy_pcm16_device(int16_t* dst, int64_t dst_stride);
    // ---- sample encodings (OutEnc, kernels.hpp): every fetch path above in any encoding, through the one output
    // stage.  The fp32 and PCM16 calls above are the ENC_F32 and ENC_PCM16 cases of these.
    void batch_fetch_encoded(int enc, void* dst, size_t capacity_bytes, float* duration);
    void batch_fetch_encoded_begin(int slot, int enc);
    void batch_fetch_encoded_end(int slot, const void** data, size_t* n_bytes, float* duration);
    void batch_copy_encoded_device(int enc, void* dst, int64_t dst_stride);  // dst_stride in samples
    // rows x W fp32 (host) -> rows x W samples of encoding enc (host, enc_bytes(enc) each): the store kernel without a gain
    void op_encode(int enc, int rows, int W, const float* x, void* y);
    // ---- dither (include/stn.h "dither"): the 16- and 24-bit PCM stores of every fetch path round (DITHER_ROUND) or
    // round behind triangular dither (DITHER_TPDF, DITHER_TPDF_HP) keyed by (seed, utterance id or programme index, sample index).  Off
    // (the default): the truncating store, the kernels that run without the setting.  Handle state that no graph depends on.
    void set_dither(int mode, uint64_t seed);
    int dither_mode() const { return dither_.mode; }
    uint64_t dither_seed() const { return dither_.seed; }
    // ---- pitch (include/stn.h "pitch"): every fetch path delivers the rows shifted by `semitones`: stretched by
    // a / b ~ 2^(s/12) at the model's rate (WSOLA) and resampled by b / a back to their length, in front of every other stage.  0 (the
    // default): off, nothing is launched.  Handle state that no graph depends on.
    void set_pitch(float semitones);  // throws what pitch_check refuses; the previous setting then stays
    float pitch() const { return ps_semi_; }
    int pitch_a() const { return ps_a_; }
    int pitch_b() const { return ps_b_; }
    bool pitch_on() const { return ps_a_ != ps_b_; }
    // rows x W fp32 (host) at hz, row r's span n[r] (host, or null: W), stretched by a / b: y [rows][Ws], delta and score [rows][M]
    // (host, each or null; Ws and M: pitch_plan): the launches of the batch path on the caller's rows
    void op_time_stretch(int hz, int rows, int W, const float* x, const int64_t* n, int a, int b, float* y, int* delta, float* score);
    // the same rows shifted by `semitones` -> y [rows][W] (host): the stretch and the resample behind it
    void op_pitch(int hz, int rows, int W, const float* x, const int64_t* n, float semitones, float* y);
    // ---- pitch mode (include/stn.h "formant"): STN_PITCH_RESAMPLE (the default) delivers the shifted rows as
    // they are; STN_PITCH_FORMANT puts the spectral envelope of the rows before the shift back onto them (kernels_formant.hip) at the
    // end of the pitch stage.  No effect while pitch is off: nothing is launched and no scratch exists.
    void set_pitch_mode(int mode);  // throws for any other value; the previous mode then stays
    int pitch_mode() const { return ps_mode_; }
    // the op-level probe: the tables [rows][frames][p + 1] and the per-frame gain and errors [rows][frames] (host, each or null), on
    // scratch poisoned before the launches, and whether the guard words around x, y and out still hold the poison
    struct FormantProbe {
        float *ax = nullptr, *cy = nullptr;
        double *g = nullptr, *ex = nullptr, *ey = nullptr;
        bool guard_ok = false;  // out
    };
    // x (the rows before the shift) and y (the shifted rows), rows x W fp32 (host) at hz with spans n (host, or null: W) -> out
    // [rows][W] (host): the launches of the batch path on the caller's rows
    void op_formant(int hz, int rows, int W, const float* x, const float* y, const int64_t* n, float* out, FormantProbe* probe = nullptr);
    // op_pitch under a mode: with STN_PITCH_FORMANT, bit for bit op_formant(x, op_pitch(x))
    void op_pitch_ex(int hz, int rows, int W, const float* x, const int64_t* n, float semitones, int mode, float* y);
    // launch_store_rows on the caller's whole buffers: x [rows][W] (host) placed x_misalign floats behind a 16-byte boundary on the
    // device, gain and row_id [rows] (host) or null, y [rows][dst_stride] samples of enc (host; copied in, stored into, copied out)
    void op_encode_ex(int enc, int rows, int W, const float* x, int x_misalign, const float* gain, const int64_t* row_id, int mode, uint64_t seed,
                      int64_t dst_stride, void* y);
    // ---- join (include/stn.h "join"): consecutive rows concatenated with gaps into programmes by the output
    // stage; every fetch path above with a join delivers [G][W_join] instead of [B][W].  A fetch argument: nothing here is handle state.
    JoinPlan batch_join_plan(const stn_join* j);  // the finished batch's plan at the current output rate (throws what the ABI refuses)
    void batch_fetch_joined(const stn_join* j, int enc, void* dst, size_t capacity_bytes, int64_t* prog_len, float* prog_dur);
    void batch_fetch_joined_begin(int slot, const stn_join* j, int enc);  // ended by batch_fetch_encoded_end (durations: prog_dur)
    void batch_copy_joined_device(const stn_join* j, int enc, void* dst, int64_t dst_stride);
    void batch_join_loudness(const stn_join* j, float* lufs, float* peak, float* gain);  // [G] host floats or null
    // rows x W fp32 (host) at hz, row r's first n[r] samples its segment -> y [G][W_join] samples of enc (host); with loudness, every
    // programme measured over its whole length and stored with its own gain
    void op_join(int hz, int rows, int W, const float* x, const int64_t* n, const stn_join* j, int enc, bool loudness_on, float target_lufs,
                 float ceiling_dbfs, void* y, float* prog_lufs, float* prog_peak, float* prog_gain);

    // ---- output rate (engine_resample.cpp): 0 or the model's rate = off (the default; every fetch path is then exactly the
    // native one).  On, every fetch path resamples the finished waveform on the handle's stream before its copy (kernels_resample.hip);
    // the latent geometry, the captured pipeline and the durations stay at the model's rate.
    void set_output_rate(int hz);
    int output_rate() const { return resample_on() ? out_hz_ : a_.sample_rate; }
    bool resample_on() const { return out_hz_ != 0 && out_hz_ != a_.sample_rate; }
    int64_t out_len(int64_t W) const;  // samples per utterance a fetch returns for W native samples
    // rows x W fp32 at in_hz -> rows x ceil(W * P / Q) at out_hz, as fp32 (y) and / or PCM (pcm); host pointers
    void op_resample(int in_hz, int out_hz, int rows, int W, const float* x, float* y, int16_t* pcm);

    // ---- loudness (engine_loudness.cpp): off is the default (every fetch path is then exactly the one without it).  On, every fetch
    // path measures the finished waveform at the output rate (BS.1770-4 integrated loudness of row b's first
    // n_b = min(W_out, (int64_t)(duration_b * (float)rate)) samples, kernels_loudness.hip) and scales row b by
    // g_b = min(10^((target - L_b) / 20), 10^(ceiling / 20) / peak_b) before its conversion and copy; the gain stays on the device.
    void set_loudness(bool on, float target_lufs, float ceiling_dbfs);
    bool loudness_on() const { return lo_on_; }
    void get_loudness(int* on, float* target_lufs, float* ceiling_dbfs) const;
    // the finished batch at the output rate: L_b, peak_b and the gain the current setting applies (1 when off); [B] host floats or null
    void batch_loudness(float* lufs, float* peak, float* gain);
    // rows x W fp32 (host) at hz, row r's first n[r] samples (all W when n is null) -> L, peak [rows] (host)
    void op_loudness(int hz, int rows, int W, const float* x, const int64_t* n, float* lufs, float* peak);
    // The same measurement with its scratch laid open (the kernel tests): the scratch is filled with the quiet NaN 0x7FC00000 first, x is
    // uploaded 4 bytes off 16-byte alignment when x_misalign is set, and the whole per-chunk buffers come back (host, Ks = lo_chunks(W)):
    // st_end [rows][Ks][4] as the first launch left it, st_start the same after the scan, pk / pa / pb [rows][Ks]; any may be null.
    struct LoProbe {
        int x_misalign = 0;
        float *st_end = nullptr, *st_start = nullptr, *pk = nullptr, *pa = nullptr, *pb = nullptr;
        const char* form = "";  // out: the staging path that ran
    };
    void op_loudness_ex(int hz, int rows, int W, const float* x, const int64_t* n, bool on, float target, float ceiling, LoProbe& probe,
                        float* lufs, float* peak, float* gain);
    // ---- loudness report (engine_loudness.cpp; include/stn.h "loudness range"): maximum momentary loudness,
    // maximum short-term loudness, loudness range and the number of 3 s windows behind its gates, of the rows and spans the calls above
    // measure.  One more launch behind the measurement's, on its scratch; a report only: no fetch launches it.  [rows] host values or null.
    void batch_loudness_range(float* m_max, float* s_max, float* lra, int32_t* n_st);
    void batch_join_loudness_range(const stn_join* j, float* m_max, float* s_max, float* lra, int32_t* n_st);  // [G]
    void op_loudness_range(int hz, int rows, int W, const float* x, const int64_t* n, float* m_max, float* s_max, float* lra, int32_t* n_st);
    // ---- pitch report (engine_f0.cpp; include/stn.h "f0"): the YIN track of the rows and spans batch_loudness
    // measures and its per-row statistics.  Two launches (kernels_f0.hip) on out_source's rows; a report only: no fetch launches them.
    // f0, ap: [rows][cap] host floats, stats [rows]; any may be null.  p null: the defaults.
    int64_t batch_f0_frames(const stn_f0_params* p);  // the most frames a row of the finished batch holds
    void batch_f0(const stn_f0_params* p, int64_t cap, float* f0, float* ap, stn_f0_stats* stats);
    void op_f0(int hz, int rows, int W, const float* x, const int64_t* n, const stn_f0_params* p, int64_t cap, float* f0, float* ap, stn_f0_stats* stats);

    // ---- silence trimming (engine_edges.cpp; include/stn.h "silence trimming"): off is the default (every fetch
    // path is then exactly the one without it).  On, every fetch path finds row b's edges [start_b, end_b) by level at the output rate
    // (kernels_edges.hip) and delivers that segment from column 0, cut edges faded; a joined fetch joins those segments.
    void set_silence_trim(bool on, float top_db, float keep_ms, float fade_ms);
    bool silence_trim_on() const { return st_on_; }
    void get_silence_trim(int* on, float* top_db, float* keep_ms, float* fade_ms) const;
    // the finished batch's edges at the output rate under the current parameters, on or off; [B] host integers or null
    void batch_silence_edges(int64_t* start, int64_t* end);
    // rows x W fp32 (host) at hz, row r's first n[r] samples (all W when n is null) -> start, end [rows] (host)
    void op_silence_edges(int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, int64_t* start, int64_t* end);
    // the same, and y [rows][W] samples of enc (host): row r's segment from column 0 (times gain[r] when gain is not null, cut edges
    // faded), zero codewords behind it
    void op_silence_trim(int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, float fade_ms, const float* gain,
                         int enc, void* y, int64_t* start, int64_t* end);
    // ---- pause limit (engine_edges.cpp; include/stn.h "pause limit"): off is the default, and without silence
    // trimming it has no effect (every fetch path is then exactly the one without it).  On with trimming on, the detection is followed by
    // one launch (pause_rows_kernel) that cuts every pause inside a row's [start, end) longer than max_pause_ms down to it; the trimmed
    // store and the join then run on the row's several segments.
    void set_pause_limit(bool on, float max_pause_ms);
    bool pause_limit_active() const { return pl_on_ && st_on_; }
    void get_pause_limit(int* on, float* max_pause_ms) const;
    // the finished batch as the current parameters cut it (limit and trimming on or off): len [B], n_cuts [B], cuts [B][cap_pairs][2]
    // (lo, hi; the first min(n_cuts, cap_pairs) pairs of a row); host arrays or null
    void batch_pauses(int64_t* len, int32_t* n_cuts, int64_t* cuts, int cap_pairs);
    // op_silence_trim with the pause limit: y rows hold the row's segments end to end from column 0
    void op_pause_trim(int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, float fade_ms, float max_pause_ms,
                       const float* gain, int enc, void* y, int64_t* start, int64_t* end, int64_t* len, int32_t* n_cuts, int64_t* cuts, int cap_pairs);
    // The same detection (ed_enqueue itself: the frame pass, the row pass and, with max_pause_ms > 0, the pause pass) with its scratch
    // laid open (the kernel tests): every 32-bit word of the scratch is 0x7FC00000 before the first launch (a NaN as a float; two of
    // them as a double are 2^1021 * 1.0000005), x is uploaded 4 bytes off 16-byte alignment when x_misalign is set, and the per-chunk
    // shares and the frame levels come back whole (host): pa / pb [rows][ed_chunks(W)], lev [rows][edges_frames(W, hz)]; any may be
    // null.  max_pause_ms = 0: no pause pass, len = end - start and n_cuts = 0.
    struct EdProbe {
        int x_misalign = 0;
        float *pa = nullptr, *pb = nullptr;
        double* lev = nullptr;
        const char* form = "";  // out: the staging path that ran
    };
    void op_silence_edges_ex(int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, float fade_ms, float max_pause_ms,
                             EdProbe& probe, int64_t* start, int64_t* end, int64_t* len, int32_t* n_cuts, int64_t* cuts, int cap_pairs);
    // diagnostic: overwrite the finished batch's model-rate waveform ([B][L * chunk] host floats) and forget what was measured on it
    void dbg_batch_set_wav(const float* wav);
    // diagnostic: uploads of the batch span table (batch_spans) since the engine was created
    int64_t span_uploads() const { return sp_uploads_; }

    // ---- limiter (engine_limiter.cpp; include/stn.h "limiter"): off is the default, and without loudness it
    // has no effect (every fetch path is then exactly the one without it).  On with loudness on, the loudness gain is the uncapped
    // 10^((target - L_b) / 20) and the ceiling is enforced by a look-ahead peak limiter (kernels_limiter.hip) that writes the limited
    // fp32 rows into fetch scratch; the store and join kernels then run on those rows without a gain.
    void set_limiter(bool on, float lookahead_ms);
    bool limiter_active() const { return lm_on_ && lo_on_; }
    void get_limiter(int* on, float* lookahead_ms) const;
    // the finished batch as a fetch limits it: per row the deepest reduction in dB and the samples whose curve is below 1 (both 0
    // while the limiter is not active); [B] host arrays or null
    void batch_limiter(float* reduction_db, int64_t* limited);
    // rows x W fp32 (host) at hz, row r's first n[r] samples (all W when n is null) times gain[r] (1 when null) -> y, s [rows][W]
    // (host; s may be null), reduction_db, limited [rows] (host, or null)
    void op_limiter(int hz, int rows, int W, const float* x, const int64_t* n, const float* gain, float ceiling_dbfs, float lookahead_ms, float* y,
                    float* s, float* reduction_db, int64_t* limited);
    // the same under a peak mode: STN_PEAK_TRUE drives the curve by the true-peak envelope of x * gain (env [rows][W], host or null) and
    // reports trim [rows] = min(1, c / true peak of y) (host or null; 1 in sample mode); y is the limited row before the trim
    void op_limiter_ex(int hz, int rows, int W, const float* x, const int64_t* n, const float* gain, float ceiling_dbfs, float lookahead_ms, float* y,
                       float* s, float* reduction_db, int64_t* limited, int peak_mode, float* env, float* trim);

    // ---- true peak (engine_truepeak.cpp; include/stn.h "true peak"): STN_PEAK_SAMPLE is the default (every
    // fetch path is then exactly the one without it).  STN_PEAK_TRUE with loudness on: the ceiling is a true-peak ceiling (4x
    // oversampled, kernels_truepeak.hip): the gate's peak is the row's true peak, and the limiter's curve follows the true-peak envelope
    // and is followed by one trim per row.  Without loudness the setting has no effect.
    void set_peak_mode(int mode);
    int peak_mode() const { return pk_true_ ? 1 : 0; }
    // the finished batch at the output rate: the true peak of the measured row, of the fp32 row as delivered under the current settings,
    // and the limiter's trim (1 except with the limiter in true mode); [B] host floats or null
    void batch_true_peak(float* tp_in, float* tp_out, float* trim);
    // rows x W fp32 (host), row r's first n[r] samples (all W when n is null) times gain[r] (1 when null) -> tp [rows], env [rows][W],
    // pk [rows][lo_chunks(W)] (host, or null); the scratch is filled with the quiet NaN 0x7FC00000 first; returns the staging form
    const char* op_true_peak(int hz, int rows, int W, const float* x, const int64_t* n, const float* gain, int x_misalign, float* tp, float* env,
                             float* pk);

    // ---- filter chain (engine_filter.cpp; include/stn.h "filter chain"): empty is the default (every fetch path is
    // then exactly the one without it).  Set, out_source() delivers the rows at the output rate filtered in the fetch scratch
    // (kernels_filter.hip), and everything behind it (edges, pauses, loudness, limiter, true peak, stores, joins) runs on those.
    void set_filters(int n, const stn_filter* f);
    bool filter_on() const { return !fl_set_.empty(); }
    const std::vector<stn_filter>& filters() const { return fl_set_; }
    // the op-level probe: st_end / st_start [P][rows][Ks][4] (host, or null), the poisoned guards around x and y, the staging form
    struct FlProbe {
        int x_misalign = 0;
        float *st_end = nullptr, *st_start = nullptr;
        bool guard_ok = false;   // out
        const char* form = "";   // out
    };
    // rows x W fp32 (host) at hz through f[0 .. n) -> y (host)
    void op_filter(int hz, int rows, int W, const float* x, int n, const stn_filter* f, float* y, FlProbe* probe);

    // ---- compressor (engine_compressor.cpp; include/stn.h "compressor"): off is the default (every fetch path is
    // then exactly the one without it).  On, out_source() delivers the rows at the output rate compressed in place in the fetch scratch,
    // behind the filter chain (kernels_dynamics.hip), and everything behind it runs on those.
    void set_compressor(bool on, const stn_compressor* c);
    bool compressor_on() const { return cp_.on; }
    const stn_compressor& compressor() const { return cp_.set; }
    void batch_compressor(float* max_reduction_db);
    // what the op-level probes of the three dynamics stages share: the four state arrays [rows][Ks] (host, or null), the poisoned
    // guards, the staging form
    struct DynProbe {
        int x_misalign = 0, in_place = 0;  // in_place: y is written over x on the device
        float *s1_end = nullptr, *s1_start = nullptr, *s2_end = nullptr, *s2_start = nullptr;
        bool guard_ok = false;   // out
        const char* form = "";   // out
    };
    // the op-level probe: gr [rows][W] (host, or null)
    struct CpProbe : DynProbe { float* gr = nullptr; };
    // rows x W fp32 (host) at hz through the compressor c -> y (host)
    void op_compressor(int hz, int rows, int W, const float* x, const stn_compressor& c, float* y, CpProbe* probe);

    // ---- de-esser (engine_deesser.cpp; include/stn.h "de-esser"): off is the default (every fetch path is then
    // exactly the one without it).  On, out_source() delivers the rows at the output rate de-essed in place in the fetch scratch, behind
    // the filter chain and in front of the compressor (kernels_dynamics.hip), and everything behind it runs on those.
    void set_deesser(bool on, const stn_deesser* c);
    bool deesser_on() const { return ds_.on; }
    const stn_deesser& deesser() const { return ds_.set; }
    void batch_deesser(float* max_reduction_db);
    // the op-level probe: band and gr [rows][W] and the band's states [rows][Ks][4] (host, or null)
    struct DsProbe : DynProbe { float *band = nullptr, *gr = nullptr, *st_end = nullptr, *st_start = nullptr; };
    // rows x W fp32 (host) at hz through the de-esser c -> y (host)
    void op_deesser(int hz, int rows, int W, const float* x, const stn_deesser& c, float* y, DsProbe* probe);

    // ---- expander (engine_expander.cpp; include/stn.h "expander"): off is the default (every fetch path is then
    // exactly the one without it).  On, out_source() delivers the rows at the output rate expanded in place in the fetch scratch, behind
    // the filter chain and in front of the de-esser (kernels_dynamics.hip), and everything behind it runs on those.
    void set_expander(bool on, const stn_expander* c);
    bool expander_on() const { return xp_.on; }
    const stn_expander& expander() const { return xp_.set; }
    void batch_expander(float* min_attenuation_db, int64_t* closed_samples);
    // the op-level probe: open [rows][W] (host, or null)
    struct XpProbe : DynProbe { float* open = nullptr; };
    // rows x W fp32 (host) at hz through the expander c -> y (host)
    void op_expander(int hz, int rows, int W, const float* x, const stn_expander& c, float* y, XpProbe* probe);

    // ---- profiling (hipEvent pairs around launches of one kernel family, on this stream) ----------------
    void profile_enable(bool on) { if (on != prof_on_) profile_reset(); prof_on_ = on; }
    void launch_log_enable(bool on);   // record (family, kernel) of every launch while profiling is on (this thread's engine calls)
    std::string launch_log() const;    // "family\tkernel\n" per launch since the last profile_reset, dispatch order
    void profile_sample(int every) { prof_every_ = every < 1 ? 1 : every; prof_seen_ = 0; }  // time every n-th matching launch only
    void profile_filter(const std::string& family) { if (family != prof_filter_) profile_reset(); prof_filter_ = family; }  // "" = every family
    void profile_reset();
    std::vector<std::pair<std::string, KernelStat>> profile_collect();

    // ---- op-level test entry points (host pointers) ------------------------------------------------------
    void op_gemm(int dtype, int M, int N, int K, const float* A, const float* W, const float* bias, int act, float* out);
    // one GEMM with the epilogue fields the engine uses (stn_op_gemm_ex): out [out_elems] fp32 is the whole destination buffer (EPI_RESID:
    // the residual), uploaded as given (rounded to out_dtype first when that is 16-bit) and downloaded whole (widened back to fp32).
    // len [nseq], row_b [M], rowvec [nseq][N].  tr >= 0 forces the tiled kernels' 16-bit store form.  Returns the form it ran (GemmForm::str).
    std::string op_gemm_ex(int dtype, int M, int N, int K, const float* A, const float* W, int mode, int act, int out_dtype, int ldo,
                           const float* bias, const float* gamma, const int* len, int L, const int* row_b, const float* rowvec, int nseq,
                           int nt, int tr, float* out, int64_t out_elems);
    // one attention through launch_attention in the engine's layouts (stn_op_attention_ex): q [q_elems / ldq rows][ldq] with the heads from
    // column q_col, K and V in the rows of kv [kv_elems / ldk][ldk] from columns k_col and v_col, o [o_elems / ldo][ldo] from column 0.
    // kv and o are the caller's whole buffers: uploaded as given (rounded to dtype) and downloaded whole (widened to fp32).  k_rotated: the
    // keys are rotated first by launch_rope_rows over rot_groups groups rot_stride apart from column rot_col, the estimator's text-key pass.
    // Returns the form it ran (AttnForm::str).
    std::string op_attention_ex(int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, int64_t q_elems, int ldq, int q_col,
                                float* kv, int64_t kv_elems, int ldk, int k_col, int v_col, float* o, int64_t o_elems, int ldo,
                                const int* qlen, const int* klen, const int* q_off, const int* k_off, int rope_mode, int k_rotated,
                                int rot_groups, int rot_stride, int rot_col);
    // one head-split launch (stn_op_xattn_hs): xn [M][384]; Wq, Wo [384][384] plain, repacked here as prepare_xattn_weights does; K at
    // column k_col of kv's rows, V at k_col + 384; packed query rows from launch_row_map(qlen).  part [part_elems] is the caller's whole
    // buffer (rounded to dtype going up, widened coming back); pairs_mode 1: launch_xattn_hs_pairs' table, written to pairs_out
    // (2 * ceil(B / 2) ints).  Returns the form it ran (XattnHsForm::str).
    std::string op_xattn_hs(int dtype, int M, const float* xn, const float* Wq, const float* bq, const float* Wo, const float* kv,
                            int64_t kv_elems, int ldk, int k_col, int B, int L, int Lk, const int* qlen, const int* klen, const int* k_off,
                            int rope_mode, int pairs_mode, int64_t part_stride, float* part, int64_t part_elems, int* pairs_out);
    void op_attention(int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, const float* k, const float* v,
                      const int* qlen, const int* klen, int rope_mode, float* o);
    // one EPI_STORE GEMM, fp32 out, whose M rows are packed per sequence (sequence b owns rows[b] consecutive rows; rows past their sum are dead)
    // and stored through the packed-row destination map into out [B][T][N]: row t of sequence b only for t < valid[b] (stn_op_gemm_rows).  out
    // [out_elems] is the whole destination, uploaded as given and downloaded whole.  Returns the form; throws where it has no slab epilogue.
    std::string op_gemm_rows(int dtype, int M, int N, int K, const float* A, const float* W, const float* bias, int B, const int* rows,
                             const int* valid, int T, float* out, int64_t out_elems);
    void op_dwconv_ln(int dtype, int B, int L, int C, int k, int dil, const float* x, const float* w, const float* bias,
                      const float* g, const float* b, float* y, const int* seqlen = nullptr /* host [B] */);
    // launch_dwconv_ln (or, ln_only, launch_layernorm over B*L rows) on the caller's whole buffers (stn_op_dwconv_ln_ex): x [x_rows][C] uploaded as
    // given, padding rows included; packed: sequence b owns seqlen[b] consecutive rows of x / y (row_off from launch_row_map); y [y_rows][C]
    // uploaded as given (rounded to dtype) and downloaded whole.  Returns the form it ran (DwconvLnForm::str, or "layernorm").
    // tail (optional, host [rf + 1][C]; packed rows): the tail-reading variant, rows of T >= L frames (stn_op_dwconv_ln_tail)
    std::string op_dwconv_ln_ex(int dtype, int B, int L, int C, int k, int dil, const float* x, int64_t x_rows, const float* w, const float* bias,
                                const float* g, const float* b, const int* seqlen, int packed, int ln_only, float* y, int64_t y_rows,
                                const float* tail = nullptr, int T = 0, int rf = 0);
    // launch_fold_ln on host operands (stn_op_fold_ln): part [S][M][C] rounded to dtype (BF16 / F16), x [M][C] updated in place, y [M][C]
    void op_fold_ln(int dtype, int M, int C, int S, const float* part, const float* b2, const float* gamma, const float* rowvec, const int* row_b,
                    int nseq, const float* g, const float* b, float* x, float* y);
    // one layout kernel of kernels_layout.hip on host operands (stn_op_layout; `which` and the parameter lists are documented there)
    void op_layout(int which, int dtype, const int* p, const float* a, int64_t a_n, const float* b, int64_t b_n, const float* c, int64_t c_n,
                   const int64_t* ids, int64_t ids_n, const int* len, int packed, float* out, int64_t out_n, float* out2, int64_t out2_n, int* iout,
                   int64_t iout_n);
    // device-resident timing of one GEMM shape (random operands), HIP events around `iters` launches: avg ms
    double op_gemm_bench(int dtype, int M, int N, int K, int mode, int iters);
    // per-workgroup phase stamps of one launch of the tiled kernel: out[0..2] = mean cycles of (first stage landed, K loop,
    // epilogue), out[3] = max over workgroups of (end - earliest entry), out[4] = spread of entry times, out[5] = workgroups
    void op_gemm_phases(int dtype, int M, int N, int K, int mode, double* out6);
    void op_randn(uint64_t seed, int B, int D, int L, const int64_t* utt_ids, const int* len, float* out);
    // K4 on host operands: x <- x + gamma * (W2 . GELU(W1 . xn + b1) + b2) [+ rowvec[row_b[m]]]; xn is rounded to the engine's
    // 16-bit format first.  fused = false runs the two tiled GEMM launches on the same operands (the pair K4 replaces).
    // mode: 0 = two tiled launches, 1 = K4, 2 = K4-split (partial sums) + fold_ln
    void op_ffn(int M, int C, int I, const float* xn, const float* W1, const float* b1, const float* W2, const float* b2, const float* gamma,
                const float* rowvec /* [nseq][C] or null */, const int* row_b /* host [M] or null */, int nseq, float* x, int mode);
    // the pointwise pair through ffn_launch on the caller's whole buffers (stn_op_ffn_ex; 16-bit engines): xn [xn_elems] rows of ldx, rounded to the
    // engine's format; x [x_elems] rows of ldo, uploaded as given and downloaded whole; len [nseq] with L, row_b [M], rowvec [nseq][rv_ld] as
    // FfnArgs.  mode 0 / 1 / 2 as op_ffn, split != 0 forces that S.  Mode 2 stops at the partial sums: part [part_elems] (shares part_stride
    // apart) is uploaded as given (rounded) and downloaded whole, no fold runs and x is left alone.  Returns the form it ran (FfnForm::str).
    std::string op_ffn_ex(int M, int C, int I, const float* xn, int ldx, int64_t xn_elems, const float* W1, const float* b1, const float* W2,
                          const float* b2, const float* gamma, const int* len, int L, const int* row_b, const float* rowvec, int rv_ld, int nseq,
                          int mode, int split, float* x, int ldo, int64_t x_elems, float* part, int64_t part_stride, int64_t part_elems);
    // fold_dwconv_ln on host operands (packed rows: sequence b owns seqlen[b] consecutive rows; M = sum): part [S][M][C] fp32 is rounded
    // to the engine's 16-bit format first.  x_out <- folded x, y <- LayerNorm(dwconv(folded x)) as fp32.
    void op_fold_dwconv_ln(int B, int C, int k, int dil, int S, const int* seqlen, const float* x, const float* part, const float* b2,
                           const float* gamma, const float* rowvec /* [B][C] or null */, const float* w /*[C][k]*/, const float* bias,
                           const float* g, const float* b, float* x_out, float* y);
    // launch_fold_dwconv_ln, once, on the caller's whole buffers (stn_op_fold_dwconv_ln_ex): dtype BF16 / F16 whatever the engine's; L >= every length;
    // row_off from launch_row_map; part [part_elems] rounded to dtype, splits part_stride apart; rowvec [B][rv_ld]; x_in [x_rows][C]; x_out
    // [x_out_rows][C] and y [y_rows][C] uploaded as given (y rounded) and downloaded whole.  Returns the form it ran (FoldDwconvLnForm::str).
    std::string op_fold_dwconv_ln_ex(int dtype, int B, int L, int C, int k, int dil, int S, int run_frames, const int* seqlen, const float* x_in,
                                     int64_t x_rows, const float* part, int64_t part_stride, int64_t part_elems, const float* b2, const float* gamma,
                                     const float* rowvec, int rv_ld, const float* w, const float* bias, const float* g, const float* b, float* x_out,
                                     int64_t x_out_rows, float* y, int64_t y_rows);
    // device-resident timing of the block's pointwise pair on random operands: out[0] = avg ms per call (fused: one launch,
    // unfused: pw1 + pw2); fused only: out[1..3] = mean cycles per workgroup to the first stage / in the tile loop / in the
    // epilogue, out[4] = workgroups
    void op_ffn_bench(int M, int C, int I, int mode, int iters, double* out5);
    // device-resident timing of one estimator-style block chain on packed rows of B equal sequences of L frames:
    // mode 0: dwconv_ln + pw1 + pw2;  mode 2: fold_dwconv_ln + K4-split.  out[0] = avg ms per block, out[1] = avg ms of the conv kernel alone, out[2..5] = fold_dwconv_ln phase cycles (mode 2)
    void op_block_bench(int B, int L, int C, int I, int k, int dil, int mode, int iters, double* out6);

    Arena& arena() { return ar_; }

   private:
    // weights
    DevTensor& tensor(const std::string& name);
    const float* vecf(const std::string& name) { return tensor(name).f32; }
    Linear linear(const std::string& prefix);
    LNorm lnorm(const std::string& prefix);
    ConvNeXt convnext_w(const std::string& prefix);
    Attn attn_w(const std::string& prefix, bool self);
    void free_weights();
    using RawSource = std::function<std::vector<float>(const std::string& name, int kind, int rows, int cols, float gain)>;
    void load_weights(const stn_arch& a, const RawSource& src, std::vector<std::string>* names_only);

    // building blocks (enqueue on s_)
    size_t act_bytes(int64_t n) const { return (size_t)n * (is_half(dt_) ? 2 : 4); }
    void* act_alloc(int64_t n) { return ar_.alloc(act_bytes(n)); }
    float* f32_alloc(int64_t n) { return static_cast<float*>(ar_.alloc((size_t)n * 4)); }
    void gemm(const char* tag, int dt, const void* A, int lda, const Linear& w, int M, Epilogue e);
    // rowvec (optional, [B][rv_ld]): added to every row of sequence b in the same residual epilogue (time conditioning)
    // The residual stream of a stage whose blocks may run as K4-split: x plus at most one pending (unfolded) update.
    struct FoldState {
        float* x = nullptr;      // current residual rows
        float* x_alt = nullptr;  // second buffer: fold_dwconv_ln writes the folded stream there and the two swap
        void* part = nullptr;    // [S][rows padded to 128][C] 16-bit partial sums (one buffer: its reader runs before the next writer)
        int64_t part_stride = 0;
        bool pending = false;
        FoldArgs fold;           // the pending update
    };
    // the form of a stage's pointwise pairs (ffn_form with this engine's settings): every block of a stage has the same C, I, k and rows
    FfnForm ffn_plan(int stage, int C, int I, int64_t M, int64_t gate_rows, bool packed, int k, int max_dil) const {
        return ffn_form(dt_, stage, C, I, M, gate_rows, packed, k, max_dil, fused_ffn_, ffn_min_rows_, ffn_split_min_rows_, nt_hints_);
    }
    // the pointwise pair in form f.  a: its operands (a.wseq the stream packed for f; a.part / a.part_stride a K4-split's partial-sum buffer);
    // w1 / w2: the plain matrices (two GEMMs).  K4-split leaves x alone and returns the pending update, for the next reader of x to fold.
    FoldArgs ffn_launch(const FfnForm& f, int C, const FfnArgs& a, const Linear& w1, const Linear& w2);
    static FoldArgs ffn_pending(const FfnForm& f, const FfnArgs& a) {  // the update a K4-split launch leaves pending
        return FoldArgs{a.part, f.split, a.part_stride, a.b2, a.gamma, a.rowvec, a.rv_ld, a.row_b};
    }
    // the FFN op entry points' set-up: the form `mode` forces (0 two GEMMs, 1 K4, 2 K4-split with ffn_split_choose's S, or with `split` where that is not 0), W1 [I][C] / W2 [C][I]
    // (fp32, device) in the 16-bit format, and the launch's shape, packed weight stream and partial-sum buffer in `a` (operands left to fill)
    struct FfnOp { FfnForm f; Linear w1, w2; FfnArgs a; };
    FfnOp op_ffn_setup(const char* op, int mode, int M, int C, int I, const float* W1, const float* W2, int split = 0);
    // fs: x is fs->x, and a K4-split block leaves its pointwise pair pending in fs (the caller folds it with the next reader of x)
    void convnext(const ConvNeXt& p, const FfnForm& f, float* x, int B, int L, int C, int hid, int k, int dil, const int* len,
                  const int* conv_len = nullptr, const float* rowvec = nullptr, int rv_ld = 0, const Ragged* rg = nullptr, FoldState* fs = nullptr,
                  const DwconvTail& tl = DwconvTail() /* packed rows: what the conv's taps beyond a sequence's rows read (the vocoder's tail form) */);
    // LayerNorm of the stage's residual stream into xn, folding a pending update first
    void fold_layernorm(FoldState& fs, int64_t M, int C, const LNorm& ln, void* xn, const char* tag);
    void attn_block(const Attn& p, float* x, int B, int Lq, int C, int H, const void* ctx, int Lk, const int* qlen,
                    const int* klen, int rope_mode, bool self, const Ragged* qrg = nullptr);
    void* to_act(const float* src, int64_t n);

    struct ProfSpan { std::string tag; hipEvent_t a, b; double flops, bytes; };
    void prof_begin(const char* tag, double flops, double bytes);
    void prof_end();
    // A launch of the output stage in its bracket: stage_ names the stage and, while profiling, a span `tag` is open, from here to the end
    // of the scope, however it is left (launchers throw).  next(): the span ends and another begins under the same stage.
    class StageSpan {
       public:
        StageSpan(Engine& e, const char* stage, const char* tag, double flops, double bytes) : e_(e), prev_(e.stage_) {
            e_.stage_ = stage;
            begin(tag, flops, bytes);
        }
        ~StageSpan() { end(); e_.stage_ = prev_; }
        StageSpan(const StageSpan&) = delete;
        StageSpan& operator=(const StageSpan&) = delete;
        void next(const char* tag, double flops, double bytes) { end(); begin(tag, flops, bytes); }

       private:
        void begin(const char* tag, double flops, double bytes) { if ((begun_ = e_.prof_on_)) e_.prof_begin(tag, flops, bytes); }
        void end() { if (begun_) e_.prof_end(); begun_ = false; }
        Engine& e_;
        const char* prev_;
        bool begun_ = false;
    };

    int device_, dt_;
    int n_cu_ = 256;  // compute units of the device (launch shapes that depend on rounds of workgroups)
    hipStream_t s_ = nullptr, own_s_ = nullptr;
    const char* stage_ = "";
    std::string prof_filter_;
    std::string log_family_;
    int prof_every_ = 1;
    uint64_t prof_seen_ = 0;
    bool prof_active_ = false;
    stn_arch a_{};
    bool loaded_ = false;
    int64_t params_ = 0;
    std::unordered_map<std::string, DevTensor> w_;
    std::vector<void*> owned_;
    Arena ar_;
    Batch bt_;
    std::vector<void*> batch_owned_;    // every live batch buffer (freed with the engine)
    std::vector<void*> batch_retired_;  // outgrown buffers: freed at the next upload, after the stream has drained
    template <typename T> void ensure(T*& p, size_t& cap, size_t need);
    std::vector<float> reported_dur_;
    uint64_t drains_ = 0;  // bumped by every sync(): a host array whose upload was enqueued under another count is no longer read
    // ---- the finished batch's row spans (engine_loudness.cpp; DESIGN.md sections 11 and 11a).  out_spans is the rule: row b's valid
    // samples at hz inside [0, W].  batch_spans is where they live: the device pair every stage of a fetch takes (n: the spans, full: W
    // for every row) and the host copy (the spans first, W for every row behind them), uploaded once per finished batch and (hz, W)
    std::vector<int64_t> out_spans(int64_t W, int hz) const;
    struct BatchSpans {
        RowSpans dev;
        std::vector<int64_t> host;
        uint64_t seq = 0, drains = ~0ull; int hz = 0; int64_t W = 0;  // the finished batch and (hz, W) it holds; drains_ at its upload
    };
    const BatchSpans& batch_spans(int hz, int64_t W);
    BatchSpans sp_[2];     // at the model's rate and row length (what pitch reads, and everything else while no rate is set); at any other rate
    DevBuf sp_buf_;
    int64_t sp_uploads_ = 0;
    // the host copy of an op entry's spans (OpScope::spans), read by their upload until the entry's closing sync()
    friend class OpScope;
    std::vector<int64_t> op_sp_;
    void enqueue_after_duration(int total_step, const std::function<void()>& take_text_rows);
    // A captured graph holds raw pointers: everything it can have baked in is part of its key — the batch buffers (`gen`, bumped
    // by every reallocation), the weights (`wgen`, bumped by every load), the pinned staging the copy nodes read, the stream.
    struct GraphKey {
        int B = 0, Lt = 0, L = 0, steps = 0; bool noise = false, ragged = false; int xattn = 0; int ffn = 0; int rows = 0, vrows = 0, trows = 0; int vform = 0;
        uint64_t gen = 0, wgen = 0; const void* p0 = nullptr; const void* p1 = nullptr; const void* pin = nullptr; hipStream_t s = nullptr;
        bool operator==(const GraphKey& o) const {
            return B == o.B && Lt == o.Lt && L == o.L && steps == o.steps && noise == o.noise && ragged == o.ragged && xattn == o.xattn && ffn == o.ffn &&
                   rows == o.rows && vrows == o.vrows && vform == o.vform && trows == o.trows && gen == o.gen && wgen == o.wgen && p0 == o.p0 && p1 == o.p1 && pin == o.pin && s == o.s;
        }
    };
    // LRU cache of captured graphs (the reference's call() loop and the n_test loop alternate a few shapes,
    // /root/reference/cpp/helper.cpp:697-719, cpp/example_onnx.cpp:88): a shape is captured the second time it is seen
    // (`warm_keys_`: the arena must have seen its allocation sequence once) and replayed from then on.
    // (graph / exec: the pipeline up to the first text cross-attention; graph2 / exec2: the rest — the text encoder's rows are taken between the two)
    struct GraphEntry { GraphKey key; hipGraph_t graph = nullptr, graph2 = nullptr; hipGraphExec_t exec = nullptr, exec2 = nullptr; uint64_t last_use = 0; };
    static constexpr size_t kGraphCache = 8, kWarmKeys = 16;
    std::vector<GraphEntry> graphs_;
    std::vector<GraphKey> warm_keys_;
    uint64_t graph_clock_ = 0, wgen_ = 0;
    void drop_graphs();  // destroy every cached graph (weights or staging they point at are going away)
    bool graph_on_ = true;
    bool vo_ragged_ = false;
    bool packed_ve_ = true;
    bool nt_hints_ = true;
    // The duration predictor of stn_batch_run depends on the uploaded inputs only (not on the previous batch, not on the text
    // encoder): it runs on its own stream with its own workspace, beside the text encoder of the same batch and, in back-to-back
    // runs, beside the tail of the previous one.  Everything that overwrites its inputs goes through sync(), which waits for both.
    hipStream_t dp_s_ = nullptr, te_s_ = nullptr;
    Arena dp_ar_, te_ar_;
    // The text encoder depends on the uploaded inputs only as well: it runs on the same side stream (after the predictor) into
    // text_side; the main stream waits for ev_te_, copies the rows into text_rows (what the graphs read) and records ev_copied_,
    // which the side stream waits for before the NEXT run's encoder overwrites text_side (prefetch depth: one run).
    hipEvent_t ev_te_ = nullptr, ev_copied_ = nullptr, ev_dp_ = nullptr;
    std::function<void()> text_gate_;  // armed by enqueue_after_duration, fired once by the first text cross-attention of the run
    bool copied_valid_ = false;
    int64_t ffn_min_rows_ = 18432;  // K4 only from this many rows on (144 workgroups); STN_FFN_MIN_ROWS overrides
    int64_t ffn_split_min_rows_ = 1;     // K4-split from this many rows on (with the slab staged through LDS one utterance gains too: 20.0 vs 21.4 us per block); STN_FFN_SPLIT_MIN_ROWS overrides
    int fused_ffn_ = 9;         // K4 stages (set_fused_ffn): adopted where measured faster; STN_FFN=<mask> overrides
    bool shape_buckets_ = false;
    bool dur_read_always_ = false;  // measurement: read the predicted durations back (and wait for them) even when the caller overrides them
    int gelu_act_ = ACT_GELU;
    int fused_xattn_ = 1;  // cross-attention blocks of the estimator: head-split (fold_ln + one launch, kernels_xattn_hs.hip; the default) or, 0, four
                           // launches; STN_XATTN=<0|1> overrides
    int64_t last_ve_rows_ = 0, last_vo_rows_ = 0;
    // zero-latent response of the vocoder (device, owned), 16-bit engines: one set per form of the blocks' pointwise pair a batch can take
    // (index: FfnForm::kind == FFN_K4), because the cached rows must carry the bits the batch's own kernels give
    struct VoConsts {
        float* quiet = nullptr;  // [base_chunk_size]
        float* edge = nullptr;   // [rf][base_chunk_size]
        float* tail = nullptr;   // [vo_blocks][rf + 1][vo_dim]: the residual stream at the input of block l, by distance to the end of the row
    };
    VoConsts vo_c_[2];
    int vo_rf_ = 0;
    int vo_force_ffn_ = -1;          // prepare_vocoder_constants: the pointwise form vocoder_dev takes whatever the row count (-1: ffn_plan decides)
    float* vo_capture_ = nullptr;    // prepare_vocoder_constants: where vocoder_dev copies the last rf + 1 rows of every block's input
    void free_vocoder_constants();
    enum VoForm : int { VO_DENSE = 0, VO_TRIM_2RF = 1, VO_TRIM_TAIL = 2 };
    int trimmed_rows(int B, int L, std::vector<int>* n_host) const;  // sum of the trimmed extents (0: trimming not applicable)
    // the tail form, for the batches trimmed_rows leaves dense: every utterance on min(len*ccf + rf, T) frames, all of them exact, the blocks'
    // conv taps beyond them read from VoConsts::tail.  Sum of the extents, 0 where the form does not apply or removes too little.
    int tail_rows(int B, int L) const;
    int vocoder_rows(int B, int L, int* form) const;  // trimmed_rows, else tail_rows; *form: the VoForm that gives the count
    long graph_replays_ = 0;
    int* pin_tab_ = nullptr; size_t pin_tab_cap_ = 0;     // pinned host staging of the length tables (seed, lengths, row maps, pairing, vocoder
    size_t pin_tab_n_ = 0;                                // extents: host/len_tables.hpp), read by the graph's memcpy node; words in use
    bool pin_valid_ = false;
    std::vector<int32_t> h_tab_;                          // the tables of the run being enqueued, before they are compared with the staging
    unsigned long long* seed_dev_ = nullptr;              // the seed's words inside Batch::tab
    int final_xt_ = 0;
    // a pipelined fetch's buffers (bytes; n samples of encoding enc)
    struct FetchSlot { unsigned char* dev = nullptr; unsigned char* pin = nullptr; size_t cap = 0, n = 0; int enc = ENC_PCM16; hipEvent_t ready = nullptr, done = nullptr; bool busy = false; std::vector<float> dur; };
    FetchSlot fetch_[2];
    int out_hz_ = 0;                  // requested output rate (0: the model's)
    using RsTable = OnDevice<ResampleTable>;
    RsTable rs_, op_rs_;              // filter tables of the output rate and of op_resample
    void rs_prepare(RsTable& m, int in_hz, int out_hz);
    const ResampleTable& rs_table();
    void resample_enqueue(const ResampleTable& t, const float* x, int64_t rows, int64_t W, int enc, void* y, int64_t dst_stride);
    // ---- pitch (engine_pitch.cpp)
    float ps_semi_ = 0.0f;             // the setting in force and its ratio (1 / 1: off)
    int ps_a_ = 1, ps_b_ = 1;
    uint64_t ps_gen_ = 0;              // bumped by every set_pitch and by every change of the pitch mode
    RsTable ps_rs_, op_ps_rs_;         // the b / a tables of the setting and of the op entries, cached per (a, b)
    void ps_table(RsTable& m, int a, int b);
    DevBuf ps_buf_;                    // fetch-time scratch of the shift: exists only once a fetch ran with pitch on
    // the window, per frame the offset and its score, the stretched rows [rows][Ws] and the shifted rows [rows][W]
    struct PsScratch { float* win; int* delta; float* score; float* ys; float* y; size_t bytes; };
    static PsScratch ps_layout(char* base, int64_t rows, int64_t W, const PitchPlan& p);
    std::vector<float> ps_win_;        // what the upload into ps_buf_ reads
    // what ps_buf_'s shifted rows belong to: the finished batch's waveform, the setting, the shape, the scratch
    struct PsKey {
        uint64_t seq = 0, gen = 0; int64_t W = 0; int B = 0; const void* buf = nullptr;
        bool operator==(const PsKey& o) const { return seq == o.seq && gen == o.gen && W == o.W && B == o.B && buf == o.buf; }
    };
    PsKey ps_key_; bool ps_valid_ = false;
    // the two launches of the stretch on rows x W fp32 (x) with spans n (device) under win (device): the offsets, their scores and the
    // stretched rows ys [rows][p.Ws]
    void ps_enqueue(const float* x, int64_t rows, int64_t W, const int64_t* n, int a, int b, const PitchPlan& p, const float* win, int* delta, float* score,
                    float* ys);
    // the stretched rows resampled by t (b / a) into y [rows][W]: the first W outputs of each
    void ps_resample(const ResampleTable& t, const float* ys, int64_t rows, int64_t Ws, int64_t W, float* y);
    void ps_op(int hz, int rows, int W, const float* x, const int64_t* n, int a, int b, float* ys_out, int* delta_out, float* score_out, float* y_out,
               int mode = 0);
    // ---- formant correction (engine_formant.cpp): the end of the pitch stage under STN_PITCH_FORMANT
    int ps_mode_ = 0;                  // STN_PITCH_RESAMPLE; every change bumps ps_gen_
    // the lag window, per (row, frame) the two tables, the gain and the two errors, and the corrected rows [rows][W]
    struct FmScratch { double* lagw; float *ax, *cy; double *g, *ex, *ey; float* out; size_t bytes; };
    static FmScratch fm_layout(char* base, int64_t rows, int64_t W, const FormantPlan& f);
    std::vector<double> fm_lagw_;      // what the upload into the scratch reads
    // the two launches on rows x W fp32 x (before the shift) and y (shifted) with spans n (device) under win and sc.lagw (device)
    void fm_enqueue(const float* x, const float* y, int64_t rows, int64_t W, const int64_t* n, const FormantPlan& f, const float* win, const FmScratch& sc);
    // the finished batch's B rows x W at the model's rate shifted into ps_buf_ (b.wav is left as it is): the rows every later stage
    // reads, row stride W.  Enqueued unless the scratch holds them already
    const float* ps_batch();
    // the rows the output stage starts from: b.wav, or with pitch on the shifted rows
    const float* wav_rows() { return pitch_on() ? ps_batch() : bt_.wav; }
    bool lo_on_ = false;
    float lo_target_ = -23.0f, lo_ceiling_ = -1.0f;
    OnDevice<LoudTable> lo_, op_lo_;   // K-weighting tables of the output rate and of op_loudness
    DevBuf lo_buf_;                    // fetch-time scratch of the measurement
    // what a measurement leaves on the device, [rows] each, and the spans it measured
    struct LoRes { const float *lufs = nullptr, *peak = nullptr, *gain = nullptr; const int64_t* n = nullptr; };
    // per chunk the state (16 B), the peak and the two energy shares; per row the three results (res [3][rows], as the gate writes them:
    // `out` names them; its spans are the measurement's argument); bytes: the size of it all
    struct LoScratch { float *st, *pk, *pa, *pb, *res; LoRes out; size_t bytes; };
    static LoScratch lo_layout(char* base, int64_t rows, int64_t W);
    LoScratch lo_scratch(int64_t rows, int64_t W) { return lo_layout(lo_buf_.reserve(*this, lo_layout(nullptr, rows, W).bytes), rows, W); }
    void lo_prepare(OnDevice<LoudTable>& m, int hz);
    // enqueues the four measurement launches on rows x W fp32 (row stride W) with row lengths n (device): res = [L][peak][gain];
    // st_end (host, or null): the state buffer as the first launch left it, copied out before the scan overwrites it
    // true_peak: a fifth launch between the energy pass and the gate replaces pk by the per-chunk true peaks (kernels_truepeak.hip)
    void lo_measure(const LoudTable& t, const float* x, int64_t rows, int64_t W, const int64_t* n, const LoScratch& sc, int64_t max_seg, bool on, float target,
                    float ceiling, float* st_end = nullptr, bool true_peak = false);
    // op_loudness and op_loudness_ex: the upload, the measurement, the read-back; returns the spans it measured (device, in the arena)
    const int64_t* lo_op(int hz, int rows, int W, const float* x, const int64_t* n, bool on, float target, float ceiling, LoProbe* probe, float* lufs,
               float* peak, float* gain);
    // rows x W fp32 on the device (x) with row spans n (device; the longest max_seg hops of t) measured on the stream against table t
    // true_peak: the gate's peak is the row's true peak (section 16).  The callers that own the setting (lo_batch, join_measure) pass
    // lo_true_peak(); the op-level callers keep the sample peak.
    LoRes lo_rows(const LoudTable& t, const float* x, int64_t rows, int64_t W, const int64_t* n, int64_t max_seg, bool on, float target, float ceiling,
                  bool true_peak = false);
    // (with the limiter active nothing caps the gain: the limiter measures the envelope of the scaled row itself)
    bool lo_true_peak() const { return true_peak_on() && !limiter_active(); }
    // the finished batch's B rows x Wo at the output rate (x) measured on the stream
    LoRes lo_batch(const float* x, int64_t Wo, bool on);
    // the report's launch on what the measurement of rows x W with spans n (device) just left in lo_buf_ (pa, pb) and its read-back, no
    // sync; max_seg: the longest span in segments (lr_max_seg: of the host spans n)
    DevBuf lr_buf_;                    // the report's results: [3][rows] floats, [rows] counts
    static int64_t lr_max_seg(const LoudTable& t, const int64_t* n, size_t rows);
    void lr_report(const LoudTable& t, int64_t rows, int64_t W, const int64_t* n, int64_t max_seg, float* m_max, float* s_max, float* lra, int32_t* n_st);
    // ---- pitch report (engine_f0.cpp)
    DevBuf f0_buf_;                    // the report's tracks and statistics: f0, ap [rows][max_frames], stats [rows]
    // the two launches on rows x W fp32 on the device (x) with spans n (device; nh the same on the host, checked against the cap before
    // this is called) and the read-back into [rows][cap] host arrays, no sync
    void f0_report(int hz, const stn_f0_params& p, const float* x, int64_t rows, int64_t W, const int64_t* n, const int64_t* nh, int64_t cap, float* f0,
                   float* ap, stn_f0_stats* stats);
    // ---- filter chain (engine_filter.cpp)
    std::vector<stn_filter> fl_set_;   // the chain in force
    uint64_t fl_gen_ = 0;              // bumped by every set_filters
    using FlTable = OnDevice<FilterTable, (STN_MAX_FILTERS + 1) / 2>;  // one device copy per section pass
    FlTable fl_, op_fl_;               // the section passes of the chain at the output rate, and of op_filter
    DevBuf fl_buf_;                    // fetch-time scratch of the section passes
    // per chunk the state (16 B) and pass 1's peak (unused): what the measurement's launches take
    struct FlScratch { float *st, *pk; size_t bytes; };
    static FlScratch fl_layout(char* base, int64_t rows, int64_t W);
    void fl_prepare(FlTable& m, int hz, int n, const stn_filter* f);
    // the chain's section passes on rows x W fp32 (x; row stride W; full: W as every row's length, device) into y (may be x; every pass
    // after the first runs in place in y); probe (or null): the states of every pass read out, the state buffer poisoned before each
    void fl_enqueue(const FilterTable& t, const float* x, int64_t rows, int64_t W, const int64_t* full, const FlScratch& sc, float* y, FlProbe* probe);
    void fl_batch(const float* x, int64_t Wo, float* y);  // the finished batch's B rows x Wo (x) through the chain in force into y (may be x)
    // ---- the chain's identity (engine_batch.cpp): the rows behind `stage`, Wo samples each, as everything kept of them is keyed
    RowsId rows_id(Stage stage, int64_t Wo) const;
    // ---- the three dynamics stages: each file holds its layout and its launches; the skeleton around them is shared (engine_internal.hpp)
    // A scratch holds per chunk the stage's state arrays and partial results and per row the results; the launches take the rows' spans
    // beside it (RowSpans::full: what only the de-esser's band launches read)
    // compressor (engine_compressor.cpp): y1 and yL (end values, then start values) and the maximum of yL
    struct CpScratch { float *s1, *s2, *cmax, *rmax; size_t bytes; };
    // de-esser (engine_deesser.cpp): the band's state and max |x| (unused) in front of the compressor's arrays
    struct DsScratch { float *st, *pk, *s1, *s2, *cmax, *rmax; size_t bytes; };
    // expander (engine_expander.cpp): u and yL, the minimum of R - yL and the count of yL <= R / 2
    struct XpScratch { float *s1, *s2, *cmin, *rmin; int32_t* ccnt; int64_t* rcnt; size_t bytes; };
    static CpScratch cp_layout(char* base, int64_t rows, int64_t W);
    static DsScratch ds_layout(char* base, int64_t rows, int64_t W);
    static XpScratch xp_layout(char* base, int64_t rows, int64_t W);
    DynStage<stn_compressor, CompTable> cp_{false, {-24.0f, 3.0f, 6.0f, 5.0f, 120.0f, 0.0f}};
    DynStage<stn_deesser, DeessTable> ds_{false, {5500.0f, -30.0f, 4.0f, 6.0f, 1.0f, 40.0f, 12.0f, STN_DEESS_SPLIT}};
    DynStage<stn_expander, ExpTable> xp_{false, {-50.0f, 3.0f, 6.0f, 24.0f, 1.0f, 30.0f, 150.0f}};
    // the stage's launches (five and the row maxima, eight, six) on rows x W fp32 (x; row stride W) with spans n into y (may be x); probe
    // (or null): every state array read out where the sequence leaves it; gr / band / open: the per-sample outputs (rows x W on the device, or null)
    void cp_enqueue(const CompTable& t, const float* x, int64_t rows, int64_t W, const int64_t* n, const CpScratch& sc, float* y, float* gr, CpProbe* probe);
    void ds_enqueue(const DeessTable& t, const float* x, int64_t rows, int64_t W, const RowSpans& n, const DsScratch& sc, float* y, DsProbe* probe, float* band, float* gr);
    void xp_enqueue(const ExpTable& t, const float* x, int64_t rows, int64_t W, const int64_t* n, const XpScratch& sc, float* y, float* open, XpProbe* probe);
    // out_source's hooks: the finished batch's B rows x Wo (x) through the stage into y (may be x)
    void cp_batch(const float* x, int64_t Wo, float* y);
    void ds_batch(const float* x, int64_t Wo, float* y);
    void xp_batch(const float* x, int64_t Wo, float* y);
    // the skeleton (engine_internal.hpp).  dyn_prepare: m is the table of (hz, c), made by `build` and uploaded unless it is that already.
    // dyn_batch: the fetch hook around `run`, the stage's launches on the carved scratch and the batch's spans (table, scratch, launches, key).
    // dyn_report: a report's preamble around `read`, which is given the scratch to read the rows' results from, or null while the stage
    // is off (zeros).  dyn_op: the op entry around `run`; taps: the per-sample outputs (host, or null), in the order `run` is handed
    // their device rows.  read_rows: one result per row of the batch device -> host (dev null: zeros; host null: nothing).
    // dyn_enqueue: the six launches every stage ends in, with their spans, error checks and probe read-outs, around the stage's launches
    // `chunks` and `reduce`; DynSeq is what a stage says of itself for them.
    struct DynSeq {
        const char* unit;                        // the spans are out.<unit>_chunks1, _scan1, _chunks2, _scan2, _write and _<rows>
        const char* rows;                        // "rowmax" or "rows"
        double flop[3], state[3];                // the three chunk passes: flops per sample, bytes per chunk beside the samples
        double rows_flop, rows_chunk, rows_row;  // the row reduction: flops and bytes per chunk, bytes per row
    };
    template <class Tab, class Sc, class Chunks, class Reduce>
    void dyn_enqueue(const DynSeq& d, const Tab& t, int64_t rows, int64_t W, const Sc& sc, int taps, const DynProbe* probe, StageSpan* open, Chunks chunks,
                     Reduce reduce);
    template <class Made, class Set, class Build> void dyn_prepare(Made& m, int hz, const Set& c, Build build);
    template <class St, class Build, class Layout, class Run> void dyn_batch(St& st, Stage stage, int64_t Wo, Build build, Layout layout, Run run);
    template <class St, class Layout, class Read> void dyn_report(St& st, Stage stage, Layout layout, bool wanted, Read read);
    template <class St, class Set, class Probe, class Build, class Layout, class Run>
    void dyn_op(St& st, int hz, int rows, int W, const float* x, const Set& c, float* y, Probe* probe, Build build, Layout layout,
                std::initializer_list<float*> taps, Run run);
    template <class T> void read_rows(T* host, const T* dev);
    // shapes_rows: a stage behind the rate is on (the set enqueue_output's store-from-scratch branch asks for).  out_in_scratch:
    // out_source() returns the fp32 fetch scratch (row stride Wo); otherwise, pitch or nothing, wav_rows(): b.wav or the shifted rows
    // in the pitch scratch, row stride W like b.wav
    bool shapes_rows() const { return filter_on() || expander_on() || deesser_on() || compressor_on(); }
    bool out_in_scratch() const { return resample_on() || shapes_rows(); }
    bool st_on_ = false;
    float st_db_ = 40.0f, st_keep_ = 20.0f, st_fade_ = 5.0f;
    uint64_t ed_seq_ = 0;              // the finished batch's waveform: bumped by every batch_run and by dbg_batch_set_wav
    DevBuf ed_buf_;                    // fetch-time scratch of the detection
    // per chunk the two frame shares, per frame the level, per row the edges and the one-member programme of the per-row trimmed fetch
    // With the pause limit (S > 0; section 17) also S segments, one programme and 2 S words {cuts, len, lo, hi, ...} per row, behind the
    // rest: S = 0 carves exactly what trimming alone needs
    struct EdScratch {
        float *pa, *pb; double* lev; int64_t* edges; JoinSegT* seg; JoinProg* prog; size_t bytes;
        JoinSegT* pseg = nullptr; JoinProg* pprog = nullptr; int64_t* pcut = nullptr; int S = 0;
    };
    static EdScratch ed_layout(char* base, int64_t rows, int64_t W, int hz, int S);
    EdScratch ed_scratch(int64_t rows, int64_t W, int hz, int S);
    bool pl_on_ = false;
    float pl_ms_ = 300.0f;
    int pl_stride(bool pauses, int64_t W, int hz) const { return pauses ? pause_stride(W, hz, pause_samples(hz, pl_ms_)) : 0; }
    // what the scratch holds: the edges (and per-row programmes) of the rows behind the whole chain under (db, keep, fade) and mp, the
    // max_pause_ms of the cuts held beside the edges (0: none); host: read back
    struct EdKey {
        RowsId rows; const void* buf = nullptr; float db = 0, keep = 0, fade = 0, mp = 0;
        bool operator==(const EdKey& o) const { return rows == o.rows && buf == o.buf && db == o.db && keep == o.keep && fade == o.fade && mp == o.mp; }
    };
    EdKey ed_key(int64_t Wo, bool pauses) const { return {rows_id(ST_COMPRESSOR, Wo), ed_buf_.get(), st_db_, st_keep_, st_fade_, pauses ? pl_ms_ : 0.0f}; }
    EdKey ed_key_; bool ed_valid_ = false, ed_host_valid_ = false;
    std::vector<int64_t> ed_host_;          // [B][2] edges read back
    std::vector<int64_t> pz_host_; int pz_S_ = 0;  // [B][2 S] the rows' cut lists read back with the edges (key.mp != 0)
    DevBuf st_win_; int st_win_hz_ = 0; float st_win_ms_ = -1.0f;  // the fade window on the device, per (rate, fade_ms)
    const float* st_window(int hz);
    // the two detection launches on rows x W fp32 (x) at hz with the spans n (device): the edges and per-row programmes into sc
    // (sc.S > 0: and the pause limit's launch behind them, Mp samples: the rows' segment tables and cut lists into sc)
    void ed_enqueue(const float* x, int64_t rows, int64_t W, const int64_t* n, int hz, float top_db, float keep_ms, float fade_ms, const EdScratch& sc, int64_t Mp = 0);
    void ed_op(const char* entry, const char* who, bool pauses, int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms,
               float fade_ms, float max_pause_ms, const float* gain, int enc, void* y, EdProbe* probe, int64_t* start, int64_t* end, int64_t* len,
               int32_t* n_cuts, int64_t* cuts, int cap_pairs);
    // the finished batch's B rows x Wo at the output rate (x): detection enqueued unless the scratch holds it already; pauses: with the
    // cuts under pl_ms_ (the fetch paths pass pause_limit_active())
    EdScratch ed_batch(const float* x, int64_t Wo, bool pauses);
    // its edges on the host (one device->host read of 2 B integers per batch and setting), and with pauses its cut lists in pz_host_
    const std::vector<int64_t>& ed_batch_host(bool pauses);
    bool lm_on_ = false;
    float lm_ms_ = 5.0f;
    float lo_cap() const { return limiter_active() ? INFINITY : lo_ceiling_; }  // the gate's ceiling: the limiter enforces it instead
    DevBuf lm_buf_;                    // fetch-time scratch of the limiter
    // the limited rows, per tile the two partial results, per row the two results
    struct LmScratch { float* y; int* pcnt; float* pmin; int64_t* limited; float* red; size_t bytes; const float* trim = nullptr; };
    static LmScratch lm_layout(char* base, int64_t rows, int64_t W);
    LmScratch lm_scratch(int64_t rows, int64_t W);
    DevBuf lm_win_; int lm_win_hz_ = 0; float lm_win_ms_ = -1.0f;  // the weights on the device, per (rate, ms)
    const float* lm_window(int hz);
    // (engine_truepeak.cpp) per chunk the peak, per row four results, and (with_env) the envelope rows
    struct TpScratch { float *pk, *tp_in, *tp_out, *tp_y, *trim, *env; size_t bytes; };
    // The limiter's launches on rows x W fp32 (x) with spans n, times g (device [rows] or null), against the ceiling c with the A + 1
    // weights w: the limited rows and the per-row results into sc, the curve into s (device [rows][W], or null).  tp (true-peak mode, or
    // null): the envelope of x * g is taken first and drives the curve, and behind the limiter tp->tp_y and tp->trim are the true peak of
    // the limited row and the gain that holds it at c
    void lm_enqueue(const float* x, int64_t rows, int64_t W, const int64_t* n, const float* g, float c, int64_t A, const float* w, const LmScratch& sc,
                    float* s, const TpScratch* tp);
    // rows x W fp32 on the device (x) with spans n (device), times g (device [rows]), limited into the scratch: returns the rows (row
    // stride W).  In true-peak mode .trim (device [rows]) is the gain the store behind it applies
    LmScratch lm_rows(const float* x, int64_t rows, int64_t W, const int64_t* n, const float* g);
    bool pk_true_ = false;             // the peak mode (engine_truepeak.cpp)
    bool true_peak_on() const { return pk_true_ && lo_on_; }
    DevBuf tp_buf_;                    // fetch-time scratch of the true-peak mode
    static TpScratch tp_layout(char* base, int64_t rows, int64_t W, bool with_env);
    TpScratch tp_scratch(int64_t rows, int64_t W, bool with_env);
    // tp[row] (and trim[row] against c when trim is not null) of rows x W times g (device [rows] or null), spans n (device); env (device
    // [rows][W], or null): the true-peak envelope of x * g
    void tp_rows(const float* x, int64_t rows, int64_t W, const int64_t* n, const float* g, float* pk, float* env, float c, float* tp, float* trim);
    // ---- output stage (engine_batch.cpp): the one place that turns the finished batch into what a fetch delivers (rate, loudness,
    // sample encoding); every fetch path runs it into a device destination of rows `stride` samples apart, enc_bytes(enc) bytes each
    // With a join plan the G programme rows of the plan instead of the B rows (scope: STN_JOIN_GAIN_*)
    struct OutRows { void* dst = nullptr; int enc = ENC_F32; int64_t stride = 0; const JoinPlan* join = nullptr; int scope = 0; };
    void enqueue_output(const OutRows& o);
    void enqueue_joined(const OutRows& o);
    Dither dither_;  // the setting (mode, seed); the streams of a fetch are out_dither's
    // section 23: the per-row fetches key a row by its utterance id (the batch's device ids), the joined ones a programme by its index
    Dither out_dither(unsigned kind) const { return {dither_.mode, dither_.seed, kind, kind == DITHER_ROW ? bt_.utt_ids : nullptr}; }
    bool dithers(int enc) const { return dither_.mode != DITHER_OFF && (enc == ENC_PCM16 || enc == ENC_PCM24); }
    void slot_begin(int slot, OutRows o, int64_t rows, int64_t width, const std::vector<float>& dur);  // the pipelined fetch behind both _begin calls
    // The gain step between the measurement m and the store: the rows to store from, their gains and their row stride.  Those are src,
    // m.gain and `stride`; with the limiter active (section 15) the rows x W limited in the fetch scratch, their trim (null outside true
    // mode) and W.  Without loudness m is empty, and so is the gain.
    struct GainedRows { const float* src; const float* g; int64_t stride; };
    GainedRows gain_step(const float* src, int64_t rows, int64_t W, int64_t stride, const LoRes& m);
    // the joined fp32 signal of the finished batch at the output rate in the fetch scratch (rows W_join apart) and its measurement; the
    // two halves of a per-programme gain
    const float* join_f32(const JoinPlan& p);
    LoRes join_measure(const JoinPlan& p, const float* joined, bool on);
    // the plan's device tables in grow-only fetch scratch, uploaded only when the plan differs from what the scratch holds
    // tseg: trimmed sources (seg unused); span: the programmes' spans [G], what a measurement of the joined rows takes
    struct JoinTables { const JoinSeg* seg; const JoinProg* prog; const int64_t* span; const JoinSegT* tseg = nullptr; const float* fade = nullptr; };
    JoinTables join_tables(const JoinPlan& p);
    // programme g's span: what the reference's hosts write to a file, its duration at the output rate (section 11's rule) inside its length
    std::vector<int64_t> join_spans(const JoinPlan& p) const;
    // members of 3 words (JoinSeg) or, trimmed sources, 5 (JoinSegT) per piece, then the programmes, then their spans
    static std::vector<int64_t> join_table_words(const JoinPlan& p, const std::vector<int64_t>& span);
    // the pointers into those words on the device; for trimmed sources also the fade window of the output rate, uploaded here if need be
    // (st_window: why this is no static function; op_join's plans have no trimmed sources and never get there)
    JoinTables join_tables_at(const int64_t* d, const JoinPlan& p);
    // n rows' results into whichever of the three host arrays is not null; the caller syncs
    void lo_read_back(const LoRes& m, size_t n, float* lufs, float* peak, float* gain);
    int64_t native_row_len() const { return (int64_t)bt_.L * a_.base_chunk_size * a_.chunk_compress_factor; }  // samples of a row of b.wav
    void join_enqueue(const float* x, int64_t src_stride, const JoinTables& t, const JoinPlan& p, const float* g, int enc, void* y, int64_t dst_stride,
                      const Dither& d = {});
    DevBuf join_tab_;
    std::vector<int64_t> join_tab_host_;  // what join_tab_ holds (empty: nothing)
    int64_t out_row_len();               // samples per delivered row; sets the device and throws without a finished batch
    bool out_native() const;             // neither shifted, resampled, filtered nor normalized: the delivered fp32 rows are b.wav itself
    // the finished batch at the output rate: b.wav, or resampled and / or filtered (section 18) into the fp32 scratch, row stride Wo
    const float* out_source(int64_t Wo);
    float* out_f32_buf(size_t n) { return reinterpret_cast<float*>(out_f32_.reserve(*this, n * sizeof(float))); }
    void* out_enc_buf(size_t bytes) { return out_enc_.reserve(*this, bytes); }
    DevBuf out_f32_, out_enc_;        // fetch scratch: fp32 rows at the output rate, rows in the fetch's encoding
    hipStream_t copy_s_ = nullptr;
    bool prof_on_ = false;
    std::vector<ProfSpan> spans_;
    std::vector<hipEvent_t> ev_pool_;
};

}  // namespace stn
