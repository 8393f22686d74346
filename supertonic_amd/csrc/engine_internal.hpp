// engine_internal.hpp — helpers shared by the engine's translation units (engine.cpp: lifecycle, weights, blocks and the four stages;
// engine_batch.cpp: the resident-batch pipeline and its graph cache; engine_ops.cpp: the single-kernel and timing entry points of the tests
// and tools).
#pragma once
#include "engine.hpp"
#include "kernels_chunk.hpp"

#include <algorithm>
#include <array>
#include <cstdio>
#include <optional>

namespace stn {
namespace detail {
// host array -> arena (asynchronous copy on `s`)
template <typename T>
inline T* up(Arena& ar, hipStream_t s, const T* h, size_t n) {
    T* d = static_cast<T*>(ar.alloc(n * sizeof(T)));
    STN_HIP(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, s));
    return d;
}
}  // namespace detail

// a number as the refusals print it
inline std::string num(double v) {
    char b[48];
    std::snprintf(b, sizeof(b), "%g", v);
    return b;
}

// why a setting of `unit` is refused, or "": the first field outside its range, "<unit>: <name> <v> must be in [<lo>, <hi>]"
struct Lim { const char* name; float v, lo, hi; };
template <class Lims>
inline std::string range_check(const char* unit, const Lims& lim) {
    for (const Lim& l : lim)  // (a NaN fails both comparisons)
        if (!(l.v >= l.lo && l.v <= l.hi)) return std::string(unit) + ": " + l.name + " " + num(l.v) + " must be in [" + num(l.lo) + ", " + num(l.hi) + "]";
    return "";
}

// The scope of one op-level entry: constructed first thing, it selects the engine's device and resets the arena, and
// every device byte the entry touches goes through it.  Allocations come from the arena in call order (blocks 256-byte aligned);
// uploads, fills and read-backs are enqueued on the engine's stream, and the host arrays they read or write are the entry's to keep
// alive until its closing sync().
class OpScope {
   public:
    static constexpr size_t G = 64;                  // floats of guard on either side of a guarded block
    static constexpr uint32_t POISON = 0x7FC00000u;  // the quiet NaN: what a launch fails to write reads back as this
    explicit OpScope(Engine& e) : eng_(e) {
        STN_HIP(hipSetDevice(eng_.device_));
        eng_.ar_.reset();
    }
    OpScope(const OpScope&) = delete;
    OpScope& operator=(const OpScope&) = delete;

    template <typename T> T* buf(size_t n) { return static_cast<T*>(eng_.ar_.alloc(n * sizeof(T))); }
    // host -> a device array the entry already holds
    template <typename T> void put(T* dev, const T* host, size_t n) { STN_HIP(hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, eng_.s_)); }
    // host -> arena, the array `off` elements behind its block's boundary; a null host allocates nothing and gives null
    template <typename T> T* up(const T* host, size_t n, size_t off = 0) {
        if (!host) return nullptr;
        T* d = buf<T>(n + off) + off;
        put(d, host, n);
        return d;
    }
    template <typename T> T* up(const std::vector<T>& host) { return up(host.data(), host.size()); }
    static void poison(hipStream_t s, void* p, size_t words) { STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), POISON, words, s)); }
    void poison(void* p, size_t words) { poison(eng_.s_, p, words); }
    // a scratch layout (xx_layout) on a block of the size it asks for; carve_poisoned: the whole block filled with the poison when `on`
    template <class Layout, class... A> auto carve_poisoned(bool on, Layout layout, const A&... a) {
        const size_t bytes = layout(nullptr, a...).bytes;
        char* b = buf<char>(bytes);
        if (on) poison(b, bytes / 4);
        return layout(b, a...);
    }
    template <class Layout, class... A> auto carve(Layout layout, const A&... a) { return carve_poisoned(false, layout, a...); }
    // device -> host; a null host reads nothing.  rows(): `rows` rows of w elements, dev_stride elements apart on the device
    template <typename T> void down(T* host, const T* dev, size_t n) {
        if (host) STN_HIP(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, eng_.s_));
    }
    void down_rows(void* host, const void* dev, size_t w_bytes, size_t dev_stride_bytes, size_t rows) {
        if (host) STN_HIP(hipMemcpy2DAsync(host, w_bytes, dev, dev_stride_bytes, w_bytes, rows, hipMemcpyDeviceToHost, eng_.s_));
    }
    // the entry's spans (checked by stn::spans) and the width beside them; the host copy stays with the engine until the closing sync()
    RowSpans spans(int rows, int W, std::vector<int64_t> n) {
        eng_.op_sp_ = std::move(n);
        eng_.op_sp_.resize((size_t)rows * 2, (int64_t)W);
        const int64_t* d = up(eng_.op_sp_.data(), eng_.op_sp_.size());
        return {d, d + rows};
    }
    RowSpans full_spans(int rows, int W) { return spans(rows, W, std::vector<int64_t>((size_t)rows, (int64_t)W)); }
    // [guard][n floats][guard], the n floats `off` floats off the block's boundary; filled with the poison when probing.  guards_ok():
    // every guard word of every such block still holds it (waits for the stream)
    float* guarded(size_t n, size_t off, bool probing) {
        float* b = buf<float>(n + 2 * G + off);
        if (probing) poison(b, n + 2 * G + off);
        guards_.push_back({b, n, off});
        return b + G + off;
    }
    bool guards_ok() {
        std::vector<uint32_t> g;
        for (const Guarded& b : guards_) g.resize(g.size() + 2 * G + b.off);
        uint32_t* p = g.data();
        for (const Guarded& b : guards_) {
            down(p, reinterpret_cast<const uint32_t*>(b.p), G + b.off);
            down(p + G + b.off, reinterpret_cast<const uint32_t*>(b.p) + G + b.off + b.n, G);
            p += 2 * G + b.off;
        }
        eng_.sync();
        return std::all_of(g.begin(), g.end(), [](uint32_t v) { return v == POISON; });
    }

   private:
    struct Guarded { float* p; size_t n, off; };
    Engine& eng_;
    std::vector<Guarded> guards_;
};

// ---- the host skeleton of the three dynamics stages (DynStage) --------------------------------------------------
// A stage's fields with their limits, in the order of its struct: the one list its check and its equality walk (engine_<stage>.cpp)
std::array<Lim, 6> limits(const stn_compressor& c);
std::array<Lim, 7> limits(const stn_deesser& c);
std::array<Lim, 7> limits(const stn_expander& c);
template <class Set> inline bool same_tail(const Set&, const Set&) { return true; }
inline bool same_tail(const stn_deesser& a, const stn_deesser& b) { return a.mode == b.mode; }
// float == per field (so -0.0f is 0.0f, and a NaN, which no check lets in, is no setting's equal)
template <class Set>
inline bool same_setting(const Set& a, const Set& b) {
    const auto x = limits(a), y = limits(b);
    for (size_t i = 0; i < x.size(); ++i)
        if (!(x[i].v == y[i].v)) return false;
    return same_tail(a, b);
}
// a table's host arrays handed over to their owners d, and its device pointers filled in from them
inline void to_device(Engine& e, DeviceTable* d, CompTable& t) { t.dev = d[0].put(e, t.pw); }
inline void to_device(Engine& e, DeviceTable* d, ExpTable& t) { t.dev = d[0].put(e, t.pw); }
inline void to_device(Engine& e, DeviceTable* d, DeessTable& t) { t.band.dev = d[0].put(e, t.band.mpow); t.det.dev = d[1].put(e, t.det.pw); }

// set_<stage>: off bumps the generation only if the stage was on, the same setting again bumps nothing, a refused one changes nothing
template <class St, class Set>
inline void dyn_set(St& st, bool on, const Set* c, const std::string& why) {
    if (!on) {
        if (st.on) ++st.gen;
        st.on = false;
        return;
    }
    refuse(why);
    if (st.on && same_setting(st.set, *c)) return;
    st.set = *c;
    st.on = true;
    ++st.gen;
}

template <class Made, class Set, class Build>
void Engine::dyn_prepare(Made& m, int hz, const Set& c, Build build) {
    if (m.dev[0] && m.t.hz == hz && same_setting(m.from, c)) return;
    decltype(m.t) t;
    build(hz, c, t);
    m.t.hz = -1;  // (no rate's table while its device copies change hands)
    to_device(*this, m.dev, t);
    m.t = std::move(t);
    m.from = c;
}

template <class St, class Build, class Layout, class Run>
void Engine::dyn_batch(St& st, Stage stage, int64_t Wo, Build build, Layout layout, Run run) {
    const int hz = output_rate();
    dyn_prepare(st.tab, hz, st.set, build);
    const auto sc = layout(st.buf.reserve(*this, layout(nullptr, bt_.B, Wo).bytes), bt_.B, Wo);
    run(sc, batch_spans(hz, Wo).dev);
    st.key = rows_id(stage, Wo);
    st.key_buf = st.buf.get();
    st.valid = true;
}

// The six launches a dynamics stage ends in, on rows x W fp32 with the scratch sc (its s1 and s2) and the scan table t (comb and the two
// power tables in dev): chunk pass 1, scan 1, chunk pass 2, scan 2, the write pass, the row reduction.  d: the stage's description.
// chunks(pass) and reduce() are the stage's launches; taps: how many per-sample outputs the write pass stores; probe (or null): the four
// state arrays read out where the sequence leaves them; open (or null): the span a prologue of the stage's own left open.
template <class Tab, class Sc, class Chunks, class Reduce>
void Engine::dyn_enqueue(const DynSeq& d, const Tab& t, int64_t rows, int64_t W, const Sc& sc, int taps, const DynProbe* probe, StageSpan* open,
                         Chunks chunks, Reduce reduce) {
    const double samples = (double)rows * W, nchunks = (double)rows * lo_chunks(W);
    const size_t st_bytes = (size_t)rows * (size_t)lo_chunks(W) * 4;
    std::optional<StageSpan> own;
    auto step = [&](const char* name, double flops, double bytes) {
        char tag[64];
        std::snprintf(tag, sizeof(tag), "%s_%s", d.unit, name);
        if (open) open->next(tag, flops, bytes);
        else open = &own.emplace(*this, "out", tag, flops, bytes);
    };
    auto done = [&](float* dst, const float* src) {
        STN_HIP(hipGetLastError());
        if (probe && dst) STN_HIP(hipMemcpyAsync(dst, src, st_bytes, hipMemcpyDeviceToHost, s_));
    };
    auto scan = [&](ScanComb comb, int half, float* st) { launch_chunk_scan(s_, comb, d.unit, rows, W, t.dev ? t.dev + half * LO_SCAN : nullptr, st); };
    step("chunks1", d.flop[0] * samples, samples * 4 + nchunks * d.state[0]);
    chunks(1);
    done(probe ? probe->s1_end : nullptr, sc.s1);
    step("scan1", nchunks * 11 * 2, nchunks * 8);
    scan(Tab::comb, 0, sc.s1);
    done(probe ? probe->s1_start : nullptr, sc.s1);
    step("chunks2", d.flop[1] * samples, samples * 4 + nchunks * d.state[1]);
    chunks(2);
    done(probe ? probe->s2_end : nullptr, sc.s2);
    step("scan2", nchunks * 11 * 2, nchunks * 8);
    scan(SCAN_LINEAR, 1, sc.s2);
    done(probe ? probe->s2_start : nullptr, sc.s2);
    step("write", d.flop[2] * samples, samples * (8 + 4 * taps) + nchunks * d.state[2]);
    chunks(3);
    done(nullptr, nullptr);
    step(d.rows, nchunks * d.rows_flop, nchunks * d.rows_chunk + (double)rows * d.rows_row);
    reduce();
    done(nullptr, nullptr);
}

template <class St, class Layout, class Read>
void Engine::dyn_report(St& st, Stage stage, Layout layout, bool wanted, Read read) {
    const int64_t Wo = out_row_len();
    if (!wanted) return;
    if (!st.on) {  // nothing is turned down
        read(static_cast<decltype(layout(nullptr, 0, 0))*>(nullptr));
        return;
    }
    // the row results a fetch of this batch under this rate, chain and setting left in the scratch are the report; otherwise the sequence runs
    if (!(st.valid && st.key == rows_id(stage, Wo) && st.key_buf == st.buf.get())) (void)out_source(Wo);
    const auto sc = layout(st.buf.reserve(*this, layout(nullptr, bt_.B, Wo).bytes), bt_.B, Wo);
    read(&sc);
    sync();
}

template <class T>
void Engine::read_rows(T* host, const T* dev) {
    if (!host) return;
    if (!dev) std::fill(host, host + bt_.B, T(0));
    else STN_HIP(hipMemcpyAsync(host, dev, (size_t)bt_.B * sizeof(T), hipMemcpyDeviceToHost, s_));
}

template <class St, class Set, class Probe, class Build, class Layout, class Run>
void Engine::dyn_op(St& st, int hz, int rows, int W, const float* x, const Set& c, float* y, Probe* probe, Build build, Layout layout,
                    std::initializer_list<float*> taps, Run run) {
    OpScope op(*this);
    dyn_prepare(st.op_tab, hz, c, build);
    const size_t nx = (size_t)rows * W, off = probe && probe->x_misalign ? 1 : 0;
    float* dx = op.guarded(nx, off, probe);
    float* dy = probe && probe->in_place ? dx : op.guarded(nx, off, probe);
    op.put(dx, x, nx);
    std::vector<float*> dev;
    for (float* h : taps) dev.push_back(h ? op.buf<float>(nx) : nullptr);
    const auto sc = op.carve_poisoned(probe, layout, rows, W);
    for (float* d : dev)
        if (probe && d) op.poison(d, nx);
    run(st.op_tab.t, sc, op.full_spans(rows, W), dx, dy, dev.data());
    op.down(y, dy, nx);
    size_t i = 0;
    for (float* h : taps) op.down(h, dev[i++], nx);
    if (probe) {
        probe->guard_ok = op.guards_ok();
        probe->form = chunk_staging_form(dx, dy, W);
    }
    sync();
}
}  // namespace stn
