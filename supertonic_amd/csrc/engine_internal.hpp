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

// The rows of an op-level entry on the device, from the engine's arena: [guard][x][guard] and [guard][y][guard] (in place: one block),
// the blocks filled with the quiet NaN 0x7FC00000 when probing, both 4 bytes off a 16-byte boundary when misaligned (the arena's blocks
// are 256-byte aligned).  x is uploaded; the caller's launches read dx and write dy.
struct GuardedRows {
    static constexpr size_t G = 64;
    Engine& e;
    size_t nx, off;
    float *bx, *by, *dx, *dy;
    GuardedRows(Engine& eng, size_t n, const float* x, bool probing, bool misalign, bool in_place) : e(eng), nx(n), off(misalign ? 1 : 0) {
        bx = static_cast<float*>(e.arena().alloc((nx + 2 * G + off) * 4));
        by = in_place ? bx : static_cast<float*>(e.arena().alloc((nx + 2 * G + off) * 4));
        dx = bx + G + off;
        dy = by + G + off;
        if (probing)
            for (float* b : {bx, by}) STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b), 0x7FC00000, nx + 2 * G + off, e.stream()));
        STN_HIP(hipMemcpyAsync(dx, x, nx * 4, hipMemcpyHostToDevice, e.stream()));
    }
    void download(float* y) const { STN_HIP(hipMemcpyAsync(y, dy, nx * 4, hipMemcpyDeviceToHost, e.stream())); }
    // every guard word still holds the poison (waits for the stream)
    bool guards_ok() const {
        std::vector<uint32_t> g(4 * G + 2 * off);
        uint32_t* p = g.data();
        for (float* b : {bx, by}) {
            STN_HIP(hipMemcpyAsync(p, b, (G + off) * 4, hipMemcpyDeviceToHost, e.stream()));
            STN_HIP(hipMemcpyAsync(p + G + off, b + G + off + nx, G * 4, hipMemcpyDeviceToHost, e.stream()));
            p += 2 * G + off;
        }
        e.sync();
        return std::all_of(g.begin(), g.end(), [](uint32_t v) { return v == 0x7FC00000u; });
    }
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
    STN_HIP(hipSetDevice(device_));
    dyn_prepare(st.op_tab, hz, c, build);
    ar_.reset();
    const size_t nx = (size_t)rows * W;
    GuardedRows r(*this, nx, x, probe, probe && probe->x_misalign, probe && probe->in_place);
    std::vector<float*> dev;
    for (float* h : taps) dev.push_back(h ? static_cast<float*>(ar_.alloc(nx * 4)) : nullptr);
    const size_t sc_bytes = layout(nullptr, rows, W).bytes;
    char* sb = static_cast<char*>(ar_.alloc(sc_bytes));
    const auto sc = layout(sb, rows, W);
    if (probe) {
        for (float* d : dev)
            if (d) STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d), 0x7FC00000, nx, s_));
        STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sb), 0x7FC00000, sc_bytes / 4, s_));
    }
    run(st.op_tab.t, sc, op_spans(rows, W, std::vector<int64_t>((size_t)rows, (int64_t)W)), r.dx, r.dy, dev.data());
    r.download(y);
    size_t i = 0;
    for (float* h : taps) {
        if (h) STN_HIP(hipMemcpyAsync(h, dev[i], nx * 4, hipMemcpyDeviceToHost, s_));
        ++i;
    }
    if (probe) {
        probe->guard_ok = r.guards_ok();
        probe->form = chunk_staging_form(r.dx, r.dy, W);
    }
    sync();
}
}  // namespace stn
