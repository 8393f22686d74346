// kernels_dynamics.hip — the three fetch-time dynamics stages: compressor, de-esser, expander (gfx950, wave64; DESIGN.md sections 20,
// 21, 25, and 20a for this unit's form).
//
// Each stage is, per row and sample in fp32, a detector recurrence d on a level of the signal, a smoothing yL = yL + kA (drive(d) - yL)
// of it, and a gain from yL applied to the sample.  Neither recurrence is the 4-state linear system of the filter chain, but both
// compose over a chunk of len samples:
//   stage 1  d  -> the stage's max-form of (e, d)   e the chunk's end value from d = 0    (max commutes with a positive factor and a shift)
//   stage 2  yL -> E yL + c                         E = (1 - kA)^len, c the chunk's end value from yL = 0, driven by the TRUE d in the chunk
// so c exists only after stage 1's start states do.  The protocol, stated once (dyn_chunk_kernel, chunk_scan_kernel, dyn_rows_kernel;
// the host's sequence is Engine::dyn_enqueue), every hand-off a launch boundary, no atomics:
//   1. chunk pass 1: d from zero -> e_k                      2. scan 1 by the stage's combination, in double -> d at every chunk's start
//   3. chunk pass 2: d from its start, yL from zero -> c_k   4. scan 2 (+, x) in double -> yL at every chunk's start
//   5. write pass: both from their start states -> y, the probe taps, and the chunk's accumulator over the row's valid samples
//   6. the row reduction of the chunks' accumulators (stn_batch_compressor, stn_batch_deesser, stn_batch_expander)
// A stage (Compressor, Expander, DeEsser<kSplit> below) supplies only what is its own: the detector step, what drives the smoothing, the
// accumulator, the taps and the gain.  The steps themselves are kernels_chunk.hpp's (gain_want, gain_peak, gain_smooth, expand_open,
// expand_detect, biquad2_step; one definition each): the start states the scans form are exact for this arithmetic only.
// Chunks are LO_CHUNK samples counted from sample 0; a workgroup stages LO_WG of them through LDS as filter_write_kernel does
// (chunk_stage_in / chunk_stage_out: 16-byte loads and stores or the scalar form, row stride 33 words).  In place (y == x) is allowed:
// a workgroup reads the samples it owns into LDS before the first barrier and stores after the second.
// A row's y[0 .. n) depends on x[0 .. n) of that row and the coefficients only: the scans' order is fixed by the chunk index.
#include "kernels_chunk.hpp"

#include <math.h>

namespace stn {

namespace {

constexpr int DYN_SPAN = LO_WG * LO_CHUNK;  // samples a workgroup owns
constexpr int DYN_PAD = LO_CHUNK + 1;       // LDS words per chunk: the lanes' walks fall on distinct banks
constexpr int DYN_ROWS = 256;               // threads of the row reduction's workgroup

// ---- the accumulators: what the write pass leaves per chunk over the row's valid samples and the row reduction joins per row.  start
// is the value of no sample at all; R is the stage's range (AccMax reads none).  A maximum or minimum of floats and a sum of integers
// do not depend on the order they are taken in.
// the maximum of yL (compressor, de-esser): part m[row][k], 0 when the chunk has no valid sample -> out m[row]
struct AccMax {
    struct Part { float* __restrict__ m; };
    struct Out { float* __restrict__ m; };
    template <int N> struct Lds { float m[N]; };
    float m;
    static __device__ __forceinline__ AccMax start(float) { return {0.0f}; }
    __device__ __forceinline__ void sample(float, float yl) { m = fmaxf(m, yl); }
    __device__ __forceinline__ void join(const AccMax& o) { m = fmaxf(m, o.m); }
    static __device__ __forceinline__ AccMax load(const Part& p, int64_t i) { return {p.m[i]}; }
    __device__ __forceinline__ void store(const Part& p, int64_t i) const { p.m[i] = m; }
    __device__ __forceinline__ void store(const Out& o, int64_t i) const { o.m[i] = m; }
    template <int N> static __device__ __forceinline__ AccMax get(const Lds<N>& s, int i) { return {s.m[i]}; }
    template <int N> __device__ __forceinline__ void put(Lds<N>& s, int i) const { s.m[i] = m; }
    static bool null(const Part& p) { return !p.m; }
};
// the minimum of R - yL and the count of yL <= R / 2 (expander): parts m, c[row][k], R and 0 when the chunk has no valid sample -> out
// m[row] and the int64 sum c[row]
struct AccMinCount {
    struct Part { float* __restrict__ m; int32_t* __restrict__ c; };
    struct Out { float* __restrict__ m; int64_t* __restrict__ c; };
    template <int N> struct Lds { float m[N]; int64_t c[N]; };
    float m;
    int64_t c;
    static __device__ __forceinline__ AccMinCount start(float R) { return {R, 0}; }
    __device__ __forceinline__ void sample(float R, float yl) {
        m = fminf(m, R - yl);
        c += yl <= 0.5f * R ? 1 : 0;
    }
    __device__ __forceinline__ void join(const AccMinCount& o) {
        m = fminf(m, o.m);
        c += o.c;
    }
    static __device__ __forceinline__ AccMinCount load(const Part& p, int64_t i) { return {p.m[i], p.c[i]}; }
    __device__ __forceinline__ void store(const Part& p, int64_t i) const {
        p.m[i] = m;
        p.c[i] = (int32_t)c;  // (at most LO_CHUNK)
    }
    __device__ __forceinline__ void store(const Out& o, int64_t i) const {
        o.m[i] = m;
        o.c[i] = c;
    }
    template <int N> static __device__ __forceinline__ AccMinCount get(const Lds<N>& s, int i) { return {s.m[i], s.c[i]}; }
    template <int N> __device__ __forceinline__ void put(Lds<N>& s, int i) const {
        s.m[i] = m;
        s.c[i] = c;
    }
    static bool null(const Part& p) { return !p.m || !p.c; }
};

// ---- the stages.  Bufs: s1, s2, the probe taps (each or null: a fetch passes null), the per-chunk results; passed by value.  Lane:
// state a lane loads once per chunk (i = row * Ks + k).  detect: d' from the sample and d.  drive: what the smoothing follows.  range:
// the accumulator's R.  tap: the per-sample outputs at j = row * W + the sample's index.  apply: the sample's output.  Front: the stage
// whose passes 1 and 2 these are (apply and tap are the write pass's alone).
struct NoLane {};

// compressor (section 20; include/stn.h "compressor"): the level xG in dB, the gain computer's wanted reduction z >= 0, the decoupled
// peak detector y1 = max(z, y1 - kR y1) (stage 1: y1 -> max(e, D y1), D = (1 - kR)^len), yL on y1, y = x 10^((makeup - yL) / 20)
struct Compressor {
    using Coef = CompCoef;
    using Acc = AccMax;
    using Lane = NoLane;
    using Front = Compressor;
    struct Bufs { float *__restrict__ s1, *__restrict__ s2, *__restrict__ gr, *__restrict__ cmax; };
    static constexpr const char* unit = "compressor";
    static bool lane_null(const Bufs&) { return false; }
    static __host__ __device__ __forceinline__ Acc::Part part(const Bufs& b) { return {b.cmax}; }
    static __device__ __forceinline__ Lane lane(const Bufs&, int64_t) { return {}; }
    static __device__ __forceinline__ float detect(const Coef& f, Lane&, float x, float y1) { return gain_peak(f.kR, gain_want(f.T, f.S, f.K, x), y1); }
    static __device__ __forceinline__ float drive(const Coef&, float y1) { return y1; }
    static __device__ __forceinline__ float range(const Coef&) { return 0.0f; }
    static __device__ __forceinline__ void tap(const Bufs& b, const Lane&, int64_t j, float yl) { if (b.gr) b.gr[j] = yl; }
    static __device__ __forceinline__ float apply(const Coef& f, const Lane&, float x, float yl) { return x * exp10f((f.makeup - yl) / 20.0f); }
};

// expander (section 25; include/stn.h "expander"): the level xG in dB, the wanted attenuation z in [0, R], the openness o = R - z with
// the hold boost Bh on the fully open samples, the (max, +) detector u = max(t, u - delta) (stage 1: u -> max(e, u - len delta)), yL on
// min(u, R), y = x 10^((yL - R) / 20)
struct Expander {
    using Coef = ExpCoef;
    using Acc = AccMinCount;
    using Lane = NoLane;
    using Front = Expander;
    struct Bufs { float *__restrict__ s1, *__restrict__ s2, *__restrict__ open, *__restrict__ cmin; int32_t* __restrict__ ccnt; };
    static constexpr const char* unit = "expander";
    static bool lane_null(const Bufs&) { return false; }
    static __host__ __device__ __forceinline__ Acc::Part part(const Bufs& b) { return {b.cmin, b.ccnt}; }
    static __device__ __forceinline__ Lane lane(const Bufs&, int64_t) { return {}; }
    static __device__ __forceinline__ float detect(const Coef& f, Lane&, float x, float u) { return expand_detect(f.delta, expand_open(f.T, f.S, f.K, f.R, f.Bh, x), u); }
    static __device__ __forceinline__ float drive(const Coef& f, float u) { return fminf(u, f.R); }
    static __device__ __forceinline__ float range(const Coef& f) { return f.R; }
    static __device__ __forceinline__ void tap(const Bufs& b, const Lane&, int64_t j, float yl) { if (b.open) b.open[j] = yl; }
    static __device__ __forceinline__ float apply(const Coef& f, const Lane&, float x, float yl) { return x * exp10f((yl - f.R) / 20.0f); }
};

// de-esser (section 21; include/stn.h "de-esser"): the band h = HP4(x), one section pass of the filter chain's 4-state system; the
// compressor's gain computer on the band's level, capped at the range; the compressor's detector and smoothing; the gain g =
// 10^(-yL / 20) on the band alone (split: y = x - (1 - g) h) or on the whole signal (wide: y = x g).  The detector listens to one signal
// and the gain lands on another.  h is regenerated in each pass from x and the chunk's band start state st[row][k] (s1 s2 t1 t2, one
// float4 per lane, formed by the loudness measurement's chunk pass and scan) and never stored: a pass is bound by its read of the rows,
// and a stored band would be one more write and three more reads of them.
struct DeessBufs { const float* __restrict__ st; float *__restrict__ s1, *__restrict__ s2, *__restrict__ band, *__restrict__ gr, *__restrict__ cmax; };
template <bool kSplit>
struct DeEsser {
    using Coef = DeessCoef;
    using Acc = AccMax;
    using Bufs = DeessBufs;
    using Front = DeEsser<true>;
    struct Lane { float b1, b2, b3, b4, h; };  // the band's state and its current sample
    static constexpr const char* unit = "deesser";
    static bool lane_null(const Bufs& b) { return !b.st; }
    static __host__ __device__ __forceinline__ Acc::Part part(const Bufs& b) { return {b.cmax}; }
    static __device__ __forceinline__ Lane lane(const Bufs& b, int64_t i) {
        const float4 v = reinterpret_cast<const float4*>(b.st)[i];
        return {v.x, v.y, v.z, v.w, 0.0f};
    }
    static __device__ __forceinline__ float detect(const Coef& f, Lane& l, float x, float y1) {
        l.h = biquad2_step(f.band, x, l.b1, l.b2, l.b3, l.b4);
        return gain_peak(f.kR, fminf(f.range, gain_want(f.T, f.S, f.K, l.h)), y1);
    }
    static __device__ __forceinline__ float drive(const Coef&, float y1) { return y1; }
    static __device__ __forceinline__ float range(const Coef&) { return 0.0f; }
    static __device__ __forceinline__ void tap(const Bufs& b, const Lane& l, int64_t j, float yl) {
        if (b.band) b.band[j] = l.h;
        if (b.gr) b.gr[j] = yl;
    }
    // split: only the band is turned down.  g == 1 (yL == 0) hands x on as it is: the fma would turn a -0.0 under a negative h into +0.0
    static __device__ __forceinline__ float apply(const Coef&, const Lane& l, float x, float yl) {
        const float g = exp10f(-yl / 20.0f);
        if (!kSplit) return x * g;
        return g == 1.0f ? x : __builtin_fmaf(-(1.0f - g), l.h, x);
    }
};

// kPass 1: s1[row][k] = d at the end of chunk k from d = 0.
// kPass 2: s1[row][k] = d at the start of chunk k (read) -> s2[row][k] = yL at its end from yL = 0.
// kPass 3: s1, s2 = both start values (read) -> y, the taps, and the accumulator over the chunk's samples below nrow[row] (null: W),
//          its start value when there are none.
// grid (ceil(W / DYN_SPAN), rows): every workgroup's span starts inside the row.  x and y may be the same rows, so neither is __restrict__.
template <class Stage, int kPass>
__global__ void __launch_bounds__(LO_WG) dyn_chunk_kernel(const float* x, float* y, int64_t W, int vec, int64_t Ks, typename Stage::Coef f,
                                                          const int64_t* __restrict__ nrow, typename Stage::Bufs b) {
    __shared__ float win[LO_WG * DYN_PAD];
    const int64_t row = blockIdx.y;
    const int64_t s0 = (int64_t)blockIdx.x * DYN_SPAN;
    const int cnt = (int)(W - s0 < DYN_SPAN ? W - s0 : DYN_SPAN);
    const float* xr = x + row * W + s0;
    chunk_stage_in<LO_WG, LO_CHUNK, false>(win, xr, cnt, vec);  // (W % 4 == 0 in the 16-byte form: so is cnt)
    __syncthreads();
    const int c0 = threadIdx.x * LO_CHUNK;
    if (c0 < cnt) {
        const int len = cnt - c0 < LO_CHUNK ? cnt - c0 : LO_CHUNK;
        const int64_t k = (int64_t)blockIdx.x * LO_WG + threadIdx.x;
        float* w = win + threadIdx.x * DYN_PAD;
        typename Stage::Lane lane = Stage::lane(b, row * Ks + k);
        if (kPass == 1) {
            float d = 0.0f;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i)
                if (i < len) d = Stage::detect(f, lane, w[i], d);
            b.s1[row * Ks + k] = d;
        } else if (kPass == 2) {
            float d = b.s1[row * Ks + k], yl = 0.0f;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i) {
                if (i < len) {
                    d = Stage::detect(f, lane, w[i], d);
                    yl = gain_smooth(f.kA, Stage::drive(f, d), yl);
                }
            }
            b.s2[row * Ks + k] = yl;
        } else {
            float d = b.s1[row * Ks + k], yl = b.s2[row * Ks + k];
            typename Stage::Acc acc = Stage::Acc::start(Stage::range(f));
            const int64_t g0 = s0 + c0;
            const int64_t n = nrow ? nrow[row] : W;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i) {
                if (i < len) {
                    const float u = w[i];
                    d = Stage::detect(f, lane, u, d);
                    yl = gain_smooth(f.kA, Stage::drive(f, d), yl);
                    if (g0 + i < n) acc.sample(Stage::range(f), yl);
                    Stage::tap(b, lane, row * W + g0 + i, yl);  // (the op-level probes only)
                    w[i] = Stage::apply(f, lane, u, yl);
                }
            }
            acc.store(Stage::part(b), row * Ks + k);
        }
    }
    if (kPass != 3) return;
    __syncthreads();
    float* yr = y + row * W + s0;
    chunk_stage_out<LO_WG, LO_CHUNK>(win, yr, cnt, vec);
}

// SCAN_MAX_TIMES: (D, b) . v = max(v, D o); SCAN_MAX_PLUS: (c, b) . v = max(v, o - c), the expander's detector (section 25);
// otherwise the linear v + E o
template <ScanComb kComb>
__device__ __forceinline__ double scan_comb(double P, double o, double v) {
    return kComb == SCAN_MAX_TIMES ? fmax(v, P * o) : kComb == SCAN_MAX_PLUS ? fmax(v, o - P) : v + P * o;
}

// st[row][k], K chunks per row: end values from zero in, start values out.  Tile t covers chunks t*LO_SCAN ..; after the inclusive
// Hillis-Steele scan lane i holds v_i = the composition of chunks t*LO_SCAN .. t*LO_SCAN + i applied to 0, so the start value of chunk
// t*LO_SCAN + i is v_{i-1} combined with P^i c, c the tile's carry-in.  pw[i] = P^(i+1), P = D or E of a whole chunk (only a row's last
// chunk can be short, and nothing starts behind it); for SCAN_MAX_PLUS pw[i] = (i + 1) c, what i + 1 whole chunks subtract.  In double;
// only the start values stored are fp32.  Lanes past K hold 0, the neutral value of all three families (every value is >= 0), so the
// order of the combinations is fixed by the chunk index, not by K.
template <ScanComb kComb>
__global__ void __launch_bounds__(LO_SCAN) chunk_scan_kernel(int64_t K, const double* __restrict__ pw, float* st) {
    __shared__ double buf[2][LO_SCAN];  // two images, written in turn: a level's readers are done before the level after next writes
    const int64_t row = blockIdx.x;
    const int i = threadIdx.x;
    float* sr = st + row * K;
    double c = 0.0;
    int p = 0;
    for (int64_t t0 = 0; t0 < K; t0 += LO_SCAN) {
        const int64_t k = t0 + i;
        double v = k < K ? (double)sr[k] : 0.0;
        for (int d = 1; d < LO_SCAN; d <<= 1) {
            buf[p][i] = v;
            __syncthreads();
            if (i >= d) v = scan_comb<kComb>(pw[d - 1], buf[p][i - d], v);
            p ^= 1;
        }
        buf[p][i] = v;
        __syncthreads();
        const double s = i == 0 ? c : scan_comb<kComb>(pw[i - 1], c, buf[p][i - 1]);
        if (k < K) sr[k] = (float)s;
        c = scan_comb<kComb>(pw[LO_SCAN - 1], c, buf[p][LO_SCAN - 1]);
        p ^= 1;
    }
}

// out[row] = the row's chunk accumulators part[row][0 .. K) joined (in no order that matters: see the accumulators)
template <class Acc>
__global__ void __launch_bounds__(DYN_ROWS) dyn_rows_kernel(int64_t K, float R, typename Acc::Part part, typename Acc::Out out) {
    __shared__ typename Acc::template Lds<DYN_ROWS> red;
    const int64_t r0 = (int64_t)blockIdx.x * K;
    Acc a = Acc::start(R);
    for (int64_t k = threadIdx.x; k < K; k += DYN_ROWS) a.join(Acc::load(part, r0 + k));
    a.put(red, threadIdx.x);
    __syncthreads();
    for (int d = DYN_ROWS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            a = Acc::get(red, threadIdx.x);
            a.join(Acc::get(red, threadIdx.x + d));
            a.put(red, threadIdx.x);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) Acc::get(red, 0).store(out, blockIdx.x);
}

// the guards and the dispatch of a stage's three passes; one staging form for the three: that of the rows read and written
template <class Stage>
void launch_dyn_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const typename Stage::Coef& f, float* y,
                       const typename Stage::Bufs& b) {
    if (rows <= 0 || W <= 0) return;
    chunk_shape(Stage::unit, rows, W);
    if (pass < 1 || pass > 3) throw std::invalid_argument(std::string(Stage::unit) + ": pass must be 1, 2 or 3");
    if (!x || !y || Stage::lane_null(b) || !b.s1 || (pass > 1 && !b.s2) || (pass == 3 && Stage::Acc::null(Stage::part(b))))
        throw std::invalid_argument(std::string(Stage::unit) + ": null buffer");
    const int vec = chunk_vec(x, y, W);
    const dim3 grid((unsigned)((W + DYN_SPAN - 1) / DYN_SPAN), (unsigned)rows);
    const int64_t Ks = lo_chunks(W);
    using Front = typename Stage::Front;
    if (pass == 1) STN_KLAUNCH((dyn_chunk_kernel<Front, 1>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, f, n, b);
    else if (pass == 2) STN_KLAUNCH((dyn_chunk_kernel<Front, 2>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, f, n, b);
    else STN_KLAUNCH((dyn_chunk_kernel<Stage, 3>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, f, n, b);
}

template <class Acc>
void launch_dyn_rows(hipStream_t s, const char* unit, int64_t rows, int64_t W, float R, typename Acc::Part part, typename Acc::Out out) {
    if (rows <= 0 || W <= 0) return;
    chunk_shape(unit, rows, W);
    STN_KLAUNCH(dyn_rows_kernel<Acc>, dim3((unsigned)rows), dim3(DYN_ROWS), 0, s, lo_chunks(W), R, part, out);
}

}  // namespace

void launch_compressor_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const CompTable& t, float* s1,
                              float* s2, float* y, float* gr, float* cmax) {
    launch_dyn_chunks<Compressor>(s, pass, x, rows, W, n, t.coef, y, {s1, s2, gr, cmax});
}

void launch_expander_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const ExpTable& t, float* s1,
                            float* s2, float* y, float* open, float* cmin, int32_t* ccnt) {
    launch_dyn_chunks<Expander>(s, pass, x, rows, W, n, t.coef, y, {s1, s2, open, cmin, ccnt});
}

void launch_deesser_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const DeessTable& t, const float* st,
                           float* s1, float* s2, float* y, float* band, float* gr, float* cmax) {
    if (t.split) launch_dyn_chunks<DeEsser<true>>(s, pass, x, rows, W, n, t.coef, y, {st, s1, s2, band, gr, cmax});
    else launch_dyn_chunks<DeEsser<false>>(s, pass, x, rows, W, n, t.coef, y, {st, s1, s2, band, gr, cmax});
}

void launch_chunk_scan(hipStream_t s, ScanComb comb, const char* unit, int64_t rows, int64_t W, const double* pw, float* st) {
    if (rows <= 0 || W <= 0) return;
    chunk_shape(unit, rows, W);
    if (!pw || !st) throw std::invalid_argument(std::string(unit) + ": scan without its table or states");
    const dim3 grid((unsigned)rows), wg(LO_SCAN);
    if (comb == SCAN_MAX_TIMES) STN_KLAUNCH(chunk_scan_kernel<SCAN_MAX_TIMES>, grid, wg, 0, s, lo_chunks(W), pw, st);
    else if (comb == SCAN_MAX_PLUS) STN_KLAUNCH(chunk_scan_kernel<SCAN_MAX_PLUS>, grid, wg, 0, s, lo_chunks(W), pw, st);
    else STN_KLAUNCH(chunk_scan_kernel<SCAN_LINEAR>, grid, wg, 0, s, lo_chunks(W), pw, st);
}

void launch_compressor_rowmax(hipStream_t s, int64_t rows, int64_t W, const float* cmax, float* out) {
    launch_dyn_rows<AccMax>(s, "compressor", rows, W, 0.0f, {const_cast<float*>(cmax)}, {out});
}

void launch_expander_rows(hipStream_t s, int64_t rows, int64_t W, const ExpTable& t, const float* cmin, const int32_t* ccnt, float* omin, int64_t* ocnt) {
    launch_dyn_rows<AccMinCount>(s, "expander", rows, W, t.coef.R, {const_cast<float*>(cmin), const_cast<int32_t*>(ccnt)}, {omin, ocnt});
}

}  // namespace stn
