// kernels_compressor.hip — the fetch-time dynamic range compressor (gfx950, wave64).
//
// Per row and sample, in fp32 (include/stn.h "compressor"): the level xG in dB, the gain computer's wanted reduction z >= 0, the
// decoupled peak detector y1 = max(z, y1 - kR y1), its smoothing yL = yL + kA (y1 - yL), and y = x 10^((makeup - yL) / 20).
// Neither recurrence is the 4-state linear system of the filter chain, but both compose over a chunk of len samples:
//   stage 1  y1 -> max(e, D y1)   D = (1 - kR)^len, e the chunk's end value from y1 = 0   (max and a positive factor commute)
//   stage 2  yL -> E yL + c       E = (1 - kA)^len, c the chunk's end value from yL = 0, driven by the TRUE y1 inside the chunk
// so c exists only after stage 1's start states do.  Five launches, every hand-off a launch boundary, no atomics:
//   1. chunk pass 1: z, and y1 from zero -> e_k              2. scan 1 (max, x) in double -> y1 at every chunk's start
//   3. chunk pass 2: y1 from its start, yL from zero -> c_k  4. scan 2 (+, x) in double -> yL at every chunk's start
//   5. write pass: both stages from their start states -> y, optionally yL, and the chunk's max of yL over the row's valid samples
// and a sixth, small one: the row maxima of those chunk maxima (stn_batch_compressor).
// Chunks are LO_CHUNK samples counted from sample 0, a workgroup stages LO_WG of them through LDS as filter_write_kernel does
// (chunk_stage_in / chunk_stage_out, kernels_chunk.hpp: 16-byte loads and stores or the scalar form, row stride 33 words), and every
// pass calls the same gain_want, gain_peak and gain_smooth (the same header): the start states the scans form are exact for this
// arithmetic only.
// In place (y == x) is allowed: a workgroup reads the samples it owns into LDS before the first barrier and stores after the second.
// A row's y[0 .. n) depends on x[0 .. n) of that row and the coefficients only: the scans' order is fixed by the chunk index.
#include "kernels_chunk.hpp"

#include <math.h>

namespace stn {

namespace {

constexpr int CP_SPAN = LO_WG * LO_CHUNK;  // samples a workgroup owns
constexpr int CP_PAD = LO_CHUNK + 1;       // LDS words per chunk: the lanes' walks fall on distinct banks
constexpr int CP_ROWMAX = 256;             // threads of the row-maximum workgroup

__device__ __forceinline__ float cp_apply(const CompCoef& f, float x, float yl) { return x * exp10f((f.makeup - yl) / 20.0f); }

// kPass 1: s1[row][k] = y1 at the end of chunk k from y1 = 0.
// kPass 2: s1[row][k] = y1 at the start of chunk k (read) -> s2[row][k] = yL at its end from yL = 0.
// kPass 3: s1, s2 = both start values (read) -> y, gr (or null: yL per sample), cmax[row][k] = max of yL over the chunk's samples
//          below nrow[row] (null: W), 0 when there are none.
// grid (ceil(W / CP_SPAN), rows): every workgroup's span starts inside the row.  x and y may be the same rows, so neither is __restrict__.
template <int kPass>
__global__ void __launch_bounds__(LO_WG) compressor_chunk_kernel(const float* x, float* y, int64_t W, int vec, int64_t Ks, CompCoef f,
                                                                 const int64_t* __restrict__ nrow, float* __restrict__ s1, float* __restrict__ s2,
                                                                 float* __restrict__ gr, float* __restrict__ cmax) {
    __shared__ float win[LO_WG * CP_PAD];
    const int64_t row = blockIdx.y;
    const int64_t s0 = (int64_t)blockIdx.x * CP_SPAN;
    const int cnt = (int)(W - s0 < CP_SPAN ? W - s0 : CP_SPAN);
    const float* xr = x + row * W + s0;
    chunk_stage_in<LO_WG, LO_CHUNK, false>(win, xr, cnt, vec);  // (W % 4 == 0 in the 16-byte form: so is cnt)
    __syncthreads();
    const int c0 = threadIdx.x * LO_CHUNK;
    if (c0 < cnt) {
        const int len = cnt - c0 < LO_CHUNK ? cnt - c0 : LO_CHUNK;
        const int64_t k = (int64_t)blockIdx.x * LO_WG + threadIdx.x;
        float* w = win + threadIdx.x * CP_PAD;
        if (kPass == 1) {
            float y1 = 0.0f;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i)
                if (i < len) y1 = gain_peak(f.kR, gain_want(f.T, f.S, f.K, w[i]), y1);
            s1[row * Ks + k] = y1;
        } else if (kPass == 2) {
            float y1 = s1[row * Ks + k], yl = 0.0f;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i) {
                if (i < len) {
                    y1 = gain_peak(f.kR, gain_want(f.T, f.S, f.K, w[i]), y1);
                    yl = gain_smooth(f.kA, y1, yl);
                }
            }
            s2[row * Ks + k] = yl;
        } else {
            float y1 = s1[row * Ks + k], yl = s2[row * Ks + k], m = 0.0f;
            const int64_t g0 = s0 + c0;
            const int64_t n = nrow ? nrow[row] : W;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i) {
                if (i < len) {
                    const float u = w[i];
                    y1 = gain_peak(f.kR, gain_want(f.T, f.S, f.K, u), y1);
                    yl = gain_smooth(f.kA, y1, yl);
                    if (g0 + i < n) m = fmaxf(m, yl);
                    if (gr) gr[row * W + g0 + i] = yl;  // (the op-level probe only: a fetch passes null)
                    w[i] = cp_apply(f, u, yl);
                }
            }
            cmax[row * Ks + k] = m;
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
__device__ __forceinline__ double cp_comb(double P, double o, double v) {
    return kComb == SCAN_MAX_TIMES ? fmax(v, P * o) : kComb == SCAN_MAX_PLUS ? fmax(v, o - P) : v + P * o;
}

// st[row][k], K chunks per row: end values from zero in, start values out.  Tile t covers chunks t*LO_SCAN ..; after the inclusive
// Hillis-Steele scan lane i holds v_i = the composition of chunks t*LO_SCAN .. t*LO_SCAN + i applied to 0, so the start value of chunk
// t*LO_SCAN + i is v_{i-1} combined with P^i c, c the tile's carry-in.  pw[i] = P^(i+1), P = D or E of a whole chunk (only a row's last
// chunk can be short, and nothing starts behind it); for SCAN_MAX_PLUS pw[i] = (i + 1) c, what i + 1 whole chunks subtract.  In double;
// only the start values stored are fp32.  Lanes past K hold 0, the neutral value of all three families (every value is >= 0), so the
// order of the combinations is fixed by the chunk index, not by K.
template <ScanComb kComb>
__global__ void __launch_bounds__(LO_SCAN) compressor_scan_kernel(int64_t K, const double* __restrict__ pw, float* st) {
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
            if (i >= d) v = cp_comb<kComb>(pw[d - 1], buf[p][i - d], v);
            p ^= 1;
        }
        buf[p][i] = v;
        __syncthreads();
        const double s = i == 0 ? c : cp_comb<kComb>(pw[i - 1], c, buf[p][i - 1]);
        if (k < K) sr[k] = (float)s;
        c = cp_comb<kComb>(pw[LO_SCAN - 1], c, buf[p][LO_SCAN - 1]);
        p ^= 1;
    }
}

// out[row] = max over the row's chunk maxima (a maximum of floats does not depend on the order it is taken in)
__global__ void __launch_bounds__(CP_ROWMAX) compressor_rowmax_kernel(int64_t K, const float* __restrict__ cmax, float* __restrict__ out) {
    __shared__ float red[CP_ROWMAX];
    const float* cr = cmax + (int64_t)blockIdx.x * K;
    float m = 0.0f;
    for (int64_t k = threadIdx.x; k < K; k += CP_ROWMAX) m = fmaxf(m, cr[k]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int d = CP_ROWMAX / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

}  // namespace

const char* compressor_staging_form(const float* x, const float* y, int64_t W) { return chunk_vec(x, y, W) ? "vec" : "scalar"; }

void launch_compressor_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const CompTable& t, float* s1,
                              float* s2, float* y, float* gr, float* cmax) {
    if (rows <= 0 || W <= 0) return;
    chunk_shape("compressor", rows, W);
    if (pass < 1 || pass > 3) throw std::invalid_argument("compressor: pass must be 1, 2 or 3");
    if (!x || !y || !s1 || (pass > 1 && !s2) || (pass == 3 && !cmax)) throw std::invalid_argument("compressor: null buffer");
    const int vec = chunk_vec(x, y, W);  // (one form for the three passes: that of the rows read and written)
    const dim3 grid((unsigned)((W + CP_SPAN - 1) / CP_SPAN), (unsigned)rows);
    const int64_t Ks = lo_chunks(W);
    if (pass == 1) STN_KLAUNCH(compressor_chunk_kernel<1>, grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, s1, s2, gr, cmax);
    else if (pass == 2) STN_KLAUNCH(compressor_chunk_kernel<2>, grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, s1, s2, gr, cmax);
    else STN_KLAUNCH(compressor_chunk_kernel<3>, grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, s1, s2, gr, cmax);
}

void launch_chunk_scan(hipStream_t s, ScanComb comb, const char* unit, int64_t rows, int64_t W, const double* pw, float* st) {
    if (rows <= 0 || W <= 0) return;
    chunk_shape(unit, rows, W);
    if (!pw || !st) throw std::invalid_argument(std::string(unit) + ": scan without its table or states");
    const dim3 grid((unsigned)rows), wg(LO_SCAN);
    if (comb == SCAN_MAX_TIMES) STN_KLAUNCH(compressor_scan_kernel<SCAN_MAX_TIMES>, grid, wg, 0, s, lo_chunks(W), pw, st);
    else if (comb == SCAN_MAX_PLUS) STN_KLAUNCH(compressor_scan_kernel<SCAN_MAX_PLUS>, grid, wg, 0, s, lo_chunks(W), pw, st);
    else STN_KLAUNCH(compressor_scan_kernel<SCAN_LINEAR>, grid, wg, 0, s, lo_chunks(W), pw, st);
}

void launch_compressor_scan(hipStream_t s, int stage, int64_t rows, int64_t W, const CompTable& t, float* st) {
    if (rows <= 0 || W <= 0) return;
    if (!t.dev || !st) throw std::invalid_argument("compressor: scan without its table or states");
    if (stage == 1) launch_chunk_scan(s, SCAN_MAX_TIMES, "compressor", rows, W, t.dev, st);
    else launch_chunk_scan(s, SCAN_LINEAR, "compressor", rows, W, t.dev + LO_SCAN, st);
}

void launch_compressor_rowmax(hipStream_t s, int64_t rows, int64_t W, const float* cmax, float* out) {
    if (rows <= 0 || W <= 0) return;
    chunk_shape("compressor", rows, W);
    STN_KLAUNCH(compressor_rowmax_kernel, dim3((unsigned)rows), dim3(CP_ROWMAX), 0, s, lo_chunks(W), cmax, out);
}

}  // namespace stn
