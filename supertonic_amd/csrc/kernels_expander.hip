// kernels_expander.hip — the fetch-time downward expander / noise gate (gfx950, wave64).
//
// Per row and sample, in fp32 (include/stn.h "expander"): the level xG in dB, the gain computer's wanted attenuation z in [0, R], the
// openness o = R - z with the hold boost Bh on the fully open samples, the (max, +) detector u = max(t, u - delta), y1 = min(u, R), its
// smoothing yL = yL + kA (y1 - yL), and y = x 10^((yL - R) / 20).  Both recurrences compose over a chunk of len samples:
//   stage 1  u  -> max(e, u - len delta)   e the chunk's end value from u = 0          (max and a subtraction commute)
//   stage 2  yL -> E yL + c                E = (1 - kA)^len, c the chunk's end value from yL = 0, driven by the TRUE u inside the chunk
// The launches are the compressor's (kernels_compressor.hip), every hand-off a launch boundary, no atomics:
//   1. chunk pass 1: t, and u from zero -> e_k               2. scan 1 (max, +) in double -> u at every chunk's start
//   3. chunk pass 2: u from its start, yL from zero -> c_k   4. scan 2 (+, x) in double -> yL at every chunk's start
//   5. write pass: both stages from their start states -> y, optionally yL, and per chunk the minimum of R - yL and the count of
//      yL <= R / 2 over the row's valid samples
//   6. the row's minimum and count (stn_batch_expander).
// Chunks are LO_CHUNK samples counted from sample 0, a workgroup stages LO_WG of them through LDS (chunk_stage_in / chunk_stage_out,
// kernels_chunk.hpp), and every pass calls the same expand_open, expand_detect and gain_smooth (the same header): the start states the
// scans form are exact for this arithmetic only.  In place (y == x) is allowed: a workgroup reads the samples it owns into LDS before
// the first barrier and stores after the second.  A row's y[0 .. n) depends on x[0 .. n) of that row and the coefficients only.
#include "kernels_chunk.hpp"

#include <math.h>

namespace stn {

namespace {

constexpr int XP_SPAN = LO_WG * LO_CHUNK;  // samples a workgroup owns
constexpr int XP_PAD = LO_CHUNK + 1;       // LDS words per chunk: the lanes' walks fall on distinct banks
constexpr int XP_ROWS = 256;               // threads of the per-row reduction

__device__ __forceinline__ float xp_apply(const ExpCoef& f, float x, float yl) { return x * exp10f((yl - f.R) / 20.0f); }

// kPass 1: s1[row][k] = u at the end of chunk k from u = 0.
// kPass 2: s1[row][k] = u at the start of chunk k (read) -> s2[row][k] = yL at its end from yL = 0.
// kPass 3: s1, s2 = both start values (read) -> y, open (or null: yL per sample), cmin[row][k] = min of R - yL and ccnt[row][k] = count of
//          yL <= R / 2 over the chunk's samples below nrow[row] (null: W); R and 0 when there are none.
// grid (ceil(W / XP_SPAN), rows): every workgroup's span starts inside the row.  x and y may be the same rows, so neither is __restrict__.
template <int kPass>
__global__ void __launch_bounds__(LO_WG) expander_chunk_kernel(const float* x, float* y, int64_t W, int vec, int64_t Ks, ExpCoef f,
                                                               const int64_t* __restrict__ nrow, float* __restrict__ s1, float* __restrict__ s2,
                                                               float* __restrict__ open, float* __restrict__ cmin, int32_t* __restrict__ ccnt) {
    __shared__ float win[LO_WG * XP_PAD];
    const int64_t row = blockIdx.y;
    const int64_t s0 = (int64_t)blockIdx.x * XP_SPAN;
    const int cnt = (int)(W - s0 < XP_SPAN ? W - s0 : XP_SPAN);
    const float* xr = x + row * W + s0;
    chunk_stage_in<LO_WG, LO_CHUNK, false>(win, xr, cnt, vec);  // (W % 4 == 0 in the 16-byte form: so is cnt)
    __syncthreads();
    const int c0 = threadIdx.x * LO_CHUNK;
    if (c0 < cnt) {
        const int len = cnt - c0 < LO_CHUNK ? cnt - c0 : LO_CHUNK;
        const int64_t k = (int64_t)blockIdx.x * LO_WG + threadIdx.x;
        float* w = win + threadIdx.x * XP_PAD;
        if (kPass == 1) {
            float u = 0.0f;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i)
                if (i < len) u = expand_detect(f.delta, expand_open(f.T, f.S, f.K, f.R, f.Bh, w[i]), u);
            s1[row * Ks + k] = u;
        } else if (kPass == 2) {
            float u = s1[row * Ks + k], yl = 0.0f;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i) {
                if (i < len) {
                    u = expand_detect(f.delta, expand_open(f.T, f.S, f.K, f.R, f.Bh, w[i]), u);
                    yl = gain_smooth(f.kA, fminf(u, f.R), yl);
                }
            }
            s2[row * Ks + k] = yl;
        } else {
            float u = s1[row * Ks + k], yl = s2[row * Ks + k], m = f.R;
            int32_t closed = 0;
            const float half = 0.5f * f.R;
            const int64_t g0 = s0 + c0;
            const int64_t n = nrow ? nrow[row] : W;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i) {
                if (i < len) {
                    const float v = w[i];
                    u = expand_detect(f.delta, expand_open(f.T, f.S, f.K, f.R, f.Bh, v), u);
                    yl = gain_smooth(f.kA, fminf(u, f.R), yl);
                    if (g0 + i < n) {
                        m = fminf(m, f.R - yl);
                        closed += yl <= half ? 1 : 0;
                    }
                    if (open) open[row * W + g0 + i] = yl;  // (the op-level probe only: a fetch passes null)
                    w[i] = xp_apply(f, v, yl);
                }
            }
            cmin[row * Ks + k] = m;
            ccnt[row * Ks + k] = closed;
        }
    }
    if (kPass != 3) return;
    __syncthreads();
    float* yr = y + row * W + s0;
    chunk_stage_out<LO_WG, LO_CHUNK>(win, yr, cnt, vec);
}

// omin[row] = min over the row's chunk minima, ocnt[row] = the sum of its chunk counts (a minimum of floats and a sum of integers do
// not depend on the order they are taken in)
__global__ void __launch_bounds__(XP_ROWS) expander_rows_kernel(int64_t K, float R, const float* __restrict__ cmin, const int32_t* __restrict__ ccnt,
                                                                float* __restrict__ omin, int64_t* __restrict__ ocnt) {
    __shared__ float rmin[XP_ROWS];
    __shared__ int64_t rcnt[XP_ROWS];
    const float* mr = cmin + (int64_t)blockIdx.x * K;
    const int32_t* cr = ccnt + (int64_t)blockIdx.x * K;
    float m = R;
    int64_t c = 0;
    for (int64_t k = threadIdx.x; k < K; k += XP_ROWS) {
        m = fminf(m, mr[k]);
        c += cr[k];
    }
    rmin[threadIdx.x] = m;
    rcnt[threadIdx.x] = c;
    __syncthreads();
    for (int d = XP_ROWS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            rmin[threadIdx.x] = fminf(rmin[threadIdx.x], rmin[threadIdx.x + d]);
            rcnt[threadIdx.x] += rcnt[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        omin[blockIdx.x] = rmin[0];
        ocnt[blockIdx.x] = rcnt[0];
    }
}

}  // namespace

const char* expander_staging_form(const float* x, const float* y, int64_t W) { return chunk_vec(x, y, W) ? "vec" : "scalar"; }

void launch_expander_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const ExpTable& t, float* s1,
                            float* s2, float* y, float* open, float* cmin, int32_t* ccnt) {
    if (rows <= 0 || W <= 0) return;
    chunk_shape("expander", rows, W);
    if (pass < 1 || pass > 3) throw std::invalid_argument("expander: pass must be 1, 2 or 3");
    if (!x || !y || !s1 || (pass > 1 && !s2) || (pass == 3 && (!cmin || !ccnt))) throw std::invalid_argument("expander: null buffer");
    const int vec = chunk_vec(x, y, W);  // (one form for the three passes: that of the rows read and written)
    const dim3 grid((unsigned)((W + XP_SPAN - 1) / XP_SPAN), (unsigned)rows);
    const int64_t Ks = lo_chunks(W);
    if (pass == 1) STN_KLAUNCH(expander_chunk_kernel<1>, grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, s1, s2, open, cmin, ccnt);
    else if (pass == 2) STN_KLAUNCH(expander_chunk_kernel<2>, grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, s1, s2, open, cmin, ccnt);
    else STN_KLAUNCH(expander_chunk_kernel<3>, grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, s1, s2, open, cmin, ccnt);
}

void launch_expander_scan(hipStream_t s, int stage, int64_t rows, int64_t W, const ExpTable& t, float* st) {
    if (rows <= 0 || W <= 0) return;
    if (!t.dev || !st) throw std::invalid_argument("expander: scan without its table or states");
    if (stage == 1) launch_chunk_scan(s, SCAN_MAX_PLUS, "expander", rows, W, t.dev, st);
    else launch_chunk_scan(s, SCAN_LINEAR, "expander", rows, W, t.dev + LO_SCAN, st);
}

void launch_expander_rows(hipStream_t s, int64_t rows, int64_t W, const ExpTable& t, const float* cmin, const int32_t* ccnt, float* omin, int64_t* ocnt) {
    if (rows <= 0 || W <= 0) return;
    chunk_shape("expander", rows, W);
    STN_KLAUNCH(expander_rows_kernel, dim3((unsigned)rows), dim3(XP_ROWS), 0, s, lo_chunks(W), t.coef.R, cmin, ccnt, omin, ocnt);
}

}  // namespace stn
