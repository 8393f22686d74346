// kernels_deesser.hip — the chunk passes of the fetch-time de-esser (gfx950, wave64).
//
// Per row and sample, in fp32 (include/stn.h "de-esser"): the band h = HP4(x), a 4th-order Butterworth high-pass run as ONE section pass
// of the filter chain's 4-state system; the band's level in dB; the compressor's gain computer on that level, capped at range_db; the
// compressor's decoupled peak detector and smoothing (y1, yL); and the gain g = 10^(-yL / 20) applied to the band alone (split:
// y = x - (1 - g) h) or to the whole signal (wide: y = x g).  The detector listens to one signal and the gain lands on another, which
// is what neither the chain (linear) nor the compressor (one signal) can express.
// The three recurrences compose over chunks exactly as sections 18 and 20 say, so the sequence is theirs, launch for launch:
//   1. the band's chunk pass from zero state (launch_loudness_chunks)     2. its scan in double (launch_loudness_scan) -> st
//   3. pass 1 below: h from st, z, y1 from zero -> e_k                    4. the (max, x) scan (launch_compressor_scan 1) -> s1
//   5. pass 2 below: h, y1 from s1, yL from zero -> c_k                   6. the linear scan (launch_compressor_scan 2) -> s2
//   7. pass 3 below: everything from its start state -> y, the chunk's maximum of yL over the row's valid samples, the probes
//   8. the row maxima (launch_compressor_rowmax)
// h is regenerated in each of the three passes from x and the chunk's band start state (one float4 per lane) and never stored: a pass
// is bound by its read of the rows, and a stored band would be one more write and three more reads of them.
// Geometry and staging are compressor_chunk_kernel's: LO_WG chunks of LO_CHUNK samples through LDS at a row stride of 33 words, 16-byte
// loads and stores or the scalar form by (x, y, W), in place allowed (a workgroup reads the samples it owns before the first barrier
// and stores after the second).  The band's step is the filter chain's biquad2_step and the detector's steps are the compressor's
// gain_want / gain_peak / gain_smooth (kernels_chunk.hpp, one definition each): the start states the scans form are exact for that
// arithmetic only.
// A row's y[0 .. n) depends on x[0 .. n) of that row and the coefficients only: the scans' order is fixed by the chunk index.
#include "kernels_chunk.hpp"

#include <math.h>

namespace stn {

namespace {

constexpr int DS_SPAN = LO_WG * LO_CHUNK;  // samples a workgroup owns
constexpr int DS_PAD = LO_CHUNK + 1;       // LDS words per chunk: the lanes' walks fall on distinct banks

// the gain computer on the band's level, capped at the range
__device__ __forceinline__ float ds_want(const DeessCoef& f, float h) { return fminf(f.range, gain_want(f.T, f.S, f.K, h)); }
// split: only the band is turned down.  g == 1 (yL == 0) hands x on as it is: the fma would turn a -0.0 under a negative h into +0.0
template <bool kSplit>
__device__ __forceinline__ float ds_apply(float x, float h, float yl) {
    const float g = exp10f(-yl / 20.0f);
    if (!kSplit) return x * g;
    return g == 1.0f ? x : __builtin_fmaf(-(1.0f - g), h, x);
}

// st[row][k]: the band's state (s1 s2 t1 t2) at the start of chunk k (read by every pass).
// kPass 1: s1[row][k] = y1 at the end of chunk k from y1 = 0.
// kPass 2: s1[row][k] = y1 at the start of chunk k (read) -> s2[row][k] = yL at its end from yL = 0.
// kPass 3: s1, s2 = both start values (read) -> y, band and gr (each or null: h and yL per sample), cmax[row][k] = max of yL over the
//          chunk's samples below nrow[row] (null: W), 0 when there are none.
// grid (ceil(W / DS_SPAN), rows): every workgroup's span starts inside the row.  x and y may be the same rows, so neither is __restrict__.
template <int kPass, bool kSplit>
__global__ void __launch_bounds__(LO_WG) deesser_chunk_kernel(const float* x, float* y, int64_t W, int vec, int64_t Ks, DeessCoef f,
                                                              const int64_t* __restrict__ nrow, const float* __restrict__ st,
                                                              float* __restrict__ s1, float* __restrict__ s2, float* __restrict__ band,
                                                              float* __restrict__ gr, float* __restrict__ cmax) {
    __shared__ float win[LO_WG * DS_PAD];
    const int64_t row = blockIdx.y;
    const int64_t s0 = (int64_t)blockIdx.x * DS_SPAN;
    const int cnt = (int)(W - s0 < DS_SPAN ? W - s0 : DS_SPAN);
    const float* xr = x + row * W + s0;
    chunk_stage_in<LO_WG, LO_CHUNK, false>(win, xr, cnt, vec);  // (W % 4 == 0 in the 16-byte form: so is cnt)
    __syncthreads();
    const int c0 = threadIdx.x * LO_CHUNK;
    if (c0 < cnt) {
        const int len = cnt - c0 < LO_CHUNK ? cnt - c0 : LO_CHUNK;
        const int64_t k = (int64_t)blockIdx.x * LO_WG + threadIdx.x;
        float* w = win + threadIdx.x * DS_PAD;
        const float4 b = reinterpret_cast<const float4*>(st)[row * Ks + k];
        float b1 = b.x, b2 = b.y, b3 = b.z, b4 = b.w;
        if (kPass == 1) {
            float y1 = 0.0f;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i)
                if (i < len) y1 = gain_peak(f.kR, ds_want(f, biquad2_step(f.band, w[i], b1, b2, b3, b4)), y1);
            s1[row * Ks + k] = y1;
        } else if (kPass == 2) {
            float y1 = s1[row * Ks + k], yl = 0.0f;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i) {
                if (i < len) {
                    y1 = gain_peak(f.kR, ds_want(f, biquad2_step(f.band, w[i], b1, b2, b3, b4)), y1);
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
                    const float h = biquad2_step(f.band, u, b1, b2, b3, b4);
                    y1 = gain_peak(f.kR, ds_want(f, h), y1);
                    yl = gain_smooth(f.kA, y1, yl);
                    if (g0 + i < n) m = fmaxf(m, yl);
                    if (band) band[row * W + g0 + i] = h;  // (the op-level probes only: a fetch passes null for both)
                    if (gr) gr[row * W + g0 + i] = yl;
                    w[i] = ds_apply<kSplit>(u, h, yl);
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

}  // namespace

const char* deesser_staging_form(const float* x, const float* y, int64_t W) { return chunk_vec(x, y, W) ? "vec" : "scalar"; }

void launch_deesser_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const DeessTable& t, const float* st,
                           float* s1, float* s2, float* y, float* band, float* gr, float* cmax) {
    if (rows <= 0 || W <= 0) return;
    chunk_shape("deesser", rows, W);
    if (pass < 1 || pass > 3) throw std::invalid_argument("deesser: pass must be 1, 2 or 3");
    if (!x || !y || !st || !s1 || (pass > 1 && !s2) || (pass == 3 && !cmax)) throw std::invalid_argument("deesser: null buffer");
    const int vec = chunk_vec(x, y, W);  // (one form for the three passes: that of the rows read and written)
    const dim3 grid((unsigned)((W + DS_SPAN - 1) / DS_SPAN), (unsigned)rows);
    const int64_t Ks = lo_chunks(W);
    if (pass == 1) STN_KLAUNCH((deesser_chunk_kernel<1, true>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, st, s1, s2, band, gr, cmax);
    else if (pass == 2) STN_KLAUNCH((deesser_chunk_kernel<2, true>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, st, s1, s2, band, gr, cmax);
    else if (t.split) STN_KLAUNCH((deesser_chunk_kernel<3, true>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, st, s1, s2, band, gr, cmax);
    else STN_KLAUNCH((deesser_chunk_kernel<3, false>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, st, s1, s2, band, gr, cmax);
}

}  // namespace stn
