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
// and stores after the second).  ds_step restates fl_step (kernels_filter.hip) and ds_want / ds_peak / ds_smooth restate cp_want /
// cp_peak / cp_smooth (kernels_compressor.hip) operation for operation: the start states the scans form are exact for that arithmetic
// only, and those two units stay as they are.
// A row's y[0 .. n) depends on x[0 .. n) of that row and the coefficients only: the scans' order is fixed by the chunk index.
#include "kernels.hpp"

#include <math.h>

namespace stn {

namespace {

constexpr int DS_SPAN = LO_WG * LO_CHUNK;  // samples a workgroup owns
constexpr int DS_PAD = LO_CHUNK + 1;       // LDS words per chunk: the lanes' walks fall on distinct banks

// one sample through the band's two sections: fl_step
__device__ __forceinline__ float ds_step(const LoudCoef& f, float u, float& s1, float& s2, float& t1, float& t2) {
    const float v = __builtin_fmaf(f.c[0], u, s1);
    s1 = __builtin_fmaf(-f.c[3], v, __builtin_fmaf(f.c[1], u, s2));
    s2 = __builtin_fmaf(-f.c[4], v, f.c[2] * u);
    const float y = __builtin_fmaf(f.c[5], v, t1);
    t1 = __builtin_fmaf(-f.c[8], y, __builtin_fmaf(f.c[6], v, t2));
    t2 = __builtin_fmaf(-f.c[9], y, f.c[7] * v);
    return y;
}
// the gain computer on the band's level: cp_want, then the range cap
__device__ __forceinline__ float ds_want(const DeessCoef& f, float h) {
    const float xg = 20.0f * log10f(fmaxf(fabsf(h), 1e-6f));
    const float d = xg - f.T;
    const float d2 = 2.0f * d;
    float z;
    if (d2 < -f.K) z = 0.0f;
    else if (f.K > 0.0f && fabsf(d2) <= f.K) {
        const float t = d + 0.5f * f.K;
        z = (-f.S * (t * t)) / (2.0f * f.K);
    } else z = -f.S * d;
    return fminf(f.range, z);
}
__device__ __forceinline__ float ds_peak(const DeessCoef& f, float z, float y1) { return fmaxf(z, __builtin_fmaf(-f.kR, y1, y1)); }
__device__ __forceinline__ float ds_smooth(const DeessCoef& f, float y1, float yl) { return __builtin_fmaf(f.kA, y1 - yl, yl); }
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
    constexpr int U = DS_SPAN / 4 / LO_WG;
    if (vec) {  // rows 16-byte aligned and W % 4 == 0: cnt % 4 == 0, a float4 that starts below cnt ends at or below it
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = threadIdx.x + u * LO_WG;
            if (4 * q < cnt) v[u] = reinterpret_cast<const float4*>(xr)[q];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = 4 * (threadIdx.x + u * LO_WG);
            if (i < cnt) {
                float* d = win + (i / LO_CHUNK) * DS_PAD + (i % LO_CHUNK);  // (the four samples share a chunk)
                d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
            }
        }
    } else {
        for (int i0 = 0; i0 < DS_SPAN; i0 += 8 * LO_WG) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + threadIdx.x + u * LO_WG;
                v[u] = i < cnt ? xr[i] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + threadIdx.x + u * LO_WG;
                if (i < cnt) win[(i / LO_CHUNK) * DS_PAD + (i % LO_CHUNK)] = v[u];
            }
        }
    }
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
                if (i < len) y1 = ds_peak(f, ds_want(f, ds_step(f.band, w[i], b1, b2, b3, b4)), y1);
            s1[row * Ks + k] = y1;
        } else if (kPass == 2) {
            float y1 = s1[row * Ks + k], yl = 0.0f;
#pragma unroll
            for (int i = 0; i < LO_CHUNK; ++i) {
                if (i < len) {
                    y1 = ds_peak(f, ds_want(f, ds_step(f.band, w[i], b1, b2, b3, b4)), y1);
                    yl = ds_smooth(f, y1, yl);
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
                    const float h = ds_step(f.band, u, b1, b2, b3, b4);
                    y1 = ds_peak(f, ds_want(f, h), y1);
                    yl = ds_smooth(f, y1, yl);
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
    if (vec) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = threadIdx.x + u * LO_WG, i = 4 * q;
            if (i < cnt) {
                const float* d = win + (i / LO_CHUNK) * DS_PAD + (i % LO_CHUNK);
                reinterpret_cast<float4*>(yr)[q] = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += LO_WG) yr[i] = win[(i / LO_CHUNK) * DS_PAD + (i % LO_CHUNK)];
    }
}

bool ds_aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace

const char* deesser_staging_form(const float* x, const float* y, int64_t W) {
    return W % 4 == 0 && ds_aligned16(x) && ds_aligned16(y) ? "vec" : "scalar";
}

void launch_deesser_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const DeessTable& t, const float* st,
                           float* s1, float* s2, float* y, float* band, float* gr, float* cmax) {
    if (rows <= 0 || W <= 0) return;
    if (rows > 65535) throw std::invalid_argument("deesser: more than 65535 rows");
    if (lo_chunks(W) > ((int64_t)1 << 31) / LO_WG) throw std::invalid_argument("deesser: row too long");
    if (pass < 1 || pass > 3) throw std::invalid_argument("deesser: pass must be 1, 2 or 3");
    if (!x || !y || !st || !s1 || (pass > 1 && !s2) || (pass == 3 && !cmax)) throw std::invalid_argument("deesser: null buffer");
    const int vec = deesser_staging_form(x, y, W)[0] == 'v' ? 1 : 0;  // (one form for the three passes: that of the rows read and written)
    const dim3 grid((unsigned)((W + DS_SPAN - 1) / DS_SPAN), (unsigned)rows);
    const int64_t Ks = lo_chunks(W);
    if (pass == 1) STN_KLAUNCH((deesser_chunk_kernel<1, true>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, st, s1, s2, band, gr, cmax);
    else if (pass == 2) STN_KLAUNCH((deesser_chunk_kernel<2, true>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, st, s1, s2, band, gr, cmax);
    else if (t.split) STN_KLAUNCH((deesser_chunk_kernel<3, true>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, st, s1, s2, band, gr, cmax);
    else STN_KLAUNCH((deesser_chunk_kernel<3, false>), grid, dim3(LO_WG), 0, s, x, y, W, vec, Ks, t.coef, n, st, s1, s2, band, gr, cmax);
}

}  // namespace stn
