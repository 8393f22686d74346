// kernels_limiter.hip — look-ahead peak limiter behind the loudness gain (gfx950, wave64).  Runs at fetch time,
// outside the captured pipeline, on rows x W fp32 samples of which row b's first n_b count.
//
// Per sample of a row, with v = x * g_b, r = 1 where |v| <= c and c / |v| elsewhere (1 outside [0, n_b)), A the look-ahead in samples:
//   m[i] = min r[i .. i+A],  M[i] = min(m[i-A], m[i]),  s[i] = 1 where M[i] == 1, else min(sum_k w[k] m[i-k], r[i], 1 - 2^-24),
//   y[i] = clamp(v[i] * s[i], -c, c) for i < n_b, clamp(v[i], -c, c) behind.
// One launch, a workgroup per tile of LM_TILE samples of a row:
//   1. r over the tile and A samples each side is staged in LDS with coalesced loads; a tile whose whole window has r == 1 (almost
//      every tile of speech) leaves here: it streams clamp(x * g) and touches the LDS no more;
//   2. the sliding minimum by doubling, ping-pong between two LDS buffers: after the pass with step d a word holds the minimum of 2d
//      samples, and two overlapping power-of-two windows make the A+1 (min is exact, so the scheme does not show in the result);
//   3. the deficit 1 - m is stored with one pad word per 8 (a lane's 8 consecutive outputs start 9 words apart: distinct banks), and
//      each lane forms D = sum_k w[k] (1 - m[i-k]) for its 8 outputs in registers, k ascending, one LDS read per 8 multiply-adds;
//      sum_k w[k] m[i-k] is 1 - D: the weights sum to 1 within 2^-24, and D, unlike the sum itself, is small where the curve is near 1,
//      so that the fp32 sum is far inside the contract's bound and s < 1 wherever M < 1;
//   4. the curve goes back through LDS and the tile is written with coalesced stores: min with r, the multiply and the clamp.
// Every sum runs over k in ascending order for one output: a row's samples depend on its first n_b samples, g_b, the rate and the
// parameters only, not on W, the batch, the tiling or the row's place.  The per-row results (samples with M < 1, min s) are an integer
// sum and a minimum over per-tile partials, reduced by a second launch: order-independent, no atomics.
#include "kernels.hpp"

#include <math.h>

namespace stn {

namespace {

constexpr int LM_OUT = 8;                  // consecutive outputs per lane of the FIR
constexpr int LM_ROW = 256;                // threads of the per-row reduction

__device__ __forceinline__ float lm_r(float v, float c) {
    const float a = fabsf(v);
    return a <= c ? 1.0f : c / a;
}
__device__ __forceinline__ float lm_clamp(float v, float c) { return v > c ? c : (v < -c ? -c : v); }
__device__ __forceinline__ int lm_pad(int j) { return j + (j >> 3); }

// kEnv: r comes from the true-peak envelope env (rows x W: launch_truepeak of x * g) instead of the sample itself
template <bool kEnv>
__global__ void __launch_bounds__(LM_WG) limiter_kernel(const float* __restrict__ x, int64_t W, int vec, const int64_t* __restrict__ nrow,
                                                        const float* __restrict__ gain, float c, int A, int bufw,
                                                        const float* __restrict__ wts, float* __restrict__ y, float* __restrict__ sout,
                                                        int64_t tiles, int* __restrict__ pcnt, float* __restrict__ pmin,
                                                        const float* __restrict__ env) {
    extern __shared__ float lds[];
    __shared__ int redc[LM_WG / 64];
    __shared__ float redm[LM_WG / 64];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.y, t0 = (int64_t)blockIdx.x * LM_TILE;
    const int64_t n = nrow[row];
    const float g = gain ? gain[row] : 1.0f;
    const float* __restrict__ xr = x + row * W;
    float* __restrict__ yr = y + row * W;
    float* __restrict__ sr = sout ? sout + row * W : nullptr;
    const float* __restrict__ er = kEnv ? env + row * W : nullptr;
    const int N = LM_TILE + 2 * A;  // staged samples: local j is sample t0 - A + j
    float* b0 = lds;
    float* b1 = lds + bufw;
    int any = 0;
    if (t0 - A < n) {  // (else the whole window lies behind the span)
        for (int j = tid; j < N; j += LM_WG) {
            const int64_t i = t0 - A + j;
            float r = 1.0f;
            if (i >= 0 && i < n) r = kEnv ? lm_r(er[i], c) : lm_r(xr[i] * g, c);
            b0[j] = r;
            any |= r < 1.0f;
        }
    }
    any = __syncthreads_or(any);
    if (!any) {
        if (vec) {  // rows 16-byte aligned and W % 4 == 0: a float4 that starts below W ends at or below it
#pragma unroll
            for (int u = 0; u < LM_TILE / 4 / LM_WG; ++u) {
                const int64_t i = t0 + 4 * (tid + u * LM_WG);
                if (i < W) {
                    float4 v = *reinterpret_cast<const float4*>(xr + i);
                    v.x = lm_clamp(v.x * g, c); v.y = lm_clamp(v.y * g, c); v.z = lm_clamp(v.z * g, c); v.w = lm_clamp(v.w * g, c);
                    *reinterpret_cast<float4*>(yr + i) = v;
                    if (sr) *reinterpret_cast<float4*>(sr + i) = make_float4(1.f, 1.f, 1.f, 1.f);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < LM_OUT; ++u) {
                const int64_t i = t0 + tid + u * LM_WG;
                if (i < W) {
                    yr[i] = lm_clamp(xr[i] * g, c);
                    if (sr) sr[i] = 1.0f;
                }
            }
        }
        if (tid == 0) { pcnt[row * tiles + blockIdx.x] = 0; pmin[row * tiles + blockIdx.x] = 1.0f; }
        return;
    }
    // sliding minimum over A + 1 samples
    const int L = A + 1;
    float* src = b0;
    float* dst = b1;
    int d = 1;
    for (; 2 * d <= L; d *= 2) {
        for (int j = tid; j < N; j += LM_WG) dst[j] = j + d < N ? fminf(src[j], src[j + d]) : src[j];
        __syncthreads();
        float* t = src; src = dst; dst = t;
    }
    // dst: 1 - m over local j < LM_TILE + A (m[j] covers samples up to local j + A <= N - 1), padded
    for (int j = tid; j < LM_TILE + A; j += LM_WG) dst[lm_pad(j)] = 1.0f - fminf(src[j], src[j + L - d]);
    __syncthreads();
    // the lane's outputs o0 .. o0 + 7 (sample t0 + o): m[i - k] is local A + o - k
    const int o0 = tid * LM_OUT;
    float acc[LM_OUT], win[LM_OUT];
    bool lim[LM_OUT];
#pragma unroll
    for (int u = 0; u < LM_OUT; ++u) {
        acc[u] = 0.0f;
        win[u] = dst[lm_pad(A + o0 + u)];
        lim[u] = win[u] > 0.0f || dst[lm_pad(o0 + u)] > 0.0f;  // M < 1
    }
#pragma unroll 8
    for (int k = 0; k <= A; ++k) {
        const float wk = wts[k];
#pragma unroll
        for (int u = 0; u < LM_OUT; ++u) acc[u] = __builtin_fmaf(wk, win[u], acc[u]);
#pragma unroll
        for (int u = LM_OUT - 1; u > 0; --u) win[u] = win[u - 1];
        if (k < A) win[0] = dst[lm_pad(A + o0 - k - 1)];
    }
    // (src is free: every read of it lies before the barrier above)
#pragma unroll
    for (int u = 0; u < LM_OUT; ++u) src[lm_pad(o0 + u)] = lim[u] ? fminf(fmaxf(1.0f - acc[u], 0.0f), 0x1.fffffep-1f) : 1.0f;  // (D may round above 1: 0 <= s)
    __syncthreads();
    int cnt = 0;
    float mn = 1.0f;
#pragma unroll
    for (int u = 0; u < LM_OUT; ++u) {
        const int o = tid + u * LM_WG;
        const int64_t i = t0 + o;
        if (i < W) {
            const float v = xr[i] * g;
            float s = 1.0f;
            if (i < n) {
                const float sp = src[lm_pad(o)];
                if (sp < 1.0f) {
                    s = fminf(sp, kEnv ? lm_r(er[i], c) : lm_r(v, c));
                    ++cnt;
                    mn = fminf(mn, s);
                }
            }
            yr[i] = lm_clamp(s < 1.0f ? v * s : v, c);
            if (sr) sr[i] = s;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        mn = fminf(mn, __shfl_xor(mn, o, 64));
    }
    if ((tid & 63) == 0) { redc[tid >> 6] = cnt; redm[tid >> 6] = mn; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LM_WG / 64; ++w) { cnt += redc[w]; mn = fminf(mn, redm[w]); }
        pcnt[row * tiles + blockIdx.x] = cnt;
        pmin[row * tiles + blockIdx.x] = mn;
    }
}

// limited[row] = sum of the tiles' counts, red[row] = -20 log10(min of the tiles' minima) (0 where nothing was limited)
__global__ void __launch_bounds__(LM_ROW) limiter_row_kernel(int64_t tiles, const int* __restrict__ pcnt, const float* __restrict__ pmin,
                                                             int64_t* __restrict__ limited, float* __restrict__ red) {
    __shared__ long long redc[LM_ROW / 64];
    __shared__ float redm[LM_ROW / 64];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    long long cnt = 0;
    float mn = 1.0f;
    for (int64_t t = tid; t < tiles; t += LM_ROW) {
        cnt += pcnt[row * tiles + t];
        mn = fminf(mn, pmin[row * tiles + t]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        mn = fminf(mn, __shfl_xor(mn, o, 64));
    }
    if ((tid & 63) == 0) { redc[tid >> 6] = cnt; redm[tid >> 6] = mn; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LM_ROW / 64; ++w) { cnt += redc[w]; mn = fminf(mn, redm[w]); }
        limited[row] = cnt;
        red[row] = mn < 1.0f ? (float)(-20.0 * log10((double)mn)) : 0.0f;
    }
}

// words per LDS buffer: the staged window, or the padded deficits, whichever is longer
int lm_bufw(int A) {
    const int stage = LM_TILE + 2 * A, pad = LM_TILE + A + (LM_TILE + A) / 8 + 1;
    return ((stage > pad ? stage : pad) + 3) / 4 * 4;
}

}  // namespace

void launch_limiter(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, const float* gain, float c, int A, const float* wts,
                    float* y, float* s_out, int* pcnt, float* pmin, const float* env) {
    if (rows <= 0 || W <= 0) return;
    if (rows > 65535) throw std::invalid_argument("limiter: more than 65535 rows");
    if (A < 1 || A > LM_MAX_A) throw std::invalid_argument("limiter: look-ahead of " + std::to_string(A) + " samples outside [1, " + std::to_string(LM_MAX_A) + "]");
    if (!(c > 0.0f)) throw std::invalid_argument("limiter: the ceiling must be positive");
    if (x == y) throw std::logic_error("limiter: source and destination rows are the same");
    const int64_t tiles = lm_tiles(W);
    if (tiles > 0x7fffffff) throw std::invalid_argument("limiter: row too long");
    auto al16 = [](const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); };
    const int vec = (W % 4 == 0 && al16(x) && al16(y) && (!s_out || al16(s_out))) ? 1 : 0;
    const int bufw = lm_bufw(A);
    if (env) STN_KLAUNCH(limiter_kernel<true>, dim3((unsigned)tiles, (unsigned)rows), dim3(LM_WG), (unsigned)(2 * bufw * sizeof(float)), s, x, W, vec, n,
                         gain, c, A, bufw, wts, y, s_out, tiles, pcnt, pmin, env);
    else STN_KLAUNCH(limiter_kernel<false>, dim3((unsigned)tiles, (unsigned)rows), dim3(LM_WG), (unsigned)(2 * bufw * sizeof(float)), s, x, W, vec, n,
                     gain, c, A, bufw, wts, y, s_out, tiles, pcnt, pmin, env);
}

void launch_limiter_rows(hipStream_t s, int64_t rows, int64_t W, const int* pcnt, const float* pmin, int64_t* limited, float* red) {
    if (rows <= 0 || W <= 0) return;
    if (rows > 65535) throw std::invalid_argument("limiter: more than 65535 rows");
    STN_KLAUNCH(limiter_row_kernel, dim3((unsigned)rows), dim3(LM_ROW), 0, s, lm_tiles(W), pcnt, pmin, limited, red);
}

}  // namespace stn
