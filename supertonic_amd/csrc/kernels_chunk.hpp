// kernels_chunk.hpp — what the chunk kernels of the fetch-time stages share (kernels_loudness.hip, kernels_edges.hip, kernels_filter.hip,
// kernels_dynamics.hip; DESIGN.md sections 11, 14, 18, 20, 21, 25): the staging of a workgroup's span through LDS, the two-section
// biquad step, the gain computers and the detector recurrences, and the host's choice of the staging form (the engine's op entries
// report it: engine_internal.hpp includes this header for chunk_staging_form).
// One definition each: a pass and the pass that refilters from the start states the scan formed round identically by construction.
#pragma once
#include "kernels.hpp"

#include <math.h>

namespace stn {

// A workgroup of kWG lanes owns kWG chunks of kChunk consecutive samples, cnt of them inside the row (xr: the span's first sample).
// win holds chunk c at win[c * (kChunk + 1)]: at a row stride of kChunk + 1 words the lanes' walks fall on distinct banks.
// vec: 16-byte loads (xr 16-byte aligned and the row stride a multiple of 4), else the scalar form with 8 loads in flight.
// kTail: cnt need not be a multiple of 4, and the words of a float4 at or behind cnt are left out.  The caller's barrier follows.
template <int kWG, int kChunk, bool kTail>
__device__ __forceinline__ void chunk_stage_in(float* win, const float* xr, int cnt, int vec) {
    constexpr int kPad = kChunk + 1, kSpan = kWG * kChunk;
    if (vec) {
        constexpr int U = kSpan / 4 / kWG;
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = threadIdx.x + u * kWG;
            if (4 * q < cnt) v[u] = reinterpret_cast<const float4*>(xr)[q];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = 4 * (threadIdx.x + u * kWG);
            if (i < cnt) {
                float* d = win + (i / kChunk) * kPad + (i % kChunk);  // (the four samples share a chunk)
                d[0] = v[u].x;
                if (!kTail || i + 1 < cnt) d[1] = v[u].y;
                if (!kTail || i + 2 < cnt) d[2] = v[u].z;
                if (!kTail || i + 3 < cnt) d[3] = v[u].w;
            }
        }
    } else {
        for (int i0 = 0; i0 < kSpan; i0 += 8 * kWG) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + threadIdx.x + u * kWG;
                v[u] = i < cnt ? xr[i] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + threadIdx.x + u * kWG;
                if (i < cnt) win[(i / kChunk) * kPad + (i % kChunk)] = v[u];
            }
        }
    }
}

// the way back, behind the caller's second barrier: win's first cnt samples to yr (vec: cnt % 4 == 0 and yr 16-byte aligned)
template <int kWG, int kChunk>
__device__ __forceinline__ void chunk_stage_out(const float* win, float* yr, int cnt, int vec) {
    constexpr int kPad = kChunk + 1, kSpan = kWG * kChunk;
    if (vec) {
        constexpr int U = kSpan / 4 / kWG;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = threadIdx.x + u * kWG, i = 4 * q;
            if (i < cnt) {
                const float* d = win + (i / kChunk) * kPad + (i % kChunk);
                reinterpret_cast<float4*>(yr)[q] = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += kWG) yr[i] = win[(i / kChunk) * kPad + (i % kChunk)];
    }
}

// one sample through two biquad sections (b0 b1 b2 a1 a2 = c[0..4], then c[5..9]), transposed direct form II in fp32: the 4-state
// system whose chunk-end states the scan in double composes.  The start states the scan forms are exact for this arithmetic only.
__device__ __forceinline__ float biquad2_step(const LoudCoef& f, float u, float& s1, float& s2, float& t1, float& t2) {
    const float v = __builtin_fmaf(f.c[0], u, s1);
    s1 = __builtin_fmaf(-f.c[3], v, __builtin_fmaf(f.c[1], u, s2));
    s2 = __builtin_fmaf(-f.c[4], v, f.c[2] * u);
    const float y = __builtin_fmaf(f.c[5], v, t1);
    t1 = __builtin_fmaf(-f.c[8], y, __builtin_fmaf(f.c[6], v, t2));
    t2 = __builtin_fmaf(-f.c[9], y, f.c[7] * v);
    return y;
}

// the gain computer: the reduction wanted at a sample, in dB (>= 0), for threshold T, slope S = 1 / ratio - 1 and knee K.  The knee's
// quadratic only where there is a knee: with K = 0 and d = 0 it would be 0 / 0, and the hard corner gives 0 there.
__device__ __forceinline__ float gain_want(float T, float S, float K, float x) {
    const float xg = 20.0f * log10f(fmaxf(fabsf(x), 1e-6f));
    const float d = xg - T;
    const float d2 = 2.0f * d;
    if (d2 < -K) return 0.0f;
    if (K > 0.0f && fabsf(d2) <= K) {
        const float t = d + 0.5f * K;
        return (-S * (t * t)) / (2.0f * K);
    }
    return -S * d;
}
// the decoupled peak detector y1 = max(z, y1 - kR y1) and its smoothing yL = yL + kA (y1 - yL)
__device__ __forceinline__ float gain_peak(float kR, float z, float y1) { return fmaxf(z, __builtin_fmaf(-kR, y1, y1)); }
__device__ __forceinline__ float gain_smooth(float kA, float y1, float yl) { return __builtin_fmaf(kA, y1 - yl, yl); }

// the expander's gain computer (section 25), gain_want's sibling: the openness wanted at a sample, in dB, for threshold T, slope
// S = ratio - 1, knee K and range R.  z in [0, R] is the attenuation wanted d = T - xG dB under the threshold, o = R - z the openness;
// a fully open sample (z == 0) carries the hold boost Bh on top, which the (max, +) detector takes Bh / delta samples to walk down.
__device__ __forceinline__ float expand_open(float T, float S, float K, float R, float Bh, float x) {
    const float xg = 20.0f * log10f(fmaxf(fabsf(x), 1e-6f));
    const float d = T - xg;
    const float d2 = 2.0f * d;
    float z;
    if (d2 < -K) {
        z = 0.0f;
    } else if (K > 0.0f && fabsf(d2) <= K) {
        const float t = d + 0.5f * K;
        z = (S * (t * t)) / (2.0f * K);
    } else {
        z = S * d;
    }
    z = fminf(z, R);
    const float o = R - z;
    return z == 0.0f ? o + Bh : o;
}
// its detector u = max(t, u - delta): opens at once, holds, then closes at a constant rate in dB
__device__ __forceinline__ float expand_detect(float delta, float t, float u) { return fmaxf(t, u - delta); }

inline bool aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }
// 1: the 16-byte form of chunk_stage_in / chunk_stage_out for rows of stride W read at x and written at y (null: not written)
inline int chunk_vec(const float* x, const float* y, int64_t W) { return W % 4 == 0 && aligned16(x) && aligned16(y) ? 1 : 0; }
// that choice as the op-level probes name it: "vec" (16-byte loads and stores: W % 4 == 0, x and y 16-byte aligned) or "scalar"
inline const char* chunk_staging_form(const float* x, const float* y, int64_t W) { return chunk_vec(x, y, W) ? "vec" : "scalar"; }
// the limits of a grid (ceil(W / (LO_WG * LO_CHUNK)), rows) whose chunk index is an int
inline void chunk_shape(const char* unit, int64_t rows, int64_t W) {
    if (rows > 65535) throw std::invalid_argument(std::string(unit) + ": more than 65535 rows");
    if (lo_chunks(W) > ((int64_t)1 << 31) / LO_WG) throw std::invalid_argument(std::string(unit) + ": row too long");
}

}  // namespace stn
