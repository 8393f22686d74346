// kernels_truepeak.hip — true peak of the finished waveform by 4x oversampling (ITU-R BS.1770-4 Annex 2; gfx950, wave64; DESIGN.md
// section 16).  Runs at fetch time, outside the captured pipeline, on rows x W fp32 samples of which row b's first n_b count.
//
// With x = 0 outside [0, n): u[i][ph] = sum_j h[ph][j] x[i - 7 + j], j ascending in one fp32 FMA chain, is the signal at i + ph/4
// (ph = 1, 2, 3; phase 0 is the sample itself), U[i] = max_ph |u[i][ph]| for i in [-1, n - 1], and the envelope
// p[i] = max(|x[i]|, U[i-1], U[i]) covers every oversampled point strictly between i - 1 and i + 1.  One launch, the chunk pass's shape
// (kernels_loudness.hip): a lane owns TP_CHUNK consecutive samples counted from sample 0; a workgroup stages its TP_SPAN samples and 8
// on each side in LDS, masked to zero outside [0, n), times the row's gain when there is one (chunk pitch 33 words: a wave's reads at
// one step fall on distinct banks); each lane slides a 16-sample register window over its chunk and forms the 33 values
// U[first - 1 .. last] (48 FMAs each, the taps in SGPRs), so that a chunk needs nothing from its neighbours' lanes; it writes the
// chunk's maximum straight to pk.  With an envelope asked for, p goes back through the LDS and leaves in coalesced stores.
// max is exact and every chain has one order: a row's values depend on its first n samples (and its gain) only, not on W, the batch,
// the tiling or the row's place.  No atomics.
#include "kernels.hpp"

#include <math.h>

namespace stn {

namespace {

constexpr int TP_CHUNK = LO_CHUNK;            // samples per lane: pk is the loudness measurement's per-chunk buffer
constexpr int TP_WG = 256;                    // lanes (chunks) per workgroup
constexpr int TP_SPAN = TP_WG * TP_CHUNK;     // samples a workgroup owns
constexpr int TP_HALO = 8;                    // staged samples before and behind the span (TP_OFF + 1 and TP_TAPS - TP_OFF - 1 are both <= 8)
constexpr int TP_PAD = TP_CHUNK + 1;          // LDS words per chunk
constexpr int TP_LEAD = TP_CHUNK;             // local sample q (q >= -TP_HALO) sits at slot q + TP_LEAD: one leading chunk holds the front halo
constexpr int TP_SLOTS = TP_LEAD + TP_SPAN + TP_HALO;                     // slots in use: [TP_LEAD - TP_HALO, TP_SLOTS)
constexpr int TP_WORDS = ((TP_SLOTS + TP_CHUNK - 1) / TP_CHUNK) * TP_PAD;
constexpr int TP_ROW = 256;                   // threads of the per-row reduction

__device__ __forceinline__ int tp_at(int slot) { return (slot / TP_CHUNK) * TP_PAD + (slot % TP_CHUNK); }

// one oversampled instant: the 16 samples of the window against one phase
__device__ __forceinline__ float tp_phase(const float (&h)[TP_TAPS], const float (&w)[TP_TAPS]) {
    float a = h[0] * w[0];
#pragma unroll
    for (int j = 1; j < TP_TAPS; ++j) a = __builtin_fmaf(h[j], w[j], a);
    return fabsf(a);
}

template <bool kEnv>
__global__ void __launch_bounds__(TP_WG) truepeak_kernel(const float* __restrict__ x, int64_t W, int vec, const int64_t* __restrict__ nrow,
                                                         const float* __restrict__ gain, int64_t Ks, TpCoef f, float* __restrict__ pk,
                                                         float* __restrict__ env) {
    __shared__ float win[TP_WORDS];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.y;
    const int64_t n = nrow[row];
    const int64_t s0 = (int64_t)blockIdx.x * TP_SPAN;
    const float g = gain ? gain[row] : 1.0f;
    const float* __restrict__ xr = x + row * W;
    const int64_t k = (int64_t)blockIdx.x * TP_WG + tid;
    float m = 0.0f;
    const bool live = s0 < n;  // (the whole workgroup: something of the span lies in its samples)
    if (live) {
        // stage samples s0 - 8 .. s0 + TP_SPAN + 8, zero outside [0, n)
        if (vec) {  // rows 16-byte aligned and W % 4 == 0: a float4 that starts below n ends at or below W
            constexpr int NV = (TP_SPAN + 2 * TP_HALO) / 4;
#pragma unroll
            for (int u = 0; u < (NV + TP_WG - 1) / TP_WG; ++u) {
                const int q = tid + u * TP_WG;
                if (q < NV) {
                    const int64_t i = s0 - TP_HALO + 4 * (int64_t)q;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (i >= 0 && i < n) {
                        v = *reinterpret_cast<const float4*>(xr + i);
                        v.x = v.x * g;
                        v.y = i + 1 < n ? v.y * g : 0.0f;
                        v.z = i + 2 < n ? v.z * g : 0.0f;
                        v.w = i + 3 < n ? v.w * g : 0.0f;
                    }
                    float* d = win + tp_at(TP_LEAD - TP_HALO + 4 * q);  // (the four samples share a chunk)
                    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                }
            }
        } else {
            for (int q = tid; q < TP_SPAN + 2 * TP_HALO; q += TP_WG) {
                const int64_t i = s0 - TP_HALO + q;
                win[tp_at(TP_LEAD - TP_HALO + q)] = (i >= 0 && i < n) ? xr[i] * g : 0.0f;
            }
        }
        __syncthreads();
        const int64_t first = s0 + (int64_t)tid * TP_CHUNK;
        float p[kEnv ? TP_CHUNK : 1];
        if (first < n) {
            // w = x[i - 7 .. i + 8] for i = first - 1, then slid one sample per step: slot of x[first + d] is TP_LEAD + 32 tid + d
            const int base = TP_LEAD + tid * TP_CHUNK;
            float w[TP_TAPS];
#pragma unroll
            for (int j = 0; j < TP_TAPS; ++j) w[j] = win[tp_at(base - TP_HALO + j)];
            float up = 0.0f;
#pragma unroll
            for (int e = 0; e <= TP_CHUNK; ++e) {  // i = first - 1 + e
                const float u = fmaxf(fmaxf(tp_phase(f.h[0], w), tp_phase(f.h[1], w)), tp_phase(f.h[2], w));
                if (e > 0) {
                    const float pe = fmaxf(fabsf(w[TP_OFF]), fmaxf(up, u));
                    if (kEnv) p[e - 1] = pe;
                    m = fmaxf(m, first + (e - 1) < n ? pe : 0.0f);
                }
                up = u;
                if (e < TP_CHUNK) {
#pragma unroll
                    for (int j = 0; j + 1 < TP_TAPS; ++j) w[j] = w[j + 1];
                    w[TP_TAPS - 1] = win[tp_at(base + TP_HALO + e)];
                }
            }
        }
        if (kEnv) {
            __syncthreads();  // every lane's reads of the staged samples lie before here
            if (first < n) {
#pragma unroll
                for (int e = 0; e < TP_CHUNK; ++e) win[tid * TP_PAD + e] = p[e];
            }
            __syncthreads();
        }
    }
    if (k < Ks) pk[row * Ks + k] = m;
    if (kEnv) {
        // p for the samples inside the span (from the LDS), |x * g| behind it
        float* __restrict__ er = env + row * W;
        if (vec) {
#pragma unroll
            for (int u = 0; u < TP_SPAN / 4 / TP_WG; ++u) {
                const int o = 4 * (tid + u * TP_WG);
                const int64_t i = s0 + o;
                if (i < W) {
                    float4 v;
                    if (i + 3 < n) {
                        const float* d = win + (o / TP_CHUNK) * TP_PAD + (o % TP_CHUNK);
                        v = make_float4(d[0], d[1], d[2], d[3]);
                    } else {
                        const float4 a = *reinterpret_cast<const float4*>(xr + i);
                        const float* d = win + (o / TP_CHUNK) * TP_PAD + (o % TP_CHUNK);
                        v.x = i < n ? d[0] : fabsf(a.x * g);
                        v.y = i + 1 < n ? d[1] : fabsf(a.y * g);
                        v.z = i + 2 < n ? d[2] : fabsf(a.z * g);
                        v.w = fabsf(a.w * g);
                    }
                    *reinterpret_cast<float4*>(er + i) = v;
                }
            }
        } else {
#pragma unroll 4
            for (int u = 0; u < TP_CHUNK; ++u) {
                const int o = tid + u * TP_WG;
                const int64_t i = s0 + o;
                if (i < W) er[i] = i < n ? win[(o / TP_CHUNK) * TP_PAD + (o % TP_CHUNK)] : fabsf(xr[i] * g);
            }
        }
    }
}

// tp[row] = max over the span's chunks (max is exact: any order), trim[row] = 1 where tp <= c, else c / tp
__global__ void __launch_bounds__(TP_ROW) truepeak_row_kernel(const int64_t* __restrict__ nrow, int64_t Ks, const float* __restrict__ pk, float c,
                                                              float* __restrict__ tp, float* __restrict__ trim) {
    __shared__ float redm[TP_ROW / 64];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t K = lo_chunks(nrow[row]);
    float m = 0.0f;
    for (int64_t k = tid; k < K; k += TP_ROW) m = fmaxf(m, pk[row * Ks + k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) redm[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < TP_ROW / 64; ++w) m = fmaxf(m, redm[w]);
        tp[row] = m;
        if (trim) trim[row] = m <= c ? 1.0f : c / m;
    }
}

bool tp_al16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }
bool tp_vec(const float* x, int64_t W, const float* env) { return W % 4 == 0 && tp_al16(x) && (!env || tp_al16(env)); }

void tp_check(int64_t rows, int64_t W) {
    if (rows > 65535) throw std::invalid_argument("true peak: more than 65535 rows");
    if (lo_chunks(W) > ((int64_t)1 << 31) / TP_WG) throw std::invalid_argument("true peak: row too long");
}

}  // namespace

const char* truepeak_staging_form(const float* x, int64_t W, const float* env) { return tp_vec(x, W, env) ? "vec" : "scalar"; }

void launch_truepeak(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, const float* gain, float* pk, float* env) {
    if (rows <= 0 || W <= 0) return;
    tp_check(rows, W);
    if (x == env) throw std::logic_error("true peak: the envelope cannot replace its source rows");
    static const TpCoef coef = truepeak_coef();
    const int vec = tp_vec(x, W, env) ? 1 : 0;
    const dim3 grid((unsigned)((W + TP_SPAN - 1) / TP_SPAN), (unsigned)rows);
    if (env) STN_KLAUNCH(truepeak_kernel<true>, grid, dim3(TP_WG), 0, s, x, W, vec, n, gain, lo_chunks(W), coef, pk, env);
    else STN_KLAUNCH(truepeak_kernel<false>, grid, dim3(TP_WG), 0, s, x, W, vec, n, gain, lo_chunks(W), coef, pk, env);
}

void launch_truepeak_rows(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, const float* pk, float c, float* tp, float* trim) {
    if (rows <= 0 || W <= 0) return;
    tp_check(rows, W);
    STN_KLAUNCH(truepeak_row_kernel, dim3((unsigned)rows), dim3(TP_ROW), 0, s, n, lo_chunks(W), pk, c, tp, trim);
}

}  // namespace stn
