// kernels_dwconv_ln.hip — depthwise dilated conv along time fused with LayerNorm over channels, and the plain LayerNorm (gfx950, wave64).
// One wavefront per frame (or per comb of frames), 16-B (float4) coalesced channel loads, mean / variance by wavefront shuffles; HBM sees each
// frame once.  Row-major [rows][channels]; see kernels.hpp for the contracts.  Which kernel a call takes is ONE host decision, dwconv_ln_form.
#include "kernels.hpp"
#include "kernels_dev.hpp"
#include "dev_env.hpp"

#include <type_traits>
#include <stdio.h>
#include <stdlib.h>

namespace stn {

// ---------------------------------------------------------------------------------------------
// depthwise conv + LayerNorm  (CONV=false: LayerNorm only).  One wavefront per frame.
// ---------------------------------------------------------------------------------------------
template <typename OutT, bool CONV>
__global__ __launch_bounds__(256) void dwconv_ln_kernel(const float* __restrict__ x, int64_t M, int L, int C,
                                                        const float* __restrict__ w_t, const float* __restrict__ bias,
                                                        int k, int dil, const float* __restrict__ g,
                                                        const float* __restrict__ bt, float eps, OutT* __restrict__ y,
                                                        const int* __restrict__ seqlen) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;  // wave-uniform
    const int Lv = (CONV && seqlen) ? seqlen[row / L] : L;       // valid frames of this row's sequence
    const bool live = !(CONV && (int)(row % L) >= Lv);           // rows in the padding are written as zeros (+0: a select, not a product)
    const int C4 = C >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float4 h[LN_NI];
    if (CONV) {
        const int t = (int)(row % L);
        const int64_t base = row - t;
        const int half = (k - 1) >> 1;
        const float4* w4 = reinterpret_cast<const float4*>(w_t);
        const float4* b4 = reinterpret_cast<const float4*>(bias);
#pragma unroll
        for (int i = 0; i < LN_NI; ++i) {
            const int c4 = lane + 64 * i;
            h[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c4 < C4) {
                float4 a = b4[c4];
                for (int j = 0; j < k; ++j) {
                    const int tt = t + (j - half) * dil;
                    if (tt >= 0 && tt < Lv) {
                        const float4 xv = x4[(base + tt) * C4 + c4];
                        const float4 wv = w4[(int64_t)j * C4 + c4];
                        a.x = fmaf(wv.x, xv.x, a.x); a.y = fmaf(wv.y, xv.y, a.y);
                        a.z = fmaf(wv.z, xv.z, a.z); a.w = fmaf(wv.w, xv.w, a.w);
                    }
                }
                h[i] = a;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < LN_NI; ++i) {
            const int c4 = lane + 64 * i;
            h[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c4 < C4) h[i] = x4[row * C4 + c4];
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_NI; ++i) s += (h[i].x + h[i].y) + (h[i].z + h[i].w);  // slots past C4 hold zeros
    const float mean = wave_sum(s) / (float)C;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < LN_NI; ++i) {
        if (lane + 64 * i < C4) {
            const float dx = h[i].x - mean, dy = h[i].y - mean, dz = h[i].z - mean, dw = h[i].w - mean;
            v += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    }
    const float rstd = rsqrtf(wave_sum(v) / (float)C + eps);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const float4* bt4 = reinterpret_cast<const float4*>(bt);
#pragma unroll
    for (int i = 0; i < LN_NI; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < C4) {
            const float4 gg = g4[c4], bb = bt4[c4];
            store4(y + row * C + c4 * 4, live ? (h[i].x - mean) * rstd * gg.x + bb.x : 0.f, live ? (h[i].y - mean) * rstd * gg.y + bb.y : 0.f,
                   live ? (h[i].z - mean) * rstd * gg.z + bb.z : 0.f, live ? (h[i].w - mean) * rstd * gg.w + bb.w : 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// dwconv + LayerNorm, fast path: compile-time tap count K, R frames per wavefront, C <= 512.
// Every tap load of every frame is issued before the first FMA (out-of-range taps load a clamped in-range
// frame and are zeroed by a select), so a wave has R*K independent 16-B loads in flight per channel slot
// instead of one dependent load per tap; the tap weights are loaded once and shared by the R frames.
// ---------------------------------------------------------------------------------------------
template <typename OutT, int K, int R>
__global__ __launch_bounds__(256) void dwconv_ln_v2_kernel(const float* __restrict__ x, int64_t M, int L, int C,
                                                           const float* __restrict__ w_t, const float* __restrict__ bias,
                                                           int dil, const float* __restrict__ g,
                                                           const float* __restrict__ bt, float eps, OutT* __restrict__ y,
                                                           const int* __restrict__ seqlen) {
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
    if (r0 >= M) return;  // wave-uniform
    const int C4 = C >> 2;
    constexpr int HALF = (K - 1) / 2;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* w4 = reinterpret_cast<const float4*>(w_t);
    const float4* b4 = reinterpret_cast<const float4*>(bias);
    int tpos[R], lv[R];
    int64_t base[R];
    bool rowok[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = r0 + r < M ? r0 + r : M - 1;
        tpos[r] = (int)(row % L);
        base[r] = row - tpos[r];
        lv[r] = seqlen ? seqlen[row / L] : L;
        rowok[r] = r0 + r < M;
    }
    float4 h[R][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c4 = lane + 64 * i;
        const bool act = c4 < C4;
        const int cc = act ? c4 : 0;
        float4 xv[R][K];
        float4 wv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) wv[j] = w4[(int64_t)j * C4 + cc];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int tt = tpos[r] + (j - HALF) * dil;
                const int tc = tt < 0 ? 0 : (tt >= L ? L - 1 : tt);
                xv[r][j] = x4[(base[r] + tc) * C4 + cc];  // clamped in-range load; replaced by zero below when outside [0, lv)
            }
        const float4 bv = b4[cc];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float4 a = bv;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int tt = tpos[r] + (j - HALF) * dil;
                // a select, not a product with 0: what the clamped load fetched from a padding row may be a NaN or an infinity
                const bool keep = tt >= 0 && tt < lv[r];
                const float4 v = keep ? xv[r][j] : make_float4(0.f, 0.f, 0.f, 0.f);
                a.x = fmaf(wv[j].x, v.x, a.x); a.y = fmaf(wv[j].y, v.y, a.y);
                a.z = fmaf(wv[j].z, v.z, a.z); a.w = fmaf(wv[j].w, v.w, a.w);
            }
            h[r][i] = act ? a : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const float4* bt4 = reinterpret_cast<const float4*>(bt);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float s = (h[r][0].x + h[r][0].y) + (h[r][0].z + h[r][0].w) + (h[r][1].x + h[r][1].y) + (h[r][1].z + h[r][1].w);
        const float mean = wave_sum(s) / (float)C;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (lane + 64 * i < C4) {
                const float dx = h[r][i].x - mean, dy = h[r][i].y - mean, dz = h[r][i].z - mean, dw = h[r][i].w - mean;
                v += (dx * dx + dy * dy) + (dz * dz + dw * dw);
            }
        const float rstd = rsqrtf(wave_sum(v) / (float)C + eps);
        if (!rowok[r]) continue;  // wave-uniform
        const bool live = tpos[r] < lv[r];  // rows in the padding are written as zeros (+0: a select, not a product)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c4 = lane + 64 * i;
            if (c4 < C4) {
                const float4 gg = g4[c4], bb = bt4[c4];
                store4(y + (r0 + r) * C + c4 * 4, live ? (h[r][i].x - mean) * rstd * gg.x + bb.x : 0.f, live ? (h[r][i].y - mean) * rstd * gg.y + bb.y : 0.f,
                       live ? (h[r][i].z - mean) * rstd * gg.z + bb.z : 0.f, live ? (h[r][i].w - mean) * rstd * gg.w + bb.w : 0.f);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// dwconv + LayerNorm v3 ("comb"): a wavefront owns R output frames spaced by the dilation, t_i = t0 + i*dil.  Their
// taps overlap: the R outputs need only R+K-1 distinct input frames (t0 + (q - K/2)*dil), which are loaded once into
// registers as a sliding window — 1 + (K-1)/R loads per output instead of K, for ANY dilation.  Cuts the L2->CU traffic
// of the vocoder's k=7 blocks by 4x at R=8 (HBM already saw each frame once; the re-reads were L2 bandwidth).
// ---------------------------------------------------------------------------------------------
// TAIL (packed rows only; the dense vocoder trimmed to one receptive field): sequence b is the head of a row of T frames whose frames from
// seqlen[b] on are not stored because their value depends only on the distance to the end of the row.  A tap at tt >= seqlen[b] then reads
// tail[min(T - 1 - tt, rf)] ([rf + 1][C] fp32; entry rf stands for every frame further from the end) and zero from T on; tt is wave-uniform,
// so the choice is scalar address arithmetic.  The order of the tap FMAs and of the LayerNorm sums is the same in both variants.
template <typename OutT, int K, int R, bool TAIL = false>
__device__ __forceinline__ void dwconv_ln_v3_body(const float* __restrict__ x, int nseq, int L, int C,
                                                           const float* __restrict__ w_t, const float* __restrict__ bias,
                                                           int dil, int wps /*waves per sequence*/, const float* __restrict__ g,
                                                           const float* __restrict__ bt, float eps, OutT* __restrict__ y,
                                                           const int* __restrict__ seqlen, const int* __restrict__ row_off, int xcd_runs,
                                                           const float* __restrict__ tail = nullptr, int T = 0, int rf = 0) {
    const int lane = threadIdx.x & 63;
    // Workgroups are dealt to the 8 XCDs round-robin, and each XCD has its own L2: with the plain order the two workgroups that share a halo
    // (neighbours in time) sit on different XCDs and both fetch it over the fabric.  Give each XCD one contiguous run of tiles instead.
    int bid = blockIdx.x;
    if (xcd_runs) {
        const int nb = gridDim.x, q = nb >> 3, rr = nb & 7, xcd = bid & 7, idx = bid >> 3;
        bid = xcd * q + (xcd < rr ? xcd : rr) + idx;
    }
    const int64_t wid = (int64_t)bid * 4 + (threadIdx.x >> 6);
    if (wid >= (int64_t)nseq * wps) return;  // wave-uniform
    const int b = (int)(wid / wps), rem = (int)(wid % wps);
    const int t0 = (rem / dil) * (R * dil) + (rem % dil);
    const int Lv = seqlen ? seqlen[b] : L;  // valid frames of this sequence (<= L)
    constexpr int HALF = (K - 1) / 2, NWIN = R + K - 1;
    const int C4 = C >> 2;
    // packed rows (row_off given): sequence b owns rows row_off[b] .. row_off[b] + seqlen[b]; else b*L .. b*L + L
    const int64_t row0 = row_off ? (int64_t)row_off[b] : (int64_t)b * L;
    if (t0 >= Lv) {  // the whole comb lies in the padding: its rows are defined (zeros) but cost no loads or arithmetic
        if (row_off) return;  // packed layout: there are no padding rows
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int t = t0 + r * dil;
            if (t >= L) break;
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (lane + 64 * i < C4) store4(y + (row0 + t) * C + (lane + 64 * i) * 4, 0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const float4* x4 = reinterpret_cast<const float4*>(x) + row0 * C4;
    const float4* w4 = reinterpret_cast<const float4*>(w_t);
    const float4* b4 = reinterpret_cast<const float4*>(bias);
    float4 h[R][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c4 = lane + 64 * i;
        const bool act = c4 < C4;
        const int cc = act ? c4 : 0;
        float4 win[NWIN], wv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) wv[j] = w4[(int64_t)j * C4 + cc];
#pragma unroll
        for (int q = 0; q < NWIN; ++q) {
            const int tt = t0 + (q - HALF) * dil;
            const int hi_ = row_off ? Lv : L;  // clamp inside the rows this sequence owns
            const int tc = tt < 0 ? 0 : (tt >= hi_ ? hi_ - 1 : tt);
            if constexpr (TAIL) {
                const float4* src = x4 + (int64_t)tc * C4;
                bool keep = tt >= 0 && tt < Lv;
                if (tt >= Lv && tt < T) {  // wave-uniform: a frame of the row's position-dependent tail
                    const int j = T - 1 - tt;
                    src = reinterpret_cast<const float4*>(tail) + (int64_t)(j < rf ? j : rf) * C4;
                    keep = true;
                }
                const float4 v = src[cc];
                win[q] = keep ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
                const float4 v = x4[(int64_t)tc * C4 + cc];
                // a select, not a product with 0: what the clamped load fetched from a padding row may be a NaN or an infinity
                win[q] = (tt >= 0 && tt < Lv) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        const float4 bv = b4[cc];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float4 a = bv;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                a.x = fmaf(wv[j].x, win[r + j].x, a.x); a.y = fmaf(wv[j].y, win[r + j].y, a.y);
                a.z = fmaf(wv[j].z, win[r + j].z, a.z); a.w = fmaf(wv[j].w, win[r + j].w, a.w);
            }
            h[r][i] = act ? a : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const float4* bt4 = reinterpret_cast<const float4*>(bt);
    float4 gg[2], bb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c4 = lane + 64 * i;
        gg[i] = g4[c4 < C4 ? c4 : 0];
        bb[i] = bt4[c4 < C4 ? c4 : 0];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int t = t0 + r * dil;
        const float s = (h[r][0].x + h[r][0].y) + (h[r][0].z + h[r][0].w) + (h[r][1].x + h[r][1].y) + (h[r][1].z + h[r][1].w);
        const float mean = wave_sum(s) / (float)C;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (lane + 64 * i < C4) {
                const float dx = h[r][i].x - mean, dy = h[r][i].y - mean, dz = h[r][i].z - mean, dw = h[r][i].w - mean;
                v += (dx * dx + dy * dy) + (dz * dz + dw * dw);
            }
        const float rstd = rsqrtf(wave_sum(v) / (float)C + eps);
        if (t >= L) continue;  // wave-uniform (tail of the sequence)
        if (t >= Lv) {         // padding of a shorter sequence: zeros (rows that do not exist in the packed layout)
            if (row_off) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (lane + 64 * i < C4) store4(y + (row0 + t) * C + (lane + 64 * i) * 4, 0.f, 0.f, 0.f, 0.f);
            continue;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c4 = lane + 64 * i;
            if (c4 < C4)
                store4(y + (row0 + t) * C + c4 * 4, (h[r][i].x - mean) * rstd * gg[i].x + bb[i].x,
                       (h[r][i].y - mean) * rstd * gg[i].y + bb[i].y, (h[r][i].z - mean) * rstd * gg[i].z + bb[i].z,
                       (h[r][i].w - mean) * rstd * gg[i].w + bb[i].w);
        }
    }
}

template <typename OutT, int K, int R>
__global__ __launch_bounds__(256) void dwconv_ln_v3_kernel(const float* __restrict__ x, int nseq, int L, int C, const float* __restrict__ w_t,
                                                           const float* __restrict__ bias, int dil, int wps, const float* __restrict__ g, const float* __restrict__ bt,
                                                           float eps, OutT* __restrict__ y, const int* __restrict__ seqlen, const int* __restrict__ row_off, int xcd_runs) {
    dwconv_ln_v3_body<OutT, K, R>(x, nseq, L, C, w_t, bias, dil, wps, g, bt, eps, y, seqlen, row_off, xcd_runs);
}
// the same body held to 128 VGPRs (four waves per SIMD instead of three: the vocoder's k = 7 combs of four need 130 by themselves)
template <typename OutT, int K, int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void dwconv_ln_v3_occ4_kernel(
    const float* __restrict__ x, int nseq, int L, int C, const float* __restrict__ w_t, const float* __restrict__ bias, int dil, int wps,
    const float* __restrict__ g, const float* __restrict__ bt, float eps, OutT* __restrict__ y, const int* __restrict__ seqlen,
    const int* __restrict__ row_off, int xcd_runs) {
    dwconv_ln_v3_body<OutT, K, R>(x, nseq, L, C, w_t, bias, dil, wps, g, bt, eps, y, seqlen, row_off, xcd_runs);
}

// the tail-reading variants (packed rows), plain and held to four waves per SIMD like the two above
template <typename OutT, int K, int R>
__global__ __launch_bounds__(256) void dwconv_ln_v3_tail_kernel(const float* __restrict__ x, int nseq, int L, int C, const float* __restrict__ w_t,
                                                                const float* __restrict__ bias, int dil, int wps, const float* __restrict__ g,
                                                                const float* __restrict__ bt, float eps, OutT* __restrict__ y,
                                                                const int* __restrict__ seqlen, const int* __restrict__ row_off, int xcd_runs,
                                                                const float* __restrict__ tail, int T, int rf) {
    dwconv_ln_v3_body<OutT, K, R, true>(x, nseq, L, C, w_t, bias, dil, wps, g, bt, eps, y, seqlen, row_off, xcd_runs, tail, T, rf);
}
template <typename OutT, int K, int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void dwconv_ln_v3_tail_occ4_kernel(
    const float* __restrict__ x, int nseq, int L, int C, const float* __restrict__ w_t, const float* __restrict__ bias, int dil, int wps,
    const float* __restrict__ g, const float* __restrict__ bt, float eps, OutT* __restrict__ y, const int* __restrict__ seqlen,
    const int* __restrict__ row_off, int xcd_runs, const float* __restrict__ tail, int T, int rf) {
    dwconv_ln_v3_body<OutT, K, R, true>(x, nseq, L, C, w_t, bias, dil, wps, g, bt, eps, y, seqlen, row_off, xcd_runs, tail, T, rf);
}

template <typename OutT, int K, int R>
static void launch_dwconv_ln_v3_kr(hipStream_t s, bool occ4, const float* x, int nseq, int L, int C, const float* w_t, const float* bias,
                                   int dil, const float* g, const float* b, float eps, OutT* y, const int* seqlen, const int* row_off,
                                   const DwconvTail& tl) {
    const int wps = ((L + R * dil - 1) / (R * dil)) * dil;
    const int64_t nw = (int64_t)nseq * wps;
    static const int xcd_runs = [] { const char* e = stn::dev_env("STN_DWCONV_XCD"); return e ? atoi(e) : 1; }();  // A/B switch
    if (tl.tail) {
        if constexpr (K == 7 && R == 4 && !std::is_same<OutT, f16_t>::value) {
            if (occ4) {
                STN_KLAUNCH((dwconv_ln_v3_tail_occ4_kernel<OutT, K, R>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, x, nseq, L, C, w_t, bias,
                                   dil, wps, g, b, eps, y, seqlen, row_off, xcd_runs, tl.tail, tl.T, tl.rf);
                return;
            }
        }
        if (occ4) throw std::logic_error("dwconv_ln: no occ4 kernel for this form");
        STN_KLAUNCH((dwconv_ln_v3_tail_kernel<OutT, K, R>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, x, nseq, L, C, w_t, bias,
                           dil, wps, g, b, eps, y, seqlen, row_off, xcd_runs, tl.tail, tl.T, tl.rf);
        return;
    }
    // (the occ4 kernel exists where dwconv_ln_form can choose it: the IEEE-half instantiation would need 184 VGPRs and spill)
    if constexpr (K == 7 && R == 4 && !std::is_same<OutT, f16_t>::value) {
        if (occ4) {
            STN_KLAUNCH((dwconv_ln_v3_occ4_kernel<OutT, K, R>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, x, nseq, L, C, w_t, bias,
                               dil, wps, g, b, eps, y, seqlen, row_off, xcd_runs);
            return;
        }
    }
    if (occ4) throw std::logic_error("dwconv_ln: no occ4 kernel for this form");
    STN_KLAUNCH((dwconv_ln_v3_kernel<OutT, K, R>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, x, nseq, L, C, w_t, bias,
                       dil, wps, g, b, eps, y, seqlen, row_off, xcd_runs);
}

void check_ln_shape(int C) {
    if (C % 4 || C > 4 * 64 * LN_NI) { char m_[256]; snprintf(m_, sizeof m_, "LayerNorm width %d unsupported (C %% 4 == 0, C <= 1024)", C); throw std::invalid_argument(m_); }
}

bool dwconv_ln_supports_packed(int C, int k) { return C <= 512 && C % 4 == 0 && (k == 5 || k == 7); }

std::string DwconvLnForm::str() const {
    if (kernel == DW_GENERIC) return "generic";
    char m_[32];
    if (kernel == DW_V2) snprintf(m_, sizeof m_, "v2<%d>", K);
    else snprintf(m_, sizeof m_, "%s<%d,%d>", occ4 ? "v3occ4" : "v3", K, R);
    return m_;
}

DwconvLnForm dwconv_ln_form(int out_dtype, int B, int L, int C, int k, bool packed) {
    check_ln_shape(C);
    if (packed && !dwconv_ln_supports_packed(C, k)) throw std::invalid_argument("packed dwconv_ln needs lengths, C <= 512, k in {5,7}");
    DwconvLnForm f;
    f.out_dtype = out_dtype == BF16 || out_dtype == F16 ? out_dtype : F32;
    f.K = k;
    if (C > 512 || (k != 5 && k != 7)) return f;  // the generic kernel: one wavefront per frame, run-time tap count
    // enough wavefronts to fill the chip (256 CUs x ~8): long combs only when there are many frames
    const int64_t M = (int64_t)B * L;
    f.kernel = DW_V3;
    if (M >= 32768) {
        // k = 7 (the vocoder, 60 k frames at C3): combs of 4 measured 51 us per launch against 57 us for combs of 8 (twice the wavefronts
        // outweigh 2.5 instead of 1.75 loads per output; combs of 2: 58 us)
        f.R = k == 5 ? 8 : 4;
    } else if (M >= 4096) {
        // k = 5 below 16 k frames (the estimator at batch 128: 7.4 k): combs of 2 give twice the wavefronts for 1.5x the loads per output
        // (9.5 -> 8.7 us per launch)
        f.R = k == 5 ? (M < 16384 ? 2 : 4) : 4;
    } else if (packed) {  // the packed layout only exists in the v3 kernel
        // (a single utterance: ~15 wavefronts at combs of 4 — combs of 2 halve the serial work per wavefront)
        f.R = k == 5 ? (M < 1024 ? 2 : 4) : 4;
    } else {
        f.kernel = DW_V2;  // few frames: one wave per 2 frames exposes more parallelism
        f.R = 2;
    }
    // k = 7 combs of four (the vocoder at batch size): 130 VGPRs are three waves per SIMD, 127 are four — 42.5 -> 38.2 us per launch.  (The IEEE-half
    // instantiation needs 184 and would spill: it keeps the plain kernel.)
    f.occ4 = f.kernel == DW_V3 && f.K == 7 && f.R == 4 && f.out_dtype != F16;
    return f;
}

template <typename OutT>
static void launch_dwconv_ln_t(hipStream_t s, const DwconvLnForm& f, const float* x, int B, int L, int C, const float* w_t, const float* bias,
                               int k, int dil, const float* g, const float* b, float eps, OutT* y, const int* seqlen, const int* row_off,
                               const DwconvTail& tl) {
    const int64_t M = (int64_t)B * L;
    if (f.kernel == DW_V3) {
        if (f.K == 5 && f.R == 2) launch_dwconv_ln_v3_kr<OutT, 5, 2>(s, f.occ4, x, B, L, C, w_t, bias, dil, g, b, eps, y, seqlen, row_off, tl);
        else if (f.K == 5 && f.R == 4) launch_dwconv_ln_v3_kr<OutT, 5, 4>(s, f.occ4, x, B, L, C, w_t, bias, dil, g, b, eps, y, seqlen, row_off, tl);
        else if (f.K == 5 && f.R == 8) launch_dwconv_ln_v3_kr<OutT, 5, 8>(s, f.occ4, x, B, L, C, w_t, bias, dil, g, b, eps, y, seqlen, row_off, tl);
        else if (f.K == 7 && f.R == 4) launch_dwconv_ln_v3_kr<OutT, 7, 4>(s, f.occ4, x, B, L, C, w_t, bias, dil, g, b, eps, y, seqlen, row_off, tl);
        else throw std::logic_error("dwconv_ln: no v3 kernel for form " + f.str());
    } else if (f.kernel == DW_V2) {
        constexpr int R = 2;
        const dim3 grid((unsigned)((M + 4 * R - 1) / (4 * R)));
        if (f.K == 5) STN_KLAUNCH((dwconv_ln_v2_kernel<OutT, 5, R>), grid, dim3(256), 0, s, x, M, L, C, w_t, bias, dil, g, b, eps, y, seqlen);
        else if (f.K == 7) STN_KLAUNCH((dwconv_ln_v2_kernel<OutT, 7, R>), grid, dim3(256), 0, s, x, M, L, C, w_t, bias, dil, g, b, eps, y, seqlen);
        else throw std::logic_error("dwconv_ln: no v2 kernel for form " + f.str());
    } else {
        const dim3 grid((unsigned)((M + 3) / 4));
        STN_KLAUNCH((dwconv_ln_kernel<OutT, true>), grid, dim3(256), 0, s, x, M, L, C, w_t, bias, k, dil, g, b, eps, y, seqlen);
    }
}

void launch_dwconv_ln(hipStream_t s, int out_dtype, const float* x, int B, int L, int C, const float* w_t,
                      const float* bias, int k, int dil, const float* ln_g, const float* ln_b, float eps, void* y,
                      const int* seqlen, const int* row_off, const DwconvTail& tl) {
    check_ln_shape(C);
    if ((int64_t)B * L == 0) return;
    if (row_off && !seqlen) { throw std::invalid_argument("packed dwconv_ln needs lengths, C <= 512, k in {5,7}"); }
    if (tl.tail && (!row_off || tl.T < L || tl.rf < 0)) { throw std::invalid_argument("dwconv_ln: a tail table needs packed rows, T >= L and rf >= 0"); }
    const DwconvLnForm f = dwconv_ln_form(out_dtype, B, L, C, k, row_off != nullptr);  // the one place the thresholds live
    with_out_type(f.out_dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        launch_dwconv_ln_t(s, f, x, B, L, C, w_t, bias, k, dil, ln_g, ln_b, eps, static_cast<T*>(y), seqlen, row_off, tl);
    });
}

void launch_layernorm(hipStream_t s, int out_dtype, const float* x, int64_t M, int C, const float* g, const float* b,
                      float eps, void* y) {
    check_ln_shape(C);
    if (M == 0) return;
    const dim3 grid((unsigned)((M + 3) / 4));
    with_out_type(out_dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        STN_KLAUNCH((dwconv_ln_kernel<T, false>), grid, dim3(256), 0, s, x, M, 1, C, nullptr, nullptr, 1, 1, g, b, eps, static_cast<T*>(y),
                    static_cast<const int*>(nullptr));
    });
}

}  // namespace stn
