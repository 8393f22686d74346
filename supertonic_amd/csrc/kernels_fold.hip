// kernels_fold.hip — the K4-split fold (gfx950, wave64): the pending update of a K4-split launch (kernels_ffn.hip, kernels_xattn_hs.hip) folded into
// the residual stream by the kernel that reads x next, fused with LayerNorm (fold_ln) or with the depthwise conv + LayerNorm (fold_dwconv_ln).
// Device helpers: kernels_fold.hpp.  The instantiation and run length a fold_dwconv_ln call takes is ONE host decision, fold_dwconv_ln_form.
#include "kernels.hpp"
#include "kernels_dev.hpp"
#include "dev_env.hpp"
#include "kernels_fold.hpp"

#include <type_traits>
#include <stdio.h>
#include <stdlib.h>

namespace stn {

// ---------------------------------------------------------------------------------------------
// Folding the pending update of a K4-split launch (kernels_ffn.hip) into the residual stream, inside the kernel that reads x
// next anyway:   x_new = x + gamma * (((p0 + p1) + p2) + p3 + b2) + rowvec[seq]     (fp32, exactly this order in both kernels)
// Everything a thread loads is loaded unconditionally and as whole vectors (a per-element "pointer ? load : constant" makes hipcc
// branch around every load and wait for each one in turn: cdna_hip_programming.md, Projection GEMM item 4(c)); the optional
// time vector is a template parameter, the split count a compile-time constant.
// ---------------------------------------------------------------------------------------------
// fold + LayerNorm, one wavefront per row (rows are independent: x is updated in place)
template <typename OutT, bool F16, bool RV, int S>
__global__ __launch_bounds__(256) void fold_ln_kernel(float* __restrict__ x, int64_t M, int C, const uint16_t* __restrict__ part,
                                                      int64_t pstride, const float* __restrict__ b2, const float* __restrict__ gamma,
                                                      const float* __restrict__ rowvec, int rv_ld, const int* __restrict__ row_b,
                                                      const float* __restrict__ g, const float* __restrict__ bt, float eps, OutT* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;  // wave-uniform
    const int C4 = C >> 2;
    float4* x4 = reinterpret_cast<float4*>(x) + row * C4;
    const float4* rv4 = nullptr;
    if constexpr (RV) rv4 = reinterpret_cast<const float4*>(rowvec + (size_t)(row_b ? row_b[row] : 0) * rv_ld);
    const float4* b24 = reinterpret_cast<const float4*>(b2);
    const float4* gm4 = reinterpret_cast<const float4*>(gamma);
    float4 h[LN_NI];
#pragma unroll
    for (int i = 0; i < LN_NI; ++i) {
        const int c4 = lane + 64 * i;
        h[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c4 < C4) {
            const float4 xo = x4[c4];
            const float4 bb = b24[c4], gm = gm4[c4];
            float4 tv = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (RV) tv = rv4[c4];
            float acc[4];
            fold_sum<F16, 4, S>(part + (size_t)row * C + c4 * 4, pstride, acc);
            h[i] = fold_four(xo, acc, bb, gm, tv);
            x4[c4] = h[i];
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_NI; ++i) s += (h[i].x + h[i].y) + (h[i].z + h[i].w);
    const float mean = wave_sum(s) / (float)C;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < LN_NI; ++i)
        if (lane + 64 * i < C4) {
            const float dx = h[i].x - mean, dy = h[i].y - mean, dz = h[i].z - mean, dw = h[i].w - mean;
            v += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    const float rstd = rsqrtf(wave_sum(v) / (float)C + eps);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const float4* bt4 = reinterpret_cast<const float4*>(bt);
#pragma unroll
    for (int i = 0; i < LN_NI; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < C4) {
            const float4 gg = g4[c4], bb = bt4[c4];
            store4(y + row * C + c4 * 4, (h[i].x - mean) * rstd * gg.x + bb.x, (h[i].y - mean) * rstd * gg.y + bb.y,
                   (h[i].z - mean) * rstd * gg.z + bb.z, (h[i].w - mean) * rstd * gg.w + bb.w);
        }
    }
}

// A run-time value as a template argument: calls fn(std::integral_constant<int, V>) for the V among Vs that v equals; false when it equals none.
template <int... Vs, typename Fn>
static bool with_const(int v, Fn&& fn) {
    return ((v == Vs ? (fn(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

static void check_fold_args(const FoldArgs& f, int64_t M, int C, const char* who) {
    if (!f.part || (f.S != 4 && f.S != 8 && f.S != 12 && f.S != 24) || f.part_stride < M * C || !f.b2 || !f.gamma || (f.rowvec && f.rv_ld % 4) || (reinterpret_cast<uintptr_t>(f.part) & 15) ||
        (reinterpret_cast<uintptr_t>(f.b2) & 15) || (reinterpret_cast<uintptr_t>(f.gamma) & 15) || (f.rowvec && (reinterpret_cast<uintptr_t>(f.rowvec) & 15)))
        throw std::invalid_argument(std::string(who) + ": needs 16-byte aligned partial sums of 4, 8, 12 or 24 splits, b2 and gamma");
}

void launch_fold_ln(hipStream_t s, int act_dtype, float* x, int64_t M, int C, const FoldArgs& f, const float* g, const float* b, float eps, void* y) {
    check_ln_shape(C);
    if (M == 0) return;
    if (!is_half(act_dtype)) throw std::invalid_argument("launch_fold_ln: 16-bit activation format needed");
    check_fold_args(f, M, C, "launch_fold_ln");
    const dim3 grid((unsigned)((M + 3) / 4));
    const uint16_t* P = static_cast<const uint16_t*>(f.part);
    with_half_type(act_dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        with_const<0, 1>(f.rowvec != nullptr, [&](auto rv) {
            with_const<4, 8, 12, 24>(f.S, [&](auto S) {  // (check_fold_args admits no other)
                STN_KLAUNCH((fold_ln_kernel<T, std::is_same<T, f16_t>::value, rv() != 0, S()>), grid, dim3(256), 0, s, x, M, C, P, f.part_stride, f.b2, f.gamma,
                            f.rowvec, f.rv_ld, f.row_b, g, b, eps, static_cast<T*>(y));
            });
        });
    });
}

// fold + depthwise conv + LayerNorm on packed rows.  A workgroup (16 wavefronts) owns a run of consecutive frames of ONE sequence
// (a sequence is cut into ceil(len / 32) runs of equal length): it folds those frames and the (K-1)/2 * dil halo frames on either
// side into an fp32 LDS image (phase 1), runs the conv + LayerNorm out of LDS, one frame per half wavefront (phase 2), and writes
// the folded frames it owns to x_out.  x_out != x_in: the halo frames are folded again by the neighbouring workgroup from the
// same inputs.
// The kernel is a chain of memory latencies, not of bytes (one workgroup per CU, ~150 KB each): everything is arranged so that
// the chain is ONE global round trip long — the conv / LayerNorm parameters ride to LDS beside the phase-1 loads (no global load
// behind the barrier), nothing is stored to global memory before the barrier (a store in flight would be waited for there), and
// the x_out stores are the last thing a thread issues.
// Few sequences (a single utterance: two workgroups) are cut into runs of 8 frames instead: more workgroups, one pass of phase-1 loads each
// instead of two to four dependent ones; a frame's arithmetic does not depend on the run it falls in, so the result is the same bit for bit.
static constexpr int FOLD_TCH = 32, FOLD_TCH_FEW = 8, FOLD_TCH_MAX = 48, FOLD_NT = 1024;  // FOLD_TCH == 2 * wavefronts per workgroup (the longest run)
// window rows a thread of phase 1 loads per trip (the kernel's U; fold_dwconv_ln_form reports the same value)
constexpr int fold_phase1_rows(int S, int K, int nslot) { return S <= 4 ? (K == 5 && nslot <= 3 ? 3 : 2) : 1; }
template <typename OutT, bool F16, int K, bool RV, int FOLD_NSLOT /* float4 slots per lane of a half wavefront: ceil(C / 128) */, int S>
__global__ __launch_bounds__(FOLD_NT) void fold_dwconv_ln_kernel(const float* __restrict__ xin, float* __restrict__ xout, int cps, int C,
                                                                 const uint16_t* __restrict__ part, int64_t pstride,
                                                                 const float* __restrict__ b2, const float* __restrict__ gamma,
                                                                 const float* __restrict__ rowvec, int rv_ld, const float* __restrict__ w_t,
                                                                 const float* __restrict__ bias, int dil, const float* __restrict__ g,
                                                                 const float* __restrict__ bt, float eps, float inv_c, OutT* __restrict__ y,
                                                                 const int* __restrict__ seqlen, const int* __restrict__ row_off,
                                                                 unsigned long long* __restrict__ ts, int tch /* frames per run: FOLD_TCH or FOLD_TCH_FEW */) {
    extern __shared__ __attribute__((aligned(16))) float fold_sm[];
    unsigned long long st0 = 0, st1 = 0, st2 = 0;
    if (ts) st0 = __builtin_readcyclecounter();
    const int b = (int)blockIdx.x / cps, c = (int)blockIdx.x % cps;
    const int Lv = seqlen[b];
    const int64_t row0 = (int64_t)row_off[b];
    const int nch = (Lv + tch - 1) / tch;
    if (c >= nch) return;
    const int per = (Lv + nch - 1) / nch;
    const int t0 = c * per, t1 = min(t0 + per, Lv);
    if (t0 >= t1) return;
    constexpr int HALF = (K - 1) / 2;
    const int w0 = max(t0 - HALF * dil, 0), w1 = min(t1 + HALF * dil, Lv), nw = w1 - w0;
    const int tid = threadIdx.x, C8 = C >> 3, C4 = C >> 2;
    // the parameters of phase 2 as one LDS block behind the image: [K taps][C] | conv bias | LayerNorm g | LayerNorm b
    float* const zrow = fold_sm + (size_t)(tch + (K - 1) * dil) * C;  // a row of zeros: what a tap outside the sequence reads
    float* const wsm = zrow + C;
    constexpr int NPV = (K + 3 + 7) / 8;  // float4 per thread: (K + 3) * C4 <= NPV * FOLD_NT for C <= 512, K <= 7 ... checked by the launcher
    float4 pv[NPV];
#pragma unroll
    for (int i = 0; i < NPV; ++i) {
        const int q = tid + i * FOLD_NT;  // float4 index into the block
        const int seg = q / C4, c4 = q - seg * C4;
        const float* src = seg < K ? w_t + (size_t)seg * C : seg == K ? bias : seg == K + 1 ? g : bt;
        pv[i] = q < (K + 3) * C4 ? reinterpret_cast<const float4*>(src)[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ---- phase 1: a thread keeps ONE 8-channel group (its b2 / gamma / time-vector values are loaded once) and walks down the
    // window rows, `rpp` rows apart; every load of U rows is issued before the first use ----
    // Three rows per thread and trip when there are four partial sums: a run of 29 frames with a halo of 2 x 16 (dilation 8) is 61 rows = ONE trip of
    // 3 x 21 rows — one global round trip instead of two dependent ones.  The third row's loads are issued only by the threads that have one.
    // (the wider variants — C = 512, seven taps — keep two rows: three would spill; more splits: one row at a time, the partial sums in chunks of 12 loads)
    constexpr int U = fold_phase1_rows(S, K, FOLD_NSLOT);
    const int rpp = FOLD_NT / C8;  // rows per pass of the workgroup
    const int c8 = tid % C8, rq = tid / C8;
    if (rq < rpp) {
        const float4* bp = reinterpret_cast<const float4*>(b2 + c8 * 8);
        const float4* gp = reinterpret_cast<const float4*>(gamma + c8 * 8);
        const float4 bb0 = bp[0], bb1 = bp[1], gm0 = gp[0], gm1 = gp[1];
        float4 tv0 = make_float4(0.f, 0.f, 0.f, 0.f), tv1 = tv0;
        if constexpr (RV) { const float4* tp = reinterpret_cast<const float4*>(rowvec + (size_t)b * rv_ld + c8 * 8); tv0 = tp[0]; tv1 = tp[1]; }
        for (int r0 = rq; r0 < nw; r0 += rpp * U) {
            float4 xa[U][2];
            float acc[U][8];
            int64_t mrow[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int r = min(r0 + u * rpp, nw - 1);  // (past the end: the last row again, stored nowhere)
                mrow[u] = row0 + w0 + r;
            }
            if constexpr (U >= 2) {  // every load of all rows is issued before the first use
                constexpr int CH = S;
                uint4 w[U][CH];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float4* xp = reinterpret_cast<const float4*>(xin + mrow[u] * C + c8 * 8);
                    xa[u][0] = xp[0]; xa[u][1] = xp[1];
#pragma unroll
                    for (int sp = 0; sp < CH; ++sp) w[u][sp] = *reinterpret_cast<const uint4*>(part + (size_t)sp * pstride + (size_t)mrow[u] * C + c8 * 8);
                }
                if constexpr (U == 3) {
                    if (r0 + 2 * rpp < nw) {
                        const float4* xp = reinterpret_cast<const float4*>(xin + mrow[2] * C + c8 * 8);
                        xa[2][0] = xp[0]; xa[2][1] = xp[1];
#pragma unroll
                        for (int sp = 0; sp < CH; ++sp) w[2][sp] = *reinterpret_cast<const uint4*>(part + (size_t)sp * pstride + (size_t)mrow[2] * C + c8 * 8);
                    } else {
                        xa[2][0] = xa[2][1] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                        for (int sp = 0; sp < CH; ++sp) w[2][sp] = make_uint4(0u, 0u, 0u, 0u);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int sp = 0; sp < CH; ++sp) {
                        const unsigned wj[4] = {w[u][sp].x, w[u][sp].y, w[u][sp].z, w[u][sp].w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float lo = p16_to_f<F16>(wj[j] & 0xFFFFu), hi = p16_to_f<F16>(wj[j] >> 16);
                            if (sp == 0) { acc[u][2 * j] = lo; acc[u][2 * j + 1] = hi; }
                            else { acc[u][2 * j] += lo; acc[u][2 * j + 1] += hi; }
                        }
                    }
            } else {
                const float4* xp = reinterpret_cast<const float4*>(xin + mrow[0] * C + c8 * 8);
                xa[0][0] = xp[0]; xa[0][1] = xp[1];
                fold_sum<F16, 8, S>(part + (size_t)mrow[0] * C + c8 * 8, pstride, acc[0]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int r = r0 + u * rpp;
                if (r < nw) {
                    float4* sp4 = reinterpret_cast<float4*>(fold_sm + (size_t)r * C + c8 * 8);
                    sp4[0] = fold_four(xa[u][0], acc[u], bb0, gm0, tv0);
                    sp4[1] = fold_four(xa[u][1], acc[u] + 4, bb1, gm1, tv1);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NPV; ++i) {
        const int q = tid + i * FOLD_NT;
        if (q < (K + 3) * C4) reinterpret_cast<float4*>(wsm)[q] = pv[i];
    }
    if (tid < C4) reinterpret_cast<float4*>(zrow)[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ts) st1 = __builtin_readcyclecounter();
    __syncthreads();
    if (ts) st2 = __builtin_readcyclecounter();
    // ---- phase 2: one frame per HALF wavefront (32 lanes x FOLD_NSLOT float4 slots cover C): all of a run's <= 32 frames are done
    // in one pass of the 16 wavefronts, and the two LayerNorm reductions are 4 DPP steps + one swizzle over 32 lanes ----
    const int lane = tid & 63, l32 = lane & 31;
    const float4* ws4 = reinterpret_cast<const float4*>(wsm);
    for (int tp = t0; tp < t1; tp += FOLD_TCH) {  // (a run longer than 32 frames — run_frames 40 / 48 — takes a second pass)
    asm volatile("" ::: "memory");  // (keeps the pass's LDS reads of the taps and LayerNorm parameters inside it: hoisted, they would spill)
    const int t = tp + 2 * (tid >> 6) + (lane >> 5);
    const bool live = t < t1;
    const int tl = live ? t : t0;  // (a half wavefront beyond the run computes frame t0 again and stores nothing)
    float4 h[FOLD_NSLOT];
#pragma unroll
    for (int i = 0; i < FOLD_NSLOT; ++i) {
        const int c4 = l32 + 32 * i, cq = c4 < C4 ? c4 : 0;
        float4 a = ws4[K * C4 + cq];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int tt = tl + (j - HALF) * dil;
            const bool in = tt >= 0 && tt < Lv;  // (then w0 <= tt < w1)
            const float4 xv = *reinterpret_cast<const float4*>((in ? fold_sm + (size_t)(tt - w0) * C : zrow) + cq * 4);
            const float4 wv = ws4[j * C4 + cq];
            a.x = fmaf(wv.x, xv.x, a.x); a.y = fmaf(wv.y, xv.y, a.y);
            a.z = fmaf(wv.z, xv.z, a.z); a.w = fmaf(wv.w, xv.w, a.w);
        }
        h[i] = c4 < C4 ? a : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < FOLD_NSLOT; ++i) s += (h[i].x + h[i].y) + (h[i].z + h[i].w);
    const float mean = half_wave_sum(s) * inv_c;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < FOLD_NSLOT; ++i)
        if (l32 + 32 * i < C4) {
            const float dx = h[i].x - mean, dy = h[i].y - mean, dz = h[i].z - mean, dw = h[i].w - mean;
            v += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
    const float rstd = rsqrtf(half_wave_sum(v) * inv_c + eps);
    if (live) {
#pragma unroll
        for (int i = 0; i < FOLD_NSLOT; ++i) {
            const int c4 = l32 + 32 * i;
            if (c4 < C4) {
                const float4 gg = ws4[(K + 1) * C4 + c4], bb = ws4[(K + 2) * C4 + c4];
                store4(y + (row0 + t) * C + c4 * 4, (h[i].x - mean) * rstd * gg.x + bb.x, (h[i].y - mean) * rstd * gg.y + bb.y,
                       (h[i].z - mean) * rstd * gg.z + bb.z, (h[i].w - mean) * rstd * gg.w + bb.w);
            }
        }
    }
    }
    // ---- the folded frames this run owns -> x_out (each thread: the image rows it wrote itself) ----
    if (rq < rpp)
        for (int r = rq; r < nw; r += rpp) {
            const int tt = w0 + r;
            if (tt >= t0 && tt < t1) {
                const float4* sp4 = reinterpret_cast<const float4*>(fold_sm + (size_t)r * C + c8 * 8);
                float4* op = reinterpret_cast<float4*>(xout + (row0 + tt) * C + c8 * 8);
                op[0] = sp4[0]; op[1] = sp4[1];
            }
        }
    if (ts && tid == 0) {
        unsigned long long* tp = ts + (size_t)blockIdx.x * 4;
        tp[0] = st0; tp[1] = st1; tp[2] = st2; tp[3] = __builtin_readcyclecounter();
    }
}

int fold_run_frames(const int* lengths, int B, int n_cu) {
    if (!lengths || B <= 0 || n_cu <= 0) return 0;
    // The grid is B x ceil(Lmax / run): the runs a sequence does not have are workgroups too — they leave at once, but each takes a CU's LDS and 16
    // wave slots on the way (measured: 238 real workgroups in a grid of 336 run at the two-round time, 16.2 us; the same batch as 224 of 224: 13.2).
    // So the grid, not the number of real runs, is what is kept within whole rounds.
    int Lmax = 0;
    for (int i = 0; i < B; ++i) Lmax = std::max(Lmax, lengths[i]);
    // Only the clear case is acted on: a longer run that brings the whole grid into ONE round.  With several rounds either way the count of rounds stops
    // predicting the time (mixed lengths, 128 sequences of up to ~250 frames: runs of 48 = 3 rounds of grid measured 40.2 us against 37.6 for runs of
    // 32 = 4 rounds, half of them placeholders).
    if ((long)B * ((Lmax + FOLD_TCH - 1) / FOLD_TCH) <= n_cu) return 0;
    for (int tch = FOLD_TCH + 8; tch <= FOLD_TCH_MAX; tch += 8)
        if ((long)B * ((Lmax + tch - 1) / tch) <= n_cu) return tch;
    return 0;
}

static size_t fold_dwconv_lds(int C, int k, int dil, int tch = FOLD_TCH) { return ((size_t)(tch + (k - 1) * dil) + 1 + (size_t)(k + 3)) * C * 4; }  // image + zero row + parameter block
bool fold_dwconv_ln_supported(int C, int k, int dil) {
    return C % 8 == 0 && C <= 512 && (k == 5 || k == 7) && dil >= 1 && fold_dwconv_lds(C, k, dil) <= 160 * 1024;
}

std::string FoldDwconvLnForm::str() const {
    char m_[96];
    snprintf(m_, sizeof m_, "fold_dwconv_ln<%s,K%d,%s,ns%d,S%d,U%d> run %d cps %d", act_dtype == F16 ? "f16" : "bf16", K, rv ? "rv" : "norv", nslot, S, U, run, cps);
    return m_;
}

// force: the launcher's A/B switch (8, 32, 40 or 48; 0: none)
static FoldDwconvLnForm fold_dwconv_ln_form_forced(int act_dtype, int B, int L, int C, int k, int dil, int S, bool has_rowvec, int run_frames, int force) {
    if (!is_half(act_dtype) || B < 1 || L < 1 || !fold_dwconv_ln_supported(C, k, dil) || (S != 4 && S != 8 && S != 12 && S != 24) ||
        (int64_t)B * ((L + FOLD_TCH_FEW - 1) / FOLD_TCH_FEW) > 0x7FFFFFFFll)
        throw std::invalid_argument("fold_dwconv_ln: 16-bit format, k in {5,7}, C % 8 == 0, C <= 512, 4, 8, 12 or 24 splits and an image within 160 KiB of LDS needed");
    FoldDwconvLnForm f;
    f.act_dtype = act_dtype; f.K = k; f.rv = has_rowvec; f.S = S;
    f.nslot = C <= 384 ? 3 : 4;
    f.U = fold_phase1_rows(S, k, f.nslot);
    int tch = force == FOLD_TCH || force == FOLD_TCH_FEW ? force : (int64_t)B * ((L + FOLD_TCH - 1) / FOLD_TCH) < 64 ? FOLD_TCH_FEW : FOLD_TCH;
    if ((force == 40 || force == 48) && fold_dwconv_lds(C, k, dil, force) <= 160 * 1024) tch = force;
    if (!force && tch == FOLD_TCH && run_frames > FOLD_TCH && run_frames <= FOLD_TCH_MAX && run_frames % 8 == 0 && fold_dwconv_lds(C, k, dil, run_frames) <= 160 * 1024)
        tch = run_frames;  // fewer rounds of workgroups for these lengths (fold_run_frames)
    f.run = tch;
    f.cps = (L + tch - 1) / tch;
    f.grid = (unsigned)((int64_t)B * f.cps);
    f.lds = fold_dwconv_lds(C, k, dil, tch);
    return f;
}
FoldDwconvLnForm fold_dwconv_ln_form(int act_dtype, int B, int L, int C, int k, int dil, int S, bool has_rowvec, int run_frames) {
    return fold_dwconv_ln_form_forced(act_dtype, B, L, C, k, dil, S, has_rowvec, run_frames, 0);
}

// one instantiation: its LDS opt-in (once per device), the check that it is the kernel the form names, the launch
template <typename OutT, int K, bool RV, int NSLOT, int S>
static void launch_fold_dwconv_ln_one(hipStream_t s, const FoldDwconvLnForm& fm, const float* x_in, float* x_out, int C, const FoldArgs& f, const float* w_t,
                                      const float* bias, int dil, const float* g, const float* b, float eps, OutT* y, const int* seqlen, const int* row_off) {
    constexpr bool F16 = std::is_same<OutT, f16_t>::value;
    static PerDeviceOnce attr_once;
    if (attr_once.need())
        stn_check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&fold_dwconv_ln_kernel<OutT, F16, K, RV, NSLOT, S>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          160 * 1024), "hipFuncSetAttribute(fold_dwconv_ln)");
    if (fm.K != K || fm.rv != RV || fm.nslot != NSLOT || fm.S != S || fm.U != fold_phase1_rows(S, K, NSLOT)) throw std::logic_error("fold_dwconv_ln: no kernel for form " + fm.str());
    STN_KLAUNCH((fold_dwconv_ln_kernel<OutT, F16, K, RV, NSLOT, S>), dim3(fm.grid), dim3(FOLD_NT), fm.lds, s, x_in, x_out, fm.cps, C,
                static_cast<const uint16_t*>(f.part), f.part_stride, f.b2, f.gamma, f.rowvec, f.rv_ld, w_t, bias, dil, g, b, eps, 1.0f / (float)C, y, seqlen, row_off, f.ts, fm.run);
}

void launch_fold_dwconv_ln(hipStream_t s, int act_dtype, const float* x_in, float* x_out, int B, int L, int C, const FoldArgs& f, const float* w_t,
                           const float* bias, int k, int dil, const float* ln_g, const float* ln_b, float eps, void* y, const int* seqlen,
                           const int* row_off) {
    if (B == 0 || L == 0) return;
    if (!is_half(act_dtype) || !seqlen || !row_off || x_in == x_out || !fold_dwconv_ln_supported(C, k, dil) ||
        (int64_t)B * ((L + FOLD_TCH_FEW - 1) / FOLD_TCH_FEW) > 0x7FFFFFFFll)
        throw std::invalid_argument("launch_fold_dwconv_ln: packed 16-bit rows, separate output, k in {5,7}, C % 8 == 0, C <= 512 needed");
    check_fold_args(f, 0, C, "launch_fold_dwconv_ln");
    static const int force = [] { const char* e = stn::dev_env("STN_FOLD_TCH"); return e ? atoi(e) : 0; }();  // A/B switch: 8, 32, 40 or 48
    const FoldDwconvLnForm fm = fold_dwconv_ln_form_forced(act_dtype, B, L, C, k, dil, f.S, f.rowvec != nullptr, f.run_frames, force);  // the one place the run length is chosen
    // the form's five run-time values -> one of the 2 x 2 x 2 x 2 x 4 instantiations
    bool found = false;
    with_half_type(act_dtype, [&](auto* tag) {
    with_const<5, 7>(fm.K, [&](auto K) {
    with_const<0, 1>(fm.rv, [&](auto rv) {
    with_const<3, 4>(fm.nslot, [&](auto ns) {
    found = with_const<4, 8, 12, 24>(fm.S, [&](auto S) {
        using T = std::remove_pointer_t<decltype(tag)>;
        launch_fold_dwconv_ln_one<T, K(), rv() != 0, ns(), S()>(s, fm, x_in, x_out, C, f, w_t, bias, dil, ln_g, ln_b, eps, static_cast<T*>(y), seqlen, row_off);
    }); }); }); }); });
    if (!found) throw std::logic_error("fold_dwconv_ln: no kernel for form " + fm.str());
}

}  // namespace stn
