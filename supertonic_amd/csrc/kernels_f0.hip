// kernels_f0.hip — the pitch report: a YIN fundamental-frequency track of every row and its statistics (gfx950, wave64).  Runs when a
// report is asked for, outside the captured pipeline, on rows x W fp32 samples of which row b's first n_b count.  include/stn.h "f0"
// has the contract (host/f0.cpp is its float64 rule), DESIGN.md section 27 the decomposition, the LDS layout and the error bound.
//
//   1. f0_track_kernel: a workgroup owns F0_GROUP consecutive frames of one row.  It box-averages (in double, rounded once) and stages
//      their (cnt - 1) Hh + 2 tau_max analysis samples in LDS once.  A wave owns every fourth frame of the group, and a lane one lag at
//      a time: d(tau) = sum_j (u[s+j] - u[s+j+tau])^2 reads u[s+j] as a wave-wide broadcast and u[s+j+tau] at stride 1 across the
//      lanes (no bank conflict), the terms added in the order of j.  The running sum over tau is a wave scan per tile of 64 lags plus
//      the carry of the tiles before it, in tile order.  The first lag under the threshold and the end of the walk are ballots over
//      tiles in ascending order: the smallest lag wins, so no two candidates tie.  Lane 0 refines in double.
//   2. f0_stats_kernel: one workgroup per row.  The voiced frames' f0 are the sort keys (+inf for the others and the padding), so the
//      ascending bitonic sort (kernels_sort.hpp) leaves them in front: minimum, lower median and maximum are read there.  The log2 sum
//      runs in double in a fixed order (lane-strided partials, a butterfly per wave, the waves in order).
// No atomics; a frame's result depends on its own 2 tau_max k samples only, a row's statistics on its own track only.
#include "kernels.hpp"
#include "kernels_sort.hpp"
#include "stn.h"

#include <math.h>

namespace stn {

namespace {

constexpr int F0_WAVES = F0_WG / 64;
static_assert(F0_GROUP % F0_WAVES == 0, "every wave owns the same number of frames of a group");
static_assert(sizeof(stn_f0_stats) == 24, "the stats kernel stores the struct whole");

__device__ __forceinline__ int64_t f0_row_frames(int64_t n, int k, int hop, int T) {
    const int64_t na = n / k;
    return na < 2 * (int64_t)T ? 0 : (na - 2 * (int64_t)T) / hop + 1;
}

// LDS: win[(F0_GROUP - 1) hop + 2 T] (the group's analysis samples), then dd[F0_GROUP][T + 1] (a frame's d, then in place its d')
__global__ void __launch_bounds__(F0_WG) f0_track_kernel(const float* __restrict__ x, int64_t W, const int64_t* __restrict__ nrow, int k, int hop,
                                                         int tmin, int T, float thr, double ha, double gate_ms, int64_t maxF, int64_t fstride,
                                                         float* __restrict__ f0, float* __restrict__ ap) {
    extern __shared__ float f0_lds[];
    float* win = f0_lds;
    float* dd = f0_lds + (F0_GROUP - 1) * hop + 2 * T;
    const int64_t row = blockIdx.y;
    const int64_t g0 = (int64_t)blockIdx.x * F0_GROUP;
    const int64_t F = f0_row_frames(nrow[row], k, hop, T);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* __restrict__ fr = f0 + row * fstride;
    float* __restrict__ ar = ap + row * fstride;
    if (tid < F0_GROUP) {  // the columns behind the row's frames, up to the longest row's count
        const int64_t t = g0 + tid;
        if (t >= F && t < maxF) { fr[t] = 0.0f; ar[t] = 1.0f; }
    }
    if (g0 >= F) return;  // (the whole workgroup)
    const int cnt = (int)(F - g0 < F0_GROUP ? F - g0 : F0_GROUP);
    const int len = (cnt - 1) * hop + 2 * T;  // (the group's last frame ends inside n / k: nothing behind the span is read)
    const float* __restrict__ xr = x + row * W + g0 * hop * k;
    for (int j = tid; j < len; j += F0_WG) {
        const float* p = xr + (int64_t)j * k;
        double a = 0.0;
        for (int i = 0; i < k; ++i) a += (double)p[i];
        win[j] = (float)(a / (double)k);  // (k = 1: the sample itself)
    }
    __syncthreads();
    for (int gi = 0; gi < F0_GROUP / F0_WAVES; ++gi) {  // (every wave takes every barrier, with or without a frame)
        const int g = gi * F0_WAVES + wave;
        const bool active = g < cnt;
        const float* w = win + g * hop;
        float* d = dd + g * (T + 1);
        float e = 0.0f;
        if (active) {
            for (int tb = 0; tb <= T; tb += 64) {
                const int tau = tb + lane;
                if (tau <= T) {
                    const float* wt = w + tau;
                    float acc = 0.0f;
#pragma unroll 4
                    for (int j = 0; j < T; ++j) { const float v = w[j] - wt[j]; acc += v * v; }
                    d[tau] = acc;
                }
            }
            for (int j = lane; j < T; j += 64) e += w[j] * w[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
        }
        __syncthreads();
        if (active) {  // d'(tau) in place: a lane reads and writes its own lag only
            float carry = 0.0f;
            for (int tb = 1; tb <= T; tb += 64) {
                const int tau = tb + lane;
                const float dv = tau <= T ? d[tau] : 0.0f;
                float v = dv;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const float u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
                const float c = carry + v;
                if (tau <= T) d[tau] = c > 0.0f ? dv * (float)tau / c : 1.0f;
                carry = __shfl(c, 63, 64);
            }
            if (lane == 0) d[0] = 1.0f;
        }
        __syncthreads();
        if (active) {
            int lag = 0;
            if (!((double)e / (double)T < gate_ms)) {
                for (int tb = tmin; tb < T && !lag; tb += 64) {  // the smallest lag under the threshold
                    const int tau = tb + lane;
                    const unsigned long long m = __ballot(tau < T && d[tau] < thr);
                    if (m) lag = tb + __ffsll(m) - 1;
                }
                if (lag) {  // the walk: the first lag at or behind it that has no smaller right neighbour (tau = T - 1 ends it)
                    for (int tb = lag;; tb += 64) {
                        const int tau = tb + lane;
                        const unsigned long long m = __ballot(tau < T && (tau + 1 >= T || !(d[tau + 1] < d[tau])));
                        if (m) { lag = tb + __ffsll(m) - 1; break; }
                    }
                }
            }
            if (lane == 0) {
                float f = 0.0f, b = 1.0f;
                if (lag) {
                    b = d[lag];
                    const double a = d[lag - 1], c = d[lag + 1], den = a - 2.0 * (double)b + c;
                    double off = 0.0;
                    if (den > 0.0) off = fmin(1.0, fmax(-1.0, 0.5 * (a - c) / den));
                    f = (float)(ha / ((double)lag + off));
                }
                fr[g0 + g] = f;
                ar[g0 + g] = b;
            }
        }
    }
}

// fixed-order sum over the workgroup: a butterfly per wave, the waves in order
__device__ double f0_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < F0_STATS_WG / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

// LDS: key[P], P the power of two at or above the row's frame count
__global__ void __launch_bounds__(F0_STATS_WG) f0_stats_kernel(const float* __restrict__ f0, const int64_t* __restrict__ nrow, int k, int hop, int T,
                                                               int keycap, int64_t fstride, stn_f0_stats* __restrict__ stats) {
    extern __shared__ float f0_key[];
    __shared__ double red[F0_STATS_WG / 64];
    const int64_t row = blockIdx.x;
    int64_t F = f0_row_frames(nrow[row], k, hop, T);
    if (F > keycap) F = keycap;  // (never taken: the launcher sized the LDS by the longest row)
    const float* __restrict__ fr = f0 + row * fstride;
    const int tid = threadIdx.x;
    int P = 1;
    while (P < F) P <<= 1;
    double cnt = 0.0, lg = 0.0;
    for (int j = tid; j < P; j += F0_STATS_WG) {
        const float v = j < F ? fr[j] : 0.0f;
        const bool voiced = v > 0.0f;
        f0_key[j] = voiced ? v : INFINITY;
        if (voiced) { cnt += 1.0; lg += log2((double)v); }
    }
    cnt = f0_block_sum(cnt, red);  // (its barriers also order the keys before the sort's reads)
    lg = f0_block_sum(lg, red);
    lds_bitonic_sort<F0_STATS_WG>(f0_key, P);
    if (tid == 0) {
        const int nv = (int)cnt;
        stn_f0_stats s;
        s.frames = (int32_t)F;
        s.voiced = nv;
        s.median_hz = nv ? f0_key[(nv - 1) / 2] : 0.0f;
        s.mean_hz = nv ? (float)exp2(lg / (double)nv) : 0.0f;
        s.min_hz = nv ? f0_key[0] : 0.0f;
        s.max_hz = nv ? f0_key[nv - 1] : 0.0f;
        stats[row] = s;
    }
}

void f0_check_launch(int64_t rows, const F0Launch& g, int64_t max_frames, int64_t fstride) {
    if (rows > 65535) throw std::invalid_argument("f0: more than 65535 rows");
    if (g.k < 1 || g.hop < 1 || g.hop > 320 || g.tau_min < 2 || g.tau_min >= g.tau_max || g.tau_max > F0_MAX_TAU)
        throw std::invalid_argument("f0: geometry outside the kernels' limits");
    if (max_frames > fstride) throw std::invalid_argument("f0: the track buffer is shorter than the longest row");
    const std::string why = f0_frames_check(-1, max_frames);
    if (!why.empty()) throw std::invalid_argument(why);
}

}  // namespace

std::string f0_frames_check(int64_t row, int64_t frames) {
    if (frames <= F0_MAX_FRAMES) return "";
    return "f0: " + (row >= 0 ? "row " + std::to_string(row) : std::string("a row")) + " holds " + std::to_string(frames) +
           " frames, and the report takes at most " + std::to_string(F0_MAX_FRAMES);
}

void launch_f0_track(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, const F0Launch& g, int64_t max_frames, int64_t fstride,
                     float* f0, float* ap) {
    if (rows <= 0 || W <= 0 || max_frames <= 0) return;
    f0_check_launch(rows, g, max_frames, fstride);
    const unsigned lds = (unsigned)(((F0_GROUP - 1) * g.hop + 2 * g.tau_max + F0_GROUP * (g.tau_max + 1)) * sizeof(float));  // at most 51672 bytes
    const dim3 grid((unsigned)((max_frames + F0_GROUP - 1) / F0_GROUP), (unsigned)rows);
    STN_KLAUNCH(f0_track_kernel, grid, dim3(F0_WG), lds, s, x, W, n, g.k, g.hop, g.tau_min, g.tau_max, g.threshold, g.ha, g.gate_ms, max_frames, fstride,
                f0, ap);
}

void launch_f0_stats(hipStream_t s, const float* f0, int64_t rows, int64_t W, const int64_t* n, const F0Launch& g, int64_t max_frames, int64_t fstride,
                     void* stats) {
    if (rows <= 0 || W <= 0) return;
    f0_check_launch(rows, g, max_frames, fstride);
    int P = 1;
    while (P < max_frames) P <<= 1;
    static PerDeviceOnce attr_once;
    if (attr_once.need())
        stn_check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&f0_stats_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)(F0_MAX_FRAMES * sizeof(float))), "hipFuncSetAttribute(f0_stats)");
    STN_KLAUNCH(f0_stats_kernel, dim3((unsigned)rows), dim3(F0_STATS_WG), (unsigned)(P * sizeof(float)), s, f0, n, g.k, g.hop, g.tau_max, P, fstride,
                static_cast<stn_f0_stats*>(stats));
}

}  // namespace stn
