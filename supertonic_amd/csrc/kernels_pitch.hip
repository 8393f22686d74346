// kernels_pitch.hip — time-scale modification of the finished waveform (gfx950, wave64): WSOLA with a normalised search, the first half
// of the fetch-time pitch shift (the second half is the polyphase resampler, kernels_resample.hip).  Runs outside
// the captured pipeline: rows x W fp32 at rate fs -> rows x Ws, Ws = ceil(W a / b), the same pitch at a / b times the duration.
//
// Geometry (pitch_plan, host/pitch.cpp): hop H, grain N = 2 H, search radius D = 3 H / 4.  Frame m is analysed at p_m = floor(m H b / a)
// and its grain starts at q_m = p_m + d_m - H; d_0 = 0 and, for m >= 1, d_m is the offset in [-D, D] whose grain correlates best with the
// target t[i] = x[q_{m-1} + H + i], the previous grain's natural continuation: score(d) = c(d) / sqrt(E(d) + 1e-9), c the dot product
// with the target and E the candidate's energy over the N samples.  Equal scores: the smallest |d|, then the negative one.  A read
// outside the row's span [0, n) is 0.0f whatever the memory holds.
//
// pitch_search_kernel: a row's frames are a dependent chain (the target of frame m needs d_{m-1}) and rows are independent, so one
// workgroup owns a row and loops over its frames.  Per frame the target (N floats) and the candidate region (N + 2 D floats from
// p_m - D - H) lie in LDS; a thread owns candidate d = tid - D and walks the region from its own offset (stride 1 across the lanes of a
// ds_read_b32: no bank conflict) against the target (one address for the wave: a broadcast), accumulating c and E in the same loop.  The
// arg-max is a shuffle reduction per wave, one LDS slot per wave, and every thread folds the slots in the same order.  The region of
// frame m + 1 depends on p_{m+1} only: its global loads are issued before the dot products of frame m and land in the second LDS
// buffer behind the reduction.
// pitch_ola_kernel: one thread per output sample, y[m H + i] = w[H + i] x[q_m + H + i] + w[i] x[q_{m+1} + i] from the table of offsets,
// and 0.0f from the end of the row's stretched span, ceil(n a / b), on.
#include "kernels.hpp"

namespace stn {

namespace {

constexpr int PS_MAX_THREADS = 1024;
constexpr int PS_PF = 7;  // region floats a thread carries across a frame's reduction: ceil(3.5 H / threads) <= 7 up to H = 2048

// a row's sample t, 0.0f outside its span [0, nr): the address is clamped into the row (W >= 1) so that the load never waits behind a branch
__device__ __forceinline__ float ps_read(const float* __restrict__ xr, int64_t W, int64_t nr, int64_t t) {
    const float e = xr[t < 0 ? 0 : (t >= W ? W - 1 : t)];
    return (t >= 0 && t < nr) ? e : 0.0f;
}

// the order of the arg-max: the larger score, then the smaller |d|, then the negative d
__device__ __forceinline__ bool ps_better(float s1, int d1, float s2, int d2) {
    if (s1 != s2) return s1 > s2;
    const int a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2;
    return a1 < a2 || (a1 == a2 && d1 < d2);
}

__device__ __forceinline__ int64_t ps_pos(int64_t m, int H, int a, int b) { return m * H * b / a; }

__global__ void __launch_bounds__(PS_MAX_THREADS) pitch_search_kernel(const float* __restrict__ x, int64_t W, const int64_t* __restrict__ n, int H, int64_t M,
                                                                      int a, int b, int* __restrict__ delta, float* __restrict__ score) {
    extern __shared__ float ps_lds[];
    const int N = 2 * H, D = 3 * H / 4, R = N + 2 * D, C = 2 * D + 1;
    float* tgt = ps_lds;
    float* regs = ps_lds + N;  // two regions of R floats
    float* red_s = ps_lds + N + 2 * R;
    int* red_d = reinterpret_cast<int*>(red_s + PS_MAX_THREADS / 64);
    const int64_t row = blockIdx.x;
    const float* __restrict__ xr = x + row * W;
    int64_t nr = n ? n[row] : W;
    nr = nr < 0 ? 0 : (nr > W ? W : nr);
    const int T = (int)blockDim.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
    if (tid == 0) { delta[row * M] = 0; score[row * M] = 0.0f; }
    if (M > 1) {
        const int64_t r0 = ps_pos(1, H, a, b) - D - H;
        for (int i = tid; i < R; i += T) regs[i] = ps_read(xr, W, nr, r0 + i);
    }
    int cur = 0, dprev = 0;
    for (int64_t m = 1; m < M; ++m) {
        const int64_t t0 = ps_pos(m - 1, H, a, b) + dprev;  // q_{m-1} + H
        for (int i = tid; i < N; i += T) tgt[i] = ps_read(xr, W, nr, t0 + i);
        // the next frame's region: in flight under this frame's dot products
        float pf[PS_PF];
        const bool more = m + 1 < M;
        const int64_t r1 = ps_pos(m + 1, H, a, b) - D - H;
#pragma unroll
        for (int k = 0; k < PS_PF; ++k) {
            const int i = k * T + tid;
            pf[k] = (more && i < R) ? ps_read(xr, W, nr, r1 + i) : 0.0f;
        }
        __syncthreads();
        float bs = -INFINITY;
        int bd = 0;
        for (int cnd = tid; cnd < C; cnd += T) {
            const float* xs = regs + cur * R + cnd;
            float c0 = 0.f, c1 = 0.f, e0 = 0.f, e1 = 0.f;
            for (int i = 0; i < N; i += 4) {
                const float4 t = *reinterpret_cast<const float4*>(tgt + i);
                const float x0 = xs[i], x1 = xs[i + 1], x2 = xs[i + 2], x3 = xs[i + 3];
                c0 = __builtin_fmaf(t.x, x0, c0); e0 = __builtin_fmaf(x0, x0, e0);
                c1 = __builtin_fmaf(t.y, x1, c1); e1 = __builtin_fmaf(x1, x1, e1);
                c0 = __builtin_fmaf(t.z, x2, c0); e0 = __builtin_fmaf(x2, x2, e0);
                c1 = __builtin_fmaf(t.w, x3, c1); e1 = __builtin_fmaf(x3, x3, e1);
            }
            float s = (c0 + c1) / sqrtf((e0 + e1) + 1e-9f);
            if (!(s == s)) s = -INFINITY;  // (a NaN inside the span: never the winner, whatever the order of the comparisons)
            const int d = cnd - D;
            if (ps_better(s, d, bs, bd)) { bs = s; bd = d; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o, 64);
            const int od = __shfl_xor(bd, o, 64);
            if (ps_better(os, od, bs, bd)) { bs = os; bd = od; }
        }
        if (lane == 0) { red_s[wave] = bs; red_d[wave] = bd; }
        __syncthreads();
        bs = red_s[0]; bd = red_d[0];
        for (int v = 1; v < waves; ++v) {
            const float os = red_s[v];
            const int od = red_d[v];
            if (ps_better(os, od, bs, bd)) { bs = os; bd = od; }
        }
        if (tid == 0) { delta[row * M + m] = bd; score[row * M + m] = bs; }
#pragma unroll
        for (int k = 0; k < PS_PF; ++k) {
            const int i = k * T + tid;
            if (more && i < R) regs[(cur ^ 1) * R + i] = pf[k];
        }
        __syncthreads();  // the next region is whole, and the slots and the target may be written again
        cur ^= 1;
        dprev = bd;
    }
}

__global__ void __launch_bounds__(256) pitch_ola_kernel(const float* __restrict__ x, int64_t W, const int64_t* __restrict__ n, int H, int64_t M, int64_t Ws,
                                                        int a, int b, const int* __restrict__ delta, const float* __restrict__ win, float* __restrict__ y) {
    const int64_t row = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Ws) return;
    const float* __restrict__ xr = x + row * W;
    int64_t nr = n ? n[row] : W;
    nr = nr < 0 ? 0 : (nr > W ? W : nr);
    const int64_t m = j / H;
    const int i = (int)(j - m * H);
    const int64_t q0 = ps_pos(m, H, a, b) + delta[row * M + m] - H;
    const int64_t q1 = ps_pos(m + 1, H, a, b) + delta[row * M + m + 1] - H;  // (m + 1 <= Ws / H + 1 = M - 1)
    const float u = win[H + i] * ps_read(xr, W, nr, q0 + H + i);
    const float v = win[i] * ps_read(xr, W, nr, q1 + i);
    // the stretched row ends with its span, ceil(n a / b): what the last grains leave behind it would reach the resampler in a wide
    // batch and not in a narrow one
    y[row * Ws + j] = j < (nr * a + b - 1) / b ? u + v : 0.0f;
}

int ps_threads(int H) {
    const int C = 2 * (3 * H / 4) + 1;
    return std::min(PS_MAX_THREADS, (C + 63) / 64 * 64);
}

void ps_check(const char* who, int64_t rows, int64_t W, int H, int64_t M, int a, int b) {
    if (rows < 1 || W < 1) throw std::invalid_argument(std::string(who) + ": no rows");
    if (H < 64 || H > 2048 || (H & (H - 1)) != 0) throw std::invalid_argument(std::string(who) + ": H must be a power of two in [64, 2048]");
    if (a < 1 || b < 1 || a > 640 || b > 640) throw std::invalid_argument(std::string(who) + ": a and b must be in [1, 640]");
    if (M != ((W * a + b - 1) / b) / H + 2) throw std::invalid_argument(std::string(who) + ": M is not the plan's frame count");
}

}  // namespace

void launch_pitch_search(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, int H, int64_t M, int a, int b, int* delta, float* score) {
    ps_check("launch_pitch_search", rows, W, H, M, a, b);
    if (rows > 0x7fffffff) throw std::invalid_argument("launch_pitch_search: too many rows");
    const int threads = ps_threads(H);
    const int N = 2 * H, R = N + 2 * (3 * H / 4);
    if ((R + threads - 1) / threads > PS_PF) throw std::logic_error("launch_pitch_search: the region does not fit the prefetch registers");
    const size_t lds = (size_t)(N + 2 * R + 2 * (PS_MAX_THREADS / 64)) * sizeof(float);
    static PerDeviceOnce attr_once;
    if (attr_once.need())
        stn_check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&pitch_search_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024),
                      "hipFuncSetAttribute(pitch_search)");
    STN_KLAUNCH(pitch_search_kernel, dim3((unsigned)rows), dim3((unsigned)threads), (unsigned)lds, s, x, W, n, H, M, a, b, delta, score);
}

void launch_pitch_ola(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, int H, int64_t M, int64_t Ws, int a, int b, const int* delta,
                      const float* win, float* y) {
    ps_check("launch_pitch_ola", rows, W, H, M, a, b);
    if (Ws != (W * a + b - 1) / b) throw std::invalid_argument("launch_pitch_ola: Ws is not the plan's width");
    if (rows > 65535) throw std::invalid_argument("launch_pitch_ola: more than 65535 rows");
    STN_KLAUNCH(pitch_ola_kernel, dim3((unsigned)((Ws + 255) / 256), (unsigned)rows), dim3(256), 0, s, x, W, n, H, M, Ws, a, b, delta, win, y);
}

}  // namespace stn
