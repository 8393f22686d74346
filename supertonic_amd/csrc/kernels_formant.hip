// kernels_formant.hip — formant correction of pitch-shifted rows (gfx950, wave64): the spectral envelope of the
// row before the shift (x) put back onto the shifted row (y).  Runs outside the captured pipeline, behind the pitch stage's resample.
//
// Geometry (formant_plan, host/formant.cpp): the pitch stage's hop H and window w (periodic Hann, N = 2 H), frames m = 0 .. ceil(W / H)
// at s_m = (m - 1) H, order p <= 48.  A read outside a row's span [0, n) is 0.0f whatever the memory holds.
//
// formant_lpc_kernel: one workgroup of two waves per (row, frame), wave 0 on x and wave 1 on y.  The windowed frame (one fp32 product
// per sample) lies in LDS; lane k accumulates lag k in double (the frame at i: one address for the wave, a broadcast; at i + k: stride 1
// across the lanes), conditions it (1.0001 R[0] + 1e-9, the lag window) and the wave runs Levinson-Durbin in double in the same launch:
// every lane forms the step's dot product in the same order from LDS, lane j updates a[j].  Behind a barrier both errors are known:
// g = clamp(sqrt(E_x / E_y), 1/2, 2), wave 0 stores ax = fl32(a_x), wave 1 cy = fl32(g a_y).
//
// formant_filter_kernel: a thread per (hop, side).  Output hop h is w[H + i] v_h + w[i] v_{h+1}: the even lane of a pair runs frame h
// and the odd lane frame h + 1, each the whole chain of its frame's filter g A_y / A_x from zero state at s_m - N, with the p last
// inputs and outputs and the 2 p + 1 coefficients in registers (a ring of P slots, the loop body unrolled P times so that every index
// is a constant; P = 16, 32 or 48 with zero coefficients behind p).  The lanes of a wave walk the same distance in front of their hop's
// end, so the odd lane, whose frame starts H later, and the first samples of every chain, which round the length up to a multiple of
// P, see the input masked to 0.0f and hold an all-zero state until their frame begins.  Over the last H samples the pair exchanges
// its weighted outputs through one cross-lane read and the even lane stores.  The recursion's sum runs from tap p down to tap 1, so
// that the newest output enters last and one fused multiply-add separates a sample from the next.  No frame buffer, no atomics; the
// hand-off from the tables to the filter is the launch boundary.
#include "kernels.hpp"

#include <type_traits>
#include <utility>

namespace stn {

namespace {

constexpr int FM_MAX_P = 48;
constexpr int FM_P1 = FM_MAX_P + 1;

// a row's sample t, 0.0f outside its span [0, nr): the address is clamped into the row (W >= 1), as the pitch kernels read
__device__ __forceinline__ float fm_read(const float* __restrict__ xr, int64_t W, int64_t nr, int64_t t) {
    const float e = xr[t < 0 ? 0 : (t >= W ? W - 1 : t)];
    return (t >= 0 && t < nr) ? e : 0.0f;
}

__global__ void __launch_bounds__(128) formant_lpc_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t W, const int64_t* __restrict__ n,
                                                          int H, int64_t F, int p, const float* __restrict__ win, const double* __restrict__ lagw,
                                                          float* __restrict__ ax, float* __restrict__ cy, double* __restrict__ g, double* __restrict__ ex,
                                                          double* __restrict__ ey) {
    extern __shared__ double fm_lds[];
    const int N = 2 * H;
    const int tid = (int)threadIdx.x, lane = tid & 63, sig = tid >> 6;
    double* rr = fm_lds + sig * 2 * FM_P1;  // the conditioned lags and the polynomial of this wave's signal
    double* aa = rr + FM_P1;
    double* ee = fm_lds + 4 * FM_P1;        // the two final errors
    float* xw = reinterpret_cast<float*>(fm_lds + 4 * FM_P1 + 2) + sig * N;
    const int64_t row = blockIdx.y, m = blockIdx.x;
    const float* __restrict__ src = (sig ? y : x) + row * W;
    int64_t nr = n ? n[row] : W;
    nr = nr < 0 ? 0 : (nr > W ? W : nr);
    const int64_t s0 = (m - 1) * H;
    for (int i = lane; i < N; i += 64) xw[i] = win[i] * fm_read(src, W, nr, s0 + i);
    __syncthreads();
    if (lane <= p) {
        double acc = 0.0;
        const float* xs = xw + lane;
        for (int i = 0; i < N - lane; ++i) acc = __builtin_fma((double)xw[i], (double)xs[i], acc);  // (the product is exact in double)
        rr[lane] = lane == 0 ? 1.0001 * acc + 1e-9 : acc * lagw[lane];
        aa[lane] = lane == 0 ? 1.0 : 0.0;
    }
    __syncthreads();
    double E = rr[0];
    for (int i = 1; i <= p; ++i) {
        double acc = rr[i];
        for (int j = 1; j < i; ++j) acc += aa[j] * rr[i - j];
        const double k = -acc / E;
        const bool mine = lane >= 1 && lane < i;
        const double t = mine ? aa[lane] + k * aa[i - lane] : 0.0;
        __syncthreads();
        if (mine) aa[lane] = t;
        if (lane == i) aa[lane] = k;
        __syncthreads();
        E *= 1.0 - k * k;
    }
    if (lane == 0) ee[sig] = E;
    __syncthreads();
    double gg = sqrt(ee[0] / ee[1]);
    gg = gg < 0.5 ? 0.5 : (gg > 2.0 ? 2.0 : gg);
    const int64_t f = row * F + m;
    if (lane <= p) {
        if (sig == 0) ax[f * (p + 1) + lane] = (float)aa[lane];
        else cy[f * (p + 1) + lane] = (float)(gg * aa[lane]);
    }
    if (tid == 0) { g[f] = gg; ex[f] = ee[0]; ey[f] = ee[1]; }
}

template <int... S, class Fn>
__device__ __forceinline__ void fm_each(std::integer_sequence<int, S...>, Fn&& fn) {
    (fn(std::integral_constant<int, S>{}), ...);
}

template <int P>
__global__ void __launch_bounds__(64) formant_filter_kernel(const float* __restrict__ y, int64_t W, const int64_t* __restrict__ n, int H, int64_t F, int p,
                                                            const float* __restrict__ win, const float* __restrict__ ax, const float* __restrict__ cy,
                                                            float* __restrict__ out) {
    const int64_t row = blockIdx.y;
    const int64_t gt = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int side = (int)(gt & 1);
    int64_t hop = gt >> 1;
    const bool live = hop < F - 1;  // (the lanes behind the last hop walk it again and store nothing)
    if (!live) hop = F - 2;
    const int64_t f = hop + side;
    const float* __restrict__ yr = y + row * W;
    float* __restrict__ outr = out + row * W;
    int64_t nr = n ? n[row] : W;
    nr = nr < 0 ? 0 : (nr > W ? W : nr);
    const float* __restrict__ pa = ax + (row * F + f) * (p + 1);
    const float* __restrict__ pc = cy + (row * F + f) * (p + 1);
    float A[P + 1], C[P + 1], vh[P], yh[P];
#pragma unroll
    for (int k = 0; k <= P; ++k) {
        A[k] = k <= p ? pa[k] : 0.0f;
        C[k] = k <= p ? pc[k] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < P; ++k) { vh[k] = 0.0f; yh[k] = 0.0f; }
    const int64_t end = (hop + 1) * H;    // one past the hop's last sample
    const int64_t n0 = (f - 1 - 2) * H;   // s_f - N: where this lane's chain begins
    const int L = (4 * H + P - 1) / P * P;
    for (int r = -L; r < 0; r += P) {
        // (a fold over s = 0 .. P - 1 and not a loop: every ring index below must be a constant for the rings to stay in registers)
        fm_each(std::make_integer_sequence<int, P>{}, [&](auto sc) {
            constexpr int s = decltype(sc)::value;
            const int64_t j = end + r + s;
            float yj = fm_read(yr, W, nr, j);
            yj = j >= n0 ? yj : 0.0f;
            float e = C[0] * yj;
#pragma unroll
            for (int k = 1; k <= P; ++k) e = __builtin_fmaf(C[k], yh[(s - k + P) % P], e);
            float v = e;
#pragma unroll
            for (int k = P; k >= 1; --k) v = __builtin_fmaf(-A[k], vh[(s - k + P) % P], v);
            yh[s] = yj;
            vh[s] = v;
            const int i = r + s + H;  // the position inside the hop: the same in every lane
            if (i >= 0) {
                const float t = (side ? win[i] : win[H + i]) * v;
                const float o = __shfl_xor(t, 1, 64);
                if (live && side == 0 && j < W) outr[j] = j < nr ? t + o : 0.0f;
            }
        });
    }
}

void fm_check(const char* who, int64_t rows, int64_t W, int H, int64_t F, int p) {
    if (rows < 1 || W < 1) throw std::invalid_argument(std::string(who) + ": no rows");
    if (rows > 65535) throw std::invalid_argument(std::string(who) + ": more than 65535 rows");
    if (H < 64 || H > 2048 || (H & (H - 1)) != 0) throw std::invalid_argument(std::string(who) + ": H must be a power of two in [64, 2048]");
    if (F != (W + H - 1) / H + 1 || F > 0x7fffffff) throw std::invalid_argument(std::string(who) + ": F is not the plan's frame count");
    if (p < 1 || p > FM_MAX_P) throw std::invalid_argument(std::string(who) + ": p must be in [1, 48]");
}

}  // namespace

void launch_formant_lpc(hipStream_t s, const float* x, const float* y, int64_t rows, int64_t W, const int64_t* n, int H, int64_t F, int p, const float* win,
                        const double* lagw, float* ax, float* cy, double* g, double* ex, double* ey) {
    fm_check("launch_formant_lpc", rows, W, H, F, p);
    const size_t lds = (size_t)(4 * FM_P1 + 2) * sizeof(double) + (size_t)4 * H * sizeof(float);  // 33.6 KB at H = 2048
    static PerDeviceOnce attr_once;
    if (attr_once.need())
        stn_check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&formant_lpc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 40 * 1024),
                      "hipFuncSetAttribute(formant_lpc)");
    STN_KLAUNCH(formant_lpc_kernel, dim3((unsigned)F, (unsigned)rows), dim3(128), (unsigned)lds, s, x, y, W, n, H, F, p, win, lagw, ax, cy, g, ex, ey);
}

void launch_formant_filter(hipStream_t s, const float* y, int64_t rows, int64_t W, const int64_t* n, int H, int64_t F, int p, const float* win,
                           const float* ax, const float* cy, float* out) {
    fm_check("launch_formant_filter", rows, W, H, F, p);
    const dim3 grid((unsigned)((2 * (F - 1) + 63) / 64), (unsigned)rows), block(64);
    if (p <= 16) STN_KLAUNCH(formant_filter_kernel<16>, grid, block, 0, s, y, W, n, H, F, p, win, ax, cy, out);
    else if (p <= 32) STN_KLAUNCH(formant_filter_kernel<32>, grid, block, 0, s, y, W, n, H, F, p, win, ax, cy, out);
    else STN_KLAUNCH(formant_filter_kernel<48>, grid, block, 0, s, y, W, n, H, F, p, win, ax, cy, out);
}

}  // namespace stn
