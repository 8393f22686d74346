// kernels_resample.hip — rational polyphase resampler of the finished waveform (gfx950, wave64).  Runs at fetch time, outside the
// captured pipeline: rows x W fp32 samples at the model rate -> rows x W_out samples at P/Q times that rate, in any fetch encoding
// (fp32, 16- or 24-bit PCM, mu-law, A-law: enc_store1, kernels_dev.hpp), rows landing dst_stride samples apart.
//
// Output n of a row: phase (n*Q) mod P, first input floor(n*Q/P) - off, taps taps[phase][0 .. T) (resample_design, engine_resample.cpp).
// Decomposition: write n = k*P + r.  For a fixed r every k has the same phase (r*Q mod P) and its first input
// steps by Q, so a wavefront takes one r and 64 consecutive k: its taps are wave-uniform (scalar loads, SGPR operands of the FMAs —
// the table never enters LDS or VGPRs), and the lanes read the input at a stride of Q.  A workgroup (16 waves) owns G*64 consecutive
// k of one row and every r: its input span (G*64*Q + T samples) is staged once in LDS, zero outside [0, W), and the waves walk the
// (k group, r) pairs.  Spans above 160 KiB (Q > ~620) read the row through the caches instead, with the same arithmetic.  G and the path
// are ONE host decision, resample_form.
// Every output sums its T products in the same order (eight interleaved fp32 FMA chains, then a fixed tree) whatever its position in
// the row, the tile or the launch, and a read outside the row is 0.0f: a row whose samples past m are zero gives, in its first
// ceil(m*P/Q) outputs, exactly what the row cut at m gives.
#include "kernels.hpp"
#include "kernels_dev.hpp"

namespace stn {

namespace {

constexpr int RS_THREADS = 1024;
constexpr int RS_LANES = 64;
constexpr int64_t RS_LDS_MAX = 160 * 1024;

// input samples a workgroup of G*64 k values reads (every r): first input of its last output + T
__host__ __device__ inline int64_t rs_span(int G, int P, int Q, int T) {
    return (int64_t)(G * RS_LANES - 1) * Q + (int64_t)(P - 1) * Q / P + T;
}

template <bool kLds, int kEnc>
__global__ void __launch_bounds__(RS_THREADS) resample_kernel(const float* __restrict__ x, int64_t W, int64_t W_out, int P, int Q, int T,
                                                              int off, int G, const float* __restrict__ taps, unsigned char* __restrict__ y,
                                                              int64_t dst_stride) {
    extern __shared__ float win[];
    const int64_t row = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.x * G * RS_LANES;
    const int64_t s0 = k0 * Q - off;  // first input of the workgroup's span
    const float* __restrict__ xr = x + row * W;
    if (kLds) {
        // eight loads in flight per thread: every address is clamped into the row (W >= 1) and the value replaced by 0 outside it,
        // so no load waits behind a branch
        const int64_t span = rs_span(G, P, Q, T);
        for (int64_t i0 = threadIdx.x; i0 < span; i0 += 8 * RS_THREADS) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t t = s0 + i0 + (int64_t)u * RS_THREADS;
                const float e = xr[t < 0 ? 0 : (t >= W ? W - 1 : t)];
                v[u] = (t >= 0 && t < W) ? e : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i0 + (int64_t)u * RS_THREADS < span) win[i0 + (int64_t)u * RS_THREADS] = v[u];
        }
        __syncthreads();
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / RS_LANES));
    const int lane = (int)(threadIdx.x % RS_LANES);
    for (int pr = wave; pr < G * P; pr += RS_THREADS / RS_LANES) {
        const int g = pr / P, r = pr - g * P;
        const int phase = (int)(((int64_t)r * Q) % P);
        const int64_t k = k0 + (int64_t)g * RS_LANES + lane;
        const int64_t n = k * P + r;
        const int64_t first = k * Q + (int64_t)r * Q / P - off;  // input under tap 0
        const float* __restrict__ tp = taps + (int64_t)phase * T;
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (kLds) {
            const float* xs = win + (first - s0);
            for (int j = 0; j < T; j += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) a[u] = __builtin_fmaf(xs[j + u], tp[j + u], a[u]);
            }
        } else {
            for (int j = 0; j < T; j += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int64_t t = first + j + u;
                    a[u] = __builtin_fmaf((t >= 0 && t < W) ? xr[t] : 0.0f, tp[j + u], a[u]);
                }
            }
        }
        const float s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
        if (n < W_out) enc_store1<kEnc>(y, row * dst_stride + n, s);  // byte encodings: plain stores at a stride of P
    }
}

template <int kEnc>
void launch_resample_t(hipStream_t s, const float* x, int64_t rows, int64_t W, const ResampleTable& f, unsigned char* y, int64_t dst_stride, int64_t cap) {
    if (rows <= 0 || W <= 0) return;
    if (f.T % 8 != 0 || f.T < 8 || f.P < 1 || f.Q < 1 || !f.dev) throw std::runtime_error("launch_resample: filter table not prepared");
    if (rows > 65535) throw std::invalid_argument("launch_resample: more than 65535 rows");
    if (cap < 0) throw std::invalid_argument("launch_resample: negative cap");
    // (the kernel's W_out is its store guard only: a capped launch stores the first `cap` outputs of a row and computes them as ever)
    const int64_t W_out = cap > 0 ? std::min(cap, resample_out_len(W, f.P, f.Q)) : resample_out_len(W, f.P, f.Q);
    if (dst_stride < W_out) throw std::invalid_argument("launch_resample: dst_stride smaller than the output row length");
    const ResampleForm fm = resample_form(W, f);  // the one place G and the staging path are chosen
    const dim3 grid((unsigned)fm.grid_x, (unsigned)rows);
    if (fm.lds) {
        static PerDeviceOnce attr_once;
        if (attr_once.need())
            stn_check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&resample_kernel<true, kEnc>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)RS_LDS_MAX), "hipFuncSetAttribute(resample)");
        STN_KLAUNCH((resample_kernel<true, kEnc>), grid, dim3(RS_THREADS), (unsigned)fm.lds_bytes, s, x, W, W_out, f.P, f.Q, f.T, f.off, fm.G, f.dev, y, dst_stride);
    } else {
        STN_KLAUNCH((resample_kernel<false, kEnc>), grid, dim3(RS_THREADS), 0, s, x, W, W_out, f.P, f.Q, f.T, f.off, fm.G, f.dev, y, dst_stride);
    }
}

}  // namespace

std::string ResampleForm::str() const { return std::string(lds ? "resample lds G" : "resample cache G") + std::to_string(G); }

ResampleForm resample_form(int64_t W, const ResampleTable& f) {
    if (W < 1 || f.T % 8 != 0 || f.T < 8 || f.P < 1 || f.Q < 1) throw std::invalid_argument("resample_form: no row or no filter");
    const int64_t K = (resample_out_len(W, f.P, f.Q) + f.P - 1) / f.P;  // k values of a row
    ResampleForm fm;
    // G k groups per workgroup: enough (k group, r) pairs for the 16 waves where the span still fits in LDS
    int G = 1;
    while (G * f.P < RS_THREADS / RS_LANES && (int64_t)G * RS_LANES < K && rs_span(2 * G, f.P, f.Q, f.T) * 4 <= RS_LDS_MAX) G *= 2;
    const int64_t span_bytes = rs_span(G, f.P, f.Q, f.T) * 4;
    fm.G = G;
    fm.lds = span_bytes <= RS_LDS_MAX;
    fm.lds_bytes = fm.lds ? span_bytes : 0;
    fm.grid_x = (K + (int64_t)G * RS_LANES - 1) / ((int64_t)G * RS_LANES);
    return fm;
}

void launch_resample(hipStream_t s, const float* x, int64_t rows, int64_t W, const ResampleTable& f, int enc, void* y, int64_t dst_stride, int64_t cap) {
    with_enc(enc, "launch_resample", [&](auto e) { launch_resample_t<decltype(e)::value>(s, x, rows, W, f, static_cast<unsigned char*>(y), dst_stride, cap); });
}

}  // namespace stn
