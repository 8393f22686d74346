// kernels_filter.hip — the write pass of the fetch-time biquad chain (gfx950, wave64).
//
// A section pass filters rows x W fp32 through two biquads (transposed direct form II, fp32) as the 4-state linear system the loudness
// measurement runs (kernels_loudness.hip), and its first two launches ARE that measurement's: the chunk pass from zero state
// (launch_loudness_chunks, energy = false) and the scan in double (launch_loudness_scan), on a LoudTable that holds the section's
// coefficients and the powers of its own M = A^LO_CHUNK, with every row's length W.  What the measurement lacks is the launch below:
// each lane refilters its chunk from the true start state and the workgroup writes y.
//
// In place (y == x) is allowed: a workgroup reads the LO_SPAN samples it owns into LDS before the first barrier, the lanes replace
// their chunks there, and the stores come after the second barrier; no workgroup touches another's span.
// A row's y[0 .. n) depends on x[0 .. n) of that row and the coefficients only: chunks are counted from sample 0, and the scan's order
// is fixed by the chunk index.
#include "kernels.hpp"

namespace stn {

namespace {

constexpr int FL_SPAN = LO_WG * LO_CHUNK;  // samples a workgroup owns
constexpr int FL_PAD = LO_CHUNK + 1;       // LDS words per chunk: the lanes' walks fall on distinct banks

// one sample through the two sections (b0 b1 b2 a1 a2 = c[0..4], then c[5..9]): operation for operation lo_step of kernels_loudness.hip,
// which the chunk pass from zero state runs; the start states the scan forms are exact for this arithmetic only
__device__ __forceinline__ float fl_step(const LoudCoef& f, float u, float& s1, float& s2, float& t1, float& t2) {
    const float v = __builtin_fmaf(f.c[0], u, s1);
    s1 = __builtin_fmaf(-f.c[3], v, __builtin_fmaf(f.c[1], u, s2));
    s2 = __builtin_fmaf(-f.c[4], v, f.c[2] * u);
    const float y = __builtin_fmaf(f.c[5], v, t1);
    t1 = __builtin_fmaf(-f.c[8], y, __builtin_fmaf(f.c[6], v, t2));
    t2 = __builtin_fmaf(-f.c[9], y, f.c[7] * v);
    return y;
}

// grid (ceil(W / FL_SPAN), rows): every workgroup's span starts inside the row.  x and y may be the same rows (see above), so neither
// is __restrict__.
__global__ void __launch_bounds__(LO_WG) filter_write_kernel(const float* x, float* y, int64_t W, int vec, int64_t Ks, LoudCoef f,
                                                             const float* __restrict__ st) {
    __shared__ float win[LO_WG * FL_PAD];
    const int64_t row = blockIdx.y;
    const int64_t s0 = (int64_t)blockIdx.x * FL_SPAN;
    const int cnt = (int)(W - s0 < FL_SPAN ? W - s0 : FL_SPAN);
    const float* xr = x + row * W + s0;
    float* yr = y + row * W + s0;
    constexpr int U = FL_SPAN / 4 / LO_WG;
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
                float* d = win + (i / LO_CHUNK) * FL_PAD + (i % LO_CHUNK);  // (the four samples share a chunk)
                d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
            }
        }
    } else {
        for (int i0 = 0; i0 < FL_SPAN; i0 += 8 * LO_WG) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + threadIdx.x + u * LO_WG;
                v[u] = i < cnt ? xr[i] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + threadIdx.x + u * LO_WG;
                if (i < cnt) win[(i / LO_CHUNK) * FL_PAD + (i % LO_CHUNK)] = v[u];
            }
        }
    }
    __syncthreads();
    const int c0 = threadIdx.x * LO_CHUNK;
    if (c0 < cnt) {
        const int len = cnt - c0 < LO_CHUNK ? cnt - c0 : LO_CHUNK;
        const int64_t k = (int64_t)blockIdx.x * LO_WG + threadIdx.x;
        float* w = win + threadIdx.x * FL_PAD;
        const float4 s = reinterpret_cast<const float4*>(st)[row * Ks + k];
        float s1 = s.x, s2 = s.y, t1 = s.z, t2 = s.w;
#pragma unroll
        for (int i = 0; i < LO_CHUNK; ++i)
            if (i < len) w[i] = fl_step(f, w[i], s1, s2, t1, t2);
    }
    __syncthreads();
    if (vec) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = threadIdx.x + u * LO_WG, i = 4 * q;
            if (i < cnt) {
                const float* d = win + (i / LO_CHUNK) * FL_PAD + (i % LO_CHUNK);
                reinterpret_cast<float4*>(yr)[q] = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += LO_WG) yr[i] = win[(i / LO_CHUNK) * FL_PAD + (i % LO_CHUNK)];
    }
}

bool fl_aligned16(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace

const char* filter_staging_form(const float* x, const float* y, int64_t W) {
    return W % 4 == 0 && fl_aligned16(x) && fl_aligned16(y) ? "vec" : "scalar";
}

void launch_filter_write(hipStream_t s, const float* x, int64_t rows, int64_t W, const LoudTable& t, const float* st, float* y) {
    if (rows <= 0 || W <= 0) return;
    if (rows > 65535) throw std::invalid_argument("filter: more than 65535 rows");
    if (lo_chunks(W) > ((int64_t)1 << 31) / LO_WG) throw std::invalid_argument("filter: row too long");
    const int vec = filter_staging_form(x, y, W)[0] == 'v' ? 1 : 0;
    const dim3 grid((unsigned)((W + FL_SPAN - 1) / FL_SPAN), (unsigned)rows);
    STN_KLAUNCH(filter_write_kernel, grid, dim3(LO_WG), 0, s, x, y, W, vec, lo_chunks(W), t.coef, st);
}

}  // namespace stn
