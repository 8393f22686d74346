// kernels_filter.hip — the write pass of the fetch-time biquad chain (gfx950, wave64).
//
// A section pass filters rows x W fp32 through two biquads (transposed direct form II, fp32) as the 4-state linear system the loudness
// measurement runs (kernels_loudness.hip), and its first two launches ARE that measurement's: the chunk pass from zero state
// (launch_loudness_chunks, energy = false) and the scan in double (launch_loudness_scan), on a LoudTable that holds the section's
// coefficients and the powers of its own M = A^LO_CHUNK, with every row's length W.  What the measurement lacks is the launch below:
// each lane refilters its chunk from the true start state, with the biquad2_step the chunk pass ran (kernels_chunk.hpp, which also holds
// the staging), and the workgroup writes y.
//
// In place (y == x) is allowed: a workgroup reads the LO_SPAN samples it owns into LDS before the first barrier, the lanes replace
// their chunks there, and the stores come after the second barrier; no workgroup touches another's span.
// A row's y[0 .. n) depends on x[0 .. n) of that row and the coefficients only: chunks are counted from sample 0, and the scan's order
// is fixed by the chunk index.
#include "kernels_chunk.hpp"

namespace stn {

namespace {

constexpr int FL_SPAN = LO_WG * LO_CHUNK;  // samples a workgroup owns
constexpr int FL_PAD = LO_CHUNK + 1;       // LDS words per chunk (chunk_stage_in)

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
    chunk_stage_in<LO_WG, LO_CHUNK, false>(win, xr, cnt, vec);  // (W % 4 == 0 in the 16-byte form: so is cnt)
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
            if (i < len) w[i] = biquad2_step(f, w[i], s1, s2, t1, t2);
    }
    __syncthreads();
    chunk_stage_out<LO_WG, LO_CHUNK>(win, yr, cnt, vec);
}

}  // namespace

void launch_filter_write(hipStream_t s, const float* x, int64_t rows, int64_t W, const LoudTable& t, const float* st, float* y) {
    if (rows <= 0 || W <= 0) return;
    chunk_shape("filter", rows, W);
    const int vec = chunk_vec(x, y, W);
    const dim3 grid((unsigned)((W + FL_SPAN - 1) / FL_SPAN), (unsigned)rows);
    STN_KLAUNCH(filter_write_kernel, grid, dim3(LO_WG), 0, s, x, y, W, vec, lo_chunks(W), t.coef, st);
}

}  // namespace stn
