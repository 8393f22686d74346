// kernels_loudness.hip — BS.1770-4 integrated loudness of the finished waveform and the gain that normalizes it (gfx950, wave64).
// Runs at fetch time, outside the captured pipeline, on rows x W fp32 samples of which row b's first n_b count.
//
// The K-weighting cascade (shelf biquad, then high-pass biquad, each in transposed direct form II) is one 4-state linear system
// x' = A x + B u, state (s1, s2, t1, t2).  Decomposition:
//   1. chunk pass: a lane owns LO_CHUNK consecutive samples of a row, counted from sample 0; a workgroup stages its LO_WG chunks in LDS
//      with 16-byte loads (row stride 33 words: the lanes' walks fall on distinct banks; chunk_stage_in, kernels_chunk.hpp), and each
//      lane filters its chunk from zero state (biquad2_step, the same header), writing the end state e_k and the chunk's max |x|;
//   2. scan: one workgroup per row forms the true start states s_{k+1} = M s_k + e_k (M = A^LO_CHUNK, its powers from the host) by a
//      Hillis-Steele scan over tiles of LO_SCAN chunks, in place;
//   3. energy pass: each lane refilters its chunk from s_k and sums y^2 into the chunk's share of the 100 ms segment it starts in and
//      of the next one (chunks and segments need not align);
//   4. gate: one workgroup per row sums each segment's shares in a fixed order, forms the 400 ms block energies, applies the absolute
//      and relative gates and writes (L_b, peak_b, g_b);
//   5. gain: y = x * g_b per sample, in the fetch's sample encoding (launch_store_rows, kernels_output.hip).
// Every hand-off between workgroups is a launch boundary, and every sum runs in an order fixed by the sample positions within the
// row: a row's results depend on its first n_b samples and the rate only, not on W, the batch or the row's place in it.
#include "kernels_chunk.hpp"
#include "kernels_sort.hpp"
#include "host/loudness_range.hpp"

#include <math.h>

namespace stn {

namespace {

constexpr int LO_SPAN = LO_WG * LO_CHUNK;  // samples a workgroup of the chunk passes owns
constexpr int LO_PAD = LO_CHUNK + 1;       // LDS words per chunk
constexpr int LO_GATE = 1024;              // threads of the gate workgroup

template <bool kEnergy>
__global__ void __launch_bounds__(LO_WG) loudness_chunk_kernel(const float* __restrict__ x, int64_t W, int vec, const int64_t* __restrict__ nrow,
                                                               int64_t Ks, LoudCoef f, int hop, float* __restrict__ st, float* __restrict__ pk,
                                                               float* __restrict__ pa, float* __restrict__ pb) {
    __shared__ float win[LO_WG * LO_PAD];
    const int64_t row = blockIdx.y;
    const int64_t n = nrow[row];
    const int64_t s0 = (int64_t)blockIdx.x * LO_SPAN;
    if (s0 >= n) return;  // (the whole workgroup: nothing of the span lies in the row)
    const int cnt = (int)(n - s0 < LO_SPAN ? n - s0 : LO_SPAN);
    const float* __restrict__ xr = x + row * W + s0;
    chunk_stage_in<LO_WG, LO_CHUNK, true>(win, xr, cnt, vec);  // (a float4 that starts below n ends at or below W)
    __syncthreads();
    const int c0 = threadIdx.x * LO_CHUNK;
    if (c0 >= cnt) return;
    const int len = cnt - c0 < LO_CHUNK ? cnt - c0 : LO_CHUNK;
    const int64_t k = (int64_t)blockIdx.x * LO_WG + threadIdx.x;
    const float* w = win + threadIdx.x * LO_PAD;
    float4* sk = reinterpret_cast<float4*>(st) + row * Ks + k;
    if (!kEnergy) {
        float s1 = 0.f, s2 = 0.f, t1 = 0.f, t2 = 0.f, m = 0.f;
#pragma unroll
        for (int i = 0; i < LO_CHUNK; ++i) {
            if (i < len) {
                const float u = w[i];
                m = fmaxf(m, fabsf(u));
                (void)biquad2_step(f, u, s1, s2, t1, t2);
            }
        }
        *sk = make_float4(s1, s2, t1, t2);
        pk[row * Ks + k] = m;
    } else {
        const float4 s = *sk;
        float s1 = s.x, s2 = s.y, t1 = s.z, t2 = s.w, a = 0.f, b = 0.f;
        const int64_t g0 = s0 + c0;
        const int64_t bound = (g0 / hop + 1) * hop;  // first sample of the next segment
        const int64_t full = n / hop * hop;           // samples of whole segments
#pragma unroll
        for (int i = 0; i < LO_CHUNK; ++i) {
            if (i < len) {
                const float y = biquad2_step(f, w[i], s1, s2, t1, t2);
                const float yy = y * y;
                const int64_t g = g0 + i;
                a += (g < bound && g < full) ? yy : 0.0f;
                b += (g >= bound && g < full) ? yy : 0.0f;
            }
        }
        pa[row * Ks + k] = a;
        pb[row * Ks + k] = b;
    }
}

// r = v + P o (P row-major 4 x 4), each row summed in the same order
__device__ __forceinline__ double4 lo_affine(const double* __restrict__ P, double4 o, double4 v) {
    double4 r;
    r.x = v.x + (((P[0] * o.x + P[1] * o.y) + P[2] * o.z) + P[3] * o.w);
    r.y = v.y + (((P[4] * o.x + P[5] * o.y) + P[6] * o.z) + P[7] * o.w);
    r.z = v.z + (((P[8] * o.x + P[9] * o.y) + P[10] * o.z) + P[11] * o.w);
    r.w = v.w + (((P[12] * o.x + P[13] * o.y) + P[14] * o.z) + P[15] * o.w);
    return r;
}

// st[row][k]: end states from zero state in, start states out.  Tile t covers chunks t*LO_SCAN ..; after the inclusive scan, lane i
// holds v_i = sum_{j <= i} M^(i-j) e_j, so the start state of chunk t*LO_SCAN + i is v_{i-1} + M^i c with c the tile's carry-in.
// The scan runs in double on a double table, and only the start states it stores are fp32: the high-pass's two poles nearly coincide,
// so the powers of M hold entries near +-27 that almost cancel in P o, and in fp32 that rounding falls on the combination of t1 and t2
// the filter's output is most sensitive to (five times what the sample-by-sample fp32 recurrence loses at 48 kHz).
__global__ void __launch_bounds__(LO_SCAN) loudness_scan_kernel(const int64_t* __restrict__ nrow, int64_t Ks, const double* __restrict__ mp,
                                                                float* st) {
    __shared__ double4 buf[2][LO_SCAN];  // two images, written in turn: a level's readers are done before the level after next writes
    const int64_t row = blockIdx.x;
    const int64_t K = lo_chunks(nrow[row]);
    const int i = threadIdx.x;
    float4* sr = reinterpret_cast<float4*>(st) + row * Ks;
    double4 c = make_double4(0.0, 0.0, 0.0, 0.0);
    const double4 zero = c;
    int p = 0;
    for (int64_t t0 = 0; t0 < K; t0 += LO_SCAN) {
        const int64_t k = t0 + i;
        double4 v = zero;
        if (k < K) { const float4 e = sr[k]; v = make_double4(e.x, e.y, e.z, e.w); }
        for (int d = 1; d < LO_SCAN; d <<= 1) {
            buf[p][i] = v;
            __syncthreads();
            if (i >= d) v = lo_affine(mp + (d - 1) * 16, buf[p][i - d], v);
            p ^= 1;
        }
        buf[p][i] = v;
        __syncthreads();
        const double4 s = i == 0 ? c : lo_affine(mp + (i - 1) * 16, c, buf[p][i - 1]);
        if (k < K) sr[k] = make_float4((float)s.x, (float)s.y, (float)s.z, (float)s.w);
        c = lo_affine(mp + (LO_SCAN - 1) * 16, c, buf[p][LO_SCAN - 1]);
        p ^= 1;
    }
}

__device__ __forceinline__ double lo_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// fixed-order sum over the workgroup: lane-strided partials, a butterfly per wave (lane 0's order), the waves in order
__device__ double lo_block_sum(double v, double* red) {
    v = lo_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < LO_GATE / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

// 100 ms segment sums of a row (the gate's and the range kernel's): a wave per segment, its lanes strided over the chunks that touch it
// from the segment's first chunk on.  The caller synchronizes before it reads seg.
__device__ __forceinline__ void lo_segments(const float* __restrict__ par, const float* __restrict__ pbr, int64_t nseg, int hop, double* seg) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = threadIdx.x >> 6; j < nseg; j += LO_GATE / 64) {
        const int64_t k0 = j * hop / LO_CHUNK, k1 = ((j + 1) * hop - 1) / LO_CHUNK;
        double a = 0.0;
        for (int64_t k = k0 + lane; k <= k1; k += 64) a += (k * LO_CHUNK / hop == j) ? (double)par[k] : (double)pbr[k];
        a = lo_wave_sum(a);
        if (lane == 0) seg[j] = a;
    }
}

__global__ void __launch_bounds__(LO_GATE) loudness_gate_kernel(const int64_t* __restrict__ nrow, int64_t Ks, int hop, const float* __restrict__ pk,
                                                                const float* __restrict__ pa, const float* __restrict__ pb, int on, float target,
                                                                float ceiling, int64_t rows, float* __restrict__ res) {
    extern __shared__ double seg[];
    __shared__ double red[LO_GATE / 64];
    __shared__ float redm[LO_GATE / 64];
    const int64_t row = blockIdx.x;
    const int64_t n = nrow[row];
    const int64_t K = lo_chunks(n), nseg = n / hop;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* __restrict__ pkr = pk + row * Ks;
    const float* __restrict__ par = pa + row * Ks;
    const float* __restrict__ pbr = pb + row * Ks;
    // sample peak: max is order-independent, so exact
    float m = 0.f;
    for (int64_t k = tid; k < K; k += LO_GATE) m = fmaxf(m, pkr[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) redm[wave] = m;
    __syncthreads();
    float peak = 0.f;
    for (int w = 0; w < LO_GATE / 64; ++w) peak = fmaxf(peak, redm[w]);
    lo_segments(par, pbr, nseg, hop, seg);
    __syncthreads();
    // 400 ms blocks at a 100 ms hop, both gates
    const int64_t nblk = nseg >= 4 ? nseg - 3 : 0;
    const double inv = 1.0 / (4.0 * hop);
    double zs = 0.0, zc = 0.0;
    for (int64_t j = tid; j < nblk; j += LO_GATE) {
        const double z = ((seg[j] + seg[j + 1]) + (seg[j + 2] + seg[j + 3])) * inv;
        if (-0.691 + 10.0 * log10(z) > -70.0) { zs += z; zc += 1.0; }
    }
    zs = lo_block_sum(zs, red);
    zc = lo_block_sum(zc, red);
    double L = -INFINITY;
    if (zc > 0.0) {
        const double rel = -0.691 + 10.0 * log10(zs / zc) - 10.0;
        double rs = 0.0, rc = 0.0;
        for (int64_t j = tid; j < nblk; j += LO_GATE) {
            const double z = ((seg[j] + seg[j + 1]) + (seg[j + 2] + seg[j + 3])) * inv;
            const double l = -0.691 + 10.0 * log10(z);
            if (l > -70.0 && l > rel) { rs += z; rc += 1.0; }
        }
        rs = lo_block_sum(rs, red);
        rc = lo_block_sum(rc, red);
        if (rc > 0.0) L = -0.691 + 10.0 * log10(rs / rc);
    }
    if (tid == 0) {
        const float Lf = (float)L;
        float g = 1.0f;
        if (on && Lf > -INFINITY && peak > 0.f) {  // L_b undefined: gain 1
            const double gl = pow(10.0, ((double)target - (double)Lf) / 20.0);
            const double gc = pow(10.0, (double)ceiling / 20.0) / (double)peak;
            g = (float)(gl < gc ? gl : gc);
        }
        res[row] = Lf;
        res[rows + row] = peak;
        res[2 * rows + row] = g;
    }
}

// the workgroup's maximum of v (order-independent, so exact)
__device__ double lo_block_max(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double m = red[0];
    for (int w = 1; w < LO_GATE / 64; ++w) m = fmax(m, red[w]);
    __syncthreads();
    return m;
}

// The loudness report behind the same three passes: one workgroup per row.  LDS: seg[segcap] (the row's segment
// sums, formed as the gate forms them) and behind it key[P], the powers of the 3 s windows, P the power of two at or above the row's
// window count.  A window the gates drop, and the padding, hold +inf, so an ascending bitonic sort of key leaves the n_st kept powers
// in front; the power is monotone in the level, so the order statistics are read there.  Every compare-exchange of a sort stage owns
// its two elements and the stages are separated by barriers: nothing depends on thread timing.  res [3][rows]: m_max, s_max, lra.
__global__ void __launch_bounds__(LO_GATE) loudness_range_kernel(const int64_t* __restrict__ nrow, int64_t Ks, int hop, const float* __restrict__ pa,
                                                                 const float* __restrict__ pb, int segcap, int64_t rows, float* __restrict__ res,
                                                                 int32_t* __restrict__ nst) {
    extern __shared__ double seg[];
    __shared__ double red[LO_GATE / 64];
    double* key = seg + segcap;
    const int64_t row = blockIdx.x;
    int64_t nseg = nrow[row] / hop;
    if (nseg > segcap) nseg = segcap;  // (never taken: the launcher sized the LDS by the longest row)
    const int tid = threadIdx.x;
    lo_segments(pa + row * Ks, pb + row * Ks, nseg, hop, seg);
    __syncthreads();
    const int nblk = nseg >= LR_BLOCK ? (int)nseg - (LR_BLOCK - 1) : 0, nwin = nseg >= LR_WINDOW ? (int)nseg - (LR_WINDOW - 1) : 0;
    double zm = -1.0;
    for (int j = tid; j < nblk; j += LO_GATE) zm = fmax(zm, lr_block_power(seg + j, hop));
    zm = lo_block_max(zm, red);
    int P = 1;
    while (P < nwin) P <<= 1;
    // the window powers, their maximum and the absolute gate (thread tid owns key[tid], key[tid + LO_GATE], ... in this pass and the next)
    double zs = -1.0, as = 0.0, ac = 0.0;
    for (int j = tid; j < P; j += LO_GATE) {
        double z = INFINITY;
        if (j < nwin) {
            z = lr_window_power(seg + j, hop);
            zs = fmax(zs, z);
            if (lr_level(z) > LR_ABS_GATE) { as += z; ac += 1.0; }
        }
        key[j] = z;
    }
    zs = lo_block_max(zs, red);
    as = lo_block_sum(as, red);
    ac = lo_block_sum(ac, red);
    // the relative gate
    double kc = 0.0;
    const double rel = ac > 0.0 ? lr_level(as / ac) + LR_REL_GATE : INFINITY;
    for (int j = tid; j < nwin; j += LO_GATE) {
        const double l = lr_level(key[j]);
        if (l > LR_ABS_GATE && l > rel) kc += 1.0;
        else key[j] = INFINITY;
    }
    kc = lo_block_sum(kc, red);  // (its barriers also order the writes above before the sort's reads)
    lds_bitonic_sort<LO_GATE>(key, P);
    if (tid == 0) {
        const int64_t n = (int64_t)kc;
        res[row] = zm < 0.0 ? -INFINITY : (float)lr_level(zm);
        res[rows + row] = zs < 0.0 ? -INFINITY : (float)lr_level(zs);
        res[2 * rows + row] = n < 2 ? 0.0f : (float)(lr_level(key[lr_index(n, LR_HIGH)]) - lr_level(key[lr_index(n, LR_LOW)]));
        nst[row] = (int32_t)n;
    }
}

void lo_check(int64_t rows, int64_t W, const LoudTable& t) {
    if (rows > 65535) throw std::invalid_argument("loudness: more than 65535 rows");
    if (!t.dev || t.hop < 1) throw std::runtime_error("loudness: filter table not prepared");
    if (lo_chunks(W) > ((int64_t)1 << 31) / LO_WG) throw std::invalid_argument("loudness: row too long");
}

}  // namespace

void launch_loudness_chunks(hipStream_t s, bool energy, const float* x, int64_t rows, int64_t W, const int64_t* n, const LoudTable& t,
                            float* st, float* pk, float* pa, float* pb) {
    if (rows <= 0 || W <= 0) return;
    lo_check(rows, W, t);
    const int vec = chunk_vec(x, nullptr, W);
    const dim3 grid((unsigned)((W + LO_SPAN - 1) / LO_SPAN), (unsigned)rows);
    if (energy) STN_KLAUNCH(loudness_chunk_kernel<true>, grid, dim3(LO_WG), 0, s, x, W, vec, n, lo_chunks(W), t.coef, t.hop, st, pk, pa, pb);
    else STN_KLAUNCH(loudness_chunk_kernel<false>, grid, dim3(LO_WG), 0, s, x, W, vec, n, lo_chunks(W), t.coef, t.hop, st, pk, pa, pb);
}

void launch_loudness_scan(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, const LoudTable& t, float* st) {
    if (rows <= 0 || W <= 0) return;
    lo_check(rows, W, t);
    STN_KLAUNCH(loudness_scan_kernel, dim3((unsigned)rows), dim3(LO_SCAN), 0, s, n, lo_chunks(W), t.dev, st);
}

void launch_loudness_gate(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, const LoudTable& t, const float* pk, const float* pa,
                          const float* pb, int64_t max_seg, bool on, float target_lufs, float ceiling_dbfs, float* res) {
    if (rows <= 0 || W <= 0) return;
    lo_check(rows, W, t);
    if (max_seg > LO_MAX_SEG) throw std::invalid_argument("loudness: a row longer than " + std::to_string(LO_MAX_SEG) + " 100 ms segments");
    const unsigned lds = (unsigned)((max_seg > 0 ? max_seg : 1) * sizeof(double));
    static PerDeviceOnce attr_once;
    if (attr_once.need())
        stn_check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&loudness_gate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)(LO_MAX_SEG * sizeof(double))), "hipFuncSetAttribute(loudness_gate)");
    STN_KLAUNCH(loudness_gate_kernel, dim3((unsigned)rows), dim3(LO_GATE), lds, s, n, lo_chunks(W), t.hop, pk, pa, pb, on ? 1 : 0, target_lufs,
                ceiling_dbfs, rows, res);
}

std::string loudness_range_check(int64_t max_seg) {
    if (max_seg <= LR_MAX_SEG) return "";
    return "loudness range: a row of " + std::to_string(max_seg) + " 100 ms segments, and the report takes at most " + std::to_string(LR_MAX_SEG);
}

void launch_loudness_range(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, const LoudTable& t, const float* pa, const float* pb,
                           int64_t max_seg, float* res, int32_t* nst) {
    if (rows <= 0 || W <= 0) return;
    lo_check(rows, W, t);
    const std::string why = loudness_range_check(max_seg);
    if (!why.empty()) throw std::invalid_argument(why);
    const int segcap = (int)(max_seg > 0 ? max_seg : 1);
    int P = 1;
    while (P < segcap - (LR_WINDOW - 1)) P <<= 1;
    static PerDeviceOnce attr_once;
    if (attr_once.need())
        stn_check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&loudness_range_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)(2 * LR_MAX_SEG * sizeof(double))), "hipFuncSetAttribute(loudness_range)");
    STN_KLAUNCH(loudness_range_kernel, dim3((unsigned)rows), dim3(LO_GATE), (unsigned)((segcap + P) * sizeof(double)), s, n, lo_chunks(W), t.hop, pa, pb,
                segcap, rows, res, nst);
}

}  // namespace stn
