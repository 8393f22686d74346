// kernels_edges.hip — where the speech of a finished row starts and ends, by level (gfx950, wave64).  Runs at fetch
// time, outside the captured pipeline, on rows x W fp32 samples of which row b's first n_b count.
//
// Frames of F samples (10 ms) from sample 0, the last one short; frame k's level m_k is the mean of x^2 over its own samples.
//   1. frame pass: a lane owns ED_CHUNK consecutive samples of a row, counted from sample 0 (the energy pass of kernels_loudness.hip: a
//      workgroup stages its ED_WG chunks in LDS with 16-byte loads, row stride 33 words: chunk_stage_in, kernels_chunk.hpp), and sums x^2 in sample order into the chunk's
//      share of the frame it starts in and of the next one (F > ED_CHUNK: a chunk meets two frames at most);
//   2. row pass: one workgroup per row sums each frame's shares in chunk order (a thread per frame, in double), writes the levels,
//      takes their maximum, finds the first and the last frame at or above the threshold, and writes the row's edges and the one-member
//      programme of the per-row trimmed fetch (JoinSegT / JoinProg: the store is join_trim_rows_kernel, kernels_output.hip).
// The hand-off is a launch boundary and every sum runs in an order fixed by the sample positions within the row: a row's edges depend
// on its first n_b samples, the rate and the parameters only, not on W, the batch or the row's place in it.  Max, min and the
// comparisons are order-independent.
// With the pause limit a third launch follows the row pass:
//   3. pause pass: one workgroup per row reads the levels and the edges and writes the row's several segments, the row without the
//      middle of every pause inside it that is longer than the limit (pause_rows_kernel, below the row pass).
#include "kernels_chunk.hpp"

#include <math.h>

namespace stn {

namespace {

constexpr int ED_SPAN = ED_WG * ED_CHUNK;  // samples a workgroup of the frame pass owns
constexpr int ED_PAD = ED_CHUNK + 1;       // LDS words per chunk
constexpr int ED_ROW = 1024;               // threads of the row workgroup

__global__ void __launch_bounds__(ED_WG) edges_chunk_kernel(const float* __restrict__ x, int64_t W, int vec, const int64_t* __restrict__ nrow,
                                                            int64_t Ks, int F, float* __restrict__ pa, float* __restrict__ pb) {
    __shared__ float win[ED_WG * ED_PAD];
    const int64_t row = blockIdx.y;
    const int64_t n = nrow[row];
    const int64_t s0 = (int64_t)blockIdx.x * ED_SPAN;
    if (s0 >= n) return;  // (the whole workgroup: nothing of the span lies in the row)
    const int cnt = (int)(n - s0 < ED_SPAN ? n - s0 : ED_SPAN);
    const float* __restrict__ xr = x + row * W + s0;
    chunk_stage_in<ED_WG, ED_CHUNK, true>(win, xr, cnt, vec);  // (a float4 that starts below n ends at or below W)
    __syncthreads();
    const int c0 = threadIdx.x * ED_CHUNK;
    if (c0 >= cnt) return;
    const int len = cnt - c0 < ED_CHUNK ? cnt - c0 : ED_CHUNK;
    const int64_t k = (int64_t)blockIdx.x * ED_WG + threadIdx.x;
    const float* w = win + threadIdx.x * ED_PAD;
    const int64_t g0 = s0 + c0;
    const int split = (int)((g0 / F + 1) * F - g0);  // samples of this chunk before the next frame begins (>= 1)
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < ED_CHUNK; ++i) {
        if (i < len) {
            const float xx = w[i] * w[i];
            a += i < split ? xx : 0.0f;
            b += i >= split ? xx : 0.0f;
        }
    }
    pa[row * Ks + k] = a;
    pb[row * Ks + k] = b;
}

// fixed places for the wave results of a workgroup-wide max / min
template <typename T, typename Op>
__device__ T ed_block_reduce(T v, T* red, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = red[0];
    for (int w = 1; w < ED_ROW / 64; ++w) s = op(s, red[w]);
    __syncthreads();
    return s;
}

__global__ void __launch_bounds__(ED_ROW) edges_row_kernel(const int64_t* __restrict__ nrow, int64_t Ks, int64_t Kf, int F, double ratio, double floor_ms,
                                                           int64_t keep, int64_t fd, const float* __restrict__ pa, const float* __restrict__ pb,
                                                           double* lev, int64_t* __restrict__ edges, JoinSegT* __restrict__ seg,
                                                           JoinProg* __restrict__ prog) {
    __shared__ double redd[ED_ROW / 64];
    __shared__ long long redi[ED_ROW / 64];
    const int64_t row = blockIdx.x;
    const int64_t n = nrow[row];
    const int64_t K = (n + F - 1) / F;
    const int tid = threadIdx.x;
    const float* __restrict__ par = pa + row * Ks;
    const float* __restrict__ pbr = pb + row * Ks;
    double* levr = lev + row * Kf;
    // frame levels: the shares of the chunks that touch the frame, in chunk order; a chunk that starts in the frame gives its first
    // share, the one that started in the frame before its second
    double mx = 0.0;
    for (int64_t k = tid; k < K; k += ED_ROW) {
        const int64_t lo = k * F, hi = lo + F < n ? lo + F : n;
        const int64_t c0 = lo / ED_CHUNK, c1 = (hi - 1) / ED_CHUNK;
        double s = 0.0;
        for (int64_t c = c0; c <= c1; ++c) s += (c * ED_CHUNK / F == k) ? (double)par[c] : (double)pbr[c];
        const double m = s / (double)(hi - lo);
        levr[k] = m;  // (read back below by this thread only)
        mx = fmax(mx, m);
    }
    mx = ed_block_reduce(mx, redd, [](double p, double q) { return fmax(p, q); });
    const bool speech = n > 0 && mx > floor_ms;
    const double thr = mx * ratio;
    long long f0 = K, f1 = -1;
    if (speech) {
        for (int64_t k = tid; k < K; k += ED_ROW) {
            if (levr[k] >= thr) {
                if (k < f0) f0 = k;
                if (k > f1) f1 = k;
            }
        }
    }
    f0 = ed_block_reduce(f0, redi, [](long long p, long long q) { return p < q ? p : q; });
    f1 = ed_block_reduce(f1, redi, [](long long p, long long q) { return p > q ? p : q; });
    if (tid == 0) {
        int64_t start = 0, end = n;
        if (speech && f1 >= f0) {
            start = f0 * F - keep;
            if (start < 0) start = 0;
            end = (f1 + 1) * F + keep;
            if (end > n) end = n;
        }
        edges[2 * row] = start;
        edges[2 * row + 1] = end;
        if (seg) {
            const int64_t len = end - start, fl = fd < len ? fd : len;
            JoinSegT sg;
            sg.dst = 0; sg.len = len; sg.row = row; sg.src = start;
            sg.fin = start > 0 ? (int32_t)fl : 0;
            sg.fout = end < n ? (int32_t)fl : 0;
            seg[row] = sg;
            JoinProg pg;
            pg.len = len; pg.first = (int32_t)row; pg.count = 1;
            prog[row] = pg;
        }
    }
}


// The pause limit: a row's frame levels -> its segment table with every pause inside [f0, f1] longer than Mp
// shortened to Mp.  One workgroup per row.  The threshold and f0, f1 are recomputed from lev as edges_row_kernel computed them (max, min
// and comparisons: no order to depend on).  The frames are then walked in tiles of ED_ROW, a thread per frame: an active frame b whose
// previous active frame is pa closes the pause a = pa + 1 .. b - 1, and cuts it when (b - a) F > Mp.  "The previous active frame" is an
// exclusive max-scan of (active ? k : -1), the cut's index and the samples dropped up to it are inclusive sum-scans of the cut flag and
// of P - Mp; each is a shuffle scan inside the wave, the waves' totals combined through LDS in wave order, and a carry from tile to
// tile.  Cut j < cap is staged in LDS as {lo, hi, dropped through j}; behind the walk thread j writes segment j from cuts j - 1 and j,
// so that no table entry has two writers.  No atomics: a row's table depends on its own levels and the parameters only.
struct PauseCarry { long long last; int cuts; long long drop; };

template <typename T>
__device__ __forceinline__ T pz_shfl_up(T v, int o) { return __shfl_up(v, o, 64); }

__global__ void __launch_bounds__(ED_ROW) pause_rows_kernel(const int64_t* __restrict__ nrow, int64_t Kf, int F, double ratio, double floor_ms, int64_t fd,
                                                            int64_t Mp, int S, const double* __restrict__ lev, const int64_t* __restrict__ edges,
                                                            JoinSegT* __restrict__ seg, JoinProg* __restrict__ prog, int64_t* __restrict__ cuts) {
    constexpr int NW = ED_ROW / 64;
    __shared__ double redd[NW];
    __shared__ long long w_last[NW], w_drop[NW];
    __shared__ int w_cuts[NW];
    __shared__ long long c_lo[PZ_MAX_CUTS], c_hi[PZ_MAX_CUTS], c_drop[PZ_MAX_CUTS];
    const int64_t row = blockIdx.x;
    const int64_t n = nrow[row];
    const int64_t K = (n + F - 1) / F;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = S - 1 < PZ_MAX_CUTS ? S - 1 : PZ_MAX_CUTS;
    const double* __restrict__ levr = lev + row * Kf;
    double mx = 0.0;
    for (int64_t k = tid; k < K; k += ED_ROW) mx = fmax(mx, levr[k]);
    mx = ed_block_reduce(mx, redd, [](double p, double q) { return fmax(p, q); });
    const bool speech = n > 0 && mx > floor_ms;
    const double thr = mx * ratio;
    const int64_t hr = Mp / 2, hl = Mp - hr;
    PauseCarry carry{-1, 0, 0};  // (every thread keeps the same copy)
    const int64_t tiles = speech ? (K + ED_ROW - 1) / ED_ROW : 0;
    for (int64_t t = 0; t < tiles; ++t) {
        const int64_t k = t * ED_ROW + tid;
        const bool active = k < K && levr[k] >= thr;
        // the last active frame at or before k within the wave, then before k
        long long inc = active ? (long long)k : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long u = pz_shfl_up(inc, o);
            if (lane >= o && u > inc) inc = u;
        }
        long long prev = pz_shfl_up(inc, 1);
        if (lane == 0) prev = -1;
        if (lane == 63) w_last[wave] = inc;
        __syncthreads();
        long long before = carry.last, tile_last = carry.last;
        for (int w = 0; w < NW; ++w) {
            if (w < wave && w_last[w] > before) before = w_last[w];
            if (w_last[w] > tile_last) tile_last = w_last[w];
        }
        if (before > prev) prev = before;
        // frame k closes a pause when it is active, an active frame lies before it, and frames lie between them
        const long long a = prev + 1;
        const long long P = (active && prev >= 0) ? ((long long)k - a) * F : 0;
        const bool cut = P > Mp;
        int ci = cut ? 1 : 0;
        long long di = cut ? P - Mp : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int uc = pz_shfl_up(ci, o);
            const long long ud = pz_shfl_up(di, o);
            if (lane >= o) { ci += uc; di += ud; }
        }
        if (lane == 63) { w_cuts[wave] = ci; w_drop[wave] = di; }
        __syncthreads();
        int cb = carry.cuts, ct = carry.cuts;
        long long db = carry.drop, dt = carry.drop;
        for (int w = 0; w < NW; ++w) {
            if (w < wave) { cb += w_cuts[w]; db += w_drop[w]; }
            ct += w_cuts[w]; dt += w_drop[w];
        }
        // cuts behind the cap stay whole: a dropped count that includes one is never used (the walk ends at the cap below)
        if (cut) {
            const int j = cb + ci - 1;
            if (j < cap) { c_lo[j] = a * F + hl; c_hi[j] = (long long)k * F - hr; c_drop[j] = db + di; }
        }
        carry.last = tile_last; carry.cuts = ct; carry.drop = dt;
        __syncthreads();  // (w_* are rewritten by the next tile)
        if (carry.cuts >= cap) break;  // (uniform: every thread holds the same carry)
    }
    __syncthreads();
    const int m = carry.cuts < cap ? carry.cuts : cap;
    const int64_t start = edges[2 * row], end = edges[2 * row + 1];
    if (tid <= m) {
        const int64_t src = tid == 0 ? start : (int64_t)c_hi[tid - 1];
        const int64_t stop = tid == m ? end : (int64_t)c_lo[tid];
        const int64_t gone = tid == 0 ? 0 : (int64_t)c_drop[tid - 1];
        const int64_t len = stop - src, fl = fd < len ? fd : len;
        JoinSegT sg;
        sg.dst = src - start - gone; sg.len = len; sg.row = row; sg.src = src;
        sg.fin = (tid > 0 || start > 0) ? (int32_t)fl : 0;
        sg.fout = (tid < m || end < n) ? (int32_t)fl : 0;
        seg[row * S + tid] = sg;
    }
    int64_t* cr = cuts + row * (2 * (int64_t)S);
    if (tid < m) { cr[2 + 2 * tid] = c_lo[tid]; cr[3 + 2 * tid] = c_hi[tid]; }
    if (tid == 0) {
        const int64_t len = end - start - (m > 0 ? (int64_t)c_drop[m - 1] : 0);
        JoinProg pg;
        pg.len = len; pg.first = (int32_t)(row * S); pg.count = m + 1;
        prog[row] = pg;
        cr[0] = m; cr[1] = len;
    }
}

}  // namespace

static int edges_check(int64_t rows, int64_t W, int hz) {
    if (rows > 65535) throw std::invalid_argument("silence edges: more than 65535 rows");
    const int F = edges_frame(hz);
    if (F <= ED_CHUNK) throw std::invalid_argument("silence edges: the rate is too low for a 10 ms frame of more than " + std::to_string(ED_CHUNK) + " samples");
    if (ed_chunks(W) > ((int64_t)1 << 31) / ED_WG) throw std::invalid_argument("silence edges: row too long");
    return F;
}

void launch_edges_frames(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, int hz, float* pa, float* pb) {
    if (rows <= 0 || W <= 0) return;
    const int F = edges_check(rows, W, hz);
    const int vec = chunk_vec(x, nullptr, W);
    STN_KLAUNCH(edges_chunk_kernel, dim3((unsigned)((W + ED_SPAN - 1) / ED_SPAN), (unsigned)rows), dim3(ED_WG), 0, s, x, W, vec, n, ed_chunks(W), F, pa, pb);
}

void launch_edges_rows(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, int hz, double top_db, int64_t keep, int64_t fd, const float* pa,
                       const float* pb, double* lev, int64_t* edges, JoinSegT* seg, JoinProg* prog) {
    if (rows <= 0 || W <= 0) return;
    const int F = edges_check(rows, W, hz);
    if (fd < 0 || fd > 0x7fffffff || keep < 0) throw std::invalid_argument("silence edges: bad keep or fade length");
    STN_KLAUNCH(edges_row_kernel, dim3((unsigned)rows), dim3(ED_ROW), 0, s, n, ed_chunks(W), edges_frames(W, hz), F, std::pow(10.0, -top_db / 10.0), 1e-7,
                keep, fd, pa, pb, lev, edges, seg, prog);
}

void launch_pause_rows(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, int hz, double top_db, int64_t fd, int64_t Mp, int S, const double* lev,
                       const int64_t* edges, JoinSegT* seg, JoinProg* prog, int64_t* cuts) {
    if (rows <= 0 || W <= 0) return;
    const int F = edges_check(rows, W, hz);
    if (fd < 0 || fd > 0x7fffffff || Mp < 1) throw std::invalid_argument("pause limit: bad fade or pause length");
    if (S < 1 || S > PZ_MAX_CUTS + 1) throw std::invalid_argument("pause limit: table stride outside [1, 256]");
    STN_KLAUNCH(pause_rows_kernel, dim3((unsigned)rows), dim3(ED_ROW), 0, s, n, edges_frames(W, hz), F, std::pow(10.0, -top_db / 10.0), 1e-7, fd, Mp, S, lev,
                edges, seg, prog, cuts);
}

}  // namespace stn
