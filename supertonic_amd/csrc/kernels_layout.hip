// kernels_layout.hip — the HBM-bound layout and element-wise kernels between the GEMMs (gfx950, wave64): gather / mask / transpose / pack helpers,
// the vocoder front (latent un-compress + input conv, or its im2col for the MFMA path), pooling, casts, step counters and the Philox noise.
// All row-major [rows][channels]; see kernels.hpp for the contracts.
#include "kernels.hpp"
#include "kernels_dev.hpp"

#include <type_traits>

namespace stn {

__global__ void embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ emb, int vocab, int L, int C,
                             const int* __restrict__ len, float* __restrict__ x, const int* __restrict__ row_off) {
    const int row = blockIdx.x, b = row / L, t = row - b * L;
    if (row_off && t >= len[b]) return;  // packed destination: the position does not exist
    const int64_t id = ids[row];
    const bool ok = t < len[b] && id >= 0 && id < vocab;
    const int C4 = C >> 2;
    float4* o = reinterpret_cast<float4*>(x) + (row_off ? (int64_t)row_off[b] + t : (int64_t)row) * C4;
    const float4* e = reinterpret_cast<const float4*>(emb) + (ok ? id : 0) * C4;
    for (int c = threadIdx.x; c < C4; c += blockDim.x) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) v = e[c];
        o[c] = v;
    }
}
void launch_embed(hipStream_t s, const int64_t* ids, const float* emb, int vocab, int B, int L, int C, const int* len,
                  float* x, const int* row_off) {
    if (B * L == 0) return;
    STN_KLAUNCH(embed_kernel, dim3(B * L), dim3(64), 0, s, ids, emb, vocab, L, C, len, x, row_off);
}

__global__ void mask_to_len_kernel(const float* __restrict__ mask, int L, int* __restrict__ len) {
    const int b = blockIdx.x;
    float c = 0.f;
    for (int t = threadIdx.x; t < L; t += 64) c += mask[(int64_t)b * L + t] > 0.5f ? 1.f : 0.f;
    c = wave_sum(c);
    if (threadIdx.x == 0) len[b] = (int)(c + 0.5f);
}
void launch_mask_to_len(hipStream_t s, const float* mask, int B, int L, int* len) {
    if (B == 0) return;
    STN_KLAUNCH(mask_to_len_kernel, dim3(B), dim3(64), 0, s, mask, L, len);
}

template <typename OutT>
__global__ void ncl_to_rows_kernel(const float* __restrict__ in, int C, int L, int ldo, int64_t n, OutT* __restrict__ out,
                                   const int* __restrict__ len, const int* __restrict__ row_off) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over [B][L][ldo]
    if (i >= n) return;
    const int c = (int)(i % ldo);
    const int64_t r = i / ldo;
    const int t = (int)(r % L);
    const int64_t b = r / L;
    const float v = c < C ? in[(b * C + c) * L + t] : 0.f;
    if (row_off) {  // packed destination: only the frames the sequence owns exist
        if (t < len[b]) store1(out + ((int64_t)row_off[b] + t) * ldo + c, v);
    } else {
        store1(out + i, v);
    }
}
void launch_ncl_to_rows(hipStream_t s, int out_dtype, const float* in, int B, int C, int L, void* out, int ld_out, const int* len,
                        const int* row_off) {
    const int ldo = ld_out > 0 ? ld_out : C;
    const int64_t n = (int64_t)B * ldo * L;
    if (n == 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    with_out_type(out_dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        STN_KLAUNCH(ncl_to_rows_kernel<T>, grid, dim3(256), 0, s, in, C, L, ldo, n, static_cast<T*>(out), len, row_off);
    });
}

// 32 x 32 LDS tile transpose: reads of v are coalesced along d, writes of out along t.  ZT != void: the new latent is ALSO written as the rows the
// next step's input projection reads (z[row][d], row stride ldz, the activation format — what launch_ncl_to_rows would make of `out`, bit for bit), through
// a second transpose of the tile: the step after this one starts without that launch (its strided reads cost 11 us for 6 MB).
template <typename ZT>
__global__ __launch_bounds__(256) void euler_ncl_kernel(const float* __restrict__ prev, const float* __restrict__ v,
                                                        const float* __restrict__ dt, const int* __restrict__ len, int D, int L,
                                                        float* __restrict__ out, const int* __restrict__ row_off, ZT* __restrict__ z, int ldz) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int n = len ? len[b] : L;
    const int64_t vrow0 = row_off ? (int64_t)row_off[b] : (int64_t)b * L;
    const int vrows = row_off ? n : L;  // rows of v this sequence owns
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = t0 + ty + 8 * k, d = d0 + tx;
        tile[ty + 8 * k][tx] = (t < vrows && d < D) ? v[(vrow0 + t) * D + d] : 0.f;
    }
    __syncthreads();
    const float scale = dt[b];
    float nv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = d0 + ty + 8 * k, t = t0 + tx;
        nv[k] = 0.f;
        if (d < D && t < L) {
            const int64_t o = ((int64_t)b * D + d) * L + t;
            nv[k] = t < n ? prev[o] + tile[tx][ty + 8 * k] * scale : 0.f;
            out[o] = nv[k];
        }
    }
    if constexpr (!std::is_same<ZT, void>::value) {
        __syncthreads();  // every read of the velocity tile is done
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[ty + 8 * k][tx] = nv[k];  // [d][t]
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = t0 + ty + 8 * k, d = d0 + tx;
            if (t < vrows && d < D) store1(z + (vrow0 + t) * ldz + d, tile[tx][ty + 8 * k]);
        }
    }
}
void launch_euler_ncl(hipStream_t s, const float* prev, const float* v, const float* dt, const int* len, int B, int D, int L, float* out,
                      const int* row_off, void* z_rows, int z_dtype, int ldz) {
    if (B * D * L == 0) return;
    if (row_off && !len) { throw std::invalid_argument("packed euler_ncl needs lengths"); }
    const dim3 grid((L + 31) / 32, (D + 31) / 32, B);
    if (!z_rows) {
        STN_KLAUNCH(euler_ncl_kernel<void>, grid, dim3(256), 0, s, prev, v, dt, len, D, L, out, row_off, static_cast<void*>(nullptr), 0);
        return;
    }
    with_out_type(z_dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        STN_KLAUNCH(euler_ncl_kernel<T>, grid, dim3(256), 0, s, prev, v, dt, len, D, L, out, row_off, static_cast<T*>(z_rows), ldz);
    });
}

// row_off[b] = sum of len[0..b) (row_off[B] = total), row_b[row_off[b] + t] = b: the packed-row bookkeeping, one block
__global__ void row_map_kernel(const int* __restrict__ len, int B, int* __restrict__ row_off, int* __restrict__ row_b, int rows_padded) {
    __shared__ int off_s[1025];
    // exclusive prefix sum of up to 1024 lengths: every thread loads one, Hillis-Steele over LDS (10 steps), instead of one thread walking them
    const int tid = threadIdx.x;
    int v = tid < B ? len[tid] : 0;
    off_s[tid + 1] = v;
    if (tid == 0) off_s[0] = 0;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int add = tid + 1 > d ? off_s[tid + 1 - d] : 0;
        __syncthreads();
        if (tid + 1 > d) off_s[tid + 1] += add;
        __syncthreads();
    }
    for (int b = tid; b <= B; b += blockDim.x) row_off[b] = off_s[b];
    if (!row_b) return;
    // row -> sequence: every thread walks its own rows and finds the sequence by bisection over the offsets (B <= 1024: 10 steps)
    const int total = off_s[B];
    for (int r = tid; r < total; r += blockDim.x) {
        int lo = 0, hi = B;  // off_s[lo] <= r < off_s[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off_s[mid] <= r) lo = mid; else hi = mid; }
        row_b[r] = lo;
    }
    // dead rows behind the last sequence (a row count rounded up to a shape bucket): sequence 0, so that per-row lookups stay in range
    for (int t = total + tid; t < rows_padded; t += blockDim.x) row_b[t] = 0;
}

// packed rows [sum len][W] -> padded [B][T][W] with zeros past each sequence's length (W % 4 == 0)
__global__ void unpack_rows_kernel(const float* __restrict__ src, const int* __restrict__ len, const int* __restrict__ row_off, int T,
                                   int W4, int64_t n4, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over [B][T][W/4]
    if (i >= n4) return;
    const int c = (int)(i % W4);
    const int64_t r = i / W4;
    const int t = (int)(r % T);
    const int b = (int)(r / T);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < len[b]) v = reinterpret_cast<const float4*>(src)[((int64_t)row_off[b] + t) * W4 + c];
    reinterpret_cast<float4*>(dst)[i] = v;
}
void launch_unpack_rows(hipStream_t s, const float* src, const int* len, const int* row_off, int B, int T, int W, float* dst) {
    const int64_t n4 = (int64_t)B * T * (W / 4);
    if (n4 == 0) return;
    if (W % 4) { throw std::invalid_argument("unpack_rows needs W % 4 == 0"); }
    STN_KLAUNCH(unpack_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, src, len, row_off, T, W / 4, n4, dst);
}
void launch_row_map(hipStream_t s, const int* len, int B, int* row_off, int* row_b, int rows_padded) {
    if (B <= 0) return;
    if (B > 1024) { throw std::invalid_argument("packed layout supports at most 1024 sequences per batch"); }
    STN_KLAUNCH(row_map_kernel, dim3(1), dim3(1024), 0, s, len, B, row_off, row_b, rows_padded);
}

template <typename OutT>
__global__ void cast_kernel(const float* __restrict__ in, int64_t n, OutT* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) store1(out + i, in[i]);
}
void launch_cast(hipStream_t s, int out_dtype, const float* in, int64_t n, void* out) {
    if (n == 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    with_out_type(out_dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        STN_KLAUNCH(cast_kernel<T>, grid, dim3(256), 0, s, in, n, static_cast<T*>(out));
    });
}

__global__ void add_rowvec_kernel(float* __restrict__ x, const float* __restrict__ v, int ldv, int L, int C4, int64_t n4,
                                  const int* __restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over [B*L][C/4]
    if (i >= n4) return;
    const int c4 = (int)(i % C4);
    const int64_t r = i / C4;
    const int t = (int)(r % L);
    const int b = (int)(r / L);
    if (len && t >= len[b]) return;
    float4* xp = reinterpret_cast<float4*>(x) + i;
    const float4 a = *xp, d = *reinterpret_cast<const float4*>(v + (int64_t)b * ldv + c4 * 4);
    *xp = make_float4(a.x + d.x, a.y + d.y, a.z + d.z, a.w + d.w);
}
void launch_add_rowvec(hipStream_t s, float* x, const float* v, int ldv, int B, int L, int C, const int* len) {
    const int64_t n4 = (int64_t)B * L * (C / 4);
    if (n4 == 0) return;
    if (C % 4 || ldv % 4) { throw std::invalid_argument("add_rowvec needs C % 4 == 0"); }
    STN_KLAUNCH(add_rowvec_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, x, v, ldv, L, C / 4, n4, len);
}

__global__ void time_embed_kernel(const float* __restrict__ cur, const float* __restrict__ tot, int dim, float scale,
                                  float* __restrict__ te) {
    const int b = blockIdx.x, hd = dim >> 1;
    const float t = cur[b] / tot[b] * scale;
    for (int i = threadIdx.x; i < hd; i += blockDim.x) {
        const float f = expf(-logf(10000.0f) * (float)i / (float)hd);
        te[(int64_t)b * dim + i] = sinf(t * f);
        te[(int64_t)b * dim + hd + i] = cosf(t * f);
    }
}
void launch_time_embed(hipStream_t s, const float* cur, const float* tot, int B, int dim, float scale, float* te) {
    if (B == 0) return;
    STN_KLAUNCH(time_embed_kernel, dim3(B), dim3(64), 0, s, cur, tot, dim, scale, te);
}

// ---------------------------------------------------------------------------------------------
// vocoder front: frame (b, t = l*ccf + j) channel c  <-  latent[b][j*ld + c][l];   conv ld -> C, kernel k
// 8 frames per workgroup; the (8 + k - 1) x ld input window sits in LDS; weights [ld*k][C] (co contiguous).
// ---------------------------------------------------------------------------------------------
static constexpr int VI_FR = 8;
__global__ __launch_bounds__(256) void vocoder_in_kernel(const float* __restrict__ latent, int L, int ld, int ccf,
                                                         const float* __restrict__ w_t, const float* __restrict__ bias,
                                                         int C, int k, float* __restrict__ x, const int* __restrict__ seqlen) {
    extern __shared__ __attribute__((aligned(16))) float win[];  // [(VI_FR + k - 1)][ld]
    const int T = L * ccf, D = ld * ccf;
    const int tiles = (T + VI_FR - 1) / VI_FR;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * VI_FR;
    const int half = (k - 1) >> 1, nwin = VI_FR + k - 1;
    for (int i = threadIdx.x; i < nwin * ld; i += blockDim.x) {
        const int f = i / ld, c = i - f * ld;
        const int t = t0 - half + f;
        float v = 0.f;
        if (t >= 0 && t < (seqlen ? seqlen[b] : T)) {
            const int l = t / ccf, j = t - l * ccf;
            v = latent[((int64_t)b * D + j * ld + c) * L + l];
        }
        win[i] = v;
    }
    __syncthreads();
    for (int co = threadIdx.x; co < C; co += blockDim.x) {
        float acc[VI_FR];
        const float bv = bias[co];
#pragma unroll
        for (int f = 0; f < VI_FR; ++f) acc[f] = bv;
        for (int ci = 0; ci < ld; ++ci)
            for (int j = 0; j < k; ++j) {
                const float wv = w_t[(int64_t)(ci * k + j) * C + co];
#pragma unroll
                for (int f = 0; f < VI_FR; ++f) acc[f] = fmaf(wv, win[(f + j) * ld + ci], acc[f]);
            }
#pragma unroll
        for (int f = 0; f < VI_FR; ++f)
            if (t0 + f < T) x[((int64_t)b * T + t0 + f) * C + co] = acc[f];
    }
}
void launch_vocoder_in(hipStream_t s, const float* latent, int B, int L, int ld, int ccf, const float* w_t,
                       const float* bias, int C, int k, float* x, const int* seqlen) {
    const int T = L * ccf;
    if (B * T == 0) return;
    const int tiles = (T + VI_FR - 1) / VI_FR;
    const size_t lds = sizeof(float) * (size_t)(VI_FR + k - 1) * ld;
    STN_KLAUNCH(vocoder_in_kernel, dim3(B * tiles), dim3(256), lds, s, latent, L, ld, ccf, w_t, bias, C, k, x, seqlen);
}

// cols[(b, t)][ci * k + j] = latent frame (t + j - (k-1)/2) of sequence b, channel ci (zero outside the sequence; columns >= ld * k are the GEMM's K
// padding), where frame tt of the vocoder is latent position l = tt / ccf, channel block q = tt % ccf: latent[b][q * ld + ci][l].
// A workgroup owns IM2_TF consecutive frames of one sequence: it stages the latent positions they touch in LDS ([channel][l], the reads run along l) and
// writes whole rows of cols, consecutive lanes consecutive columns (the former one-thread-per-element form gathered 4 bytes per lane with four integer
// divisions each: 38 us for the bench's 23 MB).
constexpr int IM2_TF = 32;
// FIXED: the published shape (24 latent channels x 6, k = 7, K padded to 192) as compile-time constants — the index arithmetic is three divisions per
// element, and with run-time divisors they, not the bytes, set the kernel's time; with them and eight columns per 16-byte store 38 -> 17 us
template <typename OutT, bool FIXED>
__global__ __launch_bounds__(256) void vocoder_im2col_kernel(const float* __restrict__ latent, int L, int ld_, int ccf_, int k_, int kp_,
                                                             OutT* __restrict__ cols, const int* __restrict__ seqlen, const int* __restrict__ row_off) {
    extern __shared__ float im2_sm[];  // [D][NL]
    const int ld = FIXED ? 24 : ld_, ccf = FIXED ? 6 : ccf_, k = FIXED ? 7 : k_, kp = FIXED ? 192 : kp_;
    const int T = L * ccf, D = ld * ccf, half = (k - 1) >> 1;
    const int tiles = (T + IM2_TF - 1) / IM2_TF;
    const int b = (int)blockIdx.x / tiles, t0 = ((int)blockIdx.x % tiles) * IM2_TF;
    const int n = seqlen ? seqlen[b] : T;            // frames of this sequence that exist (taps beyond read zero)
    if (row_off && t0 >= n) return;                  // packed destination: no such rows
    const int l0 = max(t0 - half, 0) / ccf, l1 = min((min(t0 + IM2_TF, T) - 1 + half) / ccf, L - 1), NL = l1 - l0 + 1;
    for (int i = threadIdx.x; i < D * NL; i += 256) {
        const int d = i / NL, l = i - d * NL;
        im2_sm[i] = latent[((int64_t)b * D + d) * L + l0 + l];
    }
    __syncthreads();
    const int t1 = min(t0 + IM2_TF, row_off ? n : T);
    const int64_t row00 = row_off ? (int64_t)row_off[b] : (int64_t)b * T;
    auto value = [&](int t, int col) {
        float v = 0.f;
        if (col < ld * k) {
            const int ci = col / k, j = col - ci * k, tt = t + j - half;
            if (tt >= 0 && tt < n) { const int l = tt / ccf, q = tt - l * ccf; v = im2_sm[(q * ld + ci) * NL + (l - l0)]; }
        }
        return v;
    };
    if constexpr (FIXED && sizeof(OutT) == 2) {  // eight columns per thread: one 16-byte store (kp = 192 = 24 x 8)
        for (int i = threadIdx.x; i < (t1 - t0) * 24; i += 256) {
            const int r = i / 24, c8 = i - r * 24, t = t0 + r;
            OutT tmp[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) store1(tmp + e, value(t, c8 * 8 + e));
            *reinterpret_cast<uint4*>(cols + (row00 + t) * kp + c8 * 8) = *reinterpret_cast<const uint4*>(tmp);
        }
    } else {
        for (int i = threadIdx.x; i < (t1 - t0) * kp; i += 256) {
            const int r = i / kp, col = i - r * kp, t = t0 + r;
            store1(cols + (row00 + t) * kp + col, value(t, col));
        }
    }
}
void launch_vocoder_im2col(hipStream_t s, int out_dtype, const float* latent, int B, int L, int ld, int ccf, int k, int kp, void* cols,
                           const int* seqlen, const int* row_off) {
    if ((int64_t)B * L * ccf * kp == 0) return;
    const int T = L * ccf, tiles = (T + IM2_TF - 1) / IM2_TF;
    const int nl_max = (IM2_TF + k - 1) / ccf + 2;
    const size_t lds = sizeof(float) * (size_t)ld * ccf * nl_max;
    if (lds > 64 * 1024 || (int64_t)B * tiles > 0x7FFFFFFFll) throw std::invalid_argument("launch_vocoder_im2col: latent window does not fit the staging buffer");
    const dim3 grid((unsigned)(B * tiles));
    const bool fixed = ld == 24 && ccf == 6 && k == 7 && kp == 192;
    with_out_type(out_dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        if (fixed) STN_KLAUNCH((vocoder_im2col_kernel<T, true>), grid, dim3(256), lds, s, latent, L, ld, ccf, k, kp, static_cast<T*>(cols), seqlen, row_off);
        else STN_KLAUNCH((vocoder_im2col_kernel<T, false>), grid, dim3(256), lds, s, latent, L, ld, ccf, k, kp, static_cast<T*>(cols), seqlen, row_off);
    });
}

template <typename InT>
__global__ void masked_mean_kernel(const InT* __restrict__ x, int L, int C, const int* __restrict__ len,
                                   float* __restrict__ pooled, const int* __restrict__ row_off) {
    const int b = blockIdx.x, n = len[b];
    const int64_t r0 = row_off ? (int64_t)row_off[b] : (int64_t)b * L;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float s = 0.f;
        for (int t = 0; t < n; ++t) s += load1(x + (r0 + t) * C + c);
        pooled[(int64_t)b * C + c] = s / (float)(n > 0 ? n : 1);
    }
}
void launch_masked_mean(hipStream_t s, int in_dtype, const void* x, int B, int L, int C, const int* len, float* pooled,
                        const int* row_off) {
    if (B == 0) return;
    with_out_type(in_dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        STN_KLAUNCH(masked_mean_kernel<T>, dim3(B), dim3(128), 0, s, static_cast<const T*>(x), L, C, len, pooled, row_off);
    });
}

__global__ void softplus_kernel(float* x, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const float y = x[i]; x[i] = y > 20.f ? y : log1pf(expf(y)); }
}
void launch_softplus(hipStream_t s, float* x, int n) {
    if (n) STN_KLAUNCH(softplus_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, n);
}
__global__ void scale_kernel(float* x, int n, float mul) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= mul;
}
void launch_scale(hipStream_t s, float* x, int n, float mul) {
    if (n) STN_KLAUNCH(scale_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, n, mul);
}
__global__ void reciprocal_kernel(const float* in, int n, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = 1.0f / in[i];
}
void launch_reciprocal(hipStream_t s, const float* in, int n, float* out) {
    if (n) STN_KLAUNCH(reciprocal_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, n, out);
}
template <typename InT>
__global__ void half_to_f32_kernel(const InT* __restrict__ in, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = load1(in + i);
}
void launch_half_to_f32(hipStream_t s, int in_dtype, const void* in, int64_t n, float* out) {
    if (!n) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    with_half_type(in_dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        STN_KLAUNCH(half_to_f32_kernel<T>, grid, dim3(256), 0, s, static_cast<const T*>(in), n, out);
    });
}
void launch_bf16_to_f32(hipStream_t s, const uint16_t* in, int64_t n, float* out) { launch_half_to_f32(s, BF16, in, n, out); }
__global__ void fill_kernel(float* x, int n, float v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = v;
}
void launch_fill(hipStream_t s, float* x, int n, float v) {
    if (n) STN_KLAUNCH(fill_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, n, v);
}
// the step counters of a whole Euler loop in one launch: tot[st][b] = steps, cur[st][b] = st, dt[b] = 1 / steps
__global__ void step_counters_kernel(float* __restrict__ tot, float* __restrict__ cur, float* __restrict__ dt, int B, int steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * steps) { tot[i] = (float)steps; cur[i] = (float)(i / B); }
    if (i < B) dt[i] = 1.0f / (float)steps;
}
void launch_step_counters(hipStream_t s, float* tot, float* cur, float* dt, int B, int steps) {
    const int n = B * steps;
    if (n) STN_KLAUNCH(step_counters_kernel, dim3((n + 255) / 256), dim3(256), 0, s, tot, cur, dt, B, steps);
}

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 (kernels_dev.hpp) + Box-Muller; element (utt, d, t) depends only on (seed, utt, d, t)
// ---------------------------------------------------------------------------------------------
__global__ void randn_masked_kernel(unsigned long long seed, const unsigned long long* __restrict__ seed_dev,
                                    const int64_t* __restrict__ utt_ids, int D, int L, const int* __restrict__ len, int64_t n4,
                                    float* __restrict__ xt) {
    if (seed_dev) seed = *seed_dev;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over [B][D][ceil(L/4)]
    if (i >= n4) return;
    const int L4 = (L + 3) >> 2;
    const int t4 = (int)(i % L4);
    const int64_t r = i / L4;
    const int d = (int)(r % D);
    const int b = (int)(r / D);
    const unsigned long long u = utt_ids ? (unsigned long long)utt_ids[b] : (unsigned long long)b;
    unsigned c[4] = {(unsigned)t4, (unsigned)d, (unsigned)u, (unsigned)(u >> 32)};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    float nrm[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)(c[2 * h] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float u2 = ((float)(c[2 * h + 1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
        const float rr = sqrtf(-2.0f * logf(u1)), th = 6.28318530717958647692f * u2;
        nrm[2 * h] = rr * cosf(th);
        nrm[2 * h + 1] = rr * sinf(th);
    }
    const int nb = len ? len[b] : L;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int t = t4 * 4 + q;
        if (t < L) xt[((int64_t)b * D + d) * L + t] = t < nb ? nrm[q] : 0.f;
    }
}
void launch_randn_masked(hipStream_t s, uint64_t seed, const int64_t* utt_ids, int B, int D, int L, const int* len,
                         float* xt, const unsigned long long* seed_dev) {
    const int64_t n4 = (int64_t)B * D * ((L + 3) / 4);
    if (n4 == 0) return;
    STN_KLAUNCH(randn_masked_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (unsigned long long)seed,
                       seed_dev, utt_ids, D, L, len, n4, xt);
}

__global__ void scale_len_kernel(const int* __restrict__ len, int B, int factor, int* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) out[i] = len[i] * factor;
}
void launch_scale_len(hipStream_t s, const int* len, int B, int factor, int* out) {
    if (B == 0) return;
    STN_KLAUNCH(scale_len_kernel, dim3((B + 255) / 256), dim3(256), 0, s, len, B, factor, out);
}

// Extents of the exact "trimmed" dense vocoder: an utterance whose zero-latent padding is longer than twice the receptive
// field rf is computed on len*ccf + 2*rf frames (zero beyond), which is exact on its first len*ccf + rf output frames; the rest
// of its row is position-independent (quiet chunk + edge tail, see Engine::prepare_vocoder_constants).
// tail_form: every utterance is computed on its first min(len*ccf + rf, T) frames, all of them exact, because the convolutions read the
// frames beyond from the cached per-layer tails instead of zeros (DwconvTail).
__global__ void trim_len_kernel(const int* __restrict__ len, int B, int ccf, int T, int rf, int tail_form, int* __restrict__ n_out,
                                int* __restrict__ valid_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int l6 = len[i] * ccf;
    if (tail_form) {
        n_out[i] = valid_out[i] = l6 + rf < T ? l6 + rf : T;
        return;
    }
    const bool trim = l6 + 2 * rf <= T;  // the edge tail's whole receptive field [T - 2rf, T) is zero latent (quiet part may be empty)
    n_out[i] = trim ? l6 + 2 * rf : T;
    valid_out[i] = trim ? l6 + rf : T;
}
void launch_trim_len(hipStream_t s, const int* len, int B, int ccf, int T, int rf, int* n_out, int* valid_out, bool tail_form) {
    if (B == 0) return;
    STN_KLAUNCH(trim_len_kernel, dim3((B + 255) / 256), dim3(256), 0, s, len, B, ccf, T, rf, tail_form ? 1 : 0, n_out, valid_out);
}

// packed rows -> padded [B][T][W]: computed frames below valid[b], then the quiet chunk, then the edge tail of rf frames.
// A wavefront moves UNPACK_RW whole rows: where a row comes from is decided once per row (wave-uniform), and every 16-byte load of the rows is
// issued before the first store — the pass is a copy of the whole waveform and should cost what its bytes cost (one thread per 16 bytes with
// three run-time divisions each took 58 us for the 226 MB of a batch of 128, 3.9 TB/s).
constexpr int UNPACK_RW = 4;
__global__ __launch_bounds__(256) void unpack_rows_quiet_kernel(const float* __restrict__ src, const int* __restrict__ valid,
                                                                const int* __restrict__ row_off, int T, int W4, int rf,
                                                                const float* __restrict__ quiet, const float* __restrict__ edge, int64_t nrows,
                                                                float* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * UNPACK_RW;  // over [B][T]
    if (r0 >= nrows) return;
    const float4* sp[UNPACK_RW];
#pragma unroll
    for (int i = 0; i < UNPACK_RW; ++i) {
        const int64_t r = r0 + i < nrows ? r0 + i : nrows - 1;
        const int b = (int)(r / T), t = (int)(r - (int64_t)b * T);
        if (t < valid[b]) sp[i] = reinterpret_cast<const float4*>(src) + ((int64_t)row_off[b] + t) * W4;
        else if (t >= T - rf) sp[i] = reinterpret_cast<const float4*>(edge) + (int64_t)(t - (T - rf)) * W4;
        else sp[i] = reinterpret_cast<const float4*>(quiet);
    }
    float4* d4 = reinterpret_cast<float4*>(dst) + r0 * W4;
    for (int c = lane; c < W4; c += 64) {
        float4 v[UNPACK_RW];
#pragma unroll
        for (int i = 0; i < UNPACK_RW; ++i) v[i] = sp[i][c];
#pragma unroll
        for (int i = 0; i < UNPACK_RW; ++i)
            if (r0 + i < nrows) d4[(int64_t)i * W4 + c] = v[i];
    }
}
void launch_unpack_rows_quiet(hipStream_t s, const float* src, const int* valid, const int* row_off, int B, int T, int W, int rf,
                              const float* quiet, const float* edge, float* dst) {
    const int64_t nrows = (int64_t)B * T;
    if (nrows == 0 || W == 0) return;
    if (W % 4) { throw std::invalid_argument("unpack_rows needs W % 4 == 0"); }
    STN_KLAUNCH(unpack_rows_quiet_kernel, dim3((unsigned)((nrows + 4 * UNPACK_RW - 1) / (4 * UNPACK_RW))), dim3(256), 0, s, src, valid, row_off, T,
                W / 4, rf, quiet, edge, nrows, dst);
}

// The rows of [B][T][W] from valid[b] on, and nothing else: what a head GEMM that stores its packed rows in place (Epilogue::map_off) leaves to
// write.  The same decision per row as unpack_rows_quiet_kernel (edge tail, else quiet chunk), or zeros where there are no constants (quiet ==
// null: the length-aware form).  FILL_WG workgroups per sequence share its rest row by row, so every wavefront starts at a row it has to write;
// the quiet chunk is loaded once per wavefront, beside the sequence's extent, and stored to all of its rows.
constexpr int FILL_WG = 8;
__global__ __launch_bounds__(256) void fill_rows_kernel(const int* __restrict__ valid, int T, int W4, int rf, const float* __restrict__ quiet,
                                                        const float* __restrict__ edge, float* __restrict__ dst) {
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int w = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6), nw = (int)gridDim.y * 4;  // this wavefront among the sequence's
    const int v0 = valid[b];
    float4* d4 = reinterpret_cast<float4*>(dst) + (int64_t)b * T * W4;
    for (int c = lane; c < W4; c += 64) {
        const float4 q = quiet ? reinterpret_cast<const float4*>(quiet)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = v0 + w; t < T; t += nw) {
            float4 v = q;
            if (quiet && t >= T - rf) v = reinterpret_cast<const float4*>(edge)[(int64_t)(t - (T - rf)) * W4 + c];
            d4[(int64_t)t * W4 + c] = v;
        }
    }
}
void launch_fill_rows(hipStream_t s, const int* valid, int B, int T, int W, int rf, const float* quiet, const float* edge, float* dst) {
    if (B <= 0 || T <= 0 || W == 0) return;
    if (W % 4) { throw std::invalid_argument("fill_rows needs W % 4 == 0"); }
    if (quiet && rf > 0 && !edge) { throw std::invalid_argument("fill_rows: the quiet rule needs the edge tail"); }
    if (rf < 0 || rf > T) { throw std::invalid_argument("fill_rows: rf outside [0, T]"); }
    STN_KLAUNCH(fill_rows_kernel, dim3((unsigned)B, FILL_WG), dim3(256), 0, s, valid, T, W / 4, rf, quiet, quiet ? edge : nullptr, dst);
}

__global__ void mask_ncl_kernel(float* __restrict__ x, int D, int L, int64_t n, const int* __restrict__ len) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t = (int)(i % L);
    const int b = (int)(i / ((int64_t)D * L));
    if (t >= len[b]) x[i] = 0.f;
}
void launch_mask_ncl(hipStream_t s, float* x, int B, int D, int L, const int* len) {
    const int64_t n = (int64_t)B * D * L;
    if (n == 0) return;
    STN_KLAUNCH(mask_ncl_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, D, L, n, len);
}

}  // namespace stn
