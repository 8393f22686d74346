// kernels_output.hip — the end of every fetch (gfx950, wave64): the one store (store_rows_kernel: fp32 or an encoding, with or without a gain) and
// the GPU join of long-form chunks: one walk (join_walk) behind two entry points, join_rows_kernel and, from trimmed, faded sources,
// join_trim_rows_kernel.  The per-sample encoding rules are the device functions of kernels_dev.hpp.  Each kernel has a dithering
// twin (*_dither_kernel: the same body under a compile-time mode) that is launched only while a mode is set.
#include "kernels.hpp"
#include "kernels_dev.hpp"

namespace stn {

// The final store of a fetch: V samples per thread, times the row's gain when kGain, in encoding kEnc (kernels_dev.hpp).  Vector form:
// 16-B loads, V = 4 (fp32: one 16-B store), 8 (PCM16: one 16-B store) or 16 (mu-law / A-law: one 16-B store; PCM24: three, 48 B);
// scalar form (V = 1): one sample, enc_store1.  x and y may be the same fp32 rows (dst_stride == W: the gain applied in place), so
// neither is __restrict__.
template <int kEnc>
constexpr int store_vec() { return kEnc == ENC_F32 ? 4 : kEnc == ENC_PCM16 ? 8 : 16; }

// eight 16-bit codes / sixteen 24-bit codes as one / three 16-B stores at y (16-byte aligned): the packing of enc_store_vec below, for
// the dithering store (enc_store_vec keeps its own text, and with it the device code it had before there was a dithering twin)
__device__ __forceinline__ void pack_store_pcm16(unsigned char* y, const int (&c)[8]) {
    unsigned o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = ((unsigned)c[2 * j] & 0xFFFFu) | ((unsigned)c[2 * j + 1] << 16);
    *reinterpret_cast<uint4*>(y) = make_uint4(o[0], o[1], o[2], o[3]);
}
__device__ __forceinline__ void pack_store_pcm24(unsigned char* y, const int (&q)[16]) {
    // sample j's three bytes at 3j .. 3j+2 of 48: word w = bits [32w, 32w + 32) of the 384-bit little-endian run
    unsigned o[12] = {};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const unsigned c = (unsigned)q[j] & 0xFFFFFFu;
        const int b = 24 * j, w = b >> 5, sh = b & 31;
        o[w] |= c << sh;
        if (sh > 8) o[w + 1] |= c >> (32 - sh);
    }
    uint4* d = reinterpret_cast<uint4*>(y);
    d[0] = make_uint4(o[0], o[1], o[2], o[3]);
    d[1] = make_uint4(o[4], o[5], o[6], o[7]);
    d[2] = make_uint4(o[8], o[9], o[10], o[11]);
}

// V consecutive samples v, encoded, to sample index e of y: one sample by enc_store1 (V == 1), else V = store_vec<kEnc>() samples in
// one 16-B store (three for PCM24); y + e samples is then 16-byte aligned
template <int V, int kEnc>
__device__ __forceinline__ void enc_store_vec(unsigned char* y, int64_t e, const float (&v)[V]) {
    if constexpr (V == 1) {
        enc_store1<kEnc>(y, e, v[0]);
    } else if constexpr (kEnc == ENC_F32) {
        *reinterpret_cast<float4*>(y + e * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (kEnc == ENC_PCM16) {
        unsigned o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ((unsigned)pcm16(v[2 * j]) & 0xFFFFu) | ((unsigned)pcm16(v[2 * j + 1]) << 16);
        *reinterpret_cast<uint4*>(y + e * 2) = make_uint4(o[0], o[1], o[2], o[3]);
    } else if constexpr (kEnc == ENC_PCM24) {
        // sample j's three bytes at 3j .. 3j+2 of 48: word w = bits [32w, 32w + 32) of the 384-bit little-endian run
        unsigned o[12] = {};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned c = (unsigned)pcm24(v[j]) & 0xFFFFFFu;
            const int b = 24 * j, w = b >> 5, sh = b & 31;
            o[w] |= c << sh;
            if (sh > 8) o[w + 1] |= c >> (32 - sh);
        }
        uint4* d = reinterpret_cast<uint4*>(y + e * 3);
        d[0] = make_uint4(o[0], o[1], o[2], o[3]);
        d[1] = make_uint4(o[4], o[5], o[6], o[7]);
        d[2] = make_uint4(o[8], o[9], o[10], o[11]);
    } else {
        unsigned o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int s16 = pcm16(v[4 * j + k]);
                w |= (kEnc == ENC_MULAW ? mulaw8(s16) : alaw8(s16)) << (8 * k);
            }
            o[j] = w;
        }
        *reinterpret_cast<uint4*>(y + e) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// The dithered store (the rule is dither.hpp's): a launch's stream key, and one thread's place in a stream.
// ids: the rows' (programmes') 64-bit ids, null for the row (programme) index itself.
struct DitherArgs { uint64_t seed; const int64_t* ids; unsigned kind; const int64_t* lim; int64_t lim_stride; };
struct NoDither {};
__device__ __forceinline__ uint64_t dither_id(const DitherArgs& d, int64_t row) { return d.ids ? (uint64_t)d.ids[row] : (uint64_t)row; }
__device__ __forceinline__ uint64_t dither_id(const NoDither&, int64_t) { return 0; }
__device__ __forceinline__ int64_t dither_lim(const DitherArgs& d, int64_t row) { return d.lim ? d.lim[row * d.lim_stride] : INT64_MAX; }

// one sample of the stream at index n, v, to sample index e of y; samples at and behind lim (a programme's end) are the zero codeword
template <int kEnc, int kMode>
__device__ __forceinline__ void enc_store1_dither(unsigned char* y, int64_t e, float v, uint64_t seed, unsigned kind, uint64_t id, int64_t n, int64_t lim) {
    static_assert(kEnc == ENC_PCM16 || kEnc == ENC_PCM24, "dither is of the integer PCM encodings");
    constexpr int S = kEnc == ENC_PCM16 ? 32767 : 8388607;
    const int c = n < lim ? dither_sample<kMode, S>(seed, kind, id, n, v) : 0;
    if constexpr (kEnc == ENC_PCM16) {
        reinterpret_cast<int16_t*>(y)[e] = (int16_t)c;
    } else {
        y[3 * e] = (unsigned char)c; y[3 * e + 1] = (unsigned char)(c >> 8); y[3 * e + 2] = (unsigned char)(c >> 16);
    }
}
// V consecutive samples from stream index n0 (a multiple of 4: the vector forms' V is 8 or 16): one Philox block per four samples, live
// one at a time (four words and the predecessor's a), and for TPDF_HP the block in front of the first, of which only the last a is kept
template <int V, int kEnc, int kMode>
__device__ __forceinline__ void enc_store_vec_dither(unsigned char* y, int64_t e, const float (&v)[V], uint64_t seed, unsigned kind, uint64_t id, int64_t n0,
                                                     int64_t lim) {
    if constexpr (V == 1) {
        enc_store1_dither<kEnc, kMode>(y, e, v[0], seed, kind, id, n0, lim);
    } else {
        static_assert(kEnc == ENC_PCM16 || kEnc == ENC_PCM24, "dither is of the integer PCM encodings");
        static_assert(V % 4 == 0, "whole Philox blocks");
        constexpr int S = kEnc == ENC_PCM16 ? 32767 : 8388607;
        int c[V];
        if (n0 >= lim) {  // (padding behind the programme)
#pragma unroll
            for (int j = 0; j < V; ++j) c[j] = 0;
        } else {
            unsigned prev = 0;
            if constexpr (kMode == DITHER_TPDF_HP) {
                if (n0 > 0) {
                    unsigned u[4];
                    dither_block(seed, kind, id, (n0 >> 2) - 1, u);
                    prev = u[3] & 0xFFFFu;
                }
            }
#pragma unroll
            for (int b = 0; b < V / 4; ++b) {
                unsigned w[4] = {};
                if constexpr (kMode != DITHER_ROUND) dither_block(seed, kind, id, (n0 >> 2) + b, w);
                if constexpr (kMode == DITHER_TPDF_HP) {
                    if (b == 0 && n0 == 0) prev = w[0] >> 16;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int q = dither_quantize<S>(v[4 * b + k], dither_num<kMode>(w[k], prev));
                    prev = w[k] & 0xFFFFu;
                    c[4 * b + k] = n0 + 4 * b + k < lim ? q : 0;
                }
            }
        }
        if constexpr (kEnc == ENC_PCM16) pack_store_pcm16(y + e * 2, c);
        else pack_store_pcm24(y + e * 3, c);
    }
}

// the dithering store's body (both of its kernels): store_rows_kernel below with the dithered quantizer in place of the encoding
template <int V, bool kGain, int kEnc, int kMode>
__device__ __forceinline__ void store_rows_body(const float* x, int64_t Wv, int64_t nv, const float* __restrict__ g, unsigned char* y, int64_t dst_stride,
                                                const DitherArgs& d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over [rows][W/V]
    if (i >= nv) return;
    const int64_t row = i / Wv;
    float v[V];
    if constexpr (V == 1) {
        v[0] = x[i];
    } else {
#pragma unroll
        for (int j = 0; j < V / 4; ++j) {
            const float4 a = reinterpret_cast<const float4*>(x)[i * (V / 4) + j];
            v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w;
        }
    }
    if constexpr (kGain) {
        const float s = g[row];
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] *= s;
    }
    const int64_t n0 = (i - row * Wv) * V;  // the first sample's place in its row; without lengths all W samples are dithered
    enc_store_vec_dither<V, kEnc, kMode>(y, row * dst_stride + n0, v, d.seed, d.kind, dither_id(d, row), n0, dither_lim(d, row));
}
// (the store without dither keeps its own text: as a call of the body above its gain load compiles to other instructions)
template <int V, bool kGain, int kEnc>
__global__ void store_rows_kernel(const float* x, int64_t Wv, int64_t nv, const float* __restrict__ g, unsigned char* y, int64_t dst_stride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over [rows][W/V]
    if (i >= nv) return;
    const int64_t row = i / Wv;
    float v[V];
    if constexpr (V == 1) {
        v[0] = x[i];
    } else {
#pragma unroll
        for (int j = 0; j < V / 4; ++j) {
            const float4 a = reinterpret_cast<const float4*>(x)[i * (V / 4) + j];
            v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w;
        }
    }
    if constexpr (kGain) {
        const float s = g[row];
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] *= s;
    }
    enc_store_vec<V, kEnc>(y, row * dst_stride + (i - row * Wv) * V, v);  // (first destination sample)
}
template <int V, bool kGain, int kEnc, int kMode>
__global__ void store_rows_dither_kernel(const float* x, int64_t Wv, int64_t nv, const float* __restrict__ g, unsigned char* y, int64_t dst_stride, DitherArgs d) {
    store_rows_body<V, kGain, kEnc, kMode>(x, Wv, nv, g, y, dst_stride, d);
}
// (the one-sample form under a name of its own: the launch log, which keeps names only, then tells which form ran)
template <bool kGain, int kEnc, int kMode>
__global__ void store_rows_dither1_kernel(const float* x, int64_t Wv, int64_t nv, const float* __restrict__ g, unsigned char* y, int64_t dst_stride, DitherArgs d) {
    store_rows_body<1, kGain, kEnc, kMode>(x, Wv, nv, g, y, dst_stride, d);
}
// a dithering mode as a template argument (the integer PCM encodings only; every other encoding is stored as without)
template <typename Fn>
static void with_dither_mode(int mode, const char* who, Fn&& fn) {
    switch (mode) {
        case DITHER_ROUND: fn(std::integral_constant<int, DITHER_ROUND>{}); break;
        case DITHER_TPDF: fn(std::integral_constant<int, DITHER_TPDF>{}); break;
        case DITHER_TPDF_HP: fn(std::integral_constant<int, DITHER_TPDF_HP>{}); break;
        default: throw std::invalid_argument(std::string(who) + ": unknown dither mode " + std::to_string(mode));
    }
}
static bool dithers(const Dither& d, int enc, const char* who, int64_t W) {
    if (d.mode == DITHER_OFF || (enc != ENC_PCM16 && enc != ENC_PCM24)) return false;
    if (W > DITHER_MAX_N) throw std::invalid_argument(std::string(who) + ": a dithered row is limited to 2^34 samples");
    return true;
}

template <int kEnc>
void launch_store_rows_t(hipStream_t s, const float* x, int64_t rows, int64_t W, const float* g, unsigned char* y, int64_t dst_stride, const Dither& dth) {
    const int64_t n = rows * W;
    if (n <= 0) return;
    if (dst_stride < W) throw std::invalid_argument("store_rows: dst_stride smaller than the row length");
    constexpr int V = store_vec<kEnc>();
    const bool vec = W % V == 0 && dst_stride % V == 0 && !(reinterpret_cast<uintptr_t>(x) & 15) && !(reinterpret_cast<uintptr_t>(y) & 15);
    const int64_t nv = vec ? n / V : n;
    const dim3 grid((unsigned)((nv + 255) / 256));
    if constexpr (kEnc == ENC_PCM16 || kEnc == ENC_PCM24) {
        if (dithers(dth, kEnc, "store_rows", W)) {
            const DitherArgs d{dth.seed, dth.ids, dth.kind, dth.lim, dth.lim_stride};
            with_dither_mode(dth.mode, "store_rows", [&](auto m) {
                constexpr int kMode = decltype(m)::value;
                if (vec && g) STN_KLAUNCH((store_rows_dither_kernel<V, true, kEnc, kMode>), grid, dim3(256), 0, s, x, W / V, nv, g, y, dst_stride, d);
                else if (vec) STN_KLAUNCH((store_rows_dither_kernel<V, false, kEnc, kMode>), grid, dim3(256), 0, s, x, W / V, nv, g, y, dst_stride, d);
                else if (g) STN_KLAUNCH((store_rows_dither1_kernel<true, kEnc, kMode>), grid, dim3(256), 0, s, x, W, nv, g, y, dst_stride, d);
                else STN_KLAUNCH((store_rows_dither1_kernel<false, kEnc, kMode>), grid, dim3(256), 0, s, x, W, nv, g, y, dst_stride, d);
            });
            return;
        }
    }
    if (vec && g) STN_KLAUNCH((store_rows_kernel<V, true, kEnc>), grid, dim3(256), 0, s, x, W / V, nv, g, y, dst_stride);
    else if (vec) STN_KLAUNCH((store_rows_kernel<V, false, kEnc>), grid, dim3(256), 0, s, x, W / V, nv, g, y, dst_stride);
    else if (g) STN_KLAUNCH((store_rows_kernel<1, true, kEnc>), grid, dim3(256), 0, s, x, W, nv, g, y, dst_stride);
    else STN_KLAUNCH((store_rows_kernel<1, false, kEnc>), grid, dim3(256), 0, s, x, W, nv, g, y, dst_stride);
}
void launch_store_rows(hipStream_t s, const float* x, int64_t rows, int64_t W, const float* g, int enc, void* y, int64_t dst_stride, const Dither& d) {
    with_enc(enc, "store_rows", [&](auto e) { launch_store_rows_t<decltype(e)::value>(s, x, rows, W, g, static_cast<unsigned char*>(y), dst_stride, d); });
}

// The join of a fetch: programme p's output row is its members' segments with gaps between them,
// seg[m].len samples of source row seg[m].row landing at seg[m].dst, everything else of [0, Wj) the encoding's zero codeword (the
// encoding of +0.0f).  One workgroup per (tile of JOIN_WG * V * T output samples, programme): it stages the programme's members in LDS
// once (one load per lane; members past JOIN_WG, which a chunked text never has, are read from the table), and a thread, which owns T vectors of V
// consecutive output samples JOIN_WG * V apart, finds for each the first member that ends behind its first sample by a binary search over the members' ascending
// ends in LDS.  Inside one segment the V samples are 16-B loads that ask for dword alignment only (a segment's offset against its row
// is arbitrary: the hardware takes a dwordx4 at any dword address) and the store of store_rows_kernel; a vector that meets a segment
// edge, a gap or the row's end selects per sample, and the last, partial vector of a row is stored sample by sample.  No sample
// outside a member's [0, len) is read, nothing outside [0, Wj) of a row is written.  kGain: times g[source row], the product
// store_rows_kernel forms.
constexpr int JOIN_WG = 256;
typedef float join_f4 __attribute__((ext_vector_type(4), aligned(4)));  // four floats at a dword-aligned address

// The walk behind both entry points.  kTrim (the join from trimmed sources): a member's samples start at its
// source offset seg[m].src, and its cut edges are faded by the window `fade` in global memory: a vector that meets a fade takes the
// per-sample path.  A delivered sample is ((x * g) * w_in) * w_out, each multiply only where it applies.  The entry points declare the
// LDS arrays (s_src and s_fade: the trimmed one only, null otherwise).
template <int V, int T, bool kGain, int kEnc, bool kTrim, int kMode = DITHER_OFF, typename D = NoDither>
__device__ __forceinline__ void join_walk(const float* __restrict__ x, int64_t src_stride,
                                          const std::conditional_t<kTrim, JoinSegT, JoinSeg>* __restrict__ seg, const JoinProg* __restrict__ prog,
                                          const float* __restrict__ g, const float* __restrict__ fade, int64_t Wj, unsigned char* __restrict__ y,
                                          int64_t dst_stride, int64_t* s_dst, int64_t* s_len, int64_t* s_row, int64_t* s_src, int2* s_fade, const D& d = D{}) {
    const int p = blockIdx.y, tid = threadIdx.x;
    const JoinProg pg = prog[p];
    const auto* __restrict__ ps = seg + pg.first;
    const int64_t t0 = (int64_t)blockIdx.x * (JOIN_WG * V * T);
    const int k = t0 < pg.len ? pg.count : 0;  // (a tile behind the programme's end is padding: no member to find)
    if (tid < k) {
        s_dst[tid] = ps[tid].dst; s_len[tid] = ps[tid].len; s_row[tid] = ps[tid].row;
        if constexpr (kTrim) { s_src[tid] = ps[tid].src; s_fade[tid] = make_int2(ps[tid].fin, ps[tid].fout); }
    }
    __syncthreads();
    auto dst_of = [&](int r) { return r < JOIN_WG ? s_dst[r] : ps[r].dst; };
    auto len_of = [&](int r) { return r < JOIN_WG ? s_len[r] : ps[r].len; };
    auto row_of = [&](int r) { return r < JOIN_WG ? s_row[r] : ps[r].row; };
    auto src_of = [&](auto r) { return r < JOIN_WG ? s_src[r] : ps[r].src; };  // (these two are generic: instantiated under kTrim only)
    auto fade_of = [&](auto r) { return r < JOIN_WG ? s_fade[r] : make_int2(ps[r].fin, ps[r].fout); };
    float v[T][V];
    // all T vectors are loaded before the first is stored: the loads of a thread are in flight together
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int64_t o = t0 + ((int64_t)i * JOIN_WG + tid) * V;  // this vector's first output sample
        if (o >= Wj) break;
        int r = 0;
        for (int hi = k; r < hi;) {  // the first member that ends behind o (the ends ascend)
            const int mid = (r + hi) >> 1;
            if (dst_of(mid) + len_of(mid) <= o) r = mid + 1; else hi = mid;
        }
        const int64_t d0 = r < k ? dst_of(r) : 0, l0 = r < k ? len_of(r) : 0;
        bool whole = r < k && o >= d0 && o + V <= d0 + l0;  // the whole vector inside one segment
        if constexpr (kTrim) {
            if (whole) {  // ... and clear of its faded edges
                const int2 f = fade_of(r);
                whole = o - d0 >= f.x && o - d0 + V <= l0 - f.y;
            }
        }
        if (whole) {
            const int64_t row = row_of(r);
            const float* __restrict__ src = x + row * src_stride + (o - d0);
            if constexpr (kTrim) src = x + row * src_stride + src_of(r) + (o - d0);
            if constexpr (V >= 4) {
#pragma unroll
                for (int j = 0; j < V / 4; ++j) {
                    const join_f4 a = reinterpret_cast<const join_f4*>(src)[j];
                    v[i][4 * j] = a.x; v[i][4 * j + 1] = a.y; v[i][4 * j + 2] = a.z; v[i][4 * j + 3] = a.w;
                }
            } else {
                v[i][0] = src[0];
            }
            if constexpr (kGain) {
                const float s = g[row];
#pragma unroll
                for (int j = 0; j < V; ++j) v[i][j] *= s;
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int64_t oj = o + j;
                while (r < k && dst_of(r) + len_of(r) <= oj) ++r;
                float t = 0.f;
                if (r < k && oj >= dst_of(r)) {
                    const int64_t row = row_of(r);
                    const int64_t q = oj - dst_of(r);  // the sample's place in its segment
                    if constexpr (kTrim) t = x[row * src_stride + src_of(r) + q];
                    else t = x[row * src_stride + q];
                    if constexpr (kGain) t *= g[row];
                    if constexpr (kTrim) {
                        const int2 f = fade_of(r);
                        const int64_t back = len_of(r) - 1 - q;
                        if (q < f.x) t *= fade[q];
                        if (back < f.y) t *= fade[back];
                    }
                }
                v[i][j] = t;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int64_t o = t0 + ((int64_t)i * JOIN_WG + tid) * V;
        if (o >= Wj) break;
        const int64_t e = (int64_t)p * dst_stride + o;
        if constexpr (kMode == DITHER_OFF) {
            if (V == 1 || o + V <= Wj) {
                enc_store_vec<V, kEnc>(y, e, v[i]);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (o + j < Wj) enc_store1<kEnc>(y, e + j, v[i][j]);
            }
        } else {
            // section 23: programme p's stream runs over [0, pg.len), gaps included; behind it the zero codeword.  The partial vector's
            // samples draw the words the whole vector would.
            const uint64_t id = dither_id(d, p);
            if (V == 1 || o + V <= Wj) {
                enc_store_vec_dither<V, kEnc, kMode>(y, e, v[i], d.seed, d.kind, id, o, pg.len);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j)
                    if (o + j < Wj) enc_store1_dither<kEnc, kMode>(y, e + j, v[i][j], d.seed, d.kind, id, o + j, pg.len);
            }
        }
    }
}
template <int V, int T, bool kGain, int kEnc>
__global__ void __launch_bounds__(JOIN_WG) join_rows_kernel(const float* __restrict__ x, int64_t src_stride, const JoinSeg* __restrict__ seg,
                                                            const JoinProg* __restrict__ prog, const float* __restrict__ g, int64_t Wj,
                                                            unsigned char* __restrict__ y, int64_t dst_stride) {
    __shared__ int64_t s_dst[JOIN_WG], s_len[JOIN_WG], s_row[JOIN_WG];
    join_walk<V, T, kGain, kEnc, false>(x, src_stride, seg, prog, g, nullptr, Wj, y, dst_stride, s_dst, s_len, s_row, nullptr, nullptr);
}
template <int V, int T, bool kGain, int kEnc>
__global__ void __launch_bounds__(JOIN_WG) join_trim_rows_kernel(const float* __restrict__ x, int64_t src_stride, const JoinSegT* __restrict__ seg,
                                                                 const JoinProg* __restrict__ prog, const float* __restrict__ g,
                                                                 const float* __restrict__ fade, int64_t Wj, unsigned char* __restrict__ y,
                                                                 int64_t dst_stride) {
    __shared__ int64_t s_dst[JOIN_WG], s_len[JOIN_WG], s_row[JOIN_WG], s_src[JOIN_WG];
    __shared__ int2 s_fade[JOIN_WG];  // (samples faded at the head, at the tail)
    join_walk<V, T, kGain, kEnc, true>(x, src_stride, seg, prog, g, fade, Wj, y, dst_stride, s_dst, s_len, s_row, s_src, s_fade);
}

template <int V, int T, bool kGain, int kEnc, int kMode>
__global__ void __launch_bounds__(JOIN_WG) join_rows_dither_kernel(const float* __restrict__ x, int64_t src_stride, const JoinSeg* __restrict__ seg,
                                                                   const JoinProg* __restrict__ prog, const float* __restrict__ g, int64_t Wj,
                                                                   unsigned char* __restrict__ y, int64_t dst_stride, DitherArgs d) {
    __shared__ int64_t s_dst[JOIN_WG], s_len[JOIN_WG], s_row[JOIN_WG];
    join_walk<V, T, kGain, kEnc, false, kMode>(x, src_stride, seg, prog, g, nullptr, Wj, y, dst_stride, s_dst, s_len, s_row, nullptr, nullptr, d);
}
template <int V, int T, bool kGain, int kEnc, int kMode>
__global__ void __launch_bounds__(JOIN_WG) join_trim_rows_dither_kernel(const float* __restrict__ x, int64_t src_stride, const JoinSegT* __restrict__ seg,
                                                                        const JoinProg* __restrict__ prog, const float* __restrict__ g,
                                                                        const float* __restrict__ fade, int64_t Wj, unsigned char* __restrict__ y,
                                                                        int64_t dst_stride, DitherArgs d) {
    __shared__ int64_t s_dst[JOIN_WG], s_len[JOIN_WG], s_row[JOIN_WG], s_src[JOIN_WG];
    __shared__ int2 s_fade[JOIN_WG];
    join_walk<V, T, kGain, kEnc, true, kMode>(x, src_stride, seg, prog, g, fade, Wj, y, dst_stride, s_dst, s_len, s_row, s_src, s_fade, d);
}

// both public launchers: Seg = JoinSeg (fade unused) or JoinSegT picks the entry point
template <typename Seg>
void launch_join(const char* who, hipStream_t s, const float* x, int64_t src_stride, const Seg* seg, const JoinProg* prog, int G, int64_t Wj,
                 const float* g, const float* fade, int enc, void* yv, int64_t dst_stride, const Dither& dth) {
    if (G <= 0 || Wj <= 0) return;
    if (G > 65535) throw std::invalid_argument(std::string(who) + ": more than 65535 programmes");
    if (dst_stride < Wj) throw std::invalid_argument(std::string(who) + ": dst_stride smaller than the joined row length");
    unsigned char* y = static_cast<unsigned char*>(yv);
    with_enc(enc, who, [&](auto e) {
        constexpr int kEnc = decltype(e)::value;
        constexpr int V = store_vec<kEnc>();
        constexpr int T = V == 16 ? 2 : 4;  // vectors per thread: a workgroup's table lookup is paid once for 32 (fp32: 16) samples a thread
        const bool vec = (G == 1 || dst_stride % V == 0) && !(reinterpret_cast<uintptr_t>(y) & 15);  // (every row's start 16-byte aligned)
        const int64_t tile = (int64_t)JOIN_WG * T * (vec ? V : 1);
        const dim3 grid((unsigned)((Wj + tile - 1) / tile), (unsigned)G);
        if constexpr (kEnc == ENC_PCM16 || kEnc == ENC_PCM24) {
            if (dithers(dth, kEnc, who, Wj)) {
                const DitherArgs d{dth.seed, dth.ids, dth.kind, dth.lim, dth.lim_stride};
                with_dither_mode(dth.mode, who, [&](auto m) {
                    constexpr int kMode = decltype(m)::value;
                    if constexpr (std::is_same_v<Seg, JoinSegT>) {
                        if (vec && g) STN_KLAUNCH((join_trim_rows_dither_kernel<V, T, true, kEnc, kMode>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, fade, Wj, y, dst_stride, d);
                        else if (vec) STN_KLAUNCH((join_trim_rows_dither_kernel<V, T, false, kEnc, kMode>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, fade, Wj, y, dst_stride, d);
                        else if (g) STN_KLAUNCH((join_trim_rows_dither_kernel<1, T, true, kEnc, kMode>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, fade, Wj, y, dst_stride, d);
                        else STN_KLAUNCH((join_trim_rows_dither_kernel<1, T, false, kEnc, kMode>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, fade, Wj, y, dst_stride, d);
                    } else {
                        if (vec && g) STN_KLAUNCH((join_rows_dither_kernel<V, T, true, kEnc, kMode>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, Wj, y, dst_stride, d);
                        else if (vec) STN_KLAUNCH((join_rows_dither_kernel<V, T, false, kEnc, kMode>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, Wj, y, dst_stride, d);
                        else if (g) STN_KLAUNCH((join_rows_dither_kernel<1, T, true, kEnc, kMode>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, Wj, y, dst_stride, d);
                        else STN_KLAUNCH((join_rows_dither_kernel<1, T, false, kEnc, kMode>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, Wj, y, dst_stride, d);
                    }
                });
                return;
            }
        }
        if constexpr (std::is_same_v<Seg, JoinSegT>) {
            if (vec && g) STN_KLAUNCH((join_trim_rows_kernel<V, T, true, kEnc>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, fade, Wj, y, dst_stride);
            else if (vec) STN_KLAUNCH((join_trim_rows_kernel<V, T, false, kEnc>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, fade, Wj, y, dst_stride);
            else if (g) STN_KLAUNCH((join_trim_rows_kernel<1, T, true, kEnc>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, fade, Wj, y, dst_stride);
            else STN_KLAUNCH((join_trim_rows_kernel<1, T, false, kEnc>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, fade, Wj, y, dst_stride);
        } else {
            if (vec && g) STN_KLAUNCH((join_rows_kernel<V, T, true, kEnc>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, Wj, y, dst_stride);
            else if (vec) STN_KLAUNCH((join_rows_kernel<V, T, false, kEnc>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, Wj, y, dst_stride);
            else if (g) STN_KLAUNCH((join_rows_kernel<1, T, true, kEnc>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, Wj, y, dst_stride);
            else STN_KLAUNCH((join_rows_kernel<1, T, false, kEnc>), grid, dim3(JOIN_WG), 0, s, x, src_stride, seg, prog, g, Wj, y, dst_stride);
        }
    });
}
void launch_join_rows(hipStream_t s, const float* x, int64_t src_stride, const JoinSeg* seg, const JoinProg* prog, int G, int64_t Wj, const float* g,
                      int enc, void* y, int64_t dst_stride, const Dither& d) {
    launch_join("join_rows", s, x, src_stride, seg, prog, G, Wj, g, nullptr, enc, y, dst_stride, d);
}
void launch_join_trim_rows(hipStream_t s, const float* x, int64_t src_stride, const JoinSegT* seg, const JoinProg* prog, int G, int64_t Wj,
                           const float* g, const float* fade, int enc, void* y, int64_t dst_stride, const Dither& d) {
    launch_join("join_trim_rows", s, x, src_stride, seg, prog, G, Wj, g, fade, enc, y, dst_stride, d);
}

}  // namespace stn
