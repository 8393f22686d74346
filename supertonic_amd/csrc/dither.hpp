// dither.hpp — the dithered PCM quantizer of a fetch (include/stn.h "dither") as one definition for the device
// (kernels_dev.hpp, kernels_output.hip) and the host (host/dither.cpp: stn_dither_noise, stn_dither_quantize): the counter-based
// Philox4x32-10 (also the latent noise's, kernels_layout.hip), the stream's counter and key, the dither value of a mode and the
// quantizer.  No HIP beyond the function attributes: the host-only library compiles it with a plain C++ compiler.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define STN_HD __host__ __device__ __forceinline__
#else
#define STN_HD inline
#endif

namespace stn {

// the values of STN_DITHER_* (include/stn.h)
enum DitherMode : int { DITHER_OFF = 0, DITHER_ROUND = 1, DITHER_TPDF = 2, DITHER_TPDF_HP = 3 };
// the streams of a fetch: a row (id: its utterance id) or a joined programme (id: its index)
enum DitherKind : unsigned { DITHER_ROW = 0, DITHER_PROG = 1 };
// a stream has at most this many samples: the block counter n >> 2 is one 32-bit word
constexpr int64_t DITHER_MAX_N = (int64_t)1 << 34;

STN_HD void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// the four words of samples 4 blk .. 4 blk + 3 of stream (kind, id) under seed: sample n's word is w[n & 3], a = w & 0xFFFF, b = w >> 16
STN_HD void dither_block(uint64_t seed, unsigned kind, uint64_t id, int64_t blk, unsigned (&w)[4]) {
    w[0] = (unsigned)blk; w[1] = (unsigned)id; w[2] = (unsigned)(id >> 32); w[3] = 0xD17E0000u | kind;
    philox4x32_10(w, (unsigned)seed, (unsigned)(seed >> 32));
}

// The dither of one sample in units of 1/65536 LSB, from its word and (TPDF_HP) its predecessor's a: TPDF a - b, two independent
// uniforms; TPDF_HP a_n - a_{n-1}, the first difference of one uniform sequence (a_{-1} := b_0): the same triangular density and
// power, its spectrum rising as 2 - 2 cos w.  ROUND: 0.
template <int kMode>
STN_HD int dither_num(unsigned w, unsigned prev_a) {
    if constexpr (kMode == DITHER_TPDF) return (int)(w & 0xFFFFu) - (int)(w >> 16);
    if constexpr (kMode == DITHER_TPDF_HP) return (int)(w & 0xFFFFu) - (int)prev_a;
    return 0;
}

// The quantizer: v clamped to [-1, 1] in fp32, scaled to S = 32767 (PCM16) or 8388607 (PCM24) and offset by 1/2 + d in double (fp32
// cannot hold vc S + d for PCM24; the product is exact in double, so a contracted multiply-add rounds as the separate pair), floor,
// clamped to [-S, S].
template <int S>
STN_HD int dither_quantize(float v, int num) {
    const float vc = fminf(1.0f, fmaxf(-1.0f, v));
    const double t = (double)vc * (double)S + 0.5 + (double)num * (1.0 / 65536.0);
    const int q = (int)floor(t);
    return q < -S ? -S : q > S ? S : q;
}

// sample n alone (the scalar forms, and the host): the dither's numerator from its block and, for TPDF_HP at n % 4 == 0, n > 0, the
// block in front of it; and its code
template <int kMode>
STN_HD int dither_num_at(uint64_t seed, unsigned kind, uint64_t id, int64_t n) {
    if constexpr (kMode != DITHER_TPDF && kMode != DITHER_TPDF_HP) {
        return 0;
    } else {
        unsigned w[4];
        dither_block(seed, kind, id, n >> 2, w);
        const int k = (int)(n & 3);
        const unsigned wk = k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3];
        unsigned prev = 0;
        if constexpr (kMode == DITHER_TPDF_HP) {
            if (k) {
                prev = (k == 1 ? w[0] : k == 2 ? w[1] : w[2]) & 0xFFFFu;
            } else if (n == 0) {
                prev = w[0] >> 16;
            } else {
                unsigned u[4];
                dither_block(seed, kind, id, (n >> 2) - 1, u);
                prev = u[3] & 0xFFFFu;
            }
        }
        return dither_num<kMode>(wk, prev);
    }
}
template <int kMode, int S>
STN_HD int dither_sample(uint64_t seed, unsigned kind, uint64_t id, int64_t n, float v) {
    return dither_quantize<S>(v, dither_num_at<kMode>(seed, kind, id, n));
}

}  // namespace stn
