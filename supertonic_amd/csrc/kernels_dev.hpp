// kernels_dev.hpp — device-side helpers shared by the MFMA kernels (kernels_gemm.hip, kernels_ffn.hip): vector types,
// buffer descriptors, LDS-DMA, counted waits, the 16-bit conversions and the GELU forms; the typed loads / stores and the wavefront sum of the
// HBM-bound kernels (kernels_dwconv_ln.hip, kernels_fold.hip, kernels_layout.hip); and the sample encodings of every fetch
// (kernels_output.hip, kernels_resample.hip), with the Philox4x32-10 and the dithered quantizer of dither.hpp.  One definition, so that a fused kernel and the launches it replaces round identically.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dither.hpp"
#include "kernels.hpp"

namespace stn {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// Out-of-range lanes get this byte offset: beyond num_records, so the buffer load returns zeros
// (hardware range check) — no divergent branch, no select-of-pointers.
static constexpr unsigned OOB = 0x80000000u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, size_t bytes) {
    const unsigned n = bytes > 0x7FFFFFFFu ? 0x7FFFFFFFu : (unsigned)bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, n, 0x00020000);
}

// fp32 -> 16-bit PCM exactly as the reference's writeWavFile (cpp/helper.cpp:986-987): clamp to [-1, 1], scale to full range, truncate
__device__ __forceinline__ int pcm16(float v) { return (int)(fminf(1.0f, fmaxf(-1.0f, v)) * 32767.0f); }
// fp32 -> 24-bit PCM by the same rule: clamp, scale to 2^23 - 1 in fp32, truncate
__device__ __forceinline__ int pcm24(float v) { return (int)(fminf(1.0f, fmaxf(-1.0f, v)) * 8388607.0f); }
// G.711 mu-law codeword of a 16-bit sample s: G.191's ulaw_compress of the 14-bit p = s >> 2 as CPython's audioop.lin2ulaw(s, 2)
// computes it (sign-magnitude |p|, magnitude clipped at 8159, bias 33; the all-ones clip codeword is reached at 8191).  Segment
// e = floor(log2(m >> 5)) for m >= 32 (0 below), mantissa the four bits under it; every bit inverted, the sign bit clear for p < 0.
// Branch-free: clz and selects.
__device__ __forceinline__ unsigned mulaw8(int s) {
    const int p = s >> 2;
    const int m = min((p < 0 ? -p : p) + 33, 8191);
    const int seg = 31 - __builtin_clz((unsigned)(m >> 5) | 1u);
    return (unsigned)((seg << 4) | ((m >> (seg + 1)) & 0xF)) ^ (p < 0 ? 0x7Fu : 0xFFu);
}
// G.711 A-law codeword of a 16-bit sample s: G.191's alaw_compress of the 13-bit p = s >> 3 as audioop.lin2alaw(s, 2) computes it
// (magnitude ~p for p < 0, segment e = floor(log2(m >> 4)) for m >= 32 (0 below), mantissa (m >> max(e, 1)) & 15, even bits inverted
// by 0x55, sign bit set for p >= 0).
__device__ __forceinline__ unsigned alaw8(int s) {
    const int p = s >> 3;
    const int m = p < 0 ? ~p : p;
    const int seg = 31 - __builtin_clz((unsigned)(m >> 4) | 1u);
    return (unsigned)((seg << 4) | ((m >> max(seg, 1)) & 0xF)) ^ (p < 0 ? 0x55u : 0xD5u);
}
// one sample v of encoding kEnc (OutEnc, kernels.hpp) stored at sample index i of y (enc_bytes(kEnc) bytes per sample)
template <int kEnc>
__device__ __forceinline__ void enc_store1(unsigned char* y, int64_t i, float v) {
    if constexpr (kEnc == ENC_F32) {
        reinterpret_cast<float*>(y)[i] = v;
    } else if constexpr (kEnc == ENC_PCM16) {
        reinterpret_cast<int16_t*>(y)[i] = (int16_t)pcm16(v);
    } else if constexpr (kEnc == ENC_PCM24) {
        const int c = pcm24(v);
        y[3 * i] = (unsigned char)c; y[3 * i + 1] = (unsigned char)(c >> 8); y[3 * i + 2] = (unsigned char)(c >> 16);
    } else if constexpr (kEnc == ENC_MULAW) {
        y[i] = (unsigned char)mulaw8(pcm16(v));
    } else {
        static_assert(kEnc == ENC_ALAW, "unknown encoding");
        y[i] = (unsigned char)alaw8(pcm16(v));
    }
}

// erf by Abramowitz-Stegun 7.1.26 (|err| <= 1.5e-7): GELU(x) = 0.5 x (1 + erf(x / sqrt2))
__device__ __forceinline__ float gelu_f(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * z);  // 1 ulp; the A&S fit itself is 1.5e-7
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    const float erf_abs = 1.0f - poly * __expf(-z * z);
    const float erf_v = x < 0.f ? -erf_abs : erf_abs;
    return 0.5f * x * (1.0f + erf_v);
}
// the tanh form of GELU, 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) = x sigmoid(2 sqrt(2/pi) x (1 + 0.044715 x^2)), in full fp32
// precision: what a graph that spells GELU with Tanh (or Gelu approximate="tanh") computes (fp32 / f16 outputs; bf16 outputs take
// gelu_bf16_f below, the same function through v_exp / v_rcp)
__device__ __forceinline__ float gelu_tanh_f(float x) {
    return x / (1.0f + expf(-1.5957691216057308f * x * (1.0f + 0.044715f * x * x)));
}
__device__ __forceinline__ float act_f(float v, int act) {
    if (act == ACT_GELU) return gelu_f(v);
    if (act == ACT_GELU_TANH) return gelu_tanh_f(v);
    if (act == ACT_SILU) return v / (1.0f + expf(-v));
    return v;
}
// GELU for results that are about to be rounded to bf16 (8 significant bits): x * sigmoid(1.59577 x (1 + 0.044715 x^2)),
// the tanh form written as a sigmoid — 5 VALU + v_exp_f32 + v_rcp_f32 instead of ~20 + 2.  |error| <= 4.8e-4 absolute
// (largest 4.73e-4, at x = -2.70; tests/test_ffn_form_cpu.py), below a bf16 ulp wherever |gelu(x)| > 0.08 and relatively tiny near 0.  fp32 outputs keep the erf form above.
__device__ __forceinline__ float gelu_bf16_f(float x) {
    const float t = x * fmaf(x * x, -0.10294324f, -2.30220819f);  // -(1.5957691 + 0.0713548 x^2) x * log2(e)
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
}
__device__ __forceinline__ float act_out_f(float v, int act, bool to_bf16) {
    if ((act == ACT_GELU || act == ACT_GELU_TANH) && to_bf16) return gelu_bf16_f(v);
    return act_f(v, act);
}
// bias + activation + row mask on an 8-column group; the activation kind is resolved ONCE per group (a per-element
// switch compiles to scalar branches around every element and triples the epilogue's issue time)
__device__ __forceinline__ void act8(float (&v)[8], const float (&bias)[8], int act, bool to_bf16, float keep) {
    if (act == ACT_NONE) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (v[j] + bias[j]) * keep;
    } else if ((act == ACT_GELU || act == ACT_GELU_TANH) && to_bf16) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = gelu_bf16_f(v[j] + bias[j]) * keep;
    } else if (act == ACT_GELU) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = gelu_f(v[j] + bias[j]) * keep;
    } else if (act == ACT_GELU_TANH) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = gelu_tanh_f(v[j] + bias[j]) * keep;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float t = v[j] + bias[j]; v[j] = t / (1.0f + expf(-t)) * keep; }
    }
}
__device__ __forceinline__ uint16_t f2bf(float f) {
    __hip_bfloat16 h = __float2bfloat16(f);
    return *reinterpret_cast<uint16_t*>(&h);
}
__device__ __forceinline__ float bf2f_(uint16_t v) { return __uint_as_float(((unsigned)v) << 16); }

// four consecutive / one element of an activation row in its storage type (float, bf16 as raw uint16_t, f16_t), to and from fp32
__device__ __forceinline__ void store4(float* p, float a, float b, float c, float d) {
    *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
__device__ __forceinline__ void store4(uint16_t* p, float a, float b, float c, float d) {
    uint2 u;
    u.x = (unsigned)f2bf(a) | ((unsigned)f2bf(b) << 16);
    u.y = (unsigned)f2bf(c) | ((unsigned)f2bf(d) << 16);
    *reinterpret_cast<uint2*>(p) = u;
}
__device__ __forceinline__ void store4(f16_t* p, float a, float b, float c, float d) {
    typedef _Float16 h4_ __attribute__((ext_vector_type(4)));
    h4_ h = {(_Float16)a, (_Float16)b, (_Float16)c, (_Float16)d};  // v_cvt_f16_f32: round to nearest even
    *reinterpret_cast<h4_*>(p) = h;
}
__device__ __forceinline__ void store1(float* p, float a) { *p = a; }
__device__ __forceinline__ void store1(uint16_t* p, float a) { *p = f2bf(a); }
__device__ __forceinline__ void store1(f16_t* p, float a) { *p = (f16_t)a; }
__device__ __forceinline__ float load1(const float* p) { return *p; }
__device__ __forceinline__ float load1(const uint16_t* p) { return bf2f_(*p); }
__device__ __forceinline__ float load1(const f16_t* p) { return (float)*p; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// 16-bit formats: bf16 (F16 = false) or IEEE half (F16 = true, the STN_DTYPE_F16 mode): same tiles, same LDS images, same
// MFMA timing (v_mfma_f32_32x32x16_f16); only the conversion and the instruction differ, both resolved at compile time.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <bool F16>
__device__ __forceinline__ uint16_t cvt16(float f) {
    if constexpr (F16) { const _Float16 h = (_Float16)f; return __builtin_bit_cast(uint16_t, h); }  // v_cvt_f16_f32, RNE
    else return f2bf(f);
}
template <bool F16>
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

#define STN_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// LDS-DMA of one 1-KiB piece (16 B per lane).  Kept in a non-template function: with value-dependent arguments
// the amdgcn builtin is re-checked at template instantiation on the HOST pass, fails there, and the failure is
// swallowed as a substitution failure (the kernel silently loses its host stub).
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, unsigned char* lds_dst, unsigned voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, STN_LDS_PTR(lds_dst), 16, voff, soff, 0, 0);
}

template <int N_>
__device__ __forceinline__ void wait_vm() {
    static_assert(N_ >= 0 && N_ < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory");
}

template <int PER, int D>  // wait until at most min(ahead, D) * PER of this wave's DMAs are outstanding
__device__ __forceinline__ void wait_stage(int ahead) {
    if constexpr (D >= 7) { if (ahead >= 7) { wait_vm<7 * PER>(); return; } }
    if constexpr (D >= 6) { if (ahead >= 6) { wait_vm<6 * PER>(); return; } }
    if constexpr (D >= 5) { if (ahead >= 5) { wait_vm<5 * PER>(); return; } }
    if constexpr (D >= 4) { if (ahead >= 4) { wait_vm<4 * PER>(); return; } }
    if constexpr (D >= 3) { if (ahead >= 3) { wait_vm<3 * PER>(); return; } }
    if constexpr (D >= 2) { if (ahead >= 2) { wait_vm<2 * PER>(); return; } }
    if constexpr (D >= 1) { if (ahead >= 1) { wait_vm<1 * PER>(); return; } }
    wait_vm<0>();
}

}  // namespace stn
