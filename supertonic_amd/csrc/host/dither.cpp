// dither.cpp — the dithered quantizer on the CPU (include/stn.h "dither"): stn_dither_noise and stn_dither_quantize over dither.hpp, the
// definition the store kernels compile.  Host only: no device, no handle.
#include "../dither.hpp"

#include "../../../include/stn.h"

namespace {

bool bad_stream(int mode, int kind, int64_t n0, int64_t n) {
    return mode < STN_DITHER_OFF || mode > STN_DITHER_TPDF_HP || (kind != STN_DITHER_ROW && kind != STN_DITHER_PROG) || n0 < 0 || n < 0 ||
           n0 > stn::DITHER_MAX_N || n > stn::DITHER_MAX_N - n0;
}

template <int S>
int code(int mode, float v, uint64_t seed, unsigned kind, uint64_t id, int64_t n) {
    switch (mode) {
        case STN_DITHER_ROUND: return stn::dither_sample<stn::DITHER_ROUND, S>(seed, kind, id, n, v);
        case STN_DITHER_TPDF: return stn::dither_sample<stn::DITHER_TPDF, S>(seed, kind, id, n, v);
        case STN_DITHER_TPDF_HP: return stn::dither_sample<stn::DITHER_TPDF_HP, S>(seed, kind, id, n, v);
        default: return (int)(fminf(1.0f, fmaxf(-1.0f, v)) * (float)S);  // the truncating store (pcm16 / pcm24 of kernels_dev.hpp)
    }
}

}  // namespace

extern "C" {

int stn_dither_noise(int mode, uint64_t seed, int kind, uint64_t id, int64_t n0, int64_t n, float* d) {
    if (bad_stream(mode, kind, n0, n) || (!d && n)) return STN_ERR_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        const int num = mode == STN_DITHER_TPDF      ? stn::dither_num_at<stn::DITHER_TPDF>(seed, (unsigned)kind, id, n0 + i)
                        : mode == STN_DITHER_TPDF_HP ? stn::dither_num_at<stn::DITHER_TPDF_HP>(seed, (unsigned)kind, id, n0 + i)
                                                     : 0;
        d[i] = (float)num * (1.0f / 65536.0f);
    }
    return STN_OK;
}

int stn_dither_quantize(int enc, int mode, uint64_t seed, int kind, uint64_t id, int64_t n0, int64_t n, const float* v, void* out) {
    if (bad_stream(mode, kind, n0, n) || (enc != STN_ENC_PCM16 && enc != STN_ENC_PCM24) || ((!v || !out) && n)) return STN_ERR_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        if (enc == STN_ENC_PCM16) {
            static_cast<int16_t*>(out)[i] = (int16_t)code<32767>(mode, v[i], seed, (unsigned)kind, id, n0 + i);
        } else {
            const int c = code<8388607>(mode, v[i], seed, (unsigned)kind, id, n0 + i);
            unsigned char* o = static_cast<unsigned char*>(out) + 3 * i;
            o[0] = (unsigned char)c; o[1] = (unsigned char)(c >> 8); o[2] = (unsigned char)(c >> 16);
        }
    }
    return STN_OK;
}

}  // extern "C"
