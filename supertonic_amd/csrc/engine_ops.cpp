// engine_ops.cpp — single-kernel, phase-stamp and timing entry points (stn_op_*): what the op-level tests and the tools under tools/ call.
#include "engine.hpp"
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace stn {
using detail::up;

// =================================================================================================
// op-level test entry points
// =================================================================================================
void Engine::op_gemm(int dtype, int M, int N, int K, const float* A, const float* W, const float* bias, int act, float* out) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    float* dA = up(ar_, s_, A, (size_t)M * K);
    float* dW = up(ar_, s_, W, (size_t)N * K);
    float* dB = bias ? up(ar_, s_, bias, (size_t)N) : nullptr;
    float* dO = f32_alloc((size_t)M * N);
    const void* pa = dA;
    const void* pw = dW;
    if (is_half(dtype)) {
        void* a16 = ar_.alloc((size_t)M * K * 2);
        void* w16 = ar_.alloc((size_t)N * K * 2);
        launch_cast(s_, dtype, dA, (int64_t)M * K, a16);
        launch_cast(s_, dtype, dW, (int64_t)N * K, w16);
        pa = a16; pw = w16;
    }
    Epilogue e; e.mode = EPI_STORE; e.act = act; e.out_dtype = F32; e.out = dO; e.ldo = N; e.bias = dB;
    const GemmForm f = gemm_form(dtype, M, N, K, K, K, e, pa, pw);  // the same decision the model path takes (Engine::gemm)
    launch_gemm_form(s_, f, pa, K, pw, K, M, N, K, e, f.split > 1 ? f32_alloc((int64_t)f.split * M * N) : nullptr);
    STN_HIP(hipMemcpyAsync(out, dO, (size_t)M * N * 4, hipMemcpyDeviceToHost, s_));
    sync();
}

std::string Engine::op_gemm_ex(int dtype, int M, int N, int K, const float* A, const float* W, int mode, int act, int out_dtype, int ldo,
                               const float* bias, const float* gamma, const int* len, int L, const int* row_b, const float* rowvec, int nseq,
                               int nt, int tr, float* out, int64_t out_elems) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    float* dA = up(ar_, s_, A, (size_t)M * K);
    float* dW = up(ar_, s_, W, (size_t)N * K);
    const void* pa = dA;
    const void* pw = dW;
    if (is_half(dtype)) {
        void* a16 = ar_.alloc((size_t)M * K * 2);
        void* w16 = ar_.alloc((size_t)N * K * 2);
        launch_cast(s_, dtype, dA, (int64_t)M * K, a16);
        launch_cast(s_, dtype, dW, (int64_t)N * K, w16);
        pa = a16; pw = w16;
    }
    float* dO = up(ar_, s_, out, (size_t)out_elems);
    void* o16 = nullptr;
    if (mode == EPI_STORE && out_dtype != F32) {
        o16 = ar_.alloc((size_t)out_elems * 2);
        launch_cast(s_, out_dtype, dO, out_elems, o16);
    }
    Epilogue e;
    e.mode = mode; e.act = act; e.out_dtype = mode == EPI_STORE ? out_dtype : F32; e.ldo = ldo;
    e.out = mode == EPI_RESID ? nullptr : (o16 ? o16 : static_cast<void*>(dO));
    e.resid = mode == EPI_RESID ? dO : nullptr;
    e.bias = bias ? up(ar_, s_, bias, (size_t)N) : nullptr;
    e.gamma = gamma ? up(ar_, s_, gamma, (size_t)N) : nullptr;
    e.len = len ? up(ar_, s_, len, (size_t)nseq) : nullptr;
    e.L = L;
    e.row_b = row_b ? up(ar_, s_, row_b, (size_t)M) : nullptr;
    e.rowvec = rowvec ? up(ar_, s_, rowvec, (size_t)nseq * N) : nullptr;
    e.rv_ld = N;
    e.nt = nt;
    e.tr_force = tr;
    const GemmForm f = gemm_form(dtype, M, N, K, K, K, e, pa, pw);  // the split-K decision of Engine::gemm included
    launch_gemm_form(s_, f, pa, K, pw, K, M, N, K, e, f.split > 1 ? f32_alloc((int64_t)f.split * M * N) : nullptr);
    if (o16) launch_half_to_f32(s_, out_dtype, o16, out_elems, dO);
    STN_HIP(hipMemcpyAsync(out, dO, (size_t)out_elems * 4, hipMemcpyDeviceToHost, s_));
    sync();
    return f.str();
}

std::string Engine::op_gemm_rows(int dtype, int M, int N, int K, const float* A, const float* W, const float* bias, int B, const int* rows,
                                 const int* valid, int T, float* out, int64_t out_elems) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    float* dA = up(ar_, s_, A, (size_t)M * K);
    float* dW = up(ar_, s_, W, (size_t)N * K);
    const void* pa = dA;
    const void* pw = dW;
    if (is_half(dtype)) {
        void* a16 = ar_.alloc((size_t)M * K * 2);
        void* w16 = ar_.alloc((size_t)N * K * 2);
        launch_cast(s_, dtype, dA, (int64_t)M * K, a16);
        launch_cast(s_, dtype, dW, (int64_t)N * K, w16);
        pa = a16; pw = w16;
    }
    float* dO = up(ar_, s_, out, (size_t)out_elems);
    const int* drows = up(ar_, s_, rows, (size_t)B);
    int* off = static_cast<int*>(ar_.alloc(sizeof(int) * (size_t)(B + 1)));
    launch_row_map(s_, drows, B, off, nullptr);
    Epilogue e;
    e.mode = EPI_STORE; e.out_dtype = F32; e.out = dO; e.ldo = N;
    e.bias = bias ? up(ar_, s_, bias, (size_t)N) : nullptr;
    e.map_off = off; e.map_valid = up(ar_, s_, valid, (size_t)B); e.map_B = B; e.map_T = T;
    const GemmForm f = gemm_form(dtype, M, N, K, K, K, e, pa, pw, false);
    launch_gemm_form(s_, f, pa, K, pw, K, M, N, K, e, nullptr);  // (throws for a form that cannot take the map)
    STN_HIP(hipGetLastError());
    STN_HIP(hipMemcpyAsync(out, dO, (size_t)out_elems * 4, hipMemcpyDeviceToHost, s_));
    sync();
    return f.str();
}

void Engine::op_dwconv_ln(int dtype, int B, int L, int C, int k, int dil, const float* x, const float* w, const float* bias,
                          const float* g, const float* b, float* y, const int* seqlen) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    const size_t n = (size_t)B * L * C;
    const int* dlen = seqlen ? up(ar_, s_, seqlen, (size_t)B) : nullptr;
    std::vector<float> wt((size_t)C * k);
    for (int c = 0; c < C; ++c) for (int j = 0; j < k; ++j) wt[(size_t)j * C + c] = w[(size_t)c * k + j];
    float* dx = up(ar_, s_, x, n);
    float* dw = up(ar_, s_, wt.data(), wt.size());
    float* db = up(ar_, s_, bias, (size_t)C);
    float* dg = up(ar_, s_, g, (size_t)C);
    float* dbt = up(ar_, s_, b, (size_t)C);
    void* dy = ar_.alloc(n * 4);
    float* dy32 = f32_alloc(n);
    launch_dwconv_ln(s_, dtype, dx, B, L, C, dw, db, k, dil, dg, dbt, 1e-6f, dy, dlen);
    if (is_half(dtype)) launch_half_to_f32(s_, dtype, dy, (int64_t)n, dy32);
    STN_HIP(hipMemcpyAsync(y, is_half(dtype) ? dy32 : static_cast<float*>(dy), n * 4, hipMemcpyDeviceToHost, s_));
    sync();
}

void Engine::op_attention(int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, const float* k, const float* v,
                          const int* qlen, const int* klen, int rope_mode, float* o) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    const int C = H * dh;
    const size_t nq = (size_t)B * Lq * C, nk = (size_t)B * Lk * C;
    float* dq = up(ar_, s_, q, nq);
    float* dk = up(ar_, s_, k, nk);
    float* dv = up(ar_, s_, v, nk);
    int* dql = qlen ? up(ar_, s_, qlen, (size_t)B) : nullptr;
    int* dkl = klen ? up(ar_, s_, klen, (size_t)B) : nullptr;
    const void *pq = dq, *pk = dk, *pv = dv;
    if (is_half(dtype)) {
        void* a = ar_.alloc(nq * 2); void* b = ar_.alloc(nk * 2); void* c = ar_.alloc(nk * 2);
        launch_cast(s_, dtype, dq, (int64_t)nq, a); launch_cast(s_, dtype, dk, (int64_t)nk, b); launch_cast(s_, dtype, dv, (int64_t)nk, c);
        pq = a; pk = b; pv = c;
    }
    void* dO = ar_.alloc(nq * 4);
    float* dO32 = f32_alloc(nq);
    const float rbase = a_.rope_base > 0 ? a_.rope_base : 10000.f, rgam = a_.larope_gamma > 0 ? a_.larope_gamma : 10.f;
    const bool prerot = rope_mode >= 0 && (rope_mode & 0x100) != 0;  // test hook: rotate the keys in a separate pass first
    if (prerot) rope_mode &= 0xFF;
    if (prerot) launch_rope_rows(s_, dtype, const_cast<void*>(pk), C, B, Lk, dkl, 1, 0, H, dh, rope_mode, rbase, rgam);
    launch_attention(s_, dtype, pq, C, pk, pv, C, dO, C, B, Lq, Lk, H, dh, dql, dkl, rope_mode, rbase, rgam, prerot);
    if (is_half(dtype)) launch_half_to_f32(s_, dtype, dO, (int64_t)nq, dO32);
    STN_HIP(hipMemcpyAsync(o, is_half(dtype) ? dO32 : static_cast<float*>(dO), nq * 4, hipMemcpyDeviceToHost, s_));
    sync();
}

// a host fp32 array -> device in format dtype (rounded; fp32 as it is)
static void* up_as(Arena& ar, hipStream_t s, int dtype, const float* h, size_t n) {
    float* d = up(ar, s, h, n);
    if (!is_half(dtype)) return d;
    void* d16 = ar.alloc(n * 2);
    launch_cast(s, dtype, d, (int64_t)n, d16);
    return d16;
}

std::string Engine::op_attention_ex(int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, int64_t q_elems, int ldq, int q_col,
                                    float* kv, int64_t kv_elems, int ldk, int k_col, int v_col, float* o, int64_t o_elems, int ldo,
                                    const int* qlen, const int* klen, const int* q_off, const int* k_off, int rope_mode, int k_rotated,
                                    int rot_groups, int rot_stride, int rot_col) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    const size_t esz = is_half(dtype) ? 2 : 4;
    char* dq = static_cast<char*>(up_as(ar_, s_, dtype, q, (size_t)q_elems));
    char* dkv = static_cast<char*>(up_as(ar_, s_, dtype, kv, (size_t)kv_elems));
    char* dO = static_cast<char*>(up_as(ar_, s_, dtype, o, (size_t)o_elems));
    const int* dql = qlen ? up(ar_, s_, qlen, (size_t)B) : nullptr;
    const int* dkl = klen ? up(ar_, s_, klen, (size_t)B) : nullptr;
    const int* dqo = q_off ? up(ar_, s_, q_off, (size_t)B) : nullptr;
    const int* dko = k_off ? up(ar_, s_, k_off, (size_t)B) : nullptr;
    const float rbase = a_.rope_base > 0 ? a_.rope_base : 10000.f, rgam = a_.larope_gamma > 0 ? a_.larope_gamma : 10.f;
    // as ve_text_kv_dev: every group's keys of the valid rows, once, before any attention reads them
    if (k_rotated) launch_rope_rows(s_, dtype, dkv + (size_t)rot_col * esz, ldk, B, Lk, dkl, rot_groups, rot_stride, H, dh, rope_mode, rbase, rgam, dko);
    const AttnForm f = attn_form(dtype, B, Lq, Lk, H, dh, ldq, ldk, dq + (size_t)q_col * esz, dkv + (size_t)k_col * esz, dkv + (size_t)v_col * esz);
    launch_attention(s_, dtype, dq + (size_t)q_col * esz, ldq, dkv + (size_t)k_col * esz, dkv + (size_t)v_col * esz, ldk, dO, ldo, B, Lq, Lk,
                     H, dh, dql, dkl, rope_mode, rbase, rgam, k_rotated != 0, dqo, dko);
    if (is_half(dtype)) {
        float* w = f32_alloc(std::max(kv_elems, o_elems));
        launch_half_to_f32(s_, dtype, dkv, kv_elems, w);
        STN_HIP(hipMemcpyAsync(kv, w, (size_t)kv_elems * 4, hipMemcpyDeviceToHost, s_));
        sync();
        launch_half_to_f32(s_, dtype, dO, o_elems, w);
        STN_HIP(hipMemcpyAsync(o, w, (size_t)o_elems * 4, hipMemcpyDeviceToHost, s_));
    } else {
        STN_HIP(hipMemcpyAsync(kv, dkv, (size_t)kv_elems * 4, hipMemcpyDeviceToHost, s_));
        STN_HIP(hipMemcpyAsync(o, dO, (size_t)o_elems * 4, hipMemcpyDeviceToHost, s_));
    }
    sync();
    return f.str();
}

std::string Engine::op_xattn_hs(int dtype, int M, const float* xn, const float* Wq, const float* bq, const float* Wo, const float* kv,
                                int64_t kv_elems, int ldk, int k_col, int B, int L, int Lk, const int* qlen, const int* klen, const int* k_off,
                                int rope_mode, int pairs_mode, int64_t part_stride, float* part, int64_t part_elems, int* pairs_out) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    const int C = 384, H = 4;
    const XattnHsForm f = xattn_hs_form(dtype, C, H, B, L, Lk, ldk);
    void* dx = up_as(ar_, s_, dtype, xn, (size_t)M * C);
    void* wq16 = up_as(ar_, s_, dtype, Wq, (size_t)C * C);
    void* wo16 = up_as(ar_, s_, dtype, Wo, (size_t)C * C);
    void* wqf = ar_.alloc((size_t)C * C * 2);
    void* woa = ar_.alloc((size_t)C * C * 2);
    launch_repack_frag(s_, wq16, C, C, wqf);
    launch_repack_frag_acc(s_, wo16, C, C, woa);
    const float* dbq = bq ? up(ar_, s_, bq, (size_t)C) : nullptr;
    char* dkv = static_cast<char*>(up_as(ar_, s_, dtype, kv, (size_t)kv_elems));
    void* dpart = up_as(ar_, s_, dtype, part, (size_t)part_elems);
    const int* dql = up(ar_, s_, qlen, (size_t)B);
    const int* dkl = klen ? up(ar_, s_, klen, (size_t)B) : nullptr;
    const int* dko = k_off ? up(ar_, s_, k_off, (size_t)B) : nullptr;
    int* qoff = static_cast<int*>(ar_.alloc(sizeof(int) * (size_t)(B + 1)));
    launch_row_map(s_, dql, B, qoff, nullptr);
    const int np = 2 * ((B + 1) / 2);
    int* pairs = nullptr;
    if (pairs_mode) {
        pairs = static_cast<int*>(ar_.alloc(sizeof(int) * (size_t)np));
        launch_xattn_hs_pairs(s_, dql, B, pairs);
    }
    const float rbase = a_.rope_base > 0 ? a_.rope_base : 10000.f, rgam = a_.larope_gamma > 0 ? a_.larope_gamma : 10.f;
    const char* kp = dkv + (size_t)k_col * 2;
    launch_xattn_hs(s_, dtype, dx, M, wqf, dbq, kp, kp + (size_t)C * 2, ldk, woa, dpart, part_stride, B, L, Lk, dql, dkl, qoff, dko,
                    rope_mode, rbase, rgam, nullptr, pairs);
    float* w = f32_alloc(part_elems);
    launch_half_to_f32(s_, dtype, dpart, part_elems, w);
    STN_HIP(hipMemcpyAsync(part, w, (size_t)part_elems * 4, hipMemcpyDeviceToHost, s_));
    if (pairs && pairs_out) STN_HIP(hipMemcpyAsync(pairs_out, pairs, sizeof(int) * (size_t)np, hipMemcpyDeviceToHost, s_));
    sync();
    return f.str();
}

double Engine::op_gemm_bench(int dtype, int M, int N, int K, int mode, int iters) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    const size_t esz = is_half(dtype) ? 2 : 4;
    float* tmp = f32_alloc((size_t)std::max((size_t)M * K, (size_t)N * K));
    void* A = ar_.alloc((size_t)M * K * esz);
    void* Wt = ar_.alloc((size_t)N * K * esz);
    launch_randn_masked(s_, 11, nullptr, 1, 1, (int)std::min<size_t>((size_t)M * K, 1u << 30), nullptr, tmp);
    launch_cast(s_, dtype, tmp, (int64_t)M * K, A);
    launch_randn_masked(s_, 12, nullptr, 1, 1, (int)std::min<size_t>((size_t)N * K, 1u << 30), nullptr, tmp);
    launch_scale(s_, tmp, (int)std::min<size_t>((size_t)N * K, 1u << 30), 1.0f / std::sqrt((float)K));
    launch_cast(s_, dtype, tmp, (int64_t)N * K, Wt);
    float* bias = f32_alloc(N);
    float* gamma = f32_alloc(N);
    launch_fill(s_, bias, N, 0.01f);
    launch_fill(s_, gamma, N, 0.2f);
    float* resid = f32_alloc((size_t)M * N);
    void* out = ar_.alloc((size_t)M * N * 4);
    STN_HIP(hipMemsetAsync(resid, 0, (size_t)M * N * 4, s_));
    Epilogue e;
    e.bias = bias;
    if (mode == 1) { e.mode = EPI_RESID; e.resid = resid; e.ldo = N; e.gamma = gamma; }
    else { e.mode = EPI_STORE; e.act = mode == 2 ? ACT_NONE : ACT_GELU; e.out_dtype = mode == 3 ? F32 : dtype; e.out = out; e.ldo = N; }
    for (int i = 0; i < 3; ++i) launch_gemm(s_, dtype, A, K, Wt, K, M, N, K, e);
    hipEvent_t a, b;
    STN_HIP(hipEventCreate(&a));
    STN_HIP(hipEventCreate(&b));
    STN_HIP(hipEventRecord(a, s_));
    for (int i = 0; i < iters; ++i) launch_gemm(s_, dtype, A, K, Wt, K, M, N, K, e);
    STN_HIP(hipEventRecord(b, s_));
    STN_HIP(hipEventSynchronize(b));
    float ms = 0.f;
    STN_HIP(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return (double)ms / iters;
}

void Engine::op_gemm_phases(int dtype, int M, int N, int K, int mode, double* out6) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    const size_t esz = is_half(dtype) ? 2 : 4;
    float* tmp = f32_alloc((size_t)std::max((size_t)M * K, (size_t)N * K));
    void* A = ar_.alloc((size_t)M * K * esz);
    void* Wt = ar_.alloc((size_t)N * K * esz);
    launch_randn_masked(s_, 11, nullptr, 1, 1, (int)std::min<size_t>((size_t)M * K, 1u << 30), nullptr, tmp);
    launch_cast(s_, dtype, tmp, (int64_t)M * K, A);
    launch_randn_masked(s_, 12, nullptr, 1, 1, (int)std::min<size_t>((size_t)N * K, 1u << 30), nullptr, tmp);
    launch_scale(s_, tmp, (int)std::min<size_t>((size_t)N * K, 1u << 30), 1.0f / std::sqrt((float)K));
    launch_cast(s_, dtype, tmp, (int64_t)N * K, Wt);
    float* bias = f32_alloc(N);
    float* gamma = f32_alloc(N);
    launch_fill(s_, bias, N, 0.01f);
    launch_fill(s_, gamma, N, 0.2f);
    float* resid = f32_alloc((size_t)M * N);
    void* out = ar_.alloc((size_t)M * N * 4);
    STN_HIP(hipMemsetAsync(resid, 0, (size_t)M * N * 4, s_));
    const size_t max_wg = 1 << 16;
    unsigned long long* ts = static_cast<unsigned long long*>(ar_.alloc(max_wg * 4 * 8));
    Epilogue e;
    e.bias = bias;
    if (mode == 1) { e.mode = EPI_RESID; e.resid = resid; e.ldo = N; e.gamma = gamma; }
    else { e.mode = EPI_STORE; e.act = mode == 2 ? ACT_NONE : ACT_GELU; e.out_dtype = mode == 3 ? F32 : dtype; e.out = out; e.ldo = N; }
    for (int i = 0; i < 3; ++i) launch_gemm(s_, dtype, A, K, Wt, K, M, N, K, e);
    STN_HIP(hipMemsetAsync(ts, 0, max_wg * 4 * 8, s_));
    e.ts = ts;
    launch_gemm(s_, dtype, A, K, Wt, K, M, N, K, e);
    std::vector<unsigned long long> h(max_wg * 4);
    STN_HIP(hipMemcpyAsync(h.data(), ts, max_wg * 4 * 8, hipMemcpyDeviceToHost, s_));
    sync();
    double p0 = 0, p1 = 0, p2 = 0;
    unsigned long long tmin = ~0ull, tmax_in = 0, tend = 0;
    size_t n = 0;
    for (size_t w = 0; w < max_wg; ++w) {
        const unsigned long long* t = &h[w * 4];
        if (t[3] == 0) continue;
        ++n;
        p0 += (double)(t[1] - t[0]); p1 += (double)(t[2] - t[1]); p2 += (double)(t[3] - t[2]);
        tmin = std::min(tmin, t[0]); tmax_in = std::max(tmax_in, t[0]); tend = std::max(tend, t[3]);
    }
    if (n == 0) throw std::runtime_error("op_gemm_phases: this shape does not run on the tiled kernel");
    out6[0] = p0 / n; out6[1] = p1 / n; out6[2] = p2 / n;
    out6[3] = (double)(tend - tmin); out6[4] = (double)(tmax_in - tmin); out6[5] = (double)n;
}

Engine::FfnOp Engine::op_ffn_setup(const char* op, int mode, int M, int C, int I, const float* W1, const float* W2, int split) {
    const std::string name(op);
    if (!is_half(dt_)) throw std::invalid_argument(name + ": 16-bit engines only");
    if (mode != FFN_GEMMS && !ffn_fused_supported(dt_, C, I)) throw std::invalid_argument(name + ": shape not supported by the fused kernel");
    FfnOp o;
    o.f.kind = mode;
    if (mode == FFN_K4_SPLIT && (o.f.split = split ? split : ffn_split_choose(dt_, C, I, M)) < 2)
        throw std::invalid_argument(name + ": shape not supported by the hidden-split kernel");
    if (mode == FFN_K4_SPLIT && !ffn_split_valid(dt_, C, I, o.f.split)) throw std::invalid_argument(name + ": not a split this shape runs with");
    o.f.nt = mode == FFN_GEMMS && nt_hints_ && (double)M * I * 2.0 > 128e6;  // (ffn_form's rule)
    void *w1 = act_alloc((int64_t)I * C), *w2 = act_alloc((int64_t)I * C);
    launch_cast(s_, dt_, W1, (int64_t)I * C, w1); launch_cast(s_, dt_, W2, (int64_t)I * C, w2);
    o.w1.w.bf16 = static_cast<uint16_t*>(w1); o.w1.N = I; o.w1.K = C;
    o.w2.w.bf16 = static_cast<uint16_t*>(w2); o.w2.N = C; o.w2.K = I;
    o.a.ldx = o.a.ldo = C; o.a.M = o.a.L = M; o.a.I = I;
    if (mode != FFN_GEMMS) {
        void* tmp = act_alloc((int64_t)2 * I * C);
        void* wseq = act_alloc((int64_t)2 * I * C);
        launch_ffn_pack(s_, w1, w2, C, I, tmp, wseq, o.f.split);
        o.a.wseq = wseq;
    }
    if (mode == FFN_K4_SPLIT) { o.a.part_stride = ffn_split_rows(M) * C; o.a.part = act_alloc(o.a.part_stride * o.f.split); }
    return o;
}

void Engine::op_ffn(int M, int C, int I, const float* xn, const float* W1, const float* b1, const float* W2, const float* b2, const float* gamma,
                    const float* rowvec, const int* row_b, int nseq, float* x, int mode) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    float* d_w1 = up(ar_, s_, W1, (size_t)I * C);
    float* d_w2 = up(ar_, s_, W2, (size_t)C * I);
    FfnOp op = op_ffn_setup("op_ffn", mode, M, C, I, d_w1, d_w2);
    FfnArgs& fa = op.a;
    float* d_xn = up(ar_, s_, xn, (size_t)M * C);
    void* xn16 = act_alloc((int64_t)M * C);
    launch_cast(s_, dt_, d_xn, (int64_t)M * C, xn16);
    float* d_x = up(ar_, s_, x, (size_t)M * C);
    fa.xn = xn16; fa.x = d_x; fa.b1 = up(ar_, s_, b1, (size_t)I); fa.b2 = b2 ? up(ar_, s_, b2, (size_t)C) : nullptr;
    fa.gamma = gamma ? up(ar_, s_, gamma, (size_t)C) : nullptr;
    fa.rowvec = rowvec ? up(ar_, s_, rowvec, (size_t)nseq * C) : nullptr; fa.rv_ld = C;
    fa.row_b = (rowvec && row_b) ? up(ar_, s_, row_b, (size_t)M) : nullptr;
    FoldArgs fo = ffn_launch(op.f, C, fa, op.w1, op.w2);
    if (op.f.kind == FFN_K4_SPLIT) {
        // the pending update, folded by the LayerNorm form of the fold (its normalised output is not part of this op)
        float *ones = f32_alloc(C), *zeros = f32_alloc(C);
        launch_fill(s_, ones, C, 1.f); launch_fill(s_, zeros, C, 0.f);
        if (!fo.b2) fo.b2 = zeros;
        if (!fo.gamma) fo.gamma = ones;
        void* y = act_alloc((int64_t)M * C);
        launch_fold_ln(s_, dt_, d_x, M, C, fo, ones, ones, a_.ln_eps, y);
    }
    STN_HIP(hipGetLastError());
    STN_HIP(hipMemcpyAsync(x, d_x, sizeof(float) * (size_t)M * C, hipMemcpyDeviceToHost, s_));
    sync();
}

void Engine::op_ffn_bench(int M, int C, int I, int mode, int iters, double* out5) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    for (int i = 0; i < 5; ++i) out5[i] = 0.0;
    // random operands (the clock a chip holds on zeros is not the clock it holds on data)
    float* rnd = f32_alloc((int64_t)M * C);
    launch_randn_masked(s_, 11, nullptr, 1, M, C, nullptr, rnd);
    float* wr = f32_alloc((int64_t)I * C);
    launch_randn_masked(s_, 12, nullptr, 1, I, C, nullptr, wr);
    launch_scale(s_, wr, I * C, 0.05f);
    FfnOp op = op_ffn_setup("op_ffn_bench", mode, M, C, I, wr, wr);
    void* xn16 = act_alloc((int64_t)M * C);
    launch_cast(s_, dt_, rnd, (int64_t)M * C, xn16);
    float* d_b1 = f32_alloc(I);
    float* d_b2 = f32_alloc(C);
    float* d_g = f32_alloc(C);
    launch_fill(s_, d_b1, I, 0.01f); launch_fill(s_, d_b2, C, 0.01f); launch_fill(s_, d_g, C, 0.1f);
    float* d_x = f32_alloc((int64_t)M * C);
    STN_HIP(hipMemsetAsync(d_x, 0, sizeof(float) * (size_t)M * C, s_));
    op.a.xn = xn16; op.a.b1 = d_b1; op.a.b2 = d_b2; op.a.gamma = d_g; op.a.x = d_x;
    const int S = op.f.split;
    const int nslab = (M + 127) / 128;
    const int nwg = S > 1 ? (nslab + 7) / 8 * 8 * S : nslab;
    unsigned long long* ts = static_cast<unsigned long long*>(ar_.alloc(sizeof(unsigned long long) * 4 * (size_t)nwg));
    auto run = [&](unsigned long long* stamps) { op.a.ts = stamps; ffn_launch(op.f, C, op.a, op.w1, op.w2); };
    for (int i = 0; i < 3; ++i) run(nullptr);
    hipEvent_t a, b;
    STN_HIP(hipEventCreate(&a)); STN_HIP(hipEventCreate(&b));
    STN_HIP(hipEventRecord(a, s_));
    for (int i = 0; i < iters; ++i) run(nullptr);
    STN_HIP(hipEventRecord(b, s_));
    STN_HIP(hipEventSynchronize(b));
    float ms = 0.f;
    STN_HIP(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    out5[0] = ms / iters;
    if (op.f.kind != FFN_GEMMS) {
        STN_HIP(hipMemsetAsync(ts, 0, sizeof(unsigned long long) * 4 * (size_t)nwg, s_));
        run(ts);
        std::vector<unsigned long long> h((size_t)4 * nwg);
        STN_HIP(hipMemcpyAsync(h.data(), ts, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, s_));
        sync();
        double s1 = 0, s2 = 0, s3 = 0;
        int live = 0;  // (workgroups of a hidden-split grid beyond the last slab exit at once and leave no stamps)
        for (int w = 0; w < nwg; ++w) {
            if (!h[4 * w + 3]) continue;
            ++live;
            s1 += (double)(h[4 * w + 1] - h[4 * w]); s2 += (double)(h[4 * w + 2] - h[4 * w + 1]); s3 += (double)(h[4 * w + 3] - h[4 * w + 2]);
        }
        if (live) { out5[1] = s1 / live; out5[2] = s2 / live; out5[3] = s3 / live; }
        out5[4] = live;
    }
    STN_HIP(hipGetLastError());
    sync();
}

void Engine::op_fold_dwconv_ln(int B, int C, int k, int dil, int S, const int* seqlen, const float* x, const float* part, const float* b2,
                               const float* gamma, const float* rowvec, const float* w, const float* bias, const float* g, const float* b,
                               float* x_out, float* y) {
    if (!is_half(dt_)) throw std::invalid_argument("op_fold_dwconv_ln: 16-bit engines only");
    int L = 0;
    int64_t M = 0;
    for (int i = 0; i < B; ++i) { M += seqlen[i]; L = std::max(L, seqlen[i]); }
    std::fill(x_out, x_out + M * C, 0.f);  // (the caller's buffers are results only here: nothing of what they held goes to the device)
    std::fill(y, y + M * C, 0.f);
    op_fold_dwconv_ln_ex(dt_, B, L, C, k, dil, S, 0, seqlen, x, M, part, M * C, M * C * S, b2, gamma, rowvec, C, w, bias, g, b, x_out, M, y, M);
}

void Engine::op_block_bench(int B, int L, int C, int I, int k, int dil, int mode, int iters, double* out2) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    for (int i = 0; i < 6; ++i) out2[i] = 0.0;
    const int64_t M = (int64_t)B * L;
    float* wr = f32_alloc((int64_t)I * C);
    launch_randn_masked(s_, 12, nullptr, 1, I, C, nullptr, wr);
    launch_scale(s_, wr, I * C, 0.05f);
    FfnOp op = op_ffn_setup("op_block_bench", mode, (int)M, C, I, wr, wr);
    std::vector<int> len(B, L), off(B + 1);
    for (int i = 0; i <= B; ++i) off[i] = i * L;
    const int* dlen = up(ar_, s_, len.data(), (size_t)B);
    const int* doff = up(ar_, s_, off.data(), (size_t)B + 1);
    float* xa = f32_alloc(M * C);
    float* xb = f32_alloc(M * C);
    launch_randn_masked(s_, 11, nullptr, 1, (int)M, C, nullptr, xa);
    float* d_b1 = f32_alloc(I);
    float* d_b2 = f32_alloc(C);
    float* d_g = f32_alloc(C);
    float* d_one = f32_alloc(C);
    float* dwt = f32_alloc((int64_t)k * C);
    launch_fill(s_, d_b1, I, 0.01f); launch_fill(s_, d_b2, C, 0.01f); launch_fill(s_, d_g, C, 0.01f); launch_fill(s_, d_one, C, 1.f);
    launch_fill(s_, dwt, k * C, 1.f / k);
    void* xn = act_alloc(M * C);
    op.a.xn = xn; op.a.b1 = d_b1; op.a.b2 = d_b2; op.a.gamma = d_g;
    const bool split = op.f.kind == FFN_K4_SPLIT;
    if (split) STN_HIP(hipMemsetAsync(op.a.part, 0, (size_t)op.a.part_stride * op.f.split * 2, s_));
    FoldArgs fo = ffn_pending(op.f, op.a);  // (K4-split) every block leaves the same pending update
    auto conv = [&]() {
        if (split) { launch_fold_dwconv_ln(s_, dt_, xa, xb, B, L, C, fo, dwt, d_b2, k, dil, d_one, d_b2, 1e-6f, xn, dlen, doff); std::swap(xa, xb); }
        else launch_dwconv_ln(s_, dt_, xa, B, L, C, dwt, d_b2, k, dil, d_one, d_b2, 1e-6f, xn, dlen, doff);
    };
    auto block = [&]() { conv(); op.a.x = xa; ffn_launch(op.f, C, op.a, op.w1, op.w2); };
    hipEvent_t a, b;
    STN_HIP(hipEventCreate(&a)); STN_HIP(hipEventCreate(&b));
    for (int which = 0; which < 2; ++which) {
        for (int i = 0; i < 3; ++i) { if (which) conv(); else block(); }
        STN_HIP(hipEventRecord(a, s_));
        for (int i = 0; i < iters; ++i) { if (which) conv(); else block(); }
        STN_HIP(hipEventRecord(b, s_));
        STN_HIP(hipEventSynchronize(b));
        float ms = 0.f;
        STN_HIP(hipEventElapsedTime(&ms, a, b));
        out2[which] = ms / iters;
    }
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    if (split) {  // phase stamps of one fold_dwconv_ln launch
        const int nwg = B * ((L + 7) / 8);  // (runs of 8 frames when there are few sequences, of 32 otherwise: sized for the shorter)
        unsigned long long* ts = static_cast<unsigned long long*>(ar_.alloc(sizeof(unsigned long long) * 4 * (size_t)nwg));
        STN_HIP(hipMemsetAsync(ts, 0, sizeof(unsigned long long) * 4 * (size_t)nwg, s_));
        fo.ts = ts;
        conv();
        fo.ts = nullptr;
        std::vector<unsigned long long> h((size_t)4 * nwg);
        STN_HIP(hipMemcpyAsync(h.data(), ts, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost, s_));
        sync();
        double p1 = 0, p2 = 0, p3 = 0; int live = 0;
        unsigned long long tmin = ~0ull, tmax = 0;
        for (int w = 0; w < nwg; ++w) {
            if (!h[4 * w + 3]) continue;
            ++live;
            p1 += (double)(h[4 * w + 1] - h[4 * w]); p2 += (double)(h[4 * w + 2] - h[4 * w + 1]); p3 += (double)(h[4 * w + 3] - h[4 * w + 2]);
            tmin = std::min(tmin, h[4 * w]); tmax = std::max(tmax, h[4 * w + 3]);
        }
        if (live) { out2[2] = p1 / live; out2[3] = p2 / live; out2[4] = p3 / live; out2[5] = (double)(tmax - tmin); }
    }
    STN_HIP(hipGetLastError());
    sync();
}

// the caller's whole fp32 buffer in format dtype on the device, and back (16-bit values widened, exactly)
static void down_as(Arena& ar, hipStream_t s, int dtype, const void* d, float* h, size_t n) {
    const float* src = static_cast<const float*>(d);
    if (is_half(dtype)) {
        float* w = static_cast<float*>(ar.alloc(n * 4));
        launch_half_to_f32(s, dtype, d, (int64_t)n, w);
        src = w;
    }
    STN_HIP(hipMemcpyAsync(h, src, n * 4, hipMemcpyDeviceToHost, s));
}

std::string Engine::op_ffn_ex(int M, int C, int I, const float* xn, int ldx, int64_t xn_elems, const float* W1, const float* b1, const float* W2,
                              const float* b2, const float* gamma, const int* len, int L, const int* row_b, const float* rowvec, int rv_ld, int nseq,
                              int mode, int split, float* x, int ldo, int64_t x_elems, float* part, int64_t part_stride, int64_t part_elems) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    float* d_w1 = up(ar_, s_, W1, (size_t)I * C);
    float* d_w2 = up(ar_, s_, W2, (size_t)C * I);
    FfnOp op = op_ffn_setup("op_ffn_ex", mode, M, C, I, d_w1, d_w2, split);
    FfnArgs& fa = op.a;
    fa.xn = up_as(ar_, s_, dt_, xn, (size_t)xn_elems); fa.ldx = ldx;  // as given, the columns past C of a wider row included
    float* d_x = up(ar_, s_, x, (size_t)x_elems);
    fa.x = d_x; fa.ldo = ldo;
    fa.b1 = up(ar_, s_, b1, (size_t)I);
    fa.b2 = b2 ? up(ar_, s_, b2, (size_t)C) : nullptr;
    fa.gamma = gamma ? up(ar_, s_, gamma, (size_t)C) : nullptr;
    fa.rowvec = rowvec ? up(ar_, s_, rowvec, (size_t)nseq * rv_ld) : nullptr; fa.rv_ld = rv_ld;
    fa.row_b = row_b ? up(ar_, s_, row_b, (size_t)M) : nullptr;
    fa.len = len ? up(ar_, s_, len, (size_t)nseq) : nullptr; fa.L = L;
    void* d_part = nullptr;
    if (op.f.kind == FFN_K4_SPLIT) {  // the caller's buffer takes the place of the set-up's: the partial sums are the result, no fold runs
        d_part = up_as(ar_, s_, dt_, part, (size_t)part_elems);
        fa.part = d_part; fa.part_stride = part_stride;
    }
    ffn_launch(op.f, C, fa, op.w1, op.w2);
    STN_HIP(hipGetLastError());
    STN_HIP(hipMemcpyAsync(x, d_x, sizeof(float) * (size_t)x_elems, hipMemcpyDeviceToHost, s_));
    if (d_part) down_as(ar_, s_, dt_, d_part, part, (size_t)part_elems);
    sync();
    return op.f.str();
}

std::string Engine::op_dwconv_ln_ex(int dtype, int B, int L, int C, int k, int dil, const float* x, int64_t x_rows, const float* w,
                                    const float* bias, const float* g, const float* b, const int* seqlen, int packed, int ln_only, float* y,
                                    int64_t y_rows, const float* tail, int T, int rf) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    const int* dlen = seqlen ? up(ar_, s_, seqlen, (size_t)B) : nullptr;
    float* dx = up(ar_, s_, x, (size_t)x_rows * C);  // as given, padding rows included
    float* dg = up(ar_, s_, g, (size_t)C);
    float* dbt = up(ar_, s_, b, (size_t)C);
    void* dy = up_as(ar_, s_, dtype, y, (size_t)y_rows * C);
    std::string form = "layernorm";
    if (ln_only) {
        launch_layernorm(s_, dtype, dx, (int64_t)B * L, C, dg, dbt, 1e-6f, dy);
    } else {
        std::vector<float> wt((size_t)C * k);
        for (int c = 0; c < C; ++c) for (int j = 0; j < k; ++j) wt[(size_t)j * C + c] = w[(size_t)c * k + j];
        float* dw = up(ar_, s_, wt.data(), wt.size());
        float* db = up(ar_, s_, bias, (size_t)C);
        int* off = nullptr;
        if (packed) {
            off = static_cast<int*>(ar_.alloc(sizeof(int) * (size_t)(B + 1)));
            launch_row_map(s_, dlen, B, off, nullptr);
        }
        DwconvTail tl;
        if (tail) { tl.tail = up(ar_, s_, tail, (size_t)(rf + 1) * C); tl.T = T; tl.rf = rf; }
        form = dwconv_ln_form(dtype, B, L, C, k, packed != 0).str();  // the decision launch_dwconv_ln takes
        launch_dwconv_ln(s_, dtype, dx, B, L, C, dw, db, k, dil, dg, dbt, 1e-6f, dy, dlen, off, tl);
    }
    STN_HIP(hipGetLastError());
    down_as(ar_, s_, dtype, dy, y, (size_t)y_rows * C);
    sync();
    return form;
}

void Engine::op_fold_ln(int dtype, int M, int C, int S, const float* part, const float* b2, const float* gamma, const float* rowvec,
                        const int* row_b, int nseq, const float* g, const float* b, float* x, float* y) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    const size_t n = (size_t)M * C;
    FoldArgs fo;
    fo.part = up_as(ar_, s_, dtype, part, n * S); fo.S = S; fo.part_stride = (int64_t)n;
    fo.b2 = up(ar_, s_, b2, (size_t)C); fo.gamma = up(ar_, s_, gamma, (size_t)C);
    fo.rowvec = rowvec ? up(ar_, s_, rowvec, (size_t)nseq * C) : nullptr; fo.rv_ld = C;
    fo.row_b = (rowvec && row_b) ? up(ar_, s_, row_b, (size_t)M) : nullptr;
    float* dx = up(ar_, s_, x, n);
    float* dg = up(ar_, s_, g, (size_t)C);
    float* dbt = up(ar_, s_, b, (size_t)C);
    void* dy = ar_.alloc(n * 2);
    launch_fold_ln(s_, dtype, dx, M, C, fo, dg, dbt, 1e-6f, dy);
    STN_HIP(hipGetLastError());
    STN_HIP(hipMemcpyAsync(x, dx, n * 4, hipMemcpyDeviceToHost, s_));
    down_as(ar_, s_, dtype, dy, y, n);
    sync();
}

std::string Engine::op_fold_dwconv_ln_ex(int dtype, int B, int L, int C, int k, int dil, int S, int run_frames, const int* seqlen, const float* x_in,
                                         int64_t x_rows, const float* part, int64_t part_stride, int64_t part_elems, const float* b2, const float* gamma,
                                         const float* rowvec, int rv_ld, const float* w, const float* bias, const float* g, const float* b, float* x_out,
                                         int64_t x_out_rows, float* y, int64_t y_rows) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    std::vector<float> wt((size_t)C * k);
    for (int c = 0; c < C; ++c) for (int j = 0; j < k; ++j) wt[(size_t)j * C + c] = w[(size_t)c * k + j];
    const int* dlen = up(ar_, s_, seqlen, (size_t)B);
    int* doff = static_cast<int*>(ar_.alloc(sizeof(int) * (size_t)(B + 1)));
    launch_row_map(s_, dlen, B, doff, nullptr);
    float* dx = up(ar_, s_, x_in, (size_t)x_rows * C);  // as given, the rows behind the last sequence included
    float* dxo = up(ar_, s_, x_out, (size_t)x_out_rows * C);
    void* dy = up_as(ar_, s_, dtype, y, (size_t)y_rows * C);
    float* dw = up(ar_, s_, wt.data(), wt.size());
    float* db = up(ar_, s_, bias, (size_t)C);
    float* dg = up(ar_, s_, g, (size_t)C);
    float* dbt = up(ar_, s_, b, (size_t)C);
    FoldArgs fo;
    fo.part = up_as(ar_, s_, dtype, part, (size_t)part_elems); fo.S = S; fo.part_stride = part_stride;
    if (b2) fo.b2 = up(ar_, s_, b2, (size_t)C);
    else { float* z = f32_alloc(C); launch_fill(s_, z, C, 0.f); fo.b2 = z; }
    if (gamma) fo.gamma = up(ar_, s_, gamma, (size_t)C);
    else { float* o = f32_alloc(C); launch_fill(s_, o, C, 1.f); fo.gamma = o; }
    fo.rowvec = rowvec ? up(ar_, s_, rowvec, (size_t)B * rv_ld) : nullptr; fo.rv_ld = rowvec ? rv_ld : C;
    fo.run_frames = run_frames;
    const std::string form = fold_dwconv_ln_form(dtype, B, L, C, k, dil, S, rowvec != nullptr, run_frames).str();  // the decision launch_fold_dwconv_ln takes
    launch_fold_dwconv_ln(s_, dtype, dx, dxo, B, L, C, fo, dw, db, k, dil, dg, dbt, 1e-6f, dy, dlen, doff);
    STN_HIP(hipGetLastError());
    STN_HIP(hipMemcpyAsync(x_out, dxo, sizeof(float) * (size_t)x_out_rows * C, hipMemcpyDeviceToHost, s_));
    down_as(ar_, s_, dtype, dy, y, (size_t)y_rows * C);
    sync();
    return form;
}

// One layout kernel of kernels_layout.hip on host operands (stn_op_layout).  Every destination is the caller's whole buffer: uploaded as given,
// downloaded whole.  Every extent a kernel addresses is checked against the buffers here, before anything is launched.
void Engine::op_layout(int which, int dtype, const int* p, const float* a, int64_t a_n, const float* b, int64_t b_n, const float* c, int64_t c_n,
                       const int64_t* ids, int64_t ids_n, const int* len, int packed, float* out, int64_t out_n, float* out2, int64_t out2_n,
                       int* iout, int64_t iout_n) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    auto need = [](bool ok, const char* what) { if (!ok) throw std::invalid_argument(std::string("stn_op_layout: ") + what); };
    // rows a destination / source of `rows_per_seq` rows per sequence must hold: the padded B * rows_per_seq, or the packed sum of lengths
    auto rows_needed = [&](int B, int rows_per_seq) -> int64_t {
        if (!packed) return (int64_t)B * rows_per_seq;
        int64_t t = 0;
        for (int i = 0; i < B; ++i) t += len[i];
        return t;
    };
    auto check_len = [&](int B, int hi, bool required) {
        need(B > 0 && B <= 1024, "1 <= B <= 1024");
        need(len || !(required || packed), "lengths needed");
        if (len) for (int i = 0; i < B; ++i) need(len[i] >= 0 && len[i] <= hi, "a length outside [0, rows per sequence]");
    };
    auto row_off = [&](const int* dlen, int B) -> int* {
        if (!packed) return nullptr;
        int* off = static_cast<int*>(ar_.alloc(sizeof(int) * (size_t)(B + 1)));
        launch_row_map(s_, dlen, B, off, nullptr);
        return off;
    };
    switch (which) {
    case 0: {  // row_map: p = {B, rows_padded, with_row_b}; iout = row_off [B + 1] then row_b
        const int B = p[0], rows_padded = p[1], with_b = p[2];
        need(B > 0 && len && iout && rows_padded >= 0, "row_map: B > 0, lengths and iout needed");
        if (B > 1024) { launch_row_map(s_, nullptr, B, nullptr, nullptr); return; }  // (the launcher's refusal)
        int64_t tot = 0;
        for (int i = 0; i < B; ++i) { need(len[i] >= 0 && len[i] < (1 << 20), "row_map: length out of range"); tot += len[i]; }
        need(iout_n >= B + 1 + (with_b ? std::max<int64_t>(tot, rows_padded) : 0), "row_map: iout too small");
        const int* dlen = up(ar_, s_, len, (size_t)B);
        int* d = up(ar_, s_, iout, (size_t)iout_n);
        launch_row_map(s_, dlen, B, d, with_b ? d + B + 1 : nullptr, rows_padded);
        STN_HIP(hipMemcpyAsync(iout, d, (size_t)iout_n * 4, hipMemcpyDeviceToHost, s_));
        break;
    }
    case 1: {  // ncl_to_rows: p = {B, C, L, ld_out}; a [B][C][L]; out rows of ld_out in dtype
        const int B = p[0], C = p[1], L = p[2], ldo = p[3];
        need(C > 0 && L > 0 && ldo >= C && a && out, "ncl_to_rows: bad shape");
        check_len(B, L, false);
        need(a_n >= (int64_t)B * C * L && out_n >= rows_needed(B, L) * ldo, "ncl_to_rows: buffer too small");
        const int* dlen = len ? up(ar_, s_, len, (size_t)B) : nullptr;
        float* da = up(ar_, s_, a, (size_t)a_n);
        void* d = up_as(ar_, s_, dtype, out, (size_t)out_n);
        launch_ncl_to_rows(s_, dtype, da, B, C, L, d, ldo, dlen, row_off(dlen, B));
        down_as(ar_, s_, dtype, d, out, (size_t)out_n);
        break;
    }
    case 2: {  // euler_ncl: p = {B, D, L, with_z, ldz}; a = prev [B][D][L], b = v rows of D, c = dt [B]; out [B][D][L] fp32; out2 = z rows of ldz in dtype
        const int B = p[0], D = p[1], L = p[2], with_z = p[3], ldz = p[4];
        need(D > 0 && L > 0 && a && b && c && out && (!with_z || (out2 && ldz >= D)), "euler_ncl: bad shape");
        check_len(B, L, false);
        const int64_t vr = rows_needed(B, L);
        need(a_n >= (int64_t)B * D * L && out_n >= (int64_t)B * D * L && c_n >= B && b_n >= vr * D && (!with_z || out2_n >= vr * ldz), "euler_ncl: buffer too small");
        const int* dlen = len ? up(ar_, s_, len, (size_t)B) : nullptr;
        float* dp = up(ar_, s_, a, (size_t)a_n);
        float* dv = up(ar_, s_, b, (size_t)b_n);
        float* ddt = up(ar_, s_, c, (size_t)c_n);
        float* d = up(ar_, s_, out, (size_t)out_n);
        void* dz = with_z ? up_as(ar_, s_, dtype, out2, (size_t)out2_n) : nullptr;
        launch_euler_ncl(s_, dp, dv, ddt, dlen, B, D, L, d, row_off(dlen, B), dz, dtype, ldz);
        STN_HIP(hipMemcpyAsync(out, d, (size_t)out_n * 4, hipMemcpyDeviceToHost, s_));
        if (dz) down_as(ar_, s_, dtype, dz, out2, (size_t)out2_n);
        break;
    }
    case 3: {  // unpack_rows: p = {B, T, W}; a = packed rows [sum len][W]; out [B][T][W] fp32
        const int B = p[0], T = p[1], W = p[2];
        need(T > 0 && W > 0 && W % 4 == 0 && a && out, "unpack_rows: bad shape");
        packed = 1;
        check_len(B, T, true);
        need(a_n >= rows_needed(B, T) * W && a_n > 0 && out_n >= (int64_t)B * T * W, "unpack_rows: buffer too small");
        const int* dlen = up(ar_, s_, len, (size_t)B);
        float* da = up(ar_, s_, a, (size_t)a_n);
        float* d = up(ar_, s_, out, (size_t)out_n);
        launch_unpack_rows(s_, da, dlen, row_off(dlen, B), B, T, W, d);
        STN_HIP(hipMemcpyAsync(out, d, (size_t)out_n * 4, hipMemcpyDeviceToHost, s_));
        break;
    }
    case 4: {  // embed: p = {vocab, B, L, C}; ids [B][L]; a = table [vocab][C]; out rows of C fp32
        const int vocab = p[0], B = p[1], L = p[2], C = p[3];
        need(vocab > 0 && L > 0 && C > 0 && C % 4 == 0 && ids && a && out, "embed: bad shape");
        check_len(B, L, true);
        need(ids_n >= (int64_t)B * L && a_n >= (int64_t)vocab * C && out_n >= rows_needed(B, L) * C, "embed: buffer too small");
        const int* dlen = up(ar_, s_, len, (size_t)B);
        int64_t* di = up(ar_, s_, ids, (size_t)ids_n);
        float* da = up(ar_, s_, a, (size_t)a_n);
        float* d = up(ar_, s_, out, (size_t)out_n);
        launch_embed(s_, di, da, vocab, B, L, C, dlen, d, row_off(dlen, B));
        STN_HIP(hipMemcpyAsync(out, d, (size_t)out_n * 4, hipMemcpyDeviceToHost, s_));
        break;
    }
    case 5: {  // masked_mean: p = {B, L, C}; a = rows of C (rounded to dtype); out [B][C] fp32
        const int B = p[0], L = p[1], C = p[2];
        need(L > 0 && C > 0 && a && out, "masked_mean: bad shape");
        check_len(B, L, true);
        need(a_n >= rows_needed(B, L) * C && a_n > 0 && out_n >= (int64_t)B * C, "masked_mean: buffer too small");
        const int* dlen = up(ar_, s_, len, (size_t)B);
        void* da = up_as(ar_, s_, dtype, a, (size_t)a_n);
        float* d = up(ar_, s_, out, (size_t)out_n);
        launch_masked_mean(s_, dtype, da, B, L, C, dlen, d, row_off(dlen, B));
        STN_HIP(hipMemcpyAsync(out, d, (size_t)out_n * 4, hipMemcpyDeviceToHost, s_));
        break;
    }
    case 6: {  // vocoder_im2col: p = {B, L, ld, ccf, k, kp}; a = latent [B][ld*ccf][L]; len = valid vocoder frames; out rows of kp in dtype
        const int B = p[0], L = p[1], ld = p[2], ccf = p[3], k = p[4], kp = p[5];
        need(L > 0 && ld > 0 && ccf > 0 && k > 0 && (k & 1) && kp > 0 && a && out, "vocoder_im2col: bad shape");
        check_len(B, L * ccf, false);
        need(a_n >= (int64_t)B * ld * ccf * L && out_n >= rows_needed(B, L * ccf) * kp, "vocoder_im2col: buffer too small");
        const int* dlen = len ? up(ar_, s_, len, (size_t)B) : nullptr;
        float* da = up(ar_, s_, a, (size_t)a_n);
        void* d = up_as(ar_, s_, dtype, out, (size_t)out_n);
        launch_vocoder_im2col(s_, dtype, da, B, L, ld, ccf, k, kp, d, dlen, row_off(dlen, B));
        down_as(ar_, s_, dtype, d, out, (size_t)out_n);
        break;
    }
    case 7: {  // vocoder_in: p = {B, L, ld, ccf, C, k}; a = latent, b = weights [ld*k][C], c = bias [C]; len = valid vocoder frames; out [B*T][C] fp32
        const int B = p[0], L = p[1], ld = p[2], ccf = p[3], C = p[4], k = p[5];
        need(L > 0 && ld > 0 && ccf > 0 && C > 0 && k > 0 && (k & 1) && (int64_t)(8 + k - 1) * ld * 4 <= 64 * 1024 && a && b && c && out, "vocoder_in: bad shape");
        need(!packed, "vocoder_in: padded rows only");
        check_len(B, L * ccf, false);
        need(a_n >= (int64_t)B * ld * ccf * L && b_n >= (int64_t)ld * k * C && c_n >= C && out_n >= (int64_t)B * L * ccf * C, "vocoder_in: buffer too small");
        const int* dlen = len ? up(ar_, s_, len, (size_t)B) : nullptr;
        float* da = up(ar_, s_, a, (size_t)a_n);
        float* dw = up(ar_, s_, b, (size_t)b_n);
        float* db = up(ar_, s_, c, (size_t)c_n);
        float* d = up(ar_, s_, out, (size_t)out_n);
        launch_vocoder_in(s_, da, B, L, ld, ccf, dw, db, C, k, d, dlen);
        STN_HIP(hipMemcpyAsync(out, d, (size_t)out_n * 4, hipMemcpyDeviceToHost, s_));
        break;
    }
    case 8: {  // fill_rows: p = {B, T, W, rf, zeros}; len = valid [B]; a = quiet [W], b = edge [rf][W] (unused with zeros); out [B][T][W] fp32
        const int B = p[0], T = p[1], W = p[2], rf = p[3], zeros = p[4];
        need(T > 0 && W > 0 && W % 4 == 0 && rf >= 0 && rf <= T && out, "fill_rows: bad shape");
        check_len(B, T, true);
        need(out_n >= (int64_t)B * T * W, "fill_rows: buffer too small");
        need(zeros || (a && a_n >= W && (rf == 0 || (b && b_n >= (int64_t)rf * W))), "fill_rows: the quiet rule needs quiet [W] and edge [rf][W]");
        const int* dlen = up(ar_, s_, len, (size_t)B);
        const float* dq = zeros ? nullptr : up(ar_, s_, a, (size_t)a_n);
        const float* de = (zeros || rf == 0) ? nullptr : up(ar_, s_, b, (size_t)b_n);
        float* d = up(ar_, s_, out, (size_t)out_n);
        launch_fill_rows(s_, dlen, B, T, W, rf, dq, de, d);
        STN_HIP(hipMemcpyAsync(out, d, (size_t)out_n * 4, hipMemcpyDeviceToHost, s_));
        break;
    }
    case 9: {  // hs_pairs: p = {B}; len [B]; iout: the pairing, 2 * ceil(B / 2) words
        const int B = p[0];
        check_len(B, 1 << 20, true);
        need(iout && iout_n >= 2 * ((B + 1) / 2), "hs_pairs: iout too small");
        const int* dlen = up(ar_, s_, len, (size_t)B);
        int* d = up(ar_, s_, iout, (size_t)iout_n);
        launch_xattn_hs_pairs(s_, dlen, B, d);
        STN_HIP(hipMemcpyAsync(iout, d, (size_t)iout_n * 4, hipMemcpyDeviceToHost, s_));
        break;
    }
    case 10: {  // trim_len: p = {B, ccf, T, rf, tail_form}; len [B] latent lengths; iout = n [B] then valid [B]
        const int B = p[0], ccf = p[1], T = p[2], rf = p[3], tail_form = p[4];
        need(ccf > 0 && T > 0 && rf >= 0, "trim_len: bad shape");
        check_len(B, T / ccf, true);
        need(iout && iout_n >= 2 * (int64_t)B, "trim_len: iout too small");
        const int* dlen = up(ar_, s_, len, (size_t)B);
        int* d = up(ar_, s_, iout, (size_t)iout_n);
        launch_trim_len(s_, dlen, B, ccf, T, rf, d, d + B, tail_form != 0);
        STN_HIP(hipMemcpyAsync(iout, d, (size_t)iout_n * 4, hipMemcpyDeviceToHost, s_));
        break;
    }
    default: need(false, "unknown kernel");
    }
    STN_HIP(hipGetLastError());
    sync();
}

void Engine::op_randn(uint64_t seed, int B, int D, int L, const int64_t* utt_ids, const int* len, float* out) {
    STN_HIP(hipSetDevice(device_));
    ar_.reset();
    int64_t* du = utt_ids ? up(ar_, s_, utt_ids, (size_t)B) : nullptr;
    int* dl = len ? up(ar_, s_, len, (size_t)B) : nullptr;
    float* d = f32_alloc((size_t)B * D * L);
    launch_randn_masked(s_, seed, du, B, D, L, dl, d);
    STN_HIP(hipMemcpyAsync(out, d, (size_t)B * D * L * 4, hipMemcpyDeviceToHost, s_));
    sync();
}

}  // namespace stn
