// engine_ops.cpp — single-kernel, phase-stamp and timing entry points (stn_op_*): what the op-level tests and the tools under tools/ call.
#include "engine_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace stn {

// a host fp32 array -> device in format dtype (rounded; fp32 as it is)
static void* up_as(OpScope& op, hipStream_t s, int dtype, const float* h, size_t n) {
    float* d = op.up(h, n);
    if (!is_half(dtype)) return d;
    void* d16 = op.buf<char>(n * 2);
    launch_cast(s, dtype, d, (int64_t)n, d16);
    return d16;
}
// and back into the caller's fp32 buffer (16-bit values widened, exactly)
static void down_as(OpScope& op, hipStream_t s, int dtype, const void* d, float* h, size_t n) {
    const float* src = static_cast<const float*>(d);
    if (is_half(dtype)) {
        float* w = op.buf<float>(n);
        launch_half_to_f32(s, dtype, d, (int64_t)n, w);
        src = w;
    }
    op.down(h, src, n);
}
// depthwise weights [C][k] as the kernels take them, [k][C]
static std::vector<float> dw_transposed(const float* w, int C, int k) {
    std::vector<float> wt((size_t)C * k);
    for (int c = 0; c < C; ++c) for (int j = 0; j < k; ++j) wt[(size_t)j * C + c] = w[(size_t)c * k + j];
    return wt;
}
// avg ms of fn() on stream s over `iters` runs between two events, behind three warm-up runs; the events go on every path
template <class Fn>
static double time_ms(hipStream_t s, int iters, Fn fn) {
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    for (int i = 0; i < 3; ++i) fn();
    STN_HIP(hipEventCreate(&ev.a));
    STN_HIP(hipEventCreate(&ev.b));
    STN_HIP(hipEventRecord(ev.a, s));
    for (int i = 0; i < iters; ++i) fn();
    STN_HIP(hipEventRecord(ev.b, s));
    STN_HIP(hipEventSynchronize(ev.b));
    float ms = 0.f;
    STN_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
    return (double)ms / iters;
}
// per-workgroup phase stamps t[0..3] (a workgroup that left none has t[3] == 0): the three phase means over the live workgroups, their
// count, and the earliest entry, the latest entry and the latest end
struct Stamps { double p[3] = {0, 0, 0}; size_t live = 0; unsigned long long tmin = ~0ull, tmax_in = 0, tend = 0; };
static Stamps reduce_stamps(const std::vector<unsigned long long>& h) {
    Stamps r;
    for (size_t w = 0; w + 4 <= h.size(); w += 4) {
        const unsigned long long* t = &h[w];
        if (t[3] == 0) continue;
        ++r.live;
        for (int i = 0; i < 3; ++i) r.p[i] += (double)(t[i + 1] - t[i]);
        r.tmin = std::min(r.tmin, t[0]); r.tmax_in = std::max(r.tmax_in, t[0]); r.tend = std::max(r.tend, t[3]);
    }
    for (double& v : r.p) if (r.live) v /= (double)r.live;
    return r;
}

// =================================================================================================
// op-level test entry points
// =================================================================================================
void Engine::op_gemm(int dtype, int M, int N, int K, const float* A, const float* W, const float* bias, int act, float* out) {
    OpScope op(*this);
    const void* pa = up_as(op, s_, dtype, A, (size_t)M * K);
    const void* pw = up_as(op, s_, dtype, W, (size_t)N * K);
    const float* dB = op.up(bias, (size_t)N);
    float* dO = op.buf<float>((size_t)M * N);
    Epilogue e; e.mode = EPI_STORE; e.act = act; e.out_dtype = F32; e.out = dO; e.ldo = N; e.bias = dB;
    const GemmForm f = gemm_form(dtype, M, N, K, K, K, e, pa, pw);  // the same decision the model path takes (Engine::gemm)
    launch_gemm_form(s_, f, pa, K, pw, K, M, N, K, e, f.split > 1 ? op.buf<float>((size_t)f.split * M * N) : nullptr);
    op.down(out, dO, (size_t)M * N);
    sync();
}

std::string Engine::op_gemm_ex(int dtype, int M, int N, int K, const float* A, const float* W, int mode, int act, int out_dtype, int ldo,
                               const float* bias, const float* gamma, const int* len, int L, const int* row_b, const float* rowvec, int nseq,
                               int nt, int tr, float* out, int64_t out_elems) {
    OpScope op(*this);
    const void* pa = up_as(op, s_, dtype, A, (size_t)M * K);
    const void* pw = up_as(op, s_, dtype, W, (size_t)N * K);
    const bool o_half = mode == EPI_STORE && out_dtype != F32;
    void* dO = up_as(op, s_, o_half ? out_dtype : F32, out, (size_t)out_elems);
    Epilogue e;
    e.mode = mode; e.act = act; e.out_dtype = mode == EPI_STORE ? out_dtype : F32; e.ldo = ldo;
    e.out = mode == EPI_RESID ? nullptr : dO;
    e.resid = mode == EPI_RESID ? static_cast<float*>(dO) : nullptr;
    e.bias = op.up(bias, (size_t)N);
    e.gamma = op.up(gamma, (size_t)N);
    e.len = op.up(len, (size_t)nseq);
    e.L = L;
    e.row_b = op.up(row_b, (size_t)M);
    e.rowvec = op.up(rowvec, (size_t)nseq * N);
    e.rv_ld = N;
    e.nt = nt;
    e.tr_force = tr;
    const GemmForm f = gemm_form(dtype, M, N, K, K, K, e, pa, pw);  // the split-K decision of Engine::gemm included
    launch_gemm_form(s_, f, pa, K, pw, K, M, N, K, e, f.split > 1 ? op.buf<float>((size_t)f.split * M * N) : nullptr);
    down_as(op, s_, o_half ? out_dtype : F32, dO, out, (size_t)out_elems);
    sync();
    return f.str();
}

std::string Engine::op_gemm_rows(int dtype, int M, int N, int K, const float* A, const float* W, const float* bias, int B, const int* rows,
                                 const int* valid, int T, float* out, int64_t out_elems) {
    OpScope op(*this);
    const void* pa = up_as(op, s_, dtype, A, (size_t)M * K);
    const void* pw = up_as(op, s_, dtype, W, (size_t)N * K);
    float* dO = op.up(out, (size_t)out_elems);
    const int* drows = op.up(rows, (size_t)B);
    int* off = op.buf<int>((size_t)B + 1);
    launch_row_map(s_, drows, B, off, nullptr);
    Epilogue e;
    e.mode = EPI_STORE; e.out_dtype = F32; e.out = dO; e.ldo = N;
    e.bias = op.up(bias, (size_t)N);
    e.map_off = off; e.map_valid = op.up(valid, (size_t)B); e.map_B = B; e.map_T = T;
    const GemmForm f = gemm_form(dtype, M, N, K, K, K, e, pa, pw, false);
    launch_gemm_form(s_, f, pa, K, pw, K, M, N, K, e, nullptr);  // (throws for a form that cannot take the map)
    STN_HIP(hipGetLastError());
    op.down(out, dO, (size_t)out_elems);
    sync();
    return f.str();
}

void Engine::op_dwconv_ln(int dtype, int B, int L, int C, int k, int dil, const float* x, const float* w, const float* bias,
                          const float* g, const float* b, float* y, const int* seqlen) {
    OpScope op(*this);
    const size_t n = (size_t)B * L * C;
    const int* dlen = op.up(seqlen, (size_t)B);
    const std::vector<float> wt = dw_transposed(w, C, k);
    float* dx = op.up(x, n);
    float* dw = op.up(wt);
    float* db = op.up(bias, (size_t)C);
    float* dg = op.up(g, (size_t)C);
    float* dbt = op.up(b, (size_t)C);
    void* dy = op.buf<float>(n);
    launch_dwconv_ln(s_, dtype, dx, B, L, C, dw, db, k, dil, dg, dbt, 1e-6f, dy, dlen);
    down_as(op, s_, dtype, dy, y, n);
    sync();
}

void Engine::op_attention(int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, const float* k, const float* v,
                          const int* qlen, const int* klen, int rope_mode, float* o) {
    OpScope op(*this);
    const int C = H * dh;
    const size_t nq = (size_t)B * Lq * C, nk = (size_t)B * Lk * C;
    const void* pq = up_as(op, s_, dtype, q, nq);
    void* pk = up_as(op, s_, dtype, k, nk);
    const void* pv = up_as(op, s_, dtype, v, nk);
    const int* dql = op.up(qlen, (size_t)B);
    const int* dkl = op.up(klen, (size_t)B);
    void* dO = op.buf<float>(nq);
    const float rbase = a_.rope_base > 0 ? a_.rope_base : 10000.f, rgam = a_.larope_gamma > 0 ? a_.larope_gamma : 10.f;
    const bool prerot = rope_mode >= 0 && (rope_mode & 0x100) != 0;  // test hook: rotate the keys in a separate pass first
    if (prerot) rope_mode &= 0xFF;
    if (prerot) launch_rope_rows(s_, dtype, pk, C, B, Lk, dkl, 1, 0, H, dh, rope_mode, rbase, rgam);
    launch_attention(s_, dtype, pq, C, pk, pv, C, dO, C, B, Lq, Lk, H, dh, dql, dkl, rope_mode, rbase, rgam, prerot);
    down_as(op, s_, dtype, dO, o, nq);
    sync();
}

std::string Engine::op_attention_ex(int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, int64_t q_elems, int ldq, int q_col,
                                    float* kv, int64_t kv_elems, int ldk, int k_col, int v_col, float* o, int64_t o_elems, int ldo,
                                    const int* qlen, const int* klen, const int* q_off, const int* k_off, int rope_mode, int k_rotated,
                                    int rot_groups, int rot_stride, int rot_col) {
    OpScope op(*this);
    const size_t esz = is_half(dtype) ? 2 : 4;
    char* dq = static_cast<char*>(up_as(op, s_, dtype, q, (size_t)q_elems));
    char* dkv = static_cast<char*>(up_as(op, s_, dtype, kv, (size_t)kv_elems));
    char* dO = static_cast<char*>(up_as(op, s_, dtype, o, (size_t)o_elems));
    const int* dql = op.up(qlen, (size_t)B);
    const int* dkl = op.up(klen, (size_t)B);
    const int* dqo = op.up(q_off, (size_t)B);
    const int* dko = op.up(k_off, (size_t)B);
    const float rbase = a_.rope_base > 0 ? a_.rope_base : 10000.f, rgam = a_.larope_gamma > 0 ? a_.larope_gamma : 10.f;
    // as ve_text_kv_dev: every group's keys of the valid rows, once, before any attention reads them
    if (k_rotated) launch_rope_rows(s_, dtype, dkv + (size_t)rot_col * esz, ldk, B, Lk, dkl, rot_groups, rot_stride, H, dh, rope_mode, rbase, rgam, dko);
    const AttnForm f = attn_form(dtype, B, Lq, Lk, H, dh, ldq, ldk, dq + (size_t)q_col * esz, dkv + (size_t)k_col * esz, dkv + (size_t)v_col * esz);
    launch_attention(s_, dtype, dq + (size_t)q_col * esz, ldq, dkv + (size_t)k_col * esz, dkv + (size_t)v_col * esz, ldk, dO, ldo, B, Lq, Lk,
                     H, dh, dql, dkl, rope_mode, rbase, rgam, k_rotated != 0, dqo, dko);
    if (is_half(dtype)) {
        float* w = op.buf<float>(std::max(kv_elems, o_elems));
        launch_half_to_f32(s_, dtype, dkv, kv_elems, w);
        op.down(kv, w, (size_t)kv_elems);
        sync();
        launch_half_to_f32(s_, dtype, dO, o_elems, w);
        op.down(o, w, (size_t)o_elems);
    } else {
        op.down(kv, reinterpret_cast<const float*>(dkv), (size_t)kv_elems);
        op.down(o, reinterpret_cast<const float*>(dO), (size_t)o_elems);
    }
    sync();
    return f.str();
}

std::string Engine::op_xattn_hs(int dtype, int M, const float* xn, const float* Wq, const float* bq, const float* Wo, const float* kv,
                                int64_t kv_elems, int ldk, int k_col, int B, int L, int Lk, const int* qlen, const int* klen, const int* k_off,
                                int rope_mode, int pairs_mode, int64_t part_stride, float* part, int64_t part_elems, int* pairs_out) {
    OpScope op(*this);
    const int C = 384, H = 4;
    const XattnHsForm f = xattn_hs_form(dtype, C, H, B, L, Lk, ldk);
    void* dx = up_as(op, s_, dtype, xn, (size_t)M * C);
    void* wq16 = up_as(op, s_, dtype, Wq, (size_t)C * C);
    void* wo16 = up_as(op, s_, dtype, Wo, (size_t)C * C);
    void* wqf = op.buf<char>((size_t)C * C * 2);
    void* woa = op.buf<char>((size_t)C * C * 2);
    launch_repack_frag(s_, wq16, C, C, wqf);
    launch_repack_frag_acc(s_, wo16, C, C, woa);
    const float* dbq = op.up(bq, (size_t)C);
    char* dkv = static_cast<char*>(up_as(op, s_, dtype, kv, (size_t)kv_elems));
    void* dpart = up_as(op, s_, dtype, part, (size_t)part_elems);
    const int* dql = op.up(qlen, (size_t)B);
    const int* dkl = op.up(klen, (size_t)B);
    const int* dko = op.up(k_off, (size_t)B);
    int* qoff = op.buf<int>((size_t)B + 1);
    launch_row_map(s_, dql, B, qoff, nullptr);
    const int np = 2 * ((B + 1) / 2);
    int* pairs = nullptr;
    if (pairs_mode) {
        pairs = op.buf<int>((size_t)np);
        launch_xattn_hs_pairs(s_, dql, B, pairs);
    }
    const float rbase = a_.rope_base > 0 ? a_.rope_base : 10000.f, rgam = a_.larope_gamma > 0 ? a_.larope_gamma : 10.f;
    const char* kp = dkv + (size_t)k_col * 2;
    launch_xattn_hs(s_, dtype, dx, M, wqf, dbq, kp, kp + (size_t)C * 2, ldk, woa, dpart, part_stride, B, L, Lk, dql, dkl, qoff, dko,
                    rope_mode, rbase, rgam, nullptr, pairs);
    down_as(op, s_, dtype, dpart, part, (size_t)part_elems);
    if (pairs) op.down(pairs_out, pairs, (size_t)np);
    sync();
    return f.str();
}

// The operands of the GEMM timing entries: random A [M][K] and W [N][K] / sqrt(K) in dtype, and the epilogue `mode` names
// (0 GELU store, 1 residual with gamma, 2 plain store, 3 GELU store as fp32)
struct GemmBenchOps { void *A, *W; Epilogue e; };
static GemmBenchOps gemm_bench_ops(OpScope& op, hipStream_t s, int dtype, int M, int N, int K, int mode) {
    const size_t esz = is_half(dtype) ? 2 : 4;
    GemmBenchOps o;
    float* tmp = op.buf<float>(std::max((size_t)M * K, (size_t)N * K));
    o.A = op.buf<char>((size_t)M * K * esz);
    o.W = op.buf<char>((size_t)N * K * esz);
    launch_randn_masked(s, 11, nullptr, 1, 1, (int)std::min<size_t>((size_t)M * K, 1u << 30), nullptr, tmp);
    launch_cast(s, dtype, tmp, (int64_t)M * K, o.A);
    launch_randn_masked(s, 12, nullptr, 1, 1, (int)std::min<size_t>((size_t)N * K, 1u << 30), nullptr, tmp);
    launch_scale(s, tmp, (int)std::min<size_t>((size_t)N * K, 1u << 30), 1.0f / std::sqrt((float)K));
    launch_cast(s, dtype, tmp, (int64_t)N * K, o.W);
    float* bias = op.buf<float>(N);
    float* gamma = op.buf<float>(N);
    launch_fill(s, bias, N, 0.01f);
    launch_fill(s, gamma, N, 0.2f);
    float* resid = op.buf<float>((size_t)M * N);
    void* out = op.buf<float>((size_t)M * N);
    STN_HIP(hipMemsetAsync(resid, 0, (size_t)M * N * 4, s));
    o.e.bias = bias;
    if (mode == 1) { o.e.mode = EPI_RESID; o.e.resid = resid; o.e.ldo = N; o.e.gamma = gamma; }
    else { o.e.mode = EPI_STORE; o.e.act = mode == 2 ? ACT_NONE : ACT_GELU; o.e.out_dtype = mode == 3 ? F32 : dtype; o.e.out = out; o.e.ldo = N; }
    return o;
}

double Engine::op_gemm_bench(int dtype, int M, int N, int K, int mode, int iters) {
    OpScope op(*this);
    const GemmBenchOps o = gemm_bench_ops(op, s_, dtype, M, N, K, mode);
    return time_ms(s_, iters, [&] { launch_gemm(s_, dtype, o.A, K, o.W, K, M, N, K, o.e); });
}

void Engine::op_gemm_phases(int dtype, int M, int N, int K, int mode, double* out6) {
    OpScope op(*this);
    GemmBenchOps o = gemm_bench_ops(op, s_, dtype, M, N, K, mode);
    std::vector<unsigned long long> h((size_t)4 << 16);
    unsigned long long* ts = op.buf<unsigned long long>(h.size());
    for (int i = 0; i < 3; ++i) launch_gemm(s_, dtype, o.A, K, o.W, K, M, N, K, o.e);
    STN_HIP(hipMemsetAsync(ts, 0, h.size() * 8, s_));
    o.e.ts = ts;
    launch_gemm(s_, dtype, o.A, K, o.W, K, M, N, K, o.e);
    op.down(h.data(), ts, h.size());
    sync();
    const Stamps r = reduce_stamps(h);
    if (r.live == 0) throw std::runtime_error("op_gemm_phases: this shape does not run on the tiled kernel");
    for (int i = 0; i < 3; ++i) out6[i] = r.p[i];
    out6[3] = (double)(r.tend - r.tmin); out6[4] = (double)(r.tmax_in - r.tmin); out6[5] = (double)r.live;
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
    OpScope op(*this);
    float* d_w1 = op.up(W1, (size_t)I * C);
    float* d_w2 = op.up(W2, (size_t)C * I);
    FfnOp ff = op_ffn_setup("op_ffn", mode, M, C, I, d_w1, d_w2);
    FfnArgs& fa = ff.a;
    float* d_xn = op.up(xn, (size_t)M * C);
    void* xn16 = act_alloc((int64_t)M * C);
    launch_cast(s_, dt_, d_xn, (int64_t)M * C, xn16);
    float* d_x = op.up(x, (size_t)M * C);
    fa.xn = xn16; fa.x = d_x; fa.b1 = op.up(b1, (size_t)I); fa.b2 = op.up(b2, (size_t)C);
    fa.gamma = op.up(gamma, (size_t)C);
    fa.rowvec = op.up(rowvec, (size_t)nseq * C); fa.rv_ld = C;
    fa.row_b = (rowvec && row_b) ? op.up(row_b, (size_t)M) : nullptr;
    FoldArgs fo = ffn_launch(ff.f, C, fa, ff.w1, ff.w2);
    if (ff.f.kind == FFN_K4_SPLIT) {
        // the pending update, folded by the LayerNorm form of the fold (its normalised output is not part of this op)
        float *ones = op.buf<float>(C), *zeros = op.buf<float>(C);
        launch_fill(s_, ones, C, 1.f); launch_fill(s_, zeros, C, 0.f);
        if (!fo.b2) fo.b2 = zeros;
        if (!fo.gamma) fo.gamma = ones;
        void* y = act_alloc((int64_t)M * C);
        launch_fold_ln(s_, dt_, d_x, M, C, fo, ones, ones, a_.ln_eps, y);
    }
    STN_HIP(hipGetLastError());
    op.down(x, d_x, (size_t)M * C);
    sync();
}

void Engine::op_ffn_bench(int M, int C, int I, int mode, int iters, double* out5) {
    OpScope op(*this);
    for (int i = 0; i < 5; ++i) out5[i] = 0.0;
    // random operands (the clock a chip holds on zeros is not the clock it holds on data)
    float* rnd = op.buf<float>((int64_t)M * C);
    launch_randn_masked(s_, 11, nullptr, 1, M, C, nullptr, rnd);
    float* wr = op.buf<float>((int64_t)I * C);
    launch_randn_masked(s_, 12, nullptr, 1, I, C, nullptr, wr);
    launch_scale(s_, wr, I * C, 0.05f);
    FfnOp ff = op_ffn_setup("op_ffn_bench", mode, M, C, I, wr, wr);
    void* xn16 = act_alloc((int64_t)M * C);
    launch_cast(s_, dt_, rnd, (int64_t)M * C, xn16);
    float* d_b1 = op.buf<float>(I);
    float* d_b2 = op.buf<float>(C);
    float* d_g = op.buf<float>(C);
    launch_fill(s_, d_b1, I, 0.01f); launch_fill(s_, d_b2, C, 0.01f); launch_fill(s_, d_g, C, 0.1f);
    float* d_x = op.buf<float>((int64_t)M * C);
    STN_HIP(hipMemsetAsync(d_x, 0, sizeof(float) * (size_t)M * C, s_));
    ff.a.xn = xn16; ff.a.b1 = d_b1; ff.a.b2 = d_b2; ff.a.gamma = d_g; ff.a.x = d_x;
    const int S = ff.f.split;
    const int nslab = (M + 127) / 128;
    const int nwg = S > 1 ? (nslab + 7) / 8 * 8 * S : nslab;
    unsigned long long* ts = op.buf<unsigned long long>((size_t)4 * nwg);
    auto run = [&](unsigned long long* stamps) { ff.a.ts = stamps; ffn_launch(ff.f, C, ff.a, ff.w1, ff.w2); };
    out5[0] = time_ms(s_, iters, [&] { run(nullptr); });
    if (ff.f.kind != FFN_GEMMS) {
        STN_HIP(hipMemsetAsync(ts, 0, sizeof(unsigned long long) * 4 * (size_t)nwg, s_));
        run(ts);
        std::vector<unsigned long long> h((size_t)4 * nwg);
        op.down(h.data(), ts, h.size());
        sync();
        const Stamps r = reduce_stamps(h);  // (workgroups of a hidden-split grid beyond the last slab exit at once and leave no stamps)
        for (int i = 0; i < 3; ++i) out5[1 + i] = r.p[i];
        out5[4] = (double)r.live;
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
    OpScope op(*this);
    for (int i = 0; i < 6; ++i) out2[i] = 0.0;
    const int64_t M = (int64_t)B * L;
    float* wr = op.buf<float>((int64_t)I * C);
    launch_randn_masked(s_, 12, nullptr, 1, I, C, nullptr, wr);
    launch_scale(s_, wr, I * C, 0.05f);
    FfnOp ff = op_ffn_setup("op_block_bench", mode, (int)M, C, I, wr, wr);
    std::vector<int> len(B, L), off(B + 1);
    for (int i = 0; i <= B; ++i) off[i] = i * L;
    const int* dlen = op.up(len.data(), (size_t)B);
    const int* doff = op.up(off.data(), (size_t)B + 1);
    float* xa = op.buf<float>(M * C);
    float* xb = op.buf<float>(M * C);
    launch_randn_masked(s_, 11, nullptr, 1, (int)M, C, nullptr, xa);
    float* d_b1 = op.buf<float>(I);
    float* d_b2 = op.buf<float>(C);
    float* d_g = op.buf<float>(C);
    float* d_one = op.buf<float>(C);
    float* dwt = op.buf<float>((int64_t)k * C);
    launch_fill(s_, d_b1, I, 0.01f); launch_fill(s_, d_b2, C, 0.01f); launch_fill(s_, d_g, C, 0.01f); launch_fill(s_, d_one, C, 1.f);
    launch_fill(s_, dwt, k * C, 1.f / k);
    void* xn = act_alloc(M * C);
    ff.a.xn = xn; ff.a.b1 = d_b1; ff.a.b2 = d_b2; ff.a.gamma = d_g;
    const bool split = ff.f.kind == FFN_K4_SPLIT;
    if (split) STN_HIP(hipMemsetAsync(ff.a.part, 0, (size_t)ff.a.part_stride * ff.f.split * 2, s_));
    FoldArgs fo = ffn_pending(ff.f, ff.a);  // (K4-split) every block leaves the same pending update
    auto conv = [&]() {
        if (split) { launch_fold_dwconv_ln(s_, dt_, xa, xb, B, L, C, fo, dwt, d_b2, k, dil, d_one, d_b2, 1e-6f, xn, dlen, doff); std::swap(xa, xb); }
        else launch_dwconv_ln(s_, dt_, xa, B, L, C, dwt, d_b2, k, dil, d_one, d_b2, 1e-6f, xn, dlen, doff);
    };
    auto block = [&]() { conv(); ff.a.x = xa; ffn_launch(ff.f, C, ff.a, ff.w1, ff.w2); };
    out2[0] = time_ms(s_, iters, block);
    out2[1] = time_ms(s_, iters, conv);
    if (split) {  // phase stamps of one fold_dwconv_ln launch
        const int nwg = B * ((L + 7) / 8);  // (runs of 8 frames when there are few sequences, of 32 otherwise: sized for the shorter)
        unsigned long long* ts = op.buf<unsigned long long>((size_t)4 * nwg);
        STN_HIP(hipMemsetAsync(ts, 0, sizeof(unsigned long long) * 4 * (size_t)nwg, s_));
        fo.ts = ts;
        conv();
        fo.ts = nullptr;
        std::vector<unsigned long long> h((size_t)4 * nwg);
        op.down(h.data(), ts, h.size());
        sync();
        const Stamps r = reduce_stamps(h);
        if (r.live) { out2[2] = r.p[0]; out2[3] = r.p[1]; out2[4] = r.p[2]; out2[5] = (double)(r.tend - r.tmin); }
    }
    STN_HIP(hipGetLastError());
    sync();
}

std::string Engine::op_ffn_ex(int M, int C, int I, const float* xn, int ldx, int64_t xn_elems, const float* W1, const float* b1, const float* W2,
                              const float* b2, const float* gamma, const int* len, int L, const int* row_b, const float* rowvec, int rv_ld, int nseq,
                              int mode, int split, float* x, int ldo, int64_t x_elems, float* part, int64_t part_stride, int64_t part_elems) {
    OpScope op(*this);
    float* d_w1 = op.up(W1, (size_t)I * C);
    float* d_w2 = op.up(W2, (size_t)C * I);
    FfnOp ff = op_ffn_setup("op_ffn_ex", mode, M, C, I, d_w1, d_w2, split);
    FfnArgs& fa = ff.a;
    fa.xn = up_as(op, s_, dt_, xn, (size_t)xn_elems); fa.ldx = ldx;  // as given, the columns past C of a wider row included
    float* d_x = op.up(x, (size_t)x_elems);
    fa.x = d_x; fa.ldo = ldo;
    fa.b1 = op.up(b1, (size_t)I);
    fa.b2 = op.up(b2, (size_t)C);
    fa.gamma = op.up(gamma, (size_t)C);
    fa.rowvec = op.up(rowvec, (size_t)nseq * rv_ld); fa.rv_ld = rv_ld;
    fa.row_b = op.up(row_b, (size_t)M);
    fa.len = op.up(len, (size_t)nseq); fa.L = L;
    void* d_part = nullptr;
    if (ff.f.kind == FFN_K4_SPLIT) {  // the caller's buffer takes the place of the set-up's: the partial sums are the result, no fold runs
        d_part = up_as(op, s_, dt_, part, (size_t)part_elems);
        fa.part = d_part; fa.part_stride = part_stride;
    }
    ffn_launch(ff.f, C, fa, ff.w1, ff.w2);
    STN_HIP(hipGetLastError());
    op.down(x, d_x, (size_t)x_elems);
    if (d_part) down_as(op, s_, dt_, d_part, part, (size_t)part_elems);
    sync();
    return ff.f.str();
}

std::string Engine::op_dwconv_ln_ex(int dtype, int B, int L, int C, int k, int dil, const float* x, int64_t x_rows, const float* w,
                                    const float* bias, const float* g, const float* b, const int* seqlen, int packed, int ln_only, float* y,
                                    int64_t y_rows, const float* tail, int T, int rf) {
    OpScope op(*this);
    const int* dlen = op.up(seqlen, (size_t)B);
    float* dx = op.up(x, (size_t)x_rows * C);  // as given, padding rows included
    float* dg = op.up(g, (size_t)C);
    float* dbt = op.up(b, (size_t)C);
    void* dy = up_as(op, s_, dtype, y, (size_t)y_rows * C);
    std::string form = "layernorm";
    if (ln_only) {
        launch_layernorm(s_, dtype, dx, (int64_t)B * L, C, dg, dbt, 1e-6f, dy);
    } else {
        const std::vector<float> wt = dw_transposed(w, C, k);
        float* dw = op.up(wt);
        float* db = op.up(bias, (size_t)C);
        int* off = nullptr;
        if (packed) {
            off = op.buf<int>((size_t)B + 1);
            launch_row_map(s_, dlen, B, off, nullptr);
        }
        DwconvTail tl;
        if (tail) { tl.tail = op.up(tail, (size_t)(rf + 1) * C); tl.T = T; tl.rf = rf; }
        form = dwconv_ln_form(dtype, B, L, C, k, packed != 0).str();  // the decision launch_dwconv_ln takes
        launch_dwconv_ln(s_, dtype, dx, B, L, C, dw, db, k, dil, dg, dbt, 1e-6f, dy, dlen, off, tl);
    }
    STN_HIP(hipGetLastError());
    down_as(op, s_, dtype, dy, y, (size_t)y_rows * C);
    sync();
    return form;
}

void Engine::op_fold_ln(int dtype, int M, int C, int S, const float* part, const float* b2, const float* gamma, const float* rowvec,
                        const int* row_b, int nseq, const float* g, const float* b, float* x, float* y) {
    OpScope op(*this);
    const size_t n = (size_t)M * C;
    FoldArgs fo;
    fo.part = up_as(op, s_, dtype, part, n * S); fo.S = S; fo.part_stride = (int64_t)n;
    fo.b2 = op.up(b2, (size_t)C); fo.gamma = op.up(gamma, (size_t)C);
    fo.rowvec = op.up(rowvec, (size_t)nseq * C); fo.rv_ld = C;
    fo.row_b = (rowvec && row_b) ? op.up(row_b, (size_t)M) : nullptr;
    float* dx = op.up(x, n);
    float* dg = op.up(g, (size_t)C);
    float* dbt = op.up(b, (size_t)C);
    void* dy = op.buf<char>(n * 2);
    launch_fold_ln(s_, dtype, dx, M, C, fo, dg, dbt, 1e-6f, dy);
    STN_HIP(hipGetLastError());
    op.down(x, dx, n);
    down_as(op, s_, dtype, dy, y, n);
    sync();
}

std::string Engine::op_fold_dwconv_ln_ex(int dtype, int B, int L, int C, int k, int dil, int S, int run_frames, const int* seqlen, const float* x_in,
                                         int64_t x_rows, const float* part, int64_t part_stride, int64_t part_elems, const float* b2, const float* gamma,
                                         const float* rowvec, int rv_ld, const float* w, const float* bias, const float* g, const float* b, float* x_out,
                                         int64_t x_out_rows, float* y, int64_t y_rows) {
    OpScope op(*this);
    const std::vector<float> wt = dw_transposed(w, C, k);
    const int* dlen = op.up(seqlen, (size_t)B);
    int* doff = op.buf<int>((size_t)B + 1);
    launch_row_map(s_, dlen, B, doff, nullptr);
    float* dx = op.up(x_in, (size_t)x_rows * C);  // as given, the rows behind the last sequence included
    float* dxo = op.up(x_out, (size_t)x_out_rows * C);
    void* dy = up_as(op, s_, dtype, y, (size_t)y_rows * C);
    float* dw = op.up(wt);
    float* db = op.up(bias, (size_t)C);
    float* dg = op.up(g, (size_t)C);
    float* dbt = op.up(b, (size_t)C);
    FoldArgs fo;
    fo.part = up_as(op, s_, dtype, part, (size_t)part_elems); fo.S = S; fo.part_stride = part_stride;
    if (b2) fo.b2 = op.up(b2, (size_t)C);
    else { float* z = op.buf<float>(C); launch_fill(s_, z, C, 0.f); fo.b2 = z; }
    if (gamma) fo.gamma = op.up(gamma, (size_t)C);
    else { float* o = op.buf<float>(C); launch_fill(s_, o, C, 1.f); fo.gamma = o; }
    fo.rowvec = op.up(rowvec, (size_t)B * rv_ld); fo.rv_ld = rowvec ? rv_ld : C;
    fo.run_frames = run_frames;
    const std::string form = fold_dwconv_ln_form(dtype, B, L, C, k, dil, S, rowvec != nullptr, run_frames).str();  // the decision launch_fold_dwconv_ln takes
    launch_fold_dwconv_ln(s_, dtype, dx, dxo, B, L, C, fo, dw, db, k, dil, dg, dbt, 1e-6f, dy, dlen, doff);
    STN_HIP(hipGetLastError());
    op.down(x_out, dxo, (size_t)x_out_rows * C);
    down_as(op, s_, dtype, dy, y, (size_t)y_rows * C);
    sync();
    return form;
}

// One layout kernel of kernels_layout.hip on host operands (stn_op_layout).  Every destination is the caller's whole buffer: uploaded as given,
// downloaded whole.  Every extent a kernel addresses is checked against the buffers here, before anything is launched.
void Engine::op_layout(int which, int dtype, const int* p, const float* a, int64_t a_n, const float* b, int64_t b_n, const float* c, int64_t c_n,
                       const int64_t* ids, int64_t ids_n, const int* len, int packed, float* out, int64_t out_n, float* out2, int64_t out2_n,
                       int* iout, int64_t iout_n) {
    OpScope op(*this);
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
        int* off = op.buf<int>((size_t)B + 1);
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
        const int* dlen = op.up(len, (size_t)B);
        int* d = op.up(iout, (size_t)iout_n);
        launch_row_map(s_, dlen, B, d, with_b ? d + B + 1 : nullptr, rows_padded);
        op.down(iout, d, (size_t)iout_n);
        break;
    }
    case 1: {  // ncl_to_rows: p = {B, C, L, ld_out}; a [B][C][L]; out rows of ld_out in dtype
        const int B = p[0], C = p[1], L = p[2], ldo = p[3];
        need(C > 0 && L > 0 && ldo >= C && a && out, "ncl_to_rows: bad shape");
        check_len(B, L, false);
        need(a_n >= (int64_t)B * C * L && out_n >= rows_needed(B, L) * ldo, "ncl_to_rows: buffer too small");
        const int* dlen = op.up(len, (size_t)B);
        float* da = op.up(a, (size_t)a_n);
        void* d = up_as(op, s_, dtype, out, (size_t)out_n);
        launch_ncl_to_rows(s_, dtype, da, B, C, L, d, ldo, dlen, row_off(dlen, B));
        down_as(op, s_, dtype, d, out, (size_t)out_n);
        break;
    }
    case 2: {  // euler_ncl: p = {B, D, L, with_z, ldz}; a = prev [B][D][L], b = v rows of D, c = dt [B]; out [B][D][L] fp32; out2 = z rows of ldz in dtype
        const int B = p[0], D = p[1], L = p[2], with_z = p[3], ldz = p[4];
        need(D > 0 && L > 0 && a && b && c && out && (!with_z || (out2 && ldz >= D)), "euler_ncl: bad shape");
        check_len(B, L, false);
        const int64_t vr = rows_needed(B, L);
        need(a_n >= (int64_t)B * D * L && out_n >= (int64_t)B * D * L && c_n >= B && b_n >= vr * D && (!with_z || out2_n >= vr * ldz), "euler_ncl: buffer too small");
        const int* dlen = op.up(len, (size_t)B);
        float* dp = op.up(a, (size_t)a_n);
        float* dv = op.up(b, (size_t)b_n);
        float* ddt = op.up(c, (size_t)c_n);
        float* d = op.up(out, (size_t)out_n);
        void* dz = with_z ? up_as(op, s_, dtype, out2, (size_t)out2_n) : nullptr;
        launch_euler_ncl(s_, dp, dv, ddt, dlen, B, D, L, d, row_off(dlen, B), dz, dtype, ldz);
        op.down(out, d, (size_t)out_n);
        if (dz) down_as(op, s_, dtype, dz, out2, (size_t)out2_n);
        break;
    }
    case 3: {  // unpack_rows: p = {B, T, W}; a = packed rows [sum len][W]; out [B][T][W] fp32
        const int B = p[0], T = p[1], W = p[2];
        need(T > 0 && W > 0 && W % 4 == 0 && a && out, "unpack_rows: bad shape");
        packed = 1;
        check_len(B, T, true);
        need(a_n >= rows_needed(B, T) * W && a_n > 0 && out_n >= (int64_t)B * T * W, "unpack_rows: buffer too small");
        const int* dlen = op.up(len, (size_t)B);
        float* da = op.up(a, (size_t)a_n);
        float* d = op.up(out, (size_t)out_n);
        launch_unpack_rows(s_, da, dlen, row_off(dlen, B), B, T, W, d);
        op.down(out, d, (size_t)out_n);
        break;
    }
    case 4: {  // embed: p = {vocab, B, L, C}; ids [B][L]; a = table [vocab][C]; out rows of C fp32
        const int vocab = p[0], B = p[1], L = p[2], C = p[3];
        need(vocab > 0 && L > 0 && C > 0 && C % 4 == 0 && ids && a && out, "embed: bad shape");
        check_len(B, L, true);
        need(ids_n >= (int64_t)B * L && a_n >= (int64_t)vocab * C && out_n >= rows_needed(B, L) * C, "embed: buffer too small");
        const int* dlen = op.up(len, (size_t)B);
        int64_t* di = op.up(ids, (size_t)ids_n);
        float* da = op.up(a, (size_t)a_n);
        float* d = op.up(out, (size_t)out_n);
        launch_embed(s_, di, da, vocab, B, L, C, dlen, d, row_off(dlen, B));
        op.down(out, d, (size_t)out_n);
        break;
    }
    case 5: {  // masked_mean: p = {B, L, C}; a = rows of C (rounded to dtype); out [B][C] fp32
        const int B = p[0], L = p[1], C = p[2];
        need(L > 0 && C > 0 && a && out, "masked_mean: bad shape");
        check_len(B, L, true);
        need(a_n >= rows_needed(B, L) * C && a_n > 0 && out_n >= (int64_t)B * C, "masked_mean: buffer too small");
        const int* dlen = op.up(len, (size_t)B);
        void* da = up_as(op, s_, dtype, a, (size_t)a_n);
        float* d = op.up(out, (size_t)out_n);
        launch_masked_mean(s_, dtype, da, B, L, C, dlen, d, row_off(dlen, B));
        op.down(out, d, (size_t)out_n);
        break;
    }
    case 6: {  // vocoder_im2col: p = {B, L, ld, ccf, k, kp}; a = latent [B][ld*ccf][L]; len = valid vocoder frames; out rows of kp in dtype
        const int B = p[0], L = p[1], ld = p[2], ccf = p[3], k = p[4], kp = p[5];
        need(L > 0 && ld > 0 && ccf > 0 && k > 0 && (k & 1) && kp > 0 && a && out, "vocoder_im2col: bad shape");
        check_len(B, L * ccf, false);
        need(a_n >= (int64_t)B * ld * ccf * L && out_n >= rows_needed(B, L * ccf) * kp, "vocoder_im2col: buffer too small");
        const int* dlen = op.up(len, (size_t)B);
        float* da = op.up(a, (size_t)a_n);
        void* d = up_as(op, s_, dtype, out, (size_t)out_n);
        launch_vocoder_im2col(s_, dtype, da, B, L, ld, ccf, k, kp, d, dlen, row_off(dlen, B));
        down_as(op, s_, dtype, d, out, (size_t)out_n);
        break;
    }
    case 7: {  // vocoder_in: p = {B, L, ld, ccf, C, k}; a = latent, b = weights [ld*k][C], c = bias [C]; len = valid vocoder frames; out [B*T][C] fp32
        const int B = p[0], L = p[1], ld = p[2], ccf = p[3], C = p[4], k = p[5];
        need(L > 0 && ld > 0 && ccf > 0 && C > 0 && k > 0 && (k & 1) && (int64_t)(8 + k - 1) * ld * 4 <= 64 * 1024 && a && b && c && out, "vocoder_in: bad shape");
        need(!packed, "vocoder_in: padded rows only");
        check_len(B, L * ccf, false);
        need(a_n >= (int64_t)B * ld * ccf * L && b_n >= (int64_t)ld * k * C && c_n >= C && out_n >= (int64_t)B * L * ccf * C, "vocoder_in: buffer too small");
        const int* dlen = op.up(len, (size_t)B);
        float* da = op.up(a, (size_t)a_n);
        float* dw = op.up(b, (size_t)b_n);
        float* db = op.up(c, (size_t)c_n);
        float* d = op.up(out, (size_t)out_n);
        launch_vocoder_in(s_, da, B, L, ld, ccf, dw, db, C, k, d, dlen);
        op.down(out, d, (size_t)out_n);
        break;
    }
    case 8: {  // fill_rows: p = {B, T, W, rf, zeros}; len = valid [B]; a = quiet [W], b = edge [rf][W] (unused with zeros); out [B][T][W] fp32
        const int B = p[0], T = p[1], W = p[2], rf = p[3], zeros = p[4];
        need(T > 0 && W > 0 && W % 4 == 0 && rf >= 0 && rf <= T && out, "fill_rows: bad shape");
        check_len(B, T, true);
        need(out_n >= (int64_t)B * T * W, "fill_rows: buffer too small");
        need(zeros || (a && a_n >= W && (rf == 0 || (b && b_n >= (int64_t)rf * W))), "fill_rows: the quiet rule needs quiet [W] and edge [rf][W]");
        const int* dlen = op.up(len, (size_t)B);
        const float* dq = zeros ? nullptr : op.up(a, (size_t)a_n);
        const float* de = (zeros || rf == 0) ? nullptr : op.up(b, (size_t)b_n);
        float* d = op.up(out, (size_t)out_n);
        launch_fill_rows(s_, dlen, B, T, W, rf, dq, de, d);
        op.down(out, d, (size_t)out_n);
        break;
    }
    case 9: {  // hs_pairs: p = {B}; len [B]; iout: the pairing, 2 * ceil(B / 2) words
        const int B = p[0];
        check_len(B, 1 << 20, true);
        need(iout && iout_n >= 2 * ((B + 1) / 2), "hs_pairs: iout too small");
        const int* dlen = op.up(len, (size_t)B);
        int* d = op.up(iout, (size_t)iout_n);
        launch_xattn_hs_pairs(s_, dlen, B, d);
        op.down(iout, d, (size_t)iout_n);
        break;
    }
    case 10: {  // trim_len: p = {B, ccf, T, rf, tail_form}; len [B] latent lengths; iout = n [B] then valid [B]
        const int B = p[0], ccf = p[1], T = p[2], rf = p[3], tail_form = p[4];
        need(ccf > 0 && T > 0 && rf >= 0, "trim_len: bad shape");
        check_len(B, T / ccf, true);
        need(iout && iout_n >= 2 * (int64_t)B, "trim_len: iout too small");
        const int* dlen = op.up(len, (size_t)B);
        int* d = op.up(iout, (size_t)iout_n);
        launch_trim_len(s_, dlen, B, ccf, T, rf, d, d + B, tail_form != 0);
        op.down(iout, d, (size_t)iout_n);
        break;
    }
    default: need(false, "unknown kernel");
    }
    STN_HIP(hipGetLastError());
    sync();
}

void Engine::op_randn(uint64_t seed, int B, int D, int L, const int64_t* utt_ids, const int* len, float* out) {
    OpScope op(*this);
    int64_t* du = op.up(utt_ids, (size_t)B);
    int* dl = op.up(len, (size_t)B);
    float* d = op.buf<float>((size_t)B * D * L);
    launch_randn_masked(s_, seed, du, B, D, L, dl, d);
    op.down(out, d, (size_t)B * D * L);
    sync();
}

}  // namespace stn
