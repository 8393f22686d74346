// kernels.hpp — launch interface of the hand-written gfx950 kernels (kernels_*.hip).
// Activation layout everywhere: row-major [rows = b*len + t][channels].
// The residual stream is always fp32; "operand" activations (LayerNorm outputs, GELU hidden,
// q/k/v/o) are `act_t` = float (STN_F32) or bf16 (STN_BF16).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>
#include <string>

#include "dither.hpp"

namespace stn {

// Kernel-exact timing: when a pair of events is armed here, the NEXT kernel launched through STN_KLAUNCH carries them on
// its own dispatch packet (hipExtLaunchKernelGGL: start/stop are the kernel's begin/end timestamps, what rocprofv3 reports),
// instead of being bracketed by hipEventRecord barriers that add the dispatch boundary to the span.
struct LaunchEvents { hipEvent_t start = nullptr, stop = nullptr; };
inline thread_local LaunchEvents g_launch_ev;
// Launch log (profiling runs only): kernel expression + the kernel family the engine was in, one entry per launch in dispatch
// order — what tools/pmc_families.py aligns rocprofv3's per-dispatch rows with, so that counters are attributed to families
// by position instead of by guessing from template arguments and grid sizes.
struct LaunchLog {
    bool on = false;
    const char* family = "-";
    std::vector<std::pair<std::string, const char*>> entries;  // (family, kernel expression)
    void add(const char* kexpr) { if (entries.size() < 200000) entries.emplace_back(family, kexpr); }
};
inline thread_local LaunchLog g_launch_log;
#define STN_KLAUNCH(kernel, grid, block, lds, stream, ...)                                                              \
    do {                                                                                                                \
        if (::stn::g_launch_log.on) ::stn::g_launch_log.add(#kernel);                                                   \
        if (::stn::g_launch_ev.start) {                                                                                 \
            const ::stn::LaunchEvents ev_ = ::stn::g_launch_ev;                                                         \
            ::stn::g_launch_ev = ::stn::LaunchEvents{};                                                                 \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, ev_.start, ev_.stop, 0, __VA_ARGS__);               \
        } else {                                                                                                        \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                          \
        }                                                                                                               \
    } while (0)

// hipFuncSetAttribute is per device: one flag per (kernel instantiation, device) so that several handles on different GPUs in
// one process each opt their device in (flags are only ever set to true, so a race merely repeats the call)
struct PerDeviceOnce {
    bool done[64] = {};
    bool need() { int d = 0; (void)hipGetDevice(&d); d &= 63; if (done[d]) return false; done[d] = true; return true; }
};

// launch-side HIP calls that must not fail silently (a failed attribute call leaves a sticky error that surfaces in
// whatever library checks hipGetLastError next).  Nothing in this library calls abort(): contract violations and HIP failures
// are exceptions, which the C ABI (api.cpp) turns into STN_ERR_INVALID / STN_ERR_DEVICE + stn_last_error — the reference's
// hosts get std::runtime_error from the same situations (/root/reference/cpp/helper.cpp:479-481, 193).
inline void stn_check_hip(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + what + " failed: " + hipGetErrorString(e));
}


enum DType : int { F32 = 0, BF16 = 1, F16 = 2 };  // F16: IEEE half operands / activations (v_mfma_f32_32x32x16_f16), fp32 accumulate
__host__ __device__ inline bool is_half(int dt) { return dt == BF16 || dt == F16; }  // 2-byte storage
typedef _Float16 f16_t;                                          // storage type of the F16 mode (bf16 is raw uint16_t)
// The storage type of a run-time format as a template argument: calls fn with a null pointer of float (F32 — and, as these launchers always
// have, any value that is neither of the others), uint16_t (BF16) or f16_t (F16).  In the callee: using T = std::remove_pointer_t<decltype(tag)>.
template <typename Fn>
inline void with_out_type(int dtype, Fn&& fn) {
    if (dtype == F16) fn(static_cast<f16_t*>(nullptr));
    else if (dtype == BF16) fn(static_cast<uint16_t*>(nullptr));
    else fn(static_cast<float*>(nullptr));
}
// the 16-bit pair only, for launchers that take nothing else: f16_t for F16, else uint16_t
template <typename Fn>
inline void with_half_type(int dtype, Fn&& fn) {
    if (dtype == F16) fn(static_cast<f16_t*>(nullptr));
    else fn(static_cast<uint16_t*>(nullptr));
}
enum ActFn : int { ACT_NONE = 0, ACT_GELU = 1, ACT_SILU = 2, ACT_GELU_TANH = 3 };  // GELU: erf form; GELU_TANH: 0.5 x (1 + tanh(sqrt(2/pi)(x + 0.044715 x^3)))

// GEMM epilogue description:  acc[m][n] = sum_k A[m][k] * W[n][k]
// (the order matters: EPI_STORE and EPI_RESID are the 16-byte vector epilogues, every mode above EPI_RESID transposes per lane)
enum EpiMode : int {
    EPI_STORE = 0,    // out[m*ldo + n] = act(acc + bias[n]) * rowmask(m)        (out dtype = out_dtype)
    EPI_RESID = 1,    // resid[m*ldo+n] = (resid + gamma[n]*(acc+bias[n]) + rowvec[b]) * rowmask(m)      (fp32, in place)
    EPI_STORE_T = 2,  // out[b][n][t] = (acc+bias[n]) * rowmask                                  (fp32, [B,N,L])
};

struct Epilogue {
    int mode = EPI_STORE;
    int act = ACT_NONE;
    int out_dtype = F32;         // EPI_STORE only
    const float* bias = nullptr; // [N] or null
    void* out = nullptr;         // EPI_STORE / EPI_STORE_T destination
    int ldo = 0;                 // row stride of out / resid (elements)
    const float* gamma = nullptr;// [N] layer-scale (EPI_RESID) or null
    float* resid = nullptr;      // EPI_RESID
    const int* len = nullptr;    // [B] valid rows per sequence (null -> no row mask)
    int L = 1;                   // rows per sequence (row m -> b = m / L, t = m % L)
    const int* row_b = nullptr;       // packed rows: sequence of row m (replaces m / L for rowvec; len must be null then)
    const float* rowvec = nullptr;    // EPI_RESID: per-sequence vector [B][rv_ld] added to every row of sequence b (time
    int rv_ld = 0;                    //            conditioning): resid = (resid + gamma*(acc+bias) + rowvec[b]) * keep
    // EPI_STORE, fp32 out, the tiled kernels' slab epilogue only (gemm_form_maps_rows): the rows of the GEMM are packed per sequence and each
    // is stored where it belongs in a padded [map_B][map_T] destination — row r of sequence b (map_off[b] <= r < map_off[b + 1], t = r - map_off[b])
    // goes to row b * map_T + t of out when t < map_valid[b] and is not stored otherwise (nor are rows from map_off[map_B] on).  len must be null.
    const int* map_off = nullptr;     // [map_B + 1] row offsets (launch_row_map); null: no map, row m is stored at row m
    const int* map_valid = nullptr;   // [map_B] rows of each sequence that are stored (<= the rows it owns)
    int map_B = 0, map_T = 0;
    int ksplit = 1;                   // tiled kernels: split-K factor (plain fp32 store of partials; launch_gemm_splitk)
    int nt = 0;                       // tiled kernels: 1 = non-temporal 16-bit output stores, for a stream far larger than the Infinity Cache
                                      // (the vocoder's 245 MB hidden activation): vo.pw1 185 -> 166 us.  The matching non-temporal A loads in
                                      // pw2 were measured too and cost +9 % (each A panel is read by two column tiles), non-temporal loads of the old residual in pw2's
                                      // epilogue +3 %: so there are none
    int tr_epilogue = 0;              // tiled kernels, bf16 store: wave-private transposed-image epilogue (set by the launcher)
    int tr_force = -1;                // tests only (stn_op_gemm_ex; the engine never sets it): >= 0 replaces the launcher's choice of
                                      // tr_epilogue with this value (0 = fp32 slab store, 1 = transposed image)
    unsigned long long* ts = nullptr; // diagnostics (tiled kernels): 4 shader-clock stamps per workgroup — entry, first
                                      // stage landed, K-loop done, epilogue done (stn_op_gemm_phases)
};

// The form a GEMM call takes — one decision, made by gemm_form and executed by launch_gemm_form, so that what the diagnostics report
// (stn_dbg_gemm_form, stn_op_gemm_ex) is what runs:
//   GK_TILED     gemm_tiled_kernel, configuration `cfg` (launch_tiled_auto's table: 1..18 for 16-bit operands, GEMM_CFG_F32_64 /
//                GEMM_CFG_F32_128 for the fp32 tiles) with template arguments bm..esz
//   GK_RING_VEC  gemm_bf16_ring_kernel<VEC = true>, GK_RING  <VEC = false>
//   GK_REG       the register-staged gemm_bf16_kernel / gemm_f32_kernel
// split > 1: deterministic split-K — the fields above describe the launch of the fp32 partial sums (plain store), and
// splitk_reduce_kernel applies the real epilogue (per lane).
enum GemmKernel : int { GK_TILED = 0, GK_RING_VEC = 1, GK_RING = 2, GK_REG = 3 };
enum GemmEpiForm : int { GE_LANE = 0, GE_SLAB = 1, GE_TR = 2 };  // per-lane stores, fp32 slab through LDS, transposed 16-bit image
constexpr int GEMM_CFG_F32_64 = 19, GEMM_CFG_F32_128 = 20;
struct GemmForm {
    int dtype = F32, mode = EPI_STORE;
    int kernel = GK_REG;
    int cfg = 0;
    int bm = 128, bn = 128, wm = 2, wn = 2, nstage = 2, ks = 64, esz = 2;  // tile template arguments (GK_TILED)
    int epi = GE_LANE;
    int tr_epilogue = 0;              // the value the tiled kernel receives
    int split = 1;
    std::string str() const;          // e.g. "tiled<128,128,2,4,4,64,2> cfg8 tr", "ring_vec slab", "splitk6+tiled<64,64,2,2,4,32,4> slab"
};
// A: [M][lda] (dtype), W: [N][ldw] (same dtype), K % 8 == 0 (16-bit) / K % 4 == 0 (f32), 16-byte aligned rows.  A and W are read
// for their alignment only (null is aligned); so are e.out / e.resid / e.bias / e.gamma.  allow_split = false: never split-K (a
// caller without a workspace).  Throws std::invalid_argument where the operands violate the kernel contract.
GemmForm gemm_form(int dtype, int M, int N, int K, int lda, int ldw, const Epilogue& e, const void* A, const void* W, bool allow_split = true);
// runs form f (from gemm_form on the same arguments); workspace: [f.split][M][N] fp32 when f.split > 1, else unused
void launch_gemm_form(hipStream_t s, const GemmForm& f, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
                      const Epilogue& e, float* workspace);
// whether form f can execute an Epilogue with a packed-row destination map (map_off): the tiled kernels' fp32 slab store, no split.
// launch_gemm_form throws std::invalid_argument for a map on any other form.
bool gemm_form_maps_rows(const GemmForm& f);
// gemm_form(..., allow_split = false) and launch_gemm_form in one call
void launch_gemm(hipStream_t s, int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K,
                 const Epilogue& e);
// Deterministic split-K for tiny-M, long-K GEMMs: gemm_splitk_factor says how many ways to split (1 = don't; gemm_form's rule);
// launch_gemm_splitk runs the splits into `workspace` ([S][M][N] fp32) and reduces them in split order with epilogue e.
int gemm_splitk_factor(int dtype, int M, int N, int K, const Epilogue& e);
void launch_gemm_splitk(hipStream_t s, int dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const Epilogue& e,
                        int S, float* workspace);

// K4 — the pointwise pair of a ConvNeXt block in one launch (kernels_ffn.hip):
//   x[m][:] <- (x[m][:] + gamma * (W2 . GELU(W1 . xn[m] + b1) + b2) + rowvec[seq(m)]) * keep(m)
// 16-bit modes; W1 / W2 pre-packed once at model load (launch_repack_frag / launch_repack_frag_acc).
struct FfnArgs {
    const void* xn = nullptr; int ldx = 0;        // LayerNorm output [M][ldx], 16-bit activation format
    const void* wseq = nullptr;                   // both matrices in fragment order, interleaved in the order the kernel consumes
                                                  // them (launch_ffn_pack): 2 * I * C 16-bit values
    const float* b1 = nullptr;                    // [I]
    const float* b2 = nullptr;                    // [C] or null
    const float* gamma = nullptr;                 // [C] layer scale or null
    float* x = nullptr; int ldo = 0;              // residual stream [M][ldo] fp32, updated in place
    int M = 0, I = 0;
    const int* row_b = nullptr;                   // packed rows: sequence of row m (for rowvec)
    const float* rowvec = nullptr; int rv_ld = 0; // per-sequence vector added to every row (time conditioning) or null
    const int* len = nullptr; int L = 1;          // padded rows: row m = b*L + t is zeroed when t >= len[b] (null: no mask)
    unsigned long long* ts = nullptr;             // diagnostics: 4 shader-clock stamps per workgroup (entry, first stage, loop, end)
    // hidden split (ffn_split_factor(C, I) = S > 1): S workgroups per 128-row slab, each over I/S hidden units; wseq packed with
    // the same S (launch_ffn_pack); the result is NOT applied to x: part[sp][m][:] (16-bit, [S][part_stride / C rows][C]) receives
    // W2[:, hidden share sp] . GELU(W1[hidden share sp] . xn[m] + b1) and launch_fold_ln / launch_fold_dwconv_ln fold
    // x <- x + gamma * (sum_sp part[sp] + b2) + rowvec into the residual stream.  b2 / gamma / x / rowvec / len are unused here.
    int split = 1;
    void* part = nullptr;                         // rows padded to a multiple of 128
    int64_t part_stride = 0;                      // elements between two splits (= padded rows * C)
};
bool ffn_fused_supported(int dtype, int C, int I);
// whether the block shape has a K4-split form at all (0: no; > 1: yes)
int ffn_split_factor(int dtype, int C, int I);
// the splits K4-split runs with: one packed weight stream per entry (Engine::prepare_ffn_weights); ffn_split_choose hands out no other
constexpr int FFN_SPLITS[] = {4, 8, 12};
// splits a block shape can run with (FFN_SPLITS: I / 32 / S hidden tiles per workgroup, an even number), and the one a launch of M rows
// takes: 12 ways up to 12 slabs (1536 rows), 8 ways up to 32 slabs (4096 rows: still one round of workgroups), 4 ways beyond.  The split is a function of the launch's ROW COUNT, so the order in which a
// row's 16-bit partial sums are added depends on how many rows the launch has: results on either side of the boundary (an utterance
// alone, a 16-utterance shard of a strong-scaling run, the unsharded batch) agree to rounding, not bit for bit (include/stn.h,
// tests/test_gpu_ffn.py::test_ffn_split_regimes_agree_to_rounding: 1 536, 1 664 and 4 224 rows)
bool ffn_split_valid(int dtype, int C, int I, int S);
int ffn_split_choose(int dtype, int C, int I, int64_t M);
inline int64_t ffn_split_rows(int64_t M) { return (M + 127) / 128 * 128; }
// The form a ConvNeXt block's pointwise pair takes — one decision, made by ffn_form and executed by Engine::ffn_launch, so that what the
// diagnostics report (stn_dbg_ffn_form) is what runs: two tiled GEMMs (nt: pw1's hidden activation stored non-temporally), K4, or K4-split
// over `split` hidden shares whose update the next reader of x folds in.
enum FfnKind : int { FFN_GEMMS = 0, FFN_K4 = 1, FFN_K4_SPLIT = 2 };
enum FfnStage : int { FFN_VOCODER = 1, FFN_ESTIMATOR = 2, FFN_TEXT = 4 };  // (FFN_TEXT: also the duration predictor) the stage's bit of the K4 mask
struct FfnForm {
    int kind = FFN_GEMMS, split = 1;
    bool nt = false;
    std::string str() const;  // "gemms", "gemms nt", "k4", "k4split12"
};
// M: the launch's rows; gate_rows > 0: the rows K4 is decided on instead (a trimmed vocoder's dense B*T); packed: rows packed per sequence;
// k, max_dil: the stage's conv taps and largest dilation (the fold kernel must take them); mask, min_rows, split_min_rows, nt_hints: the engine's settings.
FfnForm ffn_form(int dtype, int stage, int C, int I, int64_t M, int64_t gate_rows, bool packed, int k, int max_dil, int mask, int64_t min_rows,
                 int64_t split_min_rows, bool nt_hints);
// K4's LDS layout, one definition for the kernel and its launcher: 4 ring buffers of C * 64 bytes | b2, gamma (C floats each) | b1 (I floats) |
// at C = 384 a fifth buffer, KiB-aligned, for wave 0's rows of the slab in the prologue (kernels_ffn_body.inc)
__host__ __device__ constexpr inline int ffn_lds_side_offset(int C, int I) { return (4 * C * 64 + (I + 2 * C) * 4 + 1023) & ~1023; }
__host__ __device__ constexpr inline bool ffn_lds_has_side(int C) { return C == 384; }
void launch_ffn_fused(hipStream_t s, int dtype, int C, const FfnArgs& a);
// The pending update of a K4-split launch, folded by the next reader of x:
//   x_new[m] = x[m] + gamma * (((part[0][m] + part[1][m]) + part[2][m]) + ... + b2) + rowvec[seq(m)]      (fp32, this order)
struct FoldArgs {
    const void* part = nullptr; int S = 0; int64_t part_stride = 0;   // 16-bit partial sums (the engine's activation format)
    const float* b2 = nullptr;        // [C] or null
    const float* gamma = nullptr;     // [C] or null (1)
    const float* rowvec = nullptr; int rv_ld = 0;  // per-sequence vector or null
    const int* row_b = nullptr;       // fold_ln with rowvec: sequence of row m
    unsigned long long* ts = nullptr; // diagnostics (fold_dwconv_ln): 4 shader-clock stamps per workgroup — entry, phase 1 done, hand-over, end
    int run_frames = 0;               // fold_dwconv_ln: longest run of frames a workgroup takes (0: the default, 32; fold_run_frames() picks it from the lengths)
};
// fold_dwconv_ln puts ONE 1024-thread workgroup on a CU, so a launch of 257 workgroups takes two rounds where 256 take one (12.6 -> 16.2 us at
// the bench's shape).  The run length whose GRID (B x ceil(longest / run): the placeholders of runs a sequence does not have take a CU each on their way
// out) fits ONE round of `n_cu` workgroups — 40 or 48 frames where 32 does not; 0 (the default) otherwise: with several rounds either way the count
// of rounds stops predicting the time.  A frame's arithmetic does not depend on the run it falls in: same bits for any choice.
int fold_run_frames(const int* lengths, int B, int n_cu);
// x (in place) <- folded x;  y <- LayerNorm(folded x)       (rows are independent)
void launch_fold_ln(hipStream_t s, int act_dtype, float* x, int64_t M, int C, const FoldArgs& f, const float* g, const float* b, float eps, void* y);
// packed rows only (row_off / seqlen as launch_dwconv_ln): x_out <- folded x_in (x_out != x_in: a workgroup re-folds the halo rows
// of its neighbours);  y <- LayerNorm(dwconv(folded x)).  k = 5 or 7, C % 8 == 0, C <= 512.
bool fold_dwconv_ln_supported(int C, int k, int dil);
// The form a fold + depthwise conv + LayerNorm call takes — one decision, made by fold_dwconv_ln_form and executed by launch_fold_dwconv_ln, so
// that what the diagnostics report (stn_dbg_fold_dwconv_ln_form, stn_op_fold_dwconv_ln_ex) is what runs: the instantiation
// fold_dwconv_ln_kernel<OutT / F16, K, RV, NSLOT, S> (NSLOT 3 up to C = 384, 4 above; U: window rows per thread and trip of phase 1), the run
// length (8 when B * ceil(L / 32) < 64, else 32, else run_frames where that is 40 or 48 and its image fits 160 KiB of LDS), the workgroups per
// sequence cps = ceil(L / run), the grid B * cps and the dynamic LDS bytes.
struct FoldDwconvLnForm {
    int act_dtype = BF16, K = 5, nslot = 3, S = 4, U = 1, run = 32, cps = 1;
    bool rv = false;
    unsigned grid = 0;
    size_t lds = 0;
    std::string str() const;  // "fold_dwconv_ln<bf16,K5,rv,ns3,S4,U3> run 40 cps 3" ("norv" without a per-sequence vector)
};
// Throws std::invalid_argument where the launcher refuses: fp32, B or L < 1, !fold_dwconv_ln_supported(C, k, dil), S outside {4, 8, 12, 24}.
FoldDwconvLnForm fold_dwconv_ln_form(int act_dtype, int B, int L, int C, int k, int dil, int S, bool has_rowvec, int run_frames);
void launch_fold_dwconv_ln(hipStream_t s, int act_dtype, const float* x_in, float* x_out, int B, int L, int C, const FoldArgs& f, const float* w_t,
                           const float* bias, int k, int dil, const float* ln_g, const float* ln_b, float eps, void* y, const int* seqlen,
                           const int* row_off);
// W [N][K] row-major 16-bit -> A fragments whose k order matches a GELU'd accumulator used as the B operand (N % 32, K % 32 == 0)
void launch_repack_frag_acc(hipStream_t s, const void* W, int N, int K, void* Wf);
// W1 [I][C], W2 [C][I] (row-major 16-bit) -> wseq: hidden tile t of W1 as C/16 KiB fragment pieces, hidden tile t of W2 as
// C/16 KiB pieces in the accumulator-operand order, laid out as the stage sequence W1(0), W1(1), W2(0), W1(2), W2(1), ...,
// W1(T-1), W2(T-2), W2(T-1) (T = I/32): the kernel's LDS-DMA stream is then one linear walk through memory.
// tmp: 2 * I * C 16-bit values of scratch.
// S > 1 (hidden split): S such streams one after another, stream sp over hidden tiles [sp*T/S, (sp+1)*T/S).
void launch_ffn_pack(hipStream_t s, const void* W1, const void* W2, int C, int I, void* tmp, void* wseq, int S = 1);

// depthwise 'same' conv (taps k, dilation dil, weights TRANSPOSED [k][C]) fused with LayerNorm over C.
// x fp32 [B*L][C] -> y act [B*L][C].  C % 4 == 0, C <= 1024.
// seqlen (optional, [B]): frames at t >= seqlen[b] are treated as outside the sequence (zero taps, rows not written) — the
// length-aware mode in which a padded batch reproduces what each sequence would give on its own
// tl (packed rows only, optional): every sequence is the head of a row of tl.T >= L frames whose frames from seqlen[b] on are known without
// being stored — a tap at tt >= seqlen[b] reads tl.tail[min(tl.T - 1 - tt, tl.rf)] (device, [tl.rf + 1][C] fp32, indexed by the distance to
// the end of the row) and zero from tl.T on, instead of zero everywhere.  The same forms, in their tail-reading instantiation.
struct DwconvTail {
    const float* tail = nullptr;
    int T = 0, rf = 0;
};
void launch_dwconv_ln(hipStream_t s, int out_dtype, const float* x, int B, int L, int C, const float* w_t,
                      const float* bias, int k, int dil, const float* ln_g, const float* ln_b, float eps, void* y,
                      const int* seqlen = nullptr, const int* row_off = nullptr, const DwconvTail& tl = DwconvTail());
// The form a depthwise-conv + LayerNorm call takes — one decision, made by dwconv_ln_form and executed by launch_dwconv_ln, so that what
// the diagnostics report (stn_dbg_dwconv_ln_form, stn_op_dwconv_ln_ex) is what runs:
//   DW_V3       dwconv_ln_v3_kernel<OutT, K, R> (C <= 512, k in {5, 7}): combs of R frames; occ4: dwconv_ln_v3_occ4_kernel (k = 7, R = 4, not IEEE half);
//               with a DwconvTail their tail-reading twins dwconv_ln_v3_tail_kernel / dwconv_ln_v3_tail_occ4_kernel (same form string)
//   DW_V2       dwconv_ln_v2_kernel<OutT, K, 2> (padded rows, fewer than 4096 of them)
//   DW_GENERIC  dwconv_ln_kernel<OutT, true> (C > 512 or another tap count; padded rows only)
enum DwconvLnKernel : int { DW_V3 = 0, DW_V2 = 1, DW_GENERIC = 2 };
struct DwconvLnForm {
    int out_dtype = F32;
    int kernel = DW_GENERIC;
    int K = 0, R = 1;
    bool occ4 = false;
    std::string str() const;  // "v3<5,2>", "v3occ4<7,4>", "v2<7>", "generic"
};
// packed: rows packed per sequence (row_off given).  Throws std::invalid_argument where the launcher refuses: C % 4, C > 1024, packed with
// C > 512 or k outside {5, 7}.
DwconvLnForm dwconv_ln_form(int out_dtype, int B, int L, int C, int k, bool packed);
// Packed ("ragged") rows: sequence b owns rows row_off[b] .. row_off[b] + len[b] of x / y and nothing else — no padding rows
// exist.  row_off has B+1 entries (launch_row_map); supported where dwconv_ln_supports_packed(C, k).
bool dwconv_ln_supports_packed(int C, int k);
void launch_row_map(hipStream_t s, const int* len, int B, int* row_off /*[B+1]*/, int* row_b /*[sum len] or null*/,
                    int rows_padded = 0 /* row_b has this many entries: those behind sum len are set to sequence 0 (shape buckets) */);
// the LayerNorm kernels (dwconv_ln_kernel, fold_ln_kernel) hold a row as LN_NI float4 slots per lane: C <= 4 * 64 * LN_NI = 1024
constexpr int LN_NI = 4;
void check_ln_shape(int C);  // throws std::invalid_argument unless C % 4 == 0 and C <= 1024
// plain LayerNorm over C: x fp32 -> y act
void launch_layernorm(hipStream_t s, int out_dtype, const float* x, int64_t M, int C, const float* g, const float* b,
                      float eps, void* y);

// The form an attention call takes — one decision, made by attn_form and executed by launch_attention, so that what the diagnostics
// report (stn_dbg_attn_form, stn_op_attention_ex) is what runs:
//   mfma    attn_mfma_kernel<dh, F16> (16-bit, dh in {32, 64, 96}, ld % 8 == 0, 16-byte aligned q / k / v, operands < 2 GiB): keys
//           through LDS in chunks of kc (a multiple of 32, <= 128), nch chunks at the longest context Lk
//   scalar  attn_kernel<T, tpr> (everything else): tpr = 32 threads per query row when the grid has fewer than 96 workgroups of 32
//           query rows, else 8; fp32 only: vec says which operands are staged with 16-byte loads (ATTN_VEC_*), the others element-wise
enum AttnVec : int { ATTN_VEC_Q = 1, ATTN_VEC_K = 2, ATTN_VEC_V = 4 };
struct AttnForm {
    int dtype = F32;
    bool mfma = false;
    int dh = 0;
    int kc = 0, nch = 0;   // mfma
    int tpr = 8, vec = 0;  // scalar
    size_t lds = 0;        // dynamic LDS bytes of the launch
    std::string str() const;  // e.g. "mfma<64,bf16> kc128 nch3", "scalar<f32,TPR8> vec", "scalar<f32,TPR32> elem", "scalar<bf16,TPR32>"
};
// q / k / v are read for their alignment only (null is aligned).  Throws std::invalid_argument on a head dim the kernels do not take.
AttnForm attn_form(int dtype, int B, int Lq, int Lk, int H, int dh, int ldq, int ldk, const void* q, const void* k, const void* v);
// fused attention core: softmax(rope(q) rope(k)^T / sqrt(dh)) v, per (b, head).
// q [B*Lq][ldq], k/v [B*Lk][ldk] (act dtype); o [B*Lq][ldo] (act dtype).
// rope_mode: -1 none, 0 position index, 1 length-aware (gamma * t / len).
// k_rotated: the keys already carry their rotation (launch_rope_rows ran on them once) — only q is rotated here.
void launch_attention(hipStream_t s, int dtype, const void* q, int ldq, const void* k, const void* v, int ldk, void* o,
                      int ldo, int B, int Lq, int Lk, int H, int dh, const int* qlen, const int* klen, int rope_mode,
                      float rope_base, float rope_gamma, bool k_rotated = false,
                      const int* q_off = nullptr /* packed query/output rows: sequence b starts at q_off[b], owns qlen[b] */,
                      const int* k_off = nullptr /* packed key/value rows: sequence b starts at k_off[b], owns klen[b] */);
// [N][K] row-major 16-bit -> MFMA fragment order (one contiguous KiB per operand; kernels_ffn.hip), once at model load
void launch_repack_frag(hipStream_t s, const void* W, int N, int K, void* Wf);
// One launch per cross-attention block of the vector estimator, HEAD-SPLIT (kernels_xattn_hs.hip): one launch computes, per head h, q_h = Wq_h . xn + bq_h, its rotation, the attention
// over the given K / V and the head's share of the output projection, and stores it as a 16-bit partial sum part[h][row][:] in K4-split's
// layout; x <- x + ((p0 + p1) + p2) + p3 + bo is applied by the next reader of x through FoldArgs{part, S = 4, b2 = bo} (launch_fold_dwconv_ln
// / launch_fold_ln).  xn = LayerNorm(x) rows (16-bit, [M][C]); WqF = launch_repack_frag(Wq), WoA = launch_repack_frag_acc(Wo), both [C][C];
// packed query rows (q_off, qlen) only; keys already rotated when rope_mode >= 0.  ts: optional 8 shader-clock stamps per workgroup.
bool xattn_hs_supported(int dtype, int C, int H, int L, int Lk, int ldk);
void launch_xattn_hs(hipStream_t s, int dtype, const void* xn, int64_t M, const void* WqF, const float* bq, const void* kp, const void* vp, int ldk,
                     const void* WoA, void* part, int64_t part_stride, int B, int L, int Lk, const int* qlen, const int* klen,
                     const int* q_off, const int* k_off, int rope_mode, float rope_base, float rope_gamma, unsigned long long* ts = nullptr,
                     const int* pairs = nullptr /* launch_xattn_hs_pairs' table: which two utterances share a workgroup (null: 2g, 2g + 1) */);
// The form a head-split launch takes (decided by xattn_hs_form, executed by launch_xattn_hs): xattn_hs_kernel<F16, U> with U utterances
// per workgroup (1 or 2), keys in slots of kc = Lk rounded up to 32.  Throws std::invalid_argument where !xattn_hs_supported.
struct XattnHsForm {
    bool f16 = false;
    int U = 1, kc = 32;
    size_t lds = 0;
    std::string str() const;  // e.g. "xattn_hs<f16,U2> kc64"
};
XattnHsForm xattn_hs_form(int dtype, int C, int H, int B, int L, int Lk, int ldk);
// the pairing for U = 2: sorted by length, longest with shortest, so that the pairs' row-tile counts are as equal as the batch allows
// (pairs: 2 * ceil(B / 2) ints; once per synthesis, the lengths do not change)
void launch_xattn_hs_pairs(hipStream_t s, const int* qlen, int B, int* pairs);
// in-place RoPE of `groups` key blocks per row: element (row b*L+t, column g*group_stride + h*dh + i) for t < len[b]
// (len null: all rows).  Keys that are reused by many attention launches (the vector estimator's text keys: every
// block of every Euler step) are rotated once here instead of at every launch.  Same arithmetic as the attention
// kernels' staging (fp32 rotation, one rounding to the storage dtype).
void launch_rope_rows(hipStream_t s, int dtype, void* x, int ld, int B, int L, const int* len, int groups, int group_stride,
                      int H, int dh, int rope_mode, float rope_base, float rope_gamma, const int* row_off = nullptr /* packed rows */);

// embedding gather: x[b*L+t][:] = (t < len[b] && 0 <= id < vocab) ? emb[id][:] : 0     (fp32 out)
void launch_embed(hipStream_t s, const int64_t* ids, const float* emb, int vocab, int B, int L, int C, const int* len,
                  float* x, const int* row_off = nullptr /* packed destination rows */);
// prefix mask [B][L] (float) -> len[B] (count of entries > 0.5)
void launch_mask_to_len(hipStream_t s, const float* mask, int B, int L, int* len);
// [B][C][L] fp32 -> rows [B*L][ld_out] act (columns C..ld_out-1 are zero-filled: K padding for the GEMM that follows)
void launch_ncl_to_rows(hipStream_t s, int out_dtype, const float* in, int B, int C, int L, void* out, int ld_out = 0,
                        const int* len = nullptr, const int* row_off = nullptr /* packed destination rows */);
// Euler update with the [B*L][D] -> [B][D][L] transpose: out[b][d][t] = t < len[b] ? prev[b][d][t] + v[(b*L+t)*D + d] * dt[b] : 0
// z_rows (optional): the new latent also as rows [row][ldz] in `z_dtype` (columns < D only; the K padding beyond stays as the caller zeroed it) — what
// launch_ncl_to_rows(out) would write, so that the next step's input projection needs no such launch
void launch_euler_ncl(hipStream_t s, const float* prev, const float* v, const float* dt, const int* len, int B, int D, int L, float* out,
                      const int* row_off = nullptr /* v in packed rows */, void* z_rows = nullptr, int z_dtype = 0, int ldz = 0);
// fp32 -> act dtype copy (n elements)
void launch_cast(hipStream_t s, int out_dtype, const float* in, int64_t n, void* out);
// x[b*L+t][c] += v[b*ldv + c] for t < len[b]
void launch_add_rowvec(hipStream_t s, float* x, const float* v, int ldv, int B, int L, int C, const int* len);
// time embedding: te[b][:] = [sin(t*f_i), cos(t*f_i)], t = cur[b]/tot[b]*scale
void launch_time_embed(hipStream_t s, const float* cur, const float* tot, int B, int dim, float scale, float* te);
// vocoder front: un-compress [B,D,L] -> frames [B*T][ld] and conv1d ld->C (kernel k, 'same'), fp32 out
void launch_scale_len(hipStream_t s, const int* len, int B, int factor, int* out);  // out[b] = len[b] * factor
void launch_vocoder_in(hipStream_t s, const float* latent, int B, int L, int ld, int ccf, const float* w /*[C][ld][k]*/,
                       const float* bias, int C, int k, float* x, const int* seqlen = nullptr);
// vocoder front as im2col for the MFMA path: cols[r][ci*k + j] = frame(t + j - k/2)[ci] (0 outside the sequence / beyond ld*k),
// frame (b, t = l*ccf + q) channel c <- latent[b][q*ld + c][l]; row stride kp (>= ld*k, zero padded), act dtype
void launch_vocoder_im2col(hipStream_t s, int out_dtype, const float* latent, int B, int L, int ld, int ccf, int k, int kp, void* cols,
                           const int* seqlen = nullptr /* valid vocoder frames per sequence */,
                           const int* row_off = nullptr /* packed destination rows (needs seqlen) */);
// packed rows [sum len][W] -> padded [B][T][W], zeros past each sequence's length
// The rows of a padded [B][T][W] fp32 destination that a packed-row GEMM with a destination map (Epilogue::map_off) does not store: row t of
// sequence b for t >= valid[b].  quiet != null: the dense vocoder's position-independent rest of the row, as launch_unpack_rows_quiet decides
// it — edge[t - (T - rf)] for t >= T - rf, quiet otherwise (quiet [W], edge [rf][W]); quiet == null: zeros (the length-aware form).  Rows below
// valid[b] are not touched.  W % 4 == 0.
void launch_fill_rows(hipStream_t s, const int* valid, int B, int T, int W, int rf, const float* quiet, const float* edge, float* dst);
void launch_unpack_rows(hipStream_t s, const float* src, const int* len, const int* row_off, int B, int T, int W, float* dst);
// exact trimmed dense vocoder (see kernels_layout.hip): extents per utterance, and the unpack that fills the position-independent tail
void launch_trim_len(hipStream_t s, const int* len, int B, int ccf, int T, int rf, int* n_out, int* valid_out, bool tail_form = false);
void launch_unpack_rows_quiet(hipStream_t s, const float* src, const int* valid, const int* row_off, int B, int T, int W, int rf,
                              const float* quiet, const float* edge, float* dst);
// masked mean over valid rows: pooled[b][c] = sum_{t<len[b]} x[b*L+t][c] / max(len[b],1)   (x act dtype, out fp32)
void launch_masked_mean(hipStream_t s, int in_dtype, const void* x, int B, int L, int C, const int* len, float* pooled,
                        const int* row_off = nullptr /* packed source rows */);
// y = softplus(x) elementwise (n small)
void launch_softplus(hipStream_t s, float* x, int n);
// durations: d[b] = (override ? override[b] : d[b]) / speed ; computes per-b latent length; see engine
void launch_scale(hipStream_t s, float* x, int n, float mul);
// Philox4x32-10 + Box-Muller noise, masked: xt[b][d][t] = t < len[b] ? N(0,1) : 0
void launch_randn_masked(hipStream_t s, uint64_t seed, const int64_t* utt_ids, int B, int D, int L, const int* len,
                         float* xt, const unsigned long long* seed_dev = nullptr /* read the seed from device memory (graph replay) */);
// xt[b][d][t] *= (t < len[b])
void launch_mask_ncl(hipStream_t s, float* x, int B, int D, int L, const int* len);
// out[i] = 1 / in[i]
void launch_reciprocal(hipStream_t s, const float* in, int n, float* out);
// bf16 / f16 -> fp32 copy (tests)
void launch_bf16_to_f32(hipStream_t s, const uint16_t* in, int64_t n, float* out);
void launch_half_to_f32(hipStream_t s, int in_dtype, const void* in, int64_t n, float* out);
// total_step/current_step helper: fill n floats
void launch_fill(hipStream_t s, float* x, int n, float v);
void launch_step_counters(hipStream_t s, float* tot /*[steps][B]*/, float* cur /*[steps][B]*/, float* dt /*[B]*/, int B, int steps);
// Sample encodings of a fetch (the values of STN_ENC_*, include/stn.h) and their bytes per sample.  The rules are
// the device functions of kernels_dev.hpp (pcm16, pcm24, mulaw8, alaw8, enc_store1).
enum OutEnc : int { ENC_F32 = 0, ENC_PCM16 = 1, ENC_PCM24 = 2, ENC_MULAW = 3, ENC_ALAW = 4 };
constexpr int enc_bytes(int enc) {
    return enc == ENC_F32 ? 4 : enc == ENC_PCM16 ? 2 : enc == ENC_PCM24 ? 3 : (enc == ENC_MULAW || enc == ENC_ALAW) ? 1 : 0;
}
// An encoding as a template argument: calls fn with std::integral_constant<int, ENC_*>; any other value throws "<who>: unknown encoding <n>".
// In the callee: constexpr int kEnc = decltype(tag)::value.
template <typename Fn>
inline void with_enc(int enc, const char* who, Fn&& fn) {
    switch (enc) {
        case ENC_F32: fn(std::integral_constant<int, ENC_F32>{}); break;
        case ENC_PCM16: fn(std::integral_constant<int, ENC_PCM16>{}); break;
        case ENC_PCM24: fn(std::integral_constant<int, ENC_PCM24>{}); break;
        case ENC_MULAW: fn(std::integral_constant<int, ENC_MULAW>{}); break;
        case ENC_ALAW: fn(std::integral_constant<int, ENC_ALAW>{}); break;
        default: throw std::invalid_argument(std::string(who) + ": unknown encoding " + std::to_string(enc));
    }
}
// The final store of every fetch (the output stage, engine_batch.cpp): rows x W fp32 (row stride W), times g[row] when g (device [rows])
// is not null, to y + row * dst_stride samples (dst_stride >= W) in encoding enc: fp32, int16 PCM by writeWavFile's rule (pcm16,
// kernels_dev.hpp: int16(clamp(v, -1, 1) * 32767), truncation, cpp/helper.cpp:986-987), 24-bit PCM, or G.711 mu-law / A-law of the
// 16-bit sample.  fp32 rows may be stored in place (y == x, dst_stride == W).
// Dither (the rule is dither.hpp's): with a mode set and enc 16- or 24-bit PCM, sample n of row r is quantized with
// the dither of stream (kind, ids ? ids[r] : r) at index n, all W samples of every row (the kernel knows no lengths).  Every other
// encoding, and the mode off, launch the kernels that run without it.  W <= 2^34 then.  lim (the store only; the join has its programmes'
// lengths): row r's stream ends at lim[r * lim_stride], and at and behind it the store writes the zero codeword.
struct Dither {
    int mode = DITHER_OFF; uint64_t seed = 0; unsigned kind = DITHER_ROW; const int64_t* ids = nullptr;
    const int64_t* lim = nullptr; int64_t lim_stride = 1;
};
void launch_store_rows(hipStream_t s, const float* x, int64_t rows, int64_t W, const float* g, int enc, void* y, int64_t dst_stride, const Dither& d = {});
// The join of a fetch: G programme rows of Wj samples at y + p * dst_stride samples (dst_stride >= Wj) in encoding
// enc.  Programme p is members prog[p].first .. + prog[p].count of seg, in order: member m's first seg[m].len samples of source row
// seg[m].row (fp32, rows src_stride apart, len <= src_stride), times g[seg[m].row] when g is not null, at output samples seg[m].dst ..;
// the segments of a programme ascend and do not overlap, and end at or before prog[p].len <= Wj.  Every other sample of [0, Wj) is the
// zero codeword.  Tables on the device.  G <= 65535.  Dither d: programme p's stream is (d.kind, d.ids ? d.ids[p] : p) over its samples
// [0, prog[p].len), the gaps between members included; at and behind prog[p].len the zero codeword stays.
struct JoinSeg { int64_t dst, len, row; };
struct JoinProg { int64_t len; int32_t first, count; };
void launch_join_rows(hipStream_t s, const float* x, int64_t src_stride, const JoinSeg* seg, const JoinProg* prog, int G, int64_t Wj, const float* g,
                      int enc, void* y, int64_t dst_stride, const Dither& d = {});
// The same join from trimmed sources: member m is the seg[m].len samples of source row seg[m].row from sample
// seg[m].src on; its first seg[m].fin delivered samples are times fade[q], its last seg[m].fout times fade[len - 1 - q] (q the sample's
// place in the segment; fade on the device, at least max(fin, fout) floats; both 0: no sample changes).  A delivered sample is
// ((x * g) * w_in) * w_out, three fp32 multiplies in that order, each only where it applies.  The per-row trimmed fetch is this with one
// member per programme (the tables launch_edges_rows writes).
struct JoinSegT { int64_t dst, len, row, src; int32_t fin, fout; };
void launch_join_trim_rows(hipStream_t s, const float* x, int64_t src_stride, const JoinSegT* seg, const JoinProg* prog, int G, int64_t Wj,
                           const float* g, const float* fade, int enc, void* y, int64_t dst_stride, const Dither& d = {});

// Silence edges of the finished waveform by level (kernels_edges.hip; the setting and the caches are engine_edges.cpp; DESIGN.md section
// 14).  Frames of F = edges_frame(hz) samples (10 ms) from sample 0 without overlap, level = mean of x^2 over the frame's own samples;
// a frame is active at or above max level * 10^(-top_db / 10); a row whose max level is <= 1e-7, or that is empty, keeps [0, n).
constexpr int ED_CHUNK = 32;          // samples per lane of the frame pass
constexpr int ED_WG = 256;            // lanes (chunks) per workgroup of the frame pass
__host__ __device__ inline int64_t ed_chunks(int64_t W) { return (W + ED_CHUNK - 1) / ED_CHUNK; }
inline int edges_frame(int hz) { return (hz + 50) / 100; }
inline int64_t edges_frames(int64_t W, int hz) { const int F = edges_frame(hz); return (W + F - 1) / F; }
// rows x W fp32 (row stride W) with row lengths n[rows] (device, <= W) -> edges[row] = {start, end} with
// start = max(0, f0 * F - keep), end = min(n, (f1 + 1) * F + keep) over the first and last active frame.  Scratch (device): pa, pb
// [rows][ed_chunks(W)] floats, lev [rows][edges_frames(W, hz)] doubles (the levels, left there).  seg / prog (both or neither): the
// per-row programmes {dst 0, len, row, src = start, fin / fout = min(fd, len) where that edge was cut} and {len, row, 1}.
// Two launches, the hand-off between them a launch boundary: the frame pass (x -> pa, pb) and the row pass (pa, pb -> lev, edges, seg, prog).
void launch_edges_frames(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, int hz, float* pa, float* pb);
void launch_edges_rows(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, int hz, double top_db, int64_t keep, int64_t fd, const float* pa,
                       const float* pb, double* lev, int64_t* edges, JoinSegT* seg, JoinProg* prog);
// The pause limit, behind launch_edges_rows on the same stream: lev and edges as that launch left them -> row r's
// segments seg[r * S .. r * S + count) (the row's [start, end) without the middle of every pause longer than Mp samples, at most S - 1
// cuts, the first in time order), prog[r] = {len_r, r * S, count} and cuts[r][2 S] = {count - 1, len_r, lo_0, hi_0, lo_1, ...}.
// 1 <= S <= 256.
constexpr int PZ_MAX_CUTS = 255;
void launch_pause_rows(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, int hz, double top_db, int64_t fd, int64_t Mp, int S, const double* lev,
                       const int64_t* edges, JoinSegT* seg, JoinProg* prog, int64_t* cuts);

// Output-rate resampling of the finished waveform (kernels_resample.hip; the filter design is engine_resample.cpp).  Rational polyphase:
// out_hz / in_hz = P / Q reduced; output n of a row = sum_j taps[(n*Q) mod P][j] * x[floor(n*Q/P) - off + j] (x = 0 outside the row),
// W_out = ceil(W * P / Q).  Supported: in and out rates in [8000, 192000] Hz with P <= 640.
struct ResampleTable {
    int in_hz = 0, out_hz = 0;
    int P = 0, Q = 0, T = 0, off = 0;  // T: taps per phase (a multiple of 8); off: taps ahead of the centre tap
    std::vector<float> taps;            // host copy, [P][T]
    float* dev = nullptr;               // device copy (not owned: the engine keeps the block, a DeviceTable, beside the table)
};
constexpr int RESAMPLE_MIN_HZ = 8000, RESAMPLE_MAX_HZ = 192000, RESAMPLE_MAX_P = 640;
inline int64_t resample_out_len(int64_t W, int P, int Q) { return (W * P + Q - 1) / Q; }
// Kaiser-windowed sinc for the pair (host only): fills f (not f.dev).  Empty string on success, else why the pair is refused.
std::string resample_design(int in_hz, int out_hz, ResampleTable& f);
// The design's arithmetic for the reduced pair P / Q, with the two rates it is stated in (in_hz = Q g, out_hz = P g for one g): what
// resample_design runs behind its checks of the rates, and what the pitch shift (section 24) designs its a / b table with
void resample_design_pq(int P, int Q, int in_hz, int out_hz, ResampleTable& f);
double bessel_i0(double x);  // the Kaiser window's shape (engine_resample.cpp)
// rows x W fp32 (row stride W) -> rows x W_out at y + row * dst_stride samples (dst_stride >= W_out) in encoding enc (the encoded
// bytes are those of the fp32 output followed by launch_store_rows without a gain)
// cap > 0: only the first min(cap, W_out) samples of a row are stored (dst_stride >= that); every stored sample is what it is without a cap
void launch_resample(hipStream_t s, const float* x, int64_t rows, int64_t W, const ResampleTable& f, int enc, void* y, int64_t dst_stride, int64_t cap = 0);
// The form a resample call takes — one decision, made by resample_form (host only: P, Q and T of f) and executed by launch_resample, so
// that what the diagnostics report (stn_dbg_resample_form) is what runs.  A workgroup owns G * 64 consecutive k of a row (output
// n = k * P + r) and every r; G doubles from 1 while G * P < 16 (the waves have pairs to walk), G * 64 < K (the row has the k) and the
// span of 2 G groups fits in 160 KiB of LDS; a span of G groups above 160 KiB reads the row through the caches.
struct ResampleForm {
    int G = 1;
    bool lds = true;        // the span is staged in LDS (else read through the caches)
    int64_t lds_bytes = 0;  // dynamic LDS of the launch (0 on the cache path)
    int64_t grid_x = 0;     // workgroups per row
    std::string str() const;  // "resample lds G4", "resample cache G1"
};
ResampleForm resample_form(int64_t W, const ResampleTable& f);  // throws std::invalid_argument for W < 1 or a table without a design

// Time-scale modification of the finished waveform (kernels_pitch.hip; the geometry is host/pitch.cpp, the rule DESIGN.md section 24):
// WSOLA with a normalised search.  rows x W fp32 (row stride W), row r's span n[r] (device, clamped to [0, W]; null: W), hop H (a power
// of two in [64, 2048]), stretched by a / b over M = ceil(W a / b) / H + 2 frames.  launch_pitch_search: one workgroup per row walks its
// frames and writes delta [rows][M] (the offsets, delta[.][0] = 0) and score [rows][M] (the winners' scores, 0 for frame 0).
// launch_pitch_ola: y [rows][Ws], Ws = ceil(W a / b), the overlap-add of the grains at those offsets under win (device, 2 H floats: the
// periodic Hann of pitch_window), 0.0f from the row's stretched span ceil(n a / b) on.  A read outside a row's span is 0.0f.
void launch_pitch_search(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, int H, int64_t M, int a, int b, int* delta, float* score);
void launch_pitch_ola(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, int H, int64_t M, int64_t Ws, int a, int b, const int* delta,
                      const float* win, float* y);

// Formant correction of pitch-shifted rows (kernels_formant.hip; the geometry and the recursion's host statement are host/formant.cpp,
// the rule DESIGN.md section 26).  x: the rows before the shift, y: the shifted rows, both rows x W fp32 with spans n as above; hop H,
// frames F = ceil(W / H) + 1 of N = 2 H samples, order p in [1, 48].  launch_formant_lpc: per (row, frame) the LPC polynomials of x and
// y under win (device, 2 H floats) and lagw (device, p + 1 doubles) -> ax and cy = g a_y [rows][F][p + 1] fp32, g, ex and ey [rows][F]
// double.  launch_formant_filter: out [rows][W], the cross-faded outputs of g A_y / A_x per frame from zero state N samples ahead of
// the frame, 0.0f from the row's span on.
void launch_formant_lpc(hipStream_t s, const float* x, const float* y, int64_t rows, int64_t W, const int64_t* n, int H, int64_t F, int p, const float* win,
                        const double* lagw, float* ax, float* cy, double* g, double* ex, double* ey);
void launch_formant_filter(hipStream_t s, const float* y, int64_t rows, int64_t W, const int64_t* n, int H, int64_t F, int p, const float* win,
                           const float* ax, const float* cy, float* out);

// Loudness normalization of the finished waveform (kernels_loudness.hip; the filter design and the measurement are engine_loudness.cpp).
// BS.1770-4 integrated loudness of row b's first n_b samples: K-weighting (shelf then high-pass biquad, transposed direct form II in
// fp32) as one 4-state linear system x' = A x + B u.  Chunks of LO_CHUNK samples from sample 0: each is filtered from zero state
// (end state e_k, max |x|), a per-row scan gives the true start states s_{k+1} = M s_k + e_k with M = A^LO_CHUNK, each chunk is
// refiltered from s_k into per-chunk sums of y^2 split at the 100 ms segment boundary, and one workgroup per row gates the 400 ms blocks
// and writes (L_b, peak_b, g_b).  Every hand-off is a launch boundary; every sum runs in a fixed order.
constexpr int LO_CHUNK = 32;          // samples per lane
constexpr int LO_WG = 256;            // lanes (chunks) per workgroup of the two chunk passes
constexpr int LO_SCAN = 1024;         // chunks per scan tile; the power table holds M^1 .. M^LO_SCAN
constexpr int LO_MAX_SEG = 16384;     // 100 ms segments per row the gate holds in LDS
constexpr int LO_MIN_HZ = 8000, LO_MAX_HZ = 192000;
struct KWeighting { double shelf_b[3], shelf_a[3], hp_b[3], hp_a[3]; };  // a[0] = 1
// the BS.1770-4 K-weighting filter at hz (host only, libebur128's analog-prototype derivation); empty string, or why hz is refused
std::string kweighting_design(int hz, KWeighting& k);
struct LoudCoef { float c[10]; };     // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (fp32, what the kernels multiply by)
struct LoudTable {
    int hz = 0, hop = 0;              // hop = (hz + 5) / 10 samples (100 ms)
    LoudCoef coef{};
    std::vector<double> mpow;         // host copy, [LO_SCAN][16]: M^(i+1) row-major, M = A^LO_CHUNK of the fp32 coefficients
    double* dev = nullptr;            // device copy (not owned: the engine keeps the block, a DeviceTable, beside the table)
};
// fills t (not t.dev); empty string, or why hz is refused
std::string loudness_design(int hz, LoudTable& t);
__host__ __device__ inline int64_t lo_chunks(int64_t W) { return (W + LO_CHUNK - 1) / LO_CHUNK; }
// Pass 1 (energy = false): rows x W fp32 (row stride W) with row lengths n[rows] (<= W) -> st[row][k] = end state of chunk k from zero
// state, pk[row][k] = max |x| over chunk k.  Pass 2 (energy = true): st[row][k] = start state of chunk k -> pa/pb[row][k] = sum of y^2
// over the chunk's samples in its first 100 ms segment / in the next one, counting only whole segments.  Ks = lo_chunks(W).
void launch_loudness_chunks(hipStream_t s, bool energy, const float* x, int64_t rows, int64_t W, const int64_t* n, const LoudTable& t,
                            float* st, float* pk, float* pa, float* pb);
// in place: st[row][k] (end states) -> the start states of the chunks
void launch_loudness_scan(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, const LoudTable& t, float* st);
// res[0][b] = L_b (-inf when undefined), res[1][b] = peak_b, res[2][b] = g_b (1 when off or L_b undefined); max_seg = max_b n_b / hop
void launch_loudness_gate(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, const LoudTable& t, const float* pk, const float* pa,
                          const float* pb, int64_t max_seg, bool on, float target_lufs, float ceiling_dbfs, float* res);
// (the gain itself is applied by launch_store_rows with g = res + 2 * rows)
// The loudness report on the pa / pb the energy pass left: res[0][b] = maximum momentary loudness, res[1][b] =
// maximum short-term loudness (-inf without a block / a window), res[2][b] = loudness range, nst[b] = the 3 s windows behind both
// gates.  The rule is host/loudness_range.hpp's.  The kernel holds a row's segments and its window powers in LDS side by side, so it
// takes LR_MAX_SEG segments per row where the gate takes LO_MAX_SEG; beyond that std::invalid_argument names the cap.
constexpr int LR_MAX_SEG = 8192;      // 100 ms segments per row (13 min 39 s); a power of two
std::string loudness_range_check(int64_t max_seg);  // why rows of up to max_seg segments are refused (it names the cap), or ""
void launch_loudness_range(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, const LoudTable& t, const float* pa, const float* pb,
                           int64_t max_seg, float* res, int32_t* nst);
// The pitch report (kernels_f0.hip; the geometry is host/f0.hpp, the host side engine_f0.cpp; include/stn.h "f0"; DESIGN.md section
// 27): YIN on rows x W fp32 with row spans n[rows] (device).  The track kernel gives a workgroup F0_GROUP consecutive frames of one
// row: it box-averages and stages their samples in LDS once, a lane owns one (frame, lag) of the difference function, and one wave per
// frame scans, decides and refines.  The stats kernel is one workgroup per row over the row's track.  Fixed-order sums, no atomics.
constexpr int F0_GROUP = 8;           // frames per workgroup of the track kernel
constexpr int F0_WG = 256;            // its threads: four waves, each owning every fourth frame of the group
constexpr int F0_STATS_WG = 1024;     // threads of the stats workgroup
constexpr int F0_MAX_FRAMES = 32768;  // frames per row the stats kernel sorts in LDS (fp32 keys: 128 KiB of the 160 KiB); a power of two
constexpr int F0_MAX_TAU = 1067;      // ceil(32000 / 30): the longest lag the parameter limits allow
struct F0Launch {
    int k = 1, hop = 0, tau_min = 0, tau_max = 0;  // host/f0.hpp's geometry
    float threshold = 0.f;
    double ha = 0.0, gate_ms = 0.0;
};
std::string f0_frames_check(int64_t row, int64_t frames);  // why a row of `frames` frames is refused (it names the count and the cap), or ""
// f0, ap [rows][fstride]: row r's frames in columns 0 .. F_r - 1 (F_r from n[r] by the contract), f0 = 0 and ap = 1 behind them up to
// max_frames (the longest row's count, <= fstride); nothing is read behind n[r]
void launch_f0_track(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, const F0Launch& g, int64_t max_frames, int64_t fstride,
                     float* f0, float* ap);
// stats [rows] (stn_f0_stats: frames, voiced, median, geometric mean, min, max) of the tracks f0 [rows][fstride]
void launch_f0_stats(hipStream_t s, const float* f0, int64_t rows, int64_t W, const int64_t* n, const F0Launch& g, int64_t max_frames, int64_t fstride,
                     void* stats);

// the powers M^1 .. M^LO_SCAN ([LO_SCAN][16], double) of M = A^LO_CHUNK for the two-section cascade with the fp32 coefficients c
// (b0 b1 b2 a1 a2 twice): what the scan reads, for the K-weighting and for a section pass of the filter chain alike (host only)
void cascade_powers(const LoudCoef& c, std::vector<double>& mpow);

// Fetch-time biquad chain (kernels_filter.hip; the designer, the tables and the section passes are engine_filter.cpp; DESIGN.md section
// 18).  A section pass is two biquads as the 4-state system above, every row W long: launch_loudness_chunks (energy = false) and
// launch_loudness_scan on a LoudTable of the section's coefficients and powers (hop = 1, unused), then this launch, which refilters
// every chunk from its start state st[row][k] and writes y (row stride W, as x).  y may be x: a workgroup reads its LO_WG * LO_CHUNK
// samples before it stores any, and touches no other workgroup's.
void launch_filter_write(hipStream_t s, const float* x, int64_t rows, int64_t W, const LoudTable& t, const float* st, float* y);

// The three fetch-time dynamics stages (kernels_dynamics.hip: one chunk kernel over a stage policy, one scan, one row reduction; the
// limits and the tables are engine_<stage>.cpp, the sequence of launches Engine::dyn_enqueue; DESIGN.md sections 20, 20a, 21, 25).  Every
// row W long, chunks of LO_CHUNK samples from sample 0, workgroups of LO_WG chunks, scan tiles of LO_SCAN.  A stage's three chunk passes:
// pass 1: s1[row][k] = the detector at the end of chunk k from zero.  pass 2: s1 = the detector at the chunk's start -> s2[row][k] = yL
// at its end from zero.  pass 3: s1, s2 = the start values -> y (row stride W; may be x), the per-sample taps (rows x W, or null) and
// the per-chunk results over the chunk's samples below n[row] (device; null: W).  The staging form of all three is that of (x, y, W)
// (chunk_staging_form, kernels_chunk.hpp).
// The scan between them, for every stage whose chunks compose by one of these (pw: LO_SCAN doubles on the device): v + P o, max(v, P o)
// and max(v, o - P) (the expander's detector, section 25).  In place: st[row][k] end values from zero -> the chunks' start values; unit
// names the caller in what is refused.  A stage's table names its first scan's combination (comb, on dev[0 .. LO_SCAN)); its second is
// the linear one on dev[LO_SCAN .. 2 LO_SCAN).
enum ScanComb { SCAN_LINEAR = 0, SCAN_MAX_TIMES = 1, SCAN_MAX_PLUS = 2 };
void launch_chunk_scan(hipStream_t s, ScanComb comb, const char* unit, int64_t rows, int64_t W, const double* pw, float* st);

// Compressor: the detector is y1.
struct CompCoef { float T, S, K, kA, kR, makeup; };  // threshold dB, 1 / ratio - 1, knee dB, attack and release k, makeup dB (fp32)
struct CompTable {
    static constexpr ScanComb comb = SCAN_MAX_TIMES;
    int hz = 0;
    CompCoef coef{};
    std::vector<double> pw;           // host copy, [2][LO_SCAN]: D^(i+1) then E^(i+1), D = (1 - kR)^LO_CHUNK, E = (1 - kA)^LO_CHUNK
    double* dev = nullptr;            // device copy (not owned: the engine keeps the block, a DeviceTable, beside the table)
};
// gr: rows x W yL, or null.  cmax[row][k] = max of yL (0 without a valid sample)
void launch_compressor_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const CompTable& t, float* s1,
                              float* s2, float* y, float* gr, float* cmax);
// out[row] = max_k cmax[row][k]
void launch_compressor_rowmax(hipStream_t s, int64_t rows, int64_t W, const float* cmax, float* out);

// Downward expander / noise gate: the detector is u.
struct ExpCoef { float T, S, K, R, kA, delta, Bh; };  // threshold dB, ratio - 1, knee dB, range dB, attack k, release dB per sample, hold boost dB (fp32)
struct ExpTable {
    static constexpr ScanComb comb = SCAN_MAX_PLUS;
    int hz = 0;
    int64_t hold = 0;                 // Hs, the hold in samples
    ExpCoef coef{};
    std::vector<double> pw;           // host copy, [2][LO_SCAN]: (i + 1) LO_CHUNK delta then E^(i+1), E = (1 - kA)^LO_CHUNK
    double* dev = nullptr;            // device copy (not owned: the engine keeps the block, a DeviceTable, beside the table)
};
// open: rows x W yL, or null.  cmin[row][k] = min of R - yL and ccnt[row][k] = count of yL <= R / 2 (R and 0 without a valid sample)
void launch_expander_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const ExpTable& t, float* s1,
                            float* s2, float* y, float* open, float* cmin, int32_t* ccnt);
// omin[row] = min_k cmin[row][k], ocnt[row] = sum_k ccnt[row][k]
void launch_expander_rows(hipStream_t s, int64_t rows, int64_t W, const ExpTable& t, const float* cmin, const int32_t* ccnt, float* omin, int64_t* ocnt);

// De-esser (eight launches): the compressor's detector on the level of a band h = HP4(x), its gain on the band
// (split) or on x (wide).  The band's chunk pass and scan are the loudness measurement's on `band`, the detector's scans run on `det`,
// the row maxima are launch_compressor_rowmax.
struct DeessCoef { LoudCoef band; float T, S, K, kA, kR, range; };  // the two high-pass sections; threshold dB, 1 / ratio - 1, knee dB, k, range dB
struct DeessTable {
    int hz = 0;
    bool split = true;                // mode == STN_DEESS_SPLIT
    DeessCoef coef{};
    LoudTable band;                   // the band's section pass: coefficients and the powers of its M (hop = 1, unused)
    CompTable det;                    // the scans' powers from the same attack and release (makeup 0; its T, S, K are not read)
};
// Every pass regenerates h from x and st[row][k], the band's state at the start of chunk k.  band and gr: rows x W h and yL, or null.
// cmax as the compressor's
void launch_deesser_chunks(hipStream_t s, int pass, const float* x, int64_t rows, int64_t W, const int64_t* n, const DeessTable& t, const float* st,
                           float* s1, float* s2, float* y, float* band, float* gr, float* cmax);

// Look-ahead peak limiter behind the loudness gain (kernels_limiter.hip; the setting, the window and the scratch are engine_limiter.cpp;
// DESIGN.md section 15).  rows x W fp32 (row stride W) with row spans n[rows] (device, <= W) and gains gain[rows] (device; null: 1) ->
// y (rows x W fp32, row stride W, not x): row b times gain[b], turned down around every sample above c so that |y| <= c, the curve s
// smoothed over A + 1 samples by the weights wts (device, A + 1 floats that sum to 1); behind n[b] the clamped product.  s_out (device
// rows x W, or null): the curve.  Scratch (device): pcnt, pmin [rows][lm_tiles(W)].  Results (device [rows]): limited = samples of the
// span whose curve is below 1, red = -20 log10 of the curve's minimum.  Two launches, the hand-off between them a launch boundary: the
// tiles (x -> y, s_out, pcnt, pmin), then the per-row results (pcnt, pmin -> limited, red).
constexpr int LM_WG = 256;            // lanes per workgroup
constexpr int LM_TILE = 2048;         // samples of a row a workgroup owns (8 consecutive ones per lane)
constexpr int LM_MAX_A = 1920;        // 10 ms at 192 kHz
inline int64_t lm_tiles(int64_t W) { return (W + LM_TILE - 1) / LM_TILE; }
// env (device rows x W, or null): the true-peak envelope of the row times its gain (launch_truepeak).  Non-null, r[j] is 1 where
// env[j] <= c and c / env[j] elsewhere (1 outside [0, n)) instead of the sample's own; everything else is unchanged.  Null is the
// kernel without that argument.
void launch_limiter(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, const float* gain, float c, int A, const float* wts,
                    float* y, float* s_out, int* pcnt, float* pmin, const float* env = nullptr);
void launch_limiter_rows(hipStream_t s, int64_t rows, int64_t W, const int* pcnt, const float* pmin, int64_t* limited, float* red);

// True peak by 4x oversampling (kernels_truepeak.hip; the filter design and the consumers are engine_truepeak.cpp; DESIGN.md section 16;
// ITU-R BS.1770-4 Annex 2).  For a row with span n, x = 0 outside [0, n): u[i][ph] = sum_j taps[ph][j] x[i - 7 + j] (an fp32 FMA chain,
// j ascending) is the value at i + ph/4 for ph in {1, 2, 3} and i in [-1, n - 1]; U[i] = max_ph |u[i][ph]|;
// p[i] = max(|x[i]|, U[i-1], U[i]) for i < n and |x[i]| behind; pk[row][k] = max p over chunk k's samples inside the span (+0.0 when
// there are none; chunks of LO_CHUNK samples, the loudness measurement's pk layout).
constexpr int TP_PHASES = 4, TP_TAPS = 16, TP_OFF = 7;
constexpr double TP_BETA = 8.0;
struct TpCoef { float h[TP_PHASES - 1][TP_TAPS]; };  // phases 1..3 (phase 0 is the unit tap: the sample itself)
// all four phases [4][16] as fp32, every phase normalized in double to DC gain 1 (host only; the same taps serve every rate)
void truepeak_design(float* taps64);
TpCoef truepeak_coef();
// rows x W fp32 (row stride W) with spans n[rows] (device, <= W), times gain[row] (device, or null: one fp32 multiply at staging) ->
// pk [rows][lo_chunks(W)] (every entry written) and, when env is not null, env [rows][W] = p (not x)
void launch_truepeak(hipStream_t s, const float* x, int64_t rows, int64_t W, const int64_t* n, const float* gain, float* pk, float* env);
// the staging path launch_truepeak takes: "vec" (16-byte loads and stores: W % 4 == 0, x and env 16-byte aligned) or "scalar"
const char* truepeak_staging_form(const float* x, int64_t W, const float* env);
// tp[row] = max of pk[row][..] over the span's chunks (0 for an empty span); trim[row] (or null) = 1 where tp <= c, else c / tp
void launch_truepeak_rows(hipStream_t s, int64_t rows, int64_t W, const int64_t* n, const float* pk, float c, float* tp, float* trim);

}  // namespace stn
