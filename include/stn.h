/* stn.h — C ABI of the MI355X-native Supertonic synthesis engine (libstn.so).
 *
 * This is the drop-in boundary for the reference's hot path.  Each entry point names the reference
 * interface it replaces; all paths are relative to /root/reference.
 *
 *   reference (ONNX Runtime C++ API)                      here
 *   ------------------------------------------------      -------------------------------------------
 *   Ort::Session ctor x4, loadOnnxAll                     stn_create + stn_load_dir / stn_load_synthetic
 *     cpp/helper.cpp:776-795, loadCfgs :801-818
 *   dp_ort_->Run          cpp/helper.cpp:512-526          stn_duration
 *   text_enc_ort_->Run    cpp/helper.cpp:545-556          stn_text_enc
 *   vector_est_ort_->Run  cpp/helper.cpp:620-658          stn_vector_est   (one Euler step per call)
 *   vocoder_ort_->Run     cpp/helper.cpp:662-679          stn_vocoder
 *   TextToSpeech::_infer  cpp/helper.cpp:469-683          stn_batch_upload + stn_batch_run + stn_batch_fetch
 *   sampleNoisyLatent     cpp/helper.cpp:424-467          inside stn_batch_run (Philox noise, or injected)
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every function returns STN_OK (0) or a
 * negative error code; the message is available from stn_last_error().  Tensors are contiguous,
 * row-major, caller-owned HOST buffers with the names / dtypes / shapes of the ONNX graph I/O
 * (text_ids int64 [B,Lt]; masks float32 [B,1,L]; step counters float32 [B]; everything else float32).
 * One handle = one GPU + one HIP stream; calls on one handle must be serialised by the caller; distinct
 * handles are independent (one per GPU).  There is NO CPU fallback: without a HIP device stn_create fails.
 */
#ifndef STN_H
#define STN_H
#include <stddef.h>
#include <stdint.h>

#include "stn_arch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STN_OK 0
#define STN_ERR_INVALID (-1)      /* bad argument / shape                         */
#define STN_ERR_DEVICE (-2)       /* HIP failure or no device                     */
#define STN_ERR_STATE (-3)        /* call order (no model loaded, no batch, ...)  */
#define STN_ERR_UNSUPPORTED (-4)  /* feature not available in this build          */
#define STN_ERR_IO (-5)           /* file missing / unreadable / malformed        */

#define STN_DTYPE_F32 0   /* fp32 operands, exact fp32 MFMA                        */
#define STN_DTYPE_BF16 1  /* bf16 GEMM operands, fp32 accumulate + fp32 residual   */
#define STN_DTYPE_F16 2   /* IEEE half GEMM operands / activations (v_mfma_f32_32x32x16_f16), fp32 accumulate + fp32 residual:
                           * BASELINE config 5 ("fp16 MFMA linears"); 11 significant bits instead of bf16's 8, range 6.5e4 */

typedef struct stn_handle stn_handle;

typedef struct stn_config {
    int32_t device;  /* HIP device ordinal                                         */
    int32_t dtype;   /* STN_DTYPE_*                                                */
} stn_config;

/* ---- lifetime / model load -------------------------------------------------------------------- */
int stn_create(const stn_config* cfg, stn_handle** out);
int stn_destroy(stn_handle* h);
/* message of the last failure on this handle (or of the last failed stn_create when h == NULL) */
const char* stn_last_error(const stn_handle* h);
/* The reference's asset directory (cpp/helper.cpp:784-823): tts.json + unicode_indexer.json + the four .onnx graphs, nothing else.
 * tts.json gives the descriptor's config fields; the graphs are read by a built-in protobuf reader and their NODES are walked in
 * graph order: the nodes that carry weights (depthwise Conv, pointwise Conv / MatMul+Add / Gemm, LayerNormalization, layer-scale
 * Mul, Gather) are parsed against the engine's layout (embedding / ConvNeXt blocks / attention blocks / projections), which yields
 * the rest of the descriptor (widths, depths, kernel sizes, dilations, head counts from the Reshape constants) and binds every
 * initializer to its canonical tensor by position and role — never by name (csrc/host/graph_bind.hpp; stn_bind_graphs in
 * stn_host.h shows the result without a device).  Graph input/output names must be the ones the hosts use (cpp/helper.cpp:512-513,
 * 545-546, 620-623, 663-664); tts.json must agree with the shapes.  A graph that is not this layout fails with the first node that
 * does not fit, what the layout needs there, and the descriptor derived so far.
 * Optional `<onnx_dir>/stn_weight_map.json` overrides the walk with an explicit table
 *   {"arch": {<stn_arch field>: int, ...}, "tensors": {"<engine tensor>": {"file": "vocoder.onnx", "name": "<initializer>",
 *    "transpose": false}, ...}}   ("transpose" may be omitted: it is inferred from the stored dims, which are checked either way).
 * STN_ERR_IO: a file is missing/unreadable/malformed ("Failed to open ..." as cpp/helper.cpp:805) or does not bind;
 * STN_ERR_INVALID: the derived descriptor is outside what the kernels support (message names the field).
 * After a successful manifest-less load stn_last_error holds notes (e.g. that the graphs spell GELU with Tanh).  A head count the graphs do
 * not carry (no [batch, length, heads, head_dim] Reshape constant) is an ERROR, not a default: state it in a stn_weight_map.json that has only
 * {"arch": {"te_heads": n, "dp_heads": n, "ve_heads": n}} (no "tensors" table: the graphs are still walked).
 * Accepted spellings of the layout: LayerNormalization as one node or decomposed (ReduceMean / Sub / Pow / ReduceMean / Add / Sqrt / Div / Mul /
 * Add), q / k / v projections separate or fused (3C or 2C rows + Split), pointwise convolutions as Conv k=1, MatMul(+Add) with Transposes around it
 * or Gemm, GELU as a node or written with Erf / Tanh, the vocoder's wave head as a projection or as a one-channel ConvTranspose with stride ==
 * kernel == base_chunk_size (an overlapping transposed convolution is another head: refused with the node named).  VERIFIED ON GRAPHS THE TESTS EMIT (tests/onnx_graphs.py), not on the published files, which
 * are not available offline: for real assets the explicit stn_weight_map.json below is the documented path, and the walk says where a graph departs
 * from the layout. */
int stn_load_dir(stn_handle* h, const char* onnx_dir);
/* '\n'-separated names of every canonical tensor the descriptor implies (what a manifest must map); returns bytes needed */
int stn_tensor_names(stn_handle* h, const stn_arch* arch, char* out, size_t cap);
/* descriptor-driven deterministic weights (no asset files needed) */
int stn_load_synthetic(stn_handle* h, const stn_arch* arch, uint64_t seed);
int stn_get_arch(const stn_handle* h, stn_arch* out);
int64_t stn_param_count(const stn_handle* h);

/* ---- the four former Run sites (host pointers in, host pointers out) ------------------------------ */
int stn_duration(stn_handle* h, int B, int Lt, const int64_t* text_ids, const float* style_dp /*[B,e1,e2]*/,
                 const float* text_mask /*[B,1,Lt]*/, float* duration /*[B] seconds*/);
int stn_text_enc(stn_handle* h, int B, int Lt, const int64_t* text_ids, const float* style_ttl /*[B,d1,d2]*/,
                 const float* text_mask, float* text_emb /*[B,Ce,Lt]*/);
int stn_vector_est(stn_handle* h, int B, int L, int Lt, const float* noisy_latent /*[B,D,L]*/,
                   const float* text_emb /*[B,Ce,Lt]*/, const float* style_ttl, const float* text_mask,
                   const float* latent_mask /*[B,1,L]*/, const float* total_step /*[B]*/,
                   const float* current_step /*[B], 0-based*/, float* denoised_latent /*[B,D,L]*/);
int stn_vocoder(stn_handle* h, int B, int L, const float* latent /*[B,D,L]*/, float* wav /*[B, L*cs]*/);

/* ---- fused synthesis: everything stays in HBM between stages ---------------------------------------
 * upload: copies the batch to the GPU (text_ids, text_mask, styles; optional duration override in
 *         seconds BEFORE the /speed division; optional utterance ids that key the noise generator so a
 *         sharded batch draws the same noise as an unsharded one).
 * run:    DP -> /speed -> text encoder -> noise -> total_step x estimator -> vocoder, all on the handle's
 *         stream; returns after ENQUEUE (asynchronous) except for one tiny device->host read of the
 *         durations when no override is given.  Call stn_sync or stn_batch_fetch to wait.
 * fetch:  waits and copies out wav [B, L*cs] and duration [B] (after /speed, as the reference returns). */
int stn_batch_upload(stn_handle* h, int B, int Lt, const int64_t* text_ids, const float* text_mask,
                     const float* style_ttl, const float* style_dp, const float* duration_override_or_null,
                     const int64_t* utt_ids_or_null);
int stn_batch_set_noise(stn_handle* h, const float* noise /*[B,D,L]*/, int L);
int stn_batch_run(stn_handle* h, int total_step, float speed, uint64_t noise_seed);
/* hipGraph replay of the post-duration pipeline (default on): a shape is captured the second time it is run and replayed
 * afterwards.  Up to 8 captured shapes are kept (least recently used out first), so callers that alternate a few shapes — the
 * reference's call() chunk loop and n_test loop, cpp/helper.cpp:697-719, cpp/example_onnx.cpp:88 — replay all of them; loading
 * weights on the handle drops every captured graph.  stn_graph_replays counts replays, stn_graphs_cached the graphs held
 * (tests / diagnostics). */
int stn_set_graph_mode(stn_handle* h, int on);
int64_t stn_graphs_cached(const stn_handle* h);
/* Vocoder treatment of the padding in stn_batch_run.  0 (default) = the reference's batched Run (cpp/helper.cpp:668-679):
 * all L*ccf frames of every utterance are decoded, the padding being zero latent.  1 = length-aware: each utterance's frames
 * end at its own latent length, so wav[b, :len_b] is what a batch-of-one synthesis of utterance b gives — the mode in which
 * the chunks of a long text (TextToSpeech::call, cpp/helper.cpp:685-722, one _infer per chunk) run as ONE batch. */
int stn_set_vocoder_mode(stn_handle* h, int length_aware);
/* Row layout of the vector estimator inside stn_batch_run.  1 (default) = packed: the estimator's activations hold only the
 * latent frames each utterance owns (sum of lengths rows), 0 = padded [b*L + t] rows with the padding masked to zero after
 * every block.  The masked stages are row-independent, so both give the same latent; packed does no work on padding. */
int stn_set_row_layout(stn_handle* h, int packed);
/* Shape buckets for the graph cache (default off).  A captured pipeline has every size baked in: B, Lt, L and the packed row counts.
 * With buckets on, Lt, L and the row counts are rounded UP to bucket boundaries (4-8 per octave, at most 25 % padding), so requests of
 * unlike lengths that fall into the same buckets replay ONE captured graph instead of capturing one each — the case of a service
 * that merges requests (/root/reference/py/service.py:79-136) and of the call() chunk loop (/root/reference/cpp/helper.cpp:697-719).
 * The utterances' own lengths stay exact: every utterance's frames and samples are bit-identical to the unbucketed run.  What the
 * caller sees: stn_batch_dims reports the bucketed L (W = L * chunk samples) and fetched rows have that length (zeros / the dense
 * vocoder's padding response behind an utterance's own samples, as before); B stays exact; injected noise keeps L exact. */
int stn_set_shape_buckets(stn_handle* h, int on);
/* Measurement aid.  stn_batch_upload with a duration override skips the one device->host read of a synthesis (the predicted
 * durations, which size every later buffer): with always != 0 the read and the wait for it are performed anyway, so a timed run has
 * the critical path of a predicted-duration run (duration predictor -> read -> rest) on the controlled shapes of a forced one. */
int stn_set_duration_read(stn_handle* h, int always);
/* GELU form of the loaded model: 0 = erf (default), 1 = the tanh approximation 0.5 x (1 + tanh(sqrt(2/pi)(x + 0.044715 x^3))).
 * stn_load_dir sets it from how the graphs spell the activation (Gelu / Erf: 0; Tanh inside the GELU pattern or Gelu approximate="tanh":
 * 1); a synthetic-weight engine that should compute the tanh form sets it here.  fp32 and f16 engines follow it exactly (the fused K4
 * kernels of the 16-bit modes compute the exp2 = tanh form either way, bf16 stores the tanh-form shortcut: DESIGN.md 5d). */
int stn_set_gelu_form(stn_handle* h, int tanh_form);
int stn_get_gelu_form(const stn_handle* h);
/* Cross-attention blocks of the vector estimator: non-zero (default) = head-split: fold_ln (or LayerNorm) + ONE launch per block that
 * computes, per (utterance pair, head), the q projection, its rotation, the attention and the head's share of the output projection
 * and leaves it as a 16-bit per-head partial sum which the next ConvNeXt block's fold adds to the residual stream in head order
 * (kernels_xattn_hs.hip; 16-bit modes, packed rows with K4-split active, <= 256 frames per utterance, contexts of <= 128 keys: other
 * shapes take the four launches); 0 = four launches (LayerNorm, q projection, attention, output projection + residual).  Same result up
 * to the rounding of the per-head partial sums (tests/test_gpu_xattn.py).  (Rounds 1-3 had per-utterance one- and two-launch forms
 * here; they measured at parity or slower and were retired when the head-split form replaced them.) */
int stn_set_fused_xattn(stn_handle* h, int on);
/* K4 — the pointwise pair of a ConvNeXt block (pw1 -> GELU -> pw2 -> layer scale + residual) as ONE launch whose 4C-wide hidden
 * activation never leaves the registers (bf16 and f16 engines, block widths 384 / 512, batches of >= 18432 rows — below that a workgroup per 128 rows leaves most of the chip
 * idle while each still streams both weight matrices; other shapes keep the two GEMM launches).
 * Bit mask over the stages: 1 = vocoder, 2 = vector estimator, 4 = text encoder / duration predictor, 8 = the estimator's blocks as
 * K4-split (see stn_set_fused_ffn_min_rows); 0 = never.  The default (9) is the set of stages where a form measured faster on
 * MI355X.
 * WHAT IS AND IS NOT BIT-IDENTICAL.  Which kernel a block runs is decided by the launch's row count (these thresholds; the K4-split of
 * the estimator's blocks is 12 ways up to 1536 packed rows, 8 ways up to 4096 and 4 ways beyond; also split-K for small exact-fp32 GEMMs and the attention
 * grid shape), so an utterance synthesized alone, a small shard of a batch (e.g. 16 utterances per GPU of a strong-scaling run: below
 * 1536 rows) and the same utterance inside a large batch may run different kernels: they agree to rounding (K4 vs two launches: fp32 summation order and, in f16, the exp2- vs
 * erf-form GELU; K4-split: 16-bit partial sums), with identical predicted durations to 1e-5 and identical latent lengths
 * (tests/test_gpu_batch_invariance.py holds recorded bounds).  Within one kernel regime a row's result does not depend on the
 * number of rows, their order or their position in the launch: packed vs trimmed vs dense vocoder rows, graph replay vs eager and
 * sharded vs unsharded batches of the same regime are bit-identical (tests/test_gpu_packed.py, tests/test_gpu_ffn.py). */
int stn_set_fused_ffn(stn_handle* h, int stage_mask);
/* Row thresholds of the two fused forms (negative: leave unchanged): K4 (stage mask bits 1 / 2 / 4) is taken from k4_rows rows on,
 * K4-split (bit 8: the estimator's blocks with the hidden dimension cut over four workgroups per 128-row slab and 16-bit partial
 * sums folded by the next reader of the residual stream) from split_rows rows on.  Below a threshold the block runs as two tiled
 * GEMM launches; the forms agree to rounding, not bit for bit (tests/test_gpu_ffn.py, tests/test_gpu_batch_invariance.py). */
int stn_set_fused_ffn_min_rows(stn_handle* h, int64_t k4_rows, int64_t split_rows);
/* rows the vector estimator worked on in the last stn_batch_run: sum of the latent lengths (packed) or B*L (padded) */
int64_t stn_batch_ve_rows(const stn_handle* h);
/* frames the vocoder computed in the last stn_batch_run: B*L*ccf, or fewer when the position-independent part of the padding
 * was filled from the model's cached zero-latent response (bit-identical result; bf16 and f16 engines, packed row layout) */
int64_t stn_batch_vo_rows(const stn_handle* h);
int64_t stn_graph_replays(const stn_handle* h);
/* B, L (latent frames, model rate) and the samples per utterance every fetch returns: L * chunk at the model's rate, or
 * ceil(L * chunk * P / Q) with an output rate set (stn_set_output_rate) */
int stn_batch_dims(const stn_handle* h, int* B, int* L, int64_t* wav_len_per_utt);
int stn_batch_fetch(stn_handle* h, float* wav, size_t wav_capacity_floats, float* duration);
/* same, as 16-bit PCM converted on the GPU exactly as writeWavFile does (clamp to [-1,1], *32767, truncation;
 * cpp/helper.cpp:986-987): half the device->host bytes */
int stn_batch_fetch_pcm16(stn_handle* h, int16_t* pcm, size_t capacity_samples, float* duration);
/* the same, pipelined over two slots: _begin converts to PCM on the GPU and starts the device->host copy on a second stream,
 * so that the copy of batch i overlaps stn_batch_upload / stn_batch_run of batch i+1; _end waits for the slot's copy and hands
 * out the handle's pinned host buffer ([B, W] int16, valid until the slot's next _begin) with the batch's durations.  This is
 * the host-to-host path of _infer's contract (host inputs in, host waveform out: cpp/helper.cpp:674-682) at full overlap. */
int stn_batch_fetch_pcm16_begin(stn_handle* h, int slot /* 0 or 1 */);
int stn_batch_fetch_pcm16_end(stn_handle* h, int slot, const int16_t** pcm, size_t* n_samples, float* duration_or_null);
/* the batch a slot holds (fixed at its _begin; the resident batch may have changed since): utterances, samples per utterance;
 * `duration_or_null` of _end takes B floats */
int stn_batch_fetch_slot_dims(stn_handle* h, int slot, int* B, int64_t* samples_per_utt);
/* page-locked host memory for the caller's input buffers (ids, masks, styles): uploads from it are asynchronous DMA instead of a
 * staged copy.  NULL on failure. */
void* stn_host_alloc_pinned(size_t bytes);
void stn_host_free_pinned(void* p);
int stn_batch_fetch_latent(stn_handle* h, float* latent /*[B,D,L]*/);
/* device pointer of the finished waveform [B, L*cs] float32 (valid until the next upload/run) */
int stn_batch_wav_device_ptr(const stn_handle* h, void** ptr);
int stn_sync(stn_handle* h);
/* enqueue on a caller-owned HIP stream (hipStream_t passed as void*; NULL = the handle's own stream), e.g. the
 * framework stream that also carries the RCCL gather of the finished waveforms */
int stn_set_stream(stn_handle* h, void* hip_stream);
/* device->device copy of the finished waveform rows [B][W] into dst (row stride dst_stride floats >= W), enqueued
 * on the handle's stream */
int stn_batch_copy_wav_device(stn_handle* h, void* dst_device, int64_t dst_stride);
/* same as 16-bit PCM (the conversion of writeWavFile, cpp/helper.cpp:986-987), e.g. straight into an RCCL gather payload:
 * half the bytes over xGMI; dst_stride in samples */
int stn_batch_copy_pcm16_device(stn_handle* h, void* dst_device, int64_t dst_stride);

/* ---- sample encodings --------------------------------------------------------------------------------
 * Every fetch path can deliver the waveform in one of these encodings.  The encoded signal is the one the fp32 fetch delivers (at the
 * output rate when one is set, times the loudness gain when normalization is on); the encoding is the last step of the one store on
 * the GPU.  v = that fp32 sample:
 *   STN_ENC_F32    4 bytes  v                                                     (stn_batch_fetch)
 *   STN_ENC_PCM16  2 bytes  pcm16(v) = (int16)(clamp(v, -1, 1) * 32767), truncation  (stn_batch_fetch_pcm16)
 *   STN_ENC_PCM24  3 bytes  (int)(clamp(v, -1, 1) * 8388607.0f) in fp32, little-endian two's complement
 *   STN_ENC_MULAW  1 byte   G.711 mu-law of pcm16(v): G.191 ulaw_compress of pcm16(v) >> 2, as audioop.lin2ulaw(s, 2)
 *   STN_ENC_ALAW   1 byte   G.711 A-law of pcm16(v): G.191 alaw_compress of pcm16(v) >> 3, as audioop.lin2alaw(s, 2)
 * A mu-law or A-law codeword is a pure function of the 16-bit sample.  Zero codewords (what silence and padding are): 0.0f, 0, 00 00 00,
 * 0xFF (mu-law; 0x00 is its full-scale negative), 0xD5 (A-law).  Buffers are [B][W] samples of enc_bytes each, rows packed (host
 * fetches) or dst_stride samples apart (device copies).  The encoding is a fetch argument, not a handle setting: the captured pipeline
 * and stn_batch_wav_device_ptr are unchanged, and switching encodings drops or re-keys no captured graph.  DESIGN.md section 12. */
#define STN_ENC_F32 0
#define STN_ENC_PCM16 1
#define STN_ENC_PCM24 2
#define STN_ENC_MULAW 3
#define STN_ENC_ALAW 4
/* bytes per sample of an encoding; 0 for an unknown one */
int stn_encoding_bytes(int enc);
/* stn_batch_fetch in encoding enc: B * W * stn_encoding_bytes(enc) bytes into dst (may be NULL: durations only) */
int stn_batch_fetch_encoded(stn_handle* h, int enc, void* dst, size_t capacity_bytes, float* duration);
/* stn_batch_copy_wav_device in encoding enc; dst_stride in samples */
int stn_batch_copy_encoded_device(stn_handle* h, int enc, void* dst_device, int64_t dst_stride);
/* stn_batch_fetch_pcm16_begin / _end in encoding enc (the slot's pinned buffer holds *n_bytes bytes).  stn_batch_fetch_pcm16_begin is
 * this with STN_ENC_PCM16; stn_batch_fetch_pcm16_end on a slot begun with another encoding is STN_ERR_STATE. */
int stn_batch_fetch_encoded_begin(stn_handle* h, int slot, int enc);
int stn_batch_fetch_encoded_end(stn_handle* h, int slot, const void** data, size_t* n_bytes, float* duration_or_null);
/* op-level: rows x W fp32 (host) -> rows x W samples of encoding enc (host, rows packed): the fetch's store kernel without a gain */
int stn_op_encode(stn_handle* h, int enc, int rows, int W, const float* x, void* y);

/* ---- dither --------------------------------------------------------------------------------------------
 * The 16- and 24-bit PCM stores above truncate toward zero (the reference's writeWavFile rule): a dead zone 2 LSB wide around zero and
 * an error that is correlated with the signal.  With a mode set, every fetch path (stn_batch_fetch_pcm16*, _encoded*, the begin / end
 * slots, stn_batch_copy_*_device, stn_batch_fetch_joined*) quantizes those two encodings as follows instead; v is the fp32 sample the
 * store encodes today (after gain and fades), S = 32767 (PCM16) or 8388607 (PCM24):
 *   vc = fminf(1, fmaxf(-1, v))  (fp32);  t = (double)vc * S + 0.5 + (double)d;  q = clamp((int)floor(t), -S, S)
 *   STN_DITHER_OFF      the default: truncation, byte for byte what the handle delivers without this setting
 *   STN_DITHER_ROUND    d = 0: round to nearest, no noise
 *   STN_DITHER_TPDF     d = (a - b) / 65536: triangular density over (-1, 1) LSB; the total error has zero mean and variance LSB^2 / 4
 *                       whatever the signal
 *   STN_DITHER_TPDF_HP  d = (a_n - a_{n-1}) / 65536, a_{-1} := b_0: the same density and power, about 4.5 times as much of it in the
 *                       upper half of the band as in the lower
 * a and b are the halves of a Philox4x32-10 word: sample n (0-based in the delivered row or programme; n < 2^34) of stream (kind, id)
 * takes word [n & 3] of the block with counter {(uint32)(n >> 2), (uint32)id, (uint32)(id >> 32), 0xD17E0000 | kind} and key
 * {(uint32)seed, (uint32)(seed >> 32)}; a = w & 0xFFFF, b = w >> 16.  Streams: a per-row fetch (trimmed or not) keys row b by kind 0 and
 * its utterance id (stn_batch_upload's utt_ids; the row index without them), so an utterance's bytes do not depend on the batch it is
 * in; a joined fetch keys programme g by kind 1 and g.  Every sample of the row is dithered (a trimmed row's and a programme's: those
 * of its length, the gaps between members included; behind the length the zero codeword stays).  STN_ENC_F32, _MULAW and _ALAW
 * fetches are unaffected by any mode, byte for byte (dither in front of a logarithmic quantizer means nothing).  With loudness on, the
 * peak ceiling then holds to within 1.5 LSB of the encoding instead of exactly.  Handle state that no captured graph depends on; with
 * a rate set, a dithered PCM fetch resamples into fp32 scratch and ends in the common store (one more pass).  DESIGN.md section 23. */
#define STN_DITHER_OFF 0
#define STN_DITHER_ROUND 1
#define STN_DITHER_TPDF 2
#define STN_DITHER_TPDF_HP 3
#define STN_DITHER_ROW 0  /* stream kinds */
#define STN_DITHER_PROG 1
/* any other mode: STN_ERR_INVALID with a message, and the previous setting stays in force */
int stn_set_dither(stn_handle* h, int mode, uint64_t seed);
/* the mode (and the seed when seed_or_null is not NULL), or STN_ERR_INVALID for a NULL handle */
int stn_get_dither(const stn_handle* h, uint64_t* seed_or_null);
/* Host only (no device, no handle): the same rule on the CPU.  d[i] = the dither of sample n0 + i, i < n, of stream (kind, id) under
 * mode and seed, in LSB (0 for STN_DITHER_OFF and _ROUND) */
int stn_dither_noise(int mode, uint64_t seed, int kind, uint64_t id, int64_t n0, int64_t n, float* d);
/* ... and out[i] = the code of v[i] at stream index n0 + i in encoding enc (STN_ENC_PCM16: int16; STN_ENC_PCM24: three bytes), by the
 * mode's rule (STN_DITHER_OFF: truncation).  STN_ERR_INVALID: another encoding, an unknown mode or kind, n0 < 0 or n0 + n > 2^34 */
int stn_dither_quantize(int enc, int mode, uint64_t seed, int kind, uint64_t id, int64_t n0, int64_t n, const float* v, void* out);
/* op-level: the fetch's store kernel on the caller's whole buffers.  x [rows][W] fp32 (host), placed x_misalign (0 .. 3) floats behind a
 * 16-byte boundary on the device (not 0: the kernel's one-sample form); times gain[row] unless NULL; row's stream is (0, row_id[row]), or
 * (0, row) without row_id; y [rows][dst_stride] samples of enc (host): copied to the device, stored into, copied back, so samples
 * [W, dst_stride) of a row come back as they went in.  mode STN_DITHER_OFF is stn_op_encode with a gain and a stride. */
int stn_op_encode_ex(stn_handle* h, int enc, int rows, int W, const float* x, int x_misalign, const float* gain_or_null, const int64_t* row_id_or_null,
                     int mode, uint64_t seed, int64_t dst_stride, void* y);

/* ---- pitch ---------------------------------------------------------------------------------------------
 * Every fetch path delivers the rows shifted by `semitones` without a change of length: each row is stretched in time by a / b, the
 * fraction closest to 2^(semitones / 12), at the model's rate (WSOLA with a normalised search: the duration changes, the pitch stays), and
 * resampled by b / a back to its length (the duration is restored, the pitch moves).  Both steps run in front of every other stage of
 * the output stage, so rate, filters, de-esser, compressor, loudness, limiter, trim, pause limit, join, encodings and dither all see
 * the shifted rows; row length, spans and reported durations do not change.  0 (the default) is off: nothing is launched and no scratch
 * exists.  Formants move with the pitch (a resampling shifter) unless the pitch mode is STN_PITCH_FORMANT (section "formant" below);
 * the value is one per handle, and the tempo is the model's `speed`.
 * Handle state that no captured graph depends on.  DESIGN.md section 24.
 *
 * The stretch at rate hz: hop H, the smallest power of two with 128 H >= hz; grain N = 2 H; search radius D = 3 H / 4; window the periodic
 * Hann w[i] = 0.5 (1 - cos(2 pi i / N)) as float32.  A row x of span n reads 0.0 outside [0, n).  Frame m is analysed at
 * p_m = floor(m H b / a) and its grain starts at q_m = p_m + d_m - H, with d_0 = 0 and d_m, m >= 1, the d in [-D, D] of the largest
 * score(d) = c(d) / sqrt(E(d) + 1e-9), c(d) = sum_i t[i] x[p_m + d - H + i], E(d) = sum_i x[p_m + d - H + i]^2 over i in [0, N), against
 * the target t[i] = x[q_{m-1} + H + i]; among equal scores the smallest |d|, then the negative one.  The stretched row has
 * Ws = ceil(W a / b) samples, y[m H + i] = w[H + i] x[q_m + H + i] + w[i] x[q_{m+1} + i] for i in [0, H), over M = Ws / H + 2 frames.
 * From the end of the row's stretched span, ceil(n a / b), on y is 0.0: what the last grains leave there would reach the resampler in a
 * wide batch and not in a narrow one, and a row's result depends on its own samples only.
 * The resample back uses the resampler's design (section "resample") for P = b, Q = a, stated at the rates a k -> b k Hz with the
 * smallest k that has min(a, b) k >= 8000: stn_op_pitch(x) is, bit for bit, the first W columns of stn_op_resample(a k, b k) of
 * stn_op_time_stretch(x). */
/* Host only: the fraction a / b, 1 <= a, b <= 640, closest to r = pow(2, semitones / 12) in log ratio (the smaller of q / r and r / q,
 * q = a / b, in double); among equals the smaller b; always reduced.  The realised pitch is within 1.36 cents of the request.
 * STN_ERR_INVALID unless semitones is finite and in [-12, 12]; stn_pitch_error gives the message ("" for a value that is taken; the
 * string is the calling thread's until its next call). */
int stn_pitch_ratio(float semitones, int* a, int* b);
const char* stn_pitch_error(float semitones);
/* Host only: the geometry at hz for rows of W samples stretched by a / b; each output may be NULL.  STN_ERR_INVALID for hz outside
 * [8000, 192000], W < 0, or a term outside [1, 640] */
int stn_pitch_plan(int hz, int64_t W, int a, int b, int* H, int* delta, int64_t* M, int64_t* Ws);
/* Host only: the window at hz, the table the device multiplies by: *n = N, and w[0 .. min(N, cap)) when w is not NULL */
int stn_pitch_window(int hz, float* w_or_null, size_t cap, int* n);
/* 0: off (the default).  Not finite or outside [-12, 12]: STN_ERR_INVALID with stn_pitch_error's message, and the previous setting stays */
int stn_set_pitch(stn_handle* h, float semitones);
/* the setting and its ratio (1 / 1 when off); each output may be NULL */
int stn_get_pitch(const stn_handle* h, float* semitones, int* a, int* b);
/* op-level: the stretch of the batch path on the caller's rows.  x [rows][W] fp32 (host) at hz, row r's span n[r] in [0, W] (NULL: W);
 * y [rows][Ws] fp32, delta [rows][M] int32 (delta[r][0] = 0) and score [rows][M] fp32 (the winners' scores; 0 for frame 0), host, each
 * or NULL, with Ws and M from stn_pitch_plan */
int stn_op_time_stretch(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, int a, int b, float* y_or_null,
                        int32_t* delta_or_null, float* score_or_null);
/* ... and the whole shift: the stretch by stn_pitch_ratio(semitones) and the resample back, y [rows][W] fp32 (host) */
int stn_op_pitch(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, float semitones, float* y);

/* ---- formant (the pitch mode) ----------------------------------------------------------------------------
 * STN_PITCH_RESAMPLE (the default) delivers the shifted rows as the section above describes them.  STN_PITCH_FORMANT ends the pitch
 * stage with a correction that puts the spectral envelope of the row before the shift back onto the shifted row, so that the pitch
 * moves and the formants stay.  The mode has no effect while pitch is 0: nothing is launched and no scratch exists.  One value per
 * handle; handle state that no captured graph depends on.  DESIGN.md section 26.
 *
 * The rule at rate hz, on x (the row before the shift) and y (the shifted row), both of span n and 0.0 outside [0, n): hop H and window
 * w of the pitch stage, N = 2 H, frames m = 0 .. ceil(W / H) over [s_m, s_m + N), s_m = (m - 1) H, order
 * p = min(48, max(10, 2 ceil(hz / 2000) + 2)).  Per frame and signal: xw[i] = float32(w[i] x[s_m + i]); R[k] = sum_i xw[i] xw[i + k],
 * k = 0 .. p, in double; R'[0] = 1.0001 R[0] + 1e-9 and R'[k] = R[k] exp(-0.5 (2 pi 60 k / hz)^2); Levinson-Durbin in double gives
 * a[0 .. p], a[0] = 1, and the final error E.  Per frame g = clamp(sqrt(E_x / E_y), 1/2, 2), and the float32 tables ax[k] = a_x[k],
 * cy[k] = g a_y[k].  Frame m filters y from zero state at n0 = s_m - N (y taken as 0.0 before n0 and from n on):
 * e[j] = sum_{k=0..p} cy[k] y[j - k], v_m[j] = e[j] - sum_{k=1..p} ax[k] v_m[j - k] for j in [n0, s_m + N), in float32.
 * out[m H + i] = w[H + i] v_m[m H + i] + w[i] v_{m+1}[m H + i] for i in [0, H), and out[j] = 0.0 for j >= n.  The warm-up of N
 * samples is part of the rule.  A row's result depends on its own samples only. */
#define STN_PITCH_RESAMPLE 0
#define STN_PITCH_FORMANT 1
/* Host only: the geometry at hz for rows of W samples, each output or NULL, and the lag window lag[0 .. min(p + 1, cap)) in double when
 * lag is not NULL.  STN_ERR_INVALID for hz outside [8000, 192000] or W outside [0, 2^40] */
int stn_formant_plan(int hz, int64_t W, int* H, int* p, int64_t* frames, double* lag_or_null, size_t cap);
/* Host only: the conditioning and the recursion in double on the caller's lags r[0 .. p], 1 <= p <= 48, at hz (the lag window's rate):
 * a[0 .. p], *err = E and, when not NULL, the p reflection coefficients */
int stn_formant_lpc(int hz, const double* r, int p, double* a, double* err, double* refl_or_null);
/* any other value: STN_ERR_INVALID, and the previous mode stays */
int stn_set_pitch_mode(stn_handle* h, int mode);
/* the mode, or STN_ERR_INVALID for a NULL handle */
int stn_get_pitch_mode(const stn_handle* h);
/* op-level: the correction of the batch path on the caller's rows.  x and y [rows][W] fp32 (host) at hz, row r's span n[r] in [0, W]
 * (NULL: W); out [rows][W] fp32 (host) */
int stn_op_formant(stn_handle* h, int hz, int rows, int W, const float* x, const float* y, const int64_t* n_or_null, float* out);
/* ... and with the tables handed out: ax and cy [rows][frames][p + 1] fp32, g, ex and ey [rows][frames] double (host, each or NULL),
 * computed on scratch filled with NaN before the launches; *guard_ok: the 64 NaN words on either side of x, y and out on the device are
 * still there */
int stn_op_formant_ex(stn_handle* h, int hz, int rows, int W, const float* x, const float* y, const int64_t* n_or_null, float* out, float* ax_or_null,
                      float* cy_or_null, double* g_or_null, double* ex_or_null, double* ey_or_null, int* guard_ok);
/* stn_op_pitch under a mode.  STN_PITCH_FORMANT: bit for bit stn_op_formant(x, stn_op_pitch(x)) */
int stn_op_pitch_ex(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, float semitones, int mode, float* y);

/* ---- join ----------------------------------------------------------------------------------------------
 * Consecutive rows of the finished batch concatenated on the GPU, with a run of silence between them, into G programmes (the chunks of
 * a long text, cpp/helper.cpp:685-723): a joined fetch delivers [G][W_join] samples instead of [B][W], in any encoding, at the output
 * rate.  Programme g is seg_0 gap seg_1 gap ... seg_{k-1}: prog_len[g] = sum len_i + (k - 1) * gap_samples[g], W_join = max_g prog_len[g];
 * every gap and everything behind prog_len[g] in the row is the encoding's zero codeword (0xFF / 0xD5 for the G.711 laws).  prog_dur[g]
 * is the reference's fp32 sum in member order: d = dur_0; d += dur_i + gap_seconds[g] (cpp/helper.cpp:708,714).  The gap is given in
 * samples (at the current output rate) and in seconds: each host keeps its own rounding of silence_duration * rate.
 * Member i's length: STN_JOIN_WHOLE, its own run's whole wave, min(W, ceil(L_i * chunk * P / Q)) samples (cpp/helper.cpp:706-715);
 * STN_JOIN_TRIM, the first min(that, (int64_t)(duration_i * (float)rate)) of them (rust/src/helper.rs:700-702).
 * With loudness off, or on with STN_JOIN_GAIN_ROW (every member keeps its own gain g_b), sample s of a segment is the sample the
 * per-row fetch in the same encoding delivers at that row and column: the joined fetch is byte for byte the host concatenation of
 * stn_batch_fetch_encoded's rows.  STN_JOIN_GAIN_PROG: the joined fp32 signal, gaps included, is measured as G rows with span
 * n_g = min(prog_len[g], (int64_t)(prog_dur[g] * (float)rate)) and stored with one gain per programme (the rule of stn_set_loudness).
 * The join is a fetch argument, not a handle setting: no other fetch changes, the captured pipeline and stn_batch_wav_device_ptr are
 * untouched, and a joined fetch drops or re-captures no graph.  Refused with STN_ERR_INVALID and a message: rows that do not sum to B, a
 * count < 1, a negative gap, an unknown mode / scope / encoding, dst_stride < W_join, a buffer that is too small (the message states
 * the bytes needed); STN_ERR_STATE without a finished batch.  A group (stn_group_*) deals a batch's rows over devices and has no
 * joined fetch.  DESIGN.md section 13. */
#define STN_JOIN_WHOLE 0
#define STN_JOIN_TRIM 1
#define STN_JOIN_GAIN_ROW 0
#define STN_JOIN_GAIN_PROG 1
typedef struct stn_join {
    int32_t n_prog;              /* G >= 1 */
    const int32_t* rows;         /* [G] members per programme, each >= 1, sum == B; members are consecutive rows */
    const int64_t* gap_samples;  /* [G] zeros between two members, at the current output rate, >= 0 */
    const float* gap_seconds;    /* [G] what the duration sum adds per gap */
    int32_t mode;                /* STN_JOIN_WHOLE / STN_JOIN_TRIM */
    int32_t gain_scope;          /* STN_JOIN_GAIN_ROW / STN_JOIN_GAIN_PROG (ignored with loudness off) */
} stn_join;
/* host only, no device: the plan for B members of whole lengths member_len (each in [0, W_out]) and durations member_dur at rate hz
 * (hz is used by STN_JOIN_TRIM only).  Out: *W_join, prog_len [G], prog_dur [G]; seg_len [B] (the members' lengths under j->mode) and
 * seg_dst [B] (their first sample in the programme's row), each of the two may be NULL.  STN_ERR_INVALID for a refused argument
 * (stn_join_plan_error says why). */
int stn_join_plan(const stn_join* j, int B, int64_t W_out, int hz, const int64_t* member_len, const float* member_dur, int64_t* W_join,
                  int64_t* prog_len, float* prog_dur, int64_t* seg_len_or_null, int64_t* seg_dst_or_null);
const char* stn_join_plan_error(void);
/* the plan of the finished batch under j: *W_join, prog_len [G] and prog_dur [G] (each may be NULL) */
int stn_batch_join_dims(stn_handle* h, const stn_join* j, int64_t* W_join, int64_t* prog_len, float* prog_dur);
/* G * W_join * stn_encoding_bytes(enc) bytes into dst, rows packed (dst may be NULL: lengths and durations only) */
int stn_batch_fetch_joined(stn_handle* h, const stn_join* j, int enc, void* dst, size_t capacity_bytes, int64_t* prog_len, float* prog_dur);
/* the joined rows into a device buffer, rows dst_stride samples apart (>= W_join), on the handle's stream */
int stn_batch_copy_joined_device(stn_handle* h, const stn_join* j, int enc, void* dst_device, int64_t dst_stride);
/* the pipelined fetch of the joined rows; ended by stn_batch_fetch_encoded_end (durations: prog_dur [G]); stn_batch_fetch_slot_dims
 * reports G and W_join */
int stn_batch_fetch_joined_begin(stn_handle* h, int slot, const stn_join* j, int enc);
/* the joined signal at the output rate measured as G programmes, whether normalization is on or not: L_g (LUFS), peak_g and the gain
 * STN_JOIN_GAIN_PROG applies under the current setting (1 when off); each pointer [G] floats or NULL */
int stn_batch_join_loudness(stn_handle* h, const stn_join* j, float* lufs, float* peak, float* gain);
/* op-level, host operands: rows x W fp32 at hz, row r's first n[r] samples are member r's segment (j->mode is not applied) -> y
 * [G][W_join] samples of enc, rows packed (W_join as stn_join_plan gives it).  loudness_on: every programme measured over its prog_len
 * samples and stored with its own gain, *prog_lufs / *prog_peak / *prog_gain [G] (each may be NULL; with loudness off the gain is 1
 * and nothing is measured unless one of them is asked for). */
int stn_op_join(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, const stn_join* j, int enc, int loudness_on,
                float target_lufs, float ceiling_dbfs, void* y, float* prog_lufs, float* prog_peak, float* prog_gain);

/* ---- output rate ---------------------------------------------------------------------------------------
 * The model synthesizes at its own rate (stn_arch.sample_rate, 44.1 kHz for the published model; the reference's hosts can only
 * return that: cpp/helper.cpp:943-990).  With an output rate set, every fetch path — stn_batch_fetch, stn_batch_fetch_pcm16,
 * stn_batch_fetch_pcm16_begin / _end (slots sized in output samples), stn_batch_copy_wav_device, stn_batch_copy_pcm16_device and
 * through it the group gather — resamples the finished waveform on the handle's stream before its copy, so the host and the
 * gather move output-rate samples.  stn_batch_dims and stn_batch_fetch_slot_dims report the samples at the output rate; durations
 * stay in seconds; stn_batch_wav_device_ptr stays the model-rate waveform.  The latent geometry and the captured pipeline are the
 * model rate's: setting the rate drops or re-keys no captured graph.
 * Resampler: rational polyphase, P/Q = out/in reduced by their gcd; output n of a row uses phase (n*Q) mod P and the inputs from
 * floor(n*Q/P) - off on (zero outside the row); W_out = ceil(W*P/Q); fp32 sums in a fixed tap order, the same for every output
 * position (the first ceil(m*P/Q) outputs of a row that is zero past m are those of the row cut at m).  Filter: Kaiser-windowed
 * sinc, passband within +-0.05 dB up to 0.85 * min(in, out)/2, >= 80 dB rejection from min(in, out)/2 on, every phase's gain 1 at
 * DC.  Rates: [8000, 192000] Hz with a reduced P <= 640 (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000 Hz
 * against 44.1 kHz among them); anything else is STN_ERR_INVALID with a message.  PCM conversion as writeWavFile (clamp, *32767,
 * truncation): the PCM bytes are the fp32 output's converted.  DESIGN.md section 10 has the table sizes and the measured cost. */
/* hz = 0 or the model's rate: off (the default: every fetch is byte for byte the native one, with no extra launch) */
int stn_set_output_rate(stn_handle* h, int hz);
/* the effective rate of the fetches: the output rate, or the model's rate when off (0 before a model is loaded) */
int stn_get_output_rate(const stn_handle* h);
/* the filter the resampler uses for in_hz -> out_hz (host only, no device needed): *phases = P, *taps_per_phase = T, taps
 * [P][T] (tap j of phase p multiplies input floor(n*Q/P) - (T/2 - 1) + j) when taps != NULL and cap >= P*T.  STN_ERR_INVALID for a
 * refused pair (stn_resample_error says why).  in_hz == out_hz gives the one-phase unit filter (a copy). */
int stn_resample_filter(int in_hz, int out_hz, float* taps_or_null, size_t cap, int* phases, int* taps_per_phase);
/* why a pair is refused ("" when it is supported); host only */
const char* stn_resample_error(int in_hz, int out_hz);
/* op-level: rows x W fp32 (host) at in_hz -> rows x ceil(W*P/Q) at out_hz, as fp32 (y) and / or int16 PCM (pcm); either may be
 * NULL but not both.  1 <= rows <= 65535. */
int stn_op_resample(stn_handle* h, int in_hz, int out_hz, int rows, int W, const float* x, float* y_or_null, int16_t* pcm_or_null);
/* the form the resampler's launcher takes for rows of W samples (host only, no device needed): "resample lds G<n>" (a workgroup's
 * input span staged in LDS, n groups of 64 output periods per workgroup: 16, 8, 4, 2 or 1) or "resample cache G<n>" (a span above
 * 160 KiB, read through the caches).  Returns the string's length (written NUL-terminated when cap is larger), STN_ERR_INVALID for
 * W < 1 or a refused pair. */
int stn_dbg_resample_form(int in_hz, int out_hz, int64_t W, char* out, size_t cap);

/* ---- loudness --------------------------------------------------------------------------------------
 * With normalization on, every fetch path — stn_batch_fetch, stn_batch_fetch_pcm16, stn_batch_fetch_pcm16_begin / _end,
 * stn_batch_copy_wav_device, stn_batch_copy_pcm16_device and through it the group gather — measures the finished waveform at the
 * output rate (after resampling when a rate is set, before the PCM conversion) and scales row b by one fp32 gain on the handle's
 * stream before its copy.  Row b's span is its first n_b = min(W_out, (int64_t)(duration_b * (float)rate)) samples (duration_b: the
 * reported duration); padding beyond it is not measured and is scaled by the same gain.
 * Loudness L_b: ITU-R BS.1770-4 integrated loudness of one channel: K-weighting (shelf, then high-pass; stn_kweighting_filter), 400 ms
 * blocks at a 100 ms hop of (rate + 5) / 10 samples (whole blocks inside the span only), absolute gate -70 LUFS, relative gate -10 LU;
 * -inf when the span is shorter than one block or every block is gated out.
 * Gain g_b = min(10^((target - L_b) / 20), 10^(ceiling / 20) / peak_b), peak_b = max |x| over the span; 1 when L_b is -inf (with the
 * limiter on, "limiter" below, the first operand alone: the limiter then enforces the ceiling).  The fp32
 * output is x * g_b (one fp32 multiply); the PCM output is that product converted as writeWavFile converts.  A row's L_b, peak_b and
 * g_b depend on its first n_b samples and the rate only (fixed-order sums, no atomics): not on the batch it was in.
 * The latent geometry, the durations, stn_batch_wav_device_ptr (model rate, not normalized) and the captured pipeline are unchanged:
 * the setting drops or re-keys no captured graph.  DESIGN.md section 11 has the decomposition, the cost and the accuracy. */
/* on = 0: off (the default: every fetch is byte for byte the one without it, with no extra launch).  target_lufs in [-60, 0],
 * ceiling_dbfs (sample peak) in [-30, 0]; out of range: STN_ERR_INVALID with a message, and the previous setting stays in force. */
int stn_set_loudness(stn_handle* h, int on, float target_lufs, float ceiling_dbfs);
int stn_get_loudness(const stn_handle* h, int* on, float* target_lufs, float* ceiling_dbfs);
/* the finished batch measured at the current output rate, whether normalization is on or not: L_b (LUFS), peak_b and the gain the
 * current setting applies (1 when off); each pointer [B] floats or NULL */
int stn_batch_loudness(stn_handle* h, float* lufs, float* peak, float* gain);
/* op-level: rows x W fp32 (host) at hz in [8000, 192000]; row r's first n[r] samples (n_or_null = NULL: all W) -> L (LUFS, -inf when
 * undefined) and sample peak, [rows] floats each (either may be NULL).  1 <= rows <= 65535. */
int stn_op_loudness(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, float* lufs, float* peak);
/* the K-weighting biquads at hz (host only, no device needed): b[3] and a[3] (a[0] = 1) of the shelf and of the high-pass, in double;
 * STN_ERR_INVALID outside [8000, 192000] Hz */
int stn_kweighting_filter(int hz, double* shelf_b3, double* shelf_a3, double* hp_b3, double* hp_a3);
/* The same measurement (the same four launches through the same launchers) with its scratch laid open (the kernel tests of every pass).
 * n_or_null as stn_op_loudness; on / target_lufs / ceiling_dbfs: the gate's gain as stn_set_loudness defines it (on = 0: gain 1; not
 * range-checked).  x_misalign 0 / 1: x is uploaded 16-byte aligned / 4 bytes off, which forces the scalar staging path at W % 4 == 0.
 * Before the first launch the whole scratch (st, pk, pa, pb and the results) is filled with the quiet NaN 0x7FC00000, so an element no
 * launch wrote comes back as that.  With Ks = (W + 31) / 32 chunks per row: st_end [rows][Ks][4], the state buffer as launch 1 left it
 * (chunk k's end state (s1, s2, t1, t2) from zero state); st_start [rows][Ks][4], the same buffer after the scan (chunk k's true start
 * state); pk, pa, pb [rows][Ks] (chunk k's max |x|, its sum of y^2 inside the 100 ms segment it starts in, and inside the next one);
 * lufs, peak, gain [rows].  Every output may be NULL.  form: the staging path that ran, "vec" (16-byte loads) or "scalar",
 * NUL-terminated, truncated to form_cap; may be NULL.  Refuses what stn_op_loudness refuses, and an x_misalign outside {0, 1}. */
int stn_op_loudness_ex(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, int on, float target_lufs,
                       float ceiling_dbfs, int x_misalign, float* st_end, float* st_start, float* pk, float* pa, float* pb, float* lufs,
                       float* peak, float* gain, char* form, size_t form_cap);
/* what the measurement's kernels are given at hz (host only, no device needed): coef[10], the fp32 coefficients they multiply by (shelf
 * b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2); mpow, the first min(cap, 1024 * 16) entries of the scan's power table [1024][4][4],
 * entry i = M^(i+1) row-major with M = A^32 of the zero-input state transition A (state s1 s2 t1 t2) those coefficients define (the
 * scan reads the table in double; here it is rounded to fp32); *hop, the 100 ms segment in samples.  Each pointer may be NULL.
 * STN_ERR_INVALID outside [8000, 192000] Hz. */
int stn_loudness_table(int hz, float* coef10, float* mpow, size_t cap, int* hop);

/* ---- loudness range ------------------------------------------------------------------------------------
 * A report, not a setting: maximum momentary loudness, maximum short-term loudness (the limits of EBU R 128 s1, short-form content)
 * and loudness range (LRA, EBU Tech 3342) of the signal, rows and spans that stn_batch_loudness measures, under every combination of
 * settings (output rate, filters, de-esser, compressor, trimming, pause limit): the signal BEFORE the loudness gain.  LRA does not
 * depend on the gain; while the limiter is off the two maxima after normalization are the reported values plus 20 log10(gain).
 * Nothing is launched unless a report is asked for: no fetch, setting or captured graph changes.
 * Row b's span is its first n_b samples, hop = (rate + 5) / 10 samples, seg[j] the sum of y^2 (K-weighted) over segment j,
 * nseg = n_b / hop:
 *   momentary   M_j = -0.691 + 10 log10((seg[j] + .. + seg[j+3]) / (4 hop)), j = 0 .. nseg - 4: the very blocks of the integrated
 *               measurement, summed as (seg[j] + seg[j+1]) + (seg[j+2] + seg[j+3]).  m_max = max_j M_j, -inf when nseg < 4.
 *   short-term  S_j = -0.691 + 10 log10((seg[j] + .. + seg[j+29]) / (30 hop)), j = 0 .. nseg - 30: whole 3 s windows inside the span
 *               at a 100 ms hop, the 30 terms added left to right.  s_max = max_j S_j, -inf when nseg < 30.
 *   range       of the S_j keep those with S_j > -70 (absolute gate); rel = -0.691 + 10 log10(mean of their window powers) - 20; keep
 *               those with S_j > rel as well (relative gate).  n_st is the number kept; s[0 .. n_st - 1] the kept values ascending;
 *               lra = s[floor((n_st - 1) * 0.95 + 0.5)] - s[floor((n_st - 1) * 0.10 + 0.5)] (the index rule of Tech 3342's reference
 *               code), 0 when n_st < 2.
 * A row's four numbers depend on its first n_b samples and the rate only, not on W, the batch or the row's place in it (fixed-order
 * sums, no atomics): the same bits run twice, alone or among others.  A row may hold at most 8192 segments (13 min 39 s; the
 * integrated measurement takes 16384): beyond that STN_ERR_INVALID with a message that names the cap.  stn_group has no such report:
 * ask the ranks' handles.  DESIGN.md section 22 has the decomposition, the LDS layout, the accuracy and the cost. */
/* the finished batch at the current output rate, whether normalization is on or not; each pointer [B] or NULL.  STN_ERR_STATE without
 * a finished batch. */
int stn_batch_loudness_range(stn_handle* h, float* m_max, float* s_max, float* lra, int32_t* n_st);
/* the joined signal measured as G programmes over the spans stn_batch_join_loudness uses; each pointer [G] or NULL; refuses what that
 * call refuses */
int stn_batch_join_loudness_range(stn_handle* h, const stn_join* j, float* m_max, float* s_max, float* lra, int32_t* n_st);
/* op-level, host operands: rows x W fp32 at hz, row r's first n[r] samples (n_or_null = NULL: all W); each result [rows] or NULL.
 * Refuses what stn_op_loudness refuses. */
int stn_op_loudness_range(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, float* m_max, float* s_max,
                          float* lra, int32_t* n_st);
/* The rule itself (host only, no device needed): the definition above in double on given segment sums seg[nseg] of hop samples each.
 * Each result may be NULL.  STN_ERR_INVALID for hop < 1, nseg < 0 or seg NULL with nseg > 0.  The kernel's decisions are tested
 * against this function. */
int stn_loudness_range_rule(int hop, int64_t nseg, const double* seg, double* m_max, double* s_max, double* lra, int32_t* n_st);

/* ---- f0 ------------------------------------------------------------------------------------------------
 * A report, not a setting: the fundamental-frequency track of each row and its statistics, by YIN (de Cheveigne and Kawahara 2002,
 * steps 1 to 5), of the signal stn_batch_loudness measures: the rows at the output rate, behind pitch, filters, expander, de-esser
 * and compressor, row b's first n_b samples, BEFORE the loudness gain.  Nothing is launched unless a report is asked for: no fetch,
 * setting or captured graph changes.
 * Parameters stn_f0_params: the search range [fmin_hz, fmax_hz], the threshold of step 4 and the level gate gate_db (dB re full
 * scale, mean square).  Defaults 60, 500, 0.15, -60 (stn_f0_defaults).  Valid: 30 <= fmin < fmax <= 1000, 0 < threshold < 1,
 * -120 <= gate_db <= 0 and tau_min >= 2; anything else is STN_ERR_INVALID, and stn_f0_error(hz, params) gives the message.
 * For a row x of span n at rate hz (8000 to 192000), everything below in exact arithmetic:
 *   1. analysis signal: k = max(1, hz div 16000), ha = hz / k (a real number below 32000), u[j] = (x[jk] + .. + x[jk+k-1]) / k for
 *      j < n_a = n div k.  A box average is a poor low-pass (its first null is at ha, so the band above ha / 2 folds back attenuated
 *      by 4 dB at worst); it is enough for a detector whose shortest lag is ha / fmax >= 8 samples, and it needs no design table.
 *   2. geometry: hop Hh = floor(ha / 100 + 0.5), tau_max = ceil(ha / fmin), tau_min = floor(ha / fmax).  Frame t starts at s = t Hh
 *      and reads u[s .. s + 2 tau_max).  Frames are the whole ones inside the span: F = 0 if n_a < 2 tau_max, else
 *      (n_a - 2 tau_max) div Hh + 1.  The centre time of frame t is (s + tau_max) k / hz seconds.  Nothing behind the span is read.
 *   3. difference function: d(tau) = sum_{j < tau_max} (u[s+j] - u[s+j+tau])^2 for tau = 0 .. tau_max; d'(0) = 1 and
 *      d'(tau) = d(tau) tau / sum_{i=1..tau} d(i), 1 where that sum is 0.
 *   4. decision: the frame is unvoiced if the mean of u^2 over its first tau_max samples is below 10^(gate_db / 10).  Otherwise take
 *      the smallest tau in [tau_min, tau_max) with d'(tau) < threshold (none: unvoiced) and walk right while tau + 1 < tau_max and
 *      d'(tau + 1) < d'(tau): that is tau^.
 *   5. refinement: with a, b, c = d'(tau^ - 1), d'(tau^), d'(tau^ + 1), tau* = tau^ + clamp((a - c) / (2 (a - 2b + c)), -1, 1), and
 *      tau* = tau^ when a - 2b + c <= 0.  f0 = ha / tau* (Hz), aperiodicity ap = b.  An unvoiced frame has f0 = 0 and ap = 1.
 * Statistics stn_f0_stats over a row's voiced frames: median_hz the lower median (element (voiced - 1) div 2 of the ascending sort),
 * mean_hz the geometric mean 2^(mean of log2 f0), min_hz and max_hz; all four are 0 when no frame is voiced.
 * The device computes d in fp32 by the direct squared difference (the energy-minus-correlation form cancels in fp32) and the
 * refinement in double on the fp32 d'; DESIGN.md section 27 derives the bound of f0 and ap against the definition.  A frame's result
 * depends on its own 2 tau_max k samples, the rate and the parameters only (fixed-order sums, no atomics): not on W, the batch, the
 * row's place in it or the frames beside it.  A row may hold at most 32768 frames (5 min 27 s): beyond that STN_ERR_INVALID with a
 * message that names the row's count and the cap, before anything is uploaded or launched.  stn_group has no such report: ask the
 * ranks' handles.  DESIGN.md section 27 has the decomposition, the LDS layout, the accuracy and the cost. */
typedef struct stn_f0_params { float fmin_hz, fmax_hz, threshold, gate_db; } stn_f0_params;
typedef struct stn_f0_stats { int32_t frames, voiced; float median_hz, mean_hz, min_hz, max_hz; } stn_f0_stats;
/* host only, no device needed */
void stn_f0_defaults(stn_f0_params* p);
/* why (hz, params) is refused, or "" (params_or_null = NULL: the defaults); valid until the thread's next call */
const char* stn_f0_error(int hz, const stn_f0_params* params_or_null);
/* the geometry of a span of n samples at hz; each pointer may be NULL.  STN_ERR_INVALID for what stn_f0_error refuses or n < 0. */
int stn_f0_plan(int hz, int64_t n, const stn_f0_params* params_or_null, int* k, int* hop, int* tau_min, int* tau_max, int64_t* frames);
/* The definition above in double on the CPU: f0 and ap [cap] (either may be NULL), *frames the row's frame count.  STN_ERR_INVALID
 * for what stn_f0_plan refuses, x NULL with n > 0, or frames > cap with an array given.  The kernels are tested against this function.
 * stn_f0_rule_lags gives tau^ of each frame instead (0 for an unvoiced one). */
int stn_f0_rule(int hz, int64_t n, const float* x, const stn_f0_params* params_or_null, int64_t cap, double* f0, double* ap, int64_t* frames);
int stn_f0_rule_lags(int hz, int64_t n, const float* x, const stn_f0_params* params_or_null, int64_t cap, int32_t* lag, int64_t* frames);
/* the statistics of a track f0[frames] (fp32, 0 = unvoiced) as defined above, the log2 sum in double in frame order */
int stn_f0_stats_rule(const float* f0, int64_t frames, stn_f0_stats* out);
/* frames a workgroup of the track kernel owns (the seam the tests put rows across) and the most frames a row may hold */
int stn_f0_group(void);
int64_t stn_f0_max_frames(void);
/* the finished batch at the current output rate: *max_frames = the most frames any row holds (size f0 / ap with it).  STN_ERR_STATE
 * without a finished batch. */
int stn_batch_f0_frames(stn_handle* h, const stn_f0_params* params_or_null, int64_t* max_frames);
/* the finished batch: f0 and ap [B][cap] floats (ap may be NULL, f0 may be NULL too: statistics only), stats [B] (may be NULL).
 * Row b's frames are columns 0 .. stats[b].frames - 1; the columns behind them hold f0 = 0 and ap = 1.  STN_ERR_INVALID when a row
 * holds more than cap frames (with an array given) or more than the report takes. */
int stn_batch_f0(stn_handle* h, const stn_f0_params* params_or_null, int64_t cap, float* f0, float* ap_or_null, stn_f0_stats* stats);
/* op-level, host operands: rows x W fp32 at hz, row r's first n[r] samples (n_or_null = NULL: all W); results as stn_batch_f0.
 * 1 <= rows <= 65535. */
int stn_op_f0(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, const stn_f0_params* params_or_null, int64_t cap,
              float* f0, float* ap_or_null, stn_f0_stats* stats);

/* ---- silence trimming --------------------------------------------------------------------------------
 * With trimming on, every fetch path delivers each row without the silence in front of and behind its speech, found by level on the
 * GPU at fetch time.  It composes with the rate, the loudness, the encoding and the join; the latent geometry, the reported durations,
 * stn_batch_wav_device_ptr, the captured pipeline and the graph key are untouched, and toggling it drops or re-captures no graph.
 * Signal measured: the row at the output rate hz (after resampling when a rate is set, before any gain), row b's first
 * n_b = min(W_out, (int64_t)(duration_b * (float)hz)) samples (the loudness span).
 * Edges: frames of F = (hz + 50) / 100 samples (10 ms) from sample 0 without overlap, K = ceil(n / F), frame k over
 * [kF, min((k + 1)F, n)) with level m_k = mean of x^2 over its own samples; m_max = max m_k.  n = 0 or m_max <= 1e-7 (-70 dBFS mean
 * square): no speech, start = 0 and end = n.  Otherwise frame k is active when m_k >= m_max * 10^(-top_db / 10); with f0 the first and
 * f1 the last active frame and keep = (int64_t)(keep_ms * hz / 1000 + 0.5) (in double), start = max(0, f0 F - keep) and
 * end = min(n, (f1 + 1)F + keep).  Silence inside the row is never touched.  Every sum runs in an order fixed by sample positions within
 * the row (no float atomics): start and end depend on the row's first n samples, the rate and the parameters only, not on W, B or the
 * row's neighbours.
 * Fade: Fd = (int64_t)(fade_ms * hz / 1000 + 0.5), w[j] = float32(0.5 - 0.5 cos(pi (j + 0.5) / Fd)) (stn_silence_fade_window).  An edge
 * that was cut (start > 0, respectively end < n) is faded over the segment's first, respectively last, min(Fd, len) samples: sample q
 * of the segment times w[q], respectively w[len - 1 - q]; an edge that was not cut keeps its samples bit for bit.  A delivered sample is
 * ((x * g) * w_in) * w_out, three fp32 multiplies in that order, each only where it applies, then the encoding's rule.
 * Per-row fetches (stn_batch_fetch, _pcm16, _encoded, both pipelined slots, stn_batch_copy_*_device) still deliver [B][W_out] rows
 * (stn_batch_dims is unchanged): row b holds its segment [start_b, end_b) from column 0 and the encoding's zero codeword behind
 * len_b = end_b - start_b; the reported durations stay the model's; no host read is needed, so the pipelined _begin stays asynchronous.
 * Joined fetches (every stn_batch_*joined* entry, stn_batch_join_dims, stn_batch_join_loudness): under either mode a member's segment
 * is [start_b, end_b) and its duration in prog_dur's fp32 member-order sum is (float)len_b / (float)hz; the plan reads the edges with
 * one device-to-host copy of 2 B integers per finished batch and setting.  stn_join_plan and the refused mode values are unchanged.
 * Loudness: the per-row gain g_b stays the one measured over the untrimmed span n_b, so with fade_ms = 0 a trimmed row is byte for
 * byte a slice of the untrimmed fetch; STN_JOIN_GAIN_PROG measures the joined, faded signal.  The group (stn_group_*) does not trim.
 * DESIGN.md section 14 has the decomposition and the cost. */
/* on = 0: off (the default: every fetch is byte for byte the one without it, with no extra launch or allocation).  top_db in [1, 120],
 * keep_ms in [0, 1000], fade_ms in [0, 50]; out of range: STN_ERR_INVALID with a message, and the previous setting stays in force. */
int stn_set_silence_trim(stn_handle* h, int on, float top_db, float keep_ms, float fade_ms);
int stn_get_silence_trim(const stn_handle* h, int* on, float* top_db, float* keep_ms, float* fade_ms);
/* the finished batch's edges at the current output rate under the current parameters, whether trimming is on or not; each pointer [B]
 * integers or NULL */
int stn_batch_silence_edges(stn_handle* h, int64_t* start, int64_t* end);
/* op-level: rows x W fp32 (host) at hz in [8000, 192000]; row r's first n[r] samples (n_or_null = NULL: all W) -> start, end [rows]
 * (either may be NULL).  1 <= rows <= 65535. */
int stn_op_silence_edges(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, float top_db, float keep_ms,
                         int64_t* start, int64_t* end);
/* the same, and y: [rows][W] samples of enc, row r's segment from column 0 (times gain_or_null[r], cut edges faded), zero codewords
 * behind it */
int stn_op_silence_trim(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, float top_db, float keep_ms,
                        float fade_ms, const float* gain_or_null, int enc, void* y, int64_t* start, int64_t* end);
/* the fade window at hz (host only, no device needed): *n = Fd, and w[0 .. min(Fd, cap)) when w is not NULL; STN_ERR_INVALID when
 * fade_ms is outside [0, 50] or hz < 1 */
int stn_silence_fade_window(int hz, float fade_ms, float* w, int64_t cap, int64_t* n);
/* diagnostic: overwrite the finished batch's model-rate waveform with wav [B][L * chunk] (host; what stn_batch_dims reports at the model's
 * rate) and forget every fetch-time measurement cached for it.  For tests that need rows with known silences. */
int stn_dbg_batch_set_wav(stn_handle* h, const float* wav);
/* diagnostic: how often the handle has uploaded the finished batch's row spans (the n_b of "loudness") since it was created: once per
 * finished batch and (rate, row length) that a fetch, a report or a stage asked for, whatever the number of fetches (0 for NULL) */
int64_t stn_dbg_span_uploads(const stn_handle* h);

/* ---- pause limit -------------------------------------------------------------------------------------
 * With silence trimming on AND the pause limit on, every pause inside a row's speech that is longer than max_pause_ms is shortened to
 * max_pause_ms on the GPU at fetch time.  Without trimming the setting has no effect and adds no launch or allocation.  It uses
 * trimming's top_db, keep_ms and fade_ms and the same signal, span n, frames F, levels m_k, threshold, f0, f1, start and end.  The latent
 * geometry, the reported durations, the captured pipeline and the graph key are untouched; toggling it drops or re-captures no graph.
 * Pauses: a maximal run of inactive frames a .. b - 1 with f0 < a and b <= f1 (frames a - 1 and b are active); its samples are
 * [aF, bF), its length P = (b - a) F.  Mp = (int64_t)(max_pause_ms * hz / 1000 + 0.5) (in double).  A pause with P > Mp is cut: samples
 * [aF + hl, bF - hr) are dropped, hl = Mp - Mp / 2 and hr = Mp / 2, so exactly Mp samples of the row's own pause remain.  A pause with
 * P <= Mp, and a row without speech, is untouched.  At most 255 cuts are made per row: the first 255 in time order.
 * Segments: with cuts c_1 .. c_m the row's segments are [start, c_1.lo), [c_1.hi, c_2.lo), ..., [c_m.hi, end), laid end to end from
 * column 0; no silence is inserted.  Each segment edge made by a cut (and start > 0, end < n as under trimming) is faded over
 * min(Fd, segment length) samples with trimming's window and sample rule.  When Mp / 2 < Fd the fade reaches past the kept half of the
 * pause into the neighbouring speech frame; this is allowed.  len_b is the sum of the segment lengths.
 * Everything else follows trimming with len_b and the segment list in place of [start, end): per-row fetches deliver [B][W_out] with
 * zero codewords behind len_b and need no host read; joined fetches take a member's segments in order, its duration in prog_dur is
 * (float)len_b / (float)hz, and the plan reads the rows' cut lists with one device-to-host copy per finished batch and setting;
 * the per-row loudness gain stays the one of the untrimmed span; stn_batch_silence_edges keeps reporting start and end.  A row's table
 * depends on its own levels and the parameters only.  The group refuses the setting.  DESIGN.md section 17. */
/* on = 0: off (the default).  max_pause_ms in [20, 5000]; out of range: STN_ERR_INVALID with a message, and the previous setting stays. */
int stn_set_pause_limit(stn_handle* h, int on, float max_pause_ms);
int stn_get_pause_limit(const stn_handle* h, int* on, float* max_pause_ms);
/* the finished batch as the current trimming parameters and max_pause_ms cut it, whether either setting is on or not: len [B] = len_b,
 * n_cuts [B], and cuts_or_null [B][cap_pairs][2] = (lo, hi) of row b's first min(n_cuts[b], cap_pairs) cuts (the rest of a row's
 * pairs is left untouched).  Each pointer may be NULL. */
int stn_batch_pauses(stn_handle* h, int64_t* len, int32_t* n_cuts, int64_t* cuts_or_null, int cap_pairs);
/* op-level, on host operands as stn_op_silence_trim: y [rows][W] samples of enc, row r's segments end to end from column 0 (times
 * gain_or_null[r], cut edges faded), zero codewords behind len[r] */
int stn_op_pause_trim(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, float top_db, float keep_ms,
                      float fade_ms, float max_pause_ms, const float* gain_or_null, int enc, void* y, int64_t* start, int64_t* end,
                      int64_t* len, int32_t* n_cuts, int64_t* cuts_or_null, int cap_pairs);
/* the rule on the host, no device needed: n samples at hz in K = ceil(n / F) frames with levels level[K] -> start, end, *n_cuts and
 * cuts [cap_pairs][2] (the first min(*n_cuts, cap_pairs) pairs).  Each output pointer may be NULL.  STN_ERR_INVALID (why:
 * stn_pause_plan_error) for a parameter out of range or K != ceil(n / F). */
int stn_pause_plan(int hz, int64_t n, const double* level, int64_t K, float top_db, float keep_ms, float max_pause_ms, int64_t* start,
                   int64_t* end, int64_t* cuts, int cap_pairs, int32_t* n_cuts);
const char* stn_pause_plan_error(void);
/* The same detection (the same launches through the same launchers: the frame pass, the row pass and, with max_pause_ms > 0, the pause
 * pass) on host operands with its scratch laid open (the kernel tests of every pass).  n_or_null, top_db, keep_ms and fade_ms as
 * stn_op_silence_trim; max_pause_ms = 0: no pause pass (len = end - start, n_cuts = 0, cuts untouched), else as stn_op_pause_trim.
 * x_misalign 0 / 1: x is uploaded 16-byte aligned / 4 bytes off, which forces the scalar staging path at W % 4 == 0.  Before the first
 * launch every 32-bit word of the whole scratch (pa, pb, lev, the edges and the cut tables) is filled with 0x7FC00000 (a quiet NaN as a
 * float; two such words as a double are 2^1021 * 1.0000005, no level), so an element no launch wrote comes back as that.  With
 * Ks = (W + 31) / 32 chunks and Kf = ceil(W / F) frames per row: pa, pb [rows][Ks] (chunk k's sum of x^2 over its samples inside the
 * span that lie before the next frame boundary, and over those from it on); lev [rows][Kf] (the frame levels m_k); start, end, len,
 * n_cuts [rows] and cuts_or_null [rows][cap_pairs][2] as stn_op_pause_trim.  Every output may be NULL.  form: the staging path that ran, "vec" (16-byte
 * loads) or "scalar", NUL-terminated, truncated to form_cap; may be NULL.  Refuses what stn_op_silence_trim and (with max_pause_ms
 * != 0) stn_op_pause_trim refuse, and an x_misalign outside {0, 1}. */
int stn_op_silence_edges_ex(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, float top_db, float keep_ms,
                            float fade_ms, float max_pause_ms, int x_misalign, float* pa, float* pb, double* lev, int64_t* start,
                            int64_t* end, int64_t* len, int32_t* n_cuts, int64_t* cuts_or_null, int cap_pairs, char* form, size_t form_cap);

/* ---- limiter -----------------------------------------------------------------------------------------
 * A look-ahead peak limiter behind the loudness gain.  With the limiter on AND loudness on, the ceiling of stn_set_loudness is enforced
 * by the limiter and no longer by capping the gain: a row gets the full loudness gain, and only the few milliseconds around a sample
 * above the ceiling are turned down, smoothly, so that nothing exceeds it.  With loudness off the setting has no effect and adds no
 * launch.  It composes with the rate, the encoding, the trimming and the join; the latent geometry, the reported durations,
 * stn_batch_wav_device_ptr, the captured pipeline and the graph key are untouched, and toggling it drops or re-captures no graph.
 * For a row at the output rate hz: n its span (the loudness span n_b), g = 10^((target - L) / 20) the UNCAPPED gain (1 when L is -inf),
 * c = float32(10^(ceiling / 20)), A = (int64_t)(lookahead_ms * hz / 1000 + 0.5) (in double), and
 *   v[i] = x[i] * g (one fp32 multiply);
 *   r[j] = 1 where |v[j]| <= c, else c / |v[j]| (one fp32 divide), for 0 <= j < n; r[j] = 1 outside [0, n);
 *   m[i] = min r[i .. i+A],  M[i] = min r[i-A .. i+A];
 *   w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (A + 2)), k = 0 .. A, normalized to sum 1 in double, stored as fp32 (stn_limiter_window);
 *   s[i] = 1 exactly when M[i] == 1; otherwise s[i] = min(sum_k w[k] m[i-k], r[i], 1 - 2^-24), the sum in fp32 in an order fixed by
 *   the sample's position (every m[i-k] covers sample i, so s[i] <= r[i]; the last operand keeps s < 1 wherever M < 1 when the sum
 *   rounds to 1); the sum is within (A + 8) * 2^-24 of its exact value;
 *   y[i] = clamp(v[i] * s[i], -c, c) for i < n, and clamp(v[i], -c, c) for the padding i >= n;
 * then the trim fades and the encoding's rule as without it.  So |y| <= c exactly for every delivered fp32 sample; a row with
 * g * peak <= c is byte for byte the loudness-only fetch (same g, s = 1); and a row's output depends on its first n samples, the rate
 * and the parameters only, not on W, B or its neighbours (no float atomics).  The loudness of a limited row ends slightly under the
 * target; that is reported (stn_batch_limiter), not iterated away.
 * Trimmed rows: the limiter runs on the untrimmed span, as the gain measurement does; with fade_ms = 0 a trimmed row stays a slice of
 * the untrimmed fetch.  Joined fetches: with STN_JOIN_GAIN_ROW the segments are the limited rows; with STN_JOIN_GAIN_PROG the joined,
 * faded fp32 signal is limited as G rows, each with its programme gain and span.  No host read is added, so the pipelined _begin stays
 * asynchronous.  While the limiter is active stn_batch_loudness and stn_batch_join_loudness report the gain actually applied, the
 * uncapped one.  DESIGN.md section 15 has the decomposition and the cost. */
/* on = 0: off (the default: every fetch is byte for byte the one without it, with no extra launch or allocation).  lookahead_ms in
 * [0.5, 10]; out of range: STN_ERR_INVALID with a message, and the previous setting stays in force. */
int stn_set_limiter(stn_handle* h, int on, float lookahead_ms);
int stn_get_limiter(const stn_handle* h, int* on, float* lookahead_ms);
/* the finished batch as the current setting limits it: per row the deepest reduction -20 log10(min s) in dB and the number of samples
 * of the span with M < 1 (both 0 while the limiter or loudness is off); each pointer [B] or NULL */
int stn_batch_limiter(stn_handle* h, float* reduction_db, int64_t* limited);
/* op-level: rows x W fp32 (host) at hz in [8000, 192000]; row r's first n[r] samples (n_or_null = NULL: all W) times gain_or_null[r]
 * (NULL: 1) limited to ceiling_dbfs in [-30, 0] -> y and the curve s, [rows][W] floats each (s_or_null may be NULL), reduction_db and
 * limited [rows] (either may be NULL).  1 <= rows <= 65535. */
int stn_op_limiter(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, const float* gain_or_null,
                   float ceiling_dbfs, float lookahead_ms, float* y, float* s_or_null, float* reduction_db, int64_t* limited);
/* the weights at hz (host only, no device needed): *n = A + 1, and w[0 .. min(A + 1, cap)) when w is not NULL; STN_ERR_INVALID when
 * lookahead_ms is outside [0.5, 10] or hz outside [8000, 192000] */
int stn_limiter_window(int hz, float lookahead_ms, float* w, int64_t cap, int64_t* n);

/* ---- true peak ---------------------------------------------------------------------------------------
 * The ceiling of stn_set_loudness as a TRUE-peak ceiling (dBTP, ITU-R BS.1770-4 Annex 2: the peak of the 4x oversampled signal), which
 * is what a DAC, a codec or a later resampler sees; speech has inter-sample peaks 0.5 to 3 dB above its sample peaks.  The default,
 * STN_PEAK_SAMPLE, is the sample-peak ceiling described above.  The mode has no effect while loudness is off; it composes with the rate,
 * the encoding, the trimming, the limiter and the join; the latent geometry, the reported durations, stn_batch_wav_device_ptr, the
 * captured pipeline and the graph key are untouched, and toggling it drops or re-captures no graph.
 * Filter (stn_true_peak_filter): P = 4 phases of T = 16 taps, off = 7; tap j of phase p sits d = p - (j - 7) * 4 quarter samples from
 * the output instant, h = sinc(d / 4) * I0(8 sqrt(1 - (d / 32)^2)) / I0(8) (Kaiser window, beta = 8, cutoff at the input Nyquist; sinc
 * exactly 0 at the non-zero integers), every phase normalized in double to a DC gain of 1 and stored as fp32.  Phase 0 is the unit tap.
 * The filter lives in normalized frequency: the same 64 floats serve every rate in [8000, 192000].
 * For a row with span n (the loudness span n_b), with x = 0 outside [0, n):
 *   u[i][ph] = sum_{j = 0..15} taps[ph][j] * x[i - 7 + j], one fp32 FMA chain with j ascending, for ph in {1, 2, 3} and i in [-1, n - 1]:
 *   the value at i + ph/4;  U[i] = max_ph |u[i][ph]|;
 *   envelope p[i] = max(|x[i]|, U[i-1], U[i]) for 0 <= i < n (every oversampled point strictly between i - 1 and i + 1), and
 *   p[i] = |x[i]| for i >= n;
 *   tp = max_{i < n} p[i] (0 when n = 0);  per chunk of 32 samples from sample 0, pk[k] = max p[i] over the chunk's samples inside the
 *   span, +0.0 when there are none.
 * Every value depends on the row's first n samples only, not on W, B or the row's neighbours (one chain order; max is exact).
 * Loudness without the limiter: g_b = min(10^((target - L_b) / 20), c / tp_b), and stn_batch_loudness / stn_batch_join_loudness
 * report tp_b as the peak.  With the limiter: the curve of "limiter" above with r[j] = 1 where e[j] <= c and c / e[j] elsewhere, e the
 * envelope of v = x * g (r = 1 outside [0, n)); everything else of that contract is unchanged (m, M, w, s, y = clamp(v s, -c, c)).
 * Modulating by s moves inter-sample peaks a little, so the limited row's true peak tp_y is measured and the delivered fp32 row is
 * y * trim, trim = 1 where tp_y <= c, else c / tp_y (one fp32 divide, one fp32 multiply per sample); the trim is reported
 * (stn_batch_true_peak).  While the limiter is active the peak stn_batch_loudness reports stays the sample peak (nothing caps the gain).
 * Trimmed fetches measure and limit the untrimmed span; STN_JOIN_GAIN_ROW joins the limited, trimmed-gain rows; STN_JOIN_GAIN_PROG runs
 * all of it on the G joined rows.  No host read is added, so the pipelined _begin stays asynchronous.  DESIGN.md section 16 has the
 * decomposition, the filter's measured response and the traffic. */
#define STN_PEAK_SAMPLE 0
#define STN_PEAK_TRUE 1
/* any other value: STN_ERR_INVALID with a message, and the previous setting stays in force */
int stn_set_peak_mode(stn_handle* h, int mode);
/* the mode, or STN_ERR_INVALID for a NULL handle */
int stn_get_peak_mode(const stn_handle* h);
/* the oversampling filter (host only, no device needed): *phases = 4, *taps_per_phase = 16, taps [4][16] when taps_or_null is not NULL
 * and cap >= 64 (STN_ERR_INVALID when cap is smaller) */
int stn_true_peak_filter(float* taps_or_null, size_t cap, int* phases, int* taps_per_phase);
/* A reporting call, as stn_batch_loudness and stn_batch_limiter are: it runs the output stage's measurement again on the handle's
 * stream (with the limiter on, the whole limiter chain and three true-peak passes), overwrites what those two calls last left in the
 * shared fetch scratch, and synchronizes.  The finished batch at the current output rate, in any mode and whether loudness is on or
 * not: tp_in, the true peak of the measured row; tp_out, the true peak of the fp32 row a per-row fetch without trimming delivers under the current settings; trim, 1 except with
 * the limiter in true mode; each pointer [B] floats or NULL */
int stn_batch_true_peak(stn_handle* h, float* tp_in, float* tp_out, float* trim);
/* op-level: rows x W fp32 (host) at hz in [8000, 192000] (checked; the result does not depend on it); row r's first n[r] samples
 * (n_or_null = NULL: all W) times gain_or_null[r] (NULL: 1; one fp32 multiply) -> tp [rows], env [rows][W] (the envelope p) and pk
 * [rows][(W + 31) / 32]; each may be NULL.  Before the launches the device's tp, env and pk are filled with the quiet NaN 0x7FC00000.
 * x_misalign 0 / 1: x is uploaded 16-byte aligned / 4 bytes off, which forces the scalar staging path at W % 4 == 0.  form: the staging
 * path that ran, "vec" (16-byte loads and stores) or "scalar", NUL-terminated, truncated to form_cap; may be NULL.  1 <= rows <= 65535. */
int stn_op_true_peak(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, const float* gain_or_null,
                     int x_misalign, float* tp, float* env_or_null, float* pk_or_null, char* form, size_t form_cap);
/* stn_op_limiter under a peak mode.  STN_PEAK_SAMPLE: stn_op_limiter, trim = 1, env untouched.  STN_PEAK_TRUE: the curve follows the
 * envelope of x * gain (env_or_null [rows][W]); y is the limited row BEFORE the trim, and trim_or_null [rows] the scalar a fetch then
 * applies. */
int stn_op_limiter_ex(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n_or_null, const float* gain_or_null,
                      float ceiling_dbfs, float lookahead_ms, float* y, float* s_or_null, float* reduction_db, int64_t* limited,
                      int peak_mode, float* env_or_null, float* trim_or_null);

/* ---- filter chain -----------------------------------------------------------------------------------
 * A chain of 1 to STN_MAX_FILTERS second-order sections (biquads) applied to every row of every fetch, on the GPU, at the output rate:
 * a high-pass / DC blocker in front of the level-based steps, the telephone band in front of G.711, tone shaping.  Off (n = 0) is the
 * default: every fetch is then byte for byte the one without the feature, and no filter launch runs.
 * Order of the output stage: native rows -> resample (if a rate is set) -> FILTER CHAIN -> silence edges / pause cuts -> loudness
 * measurement -> gain / limiter / true peak -> encoding store / join.  Everything behind the chain sees the filtered signal: every
 * fetch path (synchronous, both pipelined slots, device copies, joined, the group's gather) and every report (stn_batch_loudness,
 * _silence_edges, _pauses, _limiter, _true_peak, stn_batch_join_loudness).  stn_batch_wav_device_ptr, stn_batch_fetch_latent, the
 * batch's own waveform, the captured pipeline and the graph key are untouched: the filtered rows live in fetch scratch, and setting,
 * changing or clearing the chain drops or re-captures no graph.
 * Each row is filtered on its own, causally, from zero state at its sample 0, over the row's whole width W_out (padding included; the
 * tail that decays into the padding is delivered like any other sample).  Identities:
 *   the delivered fp32 row == stn_op_filter(the fp32 row delivered with the chain off), bit for bit;
 *   a row's first n samples do not depend on W, the batch or the row's place in it;
 *   a joined fetch == the host join of the per-row fetch, byte for byte, as without the chain.
 * Section: transposed direct form II in fp32 with fp32 coefficients (b0 b1 b2 a1 a2, a0 = 1),
 *   y = fma(b0, u, s1);  s1 = fma(-a1, y, fma(b1, u, s2));  s2 = fma(-a2, y, b2 * u),
 * the signal between sections fp32.  The reference of every numeric claim is this recurrence in float64 on the same fp32-rounded
 * coefficients.  Design: the RBJ Audio-EQ-Cookbook forms in double, w0 = 2 pi freq_hz / rate, alpha = sin(w0) / (2 q),
 * A = 10^(gain_db / 40), normalized by a0 (stn_filter_coefs); HIGHPASS, LOWPASS and NOTCH ignore gain_db.
 * Refused with STN_ERR_INVALID and a message that names the field, against the output rate in force: n outside [0, STN_MAX_FILTERS],
 * an unknown type, q outside [0.3, 8], |gain_db| > 18, freq_hz above 0.45 rate, and freq_hz below rate / 2400 (high-pass and low-pass
 * with q in [0.5, 1.5]) or rate / 800 (every other filter): below those corners the fp32 rounding of the coefficients moves the
 * response by more than 0.1 dB.  The previous chain stays in force.  stn_set_output_rate to a rate at which the chain in force breaks
 * a limit is refused the same way, and the rate stays as it was.  DESIGN.md section 18 has the decomposition and the measurements. */
#define STN_FILT_HIGHPASS 0
#define STN_FILT_LOWPASS 1
#define STN_FILT_NOTCH 2
#define STN_FILT_PEAK 3
#define STN_FILT_LOWSHELF 4
#define STN_FILT_HIGHSHELF 5
#define STN_MAX_FILTERS 8
typedef struct stn_filter { int type; float freq_hz; float q; float gain_db; } stn_filter;
/* n = 0 (f may then be NULL): off */
int stn_set_filters(stn_handle* h, int n, const stn_filter* f);
/* *n and out[0 .. *n); out holds STN_MAX_FILTERS entries; either may be NULL */
int stn_get_filters(const stn_handle* h, int* n, stn_filter* out);
/* op-level: rows x W fp32 (host) at hz through the chain f[0 .. n), 1 <= n <= STN_MAX_FILTERS -> y [rows][W] (host).  1 <= rows <= 65535. */
int stn_op_filter(stn_handle* h, int hz, int rows, int W, const float* x, int n, const stn_filter* f, float* y);
/* The same with its scratch laid open (the kernel tests).  The chain runs as P = (n + 1) / 2 section passes of two biquads (an odd n
 * padded with the identity biquad), each three launches: chunks of 32 samples from zero state, the scan of the chunk states in double,
 * the chunks again from their start states, writing y.  st_end [P][rows][Ks][4] (Ks = (W + 31) / 32): pass p's chunk end states as its
 * first launch left them; st_start, the same shape: its chunks' start states (s1, s2 of the first biquad, then of the second) after the
 * scan.  Either may be NULL.  The device's state buffer is filled with the quiet NaN 0x7FC00000 before every pass, and x and y lie with
 * 64 poisoned floats in front of and behind them: *guard_ok = 1 when all of those came back untouched.  x_misalign 0 / 1: x and y lie
 * 16-byte aligned / 4 bytes off, which forces the scalar staging path at W % 4 == 0.  form: the staging path that ran, "vec" or
 * "scalar", NUL-terminated, truncated to form_cap; may be NULL. */
int stn_op_filter_ex(stn_handle* h, int hz, int rows, int W, const float* x, int n, const stn_filter* f, int x_misalign, float* y,
                     float* st_end, float* st_start, int* guard_ok, char* form, size_t form_cap);
/* host only, no device needed: the section at rate_hz.  c: b0 b1 b2 a1 a2 of the double design; c32: the same rounded to fp32, what
 * the GPU multiplies by.  Either may be NULL.  Refuses (STN_ERR_INVALID) what stn_set_filters refuses at that rate. */
int stn_filter_coefs(const stn_filter* f, int rate_hz, double c[5], float c32[5]);
/* host only: why stn_set_filters would refuse f[0 .. n) at an output rate of rate_hz ("" when it would not), as stn_resample_error;
 * the string is the calling thread's until its next call */
const char* stn_filter_error(int n, const stn_filter* f, int rate_hz);
/* host only: the magnitude response in dB of the fp32-rounded chain (what is actually run) at freq_hz[0 .. n_freq) */
int stn_filter_response(int n, const stn_filter* f, int rate_hz, int n_freq, const double* freq_hz, double* mag_db);
/* the decomposition's constants: samples per chunk, samples a workgroup of the chunk launches owns, chunks per scan tile, biquads per
 * section pass; each may be NULL */
int stn_dbg_filter_geometry(int* chunk, int* wg_span, int* scan_tile_chunks, int* biquads_per_section);

/* ---- compressor --------------------------------------------------------------------------------------
 * A feed-forward, log-domain dynamic range compressor (Giannoulis, Massberg and Reiss, "Digital Dynamic Range Compressor Design", JAES
 * 2012: level detector behind the gain computer, decoupled peak detector) applied to every row of every fetch, on the GPU, at the
 * output rate: it narrows the distance between the loud and the quiet parts of an utterance, in front of G.711's 38 dB, for playback in
 * noise, and so that the limiter is left the clicks.  Off is the default: every fetch is then byte for byte the one without the
 * feature, and no compressor launch runs.
 * Order of the output stage: native rows -> resample (if a rate is set) -> filter chain -> COMPRESSOR -> silence edges / pause cuts ->
 * loudness measurement -> gain / limiter / true peak -> encoding store / join.  Everything behind it sees the compressed signal: every
 * fetch path (synchronous, both pipelined slots, device copies, joined, the group's gather) and every report (stn_batch_loudness,
 * _silence_edges, _pauses, _limiter, _true_peak, stn_batch_join_loudness).  One consequence: the silence trim's top_db is then relative
 * to the loudest frame of the compressed signal, in which level differences above the threshold are smaller by the ratio.
 * stn_batch_wav_device_ptr, stn_batch_fetch_latent, the batch's own waveform, the captured pipeline and the graph key are untouched: the
 * compressed rows live in fetch scratch, and changing the setting drops or re-captures no graph.
 * Each row is compressed on its own, from y1 = yL = 0 at its sample 0, over the row's whole width W_out (padding included).  Per
 * sample, all values fp32:
 *   level          xG = 20 log10(max(|x|, 1e-6))
 *   gain computer  T = threshold_db, S = 1 / ratio - 1, K = knee_db, d = xG - T:
 *                  z = 0 when 2 d < -K;  z = -S (d + K / 2)^2 / (2 K) when 2 |d| <= K (and K > 0);  z = -S d otherwise   (z >= 0, dB)
 *   detector       y1 = max(z, fma(-kR, y1, y1));  yL = fma(kA, y1 - yL, yL);  k = -expm1(-1000 / (ms rate)), formed in double and
 *                  rounded to fp32 (the k form, not alpha = 1 - k: at a 3 s release and 192 kHz the fp32 neighbours of alpha are 3 %
 *                  apart in time constant)
 *   output         y = x 10^((makeup_db - yL) / 20)
 * The reference of every numeric claim is exactly this in float64 on the same fp32-rounded T, S, K, kA, kR and makeup.  Identities:
 *   the delivered fp32 row == stn_op_compressor(the fp32 row delivered with the compressor off), bit for bit;
 *   a row's first n samples do not depend on W, the batch or the row's place in it;
 *   a joined fetch == the host join of the per-row fetch, byte for byte, as without the compressor.
 * Refused with STN_ERR_INVALID and a message that names the field: threshold_db outside [-60, 0], ratio outside [1, 20], knee_db
 * outside [0, 24], attack_ms outside [0.1, 300], release_ms outside [10, 3000], makeup_db outside [-12, 24], a non-finite field.  The
 * previous setting stays in force.  None of the limits depends on the rate, so stn_set_output_rate never refuses on the compressor's
 * account.  DESIGN.md section 20 has the decomposition and the measurements. */
typedef struct stn_compressor { float threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db; } stn_compressor;
/* on = 0: off, c may then be NULL (the values last set stay readable) */
int stn_set_compressor(stn_handle* h, int on, const stn_compressor* c);
/* either may be NULL; *out: the values last set (before the first set: -24 dB, 3:1, knee 6 dB, 5 ms, 120 ms, 0 dB) */
int stn_get_compressor(const stn_handle* h, int* on, stn_compressor* out);
/* per row of the finished batch: the maximum of yL, the reduction in dB, over the row's valid samples (its reported duration at the
 * output rate); 0 for every row while the compressor is off */
int stn_batch_compressor(stn_handle* h, float* max_reduction_db);
/* op-level: rows x W fp32 (host) at hz through the compressor c -> y [rows][W] (host).  1 <= rows <= 65535. */
int stn_op_compressor(stn_handle* h, int hz, int rows, int W, const float* x, const stn_compressor* c, float* y);
/* The same with its scratch laid open (the kernel tests).  Five launches on chunks of 32 samples (Ks = (W + 31) / 32 per row): y1 of
 * every chunk from zero (s1_end), the (max, x) scan of those in double (s1_start: y1 at every chunk's start), yL of every chunk from
 * zero on its true y1 (s2_end), the linear scan in double (s2_start), and the write pass from both start values: y, and gr_db
 * [rows][W] = yL.  Each of gr_db, s1_end, s1_start, s2_end, s2_start ([rows][Ks] each) may be NULL.  The device's scratch and gr_db
 * are filled with the quiet NaN 0x7FC00000 before the first launch, and x and y lie with 64 poisoned floats in front of and behind
 * them: *guard_ok = 1 when all of those came back untouched.  x_misalign 0 / 1: x and y lie 16-byte aligned / 4 bytes off, which forces
 * the scalar staging path at W % 4 == 0.  in_place 0 / 1: y is written to rows of its own / over x on the device.  form: the staging
 * path that ran, "vec" or "scalar", NUL-terminated, truncated to form_cap; may be NULL. */
int stn_op_compressor_ex(stn_handle* h, int hz, int rows, int W, const float* x, const stn_compressor* c, int x_misalign, int in_place,
                         float* y, float* gr_db, float* s1_end, float* s1_start, float* s2_end, float* s2_start, int* guard_ok, char* form,
                         size_t form_cap);
/* host only, no device needed: kA and kR at rate_hz.  k: -expm1(-1000 / (ms rate)) in double; k32: the same rounded to fp32, what the
 * GPU multiplies by.  Either may be NULL.  Refuses (STN_ERR_INVALID) what stn_set_compressor refuses, and a rate outside [8000, 192000]. */
int stn_compressor_coefs(const stn_compressor* c, int rate_hz, double k[2], float k32[2]);
/* host only: the static curve, makeup included: out_db[i] = in_db[i] - z(in_db[i]) + makeup_db, in double on the fp32 T, S, K, makeup */
int stn_compressor_curve(const stn_compressor* c, int n, const double* in_db, double* out_db);
/* host only: why stn_set_compressor would refuse c ("" when it would not), as stn_filter_error; rate_hz > 0 is checked as well, 0 is
 * "no rate"; the string is the calling thread's until its next call */
const char* stn_compressor_error(const stn_compressor* c, int rate_hz);

/* ---- de-esser -----------------------------------------------------------------------------------------
 * A split-band de-esser applied to every row of every fetch, on the GPU, at the output rate: the compressor's detector listens to a
 * band of the signal (everything above freq_hz, a 4th-order Butterworth high-pass) and its gain turns down that band alone (split) or
 * the whole signal (wide), and only while a sibilant happens.  The filter chain is linear and cannot do that; the compressor detects on
 * the full band, where a vowel hides the "s".  Off is the default: every fetch is then byte for byte the one without the feature, and
 * no de-esser launch runs.
 * Order of the output stage: native rows -> resample (if a rate is set) -> filter chain -> DE-ESSER -> compressor -> silence edges /
 * pause cuts -> loudness measurement -> gain / limiter / true peak -> encoding store / join.  Everything behind it sees the de-essed
 * signal: every fetch path and every report (stn_batch_compressor, _loudness, _silence_edges, _pauses, _limiter, _true_peak,
 * stn_batch_join_loudness).  stn_batch_wav_device_ptr, stn_batch_fetch_latent, the batch's own waveform, the captured pipeline and the
 * graph key are untouched: the de-essed rows live in fetch scratch, and changing the setting drops or re-captures no graph.
 * Each row is de-essed on its own, from zero state at its sample 0, over the row's whole width W_out (padding included).  Per sample,
 * all values fp32:
 *   band           h  = HP4(x): two RBJ high-pass biquads at freq_hz with q = (float)0.54119610 and (float)1.30656296 (4th-order
 *                  Butterworth), designed in double and rounded to fp32 exactly as stn_filter_coefs does, run as ONE section pass of
 *                  the chain's 4-state system (the arithmetic of "filter chain", operation for operation)
 *   level          hG = 20 log10(max(|h|, 1e-6))
 *   gain computer  z  = min(range_db, zc(hG)),  zc the compressor's curve with T = threshold_db, S = 1 / ratio - 1, K = knee_db
 *   detector       y1 = max(z, fma(-kR, y1, y1));  yL = fma(kA, y1 - yL, yL),  k as stn_compressor_coefs forms it
 *   output         g  = 10^(-yL / 20)
 *                  STN_DEESS_SPLIT:  y = fma(-(1 - g), h, x)   only the band is turned down; where g == 1 (yL == 0) y is x itself,
 *                                    bit for bit, the sign of a zero included
 *                  STN_DEESS_WIDE:   y = x g
 * The reference of every numeric claim is exactly this in float64 on the same fp32-rounded coefficients.  Identities:
 *   the delivered fp32 row == stn_op_deesser(the fp32 row delivered with the de-esser off), bit for bit;
 *   a row's first n samples do not depend on W, the batch or the row's place in it;
 *   a joined fetch == the host join of the per-row fetch, byte for byte, as without the de-esser;
 *   in split mode a row whose band never reaches the knee is delivered bit for bit as without the feature.
 * Refused with STN_ERR_INVALID and a message that names the field: freq_hz outside [2000, 12000], above 0.45 x the output rate or below
 * the output rate / 2400 (the chain's corners for a high-pass with q in [0.5, 1.5]); threshold_db outside [-60, 0], ratio outside
 * [1, 20], knee_db outside [0, 24], attack_ms outside [0.1, 300], release_ms outside [10, 3000], range_db outside [1, 24]; an unknown
 * mode; a non-finite field.  The previous setting stays in force.  stn_set_output_rate to a rate at which the de-esser in force breaks
 * a limit is refused the same way, and the rate stays as it was (the speech default is refused at 8 kHz).  DESIGN.md section 21 has the
 * decomposition and the measurements. */
#define STN_DEESS_SPLIT 0
#define STN_DEESS_WIDE 1
typedef struct stn_deesser { float freq_hz, threshold_db, ratio, knee_db, attack_ms, release_ms, range_db; int mode; } stn_deesser;
/* on = 0: off, c may then be NULL (the values last set stay readable) */
int stn_set_deesser(stn_handle* h, int on, const stn_deesser* c);
/* either may be NULL; *out: the values last set (before the first set, the speech default: 5500 Hz, -30 dB, 4:1, knee 6 dB, 1 ms,
 * 40 ms, range 12 dB, split) */
int stn_get_deesser(const stn_handle* h, int* on, stn_deesser* out);
/* per row of the finished batch: the maximum of yL, the reduction in dB, over the row's valid samples (its reported duration at the
 * output rate); 0 for every row while the de-esser is off */
int stn_batch_deesser(stn_handle* h, float* max_reduction_db);
/* op-level: rows x W fp32 (host) at hz through the de-esser c -> y [rows][W] (host).  1 <= rows <= 65535. */
int stn_op_deesser(stn_handle* h, int hz, int rows, int W, const float* x, const stn_deesser* c, float* y);
/* The same with its scratch laid open (the kernel tests).  Eight launches on chunks of 32 samples (Ks = (W + 31) / 32 per row): the
 * band's state of every chunk from zero (st_end) and its scan in double (st_start: the state at every chunk's start; both
 * [rows][Ks][4] = s1 s2 t1 t2, as stn_op_filter_ex); y1 of every chunk from zero (s1_end), the (max, x) scan (s1_start), yL of every
 * chunk from zero on its true y1 (s2_end), the linear scan (s2_start; these four [rows][Ks]); the write pass from every start value:
 * y, band [rows][W] = h and gr_db [rows][W] = yL; and the row maxima.  Each of band, gr_db and the six state arrays may be NULL.  The
 * device's scratch, band and gr_db are filled with the quiet NaN 0x7FC00000 before the first launch, and x and y lie with 64 poisoned
 * floats in front of and behind them: *guard_ok = 1 when all of those came back untouched.  x_misalign, in_place, form: as
 * stn_op_compressor_ex. */
int stn_op_deesser_ex(stn_handle* h, int hz, int rows, int W, const float* x, const stn_deesser* c, int x_misalign, int in_place, float* y,
                      float* band, float* gr_db, float* st_end, float* st_start, float* s1_end, float* s1_start, float* s2_end,
                      float* s2_start, int* guard_ok, char* form, size_t form_cap);
/* host only, no device needed: the band's two sections at rate_hz, b0 b1 b2 a1 a2 each.  c: the double design; c32: the same rounded
 * to fp32, what the GPU multiplies by.  Either may be NULL.  Refuses (STN_ERR_INVALID) what stn_set_deesser refuses at that rate. */
int stn_deesser_band(const stn_deesser* c, int rate_hz, double c10[10], float c32[10]);
/* host only: kA and kR at rate_hz, as stn_compressor_coefs */
int stn_deesser_coefs(const stn_deesser* c, int rate_hz, double k[2], float k32[2]);
/* host only: why stn_set_deesser would refuse c at an output rate of rate_hz ("" when it would not); rate_hz = 0 is "no rate": the
 * limits that do not depend on it; the string is the calling thread's until its next call */
const char* stn_deesser_error(const stn_deesser* c, int rate_hz);

/* ---- expander -----------------------------------------------------------------------------------------
 * A feed-forward, log-domain downward expander / noise gate applied to every row of every fetch, on the GPU, at the output rate: it
 * turns down what lies under a threshold (the vocoder's noise floor between words and around an utterance), by up to range_db, in
 * front of the compressor's make-up gain, the loudness gain and G.711's finest segments.  A high ratio and no knee make it a gate.
 * Off is the default: every fetch is then byte for byte the one without the feature, no expander launch runs and no scratch is owned.
 * Order of the output stage: native or pitch-shifted rows -> resample (if a rate is set) -> filter chain -> EXPANDER -> de-esser ->
 * compressor -> silence edges / pause cuts -> loudness measurement -> gain / limiter / true peak -> encoding store / join.  A DC
 * blocker or rumble filter in the chain keeps an offset from holding it open.  Everything behind it sees the expanded signal: every
 * fetch path and every report (stn_batch_deesser, _compressor, _loudness, _silence_edges, _pauses, _limiter, _true_peak,
 * stn_batch_join_loudness).  One consequence: the silence trim's levels are then those of the gated signal, whose quiet frames lie up
 * to range_db lower.  stn_batch_wav_device_ptr, stn_batch_fetch_latent, the batch's own waveform, the captured pipeline and the graph
 * key are untouched: the expanded rows live in fetch scratch, and changing the setting drops or re-captures no graph.
 * Each row is expanded on its own, from u = yL = 0 at its sample 0, over the row's whole width W_out (padding included): a row starts
 * CLOSED, so a row that begins with speech gets an attack-long fade-in (the "from zero state" convention of the filter chain, the
 * compressor and the de-esser).  Per sample, all values fp32:
 *   level          xG = 20 log10(max(|x|, 1e-6));  d = T - xG   (how far UNDER the threshold)
 *   gain computer  T = threshold_db, S = ratio - 1, K = knee_db, R = range_db:
 *                  z = 0 when 2 d < -K;  z = S (d + K / 2)^2 / (2 K) when 2 |d| <= K (and K > 0);  z = S d otherwise;  z = min(z, R)
 *   openness       o = R - z in [0, R];  t = o + Bh where z == 0 (fully open), t = o elsewhere
 *   detector       u = max(t, u - delta): it opens at once, holds, then closes at a constant rate in dB;  y1 = min(u, R)
 *   smoothing      yL = fma(kA, y1 - yL, yL)   (the attack)
 *   output         y = x 10^((yL - R) / 20)    (attenuation R - yL, between 0 and R dB in the reference; see stn_batch_expander for the
 *                                              few fp32 spacings of R by which the GPU's yL may exceed R)
 * with kA = -expm1(-1000 / (attack_ms rate)), delta = R 1000 / (release_ms rate) dB per sample (release_ms: the time a fully open gate
 * takes to close through the whole range), Hs = floor(hold_ms rate / 1000 + 0.5) samples and Bh = delta32 Hs, each formed in double
 * and rounded to fp32.  After the last fully open sample y1 stays at R for Hs samples (exact arithmetic), then falls to 0 over
 * release_ms; a zero crossing of the waveform is bridged by the detector.
 * The reference of every numeric claim is exactly this in float64 on the same fp32-rounded T, S, K, R, kA, delta and Bh.  Identities:
 *   the delivered fp32 row == stn_op_expander(the fp32 row delivered with the expander off), bit for bit;
 *   a row's first n samples do not depend on W, the batch or the row's place in it;
 *   a joined fetch == the host join of the per-row fetch, byte for byte, as without the expander (rows are gated one by one).
 * Refused with STN_ERR_INVALID and a message that names the field: threshold_db outside [-90, -10], ratio outside [1, 20], knee_db
 * outside [0, 24], range_db outside [1, 80], attack_ms outside [0.1, 300], hold_ms outside [0, 500], release_ms outside [10, 3000], a
 * non-finite field.  The previous setting stays in force.  None of the limits depends on the rate.  DESIGN.md section 25 has the
 * decomposition and the measurements. */
typedef struct stn_expander { float threshold_db, ratio, knee_db, range_db, attack_ms, hold_ms, release_ms; } stn_expander;
/* on = 0: off, c may then be NULL (the values last set stay readable) */
int stn_set_expander(stn_handle* h, int on, const stn_expander* c);
/* either may be NULL; *out: the values last set (before the first set, the speech default: -50 dB, 3:1, knee 6 dB, range 24 dB, 1 ms,
 * 30 ms, 150 ms) */
int stn_get_expander(const stn_handle* h, int* on, stn_expander* out);
/* per row of the finished batch, over the row's valid samples (its reported duration at the output rate): the minimum of R - yL, the
 * least attenuation in dB (well above 0: the threshold sits above the speech), and the count of samples with yL <= R / 2.  Either may
 * be NULL; both are 0 for every row while the expander is off.  The minimum is reported as the GPU formed it, not clamped: a chunk's
 * start value of yL comes from a scan (E s + c with c rounded to fp32, the sum rounded once more) and may leave
 * yL an fp32 spacing of R above R on a fully open stretch, so a fully open row can report a slightly negative minimum (observed: one
 * spacing, -3.8e-6 dB at R = 60, a gain of 1 + 4.4e-7; the tests allow four) */
int stn_batch_expander(stn_handle* h, float* min_attenuation_db, int64_t* closed_samples);
/* op-level: rows x W fp32 (host) at hz through the expander c -> y [rows][W] (host).  1 <= rows <= 65535. */
int stn_op_expander(stn_handle* h, int hz, int rows, int W, const float* x, const stn_expander* c, float* y);
/* The same with its scratch laid open (the kernel tests).  Five launches on chunks of 32 samples (Ks = (W + 31) / 32 per row): u of
 * every chunk from zero (s1_end), the (max, +) scan of those in double (s1_start: u at every chunk's start), yL of every chunk from
 * zero on its true u (s2_end), the linear scan in double (s2_start), and the write pass from both start values: y, and open_db
 * [rows][W] = yL.  Each of open_db, s1_end, s1_start, s2_end, s2_start ([rows][Ks] each) may be NULL.  The device's scratch and
 * open_db are filled with the quiet NaN 0x7FC00000 before the first launch, and x and y lie with 64 poisoned floats in front of and
 * behind them: *guard_ok = 1 when all of those came back untouched.  x_misalign, in_place, form: as stn_op_compressor_ex. */
int stn_op_expander_ex(stn_handle* h, int hz, int rows, int W, const float* x, const stn_expander* c, int x_misalign, int in_place, float* y,
                       float* open_db, float* s1_end, float* s1_start, float* s2_end, float* s2_start, int* guard_ok, char* form,
                       size_t form_cap);
/* host only, no device needed: kA, delta and Bh at rate_hz, and Hs.  k: each in double (Bh from the fp32 delta); k32: the same rounded
 * to fp32, what the GPU computes with.  Each may be NULL.  Refuses (STN_ERR_INVALID) what stn_set_expander refuses, and a rate outside
 * [8000, 192000]. */
int stn_expander_coefs(const stn_expander* c, int rate_hz, double k[3], float k32[3], int64_t* hold_samples);
/* host only: the static curve: out_db[i] = in_db[i] - z(in_db[i]), in double on the fp32 T, S, K and R */
int stn_expander_curve(const stn_expander* c, int n, const double* in_db, double* out_db);
/* host only: why stn_set_expander would refuse c ("" when it would not), as stn_compressor_error; rate_hz > 0 is checked as well, 0 is
 * "no rate"; the string is the calling thread's until its next call */
const char* stn_expander_error(const stn_expander* c, int rate_hz);

/* ---- measurement: HIP-event timing of kernel families on the engine's own stream ------------------- */
int stn_profile_enable(stn_handle* h, int on);
int stn_profile_reset(stn_handle* h);
/* time only one kernel family ("stage.kernel", e.g. "vo.gemm_pw1_gelu"); NULL or "" = all families */
int stn_profile_filter(stn_handle* h, const char* family_or_null);
/* time only every n-th matching launch (n >= 1): a launch that carries events does not overlap its neighbours on the stream
   (~4 us each), so a timed region samples its dominant family instead of fencing every launch of it */
int stn_profile_sample(stn_handle* h, int every);
/* Launch log for profiler runs: while on (and profiling enabled) every kernel launch of this thread's engine calls is recorded
   as "family\tkernel\n" in dispatch order (family "-" outside a timed family); stn_launch_log returns the bytes needed and fills
   `out` when it fits.  tools/pmc_families.py aligns rocprofv3's per-dispatch rows with it.  Cleared by stn_profile_reset. */
int stn_launch_log_enable(stn_handle* h, int on);
int64_t stn_launch_log(stn_handle* h, char* out, size_t cap);
/* number of kernel families seen; then per index: name, total ms, launches, algorithmic flops and bytes */
int stn_profile_count(stn_handle* h);
int stn_profile_get(stn_handle* h, int idx, char* name, size_t name_cap, double* total_ms, int64_t* launches,
                    double* flops, double* bytes);

/* diagnostics (tools/xattn_hs_phases.py): with on != 0 every head-split cross-attention launch (stn_set_fused_xattn(h, 3), eager runs
   only) writes 8 shader-clock stamps per workgroup — entry, Wq in LDS, q projection done, K/V in LDS, attention done, Wo in LDS, end,
   and the workgroup's row-tile count — into one buffer; stn_dbg_xattn_hs_stamps copies the LAST launch's stamps (up to cap values)
   and returns how many workgroups that launch had. */
int stn_dbg_xattn_hs_enable(stn_handle* h, int on);
int64_t stn_dbg_xattn_hs_stamps(stn_handle* h, unsigned long long* out, size_t cap);
/* diagnostics (no device needed): the run length — frames per workgroup, 0 = the default of 32 — the estimator's fold + conv + LayerNorm kernel takes for a
   batch of these latent lengths on a device of `n_cu` compute units (one 1024-thread workgroup fills a CU: the grid is kept within ONE round of workgroups
   where a run of 40 or 48 frames achieves that; the results do not depend on the choice).  < 0: STN_ERR_INVALID. */
int stn_dbg_fold_run_frames(const int32_t* latent_lengths, int B, int n_cu);

/* ---- op-level entry points used by the kernel parity tests (host pointers) -------------------------- */
int stn_op_gemm(stn_handle* h, int dtype, int M, int N, int K, const float* A /*[M,K]*/, const float* W /*[N,K]*/,
                const float* bias_or_null, int act /*0 none,1 gelu,2 silu*/, float* out /*[M,N]*/);
/* One GEMM, acc[m][n] = sum_k A[m][k] W[n][k], through the engine's launcher with the epilogue fields the engine uses (the kernel parity tests
 * of every GEMM form).  Operands are rounded to the engine's format `dtype` first.  mode 0 (store): out[m*ldo + n] = act(acc + bias[n]) * keep(m),
 * stored as out_dtype (STN_DTYPE_F32 or `dtype` itself); mode 1 (residual): out[m*ldo + n] = (out + gamma[n] (acc + bias[n]) + rowvec[seq(m)][n])
 * * keep(m) in fp32; mode 2 (transposed store): out[(b*N + n)*L + t] = (acc + bias[n]) * keep(m) in fp32, row m = b*L + t.  act: 0 none,
 * 1 GELU, 2 SiLU, 3 GELU in the tanh form.  keep(m) = 0 where len[b] <= t (len: nseq entries, 0..L); seq(m) = row_b[m] (packed rows, M
 * entries in 0..nseq-1; not with len) or m / L.  rowvec: [nseq][N].  nt = 1: non-temporal 16-bit stores.  tr: -1 the launcher's choice,
 * 0 / 1 force the tiled kernels' 16-bit store through the fp32 slab / the transposed image.  `out` is the caller's whole buffer of out_elems
 * floats (modes 0, 1: at least M*ldo, ldo >= N; mode 2: at least ceil(M/L)*N*L, nseq >= ceil(M/L)): uploaded as given (rounded to
 * out_dtype first) and written back whole (16-bit values widened to fp32, exactly), so what lies around the written region can be checked.
 * form: the form that ran (as stn_dbg_gemm_form), NUL-terminated, truncated to form_cap; may be NULL. */
int stn_op_gemm_ex(stn_handle* h, int dtype, int M, int N, int K, const float* A /*[M,K]*/, const float* W /*[N,K]*/, int mode, int act,
                   int out_dtype, int ldo, const float* bias_or_null, const float* gamma_or_null, const int32_t* len_or_null, int L,
                   const int32_t* row_b_or_null, const float* rowvec_or_null, int nseq, int nt, int tr, float* out, int64_t out_elems,
                   char* form, size_t form_cap);
/* diagnostics (no device needed): the form the engine's GEMM launcher takes for this call — kernel family, tile template arguments
 * <BM,BN,WM,WN,NSTAGE,KS,ESZ> and configuration, 16-bit store form (tr = transposed image, slab = fp32 slab through LDS, lane = per-lane
 * stores) and split-K factor, e.g. "tiled<128,128,2,4,4,64,2> cfg8 tr", "ring_vec slab", "splitk6+tiled<64,64,2,2,4,32,4> slab".
 * Operands K-contiguous with lda = ldw = K and 16-byte aligned pointers; masked != 0: a row mask by length; tr as stn_op_gemm_ex.
 * Returns the string's length (written with its NUL when it fits in cap), < 0 on a call the launcher refuses (STN_ERR_INVALID). */
int stn_dbg_gemm_form(int dtype, int M, int N, int K, int mode, int out_dtype, int ldo, int masked, int tr, char* out, size_t cap);
/* diagnostics (no device needed): the form a ConvNeXt block's pointwise pair takes — "gemms" (two tiled GEMM launches; "gemms nt": pw1
 * stores its hidden activation non-temporally), "k4" (one fused launch) or "k4splitS" (S hidden shares, folded by the next reader of x).
 * stage: 1 vocoder, 2 estimator, 4 text encoder / duration predictor; M: the launch's rows; gate_rows > 0: the row count the K4
 * decision is taken on instead (a trimmed vocoder's dense B*T); packed: rows packed per sequence; k, max_dil: the stage's conv taps
 * and largest dilation; mask, min_rows, split_min_rows: as stn_set_fused_ffn / stn_set_fused_ffn_min_rows (defaults 9, 18432, 1);
 * nt_hints: the engine's non-temporal hints (default on).  Returns the string's length (written with its NUL when it fits in cap),
 * < 0 on invalid arguments (STN_ERR_INVALID). */
int stn_dbg_ffn_form(int dtype, int stage, int C, int I, int64_t M, int64_t gate_rows, int packed, int k, int max_dil, int mask,
                     int64_t min_rows, int64_t split_min_rows, int nt_hints, char* out, size_t cap);
/* device-resident timing of one GEMM shape on random operands; mode 0 = bias+GELU store, 1 = residual epilogue */
int stn_op_gemm_bench(stn_handle* h, int dtype, int M, int N, int K, int mode, int iters, double* avg_ms);
/* diagnostics: shader-clock phase stamps of ONE launch of the tiled GEMM kernel on this shape (mode as above).  out6 = mean
 * cycles to the first landed stage, in the K loop, in the epilogue; span of the whole grid; spread of workgroup entry times;
 * number of workgroups.  Cycles of the s_memtime counter (100 MHz on gfx950: 1 tick = 10 ns). */
int stn_op_gemm_phases(stn_handle* h, int dtype, int M, int N, int K, int mode, double* out6);
int stn_op_dwconv_ln(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, const float* x,
                     const float* w /*[C,k]*/, const float* bias, const float* ln_g, const float* ln_b, float* y);
/* same with per-sequence valid lengths (taps at t >= seqlen[b] read as zero, rows t >= seqlen[b] come back as zeros) */
int stn_op_dwconv_ln_ragged(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, const float* x,
                            const float* w /*[C,k]*/, const float* bias, const float* ln_g, const float* ln_b,
                            const int32_t* seqlen /*[B], 0..L*/, float* y);
/* One GEMM out = A W^T + bias (fp32 out) whose M rows are packed per sequence, stored through the slab epilogue's packed-row destination map (the
 * vocoder head): sequence b owns rows[b] consecutive rows of A (rows past their sum, up to M, are dead); row t of sequence b is stored at row
 * b*T + t of out [B,T,N] when t < valid[b] (0 <= valid[b] <= rows[b] <= T) and nowhere otherwise.  out: the caller's whole buffer of out_elems
 * >= B*T*N floats, uploaded as given and written back whole.  Each stored row has the bits stn_op_gemm_ex's plain store gives that row.
 * STN_ERR_INVALID for operands whose GEMM form has no slab epilogue (N % 8).  form as stn_op_gemm_ex. */
int stn_op_gemm_rows(stn_handle* h, int dtype, int M, int N, int K, const float* A, const float* W, const float* bias_or_null, int B,
                     const int32_t* rows, const int32_t* valid, int T, float* out, int64_t out_elems, char* form, size_t form_cap);
/* The same launcher on the caller's whole buffers (the kernel parity tests of every dwconv + LayerNorm form).  x: x_rows rows of C, uploaded as
 * given, padding rows included.  packed = 0: sequence b owns rows b*L .. b*L + L of x / y (seqlen optional; x_rows, y_rows >= B*L); packed != 0:
 * seqlen[b] consecutive rows in order (needs seqlen; B <= 1024; x_rows, y_rows >= their sum), L >= every length.  ln_only != 0: plain
 * LayerNorm over the B*L rows (w, bias, seqlen unused).  eps = 1e-6.  y: y_rows rows of C, the caller's whole buffer, uploaded as given
 * (rounded to dtype) and written back whole (16-bit values widened to fp32, exactly), so what lies outside the written rows can be checked.
 * form: the form that ran (as stn_dbg_dwconv_ln_form, or "layernorm"), NUL-terminated, truncated to form_cap; may be NULL. */
int stn_op_dwconv_ln_ex(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, const float* x, int64_t x_rows,
                        const float* w_or_null /*[C,k]*/, const float* bias_or_null, const float* ln_g, const float* ln_b,
                        const int32_t* seqlen_or_null, int packed, int ln_only, float* y, int64_t y_rows, char* form, size_t form_cap);
/* The tail-reading variant of the packed launch above (the dense vocoder trimmed to one receptive field): sequence b is the head of a row of
 * T >= L frames whose frames from seqlen[b] on are not stored; a tap at a frame tt >= seqlen[b] reads tail[min(T - 1 - tt, rf)] (tail: rf + 1
 * rows of C, indexed by the distance to the end of the row) and zero from T on; taps before the row's start read zero.  Packed rows only
 * (seqlen needed, B <= 1024, C <= 512, k in {5, 7}); x, y, form as in stn_op_dwconv_ln_ex; only the rows the sequences own are written. */
int stn_op_dwconv_ln_tail(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, const float* x, int64_t x_rows,
                          const float* w /*[C,k]*/, const float* bias, const float* ln_g, const float* ln_b, const int32_t* seqlen,
                          const float* tail /*[rf+1,C]*/, int T, int rf, float* y, int64_t y_rows, char* form, size_t form_cap);
/* diagnostics (no device needed): the length tables a batch run uploads in front of its pipeline (csrc/host/len_tables.hpp), built on the host
 * from the B latent lengths alone.  ve_rows: the estimator's packed row count with its dead rows (>= sum llen; 0: no row map); with_pairs:
 * the head-split cross-attention's pairing (needs ve_rows > 0); vo_form: 0 none, 1 / 2 the dense vocoder's trim extents (trim_len_kernel,
 * tail_form 0 / 1), 3 lengths scaled by ccf; T: vocoder frames of a padded row; rf: the vocoder's receptive field.  layout (9 words, may be
 * NULL): word offsets of seed, llen, ve_off [B+1], ve_row_b [ve_rows], pairs [B+2], vo_n [B], vo_valid [B], vo_off [B+1] (-1: not built) and
 * the total.  out (may be NULL; out_n >= total words): the block, the two seed words left as they are.  Returns the total, < 0 on a bad call. */
int64_t stn_dbg_len_tables(int B, const int32_t* llen, int ve_rows, int with_pairs, int vo_form, int ccf, int T, int rf, int32_t* layout,
                           int32_t* out, int64_t out_n);
/* diagnostics (no device needed): the form the engine's depthwise-conv + LayerNorm launcher takes for B sequences of L rows, C channels,
 * k taps, output format dtype, padded or packed rows: "v3<K,R>" (combs of R frames), "v3occ4<7,4>" (the same held to four waves per SIMD),
 * "v2<K>" or "generic".  Returns the string's length (written with its NUL when it fits in cap), < 0 on a call the launcher refuses
 * (STN_ERR_INVALID: C % 4, C > 1024, packed with C > 512 or k outside {5, 7}). */
int stn_dbg_dwconv_ln_form(int dtype, int B, int L, int C, int k, int packed, char* out, size_t cap);
/* The fold of a pending K4-split / head-split update fused with LayerNorm, on host operands: x [M,C] <- x + gamma * (((p0 + p1) + ...) + b2)
 * [+ rowvec[row_b[m]]] in fp32, y [M,C] = LayerNorm(x) * ln_g + ln_b in dtype (STN_DTYPE_BF16 or STN_DTYPE_F16; fp32 copy).  part [S,M,C]:
 * the partial sums, rounded to dtype first; S in {4, 8, 12, 24}.  rowvec [nseq,C] (row_b NULL: every row takes rowvec[0]). */
int stn_op_fold_ln(stn_handle* h, int dtype, int M, int C, int S, const float* part, const float* b2, const float* gamma,
                   const float* rowvec_or_null, const int32_t* row_b_or_null, int nseq, const float* ln_g, const float* ln_b, float* x,
                   float* y);
/* One layout kernel between the GEMMs on host operands (the bit-for-bit kernel tests).  which / p (int parameters) / operands:
 *   0 row_map         p = {B, rows_padded, with_row_b}; len [B]; iout = row_off [B+1] followed by row_b (with_row_b: max(sum len, rows_padded) entries)
 *   1 ncl_to_rows     p = {B, C, L, ld_out}; a [B,C,L]; out: rows of ld_out in dtype
 *   2 euler_ncl       p = {B, D, L, with_z, ldz}; a = prev [B,D,L], b = velocity rows of D, c = dt [B]; out [B,D,L]; out2 (with_z): rows of ldz in dtype
 *   3 unpack_rows     p = {B, T, W}; a: packed rows of W; len [B]; out [B,T,W]
 *   4 embed           p = {vocab, B, L, C}; ids [B,L]; a = table [vocab,C]; len [B]; out: rows of C
 *   5 masked_mean     p = {B, L, C}; a: rows of C (rounded to dtype); len [B]; out [B,C]
 *   6 vocoder_im2col  p = {B, L, ld, ccf, k, kp}; a = latent [B, ld*ccf, L]; len = valid vocoder frames (<= L*ccf) or NULL; out: rows of kp in dtype
 *   7 vocoder_in      p = {B, L, ld, ccf, C, k}; a = latent, b = weights [ld*k, C], c = bias [C]; len as above; out [B*L*ccf, C]
 *   8 fill_rows       p = {B, T, W, rf, zeros}; len = valid [B]; out [B,T,W]: only rows t >= valid[b] are written — zeros != 0: with zeros; else
 *                     a = quiet [W], b = edge [rf,W]: edge[t - (T - rf)] for t >= T - rf, quiet otherwise (what unpack_rows' dense twin writes there)
 *   9 hs_pairs        p = {B}; len [B]; iout: the head-split cross-attention's pairing, 2 * ceil(B/2) words
 *  10 trim_len        p = {B, ccf, T, rf, tail_form}; len [B] latent lengths (<= T / ccf); iout = n [B] followed by valid [B]
 * packed != 0 (1, 2, 4, 5, 6): the rows (for 2: the velocity and z rows) are packed per sequence, len[b] each, and need len; else sequence b
 * owns L (T, L*ccf) rows.  out / out2 / iout are the caller's whole buffers of out_n / out2_n / iout_n elements: uploaded as given (out of 1
 * and 6, out2 of 2: rounded to dtype) and written back whole, so what a kernel must not touch can be checked.  Buffers too small for the
 * extents a kernel addresses are refused (STN_ERR_INVALID), as is B > 1024. */
int stn_op_layout(stn_handle* h, int which, int dtype, const int32_t* p, int n_p, const float* a, int64_t a_n, const float* b, int64_t b_n,
                  const float* c, int64_t c_n, const int64_t* ids, int64_t ids_n, const int32_t* len, int packed, float* out, int64_t out_n,
                  float* out2, int64_t out2_n, int32_t* iout, int64_t iout_n);
/* rope_mode: -1 none, 0 RoPE on the position index, 1 length-aware RoPE; OR-ing 0x100 makes the engine rotate the keys in
 * a separate pass first (the way the vector estimator's step-invariant text keys are handled) — same result */
int stn_op_attention(stn_handle* h, int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, const float* k,
                     const float* v, const int32_t* qlen_or_null, const int32_t* klen_or_null, int rope_mode, float* o);
/* One attention through the engine's launcher in the layouts the engine runs (the kernel parity tests of every attention form).  Operands
 * are rounded to `dtype` first.  q: q_elems floats, rows of ldq, head hh of a row at columns q_col + hh*dh; kv: kv_elems floats, rows of
 * ldk, K at columns k_col + hh*dh, V at v_col + hh*dh (a fused QKV row, or the K/V pair of block blk of an nb*2C row); o: o_elems floats,
 * rows of ldo, written at columns 0 .. H*dh.  Dense: sequence b owns rows b*Lq .. of q / o and b*Lk .. of kv; q_off / k_off (B entries
 * each, with qlen / klen): packed rows, sequence b owns qlen[b] rows from q_off[b] (min(klen[b], Lk) from k_off[b]).  rope_mode as
 * stn_op_attention.  k_rotated != 0: the keys are rotated first, in place, by the engine's one-time text-key pass (rot_groups groups
 * rot_stride columns apart from column rot_col of each valid key row), and the attention takes them as rotated.  kv and o are the caller's
 * whole buffers: uploaded as given (rounded to dtype) and written back whole (16-bit values widened to fp32, exactly), so what lies
 * outside the written region can be checked.  form: the form that ran (as stn_dbg_attn_form), NUL-terminated, truncated to form_cap;
 * may be NULL. */
int stn_op_attention_ex(stn_handle* h, int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, int64_t q_elems, int ldq,
                        int q_col, float* kv, int64_t kv_elems, int ldk, int k_col, int v_col, float* o, int64_t o_elems, int ldo,
                        const int32_t* qlen_or_null, const int32_t* klen_or_null, const int32_t* q_off_or_null,
                        const int32_t* k_off_or_null, int rope_mode, int k_rotated, int rot_groups, int rot_stride, int rot_col,
                        char* form, size_t form_cap);
/* One launch of the vector estimator's head-split cross-attention block (16-bit engines; C = 384, 4 heads of 96):
 * part[h*part_stride + row*384 + n] = (Wo[:, 96h .. 96h+96] . attention_h(Wq[96h .., :] . xn[row] + bq[96h ..], K_h, V_h))[n], 16-bit.
 * xn [M,384] (packed query rows: utterance b owns qlen[b] <= L rows in order, sum qlen <= M); Wq, Wo [384,384] row-major (repacked here
 * as at model load); bq: 384 floats or NULL.  kv: kv_elems floats, rows of ldk, K at columns k_col .., V at k_col + 384 ..; dense keys
 * (utterance b owns rows b*Lk ..) or packed (k_off with klen).  Keys are taken as already rotated; rope_mode rotates the queries.
 * pairs_mode 1: the utterances are paired by launch_xattn_hs_pairs and the table (2*ceil(B/2) ints) is written to pairs_out; 0: no table.
 * part: part_elems floats (>= 3*part_stride + M*384, part_stride >= M*384), the caller's whole buffer, uploaded as given (rounded) and
 * written back whole (widened to fp32, exactly).  form: as stn_dbg_attn_form kind 1. */
int stn_op_xattn_hs(stn_handle* h, int dtype, int M, const float* xn, const float* Wq, const float* bq_or_null, const float* Wo,
                    const float* kv, int64_t kv_elems, int ldk, int k_col, int B, int L, int Lk, const int32_t* qlen,
                    const int32_t* klen_or_null, const int32_t* k_off_or_null, int rope_mode, int pairs_mode, int64_t part_stride,
                    float* part, int64_t part_elems, int32_t* pairs_out_or_null, char* form, size_t form_cap);
/* diagnostics (no device needed): the form the engine's attention launchers take.  kind 0, launch_attention: "mfma<DH,fmt> kcKC nchN"
 * (keys per LDS chunk, chunks at Lk), "scalar<fmt,TPRn>" with, for fp32, "vec" / "elem" / "vec qkv-subset" (the operands staged with
 * 16-byte loads).  misaligned: bit 0 / 1 / 2 = the q / k / v pointer is 4 bytes off 16-byte alignment.  kind 1, launch_xattn_hs (C =
 * H*dh, L = Lq; ldq and misaligned unused): "xattn_hs<fmt,U> kcKC".  Returns the string's length (written with its NUL when it fits in
 * cap), < 0 on a call the launcher refuses (STN_ERR_INVALID). */
int stn_dbg_attn_form(int kind, int dtype, int B, int Lq, int Lk, int H, int dh, int ldq, int ldk, int misaligned, char* out, size_t cap);
/* the pointwise pair of a ConvNeXt block on host operands (16-bit engines): x <- x + gamma * (W2 . GELU(W1 . xn + b1) + b2)
 * [+ rowvec[row_b[m]]], W1 [I,C], W2 [C,I], x [M,C] in place.  fused = 1: the K4 kernel, 0: the two tiled GEMM launches,
 * 2: K4-split (16-bit partial sums of the hidden quarters) followed by the fold. */
int stn_op_ffn(stn_handle* h, int M, int C, int I, const float* xn /*[M,C]*/, const float* W1, const float* b1, const float* W2,
               const float* b2_or_null, const float* gamma_or_null, const float* rowvec_or_null /*[nseq,C]*/,
               const int32_t* row_b_or_null /*[M]*/, int nseq, float* x, int fused);
/* The same pair through the engine's own launch (Engine::ffn_launch) on the caller's whole buffers (the kernel parity tests of every K4 and
 * K4-split form).  dtype: STN_DTYPE_BF16 or STN_DTYPE_F16, and the engine's.  xn: xn_elems floats, rows of ldx (>= C, a multiple of 8; the
 * columns past C are never read), rounded to dtype; W1 [I,C], W2 [C,I] rounded to dtype; b1 [I], b2 [C] (NULL: 0), gamma [C] (NULL: 1) fp32.
 * x: x_elems floats, rows of ldo (>= C, a multiple of 4).  Modes 0 (two tiled launches) and 1 (K4):
 *   x[m*ldo + n] = (x[m*ldo + n] + gamma[n] (y[m][n] + b2[n]) + rowvec[seq(m)*rv_ld + n]) * keep(m),  y = W2 . GELU(W1 . xn[m] + b1)
 * with keep(m) = 0 where len[b] <= t for row m = b*L + t (len: nseq entries in 0..L) and seq(m) = row_b[m] (M entries in 0..nseq-1; not with
 * len) or m / L; rowvec: nseq rows of rv_ld (>= C, a multiple of 4).  Mode 2 (K4-split): S = split, or the launcher's choice for M rows
 * when split is 0; part[sp*part_stride + m*C + n] receives share sp's y as a 16-bit value and NO fold runs: x, b2, gamma, rowvec, len are
 * not used and x comes back as it went in.  part_stride >= (M rounded up to 128) * C.  x and part (part_elems floats, rounded to dtype) are
 * uploaded as given and written back whole (16-bit values widened to fp32, exactly), so what lies around the written region can be checked.
 * Refused (STN_ERR_INVALID): fp32 engines, a shape the fused kernel does not take (modes 1, 2), a split the shape does not run with, buffers
 * smaller than the extents the launch addresses, len together with row_b, split or part outside mode 2.  form: the form that ran (as
 * stn_dbg_ffn_form), NUL-terminated, truncated to form_cap; may be NULL. */
int stn_op_ffn_ex(stn_handle* h, int dtype, int M, int C, int I, const float* xn, int ldx, int64_t xn_elems, const float* W1, const float* b1,
                  const float* W2, const float* b2_or_null, const float* gamma_or_null, const int32_t* len_or_null, int L,
                  const int32_t* row_b_or_null, const float* rowvec_or_null, int rv_ld, int nseq, int mode, int split, float* x, int ldo,
                  int64_t x_elems, float* part_or_null, int64_t part_stride, int64_t part_elems, char* form, size_t form_cap);
/* timing of the same on random device-resident operands.  out5: avg ms per call; fused only: mean shader-clock cycles per
 * workgroup until the first stage landed / in the tile loop / in the epilogue, and the number of workgroups */
int stn_op_ffn_bench(stn_handle* h, int M, int C, int I, int fused, int iters, double* out5);
/* fold + depthwise conv + LayerNorm on packed rows (16-bit engines): sequence b owns seqlen[b] consecutive rows, M = their sum;
 * part [S,M,C] (fp32, rounded to the engine's 16-bit format first).  x_out [M,C] = x + gamma * (sum_s part[s] + b2) + rowvec[b],
 * y [M,C] = LayerNorm(dwconv_{k,dil}(x_out)) (fp32 copy of the 16-bit output). */
int stn_op_fold_dwconv_ln(stn_handle* h, int B, int C, int k, int dil, int S, const int32_t* seqlen, const float* x, const float* part,
                          const float* b2_or_null, const float* gamma_or_null, const float* rowvec_or_null /*[B,C]*/, const float* w /*[C,k]*/,
                          const float* bias, const float* ln_g, const float* ln_b, float* x_out, float* y);
/* The same launcher (launch_fold_dwconv_ln, once) on the caller's whole buffers (the kernel parity tests of every fold + dwconv + LayerNorm
 * form).  dtype: STN_DTYPE_BF16 or STN_DTYPE_F16, whatever the engine's format.  Packed rows: sequence b owns seqlen[b] (0 allowed) consecutive
 * rows, M = their sum > 0, row offsets computed as the engine does; L >= every length (a larger L adds placeholder workgroups); B <= 1024.
 * run_frames: FoldArgs::run_frames (0, 40, 48; other values are ignored by the launcher).  part: part_elems floats, split s at
 * part + s*part_stride (part_stride >= M*C, a multiple of 8; part_elems >= (S-1)*part_stride + M*C), rounded to dtype on upload.  rowvec: B
 * rows of rv_ld (>= C, a multiple of 4) or NULL; b2 (NULL: 0), gamma (NULL: 1).  x_in: x_rows rows of C.  x_out (x_out_rows rows) and y (y_rows
 * rows) are the caller's whole buffers: uploaded as given (y rounded to dtype) and written back whole (16-bit values widened to fp32, exactly),
 * so what lies outside the written rows can be checked.  eps = 1e-6.  Refused (STN_ERR_INVALID): what stn_dbg_fold_dwconv_ln_form refuses,
 * buffers smaller than the extents the launch addresses, B > 1024.  form: the form that ran (as stn_dbg_fold_dwconv_ln_form), NUL-terminated,
 * truncated to form_cap; may be NULL. */
int stn_op_fold_dwconv_ln_ex(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, int S, int run_frames, const int32_t* seqlen,
                             const float* x_in, int64_t x_rows, const float* part, int64_t part_stride, int64_t part_elems,
                             const float* b2_or_null, const float* gamma_or_null, const float* rowvec_or_null, int rv_ld,
                             const float* w /*[C,k]*/, const float* bias, const float* ln_g, const float* ln_b, float* x_out, int64_t x_out_rows,
                             float* y, int64_t y_rows, char* form, size_t form_cap);
/* diagnostics (no device needed): the form the fold + depthwise conv + LayerNorm launcher takes for B packed sequences with padded length L:
 * everything that selects code — "fold_dwconv_ln<fmt,K5|K7,rv|norv,ns3|ns4,S4|S8|S12|S24,U1|U2|U3> run R cps N": the kernel instantiation
 * (ns: float4 slots per lane, 3 up to C = 384; U: window rows per thread and trip of phase 1), the run length R in frames (8 when
 * B * ceil(L/32) < 64, else 32, or run_frames where that is 40 or 48 and its image fits 160 KiB of LDS) and the workgroups per sequence
 * N = ceil(L / R); the grid is B * N.  Returns the string's length (written with its NUL when it fits in cap), < 0 on a call the launcher
 * refuses (STN_ERR_INVALID: fp32, B or L < 1, C % 8, C > 512, k outside {5, 7}, S outside {4, 8, 12, 24}, a dilation whose 32-frame image
 * does not fit LDS). */
int stn_dbg_fold_dwconv_ln_form(int dtype, int B, int L, int C, int k, int dil, int S, int has_rowvec, int run_frames, char* out, size_t cap);
/* timing of one estimator-style block on B packed sequences of L frames, random device-resident operands: mode 0 = dwconv_ln + pw1 +
 * pw2, mode 2 = fold_dwconv_ln + K4-split.  out6: avg ms per block, avg ms of its conv kernel alone; mode 2: mean shader-clock cycles per
 * fold_dwconv_ln workgroup in phase 1 / at the hand-over barrier / in phase 2, and the launch's span (first entry to last exit) */
int stn_op_block_bench(stn_handle* h, int B, int L, int C, int I, int k, int dil, int mode, int iters, double* out6);
int stn_op_randn(stn_handle* h, uint64_t seed, int B, int D, int L, const int64_t* utt_ids_or_null,
                 const int32_t* len_or_null, float* out);

const char* stn_version(void);
/* HIP runtime versions: the one libstn.so was compiled against and the one it runs on (they differ when the process loaded
 * PyTorch-ROCm's bundled runtime first); no device needed */
int stn_hip_versions(int* built, int* runtime);
/* Visible HIP devices (< 0: STN_ERR_DEVICE), and a device-wide synchronize (hipDeviceSynchronize on `device`): what a host that does not
 * link a HIP runtime itself needs around a timed region (bench.py --gpus 1 runs without PyTorch, on the runtime this library ships against). */
int stn_device_count(void);
int stn_device_sync(int device);
/* forms of the pointwise pair the kernels offer for a block shape (no device needed): 0 = two tiled launches only, 1 = K4,
 * 2 = K4 and K4-split.  Counts the LDS a workgroup needs (ring + biases <= 160 KiB), so a descriptor that loads never selects a
 * kernel that cannot launch. */
int stn_ffn_fused_forms(int dtype, int C, int I);

#ifdef __cplusplus
}
#endif
#endif /* STN_H */
