// api.cpp — the C ABI of include/stn.h over stn::Engine.  No exception leaves this file.
#include "../../include/stn.h"

#include <algorithm>
#include <complex>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "engine.hpp"
#include "host/json_min.hpp"
#include "host/graph_bind.hpp"
#include "host/onnx_reader.hpp"

#include <map>
#include <sstream>

struct stn_handle {
    stn::Engine* eng = nullptr;
    std::string err;
    std::vector<std::pair<std::string, stn::KernelStat>> prof;
};

static thread_local std::string g_create_err;

#define STN_TRY(h, body)                                             \
    if (!(h)) return STN_ERR_INVALID;                                \
    try {                                                            \
        body;                                                        \
        return STN_OK;                                               \
    } catch (const std::invalid_argument& e) {                       \
        (h)->err = e.what();                                         \
        return STN_ERR_INVALID;                                      \
    } catch (const std::exception& e) {                              \
        (h)->err = e.what();                                         \
        return (h)->err.rfind("HIP error", 0) == 0 ? STN_ERR_DEVICE : STN_ERR_STATE; \
    } catch (...) {                                                  \
        (h)->err = "unknown failure";                                \
        return STN_ERR_DEVICE;                                       \
    }

static void need(bool ok, const char* what) {
    if (!ok) throw std::invalid_argument(what);
}
// a finished batch, or "no finished batch" as the error `err` of the entry: STN_ERR_STATE, or, in the older entries, STN_ERR_INVALID
static void need_batch(stn_handle* h, int err = STN_ERR_STATE) {
    if (h->eng->batch().B > 0 && h->eng->batch().L > 0) return;
    if (err == STN_ERR_INVALID) throw std::invalid_argument("no finished batch");
    throw std::runtime_error("no finished batch");
}
// the argument checks the row entries share.  fn: the entry's name, as the messages give it; ptrs: whether every required pointer is
// there, what: their list as the message gives it; x_misalign, in_place: an _ex entry's 0 / 1 flags (null: it has none)
static void need_op_rows(const std::string& fn, int rows, int W, bool ptrs, const char* what, const int* x_misalign = nullptr, const int* in_place = nullptr) {
    need(rows > 0 && rows <= 65535 && W > 0 && ptrs, (fn + ": bad argument (1 <= rows <= 65535, W >= 1, " + what + ")").c_str());
    auto flag = [](const int* f) { return !f || *f == 0 || *f == 1; };
    need(flag(x_misalign) && flag(in_place), (fn + (in_place ? ": x_misalign and in_place must be 0 or 1" : ": x_misalign must be 0 or 1")).c_str());
}
static void need_model(stn_handle* h) {
    if (!h->eng->loaded()) throw std::runtime_error("no model loaded: call stn_load_synthetic or stn_load_dir first");
}

extern "C" {

const char* stn_version(void) { return "supertonic_amd 0.1 (gfx950)"; }

/* HIP runtime the library was compiled against vs the one it is running on (a process that imports PyTorch first binds libstn.so
 * to the runtime bundled with the wheel): for the record, and for a warning in the Python binding when they differ */
int stn_hip_versions(int* built, int* runtime) {
    int rt = 0;
    const hipError_t e = hipRuntimeGetVersion(&rt);
    if (built) *built = HIP_VERSION;
    if (runtime) *runtime = e == hipSuccess ? rt : -1;
    return e == hipSuccess ? STN_OK : STN_ERR_DEVICE;
}
int stn_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return STN_ERR_DEVICE; }
    return n;
}
int stn_device_sync(int device) {
    if (hipSetDevice(device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return STN_ERR_DEVICE; }
    return STN_OK;
}
/* which form of the pointwise pair the kernels offer for a block shape: 0 = two tiled launches only, 1 = K4, 2 = K4 and K4-split */
int stn_ffn_fused_forms(int dtype, int C, int I) {
    if (C <= 0 || I <= 0 || !stn::ffn_fused_supported(dtype, C, I)) return 0;
    return stn::ffn_split_factor(dtype, C, I) > 1 ? 2 : 1;
}

int stn_create(const stn_config* cfg, stn_handle** out) {
    if (!cfg || !out) { g_create_err = "stn_create: null argument"; return STN_ERR_INVALID; }
    *out = nullptr;
    try {
        stn_handle* h = new stn_handle;
        h->eng = new stn::Engine(cfg->device, cfg->dtype);
        *out = h;
        return STN_OK;
    } catch (const std::exception& e) {
        g_create_err = e.what();
        return STN_ERR_DEVICE;
    }
}
int stn_destroy(stn_handle* h) {
    if (!h) return STN_OK;
    try { delete h->eng; } catch (...) {}
    delete h;
    return STN_OK;
}
const char* stn_last_error(const stn_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int stn_load_synthetic(stn_handle* h, const stn_arch* arch, uint64_t seed) {
    STN_TRY(h, { need(arch != nullptr, "arch is null"); h->eng->load_synthetic(*arch, seed); })
}
extern "C++" {
namespace {
std::string slurp_text(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f.is_open()) throw std::runtime_error("Failed to open " + path);
    return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
// descriptor fields addressable from tts.json / the manifest's "arch" object
const std::map<std::string, int32_t stn_arch::*>& arch_fields() {
    static const std::map<std::string, int32_t stn_arch::*> m = {
        {"sample_rate", &stn_arch::sample_rate}, {"base_chunk_size", &stn_arch::base_chunk_size},
        {"chunk_compress_factor", &stn_arch::chunk_compress_factor}, {"latent_dim", &stn_arch::latent_dim},
        {"vocab_size", &stn_arch::vocab_size}, {"n_style_ttl", &stn_arch::n_style_ttl}, {"d_style_ttl", &stn_arch::d_style_ttl},
        {"n_style_dp", &stn_arch::n_style_dp}, {"d_style_dp", &stn_arch::d_style_dp},
        {"te_dim", &stn_arch::te_dim}, {"te_hidden", &stn_arch::te_hidden}, {"te_kernel", &stn_arch::te_kernel},
        {"te_conv_blocks", &stn_arch::te_conv_blocks}, {"te_attn_blocks", &stn_arch::te_attn_blocks}, {"te_heads", &stn_arch::te_heads},
        {"te_ffn", &stn_arch::te_ffn}, {"te_style_blocks", &stn_arch::te_style_blocks}, {"te_out_dim", &stn_arch::te_out_dim},
        {"dp_dim", &stn_arch::dp_dim}, {"dp_hidden", &stn_arch::dp_hidden}, {"dp_kernel", &stn_arch::dp_kernel},
        {"dp_conv_blocks", &stn_arch::dp_conv_blocks}, {"dp_heads", &stn_arch::dp_heads},
        {"ve_dim", &stn_arch::ve_dim}, {"ve_hidden", &stn_arch::ve_hidden}, {"ve_kernel", &stn_arch::ve_kernel},
        {"ve_main_blocks", &stn_arch::ve_main_blocks}, {"ve_dilated", &stn_arch::ve_dilated}, {"ve_tail_blocks", &stn_arch::ve_tail_blocks},
        {"ve_heads", &stn_arch::ve_heads}, {"ve_time_dim", &stn_arch::ve_time_dim},
        {"vo_dim", &stn_arch::vo_dim}, {"vo_hidden", &stn_arch::vo_hidden}, {"vo_kernel", &stn_arch::vo_kernel},
        {"vo_blocks", &stn_arch::vo_blocks}, {"vo_in_kernel", &stn_arch::vo_in_kernel}};
    return m;
}
}  // namespace
}  // extern "C++"

// Asset directory of the reference (cpp/helper.cpp:784-823): tts.json + unicode_indexer.json + four .onnx graphs.  Without a
// manifest the graphs' nodes are walked and bound to the canonical tensor list (host/graph_bind.hpp); an optional
// `stn_weight_map.json` names the initializers explicitly instead (include/stn.h).
int stn_load_dir(stn_handle* h, const char* onnx_dir) {
    if (!h) return STN_ERR_INVALID;
    if (!onnx_dir) { h->err = "onnx_dir is null"; return STN_ERR_INVALID; }
    const std::string dir = onnx_dir;
    static const char* files[] = {"tts.json", "unicode_indexer.json", "duration_predictor.onnx", "text_encoder.onnx",
                                  "vector_estimator.onnx", "vocoder.onnx"};
    for (const char* f : files) {
        std::ifstream in(dir + "/" + f, std::ios::binary);
        if (!in.is_open()) { h->err = "Failed to open " + dir + "/" + f; return STN_ERR_IO; }
    }
    try {
        using stn::json::Value;
        stn_arch a = stn::graphbind::arch_from_config(dir + "/tts.json");

        const std::string man_path = dir + "/stn_weight_map.json";
        std::map<std::string, stn::onnx::Model> models;
        static const char* graphs[] = {"duration_predictor.onnx", "text_encoder.onnx", "vector_estimator.onnx", "vocoder.onnx"};
        for (const char* g : graphs) models.emplace(g, stn::onnx::parse_file(dir + "/" + g));
        stn::graphbind::check_all_io_names(models.at(graphs[0]), models.at(graphs[1]), models.at(graphs[2]), models.at(graphs[3]));
        {
            std::ifstream probe(man_path);
            const bool heads_explicit = probe.is_open() && stn::graphbind::apply_arch_overrides(dir, a);  // a manifest without "tensors": head counts only
            if (!probe.is_open() || heads_explicit) {
                // no tensor table: recognise the layout in the graphs themselves (host/graph_bind.hpp)
                const stn::graphbind::Result gb = stn::graphbind::bind(a, models.at(graphs[0]), models.at(graphs[1]), models.at(graphs[2]), models.at(graphs[3]), heads_explicit);
                h->eng->load_tensors(gb.arch, [&](const std::string& name, int rows, int cols) {
                    auto it = gb.tensors.find(name);
                    if (it == gb.tensors.end()) throw std::runtime_error("graph binding: no initializer was bound to tensor \"" + name + "\"");
                    return stn::graphbind::fetch(it->second, name, rows, cols);
                });
                h->eng->set_gelu_form(gb.gelu == "tanh");  // the activation the graphs compute (fp32 / f16 follow it exactly)
                h->err = gb.notes;  // readable through stn_last_error after a successful load
                return STN_OK;
            }
        }
        const Value man = stn::json::parse(slurp_text(man_path));
        if (man.has("arch")) {
            for (const auto& kv : man.at("arch").obj) {
                if (kv.first == "vo_dilations") {
                    if (kv.second.arr.size() > STN_MAX_VO_BLOCKS)
                        throw std::runtime_error("manifest: vo_dilations has " + std::to_string(kv.second.arr.size()) + " entries, at most " +
                                                 std::to_string(STN_MAX_VO_BLOCKS) + " vocoder blocks are supported");
                    for (size_t i = 0; i < kv.second.arr.size(); ++i) a.vo_dilations[i] = kv.second.arr[i].as_int();
                    continue;
                }
                auto it = arch_fields().find(kv.first);
                if (it == arch_fields().end()) throw std::runtime_error("manifest: unknown arch field \"" + kv.first + "\"");
                a.*(it->second) = kv.second.as_int();
            }
        }
        const Value& tmap = man.at("tensors");
        h->eng->load_tensors(a, [&](const std::string& name, int rows, int cols) {
            if (!tmap.has(name)) throw std::runtime_error("manifest: no entry for tensor \"" + name + "\"");
            const Value& ent = tmap.at(name);
            const std::string file = ent.at("file").str, iname = ent.at("name").str;
            auto mit = models.find(file);
            if (mit == models.end()) throw std::runtime_error("manifest: unknown graph file \"" + file + "\" for " + name);
            const stn::onnx::Tensor* t = mit->second.find(iname);
            if (!t) throw std::runtime_error(file + ": no initializer named \"" + iname + "\" (for " + name + ")");
            std::vector<float> v = stn::onnx::to_float(*t);
            if (v.size() != (size_t)rows * cols)
                throw std::runtime_error(name + ": initializer " + iname + " has " + std::to_string(v.size()) + " elements, descriptor wants " +
                                         std::to_string(rows) + "x" + std::to_string(cols));
            // stored dims (1s dropped) against the canonical [rows][cols]: "transpose" may be stated; otherwise it is inferred when
            // the dims are unambiguous ([cols][rows] with rows != cols), and dims that are neither orientation are an error
            std::vector<int64_t> d;
            for (int64_t x : t->dims) if (x != 1) d.push_back(x);
            bool tr = ent.has("transpose") && ent.at("transpose").boolean;
            if (d.size() == 2 && rows > 1 && cols > 1) {
                const bool as_is = d[0] == rows && d[1] == cols, flipped = d[0] == cols && d[1] == rows;
                if (!as_is && !flipped)
                    throw std::runtime_error(name + ": initializer " + iname + " is stored [" + std::to_string(d[0]) + "][" + std::to_string(d[1]) +
                                             "], neither [" + std::to_string(rows) + "][" + std::to_string(cols) + "] nor its transpose");
                if (!ent.has("transpose")) tr = flipped && !as_is;
                else if (tr && !flipped) throw std::runtime_error(name + ": manifest says \"transpose\" but initializer " + iname + " is not stored [" + std::to_string(cols) + "][" + std::to_string(rows) + "]");
                else if (!tr && !as_is) throw std::runtime_error(name + ": initializer " + iname + " is stored transposed ([" + std::to_string(d[0]) + "][" + std::to_string(d[1]) + "]); the manifest says \"transpose\": false");
            }
            if (tr) {  // stored [cols][rows] -> canonical [rows][cols]
                std::vector<float> w(v.size());
                for (int r = 0; r < rows; ++r) for (int c = 0; c < cols; ++c) w[(size_t)r * cols + c] = v[(size_t)c * rows + r];
                v.swap(w);
            }
            return v;
        });
        return STN_OK;
    } catch (const std::invalid_argument& e) {  // the descriptor check of Engine::load_weights
        h->err = e.what();
        return STN_ERR_INVALID;
    } catch (const std::exception& e) {
        h->err = e.what();
        return h->err.rfind("HIP error", 0) == 0 ? STN_ERR_DEVICE : STN_ERR_IO;
    }
}
int stn_tensor_names(stn_handle* h, const stn_arch* arch, char* out, size_t cap) {
    if (!h || !arch) return STN_ERR_INVALID;
    try {
        std::string packed;
        const auto names = h->eng->tensor_names(*arch);
        for (const auto& n : names) { packed += n; packed.push_back('\n'); }
        if (out && cap > packed.size()) std::memcpy(out, packed.c_str(), packed.size() + 1);
        return (int)packed.size();
    } catch (const std::exception& e) { h->err = e.what(); return STN_ERR_STATE; }
}
int stn_get_arch(const stn_handle* h, stn_arch* out) {
    if (!h || !out) return STN_ERR_INVALID;
    *out = h->eng->arch();
    return STN_OK;
}
int64_t stn_param_count(const stn_handle* h) { return h ? h->eng->param_count() : 0; }

int stn_duration(stn_handle* h, int B, int Lt, const int64_t* ids, const float* style_dp, const float* text_mask, float* dur) {
    STN_TRY(h, { need_model(h); need(B > 0 && Lt > 0 && ids && style_dp && text_mask && dur, "stn_duration: bad argument");
                 h->eng->duration(B, Lt, ids, style_dp, text_mask, dur); })
}
int stn_text_enc(stn_handle* h, int B, int Lt, const int64_t* ids, const float* style_ttl, const float* text_mask, float* emb) {
    STN_TRY(h, { need_model(h); need(B > 0 && Lt > 0 && ids && style_ttl && text_mask && emb, "stn_text_enc: bad argument");
                 h->eng->text_enc(B, Lt, ids, style_ttl, text_mask, emb); })
}
int stn_vector_est(stn_handle* h, int B, int L, int Lt, const float* noisy, const float* text_emb, const float* style_ttl,
                   const float* text_mask, const float* latent_mask, const float* total_step, const float* current_step,
                   float* out) {
    STN_TRY(h, { need_model(h);
                 need(B > 0 && L > 0 && Lt > 0 && noisy && text_emb && style_ttl && text_mask && latent_mask && total_step && current_step && out,
                      "stn_vector_est: bad argument");
                 for (int b = 0; b < B; ++b) need(total_step[b] >= 1.0f, "stn_vector_est: total_step must be >= 1");
                 h->eng->vector_est(B, L, Lt, noisy, text_emb, style_ttl, text_mask, latent_mask, total_step, current_step, out); })
}
int stn_vocoder(stn_handle* h, int B, int L, const float* latent, float* wav) {
    STN_TRY(h, { need_model(h); need(B > 0 && L > 0 && latent && wav, "stn_vocoder: bad argument"); h->eng->vocoder(B, L, latent, wav); })
}

int stn_batch_upload(stn_handle* h, int B, int Lt, const int64_t* ids, const float* text_mask, const float* style_ttl,
                     const float* style_dp, const float* dur_override, const int64_t* utt_ids) {
    STN_TRY(h, { need_model(h); need(B > 0 && Lt > 0 && ids && text_mask && style_ttl && style_dp, "stn_batch_upload: bad argument");
                 if (dur_override) for (int b = 0; b < B; ++b) need(dur_override[b] > 0.f, "duration override must be > 0");
                 h->eng->batch_upload(B, Lt, ids, text_mask, style_ttl, style_dp, dur_override, utt_ids); })
}
int stn_batch_set_noise(stn_handle* h, const float* noise, int L) {
    STN_TRY(h, { need(noise != nullptr, "noise is null"); h->eng->batch_set_noise(noise, L); })
}
int stn_batch_run(stn_handle* h, int total_step, float speed, uint64_t noise_seed) {
    STN_TRY(h, { need_model(h); need(total_step >= 1, "total_step must be >= 1"); need(speed > 0.f, "speed must be > 0");
                 h->eng->batch_run(total_step, speed, noise_seed); })
}
int stn_set_graph_mode(stn_handle* h, int on) { STN_TRY(h, { h->eng->set_graph_mode(on != 0); }) }
int64_t stn_batch_vo_rows(const stn_handle* h) { return h ? h->eng->last_vo_rows() : 0; }
int64_t stn_batch_ve_rows(const stn_handle* h) { return h ? h->eng->last_ve_rows() : 0; }
int stn_set_row_layout(stn_handle* h, int packed) { STN_TRY(h, { h->eng->set_packed_rows(packed != 0); }) }
int stn_set_shape_buckets(stn_handle* h, int on) { STN_TRY(h, { h->eng->set_shape_buckets(on != 0); }) }
int stn_set_duration_read(stn_handle* h, int always) { STN_TRY(h, { h->eng->set_duration_read(always != 0); }) }
int stn_set_gelu_form(stn_handle* h, int tanh_form) { STN_TRY(h, { h->eng->set_gelu_form(tanh_form); }) }
int stn_get_gelu_form(const stn_handle* h) { return h ? h->eng->gelu_form() : STN_ERR_INVALID; }
int stn_set_fused_xattn(stn_handle* h, int on) { STN_TRY(h, { h->eng->set_fused_xattn(on); }) }
int stn_set_fused_ffn(stn_handle* h, int mask) { STN_TRY(h, { need(mask >= 0 && mask <= 15, "stage mask must be in 0..15"); h->eng->set_fused_ffn(mask); }) }
int stn_set_fused_ffn_min_rows(stn_handle* h, int64_t k4_rows, int64_t split_rows) { STN_TRY(h, { h->eng->set_fused_ffn_min_rows(k4_rows, split_rows); }) }
int stn_set_vocoder_mode(stn_handle* h, int length_aware) { STN_TRY(h, { h->eng->set_vocoder_mode(length_aware != 0); }) }
int64_t stn_graph_replays(const stn_handle* h) { return h ? h->eng->graph_replays() : 0; }
int64_t stn_graphs_cached(const stn_handle* h) { return h ? (int64_t)h->eng->graphs_cached() : 0; }
int stn_batch_dims(const stn_handle* h, int* B, int* L, int64_t* wav_len) {
    if (!h) return STN_ERR_INVALID;
    const auto& b = h->eng->batch();
    const auto& a = h->eng->arch();
    if (B) *B = b.B;
    if (L) *L = b.L;
    if (wav_len) *wav_len = h->eng->out_len((int64_t)b.L * a.base_chunk_size * a.chunk_compress_factor);  // (at the output rate)
    return STN_OK;
}
int stn_set_output_rate(stn_handle* h, int hz) { STN_TRY(h, { h->eng->set_output_rate(hz); }) }
int stn_get_output_rate(const stn_handle* h) { return h ? h->eng->output_rate() : STN_ERR_INVALID; }
int stn_resample_filter(int in_hz, int out_hz, float* taps, size_t cap, int* phases, int* taps_per_phase) {
    try {
        stn::ResampleTable f;
        if (!stn::resample_design(in_hz, out_hz, f).empty()) return STN_ERR_INVALID;
        if (phases) *phases = f.P;
        if (taps_per_phase) *taps_per_phase = f.T;
        if (taps) {
            if (cap < f.taps.size()) return STN_ERR_INVALID;
            std::memcpy(taps, f.taps.data(), f.taps.size() * sizeof(float));
        }
        return STN_OK;
    } catch (...) { return STN_ERR_INVALID; }
}
const char* stn_resample_error(int in_hz, int out_hz) {
    static thread_local std::string why;
    stn::ResampleTable f;
    try { why = stn::resample_design(in_hz, out_hz, f); } catch (const std::exception& e) { why = e.what(); }
    return why.c_str();
}
int stn_op_resample(stn_handle* h, int in_hz, int out_hz, int rows, int W, const float* x, float* y, int16_t* pcm) {
    STN_TRY(h, { need_op_rows("stn_op_resample", rows, W, x && (y || pcm), "x and y or pcm");
                 h->eng->op_resample(in_hz, out_hz, rows, W, x, y, pcm); })
}
int stn_dbg_resample_form(int in_hz, int out_hz, int64_t W, char* out, size_t cap) {
    std::string f;
    try {
        stn::ResampleTable t;
        if (W < 1 || !stn::resample_design(in_hz, out_hz, t).empty()) return STN_ERR_INVALID;
        f = stn::resample_form(W, t).str();  // the decision launch_resample takes
    } catch (const std::exception&) { return STN_ERR_INVALID; }
    if (out && cap > f.size()) std::memcpy(out, f.c_str(), f.size() + 1);
    return (int)f.size();
}
int stn_set_loudness(stn_handle* h, int on, float target_lufs, float ceiling_dbfs) {
    STN_TRY(h, { h->eng->set_loudness(on != 0, target_lufs, ceiling_dbfs); })
}
int stn_get_loudness(const stn_handle* h, int* on, float* target_lufs, float* ceiling_dbfs) {
    if (!h) return STN_ERR_INVALID;
    h->eng->get_loudness(on, target_lufs, ceiling_dbfs);
    return STN_OK;
}
int stn_batch_loudness(stn_handle* h, float* lufs, float* peak, float* gain) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_loudness(lufs, peak, gain); })
}
int stn_op_loudness(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, float* lufs, float* peak) {
    STN_TRY(h, { need_op_rows("stn_op_loudness", rows, W, x, "x");
                 h->eng->op_loudness(hz, rows, W, x, n, lufs, peak); })
}
int stn_op_loudness_ex(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, int on, float target_lufs, float ceiling_dbfs,
                       int x_misalign, float* st_end, float* st_start, float* pk, float* pa, float* pb, float* lufs, float* peak, float* gain,
                       char* form, size_t form_cap) {
    STN_TRY(h, { need_op_rows("stn_op_loudness_ex", rows, W, x, "x", &x_misalign);
                 stn::Engine::LoProbe p;
                 p.x_misalign = x_misalign; p.st_end = st_end; p.st_start = st_start; p.pk = pk; p.pa = pa; p.pb = pb;
                 h->eng->op_loudness_ex(hz, rows, W, x, n, on != 0, target_lufs, ceiling_dbfs, p, lufs, peak, gain);
                 if (form && form_cap) std::snprintf(form, form_cap, "%s", p.form); })
}
int stn_set_silence_trim(stn_handle* h, int on, float top_db, float keep_ms, float fade_ms) {
    STN_TRY(h, { h->eng->set_silence_trim(on != 0, top_db, keep_ms, fade_ms); })
}
int stn_get_silence_trim(const stn_handle* h, int* on, float* top_db, float* keep_ms, float* fade_ms) {
    if (!h) return STN_ERR_INVALID;
    h->eng->get_silence_trim(on, top_db, keep_ms, fade_ms);
    return STN_OK;
}
int stn_batch_silence_edges(stn_handle* h, int64_t* start, int64_t* end) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_silence_edges(start, end); })
}
int stn_op_silence_edges(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, int64_t* start,
                         int64_t* end) {
    STN_TRY(h, { need_op_rows("stn_op_silence_edges", rows, W, x, "x");
                 h->eng->op_silence_edges(hz, rows, W, x, n, top_db, keep_ms, start, end); })
}
int stn_op_silence_trim(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, float fade_ms,
                        const float* gain, int enc, void* y, int64_t* start, int64_t* end) {
    STN_TRY(h, { need_op_rows("stn_op_silence_trim", rows, W, x && y, "x and y");
                 h->eng->op_silence_trim(hz, rows, W, x, n, top_db, keep_ms, fade_ms, gain, enc, y, start, end); })
}
int stn_set_pause_limit(stn_handle* h, int on, float max_pause_ms) {
    STN_TRY(h, { h->eng->set_pause_limit(on != 0, max_pause_ms); })
}
int stn_get_pause_limit(const stn_handle* h, int* on, float* max_pause_ms) {
    if (!h) return STN_ERR_INVALID;
    h->eng->get_pause_limit(on, max_pause_ms);
    return STN_OK;
}
int stn_batch_pauses(stn_handle* h, int64_t* len, int32_t* n_cuts, int64_t* cuts, int cap_pairs) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_pauses(len, n_cuts, cuts, cap_pairs); })
}
int stn_op_pause_trim(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, float fade_ms,
                      float max_pause_ms, const float* gain, int enc, void* y, int64_t* start, int64_t* end, int64_t* len, int32_t* n_cuts,
                      int64_t* cuts, int cap_pairs) {
    STN_TRY(h, { need_op_rows("stn_op_pause_trim", rows, W, x && y, "x and y");
                 h->eng->op_pause_trim(hz, rows, W, x, n, top_db, keep_ms, fade_ms, max_pause_ms, gain, enc, y, start, end, len, n_cuts, cuts, cap_pairs); })
}
int stn_op_silence_edges_ex(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, float top_db, float keep_ms, float fade_ms,
                            float max_pause_ms, int x_misalign, float* pa, float* pb, double* lev, int64_t* start, int64_t* end, int64_t* len,
                            int32_t* n_cuts, int64_t* cuts, int cap_pairs, char* form, size_t form_cap) {
    STN_TRY(h, { need_op_rows("stn_op_silence_edges_ex", rows, W, x, "x", &x_misalign);
                 stn::Engine::EdProbe p;
                 p.x_misalign = x_misalign; p.pa = pa; p.pb = pb; p.lev = lev;
                 h->eng->op_silence_edges_ex(hz, rows, W, x, n, top_db, keep_ms, fade_ms, max_pause_ms, p, start, end, len, n_cuts, cuts, cap_pairs);
                 if (form && form_cap) std::snprintf(form, form_cap, "%s", p.form); })
}
int stn_silence_fade_window(int hz, float fade_ms, float* w, int64_t cap, int64_t* n) {
    if (hz < 1 || !stn::silence_check(1.0f, 0.0f, fade_ms).empty()) return STN_ERR_INVALID;
    try {
        const std::vector<float> v = stn::silence_fade_window(hz, fade_ms);
        if (n) *n = (int64_t)v.size();
        if (w) std::copy(v.begin(), v.begin() + std::min<int64_t>(cap < 0 ? 0 : cap, (int64_t)v.size()), w);
        return STN_OK;
    } catch (const std::exception&) {
        return STN_ERR_INVALID;
    }
}
int stn_set_limiter(stn_handle* h, int on, float lookahead_ms) {
    STN_TRY(h, { h->eng->set_limiter(on != 0, lookahead_ms); })
}
int stn_get_limiter(const stn_handle* h, int* on, float* lookahead_ms) {
    if (!h) return STN_ERR_INVALID;
    h->eng->get_limiter(on, lookahead_ms);
    return STN_OK;
}
int stn_batch_limiter(stn_handle* h, float* reduction_db, int64_t* limited) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_limiter(reduction_db, limited); })
}
int stn_op_limiter(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, const float* gain, float ceiling_dbfs,
                   float lookahead_ms, float* y, float* s, float* reduction_db, int64_t* limited) {
    STN_TRY(h, { need_op_rows("stn_op_limiter", rows, W, x && y, "x and y");
                 h->eng->op_limiter(hz, rows, W, x, n, gain, ceiling_dbfs, lookahead_ms, y, s, reduction_db, limited); })
}
int stn_limiter_window(int hz, float lookahead_ms, float* w, int64_t cap, int64_t* n) {
    if (!stn::limiter_check(hz, lookahead_ms).empty()) return STN_ERR_INVALID;
    try {
        const std::vector<float> v = stn::limiter_window(hz, lookahead_ms);
        if (n) *n = (int64_t)v.size();
        if (w) std::copy(v.begin(), v.begin() + std::min<int64_t>(cap < 0 ? 0 : cap, (int64_t)v.size()), w);
        return STN_OK;
    } catch (const std::exception&) {
        return STN_ERR_INVALID;
    }
}
int stn_set_filters(stn_handle* h, int n, const stn_filter* f) { STN_TRY(h, { h->eng->set_filters(n, f); }) }
int stn_get_filters(const stn_handle* h, int* n, stn_filter* out) {
    if (!h) return STN_ERR_INVALID;
    const std::vector<stn_filter>& f = h->eng->filters();
    if (n) *n = (int)f.size();
    if (out) std::copy(f.begin(), f.end(), out);
    return STN_OK;
}
int stn_op_filter(stn_handle* h, int hz, int rows, int W, const float* x, int n, const stn_filter* f, float* y) {
    STN_TRY(h, { need_op_rows("stn_op_filter", rows, W, x && f && y, "x, f and y");
                 h->eng->op_filter(hz, rows, W, x, n, f, y, nullptr); })
}
int stn_op_filter_ex(stn_handle* h, int hz, int rows, int W, const float* x, int n, const stn_filter* f, int x_misalign, float* y, float* st_end,
                     float* st_start, int* guard_ok, char* form, size_t form_cap) {
    STN_TRY(h, { need_op_rows("stn_op_filter_ex", rows, W, x && f && y, "x, f and y", &x_misalign);
                 stn::Engine::FlProbe p;
                 p.x_misalign = x_misalign; p.st_end = st_end; p.st_start = st_start;
                 h->eng->op_filter(hz, rows, W, x, n, f, y, &p);
                 if (guard_ok) *guard_ok = p.guard_ok ? 1 : 0;
                 if (form && form_cap) std::snprintf(form, form_cap, "%s", p.form); })
}
const char* stn_filter_error(int n, const stn_filter* f, int rate_hz) {
    static thread_local std::string why;
    why = rate_hz > 0 ? stn::filter_check(n, f, rate_hz) : "filters: rate_hz must be positive";
    return why.c_str();
}
int stn_filter_coefs(const stn_filter* f, int rate_hz, double c[5], float c32[5]) {
    if (!f || rate_hz <= 0 || !stn::filter_check(1, f, rate_hz).empty()) return STN_ERR_INVALID;
    double d[5];
    stn::filter_design(*f, rate_hz, d);
    for (int i = 0; i < 5; ++i) {
        if (c) c[i] = d[i];
        if (c32) c32[i] = (float)d[i];
    }
    return STN_OK;
}
int stn_filter_response(int n, const stn_filter* f, int rate_hz, int n_freq, const double* freq_hz, double* mag_db) {
    if (n < 1 || rate_hz <= 0 || n_freq < 0 || (n_freq > 0 && (!freq_hz || !mag_db)) || !stn::filter_check(n, f, rate_hz).empty()) return STN_ERR_INVALID;
    std::vector<float> c32((size_t)n * 5);
    for (int i = 0; i < n; ++i) {
        double d[5];
        stn::filter_design(f[i], rate_hz, d);
        for (int j = 0; j < 5; ++j) c32[(size_t)i * 5 + j] = (float)d[j];
    }
    for (int k = 0; k < n_freq; ++k) {
        const double w = 2.0 * M_PI * freq_hz[k] / rate_hz;
        const std::complex<double> z1 = std::polar(1.0, -w), z2 = std::polar(1.0, -2.0 * w);
        double db = 0.0;
        for (int i = 0; i < n; ++i) {
            const float* c = &c32[(size_t)i * 5];
            db += 20.0 * std::log10(std::abs(((double)c[0] + (double)c[1] * z1 + (double)c[2] * z2) / (1.0 + (double)c[3] * z1 + (double)c[4] * z2)));
        }
        mag_db[k] = db;
    }
    return STN_OK;
}
int stn_dbg_filter_geometry(int* chunk, int* wg_span, int* scan_tile_chunks, int* biquads_per_section) {
    if (chunk) *chunk = stn::LO_CHUNK;
    if (wg_span) *wg_span = stn::LO_WG * stn::LO_CHUNK;
    if (scan_tile_chunks) *scan_tile_chunks = stn::LO_SCAN;
    if (biquads_per_section) *biquads_per_section = 2;
    return STN_OK;
}
int stn_set_compressor(stn_handle* h, int on, const stn_compressor* c) { STN_TRY(h, { h->eng->set_compressor(on != 0, c); }) }
int stn_get_compressor(const stn_handle* h, int* on, stn_compressor* out) {
    if (!h) return STN_ERR_INVALID;
    if (on) *on = h->eng->compressor_on() ? 1 : 0;
    if (out) *out = h->eng->compressor();
    return STN_OK;
}
int stn_batch_compressor(stn_handle* h, float* max_reduction_db) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_compressor(max_reduction_db); })
}
int stn_op_compressor(stn_handle* h, int hz, int rows, int W, const float* x, const stn_compressor* c, float* y) {
    STN_TRY(h, { need_op_rows(__func__, rows, W, x && c && y, "x, c and y");
                 h->eng->op_compressor(hz, rows, W, x, *c, y, nullptr); })
}
int stn_op_compressor_ex(stn_handle* h, int hz, int rows, int W, const float* x, const stn_compressor* c, int x_misalign, int in_place, float* y,
                         float* gr_db, float* s1_end, float* s1_start, float* s2_end, float* s2_start, int* guard_ok, char* form, size_t form_cap) {
    STN_TRY(h, { need_op_rows(__func__, rows, W, x && c && y, "x, c and y", &x_misalign, &in_place);
                 stn::Engine::CpProbe p;
                 p.x_misalign = x_misalign; p.in_place = in_place; p.gr = gr_db;
                 p.s1_end = s1_end; p.s1_start = s1_start; p.s2_end = s2_end; p.s2_start = s2_start;
                 h->eng->op_compressor(hz, rows, W, x, *c, y, &p);
                 if (guard_ok) *guard_ok = p.guard_ok ? 1 : 0;
                 if (form && form_cap) std::snprintf(form, form_cap, "%s", p.form); })
}
const char* stn_compressor_error(const stn_compressor* c, int rate_hz) {
    static thread_local std::string why;
    why = stn::compressor_check(c);
    if (why.empty() && rate_hz < 0) why = "compressor: rate_hz must not be negative";
    if (why.empty() && rate_hz > 0) why = stn::rate_check("compressor", rate_hz);
    return why.c_str();
}
int stn_compressor_coefs(const stn_compressor* c, int rate_hz, double k[2], float k32[2]) {
    if (rate_hz <= 0 || *stn_compressor_error(c, rate_hz)) return STN_ERR_INVALID;
    const double d[2] = {stn::compressor_k(c->attack_ms, rate_hz), stn::compressor_k(c->release_ms, rate_hz)};
    for (int i = 0; i < 2; ++i) {
        if (k) k[i] = d[i];
        if (k32) k32[i] = (float)d[i];
    }
    return STN_OK;
}
int stn_compressor_curve(const stn_compressor* c, int n, const double* in_db, double* out_db) {
    if (n < 0 || (n > 0 && (!in_db || !out_db)) || !stn::compressor_check(c).empty()) return STN_ERR_INVALID;
    for (int i = 0; i < n; ++i) out_db[i] = stn::compressor_curve(*c, in_db[i]);
    return STN_OK;
}
int stn_set_deesser(stn_handle* h, int on, const stn_deesser* c) { STN_TRY(h, { h->eng->set_deesser(on != 0, c); }) }
int stn_get_deesser(const stn_handle* h, int* on, stn_deesser* out) {
    if (!h) return STN_ERR_INVALID;
    if (on) *on = h->eng->deesser_on() ? 1 : 0;
    if (out) *out = h->eng->deesser();
    return STN_OK;
}
int stn_batch_deesser(stn_handle* h, float* max_reduction_db) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_deesser(max_reduction_db); })
}
int stn_op_deesser(stn_handle* h, int hz, int rows, int W, const float* x, const stn_deesser* c, float* y) {
    STN_TRY(h, { need_op_rows(__func__, rows, W, x && c && y, "x, c and y");
                 h->eng->op_deesser(hz, rows, W, x, *c, y, nullptr); })
}
int stn_op_deesser_ex(stn_handle* h, int hz, int rows, int W, const float* x, const stn_deesser* c, int x_misalign, int in_place, float* y,
                      float* band, float* gr_db, float* st_end, float* st_start, float* s1_end, float* s1_start, float* s2_end,
                      float* s2_start, int* guard_ok, char* form, size_t form_cap) {
    STN_TRY(h, { need_op_rows(__func__, rows, W, x && c && y, "x, c and y", &x_misalign, &in_place);
                 stn::Engine::DsProbe p;
                 p.x_misalign = x_misalign; p.in_place = in_place; p.band = band; p.gr = gr_db; p.st_end = st_end; p.st_start = st_start;
                 p.s1_end = s1_end; p.s1_start = s1_start; p.s2_end = s2_end; p.s2_start = s2_start;
                 h->eng->op_deesser(hz, rows, W, x, *c, y, &p);
                 if (guard_ok) *guard_ok = p.guard_ok ? 1 : 0;
                 if (form && form_cap) std::snprintf(form, form_cap, "%s", p.form); })
}
const char* stn_deesser_error(const stn_deesser* c, int rate_hz) {
    static thread_local std::string why;
    why = rate_hz < 0 ? "deesser: rate_hz must not be negative" : stn::deesser_check(c, rate_hz);
    return why.c_str();
}
int stn_deesser_band(const stn_deesser* c, int rate_hz, double c10[10], float c32[10]) {
    if (rate_hz <= 0 || *stn_deesser_error(c, rate_hz)) return STN_ERR_INVALID;
    stn_filter f[2];
    stn::deesser_band(*c, f);
    for (int h = 0; h < 2; ++h) {
        double d[5];
        stn::filter_design(f[h], rate_hz, d);
        for (int i = 0; i < 5; ++i) {
            if (c10) c10[h * 5 + i] = d[i];
            if (c32) c32[h * 5 + i] = (float)d[i];
        }
    }
    return STN_OK;
}
int stn_deesser_coefs(const stn_deesser* c, int rate_hz, double k[2], float k32[2]) {
    if (rate_hz <= 0 || *stn_deesser_error(c, rate_hz)) return STN_ERR_INVALID;
    const double d[2] = {stn::compressor_k(c->attack_ms, rate_hz), stn::compressor_k(c->release_ms, rate_hz)};
    for (int i = 0; i < 2; ++i) {
        if (k) k[i] = d[i];
        if (k32) k32[i] = (float)d[i];
    }
    return STN_OK;
}
int stn_set_expander(stn_handle* h, int on, const stn_expander* c) { STN_TRY(h, { h->eng->set_expander(on != 0, c); }) }
int stn_get_expander(const stn_handle* h, int* on, stn_expander* out) {
    if (!h) return STN_ERR_INVALID;
    if (on) *on = h->eng->expander_on() ? 1 : 0;
    if (out) *out = h->eng->expander();
    return STN_OK;
}
int stn_batch_expander(stn_handle* h, float* min_attenuation_db, int64_t* closed_samples) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_expander(min_attenuation_db, closed_samples); })
}
int stn_op_expander(stn_handle* h, int hz, int rows, int W, const float* x, const stn_expander* c, float* y) {
    STN_TRY(h, { need_op_rows(__func__, rows, W, x && c && y, "x, c and y");
                 h->eng->op_expander(hz, rows, W, x, *c, y, nullptr); })
}
int stn_op_expander_ex(stn_handle* h, int hz, int rows, int W, const float* x, const stn_expander* c, int x_misalign, int in_place, float* y,
                       float* open_db, float* s1_end, float* s1_start, float* s2_end, float* s2_start, int* guard_ok, char* form, size_t form_cap) {
    STN_TRY(h, { need_op_rows(__func__, rows, W, x && c && y, "x, c and y", &x_misalign, &in_place);
                 stn::Engine::XpProbe p;
                 p.x_misalign = x_misalign; p.in_place = in_place; p.open = open_db;
                 p.s1_end = s1_end; p.s1_start = s1_start; p.s2_end = s2_end; p.s2_start = s2_start;
                 h->eng->op_expander(hz, rows, W, x, *c, y, &p);
                 if (guard_ok) *guard_ok = p.guard_ok ? 1 : 0;
                 if (form && form_cap) std::snprintf(form, form_cap, "%s", p.form); })
}
const char* stn_expander_error(const stn_expander* c, int rate_hz) {
    static thread_local std::string why;
    why = stn::expander_check(c);
    if (why.empty() && rate_hz < 0) why = "expander: rate_hz must not be negative";
    if (why.empty() && rate_hz > 0) why = stn::rate_check("expander", rate_hz);
    return why.c_str();
}
int stn_expander_coefs(const stn_expander* c, int rate_hz, double k[3], float k32[3], int64_t* hold_samples) {
    if (rate_hz <= 0 || *stn_expander_error(c, rate_hz)) return STN_ERR_INVALID;
    stn::ExpTable t;
    stn::expander_table(rate_hz, *c, t);
    // each in double from the setting's fp32 fields; Bh from the fp32 delta the GPU subtracts, as the table forms it
    const double d[3] = {stn::compressor_k(c->attack_ms, rate_hz), (double)c->range_db * 1000.0 / ((double)c->release_ms * (double)rate_hz),
                         (double)t.coef.delta * (double)t.hold};
    const float f[3] = {t.coef.kA, t.coef.delta, t.coef.Bh};
    for (int i = 0; i < 3; ++i) {
        if (k) k[i] = d[i];
        if (k32) k32[i] = f[i];
    }
    if (hold_samples) *hold_samples = t.hold;
    return STN_OK;
}
int stn_expander_curve(const stn_expander* c, int n, const double* in_db, double* out_db) {
    if (n < 0 || (n > 0 && (!in_db || !out_db)) || !stn::expander_check(c).empty()) return STN_ERR_INVALID;
    for (int i = 0; i < n; ++i) out_db[i] = stn::expander_curve(*c, in_db[i]);
    return STN_OK;
}
int stn_set_dither(stn_handle* h, int mode, uint64_t seed) { STN_TRY(h, { h->eng->set_dither(mode, seed); }) }
int stn_get_dither(const stn_handle* h, uint64_t* seed) {
    if (!h) return STN_ERR_INVALID;
    if (seed) *seed = h->eng->dither_seed();
    return h->eng->dither_mode();
}
int stn_op_encode_ex(stn_handle* h, int enc, int rows, int W, const float* x, int x_misalign, const float* gain, const int64_t* row_id, int mode,
                     uint64_t seed, int64_t dst_stride, void* y) {
    STN_TRY(h, { need(rows > 0 && W > 0 && x && y, "stn_op_encode_ex: bad argument (rows >= 1, W >= 1, x and y)");
                 h->eng->op_encode_ex(enc, rows, W, x, x_misalign, gain, row_id, mode, seed, dst_stride, y); })
}
int stn_set_pitch(stn_handle* h, float semitones) { STN_TRY(h, { h->eng->set_pitch(semitones); }) }
int stn_get_pitch(const stn_handle* h, float* semitones, int* a, int* b) {
    if (!h) return STN_ERR_INVALID;
    if (semitones) *semitones = h->eng->pitch();
    if (a) *a = h->eng->pitch_a();
    if (b) *b = h->eng->pitch_b();
    return STN_OK;
}
int stn_op_time_stretch(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, int a, int b, float* y, int32_t* delta, float* score) {
    STN_TRY(h, { need_op_rows("stn_op_time_stretch", rows, W, x, "x");
                 h->eng->op_time_stretch(hz, rows, W, x, n, a, b, y, delta, score); })
}
int stn_op_pitch(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, float semitones, float* y) {
    STN_TRY(h, { need_op_rows("stn_op_pitch", rows, W, x && y, "x and y");
                 h->eng->op_pitch(hz, rows, W, x, n, semitones, y); })
}
int stn_set_pitch_mode(stn_handle* h, int mode) { STN_TRY(h, { h->eng->set_pitch_mode(mode); }) }
int stn_get_pitch_mode(const stn_handle* h) { return h ? h->eng->pitch_mode() : STN_ERR_INVALID; }
int stn_op_formant(stn_handle* h, int hz, int rows, int W, const float* x, const float* y, const int64_t* n, float* out) {
    STN_TRY(h, { need_op_rows("stn_op_formant", rows, W, x && y && out, "x, y and out");
                 h->eng->op_formant(hz, rows, W, x, y, n, out); })
}
int stn_op_formant_ex(stn_handle* h, int hz, int rows, int W, const float* x, const float* y, const int64_t* n, float* out, float* ax, float* cy, double* g,
                      double* ex, double* ey, int* guard_ok) {
    STN_TRY(h, { need_op_rows("stn_op_formant_ex", rows, W, x && y && out, "x, y and out");
                 stn::Engine::FormantProbe p;
                 p.ax = ax; p.cy = cy; p.g = g; p.ex = ex; p.ey = ey;
                 h->eng->op_formant(hz, rows, W, x, y, n, out, &p);
                 if (guard_ok) *guard_ok = p.guard_ok ? 1 : 0; })
}
int stn_op_pitch_ex(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, float semitones, int mode, float* y) {
    STN_TRY(h, { need_op_rows("stn_op_pitch_ex", rows, W, x && y, "x and y");
                 h->eng->op_pitch_ex(hz, rows, W, x, n, semitones, mode, y); })
}
int stn_set_peak_mode(stn_handle* h, int mode) { STN_TRY(h, { h->eng->set_peak_mode(mode); }) }
int stn_get_peak_mode(const stn_handle* h) { return h ? h->eng->peak_mode() : STN_ERR_INVALID; }
int stn_true_peak_filter(float* taps, size_t cap, int* phases, int* taps_per_phase) {
    if (phases) *phases = stn::TP_PHASES;
    if (taps_per_phase) *taps_per_phase = stn::TP_TAPS;
    if (taps) {
        if (cap < (size_t)stn::TP_PHASES * stn::TP_TAPS) return STN_ERR_INVALID;
        stn::truepeak_design(taps);
    }
    return STN_OK;
}
int stn_batch_true_peak(stn_handle* h, float* tp_in, float* tp_out, float* trim) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_true_peak(tp_in, tp_out, trim); })
}
int stn_op_true_peak(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, const float* gain, int x_misalign, float* tp,
                     float* env, float* pk, char* form, size_t form_cap) {
    STN_TRY(h, { need_op_rows("stn_op_true_peak", rows, W, x, "x", &x_misalign);
                 const char* f = h->eng->op_true_peak(hz, rows, W, x, n, gain, x_misalign, tp, env, pk);
                 if (form && form_cap) std::snprintf(form, form_cap, "%s", f); })
}
int stn_op_limiter_ex(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, const float* gain, float ceiling_dbfs,
                      float lookahead_ms, float* y, float* s, float* reduction_db, int64_t* limited, int peak_mode, float* env, float* trim) {
    STN_TRY(h, { need_op_rows("stn_op_limiter_ex", rows, W, x && y, "x and y");
                 h->eng->op_limiter_ex(hz, rows, W, x, n, gain, ceiling_dbfs, lookahead_ms, y, s, reduction_db, limited, peak_mode, env, trim); })
}
int stn_dbg_batch_set_wav(stn_handle* h, const float* wav) {
    STN_TRY(h, { need(wav != nullptr, "wav is null"); need_batch(h, STN_ERR_INVALID); h->eng->dbg_batch_set_wav(wav); })
}
int64_t stn_dbg_span_uploads(const stn_handle* h) { return h ? h->eng->span_uploads() : 0; }
int stn_kweighting_filter(int hz, double* shelf_b, double* shelf_a, double* hp_b, double* hp_a) {
    stn::KWeighting k;
    if (!stn::kweighting_design(hz, k).empty()) return STN_ERR_INVALID;
    for (int i = 0; i < 3; ++i) {
        if (shelf_b) shelf_b[i] = k.shelf_b[i];
        if (shelf_a) shelf_a[i] = k.shelf_a[i];
        if (hp_b) hp_b[i] = k.hp_b[i];
        if (hp_a) hp_a[i] = k.hp_a[i];
    }
    return STN_OK;
}
int stn_loudness_table(int hz, float* coef10, float* mpow, size_t cap, int* hop) {
    stn::LoudTable t;
    if (!stn::loudness_design(hz, t).empty()) return STN_ERR_INVALID;
    if (coef10) std::copy(t.coef.c, t.coef.c + 10, coef10);
    if (mpow) for (size_t i = 0; i < std::min(cap, t.mpow.size()); ++i) mpow[i] = (float)t.mpow[i];
    if (hop) *hop = t.hop;
    return STN_OK;
}
int stn_batch_fetch(stn_handle* h, float* wav, size_t cap, float* duration) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_fetch(wav, cap, duration); })
}
int stn_batch_fetch_pcm16(stn_handle* h, int16_t* pcm, size_t cap, float* duration) {
    STN_TRY(h, { need(pcm != nullptr, "no finished batch"); need_batch(h, STN_ERR_INVALID); h->eng->batch_fetch_pcm16(pcm, cap, duration); })
}
int stn_batch_fetch_slot_dims(stn_handle* h, int slot, int* B, int64_t* W) {
    if (!h) return STN_ERR_INVALID;
    if (slot < 0 || slot > 1) { h->err = "fetch slot must be 0 or 1"; return STN_ERR_INVALID; }
    int b = 0; int64_t w = 0;
    if (!h->eng->fetch_slot_dims(slot, &b, &w)) { h->err = "no fetch in flight on this slot"; return STN_ERR_STATE; }
    if (B) *B = b;
    if (W) *W = w;
    return STN_OK;
}
int stn_batch_fetch_pcm16_begin(stn_handle* h, int slot) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_fetch_pcm16_begin(slot); })
}
int stn_batch_fetch_pcm16_end(stn_handle* h, int slot, const int16_t** pcm, size_t* n_samples, float* duration) {
    STN_TRY(h, { h->eng->batch_fetch_pcm16_end(slot, pcm, n_samples, duration); })
}
void* stn_host_alloc_pinned(size_t bytes) {
    void* p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
void stn_host_free_pinned(void* p) { if (p) (void)hipHostFree(p); }
int stn_batch_fetch_latent(stn_handle* h, float* latent) {
    STN_TRY(h, { need(latent != nullptr, "no finished batch"); need_batch(h, STN_ERR_INVALID); h->eng->batch_fetch_latent(latent); })
}
int stn_batch_wav_device_ptr(const stn_handle* h, void** ptr) {
    if (!h || !ptr) return STN_ERR_INVALID;
    *ptr = h->eng->batch().wav;
    return *ptr ? STN_OK : STN_ERR_STATE;
}
int stn_sync(stn_handle* h) { STN_TRY(h, { h->eng->sync(); }) }
int stn_set_stream(stn_handle* h, void* hip_stream) { STN_TRY(h, { h->eng->set_stream(static_cast<hipStream_t>(hip_stream)); }) }
int stn_batch_copy_pcm16_device(stn_handle* h, void* dst, int64_t stride) {
    STN_TRY(h, { need(dst != nullptr, "dst is null"); h->eng->batch_copy_pcm16_device(static_cast<int16_t*>(dst), stride); })
}
static_assert(STN_ENC_F32 == stn::ENC_F32 && STN_ENC_PCM16 == stn::ENC_PCM16 && STN_ENC_PCM24 == stn::ENC_PCM24 && STN_ENC_MULAW == stn::ENC_MULAW &&
              STN_ENC_ALAW == stn::ENC_ALAW, "include/stn.h and kernels.hpp disagree on the encodings");
int stn_encoding_bytes(int enc) { return stn::enc_bytes(enc); }
int stn_batch_fetch_encoded(stn_handle* h, int enc, void* dst, size_t cap, float* duration) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_fetch_encoded(enc, dst, cap, duration); })
}
int stn_batch_copy_encoded_device(stn_handle* h, int enc, void* dst, int64_t stride) {
    STN_TRY(h, { need(dst != nullptr, "dst is null"); h->eng->batch_copy_encoded_device(enc, dst, stride); })
}
int stn_batch_fetch_encoded_begin(stn_handle* h, int slot, int enc) {
    STN_TRY(h, { need_batch(h, STN_ERR_INVALID); h->eng->batch_fetch_encoded_begin(slot, enc); })
}
int stn_batch_fetch_encoded_end(stn_handle* h, int slot, const void** data, size_t* n_bytes, float* duration) {
    STN_TRY(h, { h->eng->batch_fetch_encoded_end(slot, data, n_bytes, duration); })
}
int stn_op_encode(stn_handle* h, int enc, int rows, int W, const float* x, void* y) {
    STN_TRY(h, { need(rows > 0 && W > 0 && x && y, "stn_op_encode: bad argument (rows >= 1, W >= 1, x and y)"); h->eng->op_encode(enc, rows, W, x, y); })
}
static_assert(STN_JOIN_WHOLE == 0 && STN_JOIN_TRIM == 1 && STN_JOIN_GAIN_ROW == 0 && STN_JOIN_GAIN_PROG == 1, "include/stn.h: join constants");
int stn_batch_join_dims(stn_handle* h, const stn_join* j, int64_t* W_join, int64_t* prog_len, float* prog_dur) {
    STN_TRY(h, { need(j != nullptr, "join is null"); need_batch(h);
                 const stn::JoinPlan p = h->eng->batch_join_plan(j);
                 if (W_join) *W_join = p.W_join;
                 if (prog_len) std::copy(p.prog_len.begin(), p.prog_len.end(), prog_len);
                 if (prog_dur) std::copy(p.prog_dur.begin(), p.prog_dur.end(), prog_dur); })
}
int stn_batch_fetch_joined(stn_handle* h, const stn_join* j, int enc, void* dst, size_t cap, int64_t* prog_len, float* prog_dur) {
    STN_TRY(h, { need(j != nullptr, "join is null"); need_batch(h); h->eng->batch_fetch_joined(j, enc, dst, cap, prog_len, prog_dur); })
}
int stn_batch_copy_joined_device(stn_handle* h, const stn_join* j, int enc, void* dst, int64_t stride) {
    STN_TRY(h, { need(j != nullptr && dst != nullptr, "join or dst is null"); need_batch(h); h->eng->batch_copy_joined_device(j, enc, dst, stride); })
}
int stn_batch_fetch_joined_begin(stn_handle* h, int slot, const stn_join* j, int enc) {
    STN_TRY(h, { need(j != nullptr, "join is null"); need_batch(h); h->eng->batch_fetch_joined_begin(slot, j, enc); })
}
int stn_batch_join_loudness(stn_handle* h, const stn_join* j, float* lufs, float* peak, float* gain) {
    STN_TRY(h, { need(j != nullptr, "join is null"); need_batch(h); h->eng->batch_join_loudness(j, lufs, peak, gain); })
}
int stn_batch_loudness_range(stn_handle* h, float* m_max, float* s_max, float* lra, int32_t* n_st) {
    STN_TRY(h, { need_batch(h); h->eng->batch_loudness_range(m_max, s_max, lra, n_st); })
}
int stn_batch_join_loudness_range(stn_handle* h, const stn_join* j, float* m_max, float* s_max, float* lra, int32_t* n_st) {
    STN_TRY(h, { need(j != nullptr, "join is null"); need_batch(h); h->eng->batch_join_loudness_range(j, m_max, s_max, lra, n_st); })
}
int stn_op_loudness_range(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, float* m_max, float* s_max, float* lra,
                          int32_t* n_st) {
    STN_TRY(h, { need_op_rows("stn_op_loudness_range", rows, W, x, "x");
                 h->eng->op_loudness_range(hz, rows, W, x, n, m_max, s_max, lra, n_st); })
}
int stn_f0_group(void) { return stn::F0_GROUP; }
int64_t stn_f0_max_frames(void) { return stn::F0_MAX_FRAMES; }
int stn_batch_f0_frames(stn_handle* h, const stn_f0_params* p, int64_t* max_frames) {
    STN_TRY(h, { need(max_frames != nullptr, "max_frames is null"); need_batch(h); *max_frames = h->eng->batch_f0_frames(p); })
}
int stn_batch_f0(stn_handle* h, const stn_f0_params* p, int64_t cap, float* f0, float* ap, stn_f0_stats* stats) {
    STN_TRY(h, { need_batch(h); h->eng->batch_f0(p, cap, f0, ap, stats); })
}
int stn_op_f0(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, const stn_f0_params* p, int64_t cap, float* f0, float* ap,
              stn_f0_stats* stats) {
    STN_TRY(h, { need_op_rows("stn_op_f0", rows, W, x, "x");
                 h->eng->op_f0(hz, rows, W, x, n, p, cap, f0, ap, stats); })
}
int stn_op_join(stn_handle* h, int hz, int rows, int W, const float* x, const int64_t* n, const stn_join* j, int enc, int loudness_on, float target_lufs,
                float ceiling_dbfs, void* y, float* prog_lufs, float* prog_peak, float* prog_gain) {
    STN_TRY(h, { need_op_rows("stn_op_join", rows, W, x && n && j && y, "x, n, j and y");
                 h->eng->op_join(hz, rows, W, x, n, j, enc, loudness_on != 0, target_lufs, ceiling_dbfs, y, prog_lufs, prog_peak, prog_gain); })
}
int stn_batch_copy_wav_device(stn_handle* h, void* dst, int64_t stride) {
    STN_TRY(h, { need(dst != nullptr, "dst is null"); h->eng->batch_copy_wav_device(static_cast<float*>(dst), stride); })
}

int stn_profile_enable(stn_handle* h, int on) { STN_TRY(h, { h->eng->profile_enable(on != 0); }) }
int stn_launch_log_enable(stn_handle* h, int on) { STN_TRY(h, { h->eng->launch_log_enable(on != 0); }) }
int64_t stn_launch_log(stn_handle* h, char* out, size_t cap) {
    if (!h) return STN_ERR_INVALID;
    try {
        const std::string s = h->eng->launch_log();
        if (out && cap > s.size()) std::memcpy(out, s.c_str(), s.size() + 1);
        return (int64_t)s.size();
    } catch (const std::exception& e) { h->err = e.what(); return STN_ERR_STATE; }
}
int stn_dbg_xattn_hs_enable(stn_handle* h, int on) { STN_TRY(h, { h->eng->hs_stamps_enable(on != 0); }) }
int stn_dbg_fold_run_frames(const int32_t* latent_lengths, int B, int n_cu) {
    if (!latent_lengths || B < 1 || n_cu < 1) return STN_ERR_INVALID;
    return stn::fold_run_frames(latent_lengths, B, n_cu);
}
int64_t stn_dbg_xattn_hs_stamps(stn_handle* h, unsigned long long* out, size_t cap) {
    if (!h) return STN_ERR_INVALID;
    try { return h->eng->hs_stamps_fetch(out, cap); } catch (const std::exception& e) { h->err = e.what(); return STN_ERR_STATE; }
}
int stn_profile_sample(stn_handle* h, int every) { STN_TRY(h, { h->eng->profile_sample(every); }) }
int stn_profile_filter(stn_handle* h, const char* fam) { STN_TRY(h, { h->eng->profile_filter(fam ? fam : ""); }) }
int stn_profile_reset(stn_handle* h) { STN_TRY(h, { h->eng->profile_reset(); h->prof.clear(); }) }
int stn_profile_count(stn_handle* h) {
    if (!h) return STN_ERR_INVALID;
    try { h->prof = h->eng->profile_collect(); } catch (const std::exception& e) { h->err = e.what(); return STN_ERR_DEVICE; }
    return (int)h->prof.size();
}
int stn_profile_get(stn_handle* h, int idx, char* name, size_t cap, double* ms, int64_t* launches, double* flops, double* bytes) {
    if (!h || idx < 0 || idx >= (int)h->prof.size()) return STN_ERR_INVALID;
    const auto& p = h->prof[idx];
    if (name && cap) { std::snprintf(name, cap, "%s", p.first.c_str()); }
    if (ms) *ms = p.second.ms;
    if (launches) *launches = p.second.launches;
    if (flops) *flops = p.second.flops;
    if (bytes) *bytes = p.second.bytes;
    return STN_OK;
}

int stn_op_gemm(stn_handle* h, int dtype, int M, int N, int K, const float* A, const float* W, const float* bias, int act, float* out) {
    STN_TRY(h, { need(M > 0 && N > 0 && K > 0 && A && W && out, "stn_op_gemm: bad argument");
                 need(K % (dtype != STN_DTYPE_F32 ? 8 : 4) == 0, "stn_op_gemm: K must be a multiple of 8 (bf16) / 4 (f32)");
                 h->eng->op_gemm(dtype, M, N, K, A, W, bias, act, out); })
}
int stn_op_gemm_ex(stn_handle* h, int dtype, int M, int N, int K, const float* A, const float* W, int mode, int act, int out_dtype, int ldo,
                   const float* bias, const float* gamma, const int32_t* len, int L, const int32_t* row_b, const float* rowvec, int nseq, int nt,
                   int tr, float* out, int64_t out_elems, char* form, size_t form_cap) {
    STN_TRY(h, { need(M > 0 && N > 0 && K > 0 && A && W && out && L >= 1, "stn_op_gemm_ex: bad argument");
                 need(dtype == STN_DTYPE_F32 || dtype == STN_DTYPE_BF16 || dtype == STN_DTYPE_F16, "stn_op_gemm_ex: unknown dtype");
                 need(K % (dtype != STN_DTYPE_F32 ? 8 : 4) == 0, "stn_op_gemm_ex: K must be a multiple of 8 (16-bit) / 4 (f32)");
                 need(mode == stn::EPI_STORE || mode == stn::EPI_RESID || mode == stn::EPI_STORE_T, "stn_op_gemm_ex: mode must be 0, 1 or 2");
                 need(act >= stn::ACT_NONE && act <= stn::ACT_GELU_TANH, "stn_op_gemm_ex: unknown activation");
                 need(out_dtype == STN_DTYPE_F32 || (mode == stn::EPI_STORE && out_dtype == dtype), "stn_op_gemm_ex: out_dtype must be f32 or the engine's dtype (store only)");
                 need(nt == 0 || nt == 1, "stn_op_gemm_ex: nt must be 0 or 1");
                 need(tr >= -1 && tr <= 1, "stn_op_gemm_ex: tr must be -1, 0 or 1");
                 need(!(len && row_b), "stn_op_gemm_ex: len and row_b exclude each other");
                 const int64_t seqs = ((int64_t)M + L - 1) / L;  // sequences m / L reaches
                 if (mode == stn::EPI_STORE_T) {
                     need(!row_b && nseq >= seqs && out_elems >= seqs * N * L, "stn_op_gemm_ex: mode 2 needs nseq >= ceil(M/L), out_elems >= ceil(M/L)*N*L, no row_b");
                 } else {
                     need(ldo >= N && out_elems >= (int64_t)M * ldo, "stn_op_gemm_ex: needs ldo >= N and out_elems >= M*ldo");
                 }
                 if (len || (rowvec && !row_b)) need(nseq >= seqs, "stn_op_gemm_ex: len / rowvec by m / L need nseq >= ceil(M/L)");
                 if (rowvec || len || row_b) need(nseq > 0, "stn_op_gemm_ex: nseq must be > 0");
                 if (len) for (int b = 0; b < nseq; ++b) need(len[b] >= 0 && len[b] <= L, "stn_op_gemm_ex: len out of [0, L]");
                 if (row_b) for (int m = 0; m < M; ++m) need(row_b[m] >= 0 && row_b[m] < nseq, "stn_op_gemm_ex: row_b out of [0, nseq)");
                 const std::string f = h->eng->op_gemm_ex(dtype, M, N, K, A, W, mode, act, out_dtype, ldo, bias, gamma, len, L, row_b, rowvec,
                                                          nseq, nt, tr, out, out_elems);
                 if (form && form_cap) std::snprintf(form, form_cap, "%s", f.c_str()); })
}
int stn_dbg_gemm_form(int dtype, int M, int N, int K, int mode, int out_dtype, int ldo, int masked, int tr, char* out, size_t cap) {
    if (M < 1 || N < 1 || K < 1 || (dtype != STN_DTYPE_F32 && dtype != STN_DTYPE_BF16 && dtype != STN_DTYPE_F16) || tr < -1 || tr > 1)
        return STN_ERR_INVALID;
    static const int dummy_len[4] = {};  // alignment is all the launcher reads of it
    stn::Epilogue e;
    e.mode = mode; e.out_dtype = out_dtype; e.ldo = ldo; e.len = masked ? dummy_len : nullptr; e.tr_force = tr;
    std::string f;
    try { f = stn::gemm_form(dtype, M, N, K, K, K, e, nullptr, nullptr).str(); } catch (const std::exception&) { return STN_ERR_INVALID; }
    if (out && cap > f.size()) std::memcpy(out, f.c_str(), f.size() + 1);
    return (int)f.size();
}
int stn_dbg_ffn_form(int dtype, int stage, int C, int I, int64_t M, int64_t gate_rows, int packed, int k, int max_dil, int mask,
                     int64_t min_rows, int64_t split_min_rows, int nt_hints, char* out, size_t cap) {
    if (C < 1 || I < 1 || M < 1 || k < 1 || max_dil < 1 || (stage != stn::FFN_VOCODER && stage != stn::FFN_ESTIMATOR && stage != stn::FFN_TEXT) ||
        (dtype != STN_DTYPE_F32 && dtype != STN_DTYPE_BF16 && dtype != STN_DTYPE_F16))
        return STN_ERR_INVALID;
    const std::string f = stn::ffn_form(dtype, stage, C, I, M, gate_rows, packed != 0, k, max_dil, mask, min_rows, split_min_rows, nt_hints != 0).str();
    if (out && cap > f.size()) std::memcpy(out, f.c_str(), f.size() + 1);
    return (int)f.size();
}
int stn_op_gemm_bench(stn_handle* h, int dtype, int M, int N, int K, int mode, int iters, double* avg_ms) {
    STN_TRY(h, { need(M > 0 && N > 0 && K > 0 && iters > 0 && avg_ms, "stn_op_gemm_bench: bad argument");
                 need(K % (dtype != STN_DTYPE_F32 ? 8 : 4) == 0, "K must be a multiple of 8 (bf16) / 4 (f32)");
                 *avg_ms = h->eng->op_gemm_bench(dtype, M, N, K, mode, iters); })
}
int stn_op_gemm_phases(stn_handle* h, int dtype, int M, int N, int K, int mode, double* out6) {
    STN_TRY(h, { need(M > 0 && N > 0 && K > 0 && out6, "stn_op_gemm_phases: bad argument");
                 need(K % (dtype != STN_DTYPE_F32 ? 8 : 4) == 0, "K must be a multiple of 8 (bf16) / 4 (f32)");
                 h->eng->op_gemm_phases(dtype, M, N, K, mode, out6); })
}
int stn_op_dwconv_ln(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, const float* x, const float* w,
                     const float* bias, const float* g, const float* b, float* y) {
    STN_TRY(h, { need(B > 0 && L > 0 && C > 0 && C % 4 == 0 && C <= 1024 && k > 0 && (k & 1) && dil > 0 && x && w && bias && g && b && y,
                      "stn_op_dwconv_ln: bad argument");
                 h->eng->op_dwconv_ln(dtype, B, L, C, k, dil, x, w, bias, g, b, y); })
}
int stn_op_dwconv_ln_ragged(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, const float* x, const float* w,
                            const float* bias, const float* g, const float* b, const int32_t* seqlen, float* y) {
    STN_TRY(h, { need(B > 0 && L > 0 && C > 0 && C % 4 == 0 && C <= 1024 && k > 0 && (k & 1) && dil > 0 && x && w && bias && g && b && y && seqlen,
                      "stn_op_dwconv_ln_ragged: bad argument");
                 for (int i = 0; i < B; ++i) need(seqlen[i] >= 0 && seqlen[i] <= L, "stn_op_dwconv_ln_ragged: seqlen out of [0, L]");
                 h->eng->op_dwconv_ln(dtype, B, L, C, k, dil, x, w, bias, g, b, y, seqlen); })
}
static void gemm_rows_checked(stn_handle* h, int dtype, int M, int N, int K, const float* A, const float* W, const float* bias, int B,
                              const int32_t* rows, const int32_t* valid, int T, float* out, int64_t out_elems, char* form, size_t form_cap) {
    need(M > 0 && N > 0 && K > 0 && A && W && out && rows && valid && B > 0 && B <= 1024 && T > 0, "stn_op_gemm_rows: bad argument");
    need(dtype == STN_DTYPE_F32 || dtype == STN_DTYPE_BF16 || dtype == STN_DTYPE_F16, "stn_op_gemm_rows: unknown dtype");
    need(K % (dtype != STN_DTYPE_F32 ? 8 : 4) == 0, "stn_op_gemm_rows: K must be a multiple of 8 (16-bit) / 4 (f32)");
    int64_t tot = 0;
    for (int b = 0; b < B; ++b) {
        need(rows[b] >= 0 && rows[b] <= T && valid[b] >= 0 && valid[b] <= rows[b], "stn_op_gemm_rows: needs 0 <= valid[b] <= rows[b] <= T");
        tot += rows[b];
    }
    need(tot <= M && out_elems >= (int64_t)B * T * N, "stn_op_gemm_rows: needs sum rows <= M and out_elems >= B*T*N");
    const std::string f = h->eng->op_gemm_rows(dtype, M, N, K, A, W, bias, B, rows, valid, T, out, out_elems);
    if (form && form_cap) std::snprintf(form, form_cap, "%s", f.c_str());
}
int stn_op_gemm_rows(stn_handle* h, int dtype, int M, int N, int K, const float* A, const float* W, const float* bias, int B, const int32_t* rows,
                     const int32_t* valid, int T, float* out, int64_t out_elems, char* form, size_t form_cap) {
    STN_TRY(h, gemm_rows_checked(h, dtype, M, N, K, A, W, bias, B, rows, valid, T, out, out_elems, form, form_cap))
}
static void dwconv_ln_ex_checked(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, const float* x, int64_t x_rows, const float* w,
                                 const float* bias, const float* g, const float* b, const int32_t* seqlen, int packed, int ln_only, float* y,
                                 int64_t y_rows, char* form, size_t form_cap) {
    need(B > 0 && L > 0 && C > 0 && C % 4 == 0 && C <= 1024 && k > 0 && (k & 1) && dil > 0 && x && g && b && y && x_rows > 0 && y_rows > 0,
         "stn_op_dwconv_ln_ex: bad argument");
    need(dtype == STN_DTYPE_F32 || dtype == STN_DTYPE_BF16 || dtype == STN_DTYPE_F16, "stn_op_dwconv_ln_ex: unknown dtype");
    need(ln_only || (w && bias), "stn_op_dwconv_ln_ex: the conv needs w and bias");
    need(!(packed && ln_only), "stn_op_dwconv_ln_ex: ln_only takes no packed layout");
    need(!packed || (seqlen && B <= 1024), "stn_op_dwconv_ln_ex: packed rows need seqlen and B <= 1024");
    int64_t rows = (int64_t)B * L;
    if (seqlen && !ln_only) {
        int64_t tot = 0;
        for (int i = 0; i < B; ++i) { need(seqlen[i] >= 0 && seqlen[i] <= L, "stn_op_dwconv_ln_ex: seqlen out of [0, L]"); tot += seqlen[i]; }
        if (packed) rows = tot;
    }
    need(x_rows >= rows && y_rows >= rows, "stn_op_dwconv_ln_ex: x / y hold fewer rows than the launch addresses");
    const std::string f = h->eng->op_dwconv_ln_ex(dtype, B, L, C, k, dil, x, x_rows, w, bias, g, b, ln_only ? nullptr : seqlen, packed, ln_only, y, y_rows);
    if (form && form_cap) std::snprintf(form, form_cap, "%s", f.c_str());
}
int stn_op_dwconv_ln_ex(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, const float* x, int64_t x_rows, const float* w,
                        const float* bias, const float* g, const float* b, const int32_t* seqlen, int packed, int ln_only, float* y,
                        int64_t y_rows, char* form, size_t form_cap) {
    STN_TRY(h, dwconv_ln_ex_checked(h, dtype, B, L, C, k, dil, x, x_rows, w, bias, g, b, seqlen, packed, ln_only, y, y_rows, form, form_cap))
}
static void dwconv_ln_tail_checked(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, const float* x, int64_t x_rows, const float* w,
                                   const float* bias, const float* g, const float* b, const int32_t* seqlen, const float* tail, int T, int rf,
                                   float* y, int64_t y_rows, char* form, size_t form_cap) {
    need(B > 0 && B <= 1024 && L > 0 && C > 0 && C % 4 == 0 && C <= 512 && (k == 5 || k == 7) && dil > 0 && x && w && bias && g && b && y && seqlen &&
             x_rows > 0 && y_rows > 0,
         "stn_op_dwconv_ln_tail: bad argument");
    need(dtype == STN_DTYPE_F32 || dtype == STN_DTYPE_BF16 || dtype == STN_DTYPE_F16, "stn_op_dwconv_ln_tail: unknown dtype");
    need(tail && rf >= 0 && T >= L, "stn_op_dwconv_ln_tail: needs a tail table of rf + 1 >= 1 rows and T >= L");
    int64_t rows = 0;
    for (int i = 0; i < B; ++i) { need(seqlen[i] >= 0 && seqlen[i] <= L, "stn_op_dwconv_ln_tail: seqlen out of [0, L]"); rows += seqlen[i]; }
    need(x_rows >= rows && y_rows >= rows, "stn_op_dwconv_ln_tail: x / y hold fewer rows than the launch addresses");
    const std::string f = h->eng->op_dwconv_ln_ex(dtype, B, L, C, k, dil, x, x_rows, w, bias, g, b, seqlen, 1, 0, y, y_rows, tail, T, rf);
    if (form && form_cap) std::snprintf(form, form_cap, "%s", f.c_str());
}
int stn_op_dwconv_ln_tail(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, const float* x, int64_t x_rows, const float* w,
                          const float* bias, const float* g, const float* b, const int32_t* seqlen, const float* tail, int T, int rf, float* y,
                          int64_t y_rows, char* form, size_t form_cap) {
    STN_TRY(h, dwconv_ln_tail_checked(h, dtype, B, L, C, k, dil, x, x_rows, w, bias, g, b, seqlen, tail, T, rf, y, y_rows, form, form_cap))
}
int64_t stn_dbg_len_tables(int B, const int32_t* llen, int ve_rows, int with_pairs, int vo_form, int ccf, int T, int rf, int32_t* layout,
                           int32_t* out, int64_t out_n) {
    if (B < 1 || B > 1024 || !llen || ve_rows < 0 || vo_form < stn::LEN_VO_NONE || vo_form > stn::LEN_VO_SCALED || ccf < 1 || T < 0 || rf < 0) return STN_ERR_INVALID;
    int64_t tot = 0;
    for (int b = 0; b < B; ++b) {
        if (llen[b] < 0 || llen[b] > (1 << 20)) return STN_ERR_INVALID;
        tot += llen[b];
    }
    if (ve_rows > 0 && tot > ve_rows) return STN_ERR_INVALID;
    if (with_pairs && ve_rows == 0) return STN_ERR_INVALID;
    const stn::LenTables t = stn::len_tables_layout(B, ve_rows, with_pairs != 0, vo_form);
    if (layout) {
        const int v[9] = {t.seed, t.llen, t.ve_off, t.ve_row_b, t.pairs, t.vo_n, t.vo_valid, t.vo_off, t.total};
        std::memcpy(layout, v, sizeof v);
    }
    if (out) {
        if (out_n < t.total) return STN_ERR_INVALID;
        stn::len_tables_build(t, llen, B, ve_rows, with_pairs != 0, vo_form, ccf, T, rf, out);
    }
    return t.total;
}
int stn_dbg_dwconv_ln_form(int dtype, int B, int L, int C, int k, int packed, char* out, size_t cap) {
    if (B < 1 || L < 1 || C < 1 || k < 1 || !(k & 1) || (dtype != STN_DTYPE_F32 && dtype != STN_DTYPE_BF16 && dtype != STN_DTYPE_F16)) return STN_ERR_INVALID;
    std::string f;
    try { f = stn::dwconv_ln_form(dtype, B, L, C, k, packed != 0).str(); } catch (const std::exception&) { return STN_ERR_INVALID; }
    if (out && cap > f.size()) std::memcpy(out, f.c_str(), f.size() + 1);
    return (int)f.size();
}
int stn_op_fold_ln(stn_handle* h, int dtype, int M, int C, int S, const float* part, const float* b2, const float* gamma, const float* rowvec,
                   const int32_t* row_b, int nseq, const float* g, const float* b, float* x, float* y) {
    STN_TRY(h, { need(M > 0 && C > 0 && C % 4 == 0 && C <= 1024 && (S == 4 || S == 8 || S == 12 || S == 24) && part && b2 && gamma && g && b && x && y,
                      "stn_op_fold_ln: bad argument");
                 need(dtype == STN_DTYPE_BF16 || dtype == STN_DTYPE_F16, "stn_op_fold_ln: a 16-bit format needed");
                 need(!rowvec || nseq > 0, "stn_op_fold_ln: rowvec needs nseq > 0");
                 if (rowvec && row_b) for (int m = 0; m < M; ++m) need(row_b[m] >= 0 && row_b[m] < nseq, "stn_op_fold_ln: row_b out of range");
                 h->eng->op_fold_ln(dtype, M, C, S, part, b2, gamma, rowvec, row_b, nseq, g, b, x, y); })
}
int stn_op_layout(stn_handle* h, int which, int dtype, const int32_t* p, int n_p, const float* a, int64_t a_n, const float* b, int64_t b_n,
                  const float* c, int64_t c_n, const int64_t* ids, int64_t ids_n, const int32_t* len, int packed, float* out, int64_t out_n,
                  float* out2, int64_t out2_n, int32_t* iout, int64_t iout_n) {
    static const int n_params[11] = {3, 4, 5, 3, 4, 3, 6, 6, 5, 1, 5};
    STN_TRY(h, { need(which >= 0 && which < 11 && p && n_p == n_params[which], "stn_op_layout: unknown kernel or parameter count");
                 need(dtype == STN_DTYPE_F32 || dtype == STN_DTYPE_BF16 || dtype == STN_DTYPE_F16, "stn_op_layout: unknown dtype");
                 need(a_n >= 0 && b_n >= 0 && c_n >= 0 && ids_n >= 0 && out_n >= 0 && out2_n >= 0 && iout_n >= 0 && (a || !a_n) && (b || !b_n) && (c || !c_n) &&
                          (ids || !ids_n) && (out || !out_n) && (out2 || !out2_n) && (iout || !iout_n),
                      "stn_op_layout: a buffer without a pointer");
                 h->eng->op_layout(which, dtype, p, a, a_n, b, b_n, c, c_n, ids, ids_n, len, packed, out, out_n, out2, out2_n, iout, iout_n); })
}
int stn_op_attention(stn_handle* h, int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, const float* k,
                     const float* v, const int32_t* qlen, const int32_t* klen, int rope_mode, float* o) {
    STN_TRY(h, { need(B > 0 && Lq > 0 && Lk > 0 && H > 0 && dh >= 8 && dh % 8 == 0 && dh <= 96 && q && k && v && o,
                      "stn_op_attention: bad argument");
                 h->eng->op_attention(dtype, B, Lq, Lk, H, dh, q, k, v, qlen, klen, rope_mode, o); })
}
// (the argument checks of the two entry points below declare several variables per statement: too many commas for STN_TRY's body)
static void attention_ex_checked(stn_handle* h, int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, int64_t q_elems, int ldq,
                                 int q_col, float* kv, int64_t kv_elems, int ldk, int k_col, int v_col, float* o, int64_t o_elems, int ldo,
                                 const int32_t* qlen, const int32_t* klen, const int32_t* q_off, const int32_t* k_off, int rope_mode,
                                 int k_rotated, int rot_groups, int rot_stride, int rot_col, char* form, size_t form_cap) {
    need(B > 0 && Lq > 0 && Lk > 0 && H > 0 && dh >= 8 && dh % 8 == 0 && dh <= 96 && q && kv && o, "stn_op_attention_ex: bad argument");
    need(dtype == STN_DTYPE_F32 || dtype == STN_DTYPE_BF16 || dtype == STN_DTYPE_F16, "stn_op_attention_ex: unknown dtype");
    need(rope_mode >= -1 && rope_mode <= 1, "stn_op_attention_ex: rope_mode must be -1, 0 or 1");
    const int64_t C = (int64_t)H * dh;
    need(ldq > 0 && ldk > 0 && ldo >= C && q_col >= 0 && k_col >= 0 && v_col >= 0 && q_col + C <= ldq && k_col + C <= ldk && v_col + C <= ldk,
         "stn_op_attention_ex: the heads must lie inside the rows (col + H*dh <= ld, ldo >= H*dh)");
    need((q_off == nullptr || qlen) && (k_off == nullptr || klen), "stn_op_attention_ex: packed rows need their lengths");
    const int64_t qrows = q_elems / ldq, krows = kv_elems / ldk, orows = o_elems / ldo;
    for (int b = 0; b < B; ++b) {
        need(!qlen || qlen[b] >= 0, "stn_op_attention_ex: qlen < 0");
        need(!klen || klen[b] >= 0, "stn_op_attention_ex: klen < 0");
        if (q_off)
            need(qlen[b] <= Lq && q_off[b] >= 0 && (int64_t)q_off[b] + qlen[b] <= std::min(qrows, orows),
                 "stn_op_attention_ex: packed query rows outside q / o (or qlen > Lq)");
        if (k_off) need(k_off[b] >= 0 && (int64_t)k_off[b] + std::min(klen[b], Lk) <= krows, "stn_op_attention_ex: packed key rows outside kv");
    }
    if (!q_off) need((int64_t)B * Lq <= std::min(qrows, orows), "stn_op_attention_ex: q / o hold fewer than B*Lq rows");
    if (!k_off) need((int64_t)B * Lk <= krows, "stn_op_attention_ex: kv holds fewer than B*Lk rows");
    if (k_rotated)
        need(rot_groups >= 1 && rot_stride >= 0 && rot_col >= 0 && rot_col + (int64_t)(rot_groups - 1) * rot_stride + C <= ldk,
             "stn_op_attention_ex: the rotated groups must lie inside the kv rows");
    const std::string f = h->eng->op_attention_ex(dtype, B, Lq, Lk, H, dh, q, q_elems, ldq, q_col, kv, kv_elems, ldk, k_col, v_col, o, o_elems,
                                                  ldo, qlen, klen, q_off, k_off, rope_mode, k_rotated, rot_groups, rot_stride, rot_col);
    if (form && form_cap) std::snprintf(form, form_cap, "%s", f.c_str());
}
int stn_op_attention_ex(stn_handle* h, int dtype, int B, int Lq, int Lk, int H, int dh, const float* q, int64_t q_elems, int ldq,
                        int q_col, float* kv, int64_t kv_elems, int ldk, int k_col, int v_col, float* o, int64_t o_elems, int ldo,
                        const int32_t* qlen, const int32_t* klen, const int32_t* q_off, const int32_t* k_off, int rope_mode, int k_rotated,
                        int rot_groups, int rot_stride, int rot_col, char* form, size_t form_cap) {
    STN_TRY(h, attention_ex_checked(h, dtype, B, Lq, Lk, H, dh, q, q_elems, ldq, q_col, kv, kv_elems, ldk, k_col, v_col, o, o_elems, ldo,
                                    qlen, klen, q_off, k_off, rope_mode, k_rotated, rot_groups, rot_stride, rot_col, form, form_cap))
}
static void xattn_hs_checked(stn_handle* h, int dtype, int M, const float* xn, const float* Wq, const float* bq, const float* Wo, const float* kv,
                             int64_t kv_elems, int ldk, int k_col, int B, int L, int Lk, const int32_t* qlen, const int32_t* klen,
                             const int32_t* k_off, int rope_mode, int pairs_mode, int64_t part_stride, float* part, int64_t part_elems,
                             int32_t* pairs_out, char* form, size_t form_cap) {
    const int C = 384;
    need(M > 0 && B > 0 && B <= 1024 && L > 0 && Lk > 0 && xn && Wq && Wo && kv && qlen && part, "stn_op_xattn_hs: bad argument");
    need(stn::xattn_hs_supported(dtype, C, 4, L, Lk, ldk), "stn_op_xattn_hs: unsupported dtype or shape (xattn_hs_supported)");
    need(rope_mode >= -1 && rope_mode <= 1 && (pairs_mode == 0 || pairs_mode == 1), "stn_op_xattn_hs: rope_mode -1..1, pairs_mode 0 or 1");
    need(k_col >= 0 && k_col % 8 == 0 && k_col + 2 * C <= ldk, "stn_op_xattn_hs: K and V (k_col .. k_col + 768) must lie inside the rows, k_col % 8 == 0");
    need(k_off == nullptr || klen, "stn_op_xattn_hs: packed keys need klen");
    need(part_stride >= (int64_t)M * C && part_elems >= 3 * part_stride + (int64_t)M * C,
         "stn_op_xattn_hs: part must hold 4 heads of M*384 values part_stride apart");
    int64_t rows = 0;
    const int64_t krows = kv_elems / ldk;
    for (int b = 0; b < B; ++b) {
        need(qlen[b] >= 0 && qlen[b] <= L, "stn_op_xattn_hs: qlen out of [0, L]");
        rows += qlen[b];
        need(!klen || klen[b] >= 0, "stn_op_xattn_hs: klen < 0");
        if (k_off) need(k_off[b] >= 0 && (int64_t)k_off[b] + std::min(klen[b], Lk) <= krows, "stn_op_xattn_hs: packed key rows outside kv");
    }
    need(rows <= M, "stn_op_xattn_hs: sum qlen > M");
    if (!k_off) need((int64_t)B * Lk <= krows, "stn_op_xattn_hs: kv holds fewer than B*Lk rows");
    const std::string f = h->eng->op_xattn_hs(dtype, M, xn, Wq, bq, Wo, kv, kv_elems, ldk, k_col, B, L, Lk, qlen, klen, k_off, rope_mode,
                                              pairs_mode, part_stride, part, part_elems, pairs_out);
    if (form && form_cap) std::snprintf(form, form_cap, "%s", f.c_str());
}
int stn_op_xattn_hs(stn_handle* h, int dtype, int M, const float* xn, const float* Wq, const float* bq, const float* Wo, const float* kv,
                    int64_t kv_elems, int ldk, int k_col, int B, int L, int Lk, const int32_t* qlen, const int32_t* klen, const int32_t* k_off,
                    int rope_mode, int pairs_mode, int64_t part_stride, float* part, int64_t part_elems, int32_t* pairs_out, char* form,
                    size_t form_cap) {
    STN_TRY(h, xattn_hs_checked(h, dtype, M, xn, Wq, bq, Wo, kv, kv_elems, ldk, k_col, B, L, Lk, qlen, klen, k_off, rope_mode, pairs_mode,
                                part_stride, part, part_elems, pairs_out, form, form_cap))
}
int stn_dbg_attn_form(int kind, int dtype, int B, int Lq, int Lk, int H, int dh, int ldq, int ldk, int misaligned, char* out, size_t cap) {
    if (B < 1 || Lq < 1 || Lk < 1 || H < 1 || (dtype != STN_DTYPE_F32 && dtype != STN_DTYPE_BF16 && dtype != STN_DTYPE_F16) || (kind != 0 && kind != 1))
        return STN_ERR_INVALID;
    std::string f;
    try {
        if (kind == 0) {
            auto ptr = [&](int bit) { return reinterpret_cast<const void*>((uintptr_t)(misaligned & bit ? 4 : 0)); };  // read for alignment only
            f = stn::attn_form(dtype, B, Lq, Lk, H, dh, ldq, ldk, ptr(1), ptr(2), ptr(4)).str();
        } else {
            f = stn::xattn_hs_form(dtype, H * dh, H, B, Lq, Lk, ldk).str();
        }
    } catch (const std::exception&) { return STN_ERR_INVALID; }
    if (out && cap > f.size()) std::memcpy(out, f.c_str(), f.size() + 1);
    return (int)f.size();
}
int stn_op_ffn(stn_handle* h, int M, int C, int I, const float* xn, const float* W1, const float* b1, const float* W2, const float* b2,
               const float* gamma, const float* rowvec, const int32_t* row_b, int nseq, float* x, int fused) {
    STN_TRY(h, { need(M > 0 && C > 0 && I > 0 && C % 8 == 0 && I % 8 == 0 && xn && W1 && b1 && W2 && x, "stn_op_ffn: bad argument");
                 need(!rowvec || nseq > 0, "stn_op_ffn: rowvec needs nseq > 0");
                 if (rowvec && row_b) for (int m = 0; m < M; ++m) need(row_b[m] >= 0 && row_b[m] < nseq, "stn_op_ffn: row_b out of range");
                 need(fused >= 0 && fused <= 2, "stn_op_ffn: mode must be 0 (two launches), 1 (K4) or 2 (K4-split + fold)");
                 h->eng->op_ffn(M, C, I, xn, W1, b1, W2, b2, gamma, rowvec, row_b, nseq, x, fused); })
}
static void ffn_ex_checked(stn_handle* h, int dtype, int M, int C, int I, const float* xn, int ldx, int64_t xn_elems, const float* W1, const float* b1,
                           const float* W2, const float* b2, const float* gamma, const int32_t* len, int L, const int32_t* row_b, const float* rowvec,
                           int rv_ld, int nseq, int mode, int split, float* x, int ldo, int64_t x_elems, float* part, int64_t part_stride,
                           int64_t part_elems, char* form, size_t form_cap) {
    need(M > 0 && C > 0 && I > 0 && C % 8 == 0 && I % 8 == 0 && xn && W1 && b1 && W2 && x && L >= 1, "stn_op_ffn_ex: bad argument");
    need((dtype == STN_DTYPE_BF16 || dtype == STN_DTYPE_F16) && dtype == h->eng->dtype(), "stn_op_ffn_ex: dtype must be the 16-bit format of the engine");
    need(mode >= stn::FFN_GEMMS && mode <= stn::FFN_K4_SPLIT, "stn_op_ffn_ex: mode must be 0 (two launches), 1 (K4) or 2 (K4-split)");
    need(mode == stn::FFN_GEMMS || stn::ffn_fused_supported(dtype, C, I), "stn_op_ffn_ex: shape not supported by the fused kernel");
    need(ldx >= C && ldx % 8 == 0 && xn_elems >= (int64_t)M * ldx, "stn_op_ffn_ex: needs ldx >= C, ldx % 8 == 0 and xn_elems >= M*ldx");
    need(ldo >= C && ldo % 4 == 0 && x_elems >= (int64_t)M * ldo, "stn_op_ffn_ex: needs ldo >= C, ldo % 4 == 0 and x_elems >= M*ldo");
    need(!(len && row_b), "stn_op_ffn_ex: len and row_b exclude each other");
    const int64_t seqs = ((int64_t)M + L - 1) / L;  // sequences m / L reaches
    if (len || (rowvec && !row_b)) need(nseq >= seqs, "stn_op_ffn_ex: len / rowvec by m / L need nseq >= ceil(M/L)");
    if (rowvec || len || row_b) need(nseq > 0, "stn_op_ffn_ex: nseq must be > 0");
    if (rowvec) need(rv_ld >= C && rv_ld % 4 == 0, "stn_op_ffn_ex: needs rv_ld >= C and rv_ld % 4 == 0");
    if (len) for (int b = 0; b < nseq; ++b) need(len[b] >= 0 && len[b] <= L, "stn_op_ffn_ex: len out of [0, L]");
    if (row_b) for (int m = 0; m < M; ++m) need(row_b[m] >= 0 && row_b[m] < nseq, "stn_op_ffn_ex: row_b out of [0, nseq)");
    if (mode == stn::FFN_K4_SPLIT) {
        const int S = split ? split : stn::ffn_split_choose(dtype, C, I, M);
        need(stn::ffn_split_valid(dtype, C, I, S), "stn_op_ffn_ex: not a split this shape runs with");
        need(part && part_stride >= stn::ffn_split_rows(M) * C && part_stride % 8 == 0 && part_elems >= (int64_t)S * part_stride,
             "stn_op_ffn_ex: mode 2 needs part, part_stride >= rows padded to 128 * C (a multiple of 8) and part_elems >= S * part_stride");
    } else {
        need(split == 0 && !part, "stn_op_ffn_ex: split and part belong to mode 2");
    }
    const std::string f = h->eng->op_ffn_ex(M, C, I, xn, ldx, xn_elems, W1, b1, W2, b2, gamma, len, L, row_b, rowvec, rv_ld, nseq, mode, split, x, ldo,
                                            x_elems, part, part_stride, part_elems);
    if (form && form_cap) std::snprintf(form, form_cap, "%s", f.c_str());
}
int stn_op_ffn_ex(stn_handle* h, int dtype, int M, int C, int I, const float* xn, int ldx, int64_t xn_elems, const float* W1, const float* b1,
                  const float* W2, const float* b2, const float* gamma, const int32_t* len, int L, const int32_t* row_b, const float* rowvec, int rv_ld,
                  int nseq, int mode, int split, float* x, int ldo, int64_t x_elems, float* part, int64_t part_stride, int64_t part_elems, char* form,
                  size_t form_cap) {
    STN_TRY(h, ffn_ex_checked(h, dtype, M, C, I, xn, ldx, xn_elems, W1, b1, W2, b2, gamma, len, L, row_b, rowvec, rv_ld, nseq, mode, split, x, ldo,
                              x_elems, part, part_stride, part_elems, form, form_cap))
}
int stn_op_ffn_bench(stn_handle* h, int M, int C, int I, int fused, int iters, double* out5) {
    STN_TRY(h, { need(M > 0 && C > 0 && I > 0 && C % 8 == 0 && I % 8 == 0 && iters > 0 && out5, "stn_op_ffn_bench: bad argument");
                 need(fused >= 0 && fused <= 2, "stn_op_ffn_bench: mode must be 0, 1 or 2");
                 h->eng->op_ffn_bench(M, C, I, fused, iters, out5); })
}
int stn_op_fold_dwconv_ln(stn_handle* h, int B, int C, int k, int dil, int S, const int32_t* seqlen, const float* x, const float* part,
                          const float* b2, const float* gamma, const float* rowvec, const float* w, const float* bias, const float* g,
                          const float* b, float* x_out, float* y) {
    STN_TRY(h, { need(B > 0 && C > 0 && C % 8 == 0 && (k == 5 || k == 7) && dil > 0 && (S == 4 || S == 8 || S == 12 || S == 24) && seqlen && x && part && w && bias && g && b && x_out && y,
                      "stn_op_fold_dwconv_ln: bad argument");
                 int64_t tot = 0;
                 for (int i = 0; i < B; ++i) { need(seqlen[i] >= 0 && seqlen[i] < (1 << 20), "stn_op_fold_dwconv_ln: seqlen out of range"); tot += seqlen[i]; }
                 need(tot > 0, "stn_op_fold_dwconv_ln: no rows");
                 h->eng->op_fold_dwconv_ln(B, C, k, dil, S, seqlen, x, part, b2, gamma, rowvec, w, bias, g, b, x_out, y); })
}
static void fold_dwconv_ln_ex_checked(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, int S, int run_frames, const int32_t* seqlen,
                                      const float* x_in, int64_t x_rows, const float* part, int64_t part_stride, int64_t part_elems, const float* b2,
                                      const float* gamma, const float* rowvec, int rv_ld, const float* w, const float* bias, const float* g,
                                      const float* b, float* x_out, int64_t x_out_rows, float* y, int64_t y_rows, char* form, size_t form_cap) {
    const char* who = "stn_op_fold_dwconv_ln_ex";
    auto req = [&](bool ok, const char* what) { need(ok, (std::string(who) + ": " + what).c_str()); };
    req(B > 0 && L > 0 && C > 0 && seqlen && x_in && part && w && bias && g && b && x_out && y, "bad argument");
    req(dtype == STN_DTYPE_BF16 || dtype == STN_DTYPE_F16, "a 16-bit format needed");
    req(B <= 1024, "B <= 1024 needed");
    try { (void)stn::fold_dwconv_ln_form(dtype, B, L, C, k, dil, S, rowvec != nullptr, run_frames); }
    catch (const std::invalid_argument& e) { req(false, e.what()); }
    int64_t tot = 0;
    for (int i = 0; i < B; ++i) { req(seqlen[i] >= 0 && seqlen[i] <= L, "seqlen out of [0, L]"); tot += seqlen[i]; }
    req(tot > 0, "no rows");
    req(tot * C * 2 < 0x7FFFFFFFll, "too many rows");
    req(x_rows >= tot && x_out_rows >= tot && y_rows >= tot, "x_in / x_out / y hold fewer rows than the launch addresses");
    req(part_stride >= tot * C && part_stride % 8 == 0 && part_elems >= (int64_t)(S - 1) * part_stride + tot * C, "part smaller than the launch addresses, or a stride that is no multiple of 8");
    req(!rowvec || (rv_ld >= C && rv_ld % 4 == 0), "rv_ld >= C, a multiple of 4, needed");
    const std::string f = h->eng->op_fold_dwconv_ln_ex(dtype, B, L, C, k, dil, S, run_frames, seqlen, x_in, x_rows, part, part_stride, part_elems, b2, gamma,
                                                       rowvec, rv_ld, w, bias, g, b, x_out, x_out_rows, y, y_rows);
    if (form && form_cap) std::snprintf(form, form_cap, "%s", f.c_str());
}
int stn_op_fold_dwconv_ln_ex(stn_handle* h, int dtype, int B, int L, int C, int k, int dil, int S, int run_frames, const int32_t* seqlen,
                             const float* x_in, int64_t x_rows, const float* part, int64_t part_stride, int64_t part_elems, const float* b2,
                             const float* gamma, const float* rowvec, int rv_ld, const float* w, const float* bias, const float* g, const float* b,
                             float* x_out, int64_t x_out_rows, float* y, int64_t y_rows, char* form, size_t form_cap) {
    STN_TRY(h, fold_dwconv_ln_ex_checked(h, dtype, B, L, C, k, dil, S, run_frames, seqlen, x_in, x_rows, part, part_stride, part_elems, b2, gamma, rowvec,
                                         rv_ld, w, bias, g, b, x_out, x_out_rows, y, y_rows, form, form_cap))
}
int stn_dbg_fold_dwconv_ln_form(int dtype, int B, int L, int C, int k, int dil, int S, int has_rowvec, int run_frames, char* out, size_t cap) {
    std::string f;
    try { f = stn::fold_dwconv_ln_form(dtype, B, L, C, k, dil, S, has_rowvec != 0, run_frames).str(); } catch (const std::exception&) { return STN_ERR_INVALID; }
    if (out && cap > f.size()) std::memcpy(out, f.c_str(), f.size() + 1);
    return (int)f.size();
}
int stn_op_block_bench(stn_handle* h, int B, int L, int C, int I, int k, int dil, int mode, int iters, double* out2) {
    STN_TRY(h, { need(B > 0 && L > 0 && C > 0 && I > 0 && C % 8 == 0 && I % 8 == 0 && (k == 5 || k == 7) && dil > 0 && iters > 0 && out2 && (mode == 0 || mode == 2),
                      "stn_op_block_bench: bad argument");
                 h->eng->op_block_bench(B, L, C, I, k, dil, mode, iters, out2); })
}
int stn_op_randn(stn_handle* h, uint64_t seed, int B, int D, int L, const int64_t* utt_ids, const int32_t* len, float* out) {
    STN_TRY(h, { need(B > 0 && D > 0 && L > 0 && out, "stn_op_randn: bad argument"); h->eng->op_randn(seed, B, D, L, utt_ids, len, out); })
}

}  // extern "C"
