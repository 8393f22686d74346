// tts_host.hpp — the C++ call surface of the reference's host, on top of the C ABI (include/stn.h).
//
// Same names, argument meaning and error behaviour as /root/reference/cpp/helper.h:77-229:
//   loadTextToSpeech, loadVoiceStyle, TextToSpeech::call / batch / getSampleRate, writeWavFile, chunkText,
//   sanitizeFilename, timer, Style, Config
// minus everything ONNX-Runtime-specific (Ort::Env, Ort::MemoryInfo, arrayToTensor, clearTensorBuffers,
// the function-local statics that keep sessions alive): the engine handle owns all device state.
#pragma once
#include <chrono>
#include <cstdint>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/stn.h"
#include "../../../include/stn_group.h"
#include "text_frontend.hpp"

namespace stn {
namespace host {

struct Config {  // the four tts.json fields the reference reads (cpp/helper.cpp:811-815)
    struct { int sample_rate = 44100, base_chunk_size = 512; } ae;
    struct { int chunk_compress_factor = 6, latent_dim = 24; } ttl;
};
Config loadCfgs(const std::string& onnx_dir);

class Style {  // cpp/helper.h:57-72
   public:
    Style(std::vector<float> ttl, std::vector<int64_t> ttl_shape, std::vector<float> dp, std::vector<int64_t> dp_shape)
        : ttl_(std::move(ttl)), dp_(std::move(dp)), ttl_shape_(std::move(ttl_shape)), dp_shape_(std::move(dp_shape)) {}
    const std::vector<float>& getTtlData() const { return ttl_; }
    const std::vector<float>& getDpData() const { return dp_; }
    const std::vector<int64_t>& getTtlShape() const { return ttl_shape_; }
    const std::vector<int64_t>& getDpShape() const { return dp_shape_; }

   private:
    std::vector<float> ttl_, dp_;
    std::vector<int64_t> ttl_shape_, dp_shape_;
};
// voice-style JSON: {"style_ttl":{"data":[[[..]]],"dims":[1,d1,d2]},"style_dp":{...}} stacked along dim 0
Style loadVoiceStyle(const std::vector<std::string>& voice_style_paths, bool verbose = false);
// assets absent: deterministic N(0, 0.1^2) styles of the model's shapes (named "voices" map to seeds)
Style syntheticVoiceStyle(const std::vector<std::string>& voice_names, const stn_arch& arch);

struct EngineOptions {
    int device = 0;
    int dtype = STN_DTYPE_BF16;
    bool allow_synthetic = false;  // opt-in (CLI --synthetic, tests): no assets -> descriptor weights instead of the reference's
                                   // error on unreadable assets (cpp/helper.cpp:805)
    uint64_t weight_seed = 7;
    uint64_t noise_seed = 0;       // 0 -> from std::random_device per call, like the unseeded reference
    int gpus = 1;                  // > 1: the batch is dealt over this many devices (include/stn_group.h: devices `device`, device + 1, ...;
                                   // weights replicated, 16-bit PCM gathered into the first over RCCL).  CLI --gpus N
    std::vector<int> devices;      // explicit ordinals instead (size = gpus); the same ordinal repeated = a rehearsal on one GPU
    int output_rate = 0;           // Hz of the returned audio and the WAV files (resampled on the GPU, stn_set_output_rate); 0: the model's.
                                   // CLI --sample-rate HZ
    float loudness_lufs = std::numeric_limits<float>::quiet_NaN();  // normalize every utterance to this BS.1770-4 integrated loudness
                                   // (measured and scaled on the GPU, stn_set_loudness; the WAV files carry the normalized PCM); NaN: off.
                                   // CLI --loudness LUFS
    float loudness_ceiling_dbfs = -1.0f;  // sample-peak ceiling that caps the normalization gain.  CLI --peak-ceiling DBFS
    float limiter_ms = std::numeric_limits<float>::quiet_NaN();  // with loudness: the full loudness gain, the ceiling held by a look-ahead peak
                                   // limiter of this many milliseconds (stn_set_limiter, [0.5, 10]); NaN: off.  CLI --limiter MS
    bool true_peak = false;        // with loudness: the ceiling is a true-peak ceiling (dBTP, 4x oversampled; stn_set_peak_mode).  CLI --peak-mode {sample,true}
    bool loudness_scope_text = false;  // long-form call() with loudness on: the joined text normalized as one programme with one gain instead
                                   // of every chunk on its own.  One device only.  CLI --loudness-scope {chunk,text}
    bool trim_chunks = false;      // long-form call(): every chunk cut at its duration before the join.  CLI --trim-chunks
    float trim_silence_db = std::numeric_limits<float>::quiet_NaN();  // trim leading and trailing silence of every utterance by level on the
                                   // GPU (stn_set_silence_trim): frames more than this many dB below the loudest 10 ms frame; NaN: off.  One
                                   // device only.  CLI --trim-silence DB
    float max_pause_ms = std::numeric_limits<float>::quiet_NaN();  // with trim_silence_db: pauses inside an utterance longer than this many
                                   // milliseconds shortened to it on the GPU (stn_set_pause_limit); NaN: off.  CLI --max-pause MS
    float trim_keep_ms = 20.0f;    // milliseconds kept in front of and behind the speech.  CLI --trim-keep MS
    float trim_fade_ms = 5.0f;     // raised-cosine fade over each cut edge.  CLI --trim-fade MS
    std::vector<stn_filter> filters;  // every utterance through this chain of up to STN_MAX_FILTERS biquads on the GPU, after the resampler
                                   // and before everything above (stn_set_filters); empty: off.  CLI --filter TYPE:FREQ[:Q[:GAIN_DB]]
                                   // (repeatable) and --filter-preset {rumble,telephone}
    bool compressor_on = false;    // every utterance through the dynamic range compressor on the GPU, behind the filters and before everything
    stn_compressor compressor{-24.0f, 3.0f, 6.0f, 5.0f, 120.0f, 0.0f};  // above (stn_set_compressor); these are the "speech" preset's values.
                                   // CLI --compressor THRESHOLD:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:MAKEUP_DB]]]] and --compressor-preset speech
    bool expander_on = false;      // every utterance through the downward expander / noise gate on the GPU, behind the filters and in front of
    stn_expander expander{-50.0f, 3.0f, 6.0f, 24.0f, 1.0f, 30.0f, 150.0f};  // the de-esser (stn_set_expander); these are the "speech" preset's values.
                                   // CLI --expander THRESHOLD:RATIO[:KNEE[:RANGE_DB[:ATTACK_MS[:HOLD_MS[:RELEASE_MS]]]]] and --expander-preset {speech,gate}
    bool deesser_on = false;       // every utterance through the de-esser on the GPU, behind the filters and in front of the compressor
    stn_deesser deesser{5500.0f, -30.0f, 4.0f, 6.0f, 1.0f, 40.0f, 12.0f, STN_DEESS_SPLIT};  // (stn_set_deesser); these are the "speech" preset's values.
                                   // CLI --deesser FREQ:THRESHOLD[:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:RANGE_DB[:MODE]]]]]] and --deesser-preset speech
    int encoding = STN_ENC_PCM16;  // sample encoding of the returned audio and the WAV files (STN_ENC_*, stn.h; encoded on the GPU).  PCM16
                                   // keeps the float waveform and writeWavFile's files.  CLI --encoding {pcm16,pcm24,f32,mulaw,alaw}
    float pitch = 0.0f;            // every utterance shifted by this many semitones ([-12, 12]) on the GPU without a change of length, in front of
                                   // everything above (stn_set_pitch); 0: off.  CLI --pitch SEMITONES
    int pitch_mode = STN_PITCH_RESAMPLE;  // what the shift does to the formants (stn_set_pitch_mode): they move with the pitch, or with
                                   // STN_PITCH_FORMANT the spectral envelope is put back on the GPU; no effect while pitch is 0.
                                   // CLI --pitch-mode {resample,formant}
    int dither = STN_DITHER_OFF;   // how 16- and 24-bit PCM is quantized on the GPU (stn_set_dither): STN_DITHER_OFF truncates as writeWavFile;
    uint64_t dither_seed = 0;      // _ROUND, _TPDF, _TPDF_HP round, behind dither keyed by this seed.  With a mode set, PCM16 is fetched as
                                   // 16-bit samples (not as floats for writeWavFile).  CLI --dither {off,round,tpdf,tpdf-hp} and --dither-seed N
};

// The command line's filter arguments (host only).  parseFilterSpec: "TYPE:FREQ[:Q[:GAIN_DB]]" (TYPE one of highpass, lowpass, notch,
// peak, lowshelf, highshelf; Q 0.7071 and 0 dB when left out) into f, or why not.  filterPreset: "rumble" (a high-pass at 80 Hz) or
// "telephone" (a 4th-order Butterworth band: high-pass 300 Hz and low-pass 3400 Hz, each as sections of Q 0.541 and 1.307) appended to
// out, or why not.  The numeric limits are stn_set_filters' own.
std::string parseFilterSpec(const std::string& spec, stn_filter& f);
std::string filterPreset(const std::string& name, std::vector<stn_filter>& out);
// The command line's compressor arguments (host only).  parseCompressorSpec: "THRESHOLD:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:MAKEUP_DB]]]]"
// (the speech preset's knee 6 dB, attack 5 ms, release 120 ms and makeup 0 dB when left out) into c, or why not.  compressorPreset:
// "speech" (-24 dB, 3:1 and those) into c, or why not.  The numeric limits are stn_set_compressor's own.
std::string parseCompressorSpec(const std::string& spec, stn_compressor& c);
std::string compressorPreset(const std::string& name, stn_compressor& c);
// The command line's de-esser arguments (host only).  parseDeesserSpec: "FREQ:THRESHOLD[:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:RANGE_DB[:MODE]]]]]]"
// (the speech preset's values for what is left out; MODE split or wide) into c, or why not.  deesserPreset: "speech" (5500 Hz, -30 dB,
// 4:1, knee 6 dB, 1 ms, 40 ms, range 12 dB, split) into c, or why not.  The numeric limits are stn_set_deesser's own.
std::string parseDeesserSpec(const std::string& spec, stn_deesser& c);
std::string deesserPreset(const std::string& name, stn_deesser& c);
// The command line's expander arguments (host only).  parseExpanderSpec: "THRESHOLD:RATIO[:KNEE[:RANGE_DB[:ATTACK_MS[:HOLD_MS[:RELEASE_MS]]]]]"
// (the values of `preset` for what is left out, as binding.parse_expander_spec takes them) into c, or why not.  expanderPreset: "speech"
// (-50 dB, 3:1, knee 6 dB, range 24 dB, 1 ms, 30 ms, 150 ms) or "gate" (-45 dB, 20:1, knee 0, range 60 dB, 0.5 ms, 50 ms, 100 ms) into c,
// or why not.  The numeric limits are stn_set_expander's own.
std::string parseExpanderSpec(const std::string& spec, stn_expander& c, const std::string& preset = "speech");
std::string expanderPreset(const std::string& name, stn_expander& c);
// The command line's dither mode (host only): "off", "round", "tpdf" or "tpdf-hp" into mode (STN_DITHER_*), or why not
std::string parseDitherMode(const std::string& name, int& mode);

class TextToSpeech {
   public:
    // wav: the float waveform [B][W].  With an encoding other than PCM16 (setEncoding), or with a dither mode set (setDither), the audio
    // is `encoded` instead: [B][W] samples of stn_encoding_bytes(encoding) bytes, as the engine's encoded fetch delivers them, and wav is empty.
    // length: with silence trimming on (setSilenceTrim), the samples each row holds from column 0, its trimmed segment (empty: off).
    struct SynthesisResult { std::vector<float> wav; std::vector<float> duration; std::vector<unsigned char> encoded; int encoding = STN_ENC_PCM16; std::vector<int64_t> length; };

    TextToSpeech(stn_handle* engine, UnicodeProcessor text_processor, const Config& cfgs, uint64_t noise_seed);
    // several devices: the group owns the handles (engine() is rank 0's); batch() / call() deal their utterances over the group
    TextToSpeech(stn_group* group, UnicodeProcessor text_processor, const Config& cfgs, uint64_t noise_seed);
    ~TextToSpeech();
    TextToSpeech(const TextToSpeech&) = delete;

    // long-form: chunkText -> the chunks as one batch -> joined with `silence_duration` of zeros by the fetch on the GPU
    // (cpp/helper.cpp:685-723; the encoding's zero codeword with an encoding set; on a group, joined on the host)
    SynthesisResult call(const std::string& text, const std::string& lang, const Style& style, int total_step,
                         float speed = 1.05f, float silence_duration = 0.3f);
    // batch: one padded batch, no chunking (cpp/helper.cpp:725-734)
    SynthesisResult batch(const std::vector<std::string>& text_list, const std::vector<std::string>& lang_list,
                          const Style& style, int total_step, float speed = 1.05f);
    // rate of the returned audio: the output rate when one is set, else the model's (cfgs.ae.sample_rate, which keeps sizing the latent)
    int getSampleRate() const { return out_rate_ ? out_rate_ : cfgs_.ae.sample_rate; }
    void setOutputRate(int hz) { out_rate_ = hz == cfgs_.ae.sample_rate ? 0 : hz; }
    // the engine's dither mode (set on it by loadTextToSpeech): with one set, PCM16 results are the GPU's 16-bit samples (`encoded`): the
    // float waveform would be truncated by writeWavFile, without the dither.  A group's PCM16 gather is dithered as it is.
    void setDither(int mode) { dither_ = mode; }
    void setEncoding(int enc);  // STN_ENC_*: the encoding of the audio batch() / call() return (and of a group's gather)
    // call() with loudness normalization on: false (default), every chunk its own gain; true, the joined text measured as one
    // BS.1770 programme and scaled by one gain (stn.h, STN_JOIN_GAIN_PROG).  Refused on a group: its chunks sit on several devices.
    void setLoudnessScope(bool whole_text);
    // call(): every chunk cut at its reported duration before the join (the reference's Rust host) instead of its whole wave
    void setTrimChunks(bool on) { trim_chunks_ = on; }
    // every utterance without its leading and trailing silence (stn_set_silence_trim; stn.h "silence trimming"): batch() rows hold the
    // trimmed segment from column 0 (SynthesisResult::length), call() joins the segments.  Refused on a group.
    void setSilenceTrim(bool on, float top_db = 40.0f, float keep_ms = 20.0f, float fade_ms = 5.0f);
    // with silence trimming on: every pause inside an utterance longer than max_pause_ms shortened to it (stn_set_pause_limit; stn.h
    // "pause limit"); the lengths are then what the cuts leave.  One device only, and refused without trimming.
    void setPauseLimit(bool on, float max_pause_ms = 300.0f);
    // The loudness of what the last batch() / call() returned, measured on the GPU before the loudness gain (stn.h "loudness range"):
    // per row after batch() (and after a call() that was one chunk), one entry for the joined text after call().  integrated, peak and
    // gain as stn_batch_loudness / stn_batch_join_loudness report them; max_momentary and max_short_term in LUFS (-inf where the
    // audio is shorter than 400 ms / 3 s); range in LU; n_short_term the 3 s windows behind the range's gates.  Refused on a group.
    struct LoudnessReport { std::vector<float> integrated, peak, gain, max_momentary, max_short_term, range; std::vector<int32_t> n_short_term; };
    LoudnessReport loudnessReport();
    // The pitch of what the last batch() / call() returned, tracked on the GPU by YIN on the signal loudnessReport measures (stn.h
    // "f0"; the default parameters): per row after batch() (and after a call() that was one chunk), one entry for the joined text
    // after call(), its statistics pooled on the host over the chunks' frames.  Hz; 0 where no frame is voiced.  Refused on a group.
    struct PitchReport { std::vector<stn_f0_stats> stats; };
    PitchReport pitchReport();
    int encoding() const { return enc_; }
    stn_handle* engine() const { return h_; }
    stn_group* group() const { return grp_; }  // null with one device
    bool synthetic() const { return synthetic_; }
    void markSynthetic() { synthetic_ = true; }

   private:
    SynthesisResult infer(const std::vector<std::string>& text_list, const std::vector<std::string>& lang_list,
                          const Style& style, int total_step, float speed);
    void runBatch(const TokenBatch& tb, const std::vector<float>& mask, const Style& style, int total_step, float speed);
    bool scope_text_ = false, trim_chunks_ = false, trim_silence_ = false, pause_limit_ = false;
    stn_handle* h_;
    stn_group* grp_ = nullptr;
    UnicodeProcessor text_processor_;
    Config cfgs_;
    uint64_t noise_seed_;
    uint64_t calls_ = 0;
    int out_rate_ = 0;  // 0: the model's rate
    int enc_ = STN_ENC_PCM16;
    int dither_ = STN_DITHER_OFF;
    bool encodedFetch() const { return enc_ != STN_ENC_PCM16 || dither_ != STN_DITHER_OFF; }
    int32_t join_members_ = 0;  // the last result: a join of this many rows with join_silence_ between them (0: the batch's rows)
    float join_silence_ = 0.f;
    bool synthetic_ = false;
};

// use_gpu=true is the only mode (the reference only had use_gpu=false and threw on true, cpp/helper.cpp:909-911)
std::unique_ptr<TextToSpeech> loadTextToSpeech(const std::string& onnx_dir, bool use_gpu = true,
                                               const EngineOptions& opts = EngineOptions());

inline void writeWavFile(const std::string& filename, const std::vector<float>& audio_data, int sample_rate) {
    write_wav_file(filename, audio_data, sample_rate);
}
// already-encoded samples (TextToSpeech::SynthesisResult::encoded) as a WAV file (stn_wav_encode_as's layout)
inline void writeWavFileEncoded(const std::string& filename, int enc, const unsigned char* samples, size_t n, int sample_rate) {
    const std::vector<unsigned char> w = wav_bytes_encoded(enc, samples, n, sample_rate);
    std::ofstream f(filename, std::ios::binary);
    if (!f.is_open()) throw std::runtime_error("Failed to open file for writing: " + filename);
    f.write(reinterpret_cast<const char*>(w.data()), (std::streamsize)w.size());
}
inline std::vector<std::string> chunkText(const std::string& text, int max_len = 300) { return chunk_text(text, max_len); }
inline std::string sanitizeFilename(const std::string& text, int max_len) { return sanitize_filename(text, max_len); }

template <typename Func>
auto timer(const std::string& name, Func&& func) -> decltype(func()) {  // cpp/helper.h:213-223
    const auto t0 = std::chrono::steady_clock::now();
    std::cout << name << "..." << std::endl;
    auto result = func();
    const std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
    std::cout << "  -> " << name << " completed in " << std::fixed << std::setprecision(2) << dt.count() << " sec" << std::endl;
    return result;
}

}  // namespace host
}  // namespace stn
