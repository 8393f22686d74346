// example_native.cpp — command-line driver with the reference's flags (/root/reference/cpp/example_onnx.cpp:35-50):
//   --onnx-dir --total-step --speed --n-test --voice-style --text --lang --save-dir --batch
// plus engine flags: --device N, --gpus N (deal the batch over N devices: include/stn_group.h), --devices a,b,.. (explicit ordinals),
// --dtype {fp32,bf16,fp16}, --seed S (0 = unseeded noise, like the reference), --sample-rate HZ (WAV files at HZ, resampled on the GPU;
// absent: the model's rate), --loudness LUFS (every utterance normalized to that BS.1770-4 integrated loudness on the GPU; absent: off),
// --peak-ceiling DBFS (the sample peak the loudness gain may reach; default -1), --peak-mode {sample,true} (with --loudness: the ceiling
// as a sample peak or as a true peak, 4x oversampled), --limiter MS (with --loudness: the full loudness gain,
// and a look-ahead peak limiter of MS milliseconds, 0.5 to 10, holds the ceiling instead of a capped gain), --encoding {pcm16,pcm24,f32,mulaw,alaw} (sample format
// of the WAV files, encoded on the GPU; default pcm16, writeWavFile's files), --loudness-scope {chunk,text} (a long text with --loudness:
// every chunk normalized on its own, the default, or the joined text as one programme with one gain; text needs one GPU),
// --trim-chunks (a long text's chunks cut at their durations before they are joined), --trim-silence DB (leading and trailing silence of
// every utterance trimmed by level on the GPU: frames more than DB below the loudest 10 ms frame; the files then hold the trimmed
// segments; one GPU only), --max-pause MS (with --trim-silence: pauses inside an utterance longer than MS shortened to MS), --trim-keep MS (kept in front of and behind the speech; default 20), --trim-fade MS (fade over a cut edge; default 5),
// --filter TYPE:FREQ[:Q[:GAIN_DB]] (repeatable, up to 8: every utterance through that biquad on the GPU, after the resampler and before
// everything else; TYPE one of highpass, lowpass, notch, peak, lowshelf, highshelf; Q 0.7071 when left out), --filter-preset
// {rumble,telephone} (a high-pass at 80 Hz; the 300 to 3400 Hz telephone band, in front of any --filter),
// --compressor THRESHOLD:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:MAKEUP_DB]]]] (every utterance through the dynamic range compressor on the
// GPU, behind the filters and before everything else; knee 6 dB, attack 5 ms, release 120 ms, makeup 0 dB when left out),
// --compressor-preset speech (-24 dB, 3:1 and those),
// --deesser FREQ:THRESHOLD[:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:RANGE_DB[:MODE]]]]]] (every utterance through the de-esser on the GPU,
// behind the filters and in front of the compressor: the band above FREQ turned down by up to RANGE_DB while its level is over THRESHOLD;
// ratio 4, knee 6 dB, attack 1 ms, release 40 ms, range 12 dB, MODE split (the band alone; wide: the whole signal) when left out),
// --deesser-preset speech (5500 Hz, -30 dB and those),
// --expander THRESHOLD:RATIO[:KNEE[:RANGE_DB[:ATTACK_MS[:HOLD_MS[:RELEASE_MS]]]]] (every utterance through the downward expander / noise
// gate on the GPU, behind the filters and in front of the de-esser: what lies under THRESHOLD turned down by up to RANGE_DB; knee 6 dB,
// range 24 dB, attack 1 ms, hold 30 ms, release 150 ms when left out, or the values of the preset given beside it),
// --expander-preset {speech,gate} (-50 dB, 3:1 and those; -45 dB, 20:1, no knee, 60 dB, 0.5 ms, 50 ms, 100 ms),
// --pitch SEMITONES (every utterance shifted by that many semitones, -12 to 12, on the GPU without a change of length, in front of
// everything else; absent or 0: off),
// --pitch-mode {resample,formant} (what --pitch does to the formants: they move with the pitch, the default, or the spectral envelope
// of the audio before the shift is put back on the GPU),
// --loudness-report (after each saved file one line "Loudness: integrated .. LUFS, range .. LU, max momentary .. LUFS, max short-term ..
// LUFS (N short-term windows), peak .., gain ..": measured on the GPU before the loudness gain, three decimals, a long text as the
// joined programme; one GPU only),
// --pitch-report (after each saved file one line "Pitch: median .. Hz, min .. Hz, max .. Hz, voiced .. % (V of F frames)": the YIN
// track of the same signal on the GPU, 60 to 500 Hz at a 10 ms hop, three decimals, a long text pooled over its chunks; one GPU only).
// Voice styles: paths to voice-style JSON files; when the model assets are absent (synthetic weights) a
// non-existing path is taken as a voice NAME and mapped to a deterministic synthetic style.
#include <sys/stat.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <fstream>
#include <iostream>

#include "../host/tts_host.hpp"

using namespace stn::host;

namespace {
std::vector<std::string> split(const std::string& s, char delim) {
    std::vector<std::string> out;
    size_t a = 0, p;
    while ((p = s.find(delim, a)) != std::string::npos) { out.push_back(s.substr(a, p - a)); a = p + 1; }
    out.push_back(s.substr(a));
    return out;
}
bool exists(const std::string& p) { std::ifstream f(p); return f.is_open(); }
std::string db3(float v) {  // three decimals, the infinities spelled "-inf" / "inf"
    if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
    char buf[32];
    std::snprintf(buf, sizeof(buf), "%.3f", (double)v);
    return buf;
}
void make_dirs(const std::string& path) {
    for (size_t i = 1; i <= path.size(); ++i)
        if (i == path.size() || path[i] == '/') ::mkdir(path.substr(0, i).c_str(), 0755);
}
}  // namespace

int main(int argc, char* argv[]) {
    std::cout << "=== TTS Inference on MI355X (native HIP engine) ===\n\n";
    std::string onnx_dir = "../assets/onnx", save_dir = "results";
    int total_step = 5, n_test = 4;
    float speed = 1.05f;
    std::vector<std::string> voice_style = {"../assets/voice_styles/M1.json"};
    std::vector<std::string> text = {"This morning, I took a walk in the park, and the sound of the birds and the breeze was so "
                                     "pleasant that I stopped for a long time just to listen."};
    std::vector<std::string> lang = {"en"};
    bool batch = false, peak_mode_given = false, loudness_report = false, pitch_report = false;
    std::string xp_spec, xp_preset = "speech";  // --expander and --expander-preset as given so far
    bool xp_spelled = false;
    EngineOptions opts;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool more = i + 1 < argc;
        if (a == "--onnx-dir" && more) onnx_dir = argv[++i];
        else if (a == "--total-step" && more) total_step = std::atoi(argv[++i]);
        else if (a == "--speed" && more) speed = (float)std::atof(argv[++i]);
        else if (a == "--n-test" && more) n_test = std::atoi(argv[++i]);
        else if (a == "--voice-style" && more) voice_style = split(argv[++i], ',');
        else if (a == "--text" && more) text = split(argv[++i], '|');
        else if (a == "--lang" && more) lang = split(argv[++i], ',');
        else if (a == "--save-dir" && more) save_dir = argv[++i];
        else if (a == "--batch") batch = true;
        else if (a == "--device" && more) opts.device = std::atoi(argv[++i]);
        else if (a == "--gpus" && more) opts.gpus = std::atoi(argv[++i]);  // > 1: the batch is dealt over devices device .. device + N - 1
        else if (a == "--devices" && more) { for (const std::string& d : split(argv[++i], ',')) opts.devices.push_back(std::atoi(d.c_str())); }
        else if (a == "--dtype" && more) { const std::string d = argv[++i]; opts.dtype = d == "fp32" ? STN_DTYPE_F32 : d == "fp16" ? STN_DTYPE_F16 : STN_DTYPE_BF16; }
        else if (a == "--seed" && more) opts.noise_seed = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--sample-rate" && more) opts.output_rate = std::atoi(argv[++i]);  // Hz of the WAV files (resampled on the GPU); absent: the model's
        else if (a == "--loudness" && more) opts.loudness_lufs = std::strtof(argv[++i], nullptr);  // LUFS of every utterance (BS.1770-4, on the GPU); absent: off
        else if (a == "--peak-ceiling" && more) opts.loudness_ceiling_dbfs = std::strtof(argv[++i], nullptr);  // dBFS cap of the loudness gain (default -1)
        else if (a == "--limiter" && more) opts.limiter_ms = std::strtof(argv[++i], nullptr);  // ms of look-ahead of the peak limiter behind the loudness gain; absent: off
        else if (a == "--peak-mode" && more) {  // with --loudness: the ceiling as a sample peak (default) or a true peak (dBTP, 4x oversampled on the GPU)
            const std::string v = argv[++i];
            if (v != "sample" && v != "true") { std::cerr << "Error: --peak-mode " << v << ": sample or true\n"; return 1; }
            opts.true_peak = v == "true";
            peak_mode_given = true;
        }
        else if (a == "--encoding" && more) {  // sample format of the WAV files (encoded on the GPU); default pcm16
            const std::string e = argv[++i];
            opts.encoding = e == "pcm16" ? STN_ENC_PCM16 : e == "pcm24" ? STN_ENC_PCM24 : e == "f32" ? STN_ENC_F32 : e == "mulaw" ? STN_ENC_MULAW : e == "alaw" ? STN_ENC_ALAW : -1;
            if (opts.encoding < 0) { std::cerr << "Error: --encoding " << e << ": one of pcm16, pcm24, f32, mulaw, alaw\n"; return 1; }
        }
        else if (a == "--loudness-scope" && more) {  // long texts with --loudness: every chunk its own gain (chunk), or the joined text one gain (text)
            const std::string v = argv[++i];
            if (v != "chunk" && v != "text") { std::cerr << "Error: --loudness-scope " << v << ": chunk or text\n"; return 1; }
            opts.loudness_scope_text = v == "text";
        }
        else if (a == "--trim-chunks") opts.trim_chunks = true;  // long texts: every chunk cut at its duration before the join
        else if (a == "--trim-silence" && more) opts.trim_silence_db = std::strtof(argv[++i], nullptr);  // dB below the loudest frame that counts as silence; absent: off
        else if (a == "--max-pause" && more) opts.max_pause_ms = std::strtof(argv[++i], nullptr);  // ms: longer pauses inside an utterance are shortened to this; absent: off
        else if (a == "--trim-keep" && more) opts.trim_keep_ms = std::strtof(argv[++i], nullptr);  // ms kept around the speech (default 20)
        else if (a == "--trim-fade" && more) opts.trim_fade_ms = std::strtof(argv[++i], nullptr);  // ms of fade over a cut edge (default 5)
        else if (a == "--filter" && more) {  // one biquad of the chain every utterance goes through on the GPU; repeatable
            stn_filter f;
            const std::string why = parseFilterSpec(argv[++i], f);
            if (!why.empty()) { std::cerr << "Error: --" << why << "\n"; return 1; }
            opts.filters.push_back(f);
        }
        else if (a == "--filter-preset" && more) {  // a named chain, expanded here, in front of any --filter
            std::vector<stn_filter> p;
            const std::string why = filterPreset(argv[++i], p);
            if (!why.empty()) { std::cerr << "Error: --" << why << "\n"; return 1; }
            opts.filters.insert(opts.filters.begin(), p.begin(), p.end());
        }
        else if ((a == "--compressor" || a == "--compressor-preset") && more) {  // the dynamic range compressor every utterance goes through on the GPU
            const std::string why = a == "--compressor" ? parseCompressorSpec(argv[++i], opts.compressor) : compressorPreset(argv[++i], opts.compressor);
            if (!why.empty()) { std::cerr << "Error: --" << why << "\n"; return 1; }
            opts.compressor_on = true;
        }
        else if ((a == "--deesser" || a == "--deesser-preset") && more) {  // the de-esser every utterance goes through on the GPU
            const std::string why = a == "--deesser" ? parseDeesserSpec(argv[++i], opts.deesser) : deesserPreset(argv[++i], opts.deesser);
            if (!why.empty()) { std::cerr << "Error: --" << why << "\n"; return 1; }
            opts.deesser_on = true;
        }
        else if ((a == "--expander" || a == "--expander-preset") && more) {  // the downward expander / noise gate every utterance goes through on the GPU
            // (a spelling takes what it leaves out from the preset given, "speech" without one, whichever of the two comes first)
            if (a == "--expander") { xp_spec = argv[++i]; xp_spelled = true; }
            else xp_preset = argv[++i];
            const std::string why = xp_spelled ? parseExpanderSpec(xp_spec, opts.expander, xp_preset) : expanderPreset(xp_preset, opts.expander);
            if (!why.empty()) { std::cerr << "Error: --" << why << "\n"; return 1; }
            opts.expander_on = true;
        }
        else if (a == "--pitch" && more) {  // every utterance shifted by this many semitones on the GPU (length unchanged); 0: off
            const std::string v = argv[++i];
            char* end = nullptr;
            opts.pitch = std::strtof(v.c_str(), &end);
            if (v.empty() || *end) { std::cerr << "Error: --pitch '" << v << "': a number of semitones in [-12, 12]\n"; return 1; }
            const char* why = stn_pitch_error(opts.pitch);
            if (why[0]) { std::cerr << "Error: --" << why << "\n"; return 1; }
        }
        else if (a == "--pitch-mode" && more) {  // what --pitch does to the formants
            const std::string v = argv[++i];
            if (v == "resample") opts.pitch_mode = STN_PITCH_RESAMPLE;
            else if (v == "formant") opts.pitch_mode = STN_PITCH_FORMANT;
            else { std::cerr << "Error: --pitch-mode '" << v << "': resample or formant\n"; return 1; }
        }
        else if (a == "--dither" && more) {  // how pcm16 / pcm24 files are quantized on the GPU: truncation (off, the default), rounding, or rounding behind dither
            const std::string why = parseDitherMode(argv[++i], opts.dither);
            if (!why.empty()) { std::cerr << "Error: --" << why << "\n"; return 1; }
        }
        else if (a == "--dither-seed" && more) {  // seed of the dither noise (default 0)
            const std::string v = argv[++i];
            char* end = nullptr;
            opts.dither_seed = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || *end || v[0] == '-') { std::cerr << "Error: --dither-seed '" << v << "': an unsigned integer\n"; return 1; }
        }
        else if (a == "--loudness-report") loudness_report = true;  // one line of loudness figures after each saved file
        else if (a == "--pitch-report") pitch_report = true;  // one line of pitch figures after each saved file
        else if (a == "--synthetic") opts.allow_synthetic = true;  // no model assets: run the default architecture on synthetic weights
    }
    if (opts.filters.size() > (size_t)STN_MAX_FILTERS) {
        std::cerr << "Error: --filter / --filter-preset: " << opts.filters.size() << " sections, at most " << STN_MAX_FILTERS << "\n";
        return 1;
    }
    if (peak_mode_given && std::isnan(opts.loudness_lufs)) {
        std::cerr << "Error: --peak-mode needs --loudness (it is the ceiling of the loudness gain)\n";
        return 1;
    }
    if (!std::isnan(opts.max_pause_ms) && std::isnan(opts.trim_silence_db)) {
        std::cerr << "Error: --max-pause needs --trim-silence (pauses are shortened inside trimmed utterances)\n";
        return 1;
    }
    if (!std::isnan(opts.limiter_ms) && std::isnan(opts.loudness_lufs)) {
        std::cerr << "Error: --limiter needs --loudness (the limiter holds the ceiling of the loudness gain)\n";
        return 1;
    }
    if ((loudness_report || pitch_report) && (opts.gpus > 1 || opts.devices.size() > 1)) {
        std::cerr << "Error: " << (loudness_report ? "--loudness-report" : "--pitch-report") << " needs the batch on one device (leave --gpus N / --devices out)\n";
        return 1;
    }
    if (voice_style.size() != text.size()) {
        std::cerr << "Error: Number of voice styles (" << voice_style.size() << ") must match number of texts (" << text.size() << ")\n";
        return 1;
    }
    if (lang.size() != text.size()) {
        std::cerr << "Error: Number of languages (" << lang.size() << ") must match number of texts (" << text.size() << ")\n";
        return 1;
    }
    const int bsz = (int)voice_style.size();
    try {
        auto tts = loadTextToSpeech(onnx_dir, true, opts);
        std::cout << std::endl;
        stn_arch arch;
        stn_get_arch(tts->engine(), &arch);
        // voice styles are files (loadVoiceStyle throws on a missing one, cpp/helper.cpp:835); only an engine on synthetic
        // weights, given NO existing file at all, maps the names to deterministic synthetic styles
        bool any_file = false;
        for (auto& p : voice_style) any_file = any_file || exists(p);
        const bool by_name = tts->synthetic() && !any_file;
        const Style style = by_name ? syntheticVoiceStyle(voice_style, arch) : loadVoiceStyle(voice_style, true);
        if (by_name) std::cout << "Voice style files not found -> synthetic styles keyed by name" << std::endl;
        make_dirs(save_dir);
        for (int n = 0; n < n_test; ++n) {
            std::cout << "\n[" << (n + 1) << "/" << n_test << "] Starting synthesis...\n";
            auto result = timer("Generating speech from text", [&]() {
                return batch ? tts->batch(text, lang, style, total_step, speed) : tts->call(text[0], lang[0], style, total_step, speed);
            });
            const int sr = tts->getSampleRate();
            TextToSpeech::LoudnessReport rep;
            if (loudness_report) rep = tts->loudnessReport();
            TextToSpeech::PitchReport pit;
            if (pitch_report) pit = tts->pitchReport();
            const size_t eb = result.wav.empty() ? (size_t)stn_encoding_bytes(result.encoding) : 0;  // 0: the float waveform
            const size_t per = (eb ? result.encoded.size() / eb : result.wav.size()) / (size_t)bsz;
            for (int b = 0; b < bsz; ++b) {
                const std::string fname = sanitizeFilename(text[b], 20) + "_" + std::to_string(n + 1) + ".wav";
                size_t wav_len = (size_t)(int)((float)sr * result.duration[b]);
                if (!result.length.empty()) wav_len = (size_t)result.length[(size_t)b];  // trimmed: the segment the GPU delivered
                if (wav_len > per) wav_len = per;
                if (eb) {
                    writeWavFileEncoded(save_dir + "/" + fname, result.encoding, result.encoded.data() + b * per * eb, wav_len, sr);
                } else {
                    std::vector<float> out(result.wav.begin() + (long)(b * per), result.wav.begin() + (long)(b * per + wav_len));
                    writeWavFile(save_dir + "/" + fname, out, sr);
                }
                std::cout << "Saved: " << save_dir << "/" << fname << "\n";
                if (loudness_report && (size_t)b < rep.integrated.size())
                    std::cout << "Loudness: integrated " << db3(rep.integrated[b]) << " LUFS, range " << db3(rep.range[b]) << " LU, max momentary "
                              << db3(rep.max_momentary[b]) << " LUFS, max short-term " << db3(rep.max_short_term[b]) << " LUFS ("
                              << rep.n_short_term[b] << " short-term windows), peak " << db3(rep.peak[b]) << ", gain " << db3(rep.gain[b]) << "\n";
                if (pitch_report && (size_t)b < pit.stats.size()) {
                    const stn_f0_stats& s = pit.stats[(size_t)b];
                    std::cout << "Pitch: median " << db3(s.median_hz) << " Hz, min " << db3(s.min_hz) << " Hz, max " << db3(s.max_hz) << " Hz, voiced "
                              << db3(s.frames ? 100.0f * (float)s.voiced / (float)s.frames : 0.0f) << " % (" << s.voiced << " of " << s.frames << " frames)\n";
                }
            }
        }
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << "\n";
        return 2;
    }
    std::cout << "\n=== Synthesis completed successfully! ===\n";
    return 0;
}
