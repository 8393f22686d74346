#include "tts_host.hpp"

#include <cmath>
#include <cstring>
#include <fstream>
#include <numeric>
#include <random>
#include <stdexcept>

#include "json_min.hpp"

namespace stn {
namespace host {

namespace {
void check(stn_handle* h, int rc) {
    if (rc != STN_OK) throw std::runtime_error(std::string("engine: ") + stn_last_error(h));
}
// with silence trimming on: the samples each row of the finished batch holds (the segments the fetch delivered)
std::vector<int64_t> trimmed_lengths(stn_handle* h, int B, bool pause_limit) {
    if (pause_limit) {  // what the cuts leave of the segment
        std::vector<int64_t> len((size_t)B);
        check(h, stn_batch_pauses(h, len.data(), nullptr, nullptr, 0));
        return len;
    }
    std::vector<int64_t> start((size_t)B), end((size_t)B);
    check(h, stn_batch_silence_edges(h, start.data(), end.data()));
    for (int b = 0; b < B; ++b) end[(size_t)b] -= start[(size_t)b];
    return end;
}
// what a group (several devices) refuses, said once: loadTextToSpeech refuses before anything is created, the instance where it is asked
std::string groupRefusesScopeText() {
    return "loudness scope 'text' needs the chunks of a text on one device: a group deals them over its devices "
           "(use one GPU, or the default scope 'chunk')";
}
std::string groupRefusesTrimChunks() { return "trimmed chunks need the chunks of a text on one device (a group keeps the untrimmed host join)"; }
std::string groupRefusesSilenceTrim() {
    return "silence trimming needs every utterance on one device: a group (--gpus N, --devices) does not trim (use one GPU, or leave --trim-silence out)";
}
std::string groupRefusesPauseLimit() {
    return "the pause limit needs every utterance on one device: a group (--gpus N, --devices) does not trim (use one GPU, or leave --max-pause out)";
}
}  // namespace

TextToSpeech::TextToSpeech(stn_handle* engine, UnicodeProcessor tp, const Config& cfgs, uint64_t noise_seed)
    : h_(engine), text_processor_(std::move(tp)), cfgs_(cfgs), noise_seed_(noise_seed) {}
TextToSpeech::TextToSpeech(stn_group* group, UnicodeProcessor tp, const Config& cfgs, uint64_t noise_seed)
    : h_(stn_group_handle(group, 0)), grp_(group), text_processor_(std::move(tp)), cfgs_(cfgs), noise_seed_(noise_seed) {}
TextToSpeech::~TextToSpeech() {
    if (grp_) stn_group_destroy(grp_);  // (owns the handles)
    else stn_destroy(h_);
}

TextToSpeech::SynthesisResult TextToSpeech::infer(const std::vector<std::string>& text_list,
                                                  const std::vector<std::string>& lang_list, const Style& style,
                                                  int total_step, float speed) {
    const int bsz = (int)text_list.size();
    if (bsz != style.getTtlShape()[0]) throw std::runtime_error("Number of texts must match number of style vectors");
    const TokenBatch tb = text_processor_(text_list, lang_list);
    const std::vector<float> mask = tb.mask();
    if (grp_) {
        // several devices: deal, synthesize, gather the 16-bit PCM into the first device (RCCL) and fetch it in caller order.  The
        // float waveform handed back is the centre-ish representative of each sample's quantisation cell, (pcm +- 0.5) / 32767, whose
        // re-quantisation by writeWavFile (clamp, * 32767, truncation: cpp/helper.cpp:986-987) gives exactly the gathered PCM.
        uint64_t seed = noise_seed_;
        if (seed == 0) { std::random_device rd; seed = ((uint64_t)rd() << 32) | rd(); }
        else seed += calls_;
        ++calls_;
        int64_t W = 0;
        if (stn_group_synthesize(grp_, bsz, tb.Lt, tb.ids.data(), mask.data(), style.getTtlData().data(), style.getDpData().data(), total_step, speed,
                                 nullptr, seed, &W) != STN_OK)
            throw std::runtime_error(std::string("engine group: ") + stn_group_last_error(grp_));
        SynthesisResult r;
        r.duration.resize(bsz);
        r.encoding = enc_;
        std::vector<unsigned char> data((size_t)bsz * (size_t)W * stn_encoding_bytes(enc_));
        if (stn_group_fetch_encoded(grp_, data.data(), data.size(), r.duration.data()) != STN_OK)
            throw std::runtime_error(std::string("engine group: ") + stn_group_last_error(grp_));
        if (enc_ != STN_ENC_PCM16) { r.encoded = std::move(data); return r; }
        std::vector<int16_t> pcm((size_t)bsz * (size_t)W);
        std::memcpy(pcm.data(), data.data(), data.size());
        r.wav.resize(pcm.size());
        for (size_t i = 0; i < pcm.size(); ++i) r.wav[i] = pcm[i] == 0 ? 0.f : ((float)pcm[i] + (pcm[i] > 0 ? 0.5f : -0.5f)) / 32767.0f;
        return r;
    }
    runBatch(tb, mask, style, total_step, speed);
    join_members_ = 0;
    int B = 0, L = 0;
    int64_t W = 0;
    check(h_, stn_batch_dims(h_, &B, &L, &W));
    SynthesisResult r;
    r.duration.resize(B);
    r.encoding = enc_;
    if (encodedFetch()) {
        r.encoded.resize((size_t)B * W * stn_encoding_bytes(enc_));
        check(h_, stn_batch_fetch_encoded(h_, enc_, r.encoded.data(), r.encoded.size(), r.duration.data()));
        if (trim_silence_) r.length = trimmed_lengths(h_, B, pause_limit_);
        return r;
    }
    r.wav.resize((size_t)B * W);
    check(h_, stn_batch_fetch(h_, r.wav.data(), r.wav.size(), r.duration.data()));
    if (trim_silence_) r.length = trimmed_lengths(h_, B, pause_limit_);
    return r;
}

void TextToSpeech::setSilenceTrim(bool on, float top_db, float keep_ms, float fade_ms) {
    if (on && grp_) throw std::runtime_error(groupRefusesSilenceTrim());
    check(h_, stn_set_silence_trim(h_, on ? 1 : 0, top_db, keep_ms, fade_ms));
    trim_silence_ = on;
}

void TextToSpeech::setPauseLimit(bool on, float max_pause_ms) {
    if (on && grp_) throw std::runtime_error(groupRefusesPauseLimit());
    if (on && !trim_silence_) throw std::runtime_error("the pause limit needs silence trimming (it shortens pauses inside trimmed utterances)");
    check(h_, stn_set_pause_limit(h_, on ? 1 : 0, max_pause_ms));
    pause_limit_ = on;
}


// one handle: the batch uploaded and run, ready for whichever fetch the caller wants
void TextToSpeech::runBatch(const TokenBatch& tb, const std::vector<float>& mask, const Style& style, int total_step, float speed) {
    check(h_, stn_batch_upload(h_, tb.B, tb.Lt, tb.ids.data(), mask.data(), style.getTtlData().data(),
                               style.getDpData().data(), nullptr, nullptr));
    uint64_t seed = noise_seed_;
    if (seed == 0) { std::random_device rd; seed = ((uint64_t)rd() << 32) | rd(); }  // unseeded, like cpp/helper.cpp:442-444
    else seed += calls_;
    ++calls_;
    check(h_, stn_batch_run(h_, total_step, speed, seed));
}

void TextToSpeech::setLoudnessScope(bool whole_text) {
    if (whole_text && grp_) throw std::runtime_error(groupRefusesScopeText());
    scope_text_ = whole_text;
}

TextToSpeech::SynthesisResult TextToSpeech::call(const std::string& text, const std::string& lang, const Style& style,
                                                 int total_step, float speed, float silence_duration) {
    if (style.getTtlShape()[0] != 1) throw std::runtime_error("Single speaker text to speech only supports single style");
    const std::vector<std::string> chunks = chunk_text(text, lang == "ko" ? 120 : 300);
    if (chunks.size() == 1 && !trim_silence_) return infer({chunks[0]}, {lang}, style, total_step, speed);  // (trimmed: the join cuts the one segment)
    // The reference synthesizes the chunks one after another (cpp/helper.cpp:697-719: one _infer, i.e. four Run calls per
    // step, per chunk).  Here they form ONE batch with the speaker's style replicated; the length-aware vocoder mode makes
    // every chunk's wave over its own frames what the batch-of-one run gives, so the joined result keeps the reference's
    // semantics (untrimmed chunk waves of L_i * chunk_size samples, zeros in between) at one pipeline pass.
    const int n = (int)chunks.size();
    const std::vector<int64_t>& ts = style.getTtlShape();
    const std::vector<int64_t>& ds = style.getDpShape();
    std::vector<float> ttl, dp;
    ttl.reserve(style.getTtlData().size() * n);
    dp.reserve(style.getDpData().size() * n);
    for (int i = 0; i < n; ++i) {
        ttl.insert(ttl.end(), style.getTtlData().begin(), style.getTtlData().end());
        dp.insert(dp.end(), style.getDpData().begin(), style.getDpData().end());
    }
    const Style rep(std::move(ttl), {n, ts[1], ts[2]}, std::move(dp), {n, ds[1], ds[2]});
    struct ModeGuard {  // (every rank's engine when the chunks are dealt over a group)
        std::vector<stn_handle*> hs;
        ModeGuard(stn_handle* h0, stn_group* grp) {
            if (grp) for (int r = 0; r < stn_group_size(grp); ++r) hs.push_back(stn_group_handle(grp, r));
            else hs.push_back(h0);
            for (stn_handle* h : hs) { check(h, stn_set_vocoder_mode(h, 1)); check(h, stn_set_shape_buckets(h, 1)); }  // chunk batches of any
                                                                                                                      // length share captured graphs
        }
        ~ModeGuard() { for (stn_handle* h : hs) { (void)stn_set_vocoder_mode(h, 0); (void)stn_set_shape_buckets(h, 0); } }
    } guard(h_, grp_);
    if (!grp_) {
        // one device: the join is the fetch's (stn_batch_fetch_joined): one programme of n members, the silence as the zero codeword
        // at the rate of the returned audio, every chunk's whole wave or (setTrimChunks) cut at its duration
        const TokenBatch tb = text_processor_(chunks, std::vector<std::string>((size_t)n, lang));
        runBatch(tb, tb.mask(), rep, total_step, speed);
        const int32_t members = n;
        const int64_t gap = (int64_t)(int)(silence_duration * (float)getSampleRate());
        stn_join j{1, &members, &gap, &silence_duration, trim_chunks_ ? STN_JOIN_TRIM : STN_JOIN_WHOLE, scope_text_ ? STN_JOIN_GAIN_PROG : STN_JOIN_GAIN_ROW};
        int64_t W_join = 0;
        check(h_, stn_batch_join_dims(h_, &j, &W_join, nullptr, nullptr));
        SynthesisResult out;
        out.encoding = enc_;
        out.duration.resize(1);
        if (encodedFetch()) {
            out.encoded.resize((size_t)W_join * stn_encoding_bytes(enc_));
            check(h_, stn_batch_fetch_joined(h_, &j, enc_, out.encoded.data(), out.encoded.size(), nullptr, out.duration.data()));
        } else {
            out.wav.resize((size_t)W_join);
            check(h_, stn_batch_fetch_joined(h_, &j, STN_ENC_F32, out.wav.data(), out.wav.size() * sizeof(float), nullptr, out.duration.data()));
        }
        if (trim_silence_) out.length = {W_join};  // (one programme: its length is the joined segments')
        join_members_ = members;
        join_silence_ = silence_duration;
        return out;
    }
    // a group deals the chunks over its devices: its long form keeps the host join of the gathered rows
    if (trim_chunks_) throw std::runtime_error(groupRefusesTrimChunks());
    const SynthesisResult r = infer(chunks, std::vector<std::string>((size_t)n, lang), rep, total_step, speed);
    const size_t eb = r.encoding == STN_ENC_PCM16 ? 0 : (size_t)stn_encoding_bytes(r.encoding);  // 0: the float waveform
    const size_t W = eb ? r.encoded.size() / eb / (size_t)n : r.wav.size() / (size_t)n;
    // silence in the encoding: its zero codeword (mu-law 0xFF, A-law 0xD5, zero bytes otherwise)
    const unsigned char zero = r.encoding == STN_ENC_MULAW ? 0xFF : r.encoding == STN_ENC_ALAW ? 0xD5 : 0;
    const int chunk_size = cfgs_.ae.base_chunk_size * cfgs_.ttl.chunk_compress_factor;
    const size_t n_sil = (size_t)(int)(silence_duration * (float)getSampleRate());  // (zeros at the rate of the returned audio)
    const int64_t rg = std::gcd(getSampleRate(), cfgs_.ae.sample_rate), rP = getSampleRate() / rg, rQ = cfgs_.ae.sample_rate / rg;
    SynthesisResult out;
    out.encoding = r.encoding;
    float dur_cat = 0.f;
    for (int i = 0; i < n; ++i) {
        const LatentGeometry g = latent_geometry({r.duration[(size_t)i]}, cfgs_.ae.sample_rate, cfgs_.ae.base_chunk_size,
                                                 cfgs_.ttl.chunk_compress_factor, cfgs_.ttl.latent_dim);
        const size_t n_i = (size_t)(((int64_t)g.L * chunk_size * rP + rQ - 1) / rQ);  // the wav length the chunk's own run would return
        if (i > 0) {  // untrimmed chunk waves joined by zeros (cpp/helper.cpp:706-715)
            if (eb) out.encoded.insert(out.encoded.end(), n_sil * eb, zero);
            else out.wav.insert(out.wav.end(), n_sil, 0.0f);
            dur_cat += r.duration[(size_t)i] + silence_duration;
        } else {
            dur_cat = r.duration[0];
        }
        if (eb) out.encoded.insert(out.encoded.end(), r.encoded.begin() + (size_t)i * W * eb, r.encoded.begin() + ((size_t)i * W + std::min(n_i, W)) * eb);
        else out.wav.insert(out.wav.end(), r.wav.begin() + (size_t)i * W, r.wav.begin() + (size_t)i * W + std::min(n_i, W));
    }
    out.duration = {dur_cat};
    return out;
}

TextToSpeech::LoudnessReport TextToSpeech::loudnessReport() {
    if (grp_) throw std::runtime_error("the loudness report needs the batch on one device: a group has none (use one GPU)");
    LoudnessReport r;
    auto size = [&](size_t n) {
        for (std::vector<float>* v : {&r.integrated, &r.peak, &r.gain, &r.max_momentary, &r.max_short_term, &r.range}) v->resize(n);
        r.n_short_term.resize(n);
    };
    if (join_members_ > 0) {  // the joined text as call() joined it
        const int64_t gap = (int64_t)(int)(join_silence_ * (float)getSampleRate());
        stn_join j{1, &join_members_, &gap, &join_silence_, trim_chunks_ ? STN_JOIN_TRIM : STN_JOIN_WHOLE, STN_JOIN_GAIN_PROG};
        size(1);
        check(h_, stn_batch_join_loudness(h_, &j, r.integrated.data(), r.peak.data(), r.gain.data()));
        check(h_, stn_batch_join_loudness_range(h_, &j, r.max_momentary.data(), r.max_short_term.data(), r.range.data(), r.n_short_term.data()));
        return r;
    }
    int B = 0, L = 0;
    int64_t W = 0;
    check(h_, stn_batch_dims(h_, &B, &L, &W));
    size((size_t)B);
    check(h_, stn_batch_loudness(h_, r.integrated.data(), r.peak.data(), r.gain.data()));
    check(h_, stn_batch_loudness_range(h_, r.max_momentary.data(), r.max_short_term.data(), r.range.data(), r.n_short_term.data()));
    return r;
}

TextToSpeech::PitchReport TextToSpeech::pitchReport() {
    if (grp_) throw std::runtime_error("the pitch report needs the batch on one device: a group has none (use one GPU)");
    int B = 0, L = 0;
    int64_t W = 0, cap = 0;
    check(h_, stn_batch_dims(h_, &B, &L, &W));
    check(h_, stn_batch_f0_frames(h_, nullptr, &cap));
    PitchReport r;
    r.stats.resize((size_t)B);
    std::vector<float> f0((size_t)B * (size_t)cap);
    check(h_, stn_batch_f0(h_, nullptr, cap, f0.data(), nullptr, r.stats.data()));
    if (join_members_ > 0) {  // the joined text as call() joined it: one set of statistics over the chunks' frames
        std::vector<float> pooled;
        for (int b = 0; b < B; ++b) pooled.insert(pooled.end(), f0.begin() + (size_t)b * cap, f0.begin() + (size_t)b * cap + r.stats[(size_t)b].frames);
        r.stats.assign(1, stn_f0_stats{});
        if (stn_f0_stats_rule(pooled.data(), (int64_t)pooled.size(), &r.stats[0]) != STN_OK) throw std::runtime_error("pitch report: a joined text too long to pool");
    }
    return r;
}

void TextToSpeech::setEncoding(int enc) {
    if (stn_encoding_bytes(enc) == 0) throw std::runtime_error("unknown sample encoding " + std::to_string(enc));
    if (grp_ && stn_group_set_encoding(grp_, enc) != STN_OK) throw std::runtime_error(std::string("encoding: ") + stn_group_last_error(grp_));
    enc_ = enc;
}

TextToSpeech::SynthesisResult TextToSpeech::batch(const std::vector<std::string>& text_list,
                                                  const std::vector<std::string>& lang_list, const Style& style,
                                                  int total_step, float speed) {
    return infer(text_list, lang_list, style, total_step, speed);
}

std::string parseFilterSpec(const std::string& spec, stn_filter& f) {
    static const char* const names[] = {"highpass", "lowpass", "notch", "peak", "lowshelf", "highshelf"};
    std::vector<std::string> parts;
    size_t a = 0, p;
    while ((p = spec.find(':', a)) != std::string::npos) { parts.push_back(spec.substr(a, p - a)); a = p + 1; }
    parts.push_back(spec.substr(a));
    const std::string who = "filter '" + spec + "': ";
    if (parts.size() < 2 || parts.size() > 4) return who + "expected TYPE:FREQ[:Q[:GAIN_DB]]";
    f = stn_filter{-1, 0.0f, 0.7071f, 0.0f};
    for (int t = 0; t < 6; ++t) if (parts[0] == names[t]) f.type = t;
    if (f.type < 0) return who + "type must be one of highpass, lowpass, notch, peak, lowshelf, highshelf";
    float* dst[3] = {&f.freq_hz, &f.q, &f.gain_db};
    for (size_t i = 1; i < parts.size(); ++i) {
        char* end = nullptr;
        *dst[i - 1] = std::strtof(parts[i].c_str(), &end);
        if (parts[i].empty() || *end) return who + "FREQ, Q and GAIN_DB must be numbers";
    }
    return "";
}

std::string filterPreset(const std::string& name, std::vector<stn_filter>& out) {
    if (name == "rumble") {
        out.push_back({STN_FILT_HIGHPASS, 80.0f, 0.7071f, 0.0f});
    } else if (name == "telephone") {
        for (int type : {STN_FILT_HIGHPASS, STN_FILT_LOWPASS})
            for (float q : {0.541f, 1.307f}) out.push_back({type, type == STN_FILT_HIGHPASS ? 300.0f : 3400.0f, q, 0.0f});
    } else {
        return "filter-preset '" + name + "': rumble or telephone";
    }
    return "";
}

std::string compressorPreset(const std::string& name, stn_compressor& c) {
    if (name != "speech") return "compressor-preset '" + name + "': speech";
    c = stn_compressor{-24.0f, 3.0f, 6.0f, 5.0f, 120.0f, 0.0f};
    return "";
}

std::string parseCompressorSpec(const std::string& spec, stn_compressor& c) {
    std::vector<std::string> parts;
    size_t a = 0, p;
    while ((p = spec.find(':', a)) != std::string::npos) { parts.push_back(spec.substr(a, p - a)); a = p + 1; }
    parts.push_back(spec.substr(a));
    const std::string who = "compressor '" + spec + "': ";
    if (parts.size() < 2 || parts.size() > 6) return who + "expected THRESHOLD:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:MAKEUP_DB]]]]";
    (void)compressorPreset("speech", c);  // what the fields left out take
    float* dst[6] = {&c.threshold_db, &c.ratio, &c.knee_db, &c.attack_ms, &c.release_ms, &c.makeup_db};
    for (size_t i = 0; i < parts.size(); ++i) {
        char* end = nullptr;
        *dst[i] = std::strtof(parts[i].c_str(), &end);
        if (parts[i].empty() || *end) return who + "THRESHOLD, RATIO, KNEE, ATTACK_MS, RELEASE_MS and MAKEUP_DB must be numbers";
    }
    return "";
}

std::string expanderPreset(const std::string& name, stn_expander& c) {
    if (name == "speech") c = stn_expander{-50.0f, 3.0f, 6.0f, 24.0f, 1.0f, 30.0f, 150.0f};
    else if (name == "gate") c = stn_expander{-45.0f, 20.0f, 0.0f, 60.0f, 0.5f, 50.0f, 100.0f};
    else return "expander-preset '" + name + "': speech or gate";
    return "";
}

std::string parseExpanderSpec(const std::string& spec, stn_expander& c, const std::string& preset) {
    std::vector<std::string> parts;
    size_t a = 0, p;
    while ((p = spec.find(':', a)) != std::string::npos) { parts.push_back(spec.substr(a, p - a)); a = p + 1; }
    parts.push_back(spec.substr(a));
    const std::string who = "expander '" + spec + "': ";
    if (parts.size() < 2 || parts.size() > 7) return who + "expected THRESHOLD:RATIO[:KNEE[:RANGE_DB[:ATTACK_MS[:HOLD_MS[:RELEASE_MS]]]]]";
    const std::string bad = expanderPreset(preset, c);  // what the fields left out take
    if (!bad.empty()) return bad;
    float* dst[7] = {&c.threshold_db, &c.ratio, &c.knee_db, &c.range_db, &c.attack_ms, &c.hold_ms, &c.release_ms};
    for (size_t i = 0; i < parts.size(); ++i) {
        char* end = nullptr;
        *dst[i] = std::strtof(parts[i].c_str(), &end);
        if (parts[i].empty() || *end) return who + "THRESHOLD, RATIO, KNEE, RANGE_DB, ATTACK_MS, HOLD_MS and RELEASE_MS must be numbers";
    }
    return "";
}

std::string deesserPreset(const std::string& name, stn_deesser& c) {
    if (name != "speech") return "deesser-preset '" + name + "': speech";
    c = stn_deesser{5500.0f, -30.0f, 4.0f, 6.0f, 1.0f, 40.0f, 12.0f, STN_DEESS_SPLIT};
    return "";
}

std::string parseDeesserSpec(const std::string& spec, stn_deesser& c) {
    std::vector<std::string> parts;
    size_t a = 0, p;
    while ((p = spec.find(':', a)) != std::string::npos) { parts.push_back(spec.substr(a, p - a)); a = p + 1; }
    parts.push_back(spec.substr(a));
    const std::string who = "deesser '" + spec + "': ";
    if (parts.size() < 2 || parts.size() > 8) return who + "expected FREQ:THRESHOLD[:RATIO[:KNEE[:ATTACK_MS[:RELEASE_MS[:RANGE_DB[:MODE]]]]]]";
    (void)deesserPreset("speech", c);  // what the fields left out take
    float* dst[7] = {&c.freq_hz, &c.threshold_db, &c.ratio, &c.knee_db, &c.attack_ms, &c.release_ms, &c.range_db};
    for (size_t i = 0; i < parts.size() && i < 7; ++i) {
        char* end = nullptr;
        *dst[i] = std::strtof(parts[i].c_str(), &end);
        if (parts[i].empty() || *end) return who + "FREQ, THRESHOLD, RATIO, KNEE, ATTACK_MS, RELEASE_MS and RANGE_DB must be numbers";
    }
    if (parts.size() == 8) {
        if (parts[7] != "split" && parts[7] != "wide") return who + "MODE must be one of split, wide";
        c.mode = parts[7] == "wide" ? STN_DEESS_WIDE : STN_DEESS_SPLIT;
    }
    return "";
}

std::string parseDitherMode(const std::string& name, int& mode) {
    static const char* const names[] = {"off", "round", "tpdf", "tpdf-hp"};  // (STN_DITHER_* in order)
    for (int m = 0; m < 4; ++m)
        if (name == names[m]) { mode = m; return ""; }
    return "dither '" + name + "': one of off, round, tpdf, tpdf-hp";
}

std::unique_ptr<TextToSpeech> loadTextToSpeech(const std::string& onnx_dir, bool use_gpu, const EngineOptions& opts) {
    if (!use_gpu) throw std::runtime_error("CPU mode is not supported: this engine runs on MI355X only");
    const char* dt_name = opts.dtype == STN_DTYPE_BF16 ? "bf16" : opts.dtype == STN_DTYPE_F16 ? "fp16" : "fp32";
    stn_handle* h = nullptr;
    stn_group* grp = nullptr;
    if (opts.gpus > 1 || !opts.devices.empty()) {
        // refused before anything is created: a group deals the chunks of a text over its devices and keeps the host join
        if (opts.loudness_scope_text) throw std::runtime_error(groupRefusesScopeText());
        if (opts.trim_chunks) throw std::runtime_error(groupRefusesTrimChunks());
        if (!std::isnan(opts.trim_silence_db)) throw std::runtime_error(groupRefusesSilenceTrim());
        if (!std::isnan(opts.max_pause_ms)) throw std::runtime_error(groupRefusesPauseLimit());
        std::vector<int> dev = opts.devices;
        if (dev.empty()) for (int i = 0; i < opts.gpus; ++i) dev.push_back(opts.device + i);
        if (stn_group_create((int)dev.size(), dev.data(), opts.dtype, &grp) != STN_OK) throw std::runtime_error(std::string("engine group: ") + stn_group_last_error(nullptr));
        h = stn_group_handle(grp, 0);
        std::cout << "Using " << dev.size() << " x MI355X (" << dt_name << ", utterances dealt by length, PCM gathered into device " << dev[0]
                  << (stn_group_uses_rccl(grp) ? " over RCCL" : " by device copies: ranks share a GPU") << ") for inference" << std::endl;
    } else {
        stn_config cfg{opts.device, opts.dtype};
        if (stn_create(&cfg, &h) != STN_OK) throw std::runtime_error(std::string("engine: ") + stn_last_error(nullptr));
        std::cout << "Using MI355X (HIP device " << opts.device << ", " << dt_name << ") for inference" << std::endl;
    }
    auto load_dir = [&]() { return grp ? stn_group_load_dir(grp, onnx_dir.c_str()) : stn_load_dir(h, onnx_dir.c_str()); };
    auto load_err = [&]() { return std::string(grp ? stn_group_last_error(grp) : stn_last_error(h)); };
    try {
        const int rc = load_dir();
        bool synthetic = false;
        Config cfgs;
        UnicodeProcessor tp;
        if (rc == STN_OK) {
            cfgs = loadCfgs(onnx_dir);
            tp = UnicodeProcessor::from_file(onnx_dir + "/unicode_indexer.json");
        } else if (opts.allow_synthetic) {
            std::cout << "  model assets unavailable (" << load_err() << ")\n"
                      << "  -> synthetic weights from the default architecture descriptor (seed " << opts.weight_seed << ")" << std::endl;
            stn_arch a;
            stn_arch_default(&a);
            if (grp) { if (stn_group_load_synthetic(grp, &a, opts.weight_seed) != STN_OK) throw std::runtime_error(load_err()); }
            else check(h, stn_load_synthetic(h, &a, opts.weight_seed));
            cfgs.ae.sample_rate = a.sample_rate; cfgs.ae.base_chunk_size = a.base_chunk_size;
            cfgs.ttl.chunk_compress_factor = a.chunk_compress_factor; cfgs.ttl.latent_dim = a.latent_dim;
            std::vector<int64_t> idx(65536);  // synthetic indexer of the same shape as unicode_indexer.json
            for (int cp = 0; cp < 65536; ++cp) idx[cp] = cp < 384 ? cp : 384 + (cp % 128);
            tp = UnicodeProcessor(std::move(idx));
            synthetic = true;
        } else {
            throw std::runtime_error(load_err());
        }
        // rc: what the group's setter (every rank) or the single handle's returned
        auto applied = [&](const char* what, int rc) {
            if (grp) { if (rc != STN_OK) throw std::runtime_error(std::string(what) + ": " + stn_group_last_error(grp)); }
            else check(h, rc);
        };
        const int nf = (int)opts.filters.size();
        if (opts.pitch != 0.0f) applied("pitch", grp ? stn_group_set_pitch(grp, opts.pitch) : stn_set_pitch(h, opts.pitch));
        if (opts.pitch_mode != STN_PITCH_RESAMPLE) applied("pitch mode", grp ? stn_group_set_pitch_mode(grp, opts.pitch_mode) : stn_set_pitch_mode(h, opts.pitch_mode));
        if (opts.output_rate) applied("output rate", grp ? stn_group_set_output_rate(grp, opts.output_rate) : stn_set_output_rate(h, opts.output_rate));
        // (after the rate: a chain is checked against the output rate in force)
        if (nf) applied("filters", grp ? stn_group_set_filters(grp, nf, opts.filters.data()) : stn_set_filters(h, nf, opts.filters.data()));
        if (opts.expander_on) applied("expander", grp ? stn_group_set_expander(grp, 1, &opts.expander) : stn_set_expander(h, 1, &opts.expander));
        // (after the rate as well: freq_hz is checked against the output rate in force)
        if (opts.deesser_on) applied("deesser", grp ? stn_group_set_deesser(grp, 1, &opts.deesser) : stn_set_deesser(h, 1, &opts.deesser));
        if (opts.compressor_on) applied("compressor", grp ? stn_group_set_compressor(grp, 1, &opts.compressor) : stn_set_compressor(h, 1, &opts.compressor));
        if (!std::isnan(opts.loudness_lufs))
            applied("loudness", grp ? stn_group_set_loudness(grp, 1, opts.loudness_lufs, opts.loudness_ceiling_dbfs)
                                    : stn_set_loudness(h, 1, opts.loudness_lufs, opts.loudness_ceiling_dbfs));
        if (!std::isnan(opts.limiter_ms)) {
            if (std::isnan(opts.loudness_lufs)) throw std::runtime_error("the limiter needs loudness normalization (it holds the ceiling of the loudness gain)");
            applied("limiter", grp ? stn_group_set_limiter(grp, 1, opts.limiter_ms) : stn_set_limiter(h, 1, opts.limiter_ms));
        }
        if (opts.true_peak) {
            if (std::isnan(opts.loudness_lufs)) throw std::runtime_error("the true-peak mode needs loudness normalization (it is the ceiling of the loudness gain)");
            applied("peak mode", grp ? stn_group_set_peak_mode(grp, STN_PEAK_TRUE) : stn_set_peak_mode(h, STN_PEAK_TRUE));
        }
        if (opts.dither != STN_DITHER_OFF)
            applied("dither", grp ? stn_group_set_dither(grp, opts.dither, opts.dither_seed) : stn_set_dither(h, opts.dither, opts.dither_seed));
        // (refused here, while this function still owns the handle: once tts owns it, a throw would destroy it twice)
        if (!std::isnan(opts.trim_silence_db)) check(h, stn_set_silence_trim(h, 1, opts.trim_silence_db, opts.trim_keep_ms, opts.trim_fade_ms));
        if (!std::isnan(opts.max_pause_ms)) {
            if (std::isnan(opts.trim_silence_db)) throw std::runtime_error("the pause limit needs silence trimming (it shortens pauses inside trimmed utterances)");
            check(h, stn_set_pause_limit(h, 1, opts.max_pause_ms));
        }
        auto tts = grp ? std::make_unique<TextToSpeech>(grp, std::move(tp), cfgs, opts.noise_seed)
                       : std::make_unique<TextToSpeech>(h, std::move(tp), cfgs, opts.noise_seed);
        tts->setOutputRate(opts.output_rate);
        tts->setEncoding(opts.encoding);
        tts->setDither(opts.dither);
        tts->setLoudnessScope(opts.loudness_scope_text);
        tts->setTrimChunks(opts.trim_chunks);
        if (!std::isnan(opts.trim_silence_db)) tts->setSilenceTrim(true, opts.trim_silence_db, opts.trim_keep_ms, opts.trim_fade_ms);  // (accepted above)
        if (!std::isnan(opts.max_pause_ms)) tts->setPauseLimit(true, opts.max_pause_ms);
        if (synthetic) tts->markSynthetic();
        return tts;
    } catch (...) {
        if (grp) stn_group_destroy(grp); else stn_destroy(h);
        throw;
    }
}

}  // namespace host
}  // namespace stn
