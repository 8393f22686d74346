"""Python host with the names of the reference's `py/helper.py` (Style, TextToSpeech, load_text_to_speech,
load_voice_style) on top of the C ABI — what `py/service.py` and `py/example_onnx.py` import.

Differences from the reference are confined to where the work happens: the four `InferenceSession.run` sites
(/root/reference/py/helper.py:190-214) are one resident-batch call into the MI355X engine, the text frontend is the C++ one
(the C++ host is the contract where the reference's hosts disagree), and the chunks of a long text go
through the engine as ONE batch (length-aware vocoder) instead of one `_infer` per chunk (py/helper.py:231-243)."""
import json
import math
import os
import secrets
import threading

import numpy as np

from . import binding, host
from .arch import default_arch


class Style:
    """py/helper.py:134-137"""

    def __init__(self, style_ttl: np.ndarray, style_dp: np.ndarray):
        self.ttl = np.ascontiguousarray(style_ttl, np.float32)
        self.dp = np.ascontiguousarray(style_dp, np.float32)


def load_voice_style(voice_style_paths, verbose=False, synthetic_arch=None):
    """py/helper.py:339-368.  With `synthetic_arch` (an engine running on synthetic weights, no assets on disk) a missing
    file yields a deterministic style keyed by the file's base name instead of an error."""
    ttl, dp = [], []
    for path in voice_style_paths:
        if not os.path.exists(path) and synthetic_arch is not None:
            a = synthetic_arch
            name = os.path.splitext(os.path.basename(path))[0]
            rng = np.random.default_rng(int.from_bytes(name.encode()[:8].ljust(8, b"\0"), "little"))
            ttl.append((rng.standard_normal((a.n_style_ttl, a.d_style_ttl)) * 0.1).astype(np.float32))
            dp.append((rng.standard_normal((a.n_style_dp, a.d_style_dp)) * 0.1).astype(np.float32))
            continue
        with open(path, "r") as f:
            vs = json.load(f)
        td, dd = vs["style_ttl"]["dims"], vs["style_dp"]["dims"]
        ttl.append(np.asarray(vs["style_ttl"]["data"], np.float32).reshape(td[1], td[2]))
        dp.append(np.asarray(vs["style_dp"]["data"], np.float32).reshape(dd[1], dd[2]))
    if len({t.shape for t in ttl}) != 1 or len({d.shape for d in dp}) != 1:
        raise ValueError("voice styles of one batch must share their dimensions")
    if verbose:
        print(f"Loaded {len(ttl)} voice styles")
    return Style(np.stack(ttl), np.stack(dp))


class TextToSpeech:
    """py/helper.py:140-258: `tts(text, lang, style, total_step, speed, silence_duration)` and `tts.batch(...)`, both
    returning (wav [B, W] float32, duration [B] float32).  One instance = one engine handle = one GPU; calls are
    serialised by a lock (the handle is single-threaded by contract)."""

    def __init__(self, engine, text_processor, cfgs, noise_seed=None, output_rate=None, loudness=None, trim_silence=None, limiter=None, peak_mode=None, max_pause=None,
                 filters=None):
        self.engine = engine
        self.text_processor = text_processor
        self.cfgs = cfgs
        self.sample_rate = cfgs["ae"]["sample_rate"]  # the model's rate: it sizes the latent (latent_geometry)
        # rate of the returned audio (resampled on the GPU at fetch time, Engine.set_output_rate); None: the model's
        self.output_rate = int(output_rate) if output_rate else self.sample_rate
        if self.output_rate != self.sample_rate:
            engine.set_output_rate(self.output_rate)
        # a chain of up to 8 biquads every returned row goes through on the GPU at fetch time, after the resampler and before everything
        # below (Engine.set_filters): None = off, or a list as binding.filter_args takes it
        self.filters = _filter_setting(filters)
        if self.filters:
            engine.set_filters(self.filters)
        # loudness normalization of the returned audio (measured and scaled on the GPU at fetch time, Engine.set_loudness): None = off,
        # a target in LUFS (peak ceiling -1 dBFS), or (target LUFS, ceiling dBFS)
        self.loudness = _loudness_setting(loudness)
        if self.loudness is not None:
            engine.set_loudness(*self.loudness)
        # leading and trailing silence of the returned audio trimmed by level (on the GPU at fetch time, Engine.set_silence_trim): None =
        # off, top_db (20 ms kept, 5 ms fade), or (top_db, keep_ms, fade_ms)
        self.trim_silence = _trim_setting(trim_silence)
        if self.trim_silence is not None:
            engine.set_silence_trim(self.trim_silence)
        # pauses inside an utterance longer than this many milliseconds shortened to it (Engine.set_pause_limit): None = off; it acts only
        # while silence trimming is on
        self.max_pause = _pause_setting(max_pause)
        if self.max_pause is not None:
            engine.set_pause_limit(self.max_pause)
        # look-ahead peak limiter behind the loudness gain (Engine.set_limiter): None = off, True = 5 ms, or the look-ahead in ms; it
        # acts only while loudness normalization is on
        self.limiter = _limiter_setting(limiter)
        if self.limiter is not None:
            engine.set_limiter(self.limiter)
        # the ceiling of the loudness gain as a sample-peak ("sample", the default) or a true-peak ceiling ("true": 4x oversampled,
        # Engine.set_peak_mode); it acts only while loudness normalization is on
        self.peak_mode = "sample" if peak_mode is None else peak_mode
        binding.peak_mode_id(self.peak_mode)
        if self.peak_mode != "sample":
            engine.set_peak_mode(self.peak_mode)
        self.base_chunk_size = cfgs["ae"]["base_chunk_size"]
        self.chunk_compress_factor = cfgs["ttl"]["chunk_compress_factor"]
        self.ldim = cfgs["ttl"]["latent_dim"]
        self.noise_seed = noise_seed  # None: fresh noise per call, like np.random.randn in the reference
        self._lock = threading.Lock()
        self._calls = 0

    def _seed(self):
        if self.noise_seed is None:
            return secrets.randbits(63) | 1
        self._calls += 1
        return self.noise_seed + self._calls - 1

    def _infer(self, text_list, lang_list, style, total_step, speed=1.05, length_aware=False, output_rate=None, loudness=None,
               encoding=None, join=None, trim_silence=None, lengths=False, limiter=None, peak_mode=None, max_pause=None, filters=None):
        """lengths: returns (wav, duration, len) with len [B] the samples each row holds from column 0: its trimmed segment with
        trimming on (Engine.batch_silence_edges, never a duration product; with the pause limit Engine.batch_pauses' len_b), else None."""
        if len(text_list) != style.ttl.shape[0]:
            raise ValueError("Number of texts must match number of style vectors")
        trim = self.trim_silence if trim_silence is None else _trim_setting(trim_silence)  # (validated before anything is set)
        lim = None if limiter is None else _limiter_setting(limiter)
        pause = self.max_pause if max_pause is None else _pause_setting(max_pause)
        binding.peak_mode_id(peak_mode)
        chain = None if filters is None else _filter_setting(filters)
        ids, mask = self.text_processor(text_list, lang_list)
        with self._lock:
            # length-aware batches (the chunks of a long text, the service's merged requests) come in ever-changing lengths: shape
            # buckets let them share captured graphs (stn_set_shape_buckets: every row stays exact over its own samples, rows are
            # just longer); a plain batch keeps the reference's exact [B, L * chunk] result
            self.engine.set_vocoder_mode(length_aware)
            self.engine.set_shape_buckets(length_aware)
            if filters is not None:  # this call's chain (fetch-time as well); off while the rate changes: a chain is checked against the rate in force
                self.engine.set_filters(None)
            if output_rate is not None:  # this call's rate (a fetch-time setting: no captured graph depends on it)
                self.engine.set_output_rate(output_rate)
            if loudness is not None:  # this call's normalization (fetch-time as well)
                self.engine.set_loudness(*(_loudness_setting(loudness) or (None,)))
            if trim_silence is not None:  # this call's trimming (fetch-time as well)
                self.engine.set_silence_trim(trim)
            if max_pause is not None:  # this call's pause limit (fetch-time as well)
                self.engine.set_pause_limit(pause)
            if limiter is not None:  # this call's limiter (fetch-time as well)
                self.engine.set_limiter(lim)
            if peak_mode is not None:  # this call's peak mode (fetch-time as well)
                self.engine.set_peak_mode(peak_mode)
            try:
                if chain:
                    self.engine.set_filters(chain)
                if join is not None:  # joined on the GPU by the fetch (Engine.batch_fetch_joined's arguments)
                    self.engine.batch_upload(ids, mask, style.ttl, style.dp)
                    self.engine.batch_run(total_step, speed, self._seed())
                    return self.engine.batch_fetch_joined(encoding=encoding, **join)
                if encoding is None:
                    out = self.engine.synthesize(ids, mask, style.ttl, style.dp, total_step, speed, noise_seed=self._seed())
                else:  # encoded on the GPU by the fetch (binding.encoded_empty's dtypes)
                    self.engine.batch_upload(ids, mask, style.ttl, style.dp)
                    self.engine.batch_run(total_step, speed, self._seed())
                    out = self.engine.batch_fetch_encoded(encoding)
                if not lengths:
                    return out
                if trim is None:
                    return out[0], out[1], None
                if pause is not None:
                    return out[0], out[1], self.engine.batch_pauses()[0]
                start, end = self.engine.batch_silence_edges()
                return out[0], out[1], end - start
            finally:
                self.engine.set_vocoder_mode(False)
                self.engine.set_shape_buckets(False)
                if filters is not None:
                    self.engine.set_filters(None)
                if output_rate is not None:
                    self.engine.set_output_rate(self.output_rate)
                if filters is not None:
                    self.engine.set_filters(self.filters)
                if loudness is not None:
                    self.engine.set_loudness(*(self.loudness or (None,)))
                if trim_silence is not None:
                    self.engine.set_silence_trim(self.trim_silence)
                if max_pause is not None:
                    self.engine.set_pause_limit(self.max_pause)
                if limiter is not None:
                    self.engine.set_limiter(self.limiter)
                if peak_mode is not None:
                    self.engine.set_peak_mode(self.peak_mode)

    def latent_lengths(self, durations):
        """Latent frames each utterance occupies (get_latent_mask, py/helper.py:276-282) from its returned duration."""
        _, _, lens = host.latent_geometry(np.asarray(durations, np.float32), self.sample_rate, self.base_chunk_size,
                                          self.chunk_compress_factor, self.ldim)
        return np.asarray(lens)

    def out_samples(self, n, output_rate=None):
        """Samples at the output rate that n model-rate samples resample to: ceil(n * P / Q)."""
        out = int(output_rate or self.output_rate)
        g = math.gcd(out, self.sample_rate)
        P, Q = out // g, self.sample_rate // g
        return -(-int(n) * P // Q)

    def solo_batch(self, text_list, lang_list, style, total_step, speed=1.05, output_rate=None, loudness=None, encoding=None,
                   trim_silence=None, limiter=None, peak_mode=None, max_pause=None, filters=None):
        """Independent utterances as one batch whose rows equal what each would give alone (length-aware vocoder):
        returns a list of per-utterance waves of L_i * chunk_size samples (at the output rate: the resampled length of those)
        and the durations.  The building block of the long-form path and of the service's dynamic batching.
        output_rate / loudness: this call's setting instead of the instance's (loudness: False = off for this call, a target in
        LUFS, or (target, ceiling dBFS)); with normalization, each utterance is normalized on its own.  encoding (a name or
        binding.ENC_*; None: float32): the waves in that sample encoding, encoded on the GPU (binding.encoded_empty's dtypes).
        trim_silence (this call's: False = off, top_db, or (top_db, keep_ms, fade_ms)): every wave is its trimmed segment, cut at the
        length the GPU found.  limiter (this call's: False = off, True = 5 ms, or the look-ahead in ms): with normalization, every
        utterance gets the full loudness gain and a look-ahead peak limiter holds the ceiling.  max_pause (this call's: False = off, or
        milliseconds in [20, 5000]; with trimming only): every pause inside an utterance longer than that is shortened to it, and the
        wave is cut at what remains.  filters (this call's: False or [] = off, or a list as binding.filter_args takes it): every
        utterance goes through that biquad chain before all of the above."""
        wav, dur, seg = self._infer(text_list, lang_list, style, total_step, speed, length_aware=True, output_rate=output_rate,
                                    loudness=loudness, encoding=encoding, trim_silence=trim_silence, lengths=True, limiter=limiter, peak_mode=peak_mode,
                                    max_pause=max_pause, filters=filters)
        if seg is not None:
            return [wav[i, : int(n)] for i, n in enumerate(seg)], dur
        cs = self.base_chunk_size * self.chunk_compress_factor
        lens = [int(self.latent_lengths(dur[i:i + 1])[0]) for i in range(len(text_list))]
        return [wav[i, : min(self.out_samples(n * cs, output_rate), wav.shape[1])] for i, n in enumerate(lens)], dur

    def joined_batch(self, text_list, lang_list, style, total_step, speed=1.05, rows=None, silence_duration=0.3, output_rate=None,
                     loudness=None, encoding=None, loudness_scope="chunk", trim_chunks=False, trim_silence=None, limiter=None, peak_mode=None,
                     max_pause=None, filters=None):
        """solo_batch whose rows are joined on the GPU into len(rows) waves: rows[g] consecutive utterances each (None: all of them
        in one), silence_duration (one value, or one per wave) seconds of silence between two of them — the encoding's zero codeword.
        Returns (list of joined waves, their durations: the reference's fp32 sum d = dur_0; d += dur_i + silence).  loudness_scope,
        with normalization on: "chunk", every utterance with its own gain (what joining solo_batch's rows gives, byte for byte);
        "text", every joined wave measured as one BS.1770 programme, silences included, and scaled by one gain.  trim_chunks: every
        utterance cut at its duration before the join (the reference's Rust host) instead of its whole wave (C++ / Python hosts).
        trim_silence (as solo_batch): every utterance is its trimmed segment, so the pause between two of them is the silence asked for
        plus twice the kept margin; the durations are then those of the segments.  max_pause (as solo_batch): the pauses inside an
        utterance are bounded as well.  filters: as solo_batch; every utterance is filtered on its own, then joined."""
        if loudness_scope not in ("chunk", "text"):
            raise ValueError(f"loudness_scope {loudness_scope!r}: 'chunk' or 'text'")
        rows = [len(text_list)] if rows is None else [int(r) for r in rows]
        rate = int(output_rate or self.output_rate)
        sil = np.broadcast_to(np.asarray(silence_duration, np.float64), (len(rows),))
        join = {"rows": rows, "gap_samples": [int(s * rate) for s in sil], "gap_seconds": sil.astype(np.float32),
                "mode": "trim" if trim_chunks else "whole", "gain_scope": "programme" if loudness_scope == "text" else "row"}
        waves, dur = self._infer(text_list, lang_list, style, total_step, speed, length_aware=True, output_rate=output_rate,
                                 loudness=loudness, encoding=encoding, join=join, trim_silence=trim_silence, limiter=limiter, peak_mode=peak_mode,
                                 max_pause=max_pause, filters=filters)
        return waves, dur

    def __call__(self, text, lang, style, total_step, speed=1.05, silence_duration=0.3, encoding=None, loudness_scope="chunk",
                 trim_chunks=False, trim_silence=None, limiter=None, peak_mode=None, max_pause=None, filters=None):
        """Long-form synthesis: the text is chunked, the chunks run as one length-aware batch and are joined with silence on the GPU
        (one joined fetch: py/helper.py:235-243's untrimmed chunk waves with zeros between).  With loudness normalization on,
        loudness_scope="chunk" normalizes each chunk as its own row (its own gain); "text" normalizes the joined text as one
        BS.1770 programme with one gain, its internal dynamics kept.  trim_chunks: as joined_batch.  encoding: as solo_batch; the
        silence is then the encoding's zero codeword.  trim_silence: as joined_batch; the returned wave then ends with the speech.
        limiter: as solo_batch; with loudness_scope="text" the joined text is limited as one programme.  max_pause, filters: as joined_batch."""
        if style.ttl.shape[0] != 1:
            raise ValueError("Single speaker text to speech only supports single style")
        if loudness_scope not in ("chunk", "text"):
            raise ValueError(f"loudness_scope {loudness_scope!r}: 'chunk' or 'text'")
        chunks = host.chunk_text(text, 120 if lang == "ko" else 300)
        trimming = (self.trim_silence if trim_silence is None else _trim_setting(trim_silence)) is not None
        if len(chunks) == 1 and not trim_chunks and not trimming:  # (one chunk is its own programme: the row's gain is the text's)
            return self._infer(chunks, [lang], style, total_step, speed, encoding=encoding, trim_silence=trim_silence, limiter=limiter, peak_mode=peak_mode,
                               max_pause=max_pause, filters=filters)
        n = len(chunks)
        rep = Style(np.repeat(style.ttl, n, axis=0), np.repeat(style.dp, n, axis=0))
        waves, dur = self.joined_batch(chunks, [lang] * n, rep, total_step, speed, silence_duration=silence_duration, encoding=encoding,
                                       loudness_scope=loudness_scope, trim_chunks=trim_chunks, trim_silence=trim_silence, limiter=limiter, peak_mode=peak_mode,
                                       max_pause=max_pause, filters=filters)
        return waves[0][None, :], np.array([dur[0]], np.float32)

    def batch(self, text_list, lang_list, style, total_step, speed=1.05, output_rate=None, loudness=None, encoding=None, trim_silence=None,
              lengths=False, limiter=None, peak_mode=None, max_pause=None, filters=None):
        """One padded batch -> (wav [B, W] float32, duration [B]); with an encoding (a name or binding.ENC_*), the rows in that sample
        encoding instead, encoded on the GPU (binding.encoded_empty's dtypes).  trim_silence (as solo_batch): row b holds its trimmed
        segment from column 0 and the zero codeword behind it; lengths=True adds a third result, the segments' lengths [B] (None with
        trimming off).  max_pause: as solo_batch; the row then holds its segments end to end.  filters: as
        solo_batch."""
        return self._infer(text_list, lang_list, style, total_step, speed, output_rate=output_rate, loudness=loudness,
                           encoding=encoding, trim_silence=trim_silence, lengths=lengths, limiter=limiter, peak_mode=peak_mode, max_pause=max_pause,
                           filters=filters)


def _filter_setting(v):
    """A filters argument -> a tuple of (type, freq_hz, q, gain_db), empty for off: None / False / [] = off.  ValueError naming the field
    for a malformed entry (binding.filter_args); the numeric limits are checked by the engine against the output rate in force."""
    return binding.filter_args(None if v is False else v)


def _limiter_setting(v):
    """A limiter argument -> the look-ahead in ms, or None for off: None / False = off, True = 5 ms, a number = the look-ahead.
    ValueError outside the ABI's range."""
    on, ms = binding.limiter_args(v)
    return ms if on else None


def _pause_setting(v):
    """A max_pause argument -> milliseconds, or None for off: None / False = off.  ValueError outside the ABI's range."""
    on, ms = binding.pause_limit_args(v)
    return ms if on else None


def _trim_setting(v):
    """A trim_silence argument -> (top_db, keep_ms, fade_ms), or None for off: None / False = off, a number = top_db with 20 ms kept
    and a 5 ms fade, a triple = all three.  ValueError outside the ABI's ranges."""
    if v is None or v is False:
        return None
    return binding.silence_trim_args(v)[1:]


def _loudness_setting(v):
    """A loudness argument -> (target LUFS, ceiling dBFS), or None for off: None / False = off, a number = the target with a
    -1 dBFS peak ceiling, a pair = (target, ceiling)."""
    if v is None or v is False:
        return None
    if isinstance(v, (tuple, list)):
        t, c = v
        return float(t), float(c)
    return float(v), -1.0


def load_cfgs(onnx_dir):
    with open(os.path.join(onnx_dir, "tts.json"), "r") as f:
        return json.load(f)


def load_text_to_speech(onnx_dir, use_gpu=True, device=0, dtype="bf16", allow_synthetic=None, weight_seed=7, noise_seed=None, output_rate=None,
                        loudness=None, trim_silence=None, limiter=None, peak_mode=None, max_pause=None, filters=None):
    """py/helper.py:316-337.  use_gpu=True is the only mode (the reference only had the CPU one).  An unusable asset directory is an
    error, as in the reference (cpp/helper.cpp:805); only when the caller opts in — `allow_synthetic=True`, or TTS_ALLOW_SYNTHETIC=1
    in the environment when the argument is left at None — does the engine fall back to the default architecture on synthetic
    weights (benchmarks and tests on machines without the Hugging Face assets), and it says so.  `output_rate` (Hz): the rate of the
    returned audio, resampled on the GPU (include/stn.h, stn_set_output_rate); None returns the model's rate.  `loudness`: normalize
    every utterance to this BS.1770-4 integrated loudness on the GPU (a target in LUFS, or (target, peak ceiling dBFS); include/stn.h,
    stn_set_loudness); None leaves the level as synthesized.  `trim_silence`: trim leading and trailing silence of every utterance by
    level on the GPU (top_db, or (top_db, keep_ms, fade_ms); include/stn.h, stn_set_silence_trim); None returns the waves as synthesized.
    `limiter`: with `loudness`, every utterance gets the full loudness gain and a look-ahead peak limiter holds the ceiling (True = 5 ms of
    look-ahead, or milliseconds in [0.5, 10]; include/stn.h, stn_set_limiter); None keeps the capped gain.
    `peak_mode`: "true" makes the ceiling of `loudness` a true-peak ceiling (dBTP, 4x oversampled; include/stn.h, stn_set_peak_mode); None
    or "sample" keeps the sample-peak ceiling.  `max_pause`: with `trim_silence`, every pause inside an utterance longer than this many
    milliseconds ([20, 5000]) is shortened to it on the GPU (include/stn.h, stn_set_pause_limit); None leaves the pauses as synthesized.
    `filters`: every utterance goes through this chain of up to 8 biquads on the GPU, after the resampler and before everything above (a
    list as binding.filter_args takes it, e.g. [("highpass", 80)]; include/stn.h, stn_set_filters); None leaves the spectrum as synthesized."""
    _trim_setting(trim_silence)  # (refused before the engine is created)
    _pause_setting(max_pause)
    _limiter_setting(limiter)
    binding.peak_mode_id(peak_mode)
    _filter_setting(filters)
    if allow_synthetic is None:
        allow_synthetic = os.getenv("TTS_ALLOW_SYNTHETIC", "0").strip().lower() in {"1", "true", "yes", "y", "on"}
    if not use_gpu:
        raise NotImplementedError("CPU mode is not supported: this engine runs on MI355X only")
    eng = binding.Engine(device, dtype)
    try:
        eng.load_dir(onnx_dir)
        cfgs = load_cfgs(onnx_dir)
        with open(os.path.join(onnx_dir, "unicode_indexer.json"), "r") as f:
            tp = host.UnicodeProcessor(np.asarray(json.load(f), np.int64))
        synthetic = False
    except binding.StnError as e:
        if not allow_synthetic:
            raise
        print(f"model assets unavailable ({e}); synthetic weights from the default architecture (seed {weight_seed})")
        a = default_arch()
        eng.load_synthetic(a, weight_seed)
        cfgs = {"ae": {"sample_rate": a.sample_rate, "base_chunk_size": a.base_chunk_size},
                "ttl": {"chunk_compress_factor": a.chunk_compress_factor, "latent_dim": a.latent_dim}}
        tp = host.UnicodeProcessor(host.synthetic_indexer())
        synthetic = True
    tts = TextToSpeech(eng, tp, cfgs, noise_seed, output_rate, loudness, trim_silence, limiter, peak_mode, max_pause, filters)
    tts.synthetic = synthetic
    return tts
