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
from .output import OutputSettings


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

    def __init__(self, engine, text_processor, cfgs, noise_seed=None, settings=OutputSettings()):
        self.engine = engine
        self.text_processor = text_processor
        self.cfgs = cfgs
        self.sample_rate = cfgs["ae"]["sample_rate"]  # the model's rate: it sizes the latent (latent_geometry)
        settings.apply(engine)
        self.settings = settings.decided()  # the instance's: what a call that sets nothing gets, every setting decided
        self.output_rate = self._rate(self.settings)  # rate of the returned audio
        self.base_chunk_size = cfgs["ae"]["base_chunk_size"]
        self.chunk_compress_factor = cfgs["ttl"]["chunk_compress_factor"]
        self.ldim = cfgs["ttl"]["latent_dim"]
        self.noise_seed = noise_seed  # None: fresh noise per call, like np.random.randn in the reference
        self._lock = threading.RLock()  # (re-entrant: a caller inside exclusive() calls the methods that take it)
        self._calls = 0

    def exclusive(self):
        """A context in which no other thread's call runs on this instance: a synthesis and the loudness_report of its batch belong in
        one, since the report is about whatever batch the engine holds when it runs."""
        return self._lock

    def _seed(self):
        if self.noise_seed is None:
            return secrets.randbits(63) | 1
        self._calls += 1
        return self.noise_seed + self._calls - 1

    def _rate(self, settings):
        return settings.output_rate or self.sample_rate

    @property
    def trim_silence(self):
        """The instance's trimming: (top_db, keep_ms, fade_ms), or None when off"""
        return self.settings.trim_silence or None

    def _infer(self, text_list, lang_list, style, total_step, speed=1.05, call=OutputSettings(), length_aware=False, encoding=None, join=None,
               lengths=False):
        """call: this call's settings over the instance's.  lengths: returns (wav, duration, len) with len [B] the samples each row holds
        from column 0: its trimmed segment with trimming on (Engine.batch_silence_edges, never a duration product; with the pause limit
        Engine.batch_pauses' len_b), else None."""
        if len(text_list) != style.ttl.shape[0]:
            raise ValueError("Number of texts must match number of style vectors")
        ids, mask = self.text_processor(text_list, lang_list)
        with self._lock, call.applied(self.engine, self.settings) as now:
            # length-aware batches (the chunks of a long text, the service's merged requests) come in ever-changing lengths: shape
            # buckets let them share captured graphs (stn_set_shape_buckets: every row stays exact over its own samples, rows are
            # just longer); a plain batch keeps the reference's exact [B, L * chunk] result
            self.engine.set_vocoder_mode(length_aware)
            self.engine.set_shape_buckets(length_aware)
            try:
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
                if not now.trim_silence:
                    return out[0], out[1], None
                if now.max_pause:
                    return out[0], out[1], self.engine.batch_pauses()[0]
                start, end = self.engine.batch_silence_edges()
                return out[0], out[1], end - start
            finally:
                self.engine.set_vocoder_mode(False)
                self.engine.set_shape_buckets(False)

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

    def solo_batch(self, text_list, lang_list, style, total_step, speed=1.05, encoding=None, **out):
        """Independent utterances as one batch whose rows equal what each would give alone (length-aware vocoder):
        returns a list of per-utterance waves of L_i * chunk_size samples (at the output rate: the resampled length of those)
        and the durations.  The building block of the long-form path and of the service's dynamic batching.
        out: this call's OutputSettings keywords instead of the instance's; every utterance is filtered, de-essed, compressed, normalized and limited on its
        own, and with trim_silence every wave is its trimmed segment (max_pause: what the cuts leave of it), cut at the length the GPU
        found.  encoding (a name or binding.ENC_*; None: float32): the waves in that sample encoding, encoded on the GPU
        (binding.encoded_empty's dtypes)."""
        call = OutputSettings.parse(**out)
        wav, dur, seg = self._infer(text_list, lang_list, style, total_step, speed, call, length_aware=True, encoding=encoding, lengths=True)
        if seg is not None:
            return [wav[i, : int(n)] for i, n in enumerate(seg)], dur
        cs = self.base_chunk_size * self.chunk_compress_factor
        lens = [int(self.latent_lengths(dur[i:i + 1])[0]) for i in range(len(text_list))]
        rate = self._rate(call.over(self.settings))
        return [wav[i, : min(self.out_samples(n * cs, rate), wav.shape[1])] for i, n in enumerate(lens)], dur

    def joined_batch(self, text_list, lang_list, style, total_step, speed=1.05, rows=None, silence_duration=0.3, encoding=None,
                     loudness_scope="chunk", trim_chunks=False, **out):
        """solo_batch whose rows are joined on the GPU into len(rows) waves: rows[g] consecutive utterances each (None: all of them
        in one), silence_duration (one value, or one per wave) seconds of silence between two of them — the encoding's zero codeword.
        Returns (list of joined waves, their durations: the reference's fp32 sum d = dur_0; d += dur_i + silence).  loudness_scope,
        with normalization on: "chunk", every utterance with its own gain (what joining solo_batch's rows gives, byte for byte);
        "text", every joined wave measured as one BS.1770 programme, silences included, and scaled by one gain (and limited as one).
        trim_chunks: every utterance cut at its duration before the join (the reference's Rust host) instead of its whole wave (C++ /
        Python hosts).  out: as solo_batch, every utterance on its own before the join; with trim_silence the pause between two of them
        is the silence asked for plus twice the kept margin, and the durations are those of the segments."""
        if loudness_scope not in ("chunk", "text"):
            raise ValueError(f"loudness_scope {loudness_scope!r}: 'chunk' or 'text'")
        call = OutputSettings.parse(**out)
        rows = [len(text_list)] if rows is None else [int(r) for r in rows]
        rate = self._rate(call.over(self.settings))
        sil = np.broadcast_to(np.asarray(silence_duration, np.float64), (len(rows),))
        join = {"rows": rows, "gap_samples": [int(s * rate) for s in sil], "gap_seconds": sil.astype(np.float32),
                "mode": "trim" if trim_chunks else "whole", "gain_scope": "programme" if loudness_scope == "text" else "row"}
        return self._infer(text_list, lang_list, style, total_step, speed, call, length_aware=True, encoding=encoding, join=join)

    def __call__(self, text, lang, style, total_step, speed=1.05, silence_duration=0.3, encoding=None, loudness_scope="chunk",
                 trim_chunks=False, **out):
        """Long-form synthesis: the text is chunked, the chunks run as one length-aware batch and are joined with silence on the GPU
        (one joined fetch: py/helper.py:235-243's untrimmed chunk waves with zeros between).  encoding, loudness_scope, trim_chunks and
        out: as joined_batch (one chunk is its own programme); with trim_silence the returned wave ends with the speech."""
        if style.ttl.shape[0] != 1:
            raise ValueError("Single speaker text to speech only supports single style")
        if loudness_scope not in ("chunk", "text"):
            raise ValueError(f"loudness_scope {loudness_scope!r}: 'chunk' or 'text'")
        chunks = host.chunk_text(text, 120 if lang == "ko" else 300)
        call = OutputSettings.parse(**out)
        if len(chunks) == 1 and not trim_chunks and not call.over(self.settings).trim_silence:  # (one chunk: the row's gain is the text's)
            return self._infer(chunks, [lang], style, total_step, speed, call, encoding=encoding)
        n = len(chunks)
        rep = Style(np.repeat(style.ttl, n, axis=0), np.repeat(style.dp, n, axis=0))
        waves, dur = self.joined_batch(chunks, [lang] * n, rep, total_step, speed, silence_duration=silence_duration, encoding=encoding,
                                       loudness_scope=loudness_scope, trim_chunks=trim_chunks, **out)
        return waves[0][None, :], np.array([dur[0]], np.float32)

    def batch(self, text_list, lang_list, style, total_step, speed=1.05, encoding=None, lengths=False, **out):
        """One padded batch -> (wav [B, W] float32, duration [B]); with an encoding (a name or binding.ENC_*), the rows in that sample
        encoding instead, encoded on the GPU (binding.encoded_empty's dtypes).  out: this call's OutputSettings keywords; with
        trim_silence row b holds its trimmed segment (max_pause: its segments end to end) from column 0 and the zero codeword behind
        it, and lengths=True adds a third result, the segments' lengths [B] (None with trimming off)."""
        return self._infer(text_list, lang_list, style, total_step, speed, OutputSettings.parse(**out), encoding=encoding, lengths=lengths)

    def loudness_report(self, rows=None, silence_duration=0.3, trim_chunks=False, **out):
        """The loudness of the batch the engine holds (after batch, solo_batch, joined_batch or __call__), measured on the GPU before the
        loudness gain -> dict of arrays: integrated (LUFS), peak, gain (Engine.batch_loudness), max_momentary and max_short_term (LUFS:
        the 400 ms and 3 s maxima EBU R 128 s1 limits; -inf where the audio is shorter), range (LU, EBU Tech 3342) and n_short_term (the
        3 s windows behind the range's gates; under 2 the range is 0).  rows None: one entry per row of the batch.  rows (as
        joined_batch's, with its silence_duration and trim_chunks): one entry per joined wave, measured as one programme, silences
        included.  out: the OutputSettings keywords the audio was asked with, when they were a call's and not the instance's.  While the
        limiter is off, a maximum after normalization is the reported one plus 20 log10(gain); the range does not depend on the gain."""
        call = OutputSettings.parse(**out)
        with self._lock, call.applied(self.engine, self.settings) as now:
            if rows is None:
                lufs, peak, gain = self.engine.batch_loudness()
                m, s, lra, n_st = self.engine.batch_loudness_range()
            else:
                rows = [int(r) for r in rows]
                rate = self._rate(now)
                sil = np.broadcast_to(np.asarray(silence_duration, np.float64), (len(rows),))
                join = (rows, [int(v * rate) for v in sil], sil.astype(np.float32), "trim" if trim_chunks else "whole")
                lufs, peak, gain = self.engine.batch_join_loudness(*join)
                m, s, lra, n_st = self.engine.batch_join_loudness_range(*join)
        return {"integrated": lufs, "peak": peak, "gain": gain, "max_momentary": m, "max_short_term": s, "range": lra, "n_short_term": n_st}

    def pitch_report(self, rows=None, params=None, **out):
        """The pitch of the batch the engine holds (after batch, solo_batch, joined_batch or __call__; inside exclusive(), like
        loudness_report), tracked on the GPU by YIN on the signal loudness_report measures (Engine.batch_f0) -> dict of arrays: frames,
        voiced, median_hz, mean_hz (geometric), min_hz, max_hz (0 where nothing is voiced), and f0 / ap, the tracks [B, Fmax] (f0 in
        Hz at a 10 ms hop, 0 = unvoiced; row b's frames are its first frames[b]).  rows None: one entry per row of the batch.  rows (as
        joined_batch's): one entry per joined wave, the statistics pooled on the host over its member rows' frames (the silences
        between them hold no voiced frame), and no tracks.  params: binding.f0_params' argument (None: 60 to 500 Hz, threshold 0.15,
        gate -60 dB).  out: the OutputSettings keywords the audio was asked with, when they were a call's and not the instance's."""
        call = OutputSettings.parse(**out)
        with self._lock, call.applied(self.engine, self.settings):
            f0, ap, st = self.engine.batch_f0(params)
        if rows is None:
            return {**st, "f0": f0, "ap": ap}
        rows = [int(r) for r in rows]
        if any(r < 1 for r in rows) or sum(rows) != f0.shape[0]:
            raise ValueError(f"rows {rows}: positive counts that add up to the batch's {f0.shape[0]} rows")
        pooled, b = [], 0
        for r in rows:
            track = np.concatenate([f0[i, : st["frames"][i]] for i in range(b, b + r)])
            pooled.append(binding.f0_stats_rule(track))
            b += r
        return {k: np.array([p[k] for p in pooled]) for k in binding.F0_STATS.names}


def _trim_setting(v):
    """A trim_silence keyword normalized: (top_db, keep_ms, fade_ms), or None for off.  (The tests of the ranges read this and the next.)"""
    return OutputSettings.parse(trim_silence=v).trim_silence or None


def _limiter_setting(v):
    """A limiter keyword normalized: the look-ahead in ms, or None for off."""
    return OutputSettings.parse(limiter=v).limiter or None


def load_cfgs(onnx_dir):
    with open(os.path.join(onnx_dir, "tts.json"), "r") as f:
        return json.load(f)


def load_text_to_speech(onnx_dir, use_gpu=True, device=0, dtype="bf16", allow_synthetic=None, weight_seed=7, noise_seed=None, **out):
    """py/helper.py:316-337.  use_gpu=True is the only mode (the reference only had the CPU one).  An unusable asset directory is an
    error, as in the reference (cpp/helper.cpp:805); only when the caller opts in — `allow_synthetic=True`, or TTS_ALLOW_SYNTHETIC=1
    in the environment when the argument is left at None — does the engine fall back to the default architecture on synthetic
    weights (benchmarks and tests on machines without the Hugging Face assets), and it says so.  out: the instance's OutputSettings
    keywords (output_rate, filters, expander, deesser, compressor, loudness, trim_silence, max_pause, limiter, peak_mode, dither, pitch), each off when
    left out.  expander=True turns the noise floor between words down by the "speech" default, expander={"threshold_db": -45} names fields.  pitch=2.0 shifts every utterance up two semitones in front of everything else.  dither acts on what is fetched as "pcm16" or "pcm24" (encoding=); the float waves are the same with and without it."""
    settings = OutputSettings.parse(**out)  # (refused before the engine is created)
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
    tts = TextToSpeech(eng, tp, cfgs, noise_seed, settings)
    tts.synthetic = synthetic
    return tts
