"""HTTP face of the engine: the request schema, validation messages and responses of the reference's FastAPI service
(/root/reference/py/service.py:28-136: GET /health, POST /tts -> audio/wav or application/zip), on top of the C ABI.

What is different is throughput under concurrency.  The reference handles one request at a time on ORT-CPU.  Here
single-utterance requests that arrive together are merged by a `DynamicBatcher` into ONE resident batch on the GPU
(length-aware vocoder: a request's audio does not depend on who it shared the batch with) — the chunks of long texts
included; a `batch: true` request keeps the reference's semantics (its own padded batch, `TextToSpeech.batch`).

    TTS_ONNX_DIR=assets/onnx TTS_DTYPE=bf16 uvicorn supertonic_amd.service:app
"""
import contextlib
import io
import os
import threading
import time
import zipfile
from collections import namedtuple
from typing import List, Literal, Optional, Union

import numpy as np

from . import binding, host
from .output import OutputSettings
from .tts import Style, load_text_to_speech, load_voice_style

AVAILABLE_LANGS = host.AVAILABLE_LANGS
# response header -> its entry of TextToSpeech.loudness_report (a request with "loudness_report": true; three decimals, -inf spelled so)
REPORT_HEADERS = {"X-Loudness-Integrated": "integrated", "X-Loudness-Range": "range", "X-Loudness-Max-Momentary": "max_momentary",
                  "X-Loudness-Max-Short-Term": "max_short_term"}
# response header -> its entry of TextToSpeech.pitch_report (a request with "pitch_report": true; Hz, three decimals); X-Pitch-Voiced,
# the share voiced / frames, goes with them
PITCH_HEADERS = {"X-Pitch-Median-Hz": "median_hz", "X-Pitch-Min-Hz": "min_hz", "X-Pitch-Max-Hz": "max_hz"}
PITCH_FIELDS = ("frames", "voiced", "median_hz", "mean_hz", "min_hz", "max_hz")


# what two requests must share to run as one engine batch (the settings cover a whole batch; every row keeps its own gain)
# (pitch_set: whether the request names a pitch.  OutputSettings compares an unset pitch equal to an off one; the key must not: a request
# that names none gets the synthesizer's own pitch, one that says 0 gets none.  expander_set: the same for the expander.  pitch_mode: the
# mode in force for the request, its own or else the synthesizer's: OutputSettings compares an unset mode equal to "resample", which is
# the same request only where the synthesizer's own is "resample")
BatchKey = namedtuple("BatchKey", "total_step speed encoding loudness_scope trim_chunks settings pitch_set expander_set pitch_mode")


def batch_key(model_rate, total_step, speed, sample_rate=None, loudness=None, peak_ceiling=-1.0, encoding=None, loudness_scope="chunk",
              trim_chunks=False, trim_silence=None, limiter_ms=None, peak_mode=None, max_pause_ms=None, filters=None, deesser=None, dither=None,
              dither_seed=None, pitch=None, expander=None, pitch_mode=None, own_pitch_mode="resample", compressor=None):
    """A request's BatchKey: two requests merge if and only if their keys are equal.  Everything is validated here (ValueError), in front
    of the queue.  A field the request leaves at None is unset in the key (the synthesizer's own setting holds), never the synthesizer's
    value; key.settings.kwargs() is then exactly what the request set, which is what the synthesizer is called with.
    sample_rate: the rate of the waves (the model's is model_rate).  loudness: normalize each wave to this many LUFS with the gain capped
    at peak_ceiling dBFS.  limiter_ms, peak_mode ("sample" or "true"): OutputSettings' limiter and peak_mode; they act on the loudness
    gain, so without loudness they (and peak_ceiling) are validated and dropped.  trim_silence: top_db or (top_db, keep_ms, fade_ms), no
    bool.  max_pause_ms: without trim_silence, validated and dropped likewise.  filters: a list as binding.filter_args takes it, [] =
    off, checked against the request's rate.  deesser: True, a dict or an 8-tuple as binding.deesser_args takes it, False = off, checked
    against the request's rate as well.  compressor: True, a dict or a 6-tuple as binding.compressor_args takes it, False = off,
    checked against the engine's limits.  dither ("off", "round", "tpdf", "tpdf-hp" or true for "tpdf"; false = off) with dither_seed (an
    integer in [0, 2^64), 0 when left out; alone it is validated and dropped): OutputSettings' dither.  encoding: the waves in that sample encoding (binding.ENC_* or a name; None: float32).
    loudness_scope, trim_chunks (TextToSpeech.joined_batch): one fetch has one scope and one mode.  pitch: semitones in [-12, 12] (0 = off),
    refused with the engine's message: requests of different pitch never share a batch, and neither do one that names none (the
    synthesizer's own holds) and one that says 0.  expander: True, a dict or a 7-tuple as binding.expander_args takes it, False = off,
    checked against the engine's limits; as with pitch, a request that names none and one that says false never share a batch.
    pitch_mode: "resample" or "formant" (OutputSettings' pitch_mode), refused with binding.pitch_mode_id's message; own_pitch_mode: the
    synthesizer's own, which a request that names none runs under: requests under different modes never share a batch."""
    chain = None if filters is None else binding.filter_args(filters)
    why = chain and binding.filter_error(chain, int(sample_rate or model_rate))
    if why:
        raise ValueError(why)
    dees = None if deesser is None else (binding.deesser_args(deesser) or False)
    why = dees and binding.deesser_error(dees, int(sample_rate or model_rate))
    if why:
        raise ValueError(why)
    comp = None if compressor is None else (binding.compressor_args(compressor) or False)
    why = comp and binding.compressor_error(comp, int(sample_rate or model_rate))
    if why:
        raise ValueError(why)
    xpd = None if expander is None else (binding.expander_args(expander) or False)
    why = xpd and binding.expander_error(xpd, int(sample_rate or model_rate))
    if why:
        raise ValueError(why)
    dith = binding.dither_args(dither or "off", dither_seed) or False
    s = OutputSettings.parse(output_rate=sample_rate, filters=chain, expander=xpd, deesser=dees, compressor=comp, dither=None if dither is None else dith, pitch=pitch, pitch_mode=pitch_mode, loudness=None if loudness is None else (loudness, peak_ceiling),
                             trim_silence=None if trim_silence is None else binding.silence_trim_args(trim_silence)[1:],
                             max_pause=None if max_pause_ms is None else float(max_pause_ms),
                             limiter=None if limiter_ms is None else float(limiter_ms), peak_mode=None if peak_mode is None else str(peak_mode))
    if s.loudness is None:
        s = s.replace(limiter=None, peak_mode=None)
    if s.trim_silence is None:
        s = s.replace(max_pause=None)
    return BatchKey(int(total_step), float(speed), None if encoding is None else binding.encoding_id(encoding), str(loudness_scope),
                    bool(trim_chunks), s, s.pitch is not None, s.expander is not None, s.pitch_mode or binding.pitch_mode_name(own_pitch_mode))


class _Job:
    __slots__ = ("texts", "lang", "style", "key", "silence", "done", "waves", "durs", "error", "want_report", "report", "want_pitch", "pitch")

    def __init__(self, texts, lang, style, key, silence=None, want_report=False, want_pitch=False):
        self.texts, self.lang, self.style, self.key, self.silence = texts, lang, style, key, silence
        self.done = threading.Event()
        self.waves = self.durs = self.error = None
        self.want_report, self.report = bool(want_report), None
        self.want_pitch, self.pitch = bool(want_pitch), None


class DynamicBatcher:
    """Merges concurrent single-speaker jobs (each: the chunks of one text, one language, one style) that share a BatchKey into one
    engine batch.  A worker thread owns the engine: it takes the oldest job, waits up to `max_wait_ms` for company (or until `max_batch`
    utterances are queued), runs `tts.solo_batch` once and hands every job its own rows.  Rows are independent by construction, so
    merging changes latency and throughput, not audio."""

    def __init__(self, tts, max_batch=128, max_wait_ms=3.0):
        self.tts, self.max_batch, self.max_wait = tts, int(max_batch), max_wait_ms / 1e3
        self._q, self._cv = [], threading.Condition()
        self._stop = False
        self.batches = []  # sizes of the engine batches run so far (diagnostics / tests)
        self._t = threading.Thread(target=self._run, name="stn-batcher", daemon=True)
        self._t.start()

    def submit(self, texts, lang, style, *request, silence_duration=None, loudness_report=False, pitch_report=False, **request_kw):
        """Blocks until the job's utterances are synthesized; returns (list of waves, durations [n]).  request: total_step, speed and the
        rest of batch_key's arguments.  silence_duration (seconds, not None): the job's utterances are the chunks of one text and come
        back as ONE wave, joined with that much silence on the GPU (one programme per job of the batch's joined fetch, each job its own
        gap), with its duration.  loudness_report (no part of the key: it changes no audio): a third result, the job's entry of
        TextToSpeech.loudness_report for its joined wave as a dict of floats, or None when the synthesizer has no such report or the
        job is not joined on the GPU.  pitch_report (no part of the key either): one more result behind those, the job's entry of
        TextToSpeech.pitch_report (pooled over its chunks) as a dict of floats, or None under the same conditions."""
        own = getattr(getattr(self.tts, "settings", None), "pitch_mode", None)
        key = batch_key(self.tts.sample_rate, *request, own_pitch_mode=own, **request_kw)
        job = _Job(list(texts), lang, style, key, None if silence_duration is None else float(silence_duration), loudness_report, pitch_report)
        with self._cv:
            if self._stop:
                raise RuntimeError("batcher is closed")
            self._q.append(job)
            self._cv.notify_all()
        job.done.wait()
        if job.error is not None:
            raise job.error
        return (job.waves, job.durs) + ((job.report,) if loudness_report else ()) + ((job.pitch,) if pitch_report else ())

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify_all()
        self._t.join(timeout=10)

    def _take(self):
        with self._cv:
            while not self._q and not self._stop:
                self._cv.wait()
            if self._stop and not self._q:
                return None
            key = self._q[0].key
            deadline = time.monotonic() + self.max_wait
            while True:
                mine = [j for j in self._q if j.key == key]
                if sum(len(j.texts) for j in mine) >= self.max_batch or self._stop:
                    break
                left = deadline - time.monotonic()
                if left <= 0:
                    break
                self._cv.wait(left)
            picked, n = [], 0
            for j in [j for j in self._q if j.key == key]:
                if picked and n + len(j.texts) > self.max_batch:
                    break
                picked.append(j)
                n += len(j.texts)
            for j in picked:
                self._q.remove(j)
            return picked

    def _run(self):
        while True:
            jobs = self._take()
            if jobs is None:
                return
            try:
                texts = [t for j in jobs for t in j.texts]
                langs = [j.lang for j in jobs for _ in j.texts]
                ttl = np.concatenate([np.repeat(j.style.ttl, len(j.texts), axis=0) for j in jobs])
                dp = np.concatenate([np.repeat(j.style.dp, len(j.texts), axis=0) for j in jobs])
                key = jobs[0].key
                extra = key.settings.kwargs()  # (only what the requests set, as they set it)
                if key.encoding is not None:
                    extra["encoding"] = key.encoding
                joined = getattr(self.tts, "joined_batch", None)
                if joined is not None and all(j.silence is not None for j in jobs):
                    # one programme per job, joined by the fetch on the GPU; the report, when a job asked for one, is about the batch
                    # the engine then holds, so nothing else may run on the synthesizer in between
                    report = getattr(self.tts, "loudness_report", None) if any(j.want_report for j in jobs) else None
                    pitch = getattr(self.tts, "pitch_report", None) if any(j.want_pitch for j in jobs) else None
                    with getattr(self.tts, "exclusive", contextlib.nullcontext)() if report or pitch else contextlib.nullcontext():
                        waves, durs = joined(texts, langs, Style(ttl, dp), key.total_step, key.speed, rows=[len(j.texts) for j in jobs],
                                             silence_duration=[j.silence for j in jobs], loudness_scope=key.loudness_scope, trim_chunks=key.trim_chunks, **extra)
                        if report is not None:
                            rep = report(rows=[len(j.texts) for j in jobs], silence_duration=[j.silence for j in jobs],
                                         trim_chunks=key.trim_chunks, **key.settings.kwargs())
                            for g, j in enumerate(jobs):
                                if j.want_report:
                                    j.report = {k: float(v[g]) for k, v in rep.items()}
                        if pitch is not None:
                            rep = pitch(rows=[len(j.texts) for j in jobs], **key.settings.kwargs())
                            for g, j in enumerate(jobs):
                                if j.want_pitch:
                                    j.pitch = {k: float(v[g]) for k, v in rep.items()}
                    self.batches.append(len(texts))
                    for g, j in enumerate(jobs):
                        j.waves, j.durs = [waves[g]], np.asarray(durs[g:g + 1], np.float32)
                else:
                    if key.loudness_scope != "chunk" or key.trim_chunks:
                        raise RuntimeError("loudness_scope / trim_chunks need a synthesizer with a joined fetch (TextToSpeech.joined_batch)")
                    # a synthesizer without a joined fetch (a stand-in), or a caller that wants the rows: per-utterance waves; a job
                    # that asked for one wave gets the host join of them
                    waves, durs = self.tts.solo_batch(texts, langs, Style(ttl, dp), key.total_step, key.speed, **extra)
                    self.batches.append(len(texts))
                    o = 0
                    for j in jobs:
                        n = len(j.texts)
                        j.waves, j.durs = waves[o:o + n], np.asarray(durs[o:o + n], np.float32)
                        if j.silence is not None:
                            w, d = join_chunks(j.waves, j.durs, j.silence, key.settings.output_rate or self.tts.sample_rate, key.encoding)
                            j.waves, j.durs = [w], np.array([d], np.float32)
                        o += n
            except Exception as e:  # the requests fail, the worker lives on
                for j in jobs:
                    j.error = e
            for j in jobs:
                j.done.set()


def join_chunks(waves, durs, silence_duration, sample_rate, encoding=None):
    """TextToSpeech.__call__'s concatenation (py/helper.py:235-243): untrimmed chunk waves with zeros between (with an encoding: its
    zero codeword between waves in that encoding)."""
    if encoding is None:
        silence = np.zeros(int(silence_duration * sample_rate), np.float32)
    else:
        silence = binding.encoded_empty(encoding, 1, int(silence_duration * sample_rate))[0]
        silence[...] = binding.ZERO_CODEWORD[binding.encoding_id(encoding)]
    parts, dur = [], None
    for i, w in enumerate(waves):
        if i == 0:
            dur = np.float32(durs[0])
        else:
            parts.append(silence)
            dur = np.float32(dur + np.float32(durs[i] + np.float32(silence_duration)))
        parts.append(w)
    return np.concatenate(parts), float(dur)


def create_app(tts, max_batch=128, max_wait_ms=3.0, style_loader=None):
    """The FastAPI application around a TextToSpeech instance (supertonic_amd.tts or anything with its surface)."""
    from fastapi import FastAPI, HTTPException
    from fastapi.responses import JSONResponse, Response
    from pydantic import BaseModel, Field

    from contextlib import asynccontextmanager

    batcher = DynamicBatcher(tts, max_batch, max_wait_ms)

    @asynccontextmanager
    async def lifespan(_app):
        yield
        batcher.close()

    app = FastAPI(title="Supertonic TTS Service (MI355X)", lifespan=lifespan)
    app.state.batcher = batcher
    if style_loader is None:
        arch = tts.engine.arch if getattr(tts, "synthetic", False) else None

        def style_loader(paths):
            return load_voice_style(paths, verbose=False, synthetic_arch=arch)

    class TTSRequest(BaseModel):  # py/service.py:28-39
        text: Union[str, List[str]] = Field(..., description="Text to synthesize.")
        lang: Union[str, List[str]] = Field("en", description="Language(s) for text.")
        voice_style: Union[str, List[str]] = Field("assets/voice_styles/M1.json", description="Voice style path(s).")
        total_step: int = Field(5, ge=1, le=50)
        speed: float = Field(1.05, gt=0.0)
        batch: bool = False
        silence_duration: float = Field(0.3, ge=0.0, description="Silence between chunks for non-batch mode.")
        sample_rate: Optional[int] = Field(None, description="Output sample rate in Hz (resampled on the GPU); null: the model's rate.")
        loudness: Optional[float] = Field(None, ge=-60.0, le=0.0, description="Normalize each utterance to this BS.1770-4 integrated "
                                                                              "loudness in LUFS (on the GPU); null: off.")
        peak_ceiling: float = Field(-1.0, ge=-30.0, le=0.0, description="Sample-peak ceiling in dBFS that caps the loudness gain.")
        limiter_ms: Optional[float] = Field(None, ge=0.5, le=10.0, description="With loudness: the full loudness gain, and a look-ahead peak "
                                                                               "limiter of this many milliseconds holds peak_ceiling; null: off.")
        peak_mode: Optional[Literal["sample", "true"]] = Field(None, description="With loudness: 'sample' holds peak_ceiling as a sample peak, 'true' as a true peak "
                                                           "(dBTP, 4x oversampled on the GPU); null: the synthesizer's setting.")
        encoding: str = Field("pcm16", description="Sample format of the WAV files (encoded on the GPU): pcm16, pcm24, f32, mulaw, alaw.")
        loudness_scope: str = Field("chunk", description="Non-batch mode with loudness: 'chunk' normalizes every chunk of a long text on its own, "
                                                         "'text' the joined text as one BS.1770 programme with one gain.")
        trim_chunks: bool = Field(False, description="Non-batch mode: cut every chunk at its duration before the join.")
        loudness_report: Optional[bool] = Field(None, description="True: a single-utterance response carries the headers X-Loudness-Integrated, "
                                                                  "X-Loudness-Range, X-Loudness-Max-Momentary and X-Loudness-Max-Short-Term "
                                                                  "(LUFS / LU, measured on the GPU before the loudness gain).  It changes no audio.")
        pitch_report: Optional[bool] = Field(None, description="True: a single-utterance response carries the headers X-Pitch-Median-Hz, "
                                                               "X-Pitch-Min-Hz, X-Pitch-Max-Hz (the YIN track of the audio on the GPU, 60 to "
                                                               "500 Hz at a 10 ms hop; 0 where nothing is voiced) and X-Pitch-Voiced (the share "
                                                               "of voiced frames).  It changes no audio.")
        trim_silence: Optional[float] = Field(None, ge=1.0, le=120.0, description="Trim leading and trailing silence by level (on the GPU): frames "
                                                                                 "more than this many dB below the loudest 10 ms frame; null: off.")
        trim_keep_ms: float = Field(20.0, ge=0.0, le=1000.0, description="Milliseconds kept in front of and behind the speech when trimming.")
        trim_fade_ms: float = Field(5.0, ge=0.0, le=50.0, description="Raised-cosine fade over each cut edge, in milliseconds.")
        max_pause_ms: Optional[float] = Field(None, ge=20.0, le=5000.0, description="With trim_silence: every pause inside an utterance longer than "
                                                                                    "this many milliseconds is shortened to it (on the GPU); null: off.")
        filters: Optional[List[dict]] = Field(None, description="Biquad chain every utterance goes through on the GPU, after the resampler and before "
                                                                "everything else: up to 8 of {type: highpass | lowpass | notch | peak | lowshelf | "
                                                                "highshelf, freq (Hz), q (0.7071), gain_db (0)}; null: off.")
        filter_preset: Optional[str] = Field(None, description="A named chain in front of filters: 'rumble' (high-pass at 80 Hz) or 'telephone' "
                                                               "(300 to 3400 Hz, 4th-order Butterworth).")
        deesser: Optional[Union[bool, dict]] = Field(None, description="De-esser every utterance goes through on the GPU, behind the filters and in "
                                                                       "front of the compressor: true (the speech default: 5500 Hz, -30 dB, "
                                                                       "4:1, knee 6 dB, attack 1 ms, release 40 ms, range 12 dB, split) or "
                                                                       "{freq_hz, threshold_db, ratio, knee_db, attack_ms, release_ms, range_db, "
                                                                       "mode}, the fields left out from that default; false: off; null: the "
                                                                       "server's.")
        expander: Optional[Union[bool, dict]] = Field(None, description="Downward expander / noise gate every utterance goes through on the GPU, "
                                                                        "behind the filters and in front of the de-esser: true (the speech "
                                                                        "default: -50 dB, 3:1, knee 6 dB, range 24 dB, attack 1 ms, hold 30 ms, "
                                                                        "release 150 ms) or {threshold_db, ratio, knee_db, range_db, attack_ms, "
                                                                        "hold_ms, release_ms}, the fields left out from that default; false: "
                                                                        "off; null: the server's.")
        compressor: Optional[Union[bool, dict]] = Field(None, description="Dynamic range compressor every utterance goes through on the GPU, behind "
                                                                          "the filters and before everything else: true (the speech default: "
                                                                          "-24 dB, 3:1, knee 6 dB, attack 5 ms, release 120 ms, makeup 0 dB) or "
                                                                          "{threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db}, the "
                                                                          "fields left out from that default; false: off; null: the server's.")
        dither: Optional[Union[bool, Literal["off", "round", "tpdf", "tpdf-hp"]]] = Field(
            None, description="How 16- and 24-bit PCM is quantized on the GPU: 'round' (to nearest), 'tpdf' (true: triangular dither of +-1 LSB "
                              "in front of the rounding), 'tpdf-hp' (the same power, high-passed); 'off' or false: truncation; null: the "
                              "server's.  No effect on f32, mulaw and alaw.")
        dither_seed: Optional[int] = Field(None, ge=0, lt=1 << 64, description="Seed of the dither noise (0 when left out): with the utterance's "
                                                                               "place in its batch and the sample index it fixes the noise.")
        pitch: Optional[float] = Field(None, description="Pitch shift in semitones, a number in [-12, 12], applied on the GPU in front of every other "
                                                         "setting without a change of duration; 0: off; null: the server's.  The response's "
                                                         "X-Pitch-Cents header carries the realised shift.")
        pitch_mode: Optional[str] = Field(None, description="What the pitch shift does to the formants: 'resample' (they move with the pitch) or "
                                                            "'formant' (the spectral envelope is put back on the GPU); null: the server's.  No "
                                                            "effect while pitch is off.")

    def ensure_list(v):
        return v if isinstance(v, list) else [v]

    @app.get("/health")
    def health():
        return JSONResponse({"status": "ok"})

    @app.post("/tts")
    def synthesize(req: TTSRequest):
        texts, langs, styles = ensure_list(req.text), ensure_list(req.lang), ensure_list(req.voice_style)
        if req.batch:
            if not (len(texts) == len(langs) == len(styles)):
                raise HTTPException(status_code=400, detail="text, lang, and voice_style must have the same length.")
        elif len(texts) != 1 or len(langs) != 1 or len(styles) != 1:
            raise HTTPException(status_code=400, detail="Non-batch mode requires single text, lang, and voice_style.")
        invalid = sorted({lang for lang in langs if lang not in AVAILABLE_LANGS})
        if invalid:
            raise HTTPException(status_code=400, detail=f"Invalid language(s): {', '.join(invalid)}")
        try:
            style = style_loader(styles)
        except (OSError, KeyError, ValueError) as e:
            raise HTTPException(status_code=400, detail=f"voice_style: {e}")
        sr = tts.sample_rate
        extra = {}
        if req.sample_rate is not None:
            why = binding.resample_error(tts.sample_rate, req.sample_rate)
            if why:
                raise HTTPException(status_code=400, detail=f"sample_rate {req.sample_rate} is not supported ({why}); supported: "
                                                            + ", ".join(str(r) for r in binding.SUPPORTED_OUTPUT_RATES) + " Hz")
            sr, extra = req.sample_rate, {"output_rate": req.sample_rate}
        if req.loudness is not None:
            extra["loudness"] = (req.loudness, req.peak_ceiling)
            if req.limiter_ms is not None:
                extra["limiter"] = req.limiter_ms
            if req.peak_mode is not None:
                extra["peak_mode"] = req.peak_mode
        chain = None
        if req.filters is not None or req.filter_preset is not None:
            try:
                chain = binding.filter_args(req.filters, req.filter_preset)
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))
            why = binding.filter_error(chain, sr) if chain else ""
            if why:
                raise HTTPException(status_code=400, detail=f"filters: {why}")
            extra["filters"] = list(chain)
        dees = None
        if req.deesser is not None:
            try:
                dees = binding.deesser_args(req.deesser) or False
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))
            why = binding.deesser_error(dees, sr) if dees else ""
            if why:
                raise HTTPException(status_code=400, detail=why)
            extra["deesser"] = dees
        xpd = None
        if req.expander is not None:
            try:
                xpd = binding.expander_args(req.expander) or False
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))
            why = binding.expander_error(xpd, sr) if xpd else ""
            if why:
                raise HTTPException(status_code=400, detail=why)
            extra["expander"] = xpd
        comp = None
        if req.compressor is not None:
            try:
                comp = binding.compressor_args(req.compressor) or False
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))
            why = binding.compressor_error(comp, sr) if comp else ""
            if why:
                raise HTTPException(status_code=400, detail=why)
            extra["compressor"] = comp
        dith = None
        try:
            dith = binding.dither_args(req.dither or "off", req.dither_seed) or False
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        if req.dither is None:
            dith = None  # (a seed alone: validated and dropped)
        else:
            extra["dither"] = dith
        pitch = None
        if req.pitch is not None:
            why = binding.pitch_error(req.pitch)
            if why:
                raise HTTPException(status_code=400, detail=why)
            pitch = binding.pitch_args(req.pitch)
            extra["pitch"] = pitch
        if req.pitch_mode is not None:
            try:
                extra["pitch_mode"] = binding.pitch_mode_name(req.pitch_mode)
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))
        if req.encoding not in binding.ENCODINGS:
            raise HTTPException(status_code=400, detail=f"encoding {req.encoding!r} is not supported; supported: " + ", ".join(binding.ENCODINGS))
        if req.loudness_scope not in ("chunk", "text"):
            raise HTTPException(status_code=400, detail=f"loudness_scope {req.loudness_scope!r} is not supported; supported: chunk, text")
        # pcm16: the float waves, written as writeWavFile writes them (truncation); with dither in force, the GPU's dithered 16-bit samples
        dithering = dith if dith is not None else getattr(getattr(tts, "settings", None), "dither", None)
        enc = None if req.encoding == "pcm16" and not dithering else req.encoding
        ts = None if req.trim_silence is None else (req.trim_silence, req.trim_keep_ms, req.trim_fade_ms)
        if req.max_pause_ms is not None and ts is None:
            raise HTTPException(status_code=400, detail="max_pause_ms needs trim_silence: pauses are shortened inside trimmed utterances")
        if enc is not None:
            extra["encoding"] = enc
        # the report of a single-utterance response (a synthesizer without loudness_report yields no headers)
        reporter = getattr(tts, "loudness_report", None) if req.loudness_report and len(texts) == 1 else None
        pitcher = getattr(tts, "pitch_report", None) if req.pitch_report and len(texts) == 1 else None  # (likewise)
        report = pitched = None
        if req.batch:
            with getattr(tts, "exclusive", contextlib.nullcontext)() if reporter or pitcher else contextlib.nullcontext():
                if ts is not None:  # every wave is its trimmed segment, cut at the length the GPU found
                    if req.max_pause_ms is not None:
                        extra["max_pause"] = req.max_pause_ms
                    wav, dur, seg = tts.batch(texts, langs, style, req.total_step, req.speed, trim_silence=ts, lengths=True, **extra)
                    chunks = [wav[i, : int(seg[i])] for i in range(wav.shape[0])]
                else:
                    wav, dur = tts.batch(texts, langs, style, req.total_step, req.speed, **extra)
                    chunks = [wav[i, : int(sr * float(dur[i]))] for i in range(wav.shape[0])]  # _slice_audio, py/service.py:62-71
                if reporter:  # (the settings of the call above, without what is no output setting)
                    kw = {k: v for k, v in extra.items() if k != "encoding"}
                    report = {k: float(v[0]) for k, v in reporter(**(kw if ts is None else dict(kw, trim_silence=ts))).items()}
                if pitcher:
                    kw = {k: v for k, v in extra.items() if k != "encoding"}
                    pitched = {k: float(v[0]) for k, v in pitcher(**(kw if ts is None else dict(kw, trim_silence=ts))).items() if k in PITCH_FIELDS}
        else:
            pieces = host.chunk_text(texts[0], 120 if langs[0] == "ko" else 300)
            more = {"loudness_report": True} if reporter else {}  # (absent otherwise: the call is today's)
            if pitcher:
                more["pitch_report"] = True
            waves, durs, *rep = batcher.submit(pieces, langs[0], style, req.total_step, req.speed, req.sample_rate, req.loudness, req.peak_ceiling,
                                               enc, silence_duration=req.silence_duration, loudness_scope=req.loudness_scope,
                                               trim_chunks=req.trim_chunks, trim_silence=ts, limiter_ms=req.limiter_ms, peak_mode=req.peak_mode,
                                               max_pause_ms=req.max_pause_ms, filters=chain, expander=xpd, deesser=dees, compressor=comp,
                                               dither=None if dith is None else (dith or "off"), dither_seed=dith[1] if dith else None, pitch=pitch, pitch_mode=extra.get("pitch_mode"), **more)
            pitched = rep.pop() if pitcher else None
            report = rep[0] if rep else None
            wav, d = waves[0], float(durs[0])  # the chunks joined by the batch's fetch (join_chunks' result)
            chunks = [wav if ts is not None else wav[: int(sr * d)]]  # (trimmed: the joined wave is already its own length)
        if len(chunks) == 1:
            name = host.sanitize_filename(texts[0], 40) or "tts"
            headers = {"Content-Disposition": f'attachment; filename="{_ascii(name)}.wav"'}
            in_force = pitch if pitch is not None else (getattr(getattr(tts, "settings", None), "pitch", None) or 0.0)
            headers["X-Pitch-Cents"] = f"{binding.pitch_cents(in_force):.3f}"  # the realised shift (a / b), 0.000 when off
            if report:
                headers.update({h: f"{report[k]:.3f}" for h, k in REPORT_HEADERS.items()})
            if pitched:
                headers.update({h: f"{pitched[k]:.3f}" for h, k in PITCH_HEADERS.items()})
                headers["X-Pitch-Voiced"] = f"{pitched['voiced'] / pitched['frames'] if pitched['frames'] else 0.0:.3f}"
            return Response(host.wav_bytes(chunks[0], sr, enc), media_type="audio/wav", headers=headers)
        zbuf = io.BytesIO()
        with zipfile.ZipFile(zbuf, "w", compression=zipfile.ZIP_DEFLATED) as zf:
            for i, c in enumerate(chunks):
                zf.writestr((host.sanitize_filename(texts[i], 40) or f"tts_{i + 1}") + ".wav", host.wav_bytes(c, sr, enc))
        return Response(zbuf.getvalue(), media_type="application/zip",
                        headers={"Content-Disposition": 'attachment; filename="tts_outputs.zip"'})

    return app


def _ascii(name):
    """HTTP header values are latin-1: non-ASCII characters of a sanitized file name become '_' in the header only."""
    return "".join(ch if ord(ch) < 128 else "_" for ch in name)


def __getattr__(name):  # `uvicorn supertonic_amd.service:app` builds the engine on first use, not at import
    if name == "app":
        flag = os.getenv("TTS_USE_GPU", "1").strip().lower() in {"1", "true", "yes", "y", "on"}
        tts = load_text_to_speech(os.getenv("TTS_ONNX_DIR", "assets/onnx"), flag, int(os.getenv("TTS_DEVICE", "0")),
                                  os.getenv("TTS_DTYPE", "bf16"))
        globals()["app"] = create_app(tts, int(os.getenv("TTS_MAX_BATCH", "128")), float(os.getenv("TTS_MAX_WAIT_MS", "3")))
        return globals()["app"]
    raise AttributeError(name)
