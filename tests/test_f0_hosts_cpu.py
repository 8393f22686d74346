"""The pitch report's hosts without a GPU, with stand-ins: TextToSpeech.pitch_report per row and pooled per
joined programme, the CLI's flag, the service's headers and the batcher's key."""
import os
import subprocess
import threading

import numpy as np
import pytest

from supertonic_amd import binding, service
from supertonic_amd.tts import Style, TextToSpeech

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
SR = 44100
STAT_KEYS = set(binding.F0_STATS.names)
TRACKS = np.array([[100.0, 0.0, 110.0, 0.0], [200.0, 210.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]], np.float32)
FRAMES = np.array([4, 2, 3], np.int32)


class FakeEngine:
    """batch_f0 as the binding has it, on three known tracks"""

    def __init__(self):
        self.calls = []

    def set_output_rate(self, hz):
        self.calls.append(("rate", hz))

    def batch_f0(self, params=None):
        self.calls.append(("f0", params))
        st = [binding.f0_stats_rule(TRACKS[b, : FRAMES[b]]) for b in range(3)]
        return TRACKS.copy(), np.ones_like(TRACKS), {k: np.array([s[k] for s in st]) for k in binding.F0_STATS.names}


def _tts(eng):
    return TextToSpeech(eng, None, {"ae": {"sample_rate": SR, "base_chunk_size": 512}, "ttl": {"chunk_compress_factor": 6, "latent_dim": 24}})


def test_tts_pitch_report():
    eng = FakeEngine()
    tts = _tts(eng)
    rep = tts.pitch_report()
    assert set(rep) == STAT_KEYS | {"f0", "ap"} and rep["f0"].shape == (3, 4)
    assert list(rep["frames"]) == [4, 2, 3] and list(rep["voiced"]) == [2, 2, 0]
    assert list(rep["median_hz"]) == [100.0, 200.0, 0.0] and list(rep["max_hz"]) == [110.0, 210.0, 0.0] and rep["mean_hz"][2] == 0.0
    assert abs(rep["mean_hz"][0] - np.sqrt(100.0 * 110.0)) < 1e-4
    # programmes: the member rows' frames pooled on the host
    rep = tts.pitch_report(rows=[2, 1])
    assert set(rep) == STAT_KEYS and all(v.shape == (2,) for v in rep.values())
    assert list(rep["frames"]) == [6, 3] and list(rep["voiced"]) == [4, 0]
    assert rep["median_hz"][0] == 110.0 and rep["min_hz"][0] == 100.0 and rep["max_hz"][0] == 210.0 and rep["median_hz"][1] == 0.0
    assert abs(rep["mean_hz"][0] - (100.0 * 110.0 * 200.0 * 210.0) ** 0.25) < 1e-3
    for bad in ([2, 2], [3, 0], [1]):
        with pytest.raises(ValueError):
            tts.pitch_report(rows=bad)
    # a call's settings are in force for the report and the instance's afterwards; the parameters reach the engine
    del eng.calls[:]
    tts.pitch_report(params={"fmax_hz": 400.0}, output_rate=16000)
    assert eng.calls == [("rate", 16000), ("f0", {"fmax_hz": 400.0}), ("rate", 0)]
    with pytest.raises(TypeError):
        tts.pitch_report(volume=3)
    with tts.exclusive():  # re-entrant: the method takes the same lock
        assert set(tts.pitch_report(rows=[3])) == STAT_KEYS


def test_cli_flag_is_parsed():
    p = subprocess.run([CLI, "--synthetic", "--pitch-report", "--gpus", "2", "--n-test", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--pitch-report needs the batch on one device" in p.stderr, p.stdout + p.stderr


class FakeTTS:
    """Each utterance -> a constant wave of 0.01 s per character; joined_batch and pitch_report as TextToSpeech has them."""
    sample_rate = SR

    def __init__(self):
        self.calls = []

    def _one(self, text):
        dur = np.float32(0.01 * max(len(text), 1))
        n = (int(SR * dur) + 3071) // 3072 * 3072
        return np.full(n, 0.25, np.float32), dur

    def joined_batch(self, texts, langs, style, total_step, speed, rows=None, silence_duration=0.3, loudness_scope="chunk", trim_chunks=False, **out):
        self.calls.append(("joined", list(rows), dict(out)))
        waves, durs, o = [], [], 0
        for g, k in enumerate(rows):
            ws, ds = zip(*[self._one(t) for t in texts[o:o + k]])
            w, d = service.join_chunks(list(ws), list(ds), silence_duration[g], SR)
            waves.append(w)
            durs.append(d)
            o += k
        return waves, np.array(durs, np.float32)

    def batch(self, texts, langs, style, total_step, speed=1.05, **out):
        self.calls.append(("batch", list(texts), dict(out)))
        ws, ds = zip(*[self._one(t) for t in texts])
        wav = np.zeros((len(ws), max(len(w) for w in ws)), np.float32)
        for i, w in enumerate(ws):
            wav[i, : len(w)] = w
        return wav, np.array(ds, np.float32)

    def pitch_report(self, rows=None, params=None, **out):
        self.calls.append(("pitch", None if rows is None else list(rows), dict(out)))
        n = 1 if rows is None else len(rows)
        vals = {"frames": 80, "voiced": 60, "median_hz": 123.4567, "mean_hz": 125.0, "min_hz": 98.5, "max_hz": 201.25}
        rep = {k: np.full(n, v, np.int32 if k in ("frames", "voiced") else np.float32) for k, v in vals.items()}
        if rows is None:
            rep.update(f0=np.zeros((n, 80), np.float32), ap=np.ones((n, 80), np.float32))
        return rep


class PlainTTS(FakeTTS):
    """A synthesizer without the report (the stand-ins of the other tests)."""
    pitch_report = None


def _styles(paths):
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


def _client(tts):
    from fastapi.testclient import TestClient
    return TestClient(service.create_app(tts, max_batch=8, max_wait_ms=5.0, style_loader=_styles))


HEADERS = ("x-pitch-median-hz", "x-pitch-min-hz", "x-pitch-max-hz", "x-pitch-voiced")


def test_service_headers():
    tts = FakeTTS()
    body = {"text": "Hello there, this is a test.", "voice_style": "M1"}
    with _client(tts) as c:
        plain = c.post("/tts", json=body)
        assert plain.status_code == 200 and not any(h in plain.headers for h in HEADERS)
        assert [k[0] for k in tts.calls] == ["joined"]  # absent: today's calls and today's response
        same = c.post("/tts", json=dict(body, pitch_report=False))
        assert same.status_code == 200 and same.content == plain.content and dict(same.headers) == dict(plain.headers)
        r = c.post("/tts", json=dict(body, pitch_report=True, sample_rate=16000))
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
        assert [r.headers[h] for h in HEADERS] == ["123.457", "98.500", "201.250", "0.750"]
        kind, rows, out = tts.calls[-1]
        assert kind == "pitch" and rows == [1] and out == tts.calls[-2][2] == {"output_rate": 16000}
        quiet = c.post("/tts", json=dict(body, sample_rate=16000))  # the audio does not depend on the field
        assert quiet.content == r.content and not any(h in quiet.headers for h in HEADERS)
        # batch mode: one utterance carries the headers, several (a zip) do not
        r = c.post("/tts", json={"text": ["one text"], "lang": ["en"], "voice_style": ["M1"], "batch": True, "pitch_report": True})
        assert r.status_code == 200 and r.headers["x-pitch-median-hz"] == "123.457" and r.headers["x-pitch-voiced"] == "0.750"
        assert tts.calls[-1] == ("pitch", None, {})
        n = len(tts.calls)
        r = c.post("/tts", json={"text": ["a b", "c d e"], "lang": ["en", "en"], "voice_style": ["M1", "M1"], "batch": True, "pitch_report": True})
        assert r.status_code == 200 and r.headers["content-type"] == "application/zip" and not any(h in r.headers for h in HEADERS)
        assert [k[0] for k in tts.calls[n:]] == ["batch"]
    with _client(PlainTTS()) as c:  # a synthesizer without the report sends no headers
        r = c.post("/tts", json=dict(body, pitch_report=True))
        assert r.status_code == 200 and not any(h in r.headers for h in HEADERS)


def test_report_is_no_part_of_the_batch_key():
    tts = FakeTTS()
    b = service.DynamicBatcher(tts, max_batch=8, max_wait_ms=200.0)
    out = {}

    def go(i):
        out[i] = b.submit([f"text {i}"], "en", _styles(["x"]), 2, 1.05, silence_duration=0.3, **({"pitch_report": True} if i % 2 else {}))

    th = [threading.Thread(target=go, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    b.close()
    assert sum(b.batches) == 4 and len(b.batches) < 4  # jobs with and without the report shared a batch
    for i in range(4):
        assert len(out[i]) == (3 if i % 2 else 2)
        if i % 2:
            assert set(out[i][2]) == STAT_KEYS and out[i][2]["median_hz"] == np.float32(123.4567) and isinstance(out[i][2]["max_hz"], float)
    assert "pitch_report" not in service.BatchKey._fields
