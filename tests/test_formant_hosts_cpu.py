"""The pitch mode through the hosts without a GPU (include/stn.h "formant"): OutputSettings.pitch_mode, the
service's batch key and request field with a stand-in synthesizer (the pattern of tests/test_pitch_service_cpu.py), and the command
line's refusal."""
import dataclasses
import os
import subprocess
import threading

import numpy as np
import pytest

from supertonic_amd import binding, service
from supertonic_amd.output import OutputSettings
from supertonic_amd.tts import Style

SR = 44100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")


class FakeTTS:
    """Each utterance -> a constant wave, 0.01 s per character; the pitch mode every call came with is recorded"""
    sample_rate = SR

    def __init__(self, settings=None):
        self.calls = []
        if settings is not None:
            self.settings = settings

    def _one(self, text):
        dur = np.float32(0.01 * max(len(text), 1))
        return np.full((int(SR * dur) + 3071) // 3072 * 3072, 0.25, np.float32), dur

    def solo_batch(self, texts, langs, style, total_step, speed, pitch_mode=None, **_):
        self.calls.append((tuple(texts), pitch_mode))
        ws, ds = zip(*[self._one(t) for t in texts])
        return list(ws), np.array(ds, np.float32)

    def batch(self, texts, langs, style, total_step, speed=1.05, pitch_mode=None, **_):
        self.calls.append((tuple(texts), pitch_mode))
        ws, ds = zip(*[self._one(t) for t in texts])
        W = min(len(w) for w in ws)
        return np.stack([w[:W] for w in ws]), np.array(ds, np.float32)


def _styles(paths):
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


class _Engine:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("set_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append((name, a))


def test_names():
    assert binding.pitch_mode_id(None) == binding.PITCH_RESAMPLE == 0 and binding.pitch_mode_id("resample") == 0
    assert binding.pitch_mode_id("formant") == binding.PITCH_FORMANT == 1 and binding.pitch_mode_name(None) == "resample"
    for bad in ("Formant", "lpc", 1, True, ""):
        with pytest.raises(ValueError, match="pitch_mode: 'resample' or 'formant'"):
            binding.pitch_mode_id(bad)


def test_output_settings_with_and_without_the_attribute():
    P = OutputSettings.parse
    assert P().pitch_mode is None and P(pitch_mode=None).pitch_mode is None
    assert P(pitch_mode="formant").pitch_mode == "formant" and P(pitch_mode="resample").pitch_mode == "resample"
    assert P(pitch_mode="resample") == P() and hash(P(pitch_mode="resample")) == hash(P())  # unset and "resample" compare equal
    assert P(pitch_mode="formant") != P() and P(pitch=2, pitch_mode="formant") != P(pitch=2) and "pitch_mode='formant'" in repr(P(pitch_mode="formant"))
    for bad in ("lpc", 1, True):
        with pytest.raises(ValueError, match="pitch_mode"):
            P(pitch_mode=bad)
    assert P(pitch_mode="formant").kwargs() == {"pitch_mode": "formant"} and P(**P(pitch=-1, pitch_mode="formant").kwargs()) == P(pitch=-1, pitch_mode="formant")
    assert P(pitch_mode="resample").over(P(pitch_mode="formant")).pitch_mode == "resample" and P().over(P(pitch_mode="formant")).pitch_mode == "formant"
    on = P(pitch=2, pitch_mode="formant", loudness=-16)
    assert on.replace(loudness=False).pitch_mode == "formant" and on.replace(pitch_mode="resample").pitch == 2.0
    # added the way dither, pitch and expander were: no dataclass field, OFF and ALL_OFF as they were, positional construction unchanged
    assert "pitch_mode" not in [f.name for f in dataclasses.fields(OutputSettings)]
    assert OutputSettings.OFF == OutputSettings(0, (), False, False, False, False, "sample") and OutputSettings.OFF.pitch_mode is None
    assert OutputSettings.ALL_OFF.pitch_mode is None and P().decided().pitch_mode == "resample" and P(pitch_mode="formant").decided().pitch_mode == "formant"
    assert P().decided() == OutputSettings.ALL_OFF.replace(dither=False)
    with pytest.raises(TypeError):
        OutputSettings(pitch_mode="formant")


def test_output_settings_apply_next_to_pitch_and_restore():
    e = _Engine()
    P = OutputSettings.parse
    P(output_rate=16000, pitch=3, pitch_mode="formant", dither="tpdf").apply(e)
    assert [c[0] for c in e.calls] == ["set_pitch", "set_pitch_mode", "set_output_rate", "set_dither"] and e.calls[1] == ("set_pitch_mode", ("formant",))
    e.calls.clear()
    P(pitch=3).apply(e)
    assert e.calls == [("set_pitch", (3.0,))]  # a value that names no mode sets none
    base = P().decided()
    e.calls.clear()
    with P(pitch_mode="formant").applied(e, base) as now:
        assert now.pitch_mode == "formant" and e.calls == [("set_pitch_mode", ("formant",))]
    assert e.calls[-1] == ("set_pitch_mode", ("resample",)) and len(e.calls) == 2  # a per-call mode is put back


def test_service_key():
    key = lambda **kw: service.batch_key(44100, 5, 1.05, **kw)
    assert key().settings.pitch_mode is None and key(pitch_mode="formant").settings.pitch_mode == "formant"
    assert key(pitch=2, pitch_mode="formant") != key(pitch=2) and key(pitch=2, pitch_mode="formant") != key(pitch=2, pitch_mode="resample")
    assert key(pitch=2, pitch_mode="formant") == key(pitch=2.0, pitch_mode="formant")
    # a request that names none is one that names "resample" where the server's own is "resample", and is not where it is "formant"
    assert key(pitch=2) == key(pitch=2, pitch_mode="resample") and hash(key(pitch=2)) == hash(key(pitch=2, pitch_mode="resample"))
    assert key(pitch=2, own_pitch_mode="formant") != key(pitch=2, pitch_mode="resample", own_pitch_mode="formant")
    assert key(pitch=2, own_pitch_mode="formant").pitch_mode == "formant" and key(pitch=2, own_pitch_mode=None).pitch_mode == "resample"
    assert key(pitch_mode="formant").settings.kwargs() == {"pitch_mode": "formant"} and key().settings.kwargs() == {}
    assert service.BatchKey._fields[-1] == "pitch_mode" and service.BatchKey._fields[:8] == (
        "total_step", "speed", "encoding", "loudness_scope", "trim_chunks", "settings", "pitch_set", "expander_set")
    with pytest.raises(ValueError) as ei:
        key(pitch_mode="lpc")
    assert str(ei.value) == "pitch_mode: 'resample' or 'formant', not 'lpc'"


def test_service_field_and_key_separation():
    from fastapi.testclient import TestClient
    tts = FakeTTS()
    with TestClient(service.create_app(tts, max_batch=8, max_wait_ms=100.0, style_loader=_styles)) as c:
        r = c.post("/tts", json={"text": "hello there", "pitch": 2, "pitch_mode": "lpc"})
        assert r.status_code == 400 and r.json()["detail"] == "pitch_mode: 'resample' or 'formant', not 'lpc'" and tts.calls == []
        r = c.post("/tts", json={"text": "hello there", "pitch": 2, "pitch_mode": "formant"})
        assert r.status_code == 200 and tts.calls[-1] == (("hello there",), "formant")
        r = c.post("/tts", json={"text": "hello there", "pitch": 2})
        assert r.status_code == 200 and tts.calls[-1] == (("hello there",), None)
        r = c.post("/tts", json={"text": ["ab", "abcd"], "lang": ["en", "en"], "voice_style": ["x", "y"], "batch": True, "pitch": -5, "pitch_mode": "formant"})
        assert r.status_code == 200 and tts.calls[-1] == (("ab", "abcd"), "formant")
        # requests that differ only in the mode never share a batch
        tts.calls.clear()
        jobs = {"aaa": "formant", "bbbb": "formant", "ccccc": "resample", "dddddd": "resample"}
        th = [threading.Thread(target=lambda t=t, m=m: c.post("/tts", json={"text": t, "pitch": 3, "pitch_mode": m})) for t, m in jobs.items()]
        [t.start() for t in th]
        [t.join() for t in th]
        assert sorted(t for texts, _ in tts.calls for t in texts) == sorted(jobs)
        for texts, mode in tts.calls:
            assert {jobs[t] for t in texts} == {mode}, tts.calls
    # a server whose own mode is "formant": a request that names none and one that says "resample" are served apart
    tts = FakeTTS(OutputSettings.parse(pitch=2, pitch_mode="formant").decided())
    with TestClient(service.create_app(tts, max_batch=8, max_wait_ms=100.0, style_loader=_styles)) as c:
        jobs = {"aaa": None, "bbbb": "resample", "ccccc": None, "dddddd": "resample"}
        th = [threading.Thread(target=lambda t=t, m=m: c.post("/tts", json={"text": t} if m is None else {"text": t, "pitch_mode": m})) for t, m in jobs.items()]
        [t.start() for t in th]
        [t.join() for t in th]
        assert sorted(t for texts, _ in tts.calls for t in texts) == sorted(jobs)
        for texts, mode in tts.calls:
            assert {jobs[t] for t in texts} == {mode}, tts.calls


def test_cli_refuses_an_unknown_mode(tmp_path):
    p = subprocess.run([CLI, "--synthetic", "--onnx-dir", "no_assets_here", "--pitch", "2", "--pitch-mode", "lpc"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 1 and "--pitch-mode 'lpc': resample or formant" in p.stderr, p.stderr
