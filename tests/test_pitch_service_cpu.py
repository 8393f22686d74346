"""Pitch through the hosts without a GPU (include/stn.h "pitch"): OutputSettings.pitch, the service's batch key
and request field with a stand-in synthesizer (the pattern of tests/test_service_cpu.py), the X-Pitch-Cents header."""
import dataclasses
import threading

import numpy as np
import pytest

from supertonic_amd import binding, service
from supertonic_amd.output import OutputSettings
from supertonic_amd.tts import Style

SR = 44100


class FakeTTS:
    """Each utterance -> a constant wave, 0.01 s per character; the pitch every call came with is recorded"""
    sample_rate = SR

    def __init__(self, settings=None):
        self.calls = []
        if settings is not None:
            self.settings = settings

    def _one(self, text):
        dur = np.float32(0.01 * max(len(text), 1))
        return np.full((int(SR * dur) + 3071) // 3072 * 3072, 0.25, np.float32), dur

    def solo_batch(self, texts, langs, style, total_step, speed, pitch=None, **_):
        self.calls.append((tuple(texts), pitch))
        ws, ds = zip(*[self._one(t) for t in texts])
        return list(ws), np.array(ds, np.float32)

    def batch(self, texts, langs, style, total_step, speed=1.05, pitch=None, **_):
        self.calls.append((tuple(texts), pitch))
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


def test_output_settings_pitch():
    P = OutputSettings.parse
    assert P().pitch is None and P(pitch=None).pitch is None and P(pitch=False).pitch is False and P(pitch=0).pitch is False
    assert P(pitch=2).pitch == 2.0 and P(pitch=-3.5).pitch == -3.5 and isinstance(P(pitch=2).pitch, float)
    assert P(pitch=2) == P(pitch=2.0) and hash(P(pitch=2)) == hash(P(pitch=2.0)) and P(pitch=2) != P(pitch=-2) and P(pitch=2) != P()
    assert P(pitch=2) != P(pitch=2, loudness=-16) and "pitch=2.0" in repr(P(pitch=2))
    for bad in (12.01, -13, float("nan"), float("inf"), "high", True):
        with pytest.raises(ValueError):
            P(pitch=bad)
    assert P(pitch=2).kwargs() == {"pitch": 2.0} and P(**P(pitch=-1).kwargs()) == P(pitch=-1)
    assert P(pitch=False).over(P(pitch=2)).pitch is False and P().over(P(pitch=2)).pitch == 2.0
    on = P(pitch=2, loudness=-16)
    assert on.replace(loudness=False).pitch == 2.0 and on.replace(pitch=False).loudness == (-16.0, -1.0)
    # added the way dither was: no dataclass field, OFF and ALL_OFF as they were, positional construction unchanged, decided() decides it
    assert "pitch" not in [f.name for f in dataclasses.fields(OutputSettings)]
    assert OutputSettings.OFF == OutputSettings(0, (), False, False, False, False, "sample") and OutputSettings.OFF.pitch is None
    assert OutputSettings.ALL_OFF.pitch is None and P().decided().pitch is False and P(pitch=3).decided().pitch == 3.0
    assert P().decided() == OutputSettings.ALL_OFF.replace(dither=False)  # (unset and off are both no shift: they compare equal)
    with pytest.raises(TypeError):
        OutputSettings(pitch=2)


def test_output_settings_apply_pitch_first_and_restore():
    e = _Engine()
    P = OutputSettings.parse
    P(output_rate=16000, loudness=-16, pitch=3, dither="tpdf").apply(e)
    assert [c[0] for c in e.calls] == ["set_pitch", "set_output_rate", "set_loudness", "set_dither"] and e.calls[0] == ("set_pitch", (3.0,))
    e.calls.clear()
    P(pitch=0).apply(e)
    assert e.calls == [("set_pitch", (None,))]
    e.calls.clear()
    P().apply(e)
    assert e.calls == []
    base = P().decided()
    with P(pitch=-2).applied(e, base) as now:
        assert now.pitch == -2.0 and e.calls == [("set_pitch", (-2.0,))]
    assert e.calls[-1] == ("set_pitch", (None,)) and len(e.calls) == 2  # a per-call pitch is put back to off
    base = P(pitch=5).decided()
    e.calls.clear()
    with P(pitch=False).applied(e, base):
        pass
    assert e.calls == [("set_pitch", (None,)), ("set_pitch", (5.0,))]


def test_service_key():
    key = lambda **kw: service.batch_key(44100, 5, 1.05, **kw)
    assert key().settings.pitch is None and key(pitch=0).settings.pitch is False and key(pitch=2).settings.pitch == 2.0
    assert key(pitch=2) == key(pitch=2.0) and hash(key(pitch=2)) == hash(key(pitch=2.0))
    assert key(pitch=2) != key() and key(pitch=2) != key(pitch=-2) and key(pitch=2) != key(pitch=2.5) and key(pitch=2, loudness=-16.0) != key(loudness=-16.0)
    assert key(pitch=-3).settings.kwargs() == {"pitch": -3.0} and key(pitch=0).settings.kwargs() == {"pitch": False} and key().settings.kwargs() == {}
    # unset is the server's own pitch, 0 is none: never one batch, though OutputSettings compares the two equal
    assert key() != key(pitch=0) and key(loudness=-16.0) != key(loudness=-16.0, pitch=0) and key(pitch=0) == key(pitch=0.0) == key(pitch=False)
    assert key().pitch_set is False and key(pitch=0).pitch_set is True and key(pitch=2).pitch_set is True
    for bad in (12.5, -12.01, float("nan")):
        with pytest.raises(ValueError) as ei:
            key(pitch=bad)
        assert str(ei.value) == binding.pitch_error(bad)


def test_service_field_header_and_key_separation():
    from fastapi.testclient import TestClient
    tts = FakeTTS()
    app = service.create_app(tts, max_batch=8, max_wait_ms=100.0, style_loader=_styles)
    with TestClient(app) as c:
        for bad in (12.5, -13):
            r = c.post("/tts", json={"text": "hello there", "pitch": bad})
            assert r.status_code == 400 and r.json()["detail"] == binding.pitch_error(bad), r.text
        assert c.post("/tts", json={"text": "hello there", "pitch": "high"}).status_code == 422 and tts.calls == []
        r = c.post("/tts", json={"text": "hello there", "pitch": 2})
        assert r.status_code == 200 and tts.calls[-1] == (("hello there",), 2.0)
        assert r.headers["x-pitch-cents"] == f"{binding.pitch_cents(2):.3f}" and abs(float(r.headers["x-pitch-cents"]) - 200.0) <= 1.36
        r = c.post("/tts", json={"text": "hello there", "pitch": 0})
        assert r.status_code == 200 and tts.calls[-1][1] is False and r.headers["x-pitch-cents"] == "0.000"
        r = c.post("/tts", json={"text": "hello there"})
        assert r.status_code == 200 and tts.calls[-1][1] is None and r.headers["x-pitch-cents"] == "0.000"
        r = c.post("/tts", json={"text": ["ab", "abcd"], "lang": ["en", "en"], "voice_style": ["x", "y"], "batch": True, "pitch": -5})
        assert r.status_code == 200 and tts.calls[-1] == (("ab", "abcd"), -5.0)
        # requests of different pitch never share a batch
        tts.calls.clear()
        jobs = {"aaa": 2, "bbbb": 2, "ccccc": -2, "dddddd": None}
        th = [threading.Thread(target=lambda t=t, p=p: c.post("/tts", json={"text": t} if p is None else {"text": t, "pitch": p})) for t, p in jobs.items()]
        [t.start() for t in th]
        [t.join() for t in th]
        assert sorted(t for texts, _ in tts.calls for t in texts) == sorted(jobs)
        for texts, pitch in tts.calls:
            assert {jobs[t] for t in texts} == {pitch}, tts.calls
    # a server whose own setting shifts: the header of a request that names none carries the server's, and such a request and one that
    # says 0 are served in separate batches, each with what it asked for
    tts = FakeTTS(OutputSettings.parse(pitch=-1).decided())
    with TestClient(service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=_styles)) as c:
        r = c.post("/tts", json={"text": "hello there"})
        assert r.status_code == 200 and r.headers["x-pitch-cents"] == f"{binding.pitch_cents(-1):.3f}"
    tts = FakeTTS(OutputSettings.parse(pitch=-1).decided())
    with TestClient(service.create_app(tts, max_batch=8, max_wait_ms=100.0, style_loader=_styles)) as c:
        out = {}
        jobs = {"aaa": None, "bbbb": 0, "ccccc": None, "dddddd": 0}
        th = [threading.Thread(target=lambda t=t, p=p: out.__setitem__(t, c.post("/tts", json={"text": t} if p is None else {"text": t, "pitch": p})))
              for t, p in jobs.items()]
        [t.start() for t in th]
        [t.join() for t in th]
        assert sorted(t for texts, _ in tts.calls for t in texts) == sorted(jobs)
        for texts, pitch in tts.calls:  # (unset reaches the synthesizer as None, 0 as False)
            assert {jobs[t] for t in texts} in ({None}, {0}) and pitch is (None if jobs[texts[0]] is None else False), tts.calls
        for t, p in jobs.items():
            assert out[t].status_code == 200 and out[t].headers["x-pitch-cents"] == ("0.000" if p == 0 else f"{binding.pitch_cents(-1):.3f}")
