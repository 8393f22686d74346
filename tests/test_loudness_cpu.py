"""Loudness normalization without a GPU: the K-weighting design the engine exposes (stn_kweighting_filter) against BS.1770-4's
published 48 kHz table and against this file's own float64 derivation at the other rates, the float64 reference itself on the standard's
calibration tones, and the service's `loudness` / `peak_ceiling` fields with a stand-in synthesizer (as tests/test_resample_cpu.py)."""
import math
import threading

import numpy as np
import pytest

from supertonic_amd import binding, service
from supertonic_amd.tts import Style
from loudness_ref import integrated_loudness, kweighting

SR = 44100


def test_kweighting_matches_the_published_48k_table():
    sb, sa, hb, ha = binding.kweighting_filter(48000)
    assert np.abs(sb - [1.53512485958697, -2.69169618940638, 1.19839281085285]).max() <= 1e-12
    assert np.abs(sa - [1.0, -1.69065929318241, 0.73248077421585]).max() <= 1e-12
    assert np.array_equal(hb, [1.0, -2.0, 1.0])
    assert np.abs(ha - [1.0, -1.99004745483398, 0.99007225036621]).max() <= 1e-12


@pytest.mark.parametrize("hz", [8000, 11025, 16000, 22050, 44100, 96000, 192000])
def test_kweighting_at_other_rates_equals_the_float64_derivation(hz):
    got = binding.kweighting_filter(hz)
    for g, r in zip(got, kweighting(hz)):
        assert np.abs(g - r).max() <= 1e-12, (hz, g, r)


def test_kweighting_refuses_rates_out_of_range():
    for bad in (7999, 192001, 0, -48000):
        with pytest.raises(binding.StnError):
            binding.kweighting_filter(bad)


def test_reference_reads_the_calibration_tones():
    """BS.1770-4: a 997 Hz sine at 0 dBFS peak reads -3.01 LKFS; 20 dB down reads -23.01."""
    n = np.arange(10 * 48000)
    tone = np.sin(2 * np.pi * 997 * n / 48000)
    assert abs(integrated_loudness(tone, 48000) - (-3.01)) <= 0.01
    assert abs(integrated_loudness(0.1 * tone, 48000) - (-23.01)) <= 0.01


def test_reference_gating_edges():
    hz = 16000
    assert integrated_loudness(np.zeros(hz * 2), hz) == -math.inf  # every block below the absolute gate
    assert integrated_loudness(np.ones(4 * 1600 - 1), hz) == -math.inf  # shorter than one block
    # a loud second and a near-silent second: the relative gate drops the quiet blocks (ungated, the mean would be ~3 dB lower;
    # the three blocks that straddle the edge still count)
    rng = np.random.default_rng(0)
    loud = rng.standard_normal(hz) * 0.1
    both = np.concatenate([loud, loud * 1e-3])
    assert abs(integrated_loudness(both, hz) - integrated_loudness(loud, hz)) < 1.0


# ---- the service (stand-in synthesizer) -----------------------------------------------------------------------------------------
class FakeTTS:
    """Each utterance -> a constant wave of 0.01 s per character; records the loudness each engine call asked for."""
    sample_rate = SR

    def __init__(self):
        self.calls = []

    def _one(self, text):
        dur = np.float32(0.01 * max(len(text), 1))
        n = (int(SR * dur) + 3071) // 3072 * 3072
        return np.full(n, min(len(text), 99) / 100.0, np.float32), dur

    def solo_batch(self, texts, langs, style, total_step, speed, output_rate=None, loudness=None):
        self.calls.append((loudness, list(texts)))
        ws, ds = zip(*[self._one(t) for t in texts])
        return list(ws), np.array(ds, np.float32)

    def batch(self, texts, langs, style, total_step, speed=1.05, output_rate=None, loudness=None):
        self.calls.append((loudness, list(texts)))
        ws, ds = zip(*[self._one(t) for t in texts])
        wav = np.zeros((len(ws), max(len(w) for w in ws)), np.float32)
        for i, w in enumerate(ws):
            wav[i, : len(w)] = w
        return wav, np.array(ds, np.float32)


def _styles(paths):
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


@pytest.fixture()
def client():
    from fastapi.testclient import TestClient
    tts = FakeTTS()
    app = service.create_app(tts, max_batch=8, max_wait_ms=5.0, style_loader=_styles)
    with TestClient(app) as c:
        c.tts = tts
        yield c


def test_service_loudness_fields(client):
    body = {"text": "Hello there, this is a test.", "voice_style": "M1"}
    assert client.post("/tts", json=body).status_code == 200
    assert client.tts.calls[-1][0] is None  # absent: today's engine call
    assert client.post("/tts", json=dict(body, loudness=None)).status_code == 200 and client.tts.calls[-1][0] is None
    r = client.post("/tts", json=dict(body, loudness=-16))
    assert r.status_code == 200 and client.tts.calls[-1][0] == (-16.0, -1.0)
    r = client.post("/tts", json=dict(body, loudness=-23, peak_ceiling=-2))
    assert r.status_code == 200 and client.tts.calls[-1][0] == (-23.0, -2.0)
    rb = client.post("/tts", json={"text": ["ab", "cde"], "lang": ["en", "en"], "voice_style": ["M1", "M1"], "batch": True, "loudness": -20})
    assert rb.status_code == 200 and client.tts.calls[-1][0] == (-20.0, -1.0)
    n = len(client.tts.calls)
    for bad in ({"loudness": -61}, {"loudness": 0.5}, {"loudness": -16, "peak_ceiling": 1}, {"loudness": -16, "peak_ceiling": -31}):
        r = client.post("/tts", json=dict(body, **bad))
        assert r.status_code == 422, bad
    assert len(client.tts.calls) == n  # refused before the engine


def test_batcher_never_mixes_loudness_settings():
    tts = FakeTTS()
    b = service.DynamicBatcher(tts, max_batch=8, max_wait_ms=50.0)
    out = {}
    settings = [(None, -1.0), (-16.0, -1.0), (None, -1.0), (-16.0, -1.0), (-23.0, -1.0), (-16.0, -3.0)]

    def go(i, lo, ceil):
        out[i] = b.submit([f"text {i}"], "en", _styles(["x"]), 2, 1.05, None, lo, ceil)

    th = [threading.Thread(target=go, args=(i, lo, c)) for i, (lo, c) in enumerate(settings)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    b.close()
    assert len(out) == 6 and sum(len(t) for _, t in tts.calls) == 6
    for lo, texts in tts.calls:  # every engine batch holds jobs of one setting only, and asks for that setting
        for t in texts:
            want_lo, want_c = settings[int(t.split()[1])]
            assert lo == (None if want_lo is None else (want_lo, want_c)), (lo, texts)
