"""The output-rate resampler's filter design and the service's `sample_rate` field, without a GPU: stn_resample_filter (host only) for
every listed rate against the spec (phase gains, passband ripple, stopband rejection from a numpy FFT of the interleaved prototype,
scipy's Kaiser design when scipy is there), the refused rates, and the HTTP schema with a stand-in synthesizer."""
import io
import math
import struct

import numpy as np
import pytest

from supertonic_amd import binding, service
from supertonic_amd.tts import Style

SR = 44100
RATES = binding.SUPPORTED_OUTPUT_RATES


def _pq(in_hz, out_hz):
    g = math.gcd(in_hz, out_hz)
    return out_hz // g, in_hz // g


def _prototype(taps):
    """the filter at the common rate in*P: tap j of phase p sits (p - (j - off) * P) fine samples from the output instant"""
    P, T = taps.shape
    h = np.zeros(P * T)
    for j in range(T):
        h[np.arange(P) + (T - 1 - j) * P] = taps[:, j]
    return h


@pytest.mark.parametrize("out_hz", RATES)
def test_phases_taps_and_unit_gain(out_hz):
    taps = binding.resample_filter(SR, out_hz)
    P, Q = _pq(SR, out_hz)
    if out_hz == SR:
        assert taps.shape == (1, 8) and taps[0, 3] == 1.0 and np.count_nonzero(taps) == 1
        return
    assert taps.shape[0] == P and taps.shape[1] % 8 == 0 and taps.dtype == np.float32
    assert np.all(np.abs(taps.astype(np.float64).sum(axis=1) - 1.0) <= 1e-6)  # a constant comes back as itself
    # symmetric (linear phase): phase p and phase P - p are mirror images around the centre tap
    T = taps.shape[1]
    h = _prototype(taps.astype(np.float64))
    assert np.allclose(h[1:], h[1:][::-1], atol=1e-7)
    print(f"44.1 kHz -> {out_hz} Hz: P/Q = {P}/{Q}, {T} taps per phase, table {P * T * 4 / 1024:.1f} KiB")


@pytest.mark.parametrize("out_hz", [r for r in RATES if r != SR])
def test_prototype_response_meets_the_spec(out_hz):
    taps = binding.resample_filter(SR, out_hz).astype(np.float64)
    P, _ = _pq(SR, out_hz)
    h = _prototype(taps)
    nfft = 1 << int(np.ceil(np.log2(len(h) * 16)))
    H = np.abs(np.fft.rfft(h, nfft)) / P
    f = np.arange(len(H)) * (SR * P) / nfft
    fmin = min(SR, out_hz)
    pb = 20 * np.log10(H[f <= 0.85 * fmin / 2])
    sb = 20 * np.log10(H[f >= fmin / 2].max())
    assert pb.max() <= 0.05 and pb.min() >= -0.05, (pb.min(), pb.max())
    assert sb <= -80, sb


@pytest.mark.parametrize("out_hz", [16000, 48000])
def test_against_scipy_kaiser_design(out_hz):
    signal = pytest.importorskip("scipy.signal")
    taps = binding.resample_filter(SR, out_hz).astype(np.float64)
    P, _ = _pq(SR, out_hz)
    h = _prototype(taps)
    fmin = min(SR, out_hz)
    fc = (0.85 * fmin / 2 + fmin / 2) / 2
    n = len(h) + 1  # odd length centred on the same instant; the last sample of ours is the window's (zero) edge
    ref = signal.firwin(n, fc, window=("kaiser", 0.1102 * (90.0 - 8.7)), fs=SR * P, scale=False)[:-1] * P
    # scipy normalises the whole prototype, we normalise each phase: the shapes agree to the stopband level
    assert np.abs(h - ref).max() <= 1e-3 * np.abs(ref).max()


def test_refused_and_accepted_rates():
    for bad in (44101, 7999, 192001, -16000, 0):
        with pytest.raises(binding.StnError):
            binding.resample_filter(SR, bad)
        assert binding.resample_error(SR, bad)
    assert "P must be <= 640" in binding.resample_error(SR, 44101)
    for ok in (8000, 12000, 192000, 8001):  # any rate in range whose reduced P is <= 640
        assert binding.resample_error(SR, ok) == ""


# ---- the service's sample_rate field (stand-in synthesizer, as tests/test_service_cpu.py) ----------------------------------------
class FakeTTS:
    """Each utterance -> a constant wave of 0.01 s per character at the rate asked for."""
    sample_rate = SR

    def __init__(self):
        self.rates, self.calls = [], []

    def _one(self, text, rate):
        dur = np.float32(0.01 * max(len(text), 1))
        n = -(-((int(SR * dur) + 3071) // 3072 * 3072) * _pq(SR, rate)[0] // _pq(SR, rate)[1])
        return np.full(n, min(len(text), 99) / 100.0, np.float32), dur

    def solo_batch(self, texts, langs, style, total_step, speed, output_rate=None):
        self.rates.append(output_rate)
        self.calls.append((output_rate, list(texts)))
        ws, ds = zip(*[self._one(t, output_rate or SR) for t in texts])
        return list(ws), np.array(ds, np.float32)

    def batch(self, texts, langs, style, total_step, speed=1.05, output_rate=None):
        self.rates.append(output_rate)
        ws, ds = zip(*[self._one(t, output_rate or SR) for t in texts])
        wav = np.zeros((len(ws), max(len(w) for w in ws)), np.float32)
        for i, w in enumerate(ws):
            wav[i, : len(w)] = w
        return wav, np.array(ds, np.float32)


def _styles(paths):
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


def _wav_rate(b):
    assert b[:4] == b"RIFF"
    return struct.unpack("<I", b[24:28])[0], struct.unpack("<I", b[40:44])[0] // 2


@pytest.fixture()
def client():
    from fastapi.testclient import TestClient
    tts = FakeTTS()
    app = service.create_app(tts, max_batch=8, max_wait_ms=5.0, style_loader=_styles)
    with TestClient(app) as c:
        c.tts = tts
        yield c


def test_service_sample_rate(client):
    body = {"text": "Hello there, this is a test.", "voice_style": "M1"}
    r0 = client.post("/tts", json=body)
    r_none = client.post("/tts", json=dict(body, sample_rate=None))
    assert r0.status_code == r_none.status_code == 200 and r0.content == r_none.content  # absent / null: today's response
    sr, n = _wav_rate(r0.content)
    assert sr == SR and client.tts.rates[:2] == [None, None]  # and today's engine call
    r16 = client.post("/tts", json=dict(body, sample_rate=16000))
    sr16, n16 = _wav_rate(r16.content)
    assert r16.status_code == 200 and sr16 == 16000 and client.tts.rates[-1] == 16000
    assert n16 == int(16000 * np.float32(0.01 * len(body["text"])))  # _slice_audio at the output rate
    rb = client.post("/tts", json={"text": ["ab", "cde"], "lang": ["en", "en"], "voice_style": ["M1", "M1"], "batch": True, "sample_rate": 24000})
    assert rb.status_code == 200 and rb.headers["content-type"] == "application/zip"
    import zipfile
    with zipfile.ZipFile(io.BytesIO(rb.content)) as zf:
        assert all(_wav_rate(zf.read(name))[0] == 24000 for name in zf.namelist())
    bad = client.post("/tts", json=dict(body, sample_rate=12345))
    assert bad.status_code == 400 and "16000" in bad.json()["detail"] and "12345" in bad.json()["detail"]


def test_batcher_never_mixes_rates():
    tts = FakeTTS()
    b = service.DynamicBatcher(tts, max_batch=8, max_wait_ms=50.0)
    import threading
    out = {}

    def go(i, rate):
        out[i] = b.submit([f"text {i}"], "en", _styles(["x"]), 2, 1.05, rate)

    rates = [None, 16000, None, 16000, 48000]
    th = [threading.Thread(target=go, args=(i, r)) for i, r in enumerate(rates)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    b.close()
    assert len(out) == 5 and sum(len(t) for _, t in tts.calls) == 5
    for rate, texts in tts.calls:  # every engine batch holds jobs of one rate only
        assert all(rates[int(t.split()[1])] == rate for t in texts), (rate, texts)
    assert all(len(out[i][0][0]) == tts._one(f"text {i}", rates[i] or SR)[0].size for i in range(5))
