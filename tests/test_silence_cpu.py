"""Silence trimming without a GPU (include/stn.h "silence trimming"): the float64 reference (tests/silence_ref.py)
on hand-made rows, the fade window of the library against the float64 formula, the ranges and messages of the setting at the Python
host and at the service (through a stand-in synthesizer), the batcher's merge key, and the CLI's refusal of a group."""
import os
import subprocess
import threading

import numpy as np
import pytest

from supertonic_amd import binding, service
from supertonic_amd.tts import Style, _trim_setting
import silence_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
HZ = 16000
F = 160


def _row(n, spans, amp=0.5):
    x = np.zeros(n, np.float32)
    for a, b in spans:
        x[a:b] = amp
    return x


def test_reference_rules_on_hand_made_rows():
    assert ref.frame(44100) == 441 and ref.frame(11025) == 110 and ref.frame(8000) == 80 and ref.samples(HZ, 20.0) == 320
    assert ref.samples(44100, 5.0) == 221 and ref.samples(8000, 0.05) == 0  # int(x + 0.5)
    assert [ref.frame(hz) for hz in (88200, 96000, 176400, 192000)] == [882, 960, 1764, 1920]
    # an all-zero row and a row below the -70 dBFS floor: no speech, nothing is cut
    assert ref.edges(np.zeros(4000, np.float32), 4000, HZ, 40.0, 20.0)[:2] == (0, 4000)
    assert ref.edges(np.full(4000, 3e-4, np.float32), 4000, HZ, 40.0, 20.0)[:2] == (0, 4000)  # 9e-8 <= 1e-7
    assert ref.edges(np.full(4000, 4e-4, np.float32), 4000, HZ, 40.0, 20.0)[:2] == (0, 4000)  # above the floor: every frame is active
    # n = 0, and n < F (one short frame)
    assert ref.edges(np.ones(100, np.float32), 0, HZ, 40.0, 20.0)[:2] == (0, 0)
    assert ref.edges(_row(4000, [(20, 60)]), 100, HZ, 40.0, 20.0)[:2] == (0, 100)
    # speech in frames 10 .. 14 of 25: the edges are frame edges widened by the keep
    x = _row(4000, [(10 * F, 15 * F)])
    assert ref.edges(x, 4000, HZ, 40.0, 20.0)[:2] == (10 * F - 320, 15 * F + 320)
    assert ref.edges(x, 4000, HZ, 40.0, 0.0)[:2] == (10 * F, 15 * F)
    # ... which is clamped at both ends; speech from sample 0; speech to the end
    assert ref.edges(x, 4000, HZ, 40.0, 1000.0)[:2] == (0, 4000)
    assert ref.edges(_row(4000, [(0, 3 * F)]), 4000, HZ, 40.0, 20.0)[:2] == (0, 3 * F + 320)
    assert ref.edges(_row(4000, [(20 * F, 4000)]), 3990, HZ, 40.0, 20.0)[:2] == (20 * F - 320, 3990)
    # a partial frame counts by its own mean: 40 samples of speech in a frame of 160 are 6 dB down, active at 40 dB and not at 3
    x = _row(4000, [(10 * F - 40, 15 * F)])
    assert ref.edges(x, 4000, HZ, 40.0, 0.0)[0] == 9 * F and ref.edges(x, 4000, HZ, 3.0, 0.0)[0] == 10 * F
    # a pause inside is never touched, and the samples behind n are never read
    x = _row(4000, [(5 * F, 8 * F), (15 * F, 18 * F), (3900, 4000)])
    s, e, margin = ref.edges(x, 3800, HZ, 40.0, 0.0)
    assert (s, e) == (5 * F, 18 * F) and abs(margin - 40.0) < 1e-9  # (every frame is silent or at the maximum: 40 dB from the threshold)
    y, ss, ee, _ = ref.trim_rows(x[None], [3800], HZ, 40.0, 0.0, 0.0)
    assert np.array_equal(y[0, : e - s], x[s:e]) and not y[0, e - s:].any() and not y[0, 3 * F:10 * F].any()
    # the margin: a frame 0.5 dB above a 20 dB threshold
    x = _row(4000, [(10 * F, 11 * F)])
    x[12 * F:13 * F] = 0.5 * 10.0 ** (-19.5 / 20.0)
    s, e, margin = ref.edges(x, 4000, HZ, 20.0, 0.0)
    assert (s, e) == (10 * F, 13 * F) and abs(margin - 0.5) < 1e-3


def test_reference_fade_is_three_float32_multiplies():
    x = np.linspace(-1.0, 1.0, 4000).astype(np.float32)
    w = ref.fade_window(HZ, 5.0)
    assert w.size == 80 and w.dtype == np.float32 and 0.0 < w[0] < w[-1] < 1.0
    seg = ref.trimmed_row(x, 4000, 1000, 3000, HZ, 5.0, gain=0.7)
    g = x[1000:3000] * np.float32(0.7)
    assert np.array_equal(seg[80:-80], g[80:-80])
    assert np.array_equal(seg[:80], g[:80] * w) and np.array_equal(seg[-80:], g[-80:] * w[::-1])
    # an edge that was not cut keeps its samples bit for bit
    assert np.array_equal(ref.trimmed_row(x, 3000, 0, 3000, HZ, 5.0), x[:3000])
    # shorter than the fades: both apply to every sample, in then out
    seg = ref.trimmed_row(x, 4000, 1000, 1050, HZ, 5.0)
    assert np.array_equal(seg, (x[1000:1050] * w[:50]) * w[:50][::-1])
    assert ref.trimmed_row(x, 4000, 1000, 1000, HZ, 5.0).size == 0


@pytest.mark.parametrize("hz", [8000, 11025, 16000, 22050, 44100, 48000, 88200, 96000, 176400, 192000])
def test_library_fade_window_is_the_float64_formula_rounded(hz):
    for ms in (0.0, 0.4, 5.0, 12.5, 50.0):
        fd = int(float(np.float32(ms)) * hz / 1000.0 + 0.5)
        want = (0.5 - 0.5 * np.cos(np.pi * (np.arange(fd, dtype=np.float64) + 0.5) / max(fd, 1))).astype(np.float32)
        got = binding.silence_fade_window(hz, ms)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (hz, ms)
    with pytest.raises(binding.StnError):
        binding.silence_fade_window(hz, 50.5)
    with pytest.raises(binding.StnError):
        binding.silence_fade_window(hz, -1.0)


@pytest.mark.parametrize("hz", [88200, 96000, 176400, 192000])
def test_reference_decides_the_gpu_rows_above_48_khz_with_margin(hz):
    """the rows tests/test_gpu_silence.py runs at the rates above 48 kHz (frames of 882 to 1920 samples): the float64 reference decides
    every edge at least 0.01 dB from its threshold, so the kernel's fp32 levels cannot move one"""
    import itertools
    x, n = ref.speech_rows(hz, 6, 2.4, hz)
    for top_db, keep_ms in itertools.product((30.0, 40.0, 50.0), (20.0, 0.0)):
        s, e, margin = ref.batch_edges(x, n, hz, top_db, keep_ms)
        assert margin.min() >= 0.01, (hz, top_db, margin)
        assert s[0] == 0 and e[1] == n[1] and np.all(e > s) and np.any(s > 0) and np.any(e < n)


def test_setting_ranges_and_messages_at_the_python_host():
    assert binding.silence_trim_args(None) == (0, 40.0, 20.0, 5.0)
    assert binding.silence_trim_args(35) == (1, 35.0, 20.0, 5.0) and binding.silence_trim_args((30, 0, 50)) == (1, 30.0, 0.0, 50.0)
    assert _trim_setting(None) is None and _trim_setting(False) is None and _trim_setting(40) == (40.0, 20.0, 5.0)
    for bad, what in ((0.5, "top_db"), (121, "top_db"), ((40, -1, 5), "keep"), ((40, 1001, 5), "keep"), ((40, 20, 51), "fade"), ((40, 20, -0.1), "fade")):
        with pytest.raises(ValueError) as ei:
            _trim_setting(bad)
        assert what in str(ei.value) and "must be in" in str(ei.value)
    for bad in (True, "loud", (40, 20), (40, 20, 5, 1)):
        with pytest.raises(ValueError):
            binding.silence_trim_args(bad)


class FakeTTS:
    """A stand-in synthesizer with solo_batch's surface: constant waves, 0.01 s per character; with trim_silence, a tenth cut off."""
    sample_rate = 44100

    def __init__(self):
        self.calls = []

    def solo_batch(self, texts, langs, style, total_step, speed, trim_silence=None):
        self.calls.append((list(texts), trim_silence))
        ws = [np.full(int(441 * len(t) * (0.9 if trim_silence else 1.0)), 0.25, np.float32) for t in texts]
        return ws, np.array([0.01 * len(t) for t in texts], np.float32)

    def batch(self, texts, langs, style, total_step, speed=1.05, trim_silence=None, lengths=False):
        ws, ds = self.solo_batch(texts, langs, style, total_step, speed, trim_silence)
        wav = np.zeros((len(ws), 441 * max(len(t) for t in texts)), np.float32)
        for i, w in enumerate(ws):
            wav[i, : w.size] = w
        return (wav, ds, np.array([w.size for w in ws], np.int64) if trim_silence else None) if lengths else (wav, ds)


def _styles(paths):
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


def test_batcher_validates_the_setting_and_keys_batches_by_it():
    tts = FakeTTS()
    b = service.DynamicBatcher(tts, max_batch=8, max_wait_ms=300.0)
    for bad in (0.5, 121, (40, 1001, 5), (40, 20, 51)):
        with pytest.raises(ValueError) as ei:
            b.submit(["abc"], "en", _styles(["x"]), 5, 1.05, trim_silence=bad)
        assert "must be in" in str(ei.value)
    assert tts.calls == []  # refused before anything was queued
    out = {}

    def go(i, ts):
        out[i] = b.submit(["text number %d" % i], "en", _styles(["x"]), 5, 1.05, trim_silence=ts)

    th = [threading.Thread(target=go, args=(i, ts)) for i, ts in enumerate((40, 40, None, 30, (40, 20, 0)))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    b.close()
    # two requests that differ only in trim_silence are not merged; like ones are
    assert sorted(len(c[0]) for c in tts.calls) == [1, 1, 1, 2]
    assert sorted(str(c[1]) for c in tts.calls) == sorted(str(v) for v in (None, (30.0, 20.0, 5.0), (40.0, 20.0, 0.0), (40.0, 20.0, 5.0)))
    assert out[0][0][0].size == int(441 * 13 * 0.9) and out[2][0][0].size == 441 * 13


def test_service_fields_are_validated_and_reach_the_synthesizer():
    from fastapi.testclient import TestClient
    tts = FakeTTS()
    app = service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=_styles)
    with TestClient(app) as c:
        for bad in ({"trim_silence": 0.5}, {"trim_silence": 121}, {"trim_silence": 40, "trim_keep_ms": 1001}, {"trim_silence": 40, "trim_keep_ms": -1},
                    {"trim_silence": 40, "trim_fade_ms": 51}):
            assert c.post("/tts", json={"text": "hello", **bad}).status_code == 422, bad
        r = c.post("/tts", json={"text": "hello there", "trim_silence": 40, "trim_keep_ms": 10})
        assert r.status_code == 200 and len(r.content) == 44 + 2 * int(441 * 11 * 0.9)  # the whole trimmed wave, not a duration product
        assert tts.calls[-1] == (["hello there"], (40.0, 10.0, 5.0))
        r = c.post("/tts", json={"text": "hello there"})
        assert r.status_code == 200 and len(r.content) == 44 + 2 * int(44100 * float(np.float32(0.11))) and tts.calls[-1][1] is None
        r = c.post("/tts", json={"text": ["ab", "abcd"], "lang": ["en", "en"], "voice_style": ["x", "y"], "batch": True, "trim_silence": 30})
        assert r.status_code == 200 and tts.calls[-1] == (["ab", "abcd"], (30.0, 20.0, 5.0))


def test_cli_refuses_a_group_with_trimming():
    p = subprocess.run([CLI, "--synthetic", "--gpus", "2", "--trim-silence", "40", "--n-test", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "silence trimming" in p.stderr and "one GPU" in p.stderr, p.stdout + p.stderr
