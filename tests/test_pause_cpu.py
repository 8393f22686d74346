"""The pause limit's rule on the host (stn_pause_plan, csrc/host/pause_plan.cpp; include/stn.h "pause limit")
against the float64 reference tests/pause_ref.py, and the service's schema and merge key with a stand-in synthesizer.  No GPU: the
kernel that computes the same integers on the device is covered by tests/test_gpu_pause.py.

Every case states the number of cuts designed into it and asserts that the reference finds exactly that many."""
import threading

import numpy as np
import pytest

from supertonic_amd import binding
import pause_ref as pz
import silence_ref as ref

HI, LO = 0.04, 1e-8  # an active frame's level and the floor's (-80 dBFS noise): 36 dB on either side of the 40 dB threshold


def _levels(K, active):
    m = np.full(K, LO, np.float64)
    m[list(active)] = HI
    return m


def _check(m, n, hz, max_pause_ms, want_cuts, top_db=40.0, keep_ms=20.0):
    s, e, cuts, margin = pz.plan_levels(m, n, hz, top_db, keep_ms, max_pause_ms)
    assert len(cuts) == want_cuts, (len(cuts), want_cuts)
    assert margin >= pz.MARGIN_DB
    gs, ge, gc, nc = binding.pause_plan(m, n, hz, top_db, keep_ms, max_pause_ms)
    assert (gs, ge, nc) == (s, e, want_cuts), (gs, ge, nc, s, e)
    assert gc.tolist() == [list(c) for c in cuts]
    return s, e, cuts


@pytest.mark.parametrize("hz", [8000, 11025, 16000, 44100, 48000])
def test_a_pause_of_exactly_mp_stays_and_one_frame_more_is_cut(hz):
    F = ref.frame(hz)
    frames = 7
    ms = frames * F * 1000.0 / hz  # Mp = frames * F exactly (asserted)
    Mp = pz.pause_samples(hz, ms)
    assert Mp == frames * F
    K = 40
    n = K * F - 3
    _check(_levels(K, [5, 6, 6 + frames + 1, 30]), n, hz, ms, 1)  # P == Mp untouched; the long one behind it cut
    _check(_levels(K, [5, 6, 6 + frames + 1]), n, hz, ms, 0)  # P == Mp alone: no cut
    s, e, cuts = _check(_levels(K, [5, 6, 6 + frames + 2]), n, hz, ms, 1)  # P == Mp + F
    (lo, hi), = cuts
    assert (7 * F + (Mp - Mp // 2), (8 + frames) * F - Mp // 2) == (lo, hi)
    assert (lo - 7 * F) + ((8 + frames) * F - hi) == Mp  # exactly Mp samples of the pause remain


def test_an_odd_mp_keeps_one_sample_more_on_the_left():
    hz, F = 11025, 110
    Mp = pz.pause_samples(hz, 33.3)
    assert Mp == 367 and Mp % 2 == 1
    s, e, cuts = _check(_levels(50, [2, 20, 21, 40]), 50 * F - 7, hz, 33.3, 2)
    hl, hr = Mp - Mp // 2, Mp // 2
    assert hl == hr + 1
    assert cuts[0] == (3 * F + hl, 20 * F - hr) and cuts[1] == (22 * F + hl, 40 * F - hr)


def test_runs_before_f0_and_behind_f1_are_no_pauses_and_a_row_without_speech_is_untouched():
    hz, F = 16000, 160
    K = 100
    n = K * F - 11
    # 30 inactive frames in front and 40 behind: neither is a pause; the one in the middle touches neither f0 nor f1
    s, e, cuts = _check(_levels(K, [30, 31, 32, 50, 51, 59]), n, hz, 100.0, 1)  # (and 7 frames of 10 ms between 51 and 59 stay)
    assert s == 30 * F - 320 and e == 60 * F + 320 and cuts[0][0] > 33 * F and cuts[0][1] < 50 * F
    # a single active frame: no pause at all
    _check(_levels(K, [44]), n, hz, 20.0, 0)
    # no speech (every level at or below the floor), and an empty row
    assert binding.pause_plan(np.full(K, 5e-8), n, hz, 40.0, 20.0, 20.0)[:2] == (0, n)
    assert binding.pause_plan(np.full(K, 5e-8), n, hz, 40.0, 20.0, 20.0)[3] == 0
    assert pz.plan_levels(np.full(K, 5e-8), n, hz, 40.0, 20.0, 20.0)[:3] == (0, n, [])
    s0, e0, c0, n0 = binding.pause_plan(np.zeros(0), 0, hz, 40.0, 20.0, 20.0)
    assert (s0, e0, n0) == (0, 0, 0) and c0.shape == (0, 2)


def test_300_cuttable_pauses_the_first_255_are_cut():
    hz, F = 8000, 80
    # active, (3 inactive, active) x 300: P = 240 > Mp = 160
    K = 1 + 4 * 300 + 5
    act = [4 * i for i in range(301)]
    n = K * F - 9
    s, e, cuts = _check(_levels(K, act), n, hz, 20.0, 255)
    assert cuts[-1] == ((4 * 254 + 1) * F + 80, (4 * 255) * F - 80)
    # a caller's table smaller than the count: the count is whole, the table its first pairs
    _, _, gc, nc = binding.pause_plan(_levels(K, act), n, hz, 40.0, 20.0, 20.0, cap_pairs=10)
    assert nc == 255 and gc.tolist() == [list(c) for c in cuts[:10]]


def test_levels_of_a_designed_waveform_give_the_designed_cuts():
    hz = 8000
    n = 12345
    x = pz.burst_row(hz, 12400, n, [(10, 6), (40, 1), (80, 20), (150, 3)], 3)
    m = ref.levels(x, n, hz)
    _check(m, n, hz, 100.0, 3)
    _check(m, n, hz, 300.0, 2)
    _check(m, n, hz, 500.0, 0)


def test_the_ranges_are_refused_with_a_message():
    m = _levels(10, [2, 8])
    for kw in (dict(max_pause_ms=19.9), dict(max_pause_ms=5000.5), dict(top_db=0.5), dict(keep_ms=1001.0)):
        with pytest.raises(binding.StnError) as ei:
            binding.pause_plan(m, 800, 8000, **kw)
        assert ei.value.code == -1 and "must be in" in str(ei.value)
    with pytest.raises(binding.StnError) as ei:
        binding.pause_plan(m, 900, 8000)  # K is not ceil(n / F)
    assert "ceil" in str(ei.value)
    with pytest.raises(binding.StnError):
        binding.pause_plan(m, 800, 7000)
    binding.pause_plan(m, 800, 8000, max_pause_ms=20.0)
    binding.pause_plan(m, 800, 8000, max_pause_ms=5000.0)
    assert binding.pause_limit_args(None) == (0, binding.MAX_PAUSE_MS) and binding.pause_limit_args(False)[0] == 0
    assert binding.pause_limit_args(250) == (1, 250.0)
    for bad in (True, 19.0, 5001, "x", (1, 2)):
        with pytest.raises(ValueError):
            binding.pause_limit_args(bad)


# ---- the service ------------------------------------------------------------------------------------------------------------------------
class FakeTTS:
    """records what the batcher asks of it; every utterance is a short constant wave"""
    sample_rate = 44100

    def __init__(self):
        self.calls = []

    def solo_batch(self, texts, langs, style, total_step, speed, **kw):
        self.calls.append((list(texts), kw))
        return [np.full(64, 0.1, np.float32) for _ in texts], np.full(len(texts), 0.01, np.float32)

    def batch(self, texts, langs, style, total_step, speed=1.05, lengths=False, **kw):
        self.calls.append((list(texts), kw))
        wav, dur = np.full((len(texts), 64), 0.1, np.float32), np.full(len(texts), 0.01, np.float32)
        return (wav, dur, np.full(len(texts), 48, np.int64)) if lengths else (wav, dur)


def _styles(paths):
    from supertonic_amd.tts import Style
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


def test_the_batcher_validates_max_pause_and_keeps_unlike_values_apart(monkeypatch):
    from supertonic_amd import service
    tts = FakeTTS()
    style = _styles(["x"])
    keys, real = [], service._Job
    monkeypatch.setattr(service, "_Job", lambda *a: (keys.append(a[3]), real(*a))[1])  # (texts, lang, style, key, silence)
    # every submission below fills its batch, which then runs at once: the batcher never waits out its window
    b = service.DynamicBatcher(tts, max_batch=2, max_wait_ms=60000.0)
    try:
        for bad in (19.0, 5001.0):
            with pytest.raises(ValueError):
                b.submit(["a"], "en", style, 2, 1.05, trim_silence=40, max_pause_ms=bad)
        # two like requests share a key, fill the batch and run as one
        th = [threading.Thread(target=lambda t=t: b.submit([t], "en", style, 2, 1.05, trim_silence=40, max_pause_ms=250)) for t in ("a", "bb")]
        [t.start() for t in th]
        [t.join() for t in th]
        assert b.batches == [2] and keys[0] == keys[1] and tts.calls[-1][1] == {"trim_silence": (40.0, 20.0, 5.0), "max_pause": 250.0}
        b.submit(["c", "d"], "en", style, 2, 1.05, trim_silence=40, max_pause_ms=300)
        b.submit(["e", "f"], "en", style, 2, 1.05, trim_silence=40)
        b.submit(["g", "h"], "en", style, 2, 1.05, max_pause_ms=300)  # without trimming: validated, no effect, out of the key
        b.submit(["i", "j"], "en", style, 2, 1.05)
    finally:
        b.close()
    assert len({keys[1], keys[2], keys[3], keys[4]}) == 4  # 250 ms, 300 ms, trimming alone and nothing: four merge keys
    assert keys[4] == keys[5]
    assert tts.calls[-4][1]["max_pause"] == 300.0 and "max_pause" not in tts.calls[-3][1]
    assert tts.calls[-2][1] == {} and tts.calls[-1][1] == {}


def test_the_service_schema_takes_max_pause_ms_only_with_trimming():
    from fastapi.testclient import TestClient
    from supertonic_amd import service
    tts = FakeTTS()
    app = service.create_app(tts, max_batch=1, max_wait_ms=20.0, style_loader=_styles)
    with TestClient(app) as c:
        for bad in (19.9, 5000.5):
            assert c.post("/tts", json={"text": "a", "trim_silence": 40, "max_pause_ms": bad}).status_code == 422
        r = c.post("/tts", json={"text": "a", "max_pause_ms": 250})
        assert r.status_code == 400 and "trim_silence" in r.json()["detail"]
        r = c.post("/tts", json={"text": "hello", "trim_silence": 40, "max_pause_ms": 250})
        assert r.status_code == 200 and tts.calls[-1][1] == {"trim_silence": (40.0, 20.0, 5.0), "max_pause": 250.0}
        r = c.post("/tts", json={"text": ["a", "b"], "lang": ["en", "en"], "voice_style": ["x", "y"], "batch": True, "trim_silence": 40,
                                 "max_pause_ms": 100})
        assert r.status_code == 200 and tts.calls[-1][1] == {"trim_silence": (40.0, 20.0, 5.0), "max_pause": 100.0}
