"""The true-peak mode's host side without a GPU (include/stn.h "true peak"): stn_true_peak_filter against the
numpy design, the filter's measured response and readings, and a check that the bounds of tests/test_gpu_truepeak.py are sharp enough
to catch a dropped phase, a zeroed halo at a workgroup seam and an envelope shifted by one sample."""
import numpy as np
import pytest

from supertonic_amd import binding

import truepeak_ref as R

W = 16400


def test_filter_equals_the_numpy_design():
    taps = binding.true_peak_filter()
    assert taps.shape == (4, 16) and taps.dtype == np.float32
    assert np.array_equal(taps.view(np.uint32), R.design().view(np.uint32))
    unit = np.zeros(16, np.float32)
    unit[7] = 1.0
    assert np.array_equal(taps[0].view(np.uint32), unit.view(np.uint32))       # phase 0 is exactly the unit tap
    assert np.all(np.abs(taps.astype(np.float64).sum(axis=1) - 1.0) <= 2.0 ** -23)
    assert np.array_equal(taps[3], taps[1][::-1])
    assert np.array_equal(taps[2], taps[2][::-1])
    assert np.allclose(np.abs(taps.astype(np.float64)).sum(axis=1), [1.0, 1.68981, 1.94730, 1.68981], atol=1e-5)


def test_filter_entry_refuses_a_short_buffer():
    L = binding.load()
    P, T = binding.ctypes.c_int(), binding.ctypes.c_int()
    buf = np.full(64, np.nan, np.float32)
    assert L.stn_true_peak_filter(buf.ctypes.data, 63, binding.ctypes.byref(P), binding.ctypes.byref(T)) < 0
    assert np.all(np.isnan(buf)) and (P.value, T.value) == (4, 16)


def _worst_response(fmax):
    t = binding.true_peak_filter().astype(np.float64)
    f = np.linspace(0.0, fmax, 2001)
    j = np.arange(16) - 7
    worst = 0.0
    for p in (1, 2, 3):
        H = (t[p][None, :] * np.exp(2j * np.pi * f[:, None] * j[None, :])).sum(axis=1)
        worst = max(worst, float(np.abs(H - np.exp(2j * np.pi * f * p / 4)).max()))
    return worst


def test_filter_response():
    """every phase against the ideal fractional delay e^{j 2 pi f p / 4}"""
    a, b = _worst_response(0.25), _worst_response(0.35)
    print(f"worst |H_p - ideal|: {a:.3e} to 0.25 fs, {b:.3e} to 0.35 fs")
    assert a <= 2e-4     # 1.2e-4 found
    assert b <= 2e-3     # 1.37e-3 found


def test_readings_of_the_reference_signals():
    x = R.tone45(4096)
    U, _ = R.oversampled(x, x.size)
    steady = float(U[64:-64].max())                       # away from the onset and the end of the burst
    print(f"fs/4 tone at 45 degrees: reading {steady:.6f}, sample peak {np.abs(x).max():.5f}")
    assert abs(20 * np.log10(steady)) <= 0.01 and abs(float(np.abs(x).max()) - 0.70711) < 1e-5
    assert 20 * np.log10(R.true_peak(x) / float(np.abs(x).max())) > 2.9
    pair = np.zeros(64, np.float32)
    pair[30:32] = 1.0
    alt = np.zeros(64, np.float32)
    alt[30:34] = [1, -1, 1, -1]
    assert abs(R.true_peak(pair) - 1.25476) <= 1e-5
    assert abs(R.true_peak(alt) - 1.17171) <= 1e-5
    assert R.true_peak(np.zeros(8, np.float32), 0) == 0.0


@pytest.fixture(scope="module")
def rows():
    x, n = R.kernel_rows(W)
    ref = [R.envelope(x[r], n[r])[0] for r in range(x.shape[0])]
    return x, n, ref


def _violating_rows(x, n, envs):
    return [r for r in range(x.shape[0]) if R.env_violations(envs[r].astype(np.float32), x[r], n[r]).size]


def test_the_reference_itself_passes_its_bounds(rows):
    x, n, ref = rows
    assert _violating_rows(x, n, ref) == []


def test_bounds_catch_a_dropped_phase(rows):
    x, n, _ = rows
    for keep in ((2, 3), (1, 3), (1, 2)):
        bad = _violating_rows(x, n, [R.envelope(x[r], n[r], phases=keep)[0] for r in range(x.shape[0])])
        assert bad, keep


def test_bounds_catch_a_zeroed_halo_at_a_workgroup_seam(rows):
    x, n, ref = rows
    envs = []
    for r in range(x.shape[0]):
        e = ref[r].copy()
        if n[r] > 8192:  # each side of the seam computed as if the other side were zero
            lo = R.envelope(np.where(np.arange(W) < 8192, x[r], 0).astype(np.float32), min(int(n[r]), 8192))[0]
            hi = R.envelope(np.where(np.arange(W) >= 8192, x[r], 0).astype(np.float32), n[r])[0]
            e[:8192] = lo[:8192]
            e[8192:n[r]] = hi[8192:n[r]]
        envs.append(e)
    bad = _violating_rows(x, n, envs)
    assert bad and all(n[r] > 8192 for r in bad)


def test_bounds_catch_a_shift_by_one_sample(rows):
    x, n, ref = rows
    for sh in (1, -1):
        envs = []
        for r in range(x.shape[0]):
            e = ref[r].copy()
            e[:n[r]] = np.roll(ref[r][:n[r]], sh)
            envs.append(e)
        assert len(_violating_rows(x, n, envs)) >= x.shape[0] // 2


def test_peak_mode_names():
    assert binding.peak_mode_id("sample") == 0 and binding.peak_mode_id("true") == 1 and binding.peak_mode_id(None) == 0
    for bad in ("peak", 2, True, ""):
        with pytest.raises(ValueError):
            binding.peak_mode_id(bad)


def test_null_handles_are_refused_without_a_device():
    L = binding.load()
    assert L.stn_get_peak_mode(None) == -1
    for mode in (0, 1, 2):
        assert L.stn_set_peak_mode(None, mode) == -1
        assert L.stn_group_set_peak_mode(None, mode) == -1
    assert L.stn_batch_true_peak(None, None, None, None) == -1
    x = np.zeros((1, 64), np.float32)
    assert L.stn_op_true_peak(None, 16000, 1, 64, x, None, None, 0, None, None, None, None, 0) == -1


# ---- the hosts ---------------------------------------------------------------------------------------------------------------------------
class FakeTTS:
    """A stand-in synthesizer with solo_batch's surface: constant waves, 0.01 s per character; it records what it was asked for."""
    sample_rate = 44100

    def __init__(self):
        self.calls = []

    def solo_batch(self, texts, langs, style, total_step, speed, loudness=None, limiter=None, peak_mode=None):
        self.calls.append((list(texts), loudness, limiter, peak_mode))
        return [np.full(441 * len(t), 0.25, np.float32) for t in texts], np.array([0.01 * len(t) for t in texts], np.float32)

    def batch(self, texts, langs, style, total_step, speed=1.05, loudness=None, limiter=None, peak_mode=None):
        ws, ds = self.solo_batch(texts, langs, style, total_step, speed, loudness, limiter, peak_mode)
        wav = np.zeros((len(ws), 441 * max(len(t) for t in texts)), np.float32)
        for i, w in enumerate(ws):
            wav[i, : w.size] = w
        return wav, ds


def _styles(paths):
    from supertonic_amd.tts import Style
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


def test_batcher_validates_the_mode_and_keys_batches_by_it():
    import threading
    from supertonic_amd import service
    tts = FakeTTS()
    b = service.DynamicBatcher(tts, max_batch=8, max_wait_ms=300.0)
    for bad in ("peak", "TRUE", 1):
        with pytest.raises(ValueError) as ei:
            b.submit(["abc"], "en", _styles(["x"]), 5, 1.05, loudness=-16.0, peak_mode=bad)
        assert "peak_mode" in str(ei.value)
    assert tts.calls == []  # refused before anything was queued

    def go(i, lo, ms, mode):
        b.submit(["text number %d" % i], "en", _styles(["x"]), 5, 1.05, loudness=lo, limiter_ms=ms, peak_mode=mode)

    cases = ((-16.0, None, "true"), (-16.0, None, "true"), (-16.0, None, "sample"), (-16.0, None, None), (-16.0, 5.0, "true"),
             (None, None, "true"), (None, None, None))
    th = [threading.Thread(target=go, args=(i,) + c) for i, c in enumerate(cases)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    b.close()
    # requests that differ in the mode are not merged, like ones are; without loudness the mode is no part of the key
    assert sorted(len(c[0]) for c in tts.calls) == [1, 1, 1, 2, 2]
    assert sorted(str(c[1:]) for c in tts.calls) == sorted(str(v) for v in (((-16.0, -1.0), None, "true"), ((-16.0, -1.0), None, "sample"),
                                                                             ((-16.0, -1.0), None, None), ((-16.0, -1.0), 5.0, "true"),
                                                                             (None, None, None)))


def test_service_field_is_validated_and_reaches_the_synthesizer():
    from fastapi.testclient import TestClient
    from supertonic_amd import service
    tts = FakeTTS()
    app = service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=_styles)
    with TestClient(app) as c:
        for bad in ("peak", "True", 1, 0.5):
            assert c.post("/tts", json={"text": "hello", "loudness": -16, "peak_mode": bad}).status_code == 422, bad
        assert c.post("/tts", json={"text": "hello there", "loudness": -16, "peak_mode": "true"}).status_code == 200
        assert tts.calls[-1] == (["hello there"], (-16.0, -1.0), None, "true")
        assert c.post("/tts", json={"text": "hello there", "loudness": -16, "peak_mode": "sample", "limiter_ms": 3}).status_code == 200
        assert tts.calls[-1] == (["hello there"], (-16.0, -1.0), 3.0, "sample")
        assert c.post("/tts", json={"text": "hello there", "loudness": -16}).status_code == 200 and tts.calls[-1][3] is None
        assert c.post("/tts", json={"text": "hello there", "peak_mode": "true"}).status_code == 200 and tts.calls[-1][1:] == (None, None, None)
        r = c.post("/tts", json={"text": ["ab", "abcd"], "lang": ["en", "en"], "voice_style": ["x", "y"], "batch": True, "loudness": -20,
                                 "peak_mode": "true"})
        assert r.status_code == 200 and tts.calls[-1] == (["ab", "abcd"], (-20.0, -1.0), None, "true")


def test_cli_refuses_the_mode_without_loudness_and_an_unknown_mode():
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "supertonic_amd", "example_native")
    for mode in ("true", "sample"):
        p = subprocess.run([cli, "--synthetic", "--peak-mode", mode, "--n-test", "1"], capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "--peak-mode needs --loudness" in p.stderr, p.stdout + p.stderr
    p = subprocess.run([cli, "--synthetic", "--loudness", "-16", "--peak-mode", "dbtp", "--n-test", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--peak-mode dbtp: sample or true" in p.stderr, p.stdout + p.stderr


def test_python_host_refuses_an_unknown_mode_before_an_engine_exists():
    from supertonic_amd import tts
    with pytest.raises(ValueError) as ei:
        tts.load_text_to_speech("/nonexistent", peak_mode="peak")
    assert "peak_mode" in str(ei.value)
