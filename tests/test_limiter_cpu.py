"""The limiter's host side without a GPU (include/stn.h "limiter"): stn_limiter_window against numpy, the refused
arguments, and the properties the contract promises, on the numpy reference (tests/limiter_ref.py) over the GPU tests' own cases."""
import itertools

import numpy as np
import pytest

from supertonic_amd import binding
import limiter_ref as ref

RATES = [8000, 11025, 16000, 44100, 48000, 192000]
MS = [0.5, 5.0, 10.0]
ULP = 2.0 ** -23


@pytest.mark.parametrize("hz,ms", list(itertools.product(RATES, MS)))
def test_window_is_the_normalized_hann_of_the_contract(hz, ms):
    w = binding.limiter_window(hz, ms)
    A = int(ms * hz / 1000.0 + 0.5)
    assert w.dtype == np.float32 and w.size == A + 1 == ref.samples(hz, ms) + 1
    assert 4 <= A <= 1920
    want = ref.window(hz, ms)
    # (both are the float64 formula rounded once: a last-bit difference of the two cosines can move the rounding by one ulp at most)
    assert np.all(np.abs(w.astype(np.float64) - want) <= ULP * want)
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 1e-6
    assert np.all(w > 0) and np.all(np.abs(w.astype(np.float64) - w[::-1]) <= ULP * w)  # symmetric
    assert int(np.argmax(w)) in (A // 2, (A + 1) // 2)


def test_window_refuses_what_the_contract_refuses():
    for hz, ms in ((44100, 0.49), (44100, 10.01), (44100, float("nan")), (7999, 5.0), (192001, 5.0), (0, 5.0)):
        with pytest.raises(binding.StnError):
            binding.limiter_window(hz, ms)
    n = binding.ctypes.c_int64()
    assert binding.load().stn_limiter_window(44100, 5.0, None, 0, binding.ctypes.byref(n)) == 0 and n.value == 222
    part = np.full(8, -1.0, np.float32)  # a short buffer gets its capacity, no more
    assert binding.load().stn_limiter_window(44100, 5.0, part.ctypes.data, 5, binding.ctypes.byref(n)) == 0
    assert np.array_equal(part[:5], binding.limiter_window(44100, 5.0)[:5]) and np.all(part[5:] == -1.0)
    for bad in (0.4, 11, "x", (1, 2)):
        with pytest.raises(ValueError):
            binding.limiter_args(bad)
    assert binding.limiter_args(None) == (0, 5.0) and binding.limiter_args(False) == (0, 5.0)
    assert binding.limiter_args(True) == (1, 5.0) and binding.limiter_args(2.5) == (1, 2.5)


@pytest.mark.parametrize("hz,ms", [(8000, 0.5), (44100, 5.0)])
def test_reference_keeps_the_contracts_properties(hz, ms):
    W = 20011
    for rep in (0, 1):
        x, n, g = ref.peaky_rows(hz, ms, -1.0, W, rep)
        for b, o in enumerate(ref.limit_rows(x, n, g, -1.0, hz, ms)):
            c, nb = float(o["c"]), int(n[b])
            assert np.abs(o["y"]).max() <= c                               # the ceiling, padding included
            assert np.all(o["s"][:nb] <= o["r"][:nb].astype(np.float64))   # never above what the sample itself needs
            assert np.array_equal(o["s"][:nb] == 1.0, o["M"][:nb] == 1.0)  # untouched exactly where no peak is in reach
            assert np.all(o["s"] > 0.0) and np.all(o["s"][nb:] == 1.0)
            assert o["limited"] == np.count_nonzero(o["s"][:nb] < 1.0)
            if nb > 1:
                assert o["limited"] > 0 and o["reduction_db"] > 6.0  # (peaks of 2 x the ceiling or more)
            if nb + 5 < W:
                assert abs(o["y"][nb + 5]) == c  # the over-level sample of the padding, clamped


@pytest.mark.parametrize("hz,ms", ref.LONG_CASES)
def test_long_look_ahead_rows_hold_what_the_kernel_can_get_wrong(hz, ms):
    """the rows of limiter_ref.long_case (A = 1920, 960, 441, 88), read off the reference's own r and M: in each whole-span row an
    isolated peak with 2A + 1 clear samples each side, two peaks A apart, two 2A + 1 apart with nothing between, a plateau of 3A
    samples, peaks on both sides of tile boundaries, a tile the reference leaves untouched (the kernel's early exit) and, at the
    largest A, a peak whose reach covers three tiles; the spans; and the contract's properties on every row."""
    A = ref.samples(hz, ms)
    lay = ref.long_layout(A)
    W, T = lay["W"], ref.TILE
    assert W == max(20011, 20 * A + 4096)
    spans = ref.long_spans(A)
    assert set(spans) >= {0, 1, A, A + 1, 2 * A + 1, W, W - 1} and len(spans) == 12
    assert sum(s % T == T - 1 for s in spans) >= 2 and sum(s % T == 1 and s > 1 for s in spans) >= 2  # tile multiples -+ 1
    whole = 0
    for rep in (0, 1):
        x, n, g, outs = ref.long_case(hz, ms, -1.0, rep)
        assert x.shape == (6, W) and n.tolist() == spans[6 * rep:6 * rep + 6]
        for b, o in enumerate(outs):
            c, nb = float(o["c"]), int(n[b])
            assert np.abs(o["y"]).max() <= c
            assert np.all(o["s"][:nb] <= o["r"][:nb].astype(np.float64))
            assert np.array_equal(o["s"][:nb] == 1.0, o["M"][:nb] == 1.0)
            assert np.all(o["s"] > 0.0) and np.all(o["s"][nb:] == 1.0)
            assert o["limited"] == np.count_nonzero(o["s"][:nb] < 1.0)
            if nb + 5 < W:
                assert abs(o["y"][nb + 5]) == c
            if nb < W - 1:
                continue
            whole += 1
            hot = o["r"] < 1.0
            iso = lay["iso"]
            assert hot[iso] and not hot[iso - 2 * A - 1:iso].any() and not hot[iso + 1:iso + 2 * A + 2].any()
            assert np.all(o["M"][iso - A:iso + A + 1] < 1.0) and o["M"][iso - A - 1] == 1.0 and o["M"][iso + A + 1] == 1.0  # its reach, no more
            p, q = lay["pair"]
            assert q - p == A and hot[p] and hot[q] and not hot[p + 1:q].any()
            p, q = lay["wide"]
            assert q - p == 2 * A + 1 and hot[p] and hot[q] and not hot[p + 1:q].any() and o["M"][p + A + 1] < 1.0  # (m[i - A] reaches q)
            p, q = lay["plateau"]
            assert q - p == 3 * A and hot[p:q].all()
            assert len(lay["bounds"]) >= 2 and all(hot[k - 1] and hot[k + 1] for k in lay["bounds"])
            tiles = o["M"][:W // T * T].reshape(-1, T)
            untouched = np.flatnonzero(np.all(tiles == 1.0, axis=1))
            assert untouched.size >= 1  # r == 1 over the tile and A samples each side
            for t in untouched:
                assert not hot[max(0, t * T - A):t * T + T + A].any()
            assert np.any(tiles < 1.0)
            if A == 1920:  # the isolated peak at 4440 turns down samples of tiles 1, 2 and 3
                assert len({(iso - A) // T, iso // T, (iso + A) // T}) == 3
    assert whole == 2


def test_reference_leaves_a_row_under_the_ceiling_alone():
    x = (0.3 * np.sin(np.arange(5000) / 7.0)).astype(np.float32)
    o = ref.limit_row(x, 4000, 1.7, -1.0, 16000, 5.0)
    assert np.all(o["s"] == 1.0) and o["limited"] == 0 and o["reduction_db"] == 0.0
    assert np.array_equal(o["y"].astype(np.float32), (x * np.float32(1.7)).astype(np.float32))


# ---- the hosts ---------------------------------------------------------------------------------------------------------------------------
class FakeTTS:
    """A stand-in synthesizer with solo_batch's surface: constant waves, 0.01 s per character; it records what it was asked for."""
    sample_rate = 44100

    def __init__(self):
        self.calls = []

    def solo_batch(self, texts, langs, style, total_step, speed, loudness=None, limiter=None):
        self.calls.append((list(texts), loudness, limiter))
        return [np.full(441 * len(t), 0.25, np.float32) for t in texts], np.array([0.01 * len(t) for t in texts], np.float32)

    def batch(self, texts, langs, style, total_step, speed=1.05, loudness=None, limiter=None):
        ws, ds = self.solo_batch(texts, langs, style, total_step, speed, loudness, limiter)
        wav = np.zeros((len(ws), 441 * max(len(t) for t in texts)), np.float32)
        for i, w in enumerate(ws):
            wav[i, : w.size] = w
        return wav, ds


def _styles(paths):
    from supertonic_amd.tts import Style
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


def test_python_host_setting():
    from supertonic_amd.tts import _limiter_setting
    assert _limiter_setting(None) is None and _limiter_setting(False) is None and _limiter_setting(True) == 5.0 and _limiter_setting(2) == 2.0
    for bad in (0.4, 10.5):
        with pytest.raises(ValueError) as ei:
            _limiter_setting(bad)
        assert "must be in [0.5, 10]" in str(ei.value)


def test_batcher_validates_the_setting_and_keys_batches_by_it():
    import threading
    from supertonic_amd import service
    tts = FakeTTS()
    b = service.DynamicBatcher(tts, max_batch=8, max_wait_ms=300.0)
    for bad in (0.4, 10.5):
        with pytest.raises(ValueError) as ei:
            b.submit(["abc"], "en", _styles(["x"]), 5, 1.05, loudness=-16.0, limiter_ms=bad)
        assert "must be in" in str(ei.value)
    assert tts.calls == []  # refused before anything was queued

    def go(i, lo, ms):
        b.submit(["text number %d" % i], "en", _styles(["x"]), 5, 1.05, loudness=lo, limiter_ms=ms)

    th = [threading.Thread(target=go, args=(i, lo, ms)) for i, (lo, ms) in enumerate(((-16.0, 5.0), (-16.0, 5.0), (-16.0, None), (-16.0, 2.0), (None, 5.0), (None, None)))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    b.close()
    # requests that differ in the limiter are not merged, like ones are; without loudness the limiter is no part of the key
    assert sorted(len(c[0]) for c in tts.calls) == [1, 1, 2, 2]
    assert sorted(str(c[1:]) for c in tts.calls) == sorted(str(v) for v in (((-16.0, -1.0), 5.0), ((-16.0, -1.0), None), ((-16.0, -1.0), 2.0), (None, None)))


def test_service_field_is_validated_and_reaches_the_synthesizer():
    from fastapi.testclient import TestClient
    from supertonic_amd import service
    tts = FakeTTS()
    app = service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=_styles)
    with TestClient(app) as c:
        for bad in (0.4, 10.5, "soft"):
            assert c.post("/tts", json={"text": "hello", "loudness": -16, "limiter_ms": bad}).status_code == 422, bad
        assert c.post("/tts", json={"text": "hello there", "loudness": -16, "limiter_ms": 3}).status_code == 200
        assert tts.calls[-1] == (["hello there"], (-16.0, -1.0), 3.0)
        assert c.post("/tts", json={"text": "hello there", "loudness": -16}).status_code == 200 and tts.calls[-1][2] is None
        r = c.post("/tts", json={"text": ["ab", "abcd"], "lang": ["en", "en"], "voice_style": ["x", "y"], "batch": True, "loudness": -20, "limiter_ms": 5})
        assert r.status_code == 200 and tts.calls[-1] == (["ab", "abcd"], (-20.0, -1.0), 5.0)


def test_cli_refuses_the_limiter_without_loudness():
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "supertonic_amd", "example_native")
    p = subprocess.run([cli, "--synthetic", "--limiter", "5", "--n-test", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--limiter needs --loudness" in p.stderr, p.stdout + p.stderr
