"""The fetch-time filter chain without a GPU (include/stn.h "filter chain"): the designer against the cookbook
restated in float64 (tests/filter_ref.py), the response function, the corner limits' 0.1 dB condition on the grid it was measured on,
the analytic facts of the six types, the validation messages, the telephone preset against the closed-form Butterworth band, the Python,
CLI and service parsers, and the numpy model of the kernels' decomposition: it stays inside the bounds of tests/filter_cases.py, and two
injected faults do not."""
import os
import subprocess
import threading

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.tts import Style
import filter_cases as fc
import filter_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)
GRID_Q, GRID_GAIN = (0.3, 0.707, 2.0, 8.0), (6.0, -6.0, 18.0, -18.0)


def test_coefs_equal_the_restated_cookbook_design():
    worst = 0.0
    for rate in (8000, 44100, 192000):
        for kind in fr.TYPES:
            for freq, q, gain in ((rate / 800.0 * 1.01, 0.3, -18.0), (1000.0, 0.7071, 6.0), (0.45 * rate * 0.999, 8.0, 18.0), (rate / 7.3, 1.3, -2.5)):
                c, c32 = binding.filter_coefs((kind, freq, q, gain), rate)
                ref = fr.design(kind, freq, q, gain, rate)
                assert np.allclose(c, ref, rtol=1e-12, atol=1e-15), (kind, rate, freq, q, gain, c, ref)
                assert np.array_equal(c32, c.astype(np.float32))
                worst = max(worst, float(np.max(np.abs(c - ref) / np.maximum(np.abs(ref), 1e-3))))
    print(f"\nlargest relative distance of stn_filter_coefs from the restated design: {worst:.1e}")
    # a0 = 1 forms: the high-pass has a double zero at DC, the low-pass at Nyquist, bit for bit after the rounding to fp32
    _, hp = binding.filter_coefs(("highpass", 80.0), 44100)
    _, lp = binding.filter_coefs(("lowpass", 3400.0), 8000)
    assert hp[1] == -2 * hp[0] and hp[2] == hp[0] and lp[1] == 2 * lp[0] and lp[2] == lp[0]


def test_response_is_the_response_of_the_fp32_coefficients():
    chain = fc.CHAINS["odd_44k"][1]
    f = np.geomspace(10.0, 20000.0, 40)
    c32 = np.stack([binding.filter_coefs(s, 44100)[1] for s in chain])
    assert np.allclose(binding.filter_response(chain, 44100, f), fr.response_db(c32, 44100, f), rtol=0, atol=1e-9)
    one = binding.filter_response(chain[:1], 44100, f)
    assert np.allclose(one, fr.response_db(c32[:1], 44100, f), rtol=0, atol=1e-9)


def _fp32_deviation(kind, freq, q, gain, rate):
    """largest |response of the fp32-rounded section - response of the double design| in dB over 25 log-spaced frequencies from 1/4 x to
    4 x the corner (below Nyquist), wherever the design is above -40 dB"""
    c = fr.design(kind, freq, q, gain, rate)
    f = np.geomspace(0.25 * freq, min(4.0 * freq, 0.499 * rate), 25)
    d, r = fr.response_db(c, rate, f), fr.response_db(c.astype(np.float32), rate, f)
    live = d > -40.0
    return float(np.abs(r - d)[live].max()) if live.any() else 0.0


def test_the_corner_limits_keep_the_fp32_response_within_a_tenth_of_a_db():
    butter = max(_fp32_deviation(k, fc.lowest_corner(rate), q, 0.0, rate) for rate in RATES for k in ("highpass", "lowpass") for q in (0.5, 0.541, 0.7071, 1.307, 1.5))
    grid = {(div, k): max(_fp32_deviation(k, rate / div, q, g, rate) for rate in RATES for q in GRID_Q for g in GRID_GAIN) for div in (800, 2400) for k in fr.TYPES}
    all800 = max(v for (div, _), v in grid.items() if div == 800)
    print(f"\nworst deviation of the fp32-rounded response: Butterworth-range high-/low-pass at rate/2400 {butter:.3f} dB; all six types at rate/800 "
          f"{all800:.3f} dB; at rate/2400 " + ", ".join(f"{k} {grid[(2400, k)]:.2f}" for k in fr.TYPES) + " dB")
    assert butter <= 0.1, butter
    assert all800 <= 0.1, {k: v for (div, k), v in grid.items() if div == 800}
    assert grid[(2400, "peak")] > 0.1  # the second limit is needed: a peak filter at the first breaks the condition
    # and the limits are the ones the C ABI enforces
    for rate in (8000, 48000, 192000):
        assert binding.filter_error([("highpass", fc.lowest_corner(rate), 0.7071)], rate) == ""
        assert "freq_hz" in binding.filter_error([("highpass", rate / 2400.0 * 0.99, 0.7071)], rate)
        assert "freq_hz" in binding.filter_error([("highpass", rate / 800.0 * 0.99, 2.0)], rate)  # outside the Butterworth range of q
        assert "freq_hz" in binding.filter_error([("peak", rate / 800.0 * 0.99, 0.7071, 3.0)], rate)
        assert binding.filter_error([("peak", rate / 800.0 * 1.01, 0.7071, 3.0)], rate) == ""


def test_analytic_facts():
    for rate in (8000, 44100, 192000):
        fcn = rate / 40.0
        for kind in ("highpass", "lowpass"):
            assert abs(binding.filter_response([(kind, fcn, 0.7071)], rate, [fcn])[0] + 3.01) <= 0.01, (kind, rate)
        for g in (-12.0, 4.0, 18.0):
            r = binding.filter_response([("peak", fcn, 1.0, g)], rate, [fcn, 1e-6, rate / 2.0])
            assert abs(r[0] - g) <= 0.01 and abs(r[1]) <= 0.01 and abs(r[2]) <= 0.01, (rate, g, r)
            lo = binding.filter_response([("lowshelf", fcn, 0.7071, g)], rate, [fcn / 10.0])[0]
            hi = binding.filter_response([("highshelf", fcn, 0.7071, g)], rate, [fcn * 10.0])[0]
            assert abs(lo - g) <= 0.05 and abs(hi - g) <= 0.05, (rate, g, lo, hi)
        assert binding.filter_response([("notch", fcn, 2.0)], rate, [fcn])[0] < -60.0


def test_every_validation_error_names_its_field():
    ok = ("peak", 1000.0, 1.0, 3.0)
    assert binding.filter_error([ok], 48000) == ""
    for bad, field in ((("peak", 1000.0, 0.29, 3.0), "q"), (("peak", 1000.0, 8.1, 3.0), "q"), (("peak", 1000.0, 1.0, 18.5), "gain_db"),
                       (("peak", 1000.0, 1.0, -18.5), "gain_db"), (("lowpass", 0.46 * 48000, 0.7071, 0.0), "freq_hz"),
                       (("highpass", 19.0, 0.7071, 0.0), "freq_hz"), (("notch", 59.0, 0.7071, 0.0), "freq_hz")):
        why = binding.filter_error([ok, bad], 48000)
        assert field in why and "filter 1" in why, (bad, why)
        with pytest.raises(binding.StnError) as ei:
            binding.filter_coefs(bad, 48000)
        assert field in str(ei.value)
    assert "type" in binding.load().stn_filter_error(1, (binding.StnFilter * 1)(binding.StnFilter(9, 1000.0, 1.0, 0.0)), 48000).decode()
    assert "n = 9" in binding.load().stn_filter_error(9, (binding.StnFilter * 9)(), 48000).decode()
    assert "sample rate" in binding.filter_error([ok], 7000)
    # the telephone band is refused below 8 kHz like any chain whose corner breaks a limit
    assert binding.filter_error(binding.FILTER_PRESETS["telephone"], 8000) == "" and binding.filter_error(binding.FILTER_PRESETS["telephone"], 7000) != ""
    assert "freq_hz" in binding.filter_error([("lowpass", 3700.0)], 8000)


def test_telephone_preset_is_the_fourth_order_butterworth_band():
    f = np.geomspace(100.0, 3900.0, 200)
    got = binding.filter_response(binding.FILTER_PRESETS["telephone"], 8000, f)
    want = fr.butterworth_band_db(f, 300.0, 3400.0, 8000, order=4)
    d = np.abs(got - want)
    print(f"\ntelephone preset against the closed form: at most {d.max():.4f} dB (at {f[d.argmax()]:.0f} Hz, {want[d.argmax()]:.1f} dB)")
    assert d.max() <= 0.1
    assert abs(got[np.abs(f - 1000.0).argmin()]) < 0.05 and binding.filter_response(binding.FILTER_PRESETS["telephone"], 8000, [300.0, 3400.0]).max() < -2.9


def test_python_spec_parser_and_presets():
    assert binding.parse_filter_spec("highpass:80") == ("highpass", 80.0, 0.7071, 0.0)
    assert binding.parse_filter_spec("peak:3000:1:4") == ("peak", 3000.0, 1.0, 4.0)
    for bad, what in (("highpass", "TYPE:FREQ"), ("bandpass:300", "type"), ("peak:abc", "numbers"), ("peak:1:2:3:4", "TYPE:FREQ")):
        with pytest.raises(ValueError) as ei:
            binding.parse_filter_spec(bad)
        assert what in str(ei.value)
    a = binding.filter_args([{"type": "highpass", "freq": 80}, ("peak", 3000, 1.0, 4), "lowshelf:200:0.7:3"], preset="rumble")
    assert a == (("highpass", 80.0, 0.7071, 0.0), ("highpass", 80.0, 0.7071, 0.0), ("peak", 3000.0, 1.0, 4.0), ("lowshelf", 200.0, 0.7, 3.0))
    assert binding.filter_args(None) == () and binding.filter_args([]) == () and len(binding.filter_args(None, "telephone")) == 4
    for bad, what in (([{"type": "highpass"}], "freq"), ([{"freq": 80}], "type"), ([{"type": "highpass", "freq": 80, "Q": 1}], "'Q'"),
                      ([("highpass", "x")], "freq"), ([("peak", 100, 1, float("nan"))], "gain_db"), ("highpass:80", "list"), ([("highpass", 80)] * 9, "at most 8")):
        with pytest.raises(ValueError) as ei:
            binding.filter_args(bad)
        assert what in str(ei.value), (bad, str(ei.value))
    with pytest.raises(ValueError) as ei:
        binding.filter_args(None, "radio")
    assert "rumble" in str(ei.value)


def test_cli_refuses_a_malformed_filter_before_it_touches_a_device():
    for args, what in ((["--filter", "bandpass:300"], "type must be one of"), (["--filter", "peak:abc"], "must be numbers"), (["--filter", "peak"], "TYPE:FREQ"),
                       (["--filter-preset", "radio"], "rumble or telephone"), (["--filter-preset", "telephone"] + ["--filter", "peak:1000:1:3"] * 5, "at most 8")):
        p = subprocess.run([CLI, "--synthetic", "--n-test", "1"] + args, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and what in p.stderr, (args, p.stdout + p.stderr)


class FakeTTS:
    """The synthesizer's surface with the fetch settings recorded: each utterance a constant wave, 0.01 s per character."""
    sample_rate = 44100

    def __init__(self):
        self.calls = []

    def _waves(self, texts):
        durs = np.array([0.01 * max(len(t), 1) for t in texts], np.float32)
        return [np.full((int(44100 * d) + 3071) // 3072 * 3072, 0.25, np.float32) for d in durs], durs

    def solo_batch(self, texts, langs, style, total_step, speed, filters=None, output_rate=None, **_):
        self.calls.append((list(texts), None if filters is None else tuple(filters), output_rate))
        return self._waves(texts)

    def batch(self, texts, langs, style, total_step, speed=1.05, filters=None, output_rate=None, **_):
        self.calls.append((list(texts), None if filters is None else tuple(filters), output_rate))
        ws, ds = self._waves(texts)
        wav = np.zeros((len(ws), max(len(w) for w in ws)), np.float32)
        for i, w in enumerate(ws):
            wav[i, : len(w)] = w
        return wav, ds


def _styles(paths):
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


def test_service_validates_filters_and_hands_them_to_the_synthesizer():
    from fastapi.testclient import TestClient
    from supertonic_amd import service
    tts = FakeTTS()
    app = service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=_styles)
    hp = {"type": "highpass", "freq": 80, "q": 0.7071, "gain_db": 0}
    with TestClient(app) as c:
        for body, what in (({"filters": [{"type": "bandpass", "freq": 80}]}, "type"), ({"filters": [{"type": "highpass"}]}, "freq"),
                           ({"filters": [{"type": "peak", "freq": 1000, "q": 9}]}, "q"), ({"filters": [{"type": "peak", "freq": 1000, "gain_db": 19}]}, "gain_db"),
                           ({"filters": [{"type": "highpass", "freq": 10}]}, "freq_hz"), ({"filter_preset": "radio"}, "filter_preset"),
                           ({"filters": [hp] * 9}, "at most 8"), ({"filters": [{"type": "lowpass", "freq": 8000}], "sample_rate": 8000}, "freq_hz"),
                           ({"filter_preset": "telephone", "filters": [hp] * 5}, "at most 8")):
            r = c.post("/tts", json=dict(text="hello there", **body))
            assert r.status_code == 400 and what in r.json()["detail"], (body, r.status_code, r.text)
        assert c.post("/tts", json={"text": "hello", "filters": "highpass:80"}).status_code == 422
        assert tts.calls == []
        assert c.post("/tts", json={"text": "hello there", "filters": [hp, {"type": "peak", "freq": 3000, "q": 1, "gain_db": 4}]}).status_code == 200
        assert tts.calls[-1] == (["hello there"], (("highpass", 80.0, 0.7071, 0.0), ("peak", 3000.0, 1.0, 4.0)), None)
        assert c.post("/tts", json={"text": "hello there", "filter_preset": "telephone", "sample_rate": 8000, "encoding": "mulaw"}).status_code == 200
        assert tts.calls[-1][1] == binding.FILTER_PRESETS["telephone"] and tts.calls[-1][2] == 8000
        assert c.post("/tts", json={"text": "hello there"}).status_code == 200 and tts.calls[-1][1] is None
        r = c.post("/tts", json={"text": ["ab", "abcd"], "lang": ["en", "en"], "voice_style": ["x", "y"], "batch": True, "filter_preset": "rumble"})
        assert r.status_code == 200 and tts.calls[-1] == (["ab", "abcd"], binding.FILTER_PRESETS["rumble"], None)


def test_batcher_merges_only_requests_with_equal_chains():
    from supertonic_amd import service
    tts = FakeTTS()
    b = service.DynamicBatcher(tts, max_batch=8, max_wait_ms=300.0)
    with pytest.raises(ValueError) as ei:
        b.submit(["abc"], "en", _styles(["x"]), 5, 1.05, filters=[("highpass", 10)])
    assert "freq_hz" in str(ei.value) and tts.calls == []
    hp, pk = [("highpass", 80)], [{"type": "highpass", "freq": 80}, ("peak", 3000, 1, 4)]

    def go(i, f):
        b.submit(["text number %d" % i], "en", _styles(["x"]), 5, 1.05, filters=f)

    th = [threading.Thread(target=go, args=(i, f)) for i, f in enumerate((hp, [{"type": "highpass", "freq": 80.0, "q": 0.7071}], pk, None, None, []))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    b.close()
    # equal chains (however they were written) share a batch; unlike chains, no chain and the chain switched off do not
    assert sorted((len(c[0]), c[1]) for c in tts.calls if c[1] is not None) == [(1, ()), (1, (("highpass", 80.0, 0.7071, 0.0), ("peak", 3000.0, 1.0, 4.0))), (2, (("highpass", 80.0, 0.7071, 0.0),))]
    assert [len(c[0]) for c in tts.calls if c[1] is None] == [2]


MODEL_CASES = ("hp_lowest_44k", "odd_44k", "telephone_8k", "peak_q8_44k", "notch_shelf_16k")


@pytest.mark.parametrize("name", MODEL_CASES)
def test_the_bound_is_attainable_and_sees_the_faults(name):
    """the numpy model of the decomposition (fp32 in the chunk, the scan in double, fp32 start states, fp32 between the passes) stays
    inside 4 x the float32 restatement's deviation with room, so the bound can be met; a scan carry dropped at a tile seam and a start
    state taken from the wrong chunk do not"""
    c = fc.case(name)
    assert c.W == 3 * 32768 + 40 and c.x.shape == (5, c.W)
    good = fc.over_bound(c, fr.decomposed(c.x, c.passes))
    carry = fc.over_bound(c, fr.decomposed(c.x, c.passes, fault="carry"))
    chunk = fc.over_bound(c, fr.decomposed(c.x, c.passes, fault="chunk"))
    print(f"\n{name}: model over bound {good}; carry dropped {carry}; wrong chunk {chunk}")
    assert max(good.values()) < 1.0, good
    assert carry["start"] > 1.0 and carry["y"] > 1.0, carry
    assert chunk["start"] > 1.0 and chunk["y"] > 1.0, chunk
    assert not np.any(fr.decomposed(c.x, c.passes)[2][fc.ZERO])  # the zero row gives exactly zero


def test_restatement_agrees_with_an_independent_filter():
    """filter_ref.chain_states in float64 against scipy's lfilter section by section, and its chunk states against a restart from them"""
    from scipy.signal import lfilter
    rate, chain = fc.CHAINS["odd_44k"]
    c32 = np.stack([binding.filter_coefs(f, rate)[1] for f in chain])
    passes = fr.passes_of(c32)
    x = fc.signals(rate, 80.0, 4000)[:3]
    start, end, y = fr.chain_states(x, passes, np.float64)
    want = x.astype(np.float64)
    for c in c32.astype(np.float64):
        want = lfilter(c[:3], [1.0, c[3], c[4]], want, axis=1)
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
    # chunk k refiltered from start[k] ends in start[k + 1]; from zero state in end[k]
    ins = x.astype(np.float64)
    for p in range(passes.shape[0]):
        out = np.zeros((3, fr.chunks(4000) * 32))
        e = fr.chunk_ends(ins, passes[p], np.float64, start=start[p], out=out)
        assert np.allclose(e[:, :-1], start[p][:, 1:], rtol=0, atol=1e-12)
        assert np.array_equal(fr.chunk_ends(ins, passes[p], np.float64), end[p])
        ins = out[:, :4000]
    assert np.allclose(ins, y, rtol=0, atol=1e-12)
