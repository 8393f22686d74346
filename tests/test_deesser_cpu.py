"""The fetch-time de-esser without a GPU (include/stn.h "de-esser"): the host-only entry points (the band's
sections, the detector's coefficients, the refusals with the two that depend on the rate), the parsers of the binding, the command line
and the service, the OutputSettings field, and the numpy model of the GPU's decomposition (tests/deesser_ref.py) on the inputs and bounds
of the kernel tests (tests/deesser_cases.py): the inputs show what they are there to show on the float64 reference alone, the model
stays inside the bound, and a scan that drops a carry or hands a chunk its neighbour's start value, in the band or in either detector
stage, lands far outside it."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.output import OutputSettings
import compressor_ref as cr
import deesser_cases as dc
import deesser_ref as dr
import filter_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
SPEECH = binding.DEESSER_SPEECH
ALL = [s for s, _ in dc.SETTINGS.values()]


# ---- host-only entry points ------------------------------------------------------------------------------------------------------------------
def test_speech_default_is_the_documented_one():
    assert SPEECH == dr.SPEECH == (5500.0, -30.0, 4.0, 6.0, 1.0, 40.0, 12.0, "split") and binding.DEESSER_FIELDS == dr.FIELDS


@pytest.mark.parametrize("rate", [16000, 44100, 192000])
def test_band_is_two_high_passes_of_the_chain_bit_for_bit(rate):
    for setting in ALL + [(2000.0,) + SPEECH[1:], (min(12000.0, 0.45 * rate),) + SPEECH[1:]]:
        if binding.deesser_error(setting, rate):
            continue
        c, c32 = binding.deesser_band(setting, rate)
        for i, q in enumerate(dr.Q):
            fc, fc32 = binding.filter_coefs(("highpass", setting[0], float(q), 0.0), rate)
            assert np.array_equal(c[i], fc) and np.array_equal(c32[i].view(np.uint32), fc32.view(np.uint32)), (rate, setting[0], i)
        assert np.array_equal(c32.ravel().view(np.uint32), dr.band(setting, rate).view(np.uint32))  # and the reference's own design


@pytest.mark.parametrize("name", list(dc.SETTINGS))
def test_band_response_is_the_fourth_order_butterworth_high_pass(name):
    setting, rate = dc.SETTINGS[name]
    f0 = setting[0]
    freq = np.geomspace(f0 / 4, 0.45 * rate, 400)
    got = binding.filter_response([("highpass", f0, float(q), 0.0) for q in dr.Q], rate, freq)
    # the closed form's high-pass half: the low-pass corner pushed to Nyquist, where its term vanishes
    want = fr.butterworth_band_db(freq, f0, 0.5 * rate * (1 - 1e-13), rate)
    assert np.abs(got - want).max() <= 0.05, (name, np.abs(got - want).max())
    assert abs(np.interp(f0, freq, got) + 3.0103) < 0.01 and got[0] < -47.0  # -3 dB at the corner, 24 dB per octave under it
    assert np.allclose(fr.response_db(binding.deesser_band(setting, rate)[1], rate, freq), got, rtol=0, atol=1e-9)


@pytest.mark.parametrize("rate", [16000, 44100, 192000])
def test_coefs_against_the_closed_form(rate):
    for setting in ALL:
        if binding.deesser_error(setting, rate):
            continue
        k, k32 = binding.deesser_coefs(setting, rate)
        for i, ms in enumerate(setting[4:6]):
            want = 1.0 - np.exp(-1000.0 / (float(np.float32(ms)) * rate))
            assert abs(k[i] / want - 1) < 1e-9 and k[i] == cr.k_of(ms, rate) and k32[i] == np.float32(k[i])
        ck, ck32 = binding.compressor_coefs(tuple(setting[1:6]) + (0.0,), rate)  # k as stn_compressor_coefs forms it
        assert np.array_equal(k, ck) and np.array_equal(k32, ck32)
        f = dr.coefs(setting, rate)
        assert k32[0] == f["kA"] and k32[1] == f["kR"] and f["S"] == np.float32(1.0 / setting[2] - 1.0)


def test_every_refusal_names_its_field():
    ok = list(SPEECH)
    assert binding.deesser_error(SPEECH, 44100) == "" and binding.deesser_error(SPEECH) == "" and binding.deesser_error(SPEECH, 0) == ""
    limits = {"freq_hz": (2000.0, 12000.0), "threshold_db": (-60.0, 0.0), "ratio": (1.0, 20.0), "knee_db": (0.0, 24.0),
              "attack_ms": (0.1, 300.0), "release_ms": (10.0, 3000.0), "range_db": (1.0, 24.0)}
    for i, (field, (lo, hi)) in enumerate(limits.items()):
        for v in (lo, hi):  # the limits themselves are inside (at a rate high enough for 12 kHz)
            s = ok[:i] + [v] + ok[i + 1:]
            assert binding.deesser_error(tuple(s), 0) == "" and binding.deesser_error(tuple(s), 48000) == "", (field, v)
        for v in (np.nextafter(np.float32(lo), np.float32(-1e9)), np.nextafter(np.float32(hi), np.float32(1e9))):
            for rate in (0, 48000):  # rate 0: the limits that need no rate are checked all the same
                why = binding.deesser_error(tuple(ok[:i] + [float(v)] + ok[i + 1:]), rate)
                assert why.startswith("deesser: " + field) and "must be in" in why, (field, v, rate, why)
    # the two corners that depend on the rate are the chain's for a high-pass with q in [0.5, 1.5]: 0.45 x rate above ...
    for rate, f0, bad in ((8000, 5500.0, True), (16000, 7200.0, False), (16000, 7201.0, True), (8000, 3600.0, False), (44100, 12000.0, False),
                          (22050, 9923.0, True)):
        why = binding.deesser_error((f0,) + SPEECH[1:], rate)
        assert (why != "") == bad and (not bad or (why.startswith("deesser: freq_hz") and "0.45" in why and str(rate) in why)), (rate, f0, why)
        chain = binding.filter_error([("highpass", f0, float(dr.Q[0]), 0.0), ("highpass", f0, float(dr.Q[1]), 0.0)], rate)
        assert (chain != "") == bad, (rate, f0, chain)  # exactly where the chain refuses the same two sections
    # ... and rate / 2400 below, which the lowest freq_hz (2000 Hz) clears at every rate there is (80 Hz at 192 kHz): nothing to refuse
    assert binding.deesser_error((2000.0,) + SPEECH[1:], 192000) == ""
    assert "SPLIT" in binding.load().stn_deesser_error(binding.StnDeesser(*SPEECH[:7], 2), 0).decode()  # an unknown mode
    assert binding.load().stn_deesser_error(None, 0).decode() == "deesser: c is null"
    for rate in (7999, 192001, -1):
        assert "rate" in binding.deesser_error(SPEECH[:0] + (3000.0,) + SPEECH[1:], rate)
    for fn in (binding.deesser_band, binding.deesser_coefs):  # the helpers refuse what the setter refuses, and want a rate
        for setting, rate in ((SPEECH, 8000), (SPEECH, 0), ((5500.0, -61.0) + SPEECH[2:], 44100)):
            with pytest.raises(binding.StnError):
                fn(setting, rate)


# ---- parsers ------------------------------------------------------------------------------------------------------------------------------------
def test_binding_parser():
    da = binding.deesser_args
    assert da(None) is None and da(False) is None and da(True) == SPEECH and da({}) == SPEECH
    assert da({"freq_hz": 6000, "threshold_db": -28}) == (6000.0, -28.0) + SPEECH[2:]
    assert da({"mode": "wide"})[7] == "wide" and da({"mode": 1})[7] == "wide" and da(SPEECH[:7] + (0,)) == SPEECH
    assert da([np.float32(4000), -36, 10, 0, 0.1, 10, np.int64(24), "wide"]) == dc.SETTINGS["wide_16k"][0]
    assert da(None, preset="speech") == SPEECH and da({"ratio": 5}, preset="speech")[2] == 5.0
    assert all(type(v) is float for v in da(True)[:7]) and hash(da({"ratio": 4.0})) == hash(SPEECH)
    for bad, word in (({"freq": 6000}, "freq"), ((1, 2, 3), "8-tuple"), ({"ratio": "3"}, "ratio"), ({"range_db": float("nan")}, "range_db"),
                      ({"ratio": True}, "ratio"), (3.0, "8-tuple"), ({"mode": "both"}, "mode"), ({"mode": 2}, "mode"), ({"mode": True}, "mode"),
                      (SPEECH[:6] + (None, "split"), "range_db")):
        with pytest.raises(ValueError) as ei:
            da(bad)
        assert word in str(ei.value), (bad, str(ei.value))
    with pytest.raises(ValueError) as ei:
        da(True, preset="music")
    assert "speech" in str(ei.value)
    s = binding._deesser_struct({"mode": "wide"})
    assert (s.freq_hz, s.range_db, s.mode) == (5500.0, 12.0, 1)


def test_command_line_spelling():
    p = binding.parse_deesser_spec
    assert p("6000:-28") == (6000.0, -28.0) + SPEECH[2:] and p("6000:-28:8") == (6000.0, -28.0, 8.0) + SPEECH[3:]
    assert p("4000:-36:10:0:0.1:10:24:wide") == dc.SETTINGS["wide_16k"][0] and p("4000:-36:10:0:0.1:10:24") == dc.SETTINGS["wide_16k"][0][:7] + ("split",)
    assert binding.deesser_args("6000:-28") == p("6000:-28")
    for bad, word in (("6000", "FREQ"), ("1:2:3:4:5:6:7:split:9", "FREQ"), ("6000:x", "must be numbers"), (":4", "must be numbers"), ("", "FREQ"),
                      ("6000:-28:4:6:1:40:12:both", "MODE"), ("6000:-28:4:6:1:40:12:1", "MODE")):
        with pytest.raises(ValueError) as ei:
            p(bad)
        assert word in str(ei.value), (bad, str(ei.value))
    # the C++ host's parser spells the same errors, before any device is touched
    if os.path.exists(CLI):
        for args, word in ((["--deesser", "6000"], "FREQ:THRESHOLD"), (["--deesser", "6000:x"], "must be numbers"),
                           (["--deesser", "6000:-28:4:6:1:40:12:both"], "MODE must be one of split, wide"), (["--deesser-preset", "music"], "speech")):
            r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and word in r.stderr, (args, r.stderr)


def test_service_key():
    from supertonic_amd import service
    key = lambda **kw: service.batch_key(44100, 5, 1.05, **kw)
    assert key().settings.deesser is None and key(deesser=False).settings.deesser is False
    assert key(deesser=True) == key(deesser=SPEECH) == key(deesser={}) and key(deesser=True).settings.deesser == SPEECH
    assert key(deesser=True) != key() and key(deesser=True) != key(deesser=False) and key(deesser={"mode": "wide"}) != key(deesser=True)
    assert key(deesser={"freq_hz": 6000}).settings.kwargs() == {"deesser": (6000.0,) + SPEECH[1:]}
    assert key(deesser=False).settings.kwargs() == {"deesser": False}
    assert key(deesser=True, compressor=True) != key(compressor=True) and key(deesser=True, compressor=True).settings.compressor == binding.COMPRESSOR_SPEECH
    for kw, word in ((dict(deesser={"ratio": 40}), "ratio"), (dict(deesser={"freq": 1}), "freq"), (dict(deesser={"range_db": 0.5}), "range_db"),
                     (dict(deesser=True, sample_rate=8000), "0.45"), (dict(deesser={"mode": "narrow"}), "mode")):
        with pytest.raises(ValueError) as ei:
            key(**kw)
        assert word in str(ei.value), (kw, str(ei.value))
    assert key(deesser={"freq_hz": 3000}, sample_rate=8000).settings.deesser[0] == 3000.0  # checked against the request's rate, not the model's


class FakeTTS:
    """The synthesizer's surface with the fetch settings recorded: each utterance a constant wave, 0.01 s per character."""
    sample_rate = 44100

    def __init__(self):
        self.calls = []

    def _waves(self, texts):
        durs = np.array([0.01 * max(len(t), 1) for t in texts], np.float32)
        return [np.full((int(44100 * d) + 3071) // 3072 * 3072, 0.25, np.float32) for d in durs], durs

    def solo_batch(self, texts, langs, style, total_step, speed, deesser=None, output_rate=None, **_):
        self.calls.append((list(texts), deesser, output_rate))
        return self._waves(texts)

    def batch(self, texts, langs, style, total_step, speed=1.05, deesser=None, output_rate=None, **_):
        self.calls.append((list(texts), deesser, output_rate))
        ws, ds = self._waves(texts)
        wav = np.zeros((len(ws), max(len(w) for w in ws)), np.float32)
        for i, w in enumerate(ws):
            wav[i, : len(w)] = w
        return wav, ds


def _styles(paths):
    from supertonic_amd.tts import Style
    return Style(np.zeros((len(paths), 2, 4), np.float32), np.zeros((len(paths), 2, 3), np.float32))


def test_service_validates_the_field_and_hands_it_to_the_synthesizer():
    from fastapi.testclient import TestClient
    from supertonic_amd import service
    tts = FakeTTS()
    app = service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=_styles)
    with TestClient(app) as c:
        for body, what in (({"deesser": {"ratio": 40}}, "ratio"), ({"deesser": {"freq": 6000}}, "freq"), ({"deesser": {"mode": "both"}}, "mode"),
                           ({"deesser": True, "sample_rate": 8000}, "freq_hz"), ({"deesser": {"range_db": 0.5}}, "range_db")):
            r = c.post("/tts", json=dict(text="hello there", **body))
            assert r.status_code == 400 and what in r.json()["detail"], (body, r.status_code, r.text)
        assert c.post("/tts", json={"text": "hello", "deesser": "6000:-28"}).status_code == 422
        assert tts.calls == []
        assert c.post("/tts", json={"text": "hello there", "deesser": True}).status_code == 200 and tts.calls[-1] == (["hello there"], SPEECH, None)
        assert c.post("/tts", json={"text": "hello there", "deesser": {"freq_hz": 3000, "mode": "wide"}, "sample_rate": 8000}).status_code == 200
        assert tts.calls[-1][1:] == ((3000.0,) + SPEECH[1:7] + ("wide",), 8000)
        assert c.post("/tts", json={"text": "hello there", "deesser": False}).status_code == 200 and tts.calls[-1][1] is False
        assert c.post("/tts", json={"text": "hello there"}).status_code == 200 and tts.calls[-1][1] is None
        r = c.post("/tts", json={"text": ["ab", "abcd"], "lang": ["en", "en"], "voice_style": ["x", "y"], "batch": True, "deesser": {"threshold_db": -28}})
        assert r.status_code == 200 and tts.calls[-1] == (["ab", "abcd"], (5500.0, -28.0) + SPEECH[2:], None)


# ---- OutputSettings ----------------------------------------------------------------------------------------------------------------------------
class _Engine:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("set_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append((name, a))


def test_output_settings_field():
    P = OutputSettings.parse
    assert P().deesser is None and P(deesser=False).deesser is False and P(deesser=None).deesser is None
    assert P(deesser=True).deesser == SPEECH and P(deesser={"freq_hz": 6000}).deesser == (6000.0,) + SPEECH[1:]
    assert P(deesser=list(SPEECH)) == P(deesser=True) and hash(P(deesser=True)) == hash(P(deesser=SPEECH))
    with pytest.raises(ValueError):
        P(deesser={"freq": 1})
    # OFF keeps exactly its fields; ALL_OFF names every field
    assert OutputSettings.OFF == OutputSettings(0, (), False, False, False, False, "sample")
    assert OutputSettings.OFF.deesser is None and OutputSettings.OFF.compressor is None and OutputSettings.ALL_OFF.deesser is False
    assert [f.name for f in dataclasses.fields(OutputSettings) if getattr(OutputSettings.ALL_OFF, f.name) is None] == []
    assert OutputSettings.ALL_OFF.replace(compressor=None, deesser=None) == OutputSettings.OFF
    # deesser is no constructor argument: replace() and parse() set it, dataclasses.replace leaves it out and refuses to be given it
    on = P(deesser=True, loudness=-16)
    assert on.replace(loudness=False).deesser == SPEECH and on.replace(deesser=False).loudness == (-16.0, -1.0) and on != P(loudness=-16)
    assert dataclasses.replace(on, loudness=False).deesser is None
    with pytest.raises(ValueError):
        dataclasses.replace(on, deesser=False)
    with pytest.raises(TypeError):
        OutputSettings(deesser=True)
    assert P(deesser=True).kwargs() == {"deesser": SPEECH} and P(**P(deesser=True).kwargs()) == P(deesser=True)
    assert P(deesser=False).over(P(deesser=True)).deesser is False and P().over(P(deesser=True)).deesser == SPEECH


def test_output_settings_apply_order_and_restore():
    e = _Engine()
    P = OutputSettings.parse
    # behind the chain and in front of the compressor; checked against the rate, so off before the rate changes and on after it, as the chain
    P(output_rate=16000, filters=[("highpass", 80)], deesser={"freq_hz": 4000}, compressor=True, loudness=-16).apply(e)
    assert [c[0] for c in e.calls] == ["set_filters", "set_deesser", "set_output_rate", "set_filters", "set_deesser", "set_compressor", "set_loudness"]
    assert e.calls[1] == ("set_deesser", (None,)) and e.calls[4] == ("set_deesser", ((4000.0,) + SPEECH[1:],))
    e.calls.clear()
    P(deesser=True).apply(e)  # without a rate in the same value, one call
    assert e.calls == [("set_deesser", (SPEECH,))]
    e.calls.clear()
    P(deesser=False, output_rate=8000).apply(e)  # the instance's de-esser goes off before a rate that would refuse it comes
    assert e.calls == [("set_deesser", (None,)), ("set_output_rate", (8000,))]
    e.calls.clear()
    P(deesser=False).apply(e)
    assert e.calls == [("set_deesser", (None,))]
    # a per-call de-esser over an instance that has none is put back to off: the instance's settings name every field (ALL_OFF)
    base = P().over(OutputSettings.ALL_OFF)
    e.calls.clear()
    with P(deesser={"mode": "wide"}).applied(e, base) as now:
        assert now.deesser == SPEECH[:7] + ("wide",) and e.calls == [("set_deesser", (now.deesser,))]
    assert e.calls[-1] == ("set_deesser", (None,)) and len(e.calls) == 2
    # and over an instance that has one, back to the instance's
    base = P(deesser=True).over(OutputSettings.ALL_OFF)
    e.calls.clear()
    with P(deesser=False).applied(e, base):
        pass
    assert e.calls == [("set_deesser", (None,)), ("set_deesser", (SPEECH,))]


# ---- the decomposition ---------------------------------------------------------------------------------------------------------------------------
def _over(c, m):
    st = c.ref.states(c.f, dc.W_MAX)
    out = {k: dc.over_bound(c, k, m[k], st[k]) for k in dc.STATES}
    out.update(h=dc.over_bound(c, "h", m["h"], c.ref.h), yl=dc.over_bound(c, "yl", m["yl"], c.ref.yl), y=dc.over_bound(c, "y", m["y"], c.ref.y))
    return out


@pytest.mark.parametrize("name", list(dc.SETTINGS))
def test_inputs_show_what_they_are_there_for_on_the_reference_alone(name):
    c = dc.case(name)
    low = dc.conditions(c)
    print(f"\n{name}: least carry into a seam {low:.2f} dB; reduction per row " + " ".join(f"{v:.2f}" for v in c.ref.yl.max(axis=1)))
    assert all(v > 0 for k in ("yl", "y") for v in c.dev[k][list(dc.LOUD)])  # the restatement does deviate where there is reduction
    assert not c.bound["yl"][list(dc.STILL)].any() and not c.bound["s1_end"][list(dc.STILL)].any()  # and the still rows get no allowance
    if c.f["split"]:  # there the reference's y is x itself
        assert np.array_equal(c.ref.y[list(dc.STILL)], c.x[list(dc.STILL)].astype(np.float64)) and not c.bound["y"][list(dc.STILL)].any()
    assert c.ref.yl.max() <= float(c.f["R"])  # nothing is ever turned down by more than the range


@pytest.mark.parametrize("name", list(dc.SETTINGS))
def test_model_of_the_decomposition_stays_inside_the_bound(name):
    c = dc.case(name)
    full = dr.model(c.x, c.f)
    worst = {k: float(v.max()) for k, v in _over(c, full).items()}
    print(f"\n{name}: model over bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    for W in (dc.SPAN + 1, dc.TILE - dr.CHUNK):  # the model at a narrower W is the model cut there
        m = dr.model(c.x[:, :W], c.f)
        assert np.array_equal(m["y"], full["y"][:, :W]) and np.array_equal(m["s2_start"], full["s2_start"][:, : dr.chunks(W)])
        assert np.array_equal(m["st_start"], full["st_start"][:, : dr.chunks(W)])


# what a fault costs on the model, in yL over its bound on the row named (measured here; DESIGN.md section 21 has the table).  Every
# fault lands over the bound on at least one of the two fast settings; at a 300 ms release a chunk's neighbour holds almost the same
# values, so slow_192k sees only the lost carries.  A lost carry of stage 1 shows only where the chunk behind the seam does not reach the
# lost level again by itself (the detector is a maximum).
FAULTS = [
    ("default_44k", "band_carry", dc.KNEE, 1e4), ("default_44k", "band_neighbour", dc.ESS, 1e4), ("default_44k", ("carry1", dr.SCAN), dc.CLICKS, 1e4),
    ("default_44k", ("carry1", dr.WG), dc.NOISE, 1000.0), ("default_44k", ("carry2", 2 * dr.SCAN), dc.ESS, 1e4), ("default_44k", "neighbour1", dc.ESS, 1e4),
    ("default_44k", "neighbour2", dc.ESS, 1e4),
    ("wide_16k", "band_carry", dc.ESS, 1e4), ("wide_16k", "band_neighbour", dc.NOISE, 1e4), ("wide_16k", ("carry1", dr.SCAN), dc.ESS, 1e4),
    ("wide_16k", ("carry1", dr.WG), dc.NOISE, 1e4), ("wide_16k", ("carry2", 2 * dr.SCAN), dc.NOISE, 1e4), ("wide_16k", "neighbour1", dc.ESS, 1e4),
    ("wide_16k", "neighbour2", dc.NOISE, 1e4),
    ("slow_192k", "band_carry", dc.KNEE, 10.0), ("slow_192k", ("carry1", dr.SCAN), dc.KNEE, 100.0), ("slow_192k", ("carry2", 2 * dr.SCAN), dc.NOISE, 1000.0),
]


@pytest.mark.parametrize("name,fault,row,factor", FAULTS)
def test_a_faulty_scan_lands_far_outside_the_bound(name, fault, row, factor):
    c = dc.case(name)
    m = dr.model(c.x, c.f, fault)
    over = dc.over_bound(c, "yl", m["yl"], c.ref.yl)
    print(f"\n{name} {fault} on {dc.NAMES[row]}: yL {over[row]:.1f} x the bound, {np.abs(m['yl'][row] - c.ref.yl[row]).max():.3f} dB")
    assert over[row] >= factor, (name, fault, dc.NAMES[row], over)
    assert over[dc.ZERO] == 0
    if isinstance(fault, str) and fault.startswith("band"):  # a band fault is seen in h itself as well, on every row with a signal
        assert dc.over_bound(c, "h", m["h"], c.ref.h)[[r for r in range(8) if r != dc.ZERO]].min() >= 1000.0
    else:
        assert not over[list(dc.STILL)].any()
