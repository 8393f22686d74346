"""The fetch-time expander without a GPU (include/stn.h "expander"): the host-only entry points (coefficients,
static curve, refusals), the hold and the release of the float64 reference, the parsers of the binding, the command line and the
service, the OutputSettings attribute, and the numpy model of the GPU's decomposition (tests/expander_ref.py) on the inputs and bounds of
the kernel tests (tests/expander_cases.py): the model stays inside the bound, and a scan that drops a carry or hands a chunk its
neighbour's start value, or a gain computer that boosts partly open samples, lands far outside it."""
import dataclasses
import inspect
import os
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.output import OutputSettings
import expander_cases as xc
import expander_ref as xr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
SPEECH, GATE = binding.EXPANDER_SPEECH, binding.EXPANDER_GATE


# ---- host-only entry points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 44100, 192000])
def test_coefs_against_the_closed_forms(rate):
    assert SPEECH == xr.SPEECH == (-50.0, 3.0, 6.0, 24.0, 1.0, 30.0, 150.0) and GATE == xr.GATE == (-45.0, 20.0, 0.0, 60.0, 0.5, 50.0, 100.0)
    for setting in (SPEECH, GATE) + tuple(s for s, _ in xc.SETTINGS.values()):
        k, k32, hs = binding.expander_coefs(setting, rate)
        R, attack, hold, release = (float(np.float32(setting[i])) for i in (3, 4, 5, 6))
        want_kA = 1.0 - np.exp(-1000.0 / (attack * rate))       # k = 1 - exp(-1 / (tau rate)), tau in seconds: section 20's k form
        assert abs(k[0] / want_kA - 1) < 1e-9 and k[0] == -np.expm1(-1000.0 / (attack * rate))
        assert k[1] == R * 1000.0 / (release * rate)             # dB per sample: the whole range in release_ms
        assert abs(R / k[1] - release * rate / 1000.0) < 1e-6 * release * rate
        assert hs == int(np.floor(hold * rate / 1000.0 + 0.5)) == xr.hold_samples(setting, rate)
        assert k[2] == float(np.float32(k[1])) * hs              # Bh from the fp32 delta the GPU subtracts
        assert np.array_equal(k32, k.astype(np.float32))
        f = xr.coefs(setting, rate)
        assert (k32[0], k32[1], k32[2]) == (f["kA"], f["delta"], f["Bh"])
    with pytest.raises(binding.StnError):
        binding.expander_coefs(SPEECH, 7999)


def test_delta_never_rounds_away():
    """At the worst corner (192 kHz, hold 500 ms plus release 3000 ms) delta is still about 12 fp32 spacings of the largest u, R + Bh,
    whatever the range: u - delta never rounds back to u."""
    worst = np.inf
    for R in np.concatenate([np.linspace(1.0, 80.0, 317), 2.0 ** np.arange(0, 7) * (6.0 / 7.0) * (1 + 1e-6)]):
        if not 1.0 <= R <= 80.0:
            continue
        _, k32, hs = binding.expander_coefs((-50.0, 3.0, 6.0, float(R), 1.0, 500.0, 3000.0), 192000)
        top = np.float32(np.float32(R) + k32[2])
        assert hs == 96000
        spacings = float(k32[1]) / float(np.spacing(top))
        worst = min(worst, spacings)
        u = top
        assert np.float32(u - k32[1]) < u
    print(f"\nsmallest delta / spacing(R + Bh) over the ranges: {worst:.2f}")
    assert 11.0 < worst < 13.0


def test_static_curve():
    T, ratio, K, R = -50.0, 3.0, 6.0, 24.0
    c = (T, ratio, K, R, 1.0, 30.0, 150.0)
    x = np.linspace(-100.0, 0.0, 10001)
    y = binding.expander_curve(c, x)
    above = x > T + K / 2
    slope_region = (x < T - K / 2) & (x > T - R / (ratio - 1) + 0.01)
    clamped = x < T - R / (ratio - 1) - 0.01
    assert np.array_equal(y[above], x[above])                                                            # identity above the knee
    assert np.allclose(np.diff(y[slope_region]) / np.diff(x[slope_region]), ratio, rtol=0, atol=1e-9)    # slope `ratio` below it
    assert np.allclose(y[slope_region], T + (x[slope_region] - T) * ratio, rtol=0, atol=1e-9)
    assert np.allclose(y[clamped], x[clamped] - R, rtol=0, atol=1e-12) and clamped.sum() > 100           # clamp at the range
    h = 1e-6
    for edge, slope in ((T + K / 2, 1.0), (T - K / 2, ratio)):                                           # value and slope continuous at both knee ends
        lo, mid, hi = binding.expander_curve(c, [edge - h, edge, edge + h])
        assert abs(hi - mid) < 4 * h and abs(mid - lo) < 4 * h
        assert abs((mid - lo) / h - (hi - mid) / h) < 1e-4 and abs((hi - lo) / (2 * h) - slope) < 1e-4, (edge, lo, mid, hi)
    assert np.all(np.diff(y) > 0)
    assert np.array_equal(binding.expander_curve((T, 1.0, K, R, 1.0, 30.0, 150.0), x), x)                # ratio 1 is the identity
    hard = binding.expander_curve((T, ratio, 0.0, R, 1.0, 30.0, 150.0), x)                               # knee 0 is the hard corner
    lo = (x < T) & (x > T - R / (ratio - 1))
    assert np.array_equal(hard[x >= T], x[x >= T]) and np.allclose(hard[lo], T + (x[lo] - T) * ratio, rtol=0, atol=1e-9)
    assert binding.expander_curve((T, ratio, 0.0, R, 1.0, 30.0, 150.0), [T])[0] == T
    # the curve is what the reference's gain computer gives
    f = xr.coefs(c, 44100)
    amp = 10.0 ** (x[::50] / 20.0)
    z = xr.want(amp.astype(np.float32)[None, :], f)[0]
    xg = 20 * np.log10(np.maximum(amp.astype(np.float32).astype(np.float64), 1e-6))
    assert np.allclose(binding.expander_curve(c, xg), xg - z, rtol=0, atol=1e-12)


LIMITS = {"threshold_db": (-90.0, -10.0), "ratio": (1.0, 20.0), "knee_db": (0.0, 24.0), "range_db": (1.0, 80.0), "attack_ms": (0.1, 300.0),
          "hold_ms": (0.0, 500.0), "release_ms": (10.0, 3000.0)}
BAD = {"threshold_db": (-90.5, -9.5), "ratio": (0.99, 20.5), "knee_db": (-0.1, 24.5), "range_db": (0.9, 80.5), "attack_ms": (0.09, 301.0),
       "hold_ms": (-0.1, 501.0), "release_ms": (9.0, 3001.0)}


def test_every_refusal_names_its_field():
    assert binding.expander_error(SPEECH) == "" and binding.expander_error(True, 48000) == "" and binding.expander_error(GATE, 8000) == ""
    lib = binding.load()
    assert tuple(LIMITS) == binding.EXPANDER_FIELDS == xr.FIELDS
    for i, name in enumerate(binding.EXPANDER_FIELDS):
        for bad in BAD[name] + (float("nan"), float("inf")):
            s = list(SPEECH)
            s[i] = bad
            why = lib.stn_expander_error(binding.ctypes.byref(binding.StnExpander(*s)), 0).decode()  # (the C ABI: the binding stops a NaN itself)
            assert name in why and all(o not in why for o in binding.EXPANDER_FIELDS if o != name), (name, bad, why)
            if np.isfinite(bad):
                assert binding.expander_error(tuple(s)) == why
                with pytest.raises(binding.StnError):
                    binding.expander_curve(tuple(s), [0.0])
                with pytest.raises(binding.StnError):
                    binding.expander_coefs(tuple(s), 44100)
        for ok in LIMITS[name]:
            s = list(SPEECH)
            s[i] = ok
            for rate in (0, 8000, 192000):  # no limit depends on the rate
                assert binding.expander_error(tuple(s), rate) == "", (name, ok, rate)
    assert "rate" in binding.expander_error(SPEECH, 7999)  # (a rate is only checked when one is given)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting,rate", [(SPEECH, 44100), (GATE, 8000), (GATE, 48000), ((-40.0, 2.0, 12.0, 12.0, 5.0, 500.0, 200.0), 16000),
                                          ((-45.0, 20.0, 0.0, 60.0, 0.1, 0.0, 10.0), 8000)])
def test_hold_and_release_of_the_reference(setting, rate):
    """after a burst ends y1 = min(u, R) stays at R for Hs samples and is 0 release_ms later, each within one sample; the row starts
    closed and the burst opens the detector at once"""
    f = xr.coefs(setting, rate)
    R, Hs, rel = float(f["R"]), xr.hold_samples(setting, rate), float(np.float32(setting[6])) * rate / 1000.0
    n0, n1 = 100, 100 + int(0.02 * rate)
    W = n1 + Hs + int(rel) + 200
    x = np.zeros((1, W), np.float32)
    x[0, n0:n1] = 0.5  # (a constant: every sample of the burst is fully open)
    r = xr.Ref(x, f)
    y1 = np.minimum(r.u[0], R)
    assert not y1[:n0].any() and not r.yl[0, :n0].any() and y1[n0] == R  # closed until the burst, then open at once
    assert np.all(y1[n0:n1] == R)
    held = int(np.argmax(y1[n1:] < R))  # samples behind the burst's last that still show R
    assert abs(held - Hs) <= 1, (held, Hs)
    closed = int(np.argmax(y1[n1:] == 0))
    assert abs(closed - (Hs + rel)) <= 1 and not y1[n1 + closed:].any(), (closed, Hs + rel)
    fall = y1[n1 + held + 1: n1 + closed - 1]
    assert np.allclose(np.diff(fall), -float(f["delta"]), rtol=0, atol=1e-9)  # a constant rate in dB
    # the attack: yL reaches 1 - 1 / e of the range within one sample of attack_ms
    n = int(np.argmax(r.yl[0] >= (1 - np.exp(-1.0)) * R)) - n0
    assert abs((n + 1) - float(np.float32(setting[4])) * rate / 1000.0) <= 1.0
    assert abs(20 * np.log10(r.y[0, n1 - 1] / 0.5) - (r.yl[0, n1 - 1] - R)) < 1e-9


def test_a_zero_crossing_is_bridged():
    f = xr.coefs((-50.0, 3.0, 6.0, 24.0, 1.0, 0.0, 150.0), 44100)  # (no hold: the release alone bridges)
    n = np.arange(4000)
    x = (0.5 * np.sin(2 * np.pi * 220.0 * n / 44100.0)).astype(np.float32)[None, :]
    r = xr.Ref(x, f)
    assert (r.z[0] > 0).sum() > 10 and (r.z[0] == float(f["R"])).any()   # some samples at the crossings want the gate shut
    assert r.yl[0, 500:].min() > float(f["R"]) - 0.05                    # the detector holds it open


# ---- parsers ------------------------------------------------------------------------------------------------------------------------------------
def test_binding_parser():
    xa = binding.expander_args
    assert xa(None) is None and xa(False) is None and xa(True) == SPEECH
    assert xa({"threshold_db": -45}) == (-45.0,) + SPEECH[1:] and xa({}) == SPEECH
    assert xa((-40, 4, 0, 30, 1, 50, 100)) == (-40.0, 4.0, 0.0, 30.0, 1.0, 50.0, 100.0)
    assert xa([np.float32(-40), 4, 0, 30, 1, 50, np.int64(100)]) == (-40.0, 4.0, 0.0, 30.0, 1.0, 50.0, 100.0)
    assert xa(None, preset="speech") == SPEECH and xa(None, preset="gate") == GATE and xa(True, preset="gate") == GATE
    assert xa({"ratio": 5}, preset="gate") == (GATE[0], 5.0) + GATE[2:]
    assert all(type(v) is float for v in xa((-40, 4, 0, 30, 1, 50, 100)))
    for bad, word in (({"threshold": -20}, "threshold"), ((1, 2, 3), "7-tuple"), ({"ratio": "3"}, "ratio"), ({"knee_db": float("nan")}, "knee_db"),
                      ({"hold_ms": True}, "hold_ms"), (3.0, "7-tuple"), ((-40, 4, 0, 30, 1, 50, None), "release_ms")):
        with pytest.raises(ValueError) as ei:
            xa(bad)
        assert word in str(ei.value), (bad, str(ei.value))
    with pytest.raises(ValueError) as ei:
        xa(True, preset="music")
    assert "speech" in str(ei.value) and "gate" in str(ei.value)


def test_command_line_spelling():
    p = binding.parse_expander_spec
    assert p("-45:4") == (-45.0, 4.0) + SPEECH[2:] and p("-45:4:0") == (-45.0, 4.0, 0.0) + SPEECH[3:]
    assert p("-45:4:3:40:2:10") == (-45.0, 4.0, 3.0, 40.0, 2.0, 10.0, 150.0) and p("-45:4:3:40:2:10:80.5") == (-45.0, 4.0, 3.0, 40.0, 2.0, 10.0, 80.5)
    assert binding.expander_args("-48:2") == (-48.0, 2.0) + SPEECH[2:]
    assert p("-48:2", "gate") == binding.expander_args("-48:2", preset="gate") == (-48.0, 2.0) + GATE[2:]  # beside a preset: the rest from it
    for bad in ("-45", "-45:4:3:40:2:10:80:9", "-45:x", ":4", ""):
        with pytest.raises(ValueError) as ei:
            p(bad)
        assert "THRESHOLD" in str(ei.value)
    # the C++ host's parser spells the same errors, before any device is touched
    assert os.path.exists(CLI), "supertonic_amd/example_native is not built (make all builds it beside libstn.so)"
    for args, word in ((["--expander", "-45"], "THRESHOLD:RATIO"), (["--expander", "-45:x"], "must be numbers"), (["--expander-preset", "music"], "speech or gate")):
        r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and word in r.stderr, (args, r.stderr)


def test_service_key():
    from supertonic_amd import service
    key = lambda **kw: service.batch_key(44100, 5, 1.05, **kw)
    assert key().settings.expander is None and key(expander=False).settings.expander is False
    assert key(expander=True) == key(expander=SPEECH) == key(expander={}) and key(expander=True).settings.expander == SPEECH
    assert key(expander=True) != key() and key(expander=True) != key(expander=False) and key(expander={"ratio": 4}) != key(expander=True)
    assert key(expander=False) != key() and key().expander_set is False and key(expander=False).expander_set is True  # none named: the server's
    assert key(expander={"ratio": 4}).settings.kwargs() == {"expander": (-50.0, 4.0) + SPEECH[2:]}
    assert key(expander=False).settings.kwargs() == {"expander": False} and key().settings.kwargs() == {}
    for bad, word in (({"ratio": 40}, "ratio"), ({"hold": 1}, "hold"), ({"release_ms": 1}, "release_ms"), ({"range_db": 90}, "range_db")):
        with pytest.raises(ValueError) as ei:
            key(expander=bad)
        assert word in str(ei.value)
    assert "expander" in inspect.signature(service.batch_key).parameters


def test_service_validates_the_field_and_hands_it_to_the_synthesizer():
    from fastapi.testclient import TestClient
    from supertonic_amd import service
    from supertonic_amd.tts import Style

    class Fake:
        sample_rate = 44100
        settings = OutputSettings().decided()

        def __init__(self):
            self.seen = []

        def solo_batch(self, texts, langs, style, total_step, speed, **out):
            self.seen.append(out)
            return [np.zeros(4410, np.float32) for _ in texts], np.full(len(texts), 0.1, np.float32)

    tts = Fake()
    style = Style(np.zeros((1, 2, 2), np.float32), np.zeros((1, 2, 2), np.float32))
    app = service.create_app(tts, max_batch=4, max_wait_ms=1.0, style_loader=lambda paths: style)
    with TestClient(app) as c:
        for body, want in ((True, SPEECH), ({"threshold_db": -45}, (-45.0,) + SPEECH[1:]), (False, False)):
            r = c.post("/tts", json={"text": "Hello there.", "expander": body})
            assert r.status_code == 200 and tts.seen[-1].get("expander") == want, (body, r.text, tts.seen[-1:])
        r = c.post("/tts", json={"text": "Hello there."})
        assert r.status_code == 200 and "expander" not in tts.seen[-1]
        r = c.post("/tts", json={"text": "Hello there.", "expander": {"attack_ms": 0.01}})
        assert r.status_code == 400 and "attack_ms" in r.json()["detail"]
        r = c.post("/tts", json={"text": "Hello there.", "expander": {"attack": 1}})
        assert r.status_code == 400 and "attack" in r.json()["detail"]


# ---- OutputSettings ----------------------------------------------------------------------------------------------------------------------------
class _Engine:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("set_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append((name, a))


def test_output_settings_attribute():
    P = OutputSettings.parse
    assert P().expander is None and P(expander=False).expander is False and P(expander=None).expander is None
    assert P(expander=True).expander == SPEECH and P(expander={"ratio": 4}).expander == (-50.0, 4.0) + SPEECH[2:]
    assert P(expander=list(SPEECH)) == P(expander=True) and hash(P(expander=True)) == hash(P(expander=SPEECH))
    assert P(expander=True) != P() and P(expander=True) != P(expander=GATE) and "expander=(-50.0" in repr(P(expander=True))
    with pytest.raises(ValueError):
        P(expander={"threshold": 1})
    # added the way dither and pitch were: no dataclass field, OFF and ALL_OFF as they were, positional construction unchanged
    assert "expander" not in [f.name for f in dataclasses.fields(OutputSettings)]
    assert OutputSettings.OFF.expander is None and OutputSettings.ALL_OFF.expander is None
    assert OutputSettings(0, (), False, False, False, False, "sample") == OutputSettings.OFF
    assert P().decided().expander is False and P(expander=GATE).decided().expander == GATE
    assert P().decided() == OutputSettings.ALL_OFF.replace(dither=False)  # decided() is still ALL_OFF (unset and off are both no expander)
    assert P(expander=True).kwargs() == {"expander": SPEECH} and P(**P(expander=True).kwargs()) == P(expander=True)   # round trip
    assert P(expander=False).kwargs() == {"expander": False} and P(**P(expander=False).kwargs()).expander is False
    assert P(expander=False).over(P(expander=True)).expander is False and P().over(P(expander=True)).expander == SPEECH
    assert P(expander=True).replace(loudness=(-16.0, -1.0)).expander == SPEECH


def test_output_settings_apply_order_and_restore():
    e = _Engine()
    P = OutputSettings.parse
    P(output_rate=16000, filters=[("highpass", 80)], expander=True, deesser={"freq_hz": 5000}, compressor=True, loudness=-16).apply(e)
    names = [c[0] for c in e.calls]
    # behind the filters, in front of the de-esser
    assert names == ["set_filters", "set_deesser", "set_output_rate", "set_filters", "set_expander", "set_deesser", "set_compressor", "set_loudness"]
    assert e.calls[4] == ("set_expander", (SPEECH,))
    e.calls.clear()
    P(expander=False).apply(e)
    assert e.calls == [("set_expander", (None,))]
    # a per-call expander over an instance that has none is put back to off
    base = P().decided()
    e.calls.clear()
    with P(expander={"ratio": 4}).applied(e, base) as now:
        assert now.expander == (-50.0, 4.0) + SPEECH[2:] and e.calls == [("set_expander", (now.expander,))]
    assert e.calls[-1] == ("set_expander", (None,)) and len(e.calls) == 2
    # and over an instance that has one, back to the instance's
    base = P(expander=GATE).decided()
    e.calls.clear()
    with P(expander=False).applied(e, base):
        pass
    assert e.calls == [("set_expander", (None,)), ("set_expander", (GATE,))]


# ---- the decomposition ---------------------------------------------------------------------------------------------------------------------------
def _over(c, m):
    st = c.ref.states(c.f, xc.W_MAX)
    out = {k: xc.over_bound(c, k, m[k], st[k]) for k in xc.STATES}
    out["yl"] = xc.over_bound(c, "yl", m["yl"], c.ref.yl)
    out["y"] = xc.over_bound(c, "y", m["y"], c.ref.y)
    return out


@pytest.mark.parametrize("name", list(xc.SETTINGS))
def test_model_of_the_decomposition_stays_inside_the_bound(name):
    c = xc.case(name)
    xc.conditions(c)
    assert all(v > 0 for k in ("yl", "y") for v in c.dev[k][list(xc.BURST_ROWS)])  # the restatement does deviate where the gate moves
    assert not c.bound["yl"][[xc.QUIET, xc.ZERO]].any() and not any(c.bound[k][[xc.QUIET, xc.ZERO]].any() for k in xc.STATES)  # the closed rows' states must be exact
    assert np.all(c.bound["y"][[xc.QUIET]] <= 4 * 2.0 ** -23)
    over = _over(c, xr.model(c.x, c.f))
    worst = {k: float(v.max()) for k, v in over.items()}
    print(f"\n{name}: model over bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    full = xr.model(c.x, c.f)
    for W in (xc.SPAN + 1, xc.TILE - xr.CHUNK):  # the model at a narrower W is the model cut there
        m = xr.model(c.x[:, :W], c.f)
        assert np.array_equal(m["y"], full["y"][:, :W]) and np.array_equal(m["s2_start"], full["s2_start"][:, : xr.chunks(W)])


# Measured on the model (over bound, in yL, on the rows named): what a fault costs on the two fast settings (DESIGN.md section 25 has the
# table).  Every seam of the burst rows lies in the hold or the release, so a lost stage-1 start value closes the gate there, and a lost
# stage-2 one restarts the smoothing from 0.  At gate_8k the hold is 0, so Bh is 0 and the boost fault changes nothing: speech_44k
# (30 ms) is the setting that catches it.  At slow_192k a chunk's neighbour holds almost the same values, so the neighbour faults stay
# close to the bound there; its lost carries still show.
FAULTS = [
    ("speech_44k", ("carry1", xr.SCAN), xc.BURSTS, 1000.0), ("speech_44k", ("carry1", 2 * xr.SCAN), xc.NOISE, 1000.0),
    ("speech_44k", ("carry1", xr.WG), xc.BURSTS, 1000.0), ("speech_44k", ("carry2", xr.SCAN), xc.BURSTS, 1000.0),
    # (a neighbour's stage-1 start value is one chunk of release off during a release: 32 delta = 0.116 dB here, 15 x the bound)
    ("speech_44k", ("carry2", 3 * xr.SCAN), xc.NOISE, 1000.0), ("speech_44k", "neighbour1", xc.BURSTS, 10.0),
    ("speech_44k", "neighbour2", xc.BURSTS, 1000.0), ("speech_44k", "boost", xc.RAMP, 100.0),
    ("gate_8k", ("carry1", xr.SCAN), xc.BURSTS, 1e4), ("gate_8k", ("carry1", 2 * xr.SCAN), xc.NOISE, 1e4), ("gate_8k", ("carry2", xr.SCAN), xc.BURSTS, 1e4),
    ("gate_8k", ("carry2", 3 * xr.SCAN), xc.NOISE, 1e4), ("gate_8k", "neighbour1", xc.BURSTS, 1e4), ("gate_8k", "neighbour2", xc.BURSTS, 1e4),
    ("slow_192k", ("carry1", xr.SCAN), xc.BURSTS, 100.0), ("slow_192k", ("carry2", 2 * xr.SCAN), xc.BURSTS, 100.0),
]


@pytest.mark.parametrize("name,fault,row,factor", FAULTS)
def test_a_fault_lands_far_outside_the_bound(name, fault, row, factor):
    c = xc.case(name)
    m = xr.model(c.x, c.f, fault)
    over = xc.over_bound(c, "yl", m["yl"], c.ref.yl)
    print(f"\n{name} {fault} on {xc.NAMES[row]}: yL {over[row]:.1f} x the bound, {np.abs(m['yl'][row] - c.ref.yl[row]).max():.3f} dB")
    assert over[row] >= factor, (name, fault, xc.NAMES[row], over)
    assert not over[[xc.QUIET, xc.ZERO]].any()


def test_the_boost_fault_is_void_without_a_hold():
    c = xc.case("gate_8k")
    assert c.hold == 0 and float(c.f["Bh"]) == 0.0
    a, b = xr.model(c.x, c.f), xr.model(c.x, c.f, "boost")
    assert np.array_equal(a["yl"], b["yl"])
