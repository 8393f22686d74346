"""The fetch-time compressor without a GPU (include/stn.h "compressor"): the host-only entry points (coefficients,
static curve, refusals), the float64 reference's step response, the parsers of the binding, the command line and the service, the
OutputSettings field, and the numpy model of the GPU's decomposition (tests/compressor_ref.py) on the inputs and bounds of the kernel
tests (tests/compressor_cases.py): the model stays inside the bound, and a scan that drops a carry or hands a chunk its neighbour's start
value lands far outside it."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.output import OutputSettings
import compressor_cases as cc
import compressor_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
SPEECH = binding.COMPRESSOR_SPEECH


# ---- host-only entry points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 44100, 192000])
def test_coefs_against_the_closed_form(rate):
    for setting in (SPEECH, (-30.0, 20.0, 0.0, 0.1, 10.0, 6.0), (-20.0, 4.0, 12.0, 300.0, 3000.0, -3.0)):
        k, k32 = binding.compressor_coefs(setting, rate)
        for i, ms in enumerate(setting[3:5]):
            want = 1.0 - np.exp(-1000.0 / (float(np.float32(ms)) * rate))  # k = 1 - exp(-1 / (tau rate)), tau in seconds
            assert abs(k[i] / want - 1) < 1e-9, (rate, ms, k[i], want)  # (1 - exp cancels up to seven of its digits at a 3 s release; expm1 does not)
            assert k[i] == cr.k_of(ms, rate) and k32[i] == np.float32(k[i])
        f = cr.coefs(setting, rate)
        assert k32[0] == f["kA"] and k32[1] == f["kR"]
    # the k form keeps what alpha = 1 - k loses: at a 3 s release and 192 kHz alpha's fp32 neighbours are about 3 % apart in time constant
    k = cr.k_of(3000.0, 192000)
    alpha = np.float32(1.0 - k)
    tau = lambda a: -1.0 / np.log(float(a))
    assert abs(tau(np.nextafter(alpha, np.float32(0))) / tau(alpha) - 1) > 0.02
    assert abs((1.0 / -np.log1p(-float(np.float32(k)))) / (1.0 / -np.log1p(-k)) - 1) < 1e-7
    with pytest.raises(binding.StnError):
        binding.compressor_coefs(SPEECH, 7999)


def test_static_curve():
    T, R, K, mk = -24.0, 3.0, 6.0, 2.0
    c = (T, R, K, 5.0, 120.0, mk)
    x = np.linspace(-90.0, 0.0, 9001)
    y = binding.compressor_curve(c, x)
    below, above = x < T - K / 2, x > T + K / 2
    assert np.array_equal(y[below], x[below] + mk)                                                       # identity below the knee
    slope = 1.0 + float(np.float32(1.0 / R - 1.0))                                                       # 1 / ratio, as the fp32 S = 1 / ratio - 1 holds it
    assert abs(slope - 1 / R) < 1e-7 and np.allclose(np.diff(y[above]) / np.diff(x[above]), slope, rtol=0, atol=1e-9)  # slope 1 / ratio above it
    assert np.allclose(y[above], T + (x[above] - T) / R + mk, rtol=0, atol=1e-5)
    h = 1e-6
    for edge, slope in ((T - K / 2, 1.0), (T + K / 2, 1 / R)):                                           # value and slope continuous at both knee ends
        lo, mid, hi = binding.compressor_curve(c, [edge - h, edge, edge + h])
        assert abs(hi - mid) < 2 * h and abs(mid - lo) < 2 * h
        assert abs((mid - lo) / h - (hi - mid) / h) < 1e-4 and abs((hi - lo) / (2 * h) - slope) < 1e-4, (edge, lo, mid, hi)
    assert np.all(np.diff(y) > 0)
    assert np.array_equal(binding.compressor_curve((T, 1.0, K, 5.0, 120.0, 0.0), x), x)                  # ratio 1 is the identity
    hard = binding.compressor_curve((T, R, 0.0, 5.0, 120.0, 0.0), x)                                     # knee 0 is the hard corner
    assert np.array_equal(hard[x <= T], x[x <= T]) and np.allclose(hard[x > T], T + (x[x > T] - T) / R, rtol=0, atol=1e-5)
    assert binding.compressor_curve((T, R, 0.0, 5.0, 120.0, 0.0), [T])[0] == T
    # the curve is what the reference's gain computer gives
    f = cr.coefs(c, 44100)
    amp = 10.0 ** (x[::50] / 20.0)
    z = cr.want(amp.astype(np.float32)[None, :], f)[0]
    xg = 20 * np.log10(np.maximum(amp.astype(np.float32).astype(np.float64), 1e-6))
    assert np.allclose(binding.compressor_curve(c, xg), xg - z + mk, rtol=0, atol=1e-12)


LIMITS = {"threshold_db": (-60.0, 0.0), "ratio": (1.0, 20.0), "knee_db": (0.0, 24.0), "attack_ms": (0.1, 300.0), "release_ms": (10.0, 3000.0),
          "makeup_db": (-12.0, 24.0)}
BAD = {"threshold_db": (-60.5, 0.5), "ratio": (0.99, 20.5), "knee_db": (-0.1, 24.5), "attack_ms": (0.09, 301.0), "release_ms": (9.0, 3001.0),
       "makeup_db": (-12.5, 24.5)}


def test_every_refusal_names_its_field():
    assert binding.compressor_error(SPEECH) == "" and binding.compressor_error(True, 48000) == ""
    lib = binding.load()
    for i, name in enumerate(binding.COMPRESSOR_FIELDS):
        for bad in BAD[name] + (float("nan"), float("inf")):
            s = list(SPEECH)
            s[i] = bad
            why = lib.stn_compressor_error(binding.ctypes.byref(binding.StnCompressor(*s)), 0).decode()  # (the C ABI: the binding stops a NaN itself)
            assert name in why and all(o not in why for o in binding.COMPRESSOR_FIELDS if o != name), (name, bad, why)
            if np.isfinite(bad):
                assert binding.compressor_error(tuple(s)) == why
                with pytest.raises(binding.StnError):
                    binding.compressor_curve(tuple(s), [0.0])
        for ok in LIMITS[name]:
            s = list(SPEECH)
            s[i] = ok
            assert binding.compressor_error(tuple(s)) == "", (name, ok)
    assert "rate" in binding.compressor_error(SPEECH, 7999)  # (a rate is only checked when one is given)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,attack_ms", [(8000, 5.0), (44100, 5.0), (44100, 0.5), (192000, 50.0)])
def test_step_response_of_the_reference(rate, attack_ms):
    """a step to 20 dB over the threshold reaches 1 - 1 / e of its final reduction within one sample of attack_ms"""
    c = (-30.0, 4.0, 0.0, attack_ms, 3000.0, 0.0)
    f = cr.coefs(c, rate)
    W = int(10 * attack_ms * rate / 1000)
    x = np.full((1, W), 10.0 ** (-10.0 / 20.0), np.float32)  # -10 dBFS: 20 dB over
    r = cr.Ref(x, f)
    final = 20.0 * (1 - 1 / 4.0)
    assert abs(r.z[0, 0] - final) < 1e-5 and np.all(np.diff(r.yl[0]) > 0)
    n = int(np.argmax(r.yl[0] >= (1 - np.exp(-1.0)) * final))  # the first sample at or above it, counted from 0: n + 1 samples in
    assert abs((n + 1) - attack_ms * rate / 1000.0) <= 1.0, (n, attack_ms * rate / 1000.0)
    assert abs(20 * np.log10(abs(r.y[0, -1] / x[0, -1])) + r.yl[0, -1]) < 1e-9


# ---- parsers ------------------------------------------------------------------------------------------------------------------------------------
def test_binding_parser():
    ca = binding.compressor_args
    assert ca(None) is None and ca(False) is None and ca(True) == SPEECH == (-24.0, 3.0, 6.0, 5.0, 120.0, 0.0)
    assert ca({"threshold_db": -18, "ratio": 2}) == (-18.0, 2.0, 6.0, 5.0, 120.0, 0.0) and ca({}) == SPEECH
    assert ca((-20, 4, 0, 1, 50, 3)) == (-20.0, 4.0, 0.0, 1.0, 50.0, 3.0) and ca([np.float32(-20), 4, 0, 1, 50, np.int64(3)]) == (-20.0, 4.0, 0.0, 1.0, 50.0, 3.0)
    assert ca(None, preset="speech") == SPEECH and ca({"ratio": 5}, preset="speech")[1] == 5.0
    assert all(type(v) is float for v in ca((-20, 4, 0, 1, 50, 3)))
    for bad, word in (({"threshold": -20}, "threshold"), ((1, 2, 3), "6-tuple"), ({"ratio": "3"}, "ratio"), ({"knee_db": float("nan")}, "knee_db"),
                      ({"ratio": True}, "ratio"), (3.0, "6-tuple"), ((-20, 4, 0, 1, 50, None), "makeup_db")):
        with pytest.raises(ValueError) as ei:
            ca(bad)
        assert word in str(ei.value), (bad, str(ei.value))
    with pytest.raises(ValueError) as ei:
        ca(True, preset="music")
    assert "speech" in str(ei.value)


def test_command_line_spelling():
    p = binding.parse_compressor_spec
    assert p("-20:4") == (-20.0, 4.0, 6.0, 5.0, 120.0, 0.0) and p("-20:4:0") == (-20.0, 4.0, 0.0, 5.0, 120.0, 0.0)
    assert p("-20:4:3:1:50") == (-20.0, 4.0, 3.0, 1.0, 50.0, 0.0) and p("-20:4:3:1:50:-2.5") == (-20.0, 4.0, 3.0, 1.0, 50.0, -2.5)
    assert binding.compressor_args("-18:2") == (-18.0, 2.0) + SPEECH[2:]
    for bad in ("-20", "-20:4:3:1:50:0:9", "-20:x", ":4", ""):
        with pytest.raises(ValueError) as ei:
            p(bad)
        assert "THRESHOLD" in str(ei.value)
    # the C++ host's parser spells the same errors, before any device is touched
    if os.path.exists(CLI):
        for args, word in ((["--compressor", "-20"], "THRESHOLD:RATIO"), (["--compressor", "-20:x"], "must be numbers"), (["--compressor-preset", "music"], "speech")):
            r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)
            assert r.returncode == 1 and word in r.stderr, (args, r.stderr)


def test_service_key():
    from supertonic_amd import service
    key = lambda **kw: service.batch_key(44100, 5, 1.05, **kw)
    assert key().settings.compressor is None and key(compressor=False).settings.compressor is False
    assert key(compressor=True) == key(compressor=SPEECH) == key(compressor={}) and key(compressor=True).settings.compressor == SPEECH
    assert key(compressor=True) != key() and key(compressor=True) != key(compressor=False) and key(compressor={"ratio": 4}) != key(compressor=True)
    assert key(compressor={"ratio": 4}).settings.kwargs() == {"compressor": (-24.0, 4.0, 6.0, 5.0, 120.0, 0.0)}
    assert key(compressor=False).settings.kwargs() == {"compressor": False}
    for bad, word in (({"ratio": 40}, "ratio"), ({"attack": 1}, "attack"), ({"release_ms": 1}, "release_ms")):
        with pytest.raises(ValueError) as ei:
            key(compressor=bad)
        assert word in str(ei.value)
    import inspect
    assert list(inspect.signature(service.batch_key).parameters)[-1] == "compressor"  # appended last


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
    assert P().compressor is None and P(compressor=False).compressor is False and P(compressor=None).compressor is None
    assert P(compressor=True).compressor == SPEECH and P(compressor={"ratio": 4}).compressor == (-24.0, 4.0, 6.0, 5.0, 120.0, 0.0)
    assert P(compressor=list(SPEECH)) == P(compressor=True) and hash(P(compressor=True)) == hash(P(compressor=SPEECH))
    with pytest.raises(ValueError):
        P(compressor={"threshold": 1})
    assert OutputSettings.OFF.compressor is None and OutputSettings.ALL_OFF.compressor is False
    unset = [f.name for f in dataclasses.fields(OutputSettings) if getattr(OutputSettings.ALL_OFF, f.name) is None]
    assert unset == [] and dataclasses.replace(OutputSettings.ALL_OFF, compressor=None) == OutputSettings.OFF
    assert P(compressor=True).kwargs() == {"compressor": SPEECH} and P(**P(compressor=True).kwargs()) == P(compressor=True)
    assert P(compressor=False).over(P(compressor=True)).compressor is False and P().over(P(compressor=True)).compressor == SPEECH


def test_output_settings_apply_order_and_restore():
    e = _Engine()
    P = OutputSettings.parse
    P(output_rate=16000, filters=[("highpass", 80)], compressor=True, loudness=-16).apply(e)
    names = [c[0] for c in e.calls]
    assert names == ["set_filters", "set_output_rate", "set_filters", "set_compressor", "set_loudness"]  # right after the filter chain
    assert e.calls[3] == ("set_compressor", (SPEECH,))
    e.calls.clear()
    P(compressor=False).apply(e)
    assert e.calls == [("set_compressor", (None,))]
    # a per-call compressor over an instance that has none is put back to off: the instance's settings name every field (ALL_OFF)
    base = P().over(OutputSettings.ALL_OFF)
    e.calls.clear()
    with P(compressor={"ratio": 4}).applied(e, base) as now:
        assert now.compressor == (-24.0, 4.0, 6.0, 5.0, 120.0, 0.0) and e.calls == [("set_compressor", (now.compressor,))]
    assert e.calls[-1] == ("set_compressor", (None,)) and len(e.calls) == 2
    # and over an instance that has one, back to the instance's
    base = P(compressor=True).over(OutputSettings.ALL_OFF)
    e.calls.clear()
    with P(compressor=False).applied(e, base):
        pass
    assert e.calls == [("set_compressor", (None,)), ("set_compressor", (SPEECH,))]


# ---- the decomposition ---------------------------------------------------------------------------------------------------------------------------
def _over(c, m):
    st = c.ref.states(c.f, cc.W_MAX)
    out = {k: cc.over_bound(c, k, m[k], st[k]) for k in cc.STATES}
    out["yl"] = cc.over_bound(c, "yl", m["yl"], c.ref.yl)
    out["y"] = cc.over_bound(c, "y", m["y"], c.ref.y)
    return out


@pytest.mark.parametrize("name", list(cc.SETTINGS))
def test_model_of_the_decomposition_stays_inside_the_bound(name):
    c = cc.case(name)
    cc.conditions(c)
    assert all(v > 0 for k in ("yl", "y") for v in c.dev[k][list(cc.LOUD)])  # the restatement does deviate where there is reduction
    assert not c.dev["yl"][[cc.QUIET, cc.ZERO]].any() and not c.bound["yl"][[cc.QUIET, cc.ZERO]].any()  # and the quiet rows' states must be exact
    over = _over(c, cr.model(c.x, c.f))
    worst = {k: float(v.max()) for k, v in over.items()}
    print(f"\n{name}: model over bound " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    for W in (cc.SPAN + 1, cc.TILE - cr.CHUNK):  # the model at a narrower W is the model cut there
        m = cr.model(c.x[:, :W], c.f)
        full = cr.model(c.x, c.f)
        assert np.array_equal(m["y"], full["y"][:, :W]) and np.array_equal(m["s2_start"], full["s2_start"][:, : cr.chunks(W)])


# measured on the model (over bound, in yL, on the rows named): what a fault costs.  A lost carry of stage 1 shows only where the chunk
# behind the seam does not reach the lost level again by itself (the detector is a maximum): on noise, not on a steady tone.  At a 3 s
# release and 300 ms attack a chunk's neighbour holds almost the same values, so that fault stays inside the bound there: it is the fast
# settings that catch it.
FAULTS = [
    ("speech_44k", ("carry1", cr.SCAN), cc.NOISE, 100.0), ("speech_44k", ("carry2", 2 * cr.SCAN), cc.BURSTS, 1e4),
    ("speech_44k", ("carry1", cr.WG), cc.NOISE, 1000.0), ("speech_44k", "neighbour1", cc.NOISE, 1000.0), ("speech_44k", "neighbour2", cc.BURSTS, 1e4),
    ("hard_8k", ("carry1", cr.SCAN), cc.NOISE, 1e4), ("hard_8k", ("carry2", 2 * cr.SCAN), cc.BURSTS, 1e4), ("hard_8k", "neighbour1", cc.BURSTS, 1e4),
    ("hard_8k", "neighbour2", cc.BURSTS, 1e4),
    ("slow_192k", ("carry1", cr.SCAN), cc.NOISE, 4.0), ("slow_192k", ("carry2", 2 * cr.SCAN), cc.BURSTS, 1000.0), ("slow_192k", ("carry2", 3 * cr.SCAN), cc.NOISE, 1000.0),
]


@pytest.mark.parametrize("name,fault,row,factor", FAULTS)
def test_a_faulty_scan_lands_far_outside_the_bound(name, fault, row, factor):
    c = cc.case(name)
    m = cr.model(c.x, c.f, fault)
    over = cc.over_bound(c, "yl", m["yl"], c.ref.yl)
    print(f"\n{name} {fault} on {cc.NAMES[row]}: yL {over[row]:.1f} x the bound, {np.abs(m['yl'][row] - c.ref.yl[row]).max():.3f} dB")
    assert over[row] >= factor, (name, fault, cc.NAMES[row], over)
    assert not over[[cc.QUIET, cc.ZERO]].any()
