"""The pitch report without a GPU (include/stn.h "f0"): the host rule (stn_f0_rule, stn_f0_stats_rule, stn_f0_plan)
against the float64 numpy contract (tests/f0_ref.py) on the case rows (tests/f0_cases.py), the parameter refusals, and what the GPU
test (tests/test_gpu_f0.py) leans on: how many frames of the case rows are undecidable, the curvature of d' that conditions the
parabola, the contract's own error on the pure tones, and how far the float64 pitch chain lands from the interval asked for."""
import math

import numpy as np
import pytest

from supertonic_amd import binding
import f0_cases as fc
import f0_ref as ref
import pitch_ref as pr

G = binding.f0_group()[0]


# ---- 1. the host rule is the contract ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", fc.RATES)
def test_rule_equals_the_float64_contract(hz):
    x, n = fc.case_rows(hz, G)
    for r, want in enumerate(fc.refs(hz, G)):
        f0, ap, lag = binding.f0_rule(x[r, : n[r]], hz, lags=True)
        assert f0.size == want["plan"]["frames"], (hz, r)
        assert np.array_equal(lag, want["lag"]), (hz, r, fc.NAMES[r])  # voicing and tau^ exactly
        assert np.array_equal(f0 > 0, want["f0"] > 0), (hz, r)
        v = want["f0"] > 0
        if v.any():
            assert np.max(np.abs(f0[v] / want["f0"][v] - 1.0)) <= 1e-9, (hz, r)
        assert np.all(f0[~v] == 0.0) and np.all(ap[~v] == 1.0)
        assert np.allclose(ap, want["ap"], rtol=1e-9, atol=1e-12), (hz, r)
        got, w = binding.f0_stats_rule(f0.astype(np.float32)), ref.stats(f0.astype(np.float32))
        assert got["frames"] == w["frames"] and got["voiced"] == w["voiced"], (hz, r)
        for key in ("median_hz", "min_hz", "max_hz"):
            assert float(got[key]) == w[key], (hz, r, key)  # elements of the fp32 track itself
        assert abs(float(got["mean_hz"]) - w["mean_hz"]) <= 2.0 ** -23 * max(w["mean_hz"], 1e-30), (hz, r)
    # the frame counts the rows were built for
    frames = [w["plan"]["frames"] for w in fc.refs(hz, G)]
    assert frames[:5] == [0, 0, 1, G, G + 1], frames
    assert n[5] % ref.plan(hz, 0)["k"] == ref.plan(hz, 0)["k"] - 1
    print(f"{hz} Hz: frames per row {frames}")


@pytest.mark.parametrize("hz,k", list(zip(fc.RATES, (1, 1, 2, 3, 12))) + [(31999, 1), (176400, 11)])
def test_plan(hz, k):
    for p in (None, {"fmin_hz": 30.0, "fmax_hz": 1000.0}, {"fmin_hz": 77.7, "fmax_hz": 333.3}):
        for n in (0, 1, 999, hz // 3, hz):
            got, want = binding.f0_plan(hz, n, p), ref.plan(hz, n, p)
            assert got == {key: want[key] for key in got}, (hz, n, p)
            assert got["k"] == k and want["ha"] < 32000.0 and got["tau_max"] <= 1067 and got["hop"] <= 320 and got["tau_min"] >= 8
    assert binding.f0_group()[1] >= 16384


def test_refusals_come_with_their_messages():
    assert binding.f0_error(16000) == "" and binding.f0_error(8000, {"fmin_hz": 30.0, "fmax_hz": 1000.0}) == ""
    assert binding.f0_params().threshold == np.float32(0.15) and binding.f0_params().gate_db == -60.0
    for hz, p, word in ((7999, None, "sample rate"), (192001, None, "sample rate"), (16000, {"fmin_hz": 29.9}, "30 <= fmin < fmax <= 1000"),
                        (16000, {"fmax_hz": 1000.5}, "30 <= fmin < fmax <= 1000"), (16000, {"fmin_hz": 500.0}, "30 <= fmin < fmax <= 1000"),
                        (16000, {"fmin_hz": float("nan")}, "fmin"), (16000, {"threshold": 0.0}, "threshold"), (16000, {"threshold": 1.0}, "threshold"),
                        (16000, {"gate_db": -120.5}, "gate"), (16000, {"gate_db": 0.5}, "gate")):
        why = binding.f0_error(hz, p)
        assert word in why, (hz, p, why)
        with pytest.raises(binding.StnError) as ei:
            binding.f0_plan(hz, 100, p)
        assert ei.value.code == -1 and word in str(ei.value)
        with pytest.raises(binding.StnError):
            binding.f0_rule(np.zeros(100, np.float32), hz, p)
    with pytest.raises(ValueError):
        binding.f0_params({"fmid_hz": 1.0})


# ---- 2. what the GPU test excludes is little -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", fc.RATES)
def test_few_frames_are_undecidable(hz):
    """at most 2 undecidable frames on the glide row, none on any other (a float64 sketch of the contract gave 1 of 57 on the glide at
    16 and 44.1 kHz)"""
    und = fc.undecidable(hz, G)
    print(f"{hz} Hz: undecidable frames per row {[len(u) for u in und]} (glide: {und[fc.GLIDE]})")
    for r, u in enumerate(und):
        assert len(u) <= (2 if r == fc.GLIDE else 0), (hz, fc.NAMES[r], u)


@pytest.mark.parametrize("hz", fc.RATES)
def test_curvature_conditions_the_parabola(hz):
    """The parabola's denominator a - 2b + c on the decidable voiced frames.  Around the dip of a periodic signal of fundamental f,
    d(tau) is A (1 - cos(2 pi f (tau - tau^) / ha)) summed over its harmonics, and d' divides by the mean of d over the lags up to
    tau^, which is A over whole periods: the second difference is (2 pi f / ha)^2 or more, f >= fmin.  Half of that is the floor, and
    the device bound (f0_ref.device_bound) must stay first order under it: its S at most a tenth of the curvature."""
    g = ref.plan(hz, 0)
    floor = 0.5 * (2.0 * math.pi * ref.DEFAULTS["fmin_hz"] / g["ha"]) ** 2
    und = fc.undecidable(hz, G)
    worst, worst_rel = math.inf, 0.0
    for r, w in enumerate(fc.refs(hz, G)):
        for t, lag in enumerate(w["lag"]):
            if lag == 0 or t in und[r]:
                continue
            dp = w["det"][t]["dp"]
            D = dp[lag - 1] - 2.0 * dp[lag] + dp[lag + 1]
            worst = min(worst, D)
            assert D >= floor, (hz, fc.NAMES[r], t, D, floor)
            rel, _ = ref.device_bound(w["det"][t], int(lag), w["plan"])
            _, S = ref.device_bound(w["det"][t], int(lag), w["plan"], terms=True)
            worst_rel = max(worst_rel, rel)
            assert math.isfinite(rel) and S <= 0.1 * D, (hz, fc.NAMES[r], t, S, D)
    print(f"{hz} Hz: smallest curvature {worst:.3e} (floor {floor:.3e}); largest device bound of f0 {worst_rel:.3e} relative")


# ---- 3. the contract's own error ---------------------------------------------------------------------------------------------------------------
def _tone_error(hz, r):
    w = fc.refs(hz, G)[r]
    f = w["f0"][w["f0"] > 0]
    return max(abs(ref.cents(v, fc.TONES[r])) for v in f), f.size, w["f0"].size


@pytest.mark.parametrize("hz", fc.RATES)
def test_contract_error_on_the_pure_tones(hz):
    """YIN's own bias on a pure tone (the parabola through three points of d'): under 0.4 cents at 16 kHz and above, 2.0 cents for 450 Hz
    at 8 kHz, every frame voiced"""
    for r in fc.TONES:
        worst, voiced, frames = _tone_error(hz, r)
        print(f"{hz} Hz, {fc.NAMES[r]}: worst frame {worst:.3f} cents, {voiced} of {frames} frames voiced")
        assert voiced == frames and frames > 40
        assert worst < (0.4 if hz >= 16000 else 2.0), (hz, r, worst)


def test_octave_trap_glide_noise_and_silence():
    for hz in fc.RATES:
        w = fc.refs(hz, G)
        trap = w[9]["f0"]
        assert np.all(np.abs(trap - 120.0) < 1.0), (hz, trap)  # not 240 Hz: the second harmonic's dip is no period of the whole
        glide = w[fc.GLIDE]["f0"]
        v = glide[glide > 0]
        assert v.size >= glide.size - 2 and v[0] < 112.0 and v[-1] > 270.0 and np.all(np.diff(v) > -1.0), (hz, glide)
        assert np.count_nonzero(w[fc.NOISE]["f0"]) == 0, hz
        tone = w[12]
        F = tone["f0"].size
        assert np.all(np.abs(tone["f0"][: F // 2] - 200.0) < 1.0) and np.all(tone["f0"][-F // 5:] == 0.0) and np.all(tone["ap"][-F // 5:] == 1.0)
        assert any(d["gated"] and d["run"][-1] == 0.0 for d in tone["det"])  # digital silence: the zero running sum, behind the gate


# ---- 4. the pitch stage's interval in float64 ------------------------------------------------------------------------------------------------
PITCH_HZ, PITCH_F, pitch_row, pitch_chain = fc.PITCH_HZ, fc.PITCH_F, fc.pitch_row, fc.pitch_chain


@pytest.mark.parametrize("semitones", [4.0, -3.0])
def test_reference_chain_moves_the_fundamental_by_the_interval(semitones):
    """The median of the shifted tone's track against 150 * a / b (the ratio stn_pitch_ratio chose: within 1.36 cents of 2^(s / 12), so
    that allowance is taken out by measuring against the ratio itself).  Bound: twice the contract's own error on the unshifted tone,
    measured here: the shifted and the unshifted tone each bring that error, and they add."""
    f0, _, _ = ref.track(pitch_row(), PITCH_HZ)
    assert np.all(f0 > 0)
    own = max(abs(ref.cents(v, PITCH_F)) for v in f0)
    y, (a, b) = pitch_chain(semitones)
    assert abs(pr.cents(a, b, semitones)) <= 1.36
    t, _, _ = ref.track(y, PITCH_HZ)
    st = ref.stats(t)
    off = ref.cents(st["median_hz"], PITCH_F * a / b)
    print(f"{semitones:+} st: ratio {a}/{b}, median {st['median_hz']:.4f} Hz against {PITCH_F * a / b:.4f} ({off:+.3f} cents), voiced {st['voiced']} of "
          f"{st['frames']}; the contract's own error on the unshifted tone {own:.3f} cents, bound {2 * own:.3f}")
    assert st["voiced"] >= st["frames"] - 2
    assert abs(off) <= 2.0 * own, (semitones, off, own)
