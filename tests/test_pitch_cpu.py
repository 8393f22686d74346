"""The pitch shift's host arithmetic and its float64 reference (include/stn.h "pitch"), without a GPU: the ratio
of a shift against two searches in Python, the geometry and the window against their formulas, what the reference does to a steady
harmonic row with and without the search, and that the decision margin the GPU tests use catches a search over half the candidates."""
import math

import numpy as np
import pytest

from supertonic_amd import binding
import pitch_cases as pc
import pitch_ref as pr


# ---- stn_pitch_ratio ------------------------------------------------------------------------------------------------------------------------
def test_ratio_exact_cases():
    assert binding.pitch_ratio(0) == (1, 1)
    assert binding.pitch_ratio(12) == (2, 1)
    assert binding.pitch_ratio(-12) == (1, 2)
    for s, ab in pc.SHIFTS.items():
        assert binding.pitch_ratio(s) == ab


def test_ratio_sweep_is_the_closest_fraction_and_within_1_36_cents():
    worst = 0.0
    for i in range(4801):
        s = -12.0 + i * 0.005
        a, b = binding.pitch_ratio(s)
        assert 1 <= a <= 640 and 1 <= b <= 640 and math.gcd(a, b) == 1, (s, a, b)
        assert (a, b) == pr.ratio_brute(s), (s, a, b)
        worst = max(worst, abs(pr.cents(a, b, s)))
    print(f"worst realised error over 4801 values: {worst:.3f} cents")
    assert worst <= 1.36


def test_ratio_against_the_full_table():
    for i in range(0, 4801, 160):
        s = -12.0 + i * 0.005
        assert binding.pitch_ratio(s) == pr.ratio_exhaustive(s), s


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), 12.01, -12.01])
def test_ratio_refusals(bad):
    with pytest.raises(binding.StnError):
        binding.pitch_ratio(bad)
    why = binding.pitch_error(bad)
    assert "[-12, 12]" in why and "semitones" in why
    with pytest.raises(ValueError, match="semitones"):
        binding.pitch_args(bad)
    assert binding.pitch_error(12.0) == "" and binding.pitch_error(-12.0) == "" and binding.pitch_error(0.0) == ""
    assert binding.pitch_args(None) == 0.0 and binding.pitch_args(False) == 0.0 and binding.pitch_args(-3) == -3.0
    with pytest.raises(ValueError):
        binding.pitch_args("high")


# ---- stn_pitch_plan, stn_pitch_window -----------------------------------------------------------------------------------------------------------
def test_plan_against_the_formulas():
    for hz, H in ((8000, 64), (16000, 128), (22050, 256), (24000, 256), (32000, 256), (44100, 512), (48000, 512), (96000, 1024), (192000, 2048)):
        assert 128 * H >= hz > 128 * (H // 2)
        for W in (0, 1, H - 1, 2 * H, 8192, 352800):
            for a, b in pc.RATIOS + ((1, 1), (640, 321)):
                p = binding.pitch_plan(hz, W, a, b)
                Ws = -(-W * a // b)
                assert p == dict(H=H, N=2 * H, delta=3 * H // 4, M=Ws // H + 2, Ws=Ws), (hz, W, a, b, p)
                assert p == {**pr.plan(hz, W, a, b)}
    for bad in ((7999, 10, 1, 1), (192001, 10, 1, 1), (16000, -1, 1, 1), (16000, 10, 0, 1), (16000, 10, 1, 641)):
        with pytest.raises(binding.StnError):
            binding.pitch_plan(*bad)


def test_window_is_the_periodic_hann_and_sums_to_one():
    for hz in (8000, 16000, 24000, 44100, 48000, 192000):
        w = binding.pitch_window(hz)
        H = pr.hop(hz)
        assert w.dtype == np.float32 and w.shape == (2 * H,)
        assert np.array_equal(w, pr.window(hz).astype(np.float32))
        assert w[0] == 0.0 and w[H] == 1.0
        assert np.max(np.abs(w[:H].astype(np.float64) + w[H:].astype(np.float64) - 1.0)) <= 2.0 ** -23
    with pytest.raises(binding.StnError):
        binding.pitch_window(7999)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", pc.RATES)
def test_reference_keeps_a_steady_row_flat_and_plain_overlap_add_does_not(hz):
    """Per-10-ms RMS of the steady part in dB against the median block.  Ten milliseconds are 2.07 periods of 207 Hz, so the row's own
    figure is not 0 and depends on where the blocks start: `own` is its range over every block phase (about -0.1 .. +0.65 dB).  WSOLA
    by 63/50 must stay inside that range widened by 0.1 dB: a splice at a similarity maximum is off by at most half a sample, which
    costs the fifth harmonic cos(0.2) = -0.17 dB at 8 kHz and the row, of whose energy that harmonic holds 3 %, under 0.01 dB.  The
    same overlap-add with every offset 0 adds grains at whatever phase they have: its deepest block lies at least 0.5 dB under the
    range (measured: -1.0 .. -2.4 dB)."""
    x = pc.harmonic(hz, pc.W[hz])
    y, delta, _ = pr.stretch(x, None, hz, 63, 50)
    y0 = pr.ola(x, None, hz, 63, 50, np.zeros_like(delta))
    lo, hi = pc.steady(hz, len(x))
    phases = [pr.envelope_db(x, hz, lo + k, hi) for k in range(hz // 100)]
    own = (min(p[0] for p in phases), max(p[1] for p in phases))
    lo, hi = pc.steady(hz, len(y))
    ws, z = pr.envelope_db(y, hz, lo, hi), pr.envelope_db(y0, hz, lo, hi)
    print(f"{hz} Hz: row {own}, wsola {ws}, plain overlap-add {z}")
    assert len(y) == -(-len(x) * 63 // 50) and np.any(delta != 0)
    assert own[0] - 0.1 <= ws[0] and ws[1] <= own[1] + 0.1
    assert z[0] <= own[0] - 0.5


def test_reference_ties_and_spans():
    hz = 16000
    x, n, names = pc.rows(hz)
    zero = names.index("zero")
    for a, b in pc.RATIOS:
        d, s = pr.search(x[zero], n[zero], hz, a, b)
        assert not d.any() and not s.any()
        assert not pr.ola(x[zero], n[zero], hz, a, b, d).any()
    # a row's result depends on its own samples only: NaN behind the span changes nothing
    r = names.index("vowel+nan")
    clean = np.where(np.isnan(x[r]), 0.0, x[r])
    ya, da, _ = pr.stretch(x[r], n[r], hz, 3, 2)
    yb, db, _ = pr.stretch(clean[:n[r]], None, hz, 3, 2)
    assert np.all(np.isfinite(ya)) and np.array_equal(da[:len(db)], db) and np.array_equal(ya[:len(yb)], yb)
    # the equal scores inside the vowel's gaps give 0
    v = names.index("vowel")
    d, _ = pr.search(x[v], None, hz, 3, 2)
    ties = pr.tie_frames(x[v], None, hz, 3, 2, d)
    assert ties and all(d[m] == 0 for m in ties)


def test_pick_order():
    s = np.zeros(7)
    assert pr.pick(s, 3) == 0
    s[[1, 5]] = 1.0  # d = -2 and +2
    assert pr.pick(s, 3) == -2
    s[4] = 1.0  # d = +1
    assert pr.pick(s, 3) == 1


@pytest.mark.parametrize("hz", pc.RATES)
def test_the_decision_margin_catches_a_search_over_half_the_candidates(hz):
    """The mutant searches d <= 0 only.  Judged frame by frame as the GPU's table is (decision_gaps), the reference's own table passes
    everywhere, and the mutant's fails on both rows at the ratios above 1.  (Below 1 the analysis hop exceeds the radius, and a whole
    period, 213 samples of the harmonic row at 44.1 kHz, fits into half the range: the mutant may then find an equal match one period
    earlier, which is no fault, so nothing is asked of it there.)"""
    x, n, names = pc.rows(hz)
    D = pr.plan(hz, pc.W[hz], 1, 1)["delta"]
    half = np.arange(-D, D + 1) <= 0
    for r in (names.index("harmonic"), names.index("vowel")):
        for a, b in pc.RATIOS:
            d, _ = pr.search(x[r], n[r], hz, a, b)
            gap, margin = pr.decision_gaps(x[r], n[r], hz, a, b, d)
            assert np.all(gap <= margin), (names[r], a, b)
            dm, _ = pr.search(x[r], n[r], hz, a, b, allowed=half)
            gap, margin = pr.decision_gaps(x[r], n[r], hz, a, b, dm)
            caught = int(np.sum(gap > margin))
            if a > b:  # (3/2, 635/504, 640/639)
                assert caught >= 1, (names[r], a, b)


@pytest.mark.parametrize("hz", pc.WIDE_RATES)
def test_the_noise_row_rejects_a_search_blind_to_any_slice_of_the_candidates_or_to_either_end(hz):
    """The wide rows are sensitive where the rows above are not (on a periodic row an equally good candidate lies a period away, inside
    what a blind search still sees).  The search's workgroup takes the candidates T at a time: a search that never looks at one slice
    [k T, (k + 1) T) of them, or at d = +D alone (the last trip's one candidate at 96 and 192 kHz), or at d = -D alone, picks another
    offset on some frame of the noise row at 8/5 or at 4/7, and the decision margin the GPU tests apply rejects its table."""
    T, C = pc.search_threads(hz)
    x, n, names = pc.wide_rows(hz)
    r = names.index("noise")
    D = (C - 1) // 2
    assert (T, C) == {24000: (448, 385), 96000: (1024, 1537), 192000: (1024, 3073)}[hz]
    j = np.arange(C)
    blind = {f"slice {k}": (j < k * T) | (j >= (k + 1) * T) for k in range(-(-C // T))}
    blind["+D"], blind["-D"] = j != C - 1, j != 0
    for a, b in ((8, 5), (4, 7)):
        d, _ = pr.search(x[r], n[r], hz, a, b)
        gap, margin = pr.decision_gaps(x[r], n[r], hz, a, b, d)
        assert np.all(gap <= margin) and d[2 if a > b else 1] == (D if a > b else -D), (a, b, d[:4])
    for name, allowed in blind.items():
        rejected = False
        for a, b in ((8, 5), (4, 7)):
            if not rejected:
                d, _ = pr.search(x[r], n[r], hz, a, b, allowed=allowed)
                gap, margin = pr.decision_gaps(x[r], n[r], hz, a, b, d)
                rejected = bool(np.any(gap > margin))
        assert rejected, (hz, name)


def test_recorded_envelope_figures_exist_and_the_reference_moves_the_pitch():
    for hz in pc.RATES:
        for s, (a, b) in pc.SHIFTS.items():
            y = pc.reference_pitch(hz, s)
            assert len(y) == pc.W[hz]
            f = pc.F0 * a / b
            f0, lag = pr.autocorr_f0(y, hz, *pc.steady(hz, pc.W[hz]), f / 1.5, f * 1.5)
            assert abs(lag - hz / f) <= 0.5, (hz, s, lag, hz / f)
            assert 0.0 < pc.reference_envelope_db(hz, s) < 3.0
