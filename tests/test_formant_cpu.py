"""The formant correction's host arithmetic and its float64 reference on the CPU (include/stn.h "formant"; csrc/host/formant.cpp;
tests/formant_ref.py): the plan, stn_formant_lpc against numpy.linalg.solve, what the rule is for on a steady
vowel, the identity, and that the bounds of tests/test_gpu_formant_kernels.py catch four mutants of the reference while a float32
restatement stays inside them."""
import numpy as np
import pytest

from supertonic_amd import binding
import formant_cases as fc
import formant_ref as fr
import pitch_cases as pc
import pitch_ref as pr


# ---- plan ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz,p", [(8000, 10), (16000, 18), (24000, 26), (44100, 48), (48000, 48), (96000, 48), (192000, 48)])
def test_plan(hz, p):
    for W in (0, 1, pr.hop(hz) - 1, pr.hop(hz), 5 * pr.hop(hz) + 1, 233472):
        got = binding.formant_plan(hz, W)
        want = fr.plan(hz, W)
        assert got["p"] == p == fr.order(hz) and got["H"] == want["H"] == binding.pitch_plan(hz, W, 1, 1)["H"] and got["N"] == 2 * got["H"]
        assert got["frames"] == want["frames"] == -(-W // got["H"]) + 1
        k = np.arange(p + 1)
        assert got["lag"].shape == (p + 1,) and got["lag"][0] == 1.0
        assert np.allclose(got["lag"], np.exp(-0.5 * (2.0 * np.pi * 60.0 * k / hz) ** 2), rtol=4e-16, atol=0)
    assert binding.formant_plan(22050, 10)["p"] == 26 and binding.formant_plan(11025, 10)["p"] == 14
    for bad in ((7999, 10), (192001, 10), (16000, -1)):
        with pytest.raises(binding.StnError):
            binding.formant_plan(*bad)


# ---- the recursion ------------------------------------------------------------------------------------------------------------------------------
def _frame_lags(hz):
    """the lags of some vowel, harmonic and noise frames of formant_cases.rows(hz), and of an all-zero frame"""
    x, n, names = fc.rows(hz)
    p = fr.order(hz)
    out = []
    for name in ("vowel", "harmonic", "noise", "zero"):
        r = names.index(name)
        R = fr.lags(fr.frames32(x[r], n[r], hz), p)
        out += [(name, m, R[m]) for m in (0, 3, R.shape[0] // 2, R.shape[0] - 2)]
    return out


@pytest.mark.parametrize("hz", (8000, 16000, 44100))
def test_lpc_against_a_dense_solve(hz):
    """The Gaussian lag window keeps the Toeplitz matrix positive semi-definite and the white-noise term lifts it: lambda_min >= 1e-4
    R[0], lambda_max <= (p + 1) 1.0001 R[0], a condition number of at most 4.9e5 at p = 48.  |da| <= 1e-8 max|a|: 4.9e5 x 48 x 2^-53
    with a factor of 4."""
    p = fr.order(hz)
    worst = 0.0
    for name, m, R in _frame_lags(hz):
        a, err, refl = binding.formant_lpc(hz, R)
        Rc = fr.condition(R[None, :], hz)[0]
        T = Rc[np.abs(np.arange(p + 1)[:, None] - np.arange(p + 1)[None, :])]
        ev = np.linalg.eigvalsh(T)
        assert ev[0] >= 1e-4 * R[0] * (1 - 1e-9) and ev[-1] <= (p + 1) * 1.0001 * R[0] + 1e-8, (name, m, ev[0], ev[-1])
        want = np.concatenate(([1.0], np.linalg.solve(T[:p, :p], -Rc[1:])))
        assert np.max(np.abs(a - want)) <= 1e-8 * np.max(np.abs(want)), (name, m)
        worst = max(worst, float(np.max(np.abs(a - want)) / np.max(np.abs(want))))
        assert np.all(np.abs(refl) < 1.0) and err > 0.0
        assert abs(err - (Rc[0] + Rc[1:] @ want[1:])) <= 1e-8 * Rc[0]
        ra, re, rk = fr.levinson(Rc)
        # (the reference's own recursion is held to the same bound against the same solve)
        assert np.max(np.abs(ra[0] - want)) <= 1e-8 * np.max(np.abs(want)) and abs(re[0] - err) <= 1e-8 * Rc[0]
        if name == "zero":
            assert np.all(a[1:] == 0.0) and a[0] == 1.0 and err == 1e-9
    print(f"{hz} Hz: largest |da| / max|a| against the dense solve {worst:.3g}")
    with pytest.raises(binding.StnError):
        binding.formant_lpc(hz, np.ones(50))


# ---- what the rule is for -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semitones", sorted(fc.SHIFTS))
@pytest.mark.parametrize("hz", fc.PROPERTY_RATES)
def test_the_envelope_comes_back_and_the_period_stays(hz, semitones):
    """The steady vowel (32 hops) shifted by the float64 pitch reference and corrected by the float64 formant reference: the RMS over
    100 Hz .. 5 kHz (0.4 hz at 8 kHz) of the difference of the mean-removed LPC log envelopes to the original's is at most 0.6 of the
    uncorrected row's (recorded: 0.23 to 0.49), and the autocorrelation period is the shifted row's.  The period is searched from
    100 Hz as long as the shifted fundamental lies above it (+4: 163.9 Hz); the -5 row's lies at 98.2 Hz, below that edge, where a
    search from 100 Hz can only lock onto a harmonic that the formants pick (lags 17 against 15 at 8 kHz, 92 against 84 at 44.1 kHz),
    so there the search runs over 3/4 to 3/2 of the fundamental, as tests/test_gpu_pitch_kernels.py searches: that still excludes the
    sub-octave and does contain the period.  The integer lags are equal except at 44.1 kHz, -5, where the shifted period is 452.51
    samples and the two rows' peaks fall on either side of the half (452 and 453): so the peaks are refined by a parabola and the
    periods held to half a sample of each other: half the lag grid, where equal integer lags allow periods up to a sample apart."""
    x, y, out = fc.property_rows(hz, semitones)
    unc, cor = fc.envelope_figures(hz, semitones)
    lo, hi = pc.steady(hz, len(x))
    print(f"{hz} Hz {semitones:+g}: envelope distance {unc:.3f} -> {cor:.3f} dB (ratio {cor / unc:.3f}; recorded {fc.ENVELOPE_DB[hz, semitones]})")
    assert np.all(np.isfinite(out)) and cor <= 0.6 * unc
    assert abs(unc - fc.ENVELOPE_DB[hz, semitones][0]) <= 2e-3 and abs(cor - fc.ENVELOPE_DB[hz, semitones][1]) <= 2e-3
    a, b = fc.SHIFTS[semitones]
    f = (hz / max(1, int(hz / 130.0))) * a / b
    f_lo, f_hi = (100.0, 600.0) if f > 100.0 else (0.75 * f, 1.5 * f)
    (per_y, lag_y), (per_o, lag_o) = fr.period(y, hz, lo, hi, f_lo, f_hi), fr.period(out, hz, lo, hi, f_lo, f_hi)
    print(f"{hz} Hz {semitones:+g}: period {per_y:.3f} (lag {lag_y}) -> {per_o:.3f} (lag {lag_o}); the shifted pulse train's is {hz / f:.3f}")
    assert abs(per_o - per_y) <= 0.5 and abs(per_y - hz / f) <= 0.5, (per_y, per_o, hz / f)
    assert lag_o == lag_y or abs(hz / f - np.floor(hz / f) - 0.5) < 0.05, (lag_y, lag_o, hz / f)


@pytest.mark.parametrize("hz", (8000, 16000, 44100, 24000))
def test_identity(hz):
    """formant(x, x) == x to 1e-7: ax == cy, the FIR and the IIR start on the same sample, and what is left is the float32 rounding of
    the tables"""
    x, n, names = fc.rows(hz)
    for name in ("vowel", "harmonic", "noise", "harmonic[:1]", "vowel+nan"):
        r = names.index(name)
        out, t = fr.formant(x[r], x[r], n[r], hz)
        want = np.where(np.arange(x.shape[1]) < n[r], np.nan_to_num(x[r].astype(np.float64)), 0.0)
        assert np.array_equal(t["ax"], t["cy"]) and np.all(t["g"] == 1.0)
        assert np.max(np.abs(out - want)) <= 1e-7, (name, np.max(np.abs(out - want)))


# ---- the GPU tests' bounds bite -----------------------------------------------------------------------------------------------------------------
def _table_excess(t, ref):
    """the largest error / bound of tables t against ref under the GPU tests' table bound"""
    worst = 0.0
    for key in ("ax", "cy"):
        r = ref[key].astype(np.float64)
        tol = 2.0 ** -23 * np.abs(r) + 1e-6 * np.max(np.abs(r), axis=1, keepdims=True)
        worst = max(worst, float(np.max(np.abs(t[key].astype(np.float64) - r) / tol)))
    return worst


@pytest.mark.parametrize("hz", (16000, 44100))
def test_mutants_land_outside_the_gpu_bounds_and_float32_inside(hz):
    """As the GPU tests judge a device: the tables against the reference's, the output against the float64 reference run on the judged
    tables, within 4 x formant_cases.FP32_DEVIATION.  A mutant of the tables fails the first, a mutant of the filter the second; the
    float32 restatement passes both."""
    s = 4.0
    x, n, names = fc.rows(hz)
    y = fc.shifted(hz, s)
    for name in ("vowel", "harmonic", "noise"):
        r = names.index(name)
        bound = 4.0 * fc.FP32_DEVIATION[hz, s][r]
        ref = fr.tables(x[r], y[r], n[r], hz)
        want = fr.apply_tables(y[r], n[r], hz, ref["ax"], ref["cy"])
        dev = fc.fp32_deviation(hz, s, r)
        assert abs(dev - fc.FP32_DEVIATION[hz, s][r]) <= 0.006 * dev, (name, dev)  # (the record is this measurement to three digits)
        assert 0.0 < dev <= bound / 4.0 * 1.006
        for mutant in fr.MUTANTS:
            t = fr.tables(x[r], y[r], n[r], hz, mutant)
            table_excess = _table_excess(t, ref)
            got = fr.apply_tables(y[r], n[r], hz, t["ax"], t["cy"], np.float64, mutant)
            out_excess = float(np.max(np.abs(got - fr.apply_tables(y[r], n[r], hz, t["ax"], t["cy"])))) / bound
            print(f"{hz} Hz {name} {mutant}: tables {table_excess:.3g} x the bound, output {out_excess:.3g} x the bound")
            if mutant in ("no-conditioning", "ay-both-sides"):
                assert table_excess > 100.0 and out_excess == 0.0, (name, mutant)
            else:
                assert table_excess == 0.0 and out_excess > 100.0, (name, mutant)
        assert np.max(np.abs(want)) > 0.1
