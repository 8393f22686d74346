"""The pitch shift's kernels on an MI355X at op level (kernels_pitch.hip, the capped resample launch; include/stn.h "pitch"; DESIGN.md
section 24) against tests/pitch_ref.py on the rows of tests/pitch_cases.py: every decision judged in float64 given the device's own
previous decision (no cascades), the overlap-add at the device's table, spans, the composition with the resampler bit for bit, and what
a shift does to a steady harmonic row."""
import numpy as np
import pytest

from supertonic_amd import binding
import pitch_cases as pc
import pitch_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


@pytest.fixture(scope="module")
def stretched(eng):
    """(hz, a, b) -> (y, delta, score) of all the rows of pc.rows(hz) in one call, computed once"""
    cache = {}

    def get(hz, a, b):
        if (hz, a, b) not in cache:
            x, n, _ = pc.rows(hz)
            cache[hz, a, b] = _by_four(lambda lo, hi: eng.op_time_stretch(x[lo:hi], hz, a, b, n=n[lo:hi]), len(x))
        return cache[hz, a, b]
    return get


def _by_four(fn, rows):
    """fn(lo, hi) over the rows four at a time (the calls stay small), the results stacked"""
    parts = [fn(lo, min(lo + 4, rows)) for lo in range(0, rows, 4)]
    if isinstance(parts[0], tuple):
        return tuple(np.concatenate(c) for c in zip(*parts))
    return np.concatenate(parts)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("ratio", pc.RATIOS)
@pytest.mark.parametrize("hz", pc.RATES)
def test_decisions_without_cascades_and_pinned_ties(stretched, hz, ratio):
    a, b = ratio
    x, n, names = pc.rows(hz)
    p = pr.plan(hz, pc.W[hz], a, b)
    y, delta, score = stretched(hz, a, b)
    assert delta.shape == (len(names), p["M"]) and y.shape == (len(names), p["Ws"])
    assert np.all(delta[:, 0] == 0) and np.all(score[:, 0] == 0) and np.all(np.abs(delta) <= p["delta"])
    worst = 0.0
    for r, name in enumerate(names):
        gap, margin = pr.decision_gaps(x[r], n[r], hz, a, b, delta[r])
        bad = np.flatnonzero(gap > margin)
        assert bad.size == 0, (name, bad[:5], gap[bad[:5]], margin[bad[:5]])
        worst = max(worst, float(np.max(gap / np.maximum(margin, 1e-300))))
        ties = pr.tie_frames(x[r], n[r], hz, a, b, delta[r])
        assert all(delta[r, m] == 0 for m in ties), (name, [m for m in ties if delta[r, m] != 0][:5])
        if name in ("zero", "harmonic[:0]"):
            assert len(ties) == p["M"] - 1 and not delta[r].any() and not score[r].any() and not y[r].any()
    print(f"{hz} Hz {a}/{b}: largest gap / margin {worst:.3g}")
    v = names.index("vowel")
    assert len(pr.tie_frames(x[v], n[v], hz, a, b, delta[v])) >= 1  # (the gaps do produce ties)
    assert np.any(delta[names.index("harmonic")] != 0)


@pytest.mark.parametrize("ratio", pc.RATIOS)
@pytest.mark.parametrize("hz", pc.RATES)
def test_overlap_add_at_the_device_table(stretched, hz, ratio):
    a, b = ratio
    x, n, names = pc.rows(hz)
    y, delta, _ = stretched(hz, a, b)
    for r, name in enumerate(names):
        want = pr.ola(x[r], n[r], hz, a, b, delta[r])
        peak = float(np.max(np.abs(x[r, :n[r]]), initial=0.0))
        assert np.all(np.isfinite(y[r])), name  # (NaN behind a span never comes through)
        assert np.max(np.abs(y[r].astype(np.float64) - want), initial=0.0) <= 4 * 2.0 ** -24 * peak, name


@pytest.mark.parametrize("hz", pc.RATES)
def test_span_discipline_bit_for_bit(eng, stretched, hz):
    x, n, names = pc.rows(hz)
    for a, b in ((3, 2), (2, 3)):
        y, delta, score = stretched(hz, a, b)
        for r, name in enumerate(names):
            if n[r] in (0, pc.W[hz]):
                continue
            cut = np.where(np.isnan(x[r, :n[r]]), 0.0, x[r, :n[r]]).astype(np.float32)
            yc, dc, sc = eng.op_time_stretch(cut, hz, a, b)
            Ws, M = yc.shape[1], dc.shape[1]
            assert _same(np.ascontiguousarray(y[r:r + 1, :Ws]), yc), (name, a, b)
            assert np.array_equal(delta[r:r + 1, :M], dc) and _same(np.ascontiguousarray(score[r:r + 1, :M]), sc), (name, a, b)
            assert Ws == -(-int(n[r]) * a // b) and not y[r, Ws:].any()  # (and nothing behind the stretched span)


@pytest.mark.parametrize("semitones", [4.0, -5.0, 12.0, -12.0, 0.37])
def test_pitch_is_the_resample_of_the_stretch_bit_for_bit(eng, semitones):
    hz = 16000
    x, n, _ = pc.rows(hz)
    a, b = binding.pitch_ratio(semitones)
    k = pr.rate_scale(a, b)
    assert 8000 <= min(a, b) * k and max(a, b) * k <= 192000
    ys, _, _ = _by_four(lambda lo, hi: eng.op_time_stretch(x[lo:hi], hz, a, b, n=n[lo:hi]), len(x))
    want = _by_four(lambda lo, hi: eng.op_resample(ys[lo:hi], a * k, b * k), len(x))
    assert want.shape[1] >= pc.W[hz]
    got = _by_four(lambda lo, hi: eng.op_pitch(x[lo:hi], hz, semitones, n=n[lo:hi]), len(x))
    assert got.shape == x.shape and _same(got, np.ascontiguousarray(want[:, :pc.W[hz]]))


@pytest.mark.parametrize("semitones", sorted(pc.SHIFTS))
@pytest.mark.parametrize("hz", pc.RATES)
def test_a_shift_moves_the_fundamental_and_keeps_length_and_envelope(eng, hz, semitones):
    """The steady-part envelope (largest |dB| of the per-10-ms RMS against the median block) is held to the float64 reference's own
    figure on this row and shift (pitch_cases.reference_envelope_db: 0.77 .. 1.37 dB, the blocks hold 1.6 or 2.6 periods) plus what
    float32 may add (pitch_cases.FP32_ENVELOPE_DB)."""
    a, b = pc.SHIFTS[semitones]
    assert binding.pitch_ratio(semitones) == (a, b)
    x = pc.harmonic(hz, pc.W[hz])
    y = eng.op_pitch(x, hz, semitones)[0]
    assert y.shape == (pc.W[hz],) and np.all(np.isfinite(y))
    lo, hi = pc.steady(hz, pc.W[hz])
    f = pc.F0 * a / b
    f0, lag = pr.autocorr_f0(y, hz, lo, hi, f / 1.5, f * 1.5)
    env = max(abs(v) for v in pr.envelope_db(y, hz, lo, hi))
    ref = pc.reference_envelope_db(hz, semitones)
    print(f"{hz} Hz {semitones:+g}: f0 {f0:.2f} Hz (lag {lag}, wanted {hz / f:.2f}), envelope {env:.4f} dB (reference {ref:.4f} dB)")
    assert abs(lag - hz / f) <= 0.5
    assert env <= ref + pc.FP32_ENVELOPE_DB


def test_refusals(eng):
    x = pc.harmonic(16000, 1024)
    for bad in (dict(hz=7999), dict(a=0), dict(b=641)):
        with pytest.raises(binding.StnError):
            eng.op_time_stretch(x, **{"hz": 16000, "a": 3, "b": 2, **bad})
    with pytest.raises(binding.StnError):
        eng.op_time_stretch(x, 16000, 3, 2, n=[1025])
    with pytest.raises(binding.StnError, match="semitones"):
        eng.op_pitch(x, 16000, 12.5)
