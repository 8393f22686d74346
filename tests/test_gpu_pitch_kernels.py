"""The pitch shift's kernels on an MI355X at op level (kernels_pitch.hip, the capped resample launch; include/stn.h "pitch"; DESIGN.md
section 24) against tests/pitch_ref.py on the rows of tests/pitch_cases.py: every decision judged in float64 given the device's own
previous decision (no cascades), the overlap-add at the device's table, spans, the composition with the resampler bit for bit, and what
a shift does to a steady harmonic row.

The rates of pitch_cases.RATES search at hops of 64, 128 and 512: a thread owns at most one candidate.  The wide rows (pitch_cases.
WIDE_RATES: 24, 96 and 192 kHz) run the other geometries: H = 256, the one workgroup of 7 waves; H = 1024 and 2048, where the 1537 and
3073 candidates take the 1024 threads 2 and 4 trips, the last by thread 0 alone for d = +D, each thread keeps the best of its several
and 16 wave slots are folded; and at H = 2048 the full prefetch registers and 73.9 KB of dynamic LDS, more than a launch gets
without launch_pitch_search's attribute call.  Their noise row has one good candidate per frame, so that a winner in every trip is
checked against the reference's pick itself (tests/test_pitch_cpu.py: a search blind to any trip fails on it).

Cost on an MI355X: the file takes 4.9 s of wall time with the runtime's start, nearly all of it the float64 scores of the wide rows
on the host: 0.3 to 0.85 s for each of the four ratios at 192 kHz, 0.08 to 0.22 s at 96 kHz, 0.02 s at 24 kHz; every other test is
under 0.05 s."""
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


@pytest.fixture(scope="module")
def wide(eng):
    """(hz, a, b) -> (y, delta, score) of the rows of pc.wide_rows(hz), four rows a call, computed once"""
    cache = {}

    def get(hz, a, b):
        if (hz, a, b) not in cache:
            x, n, _ = pc.wide_rows(hz)
            cache[hz, a, b] = _by_four(lambda lo, hi: eng.op_time_stretch(x[lo:hi], hz, a, b, n=n[lo:hi]), len(x))
        return cache[hz, a, b]
    return get


@pytest.fixture(scope="module")
def wide_judged(wide):
    """(hz, a, b) -> per row pitch_ref.judge of the device's table, computed once (the float64 scores of 3073 candidates of 4096 samples
    are the cost of these tests)"""
    cache = {}

    def get(hz, a, b):
        if (hz, a, b) not in cache:
            x, n, _ = pc.wide_rows(hz)
            delta = wide(hz, a, b)[1]
            cache[hz, a, b] = [pr.judge(x[r], n[r], hz, a, b, delta[r]) for r in range(len(x))]
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


# ---- the wide hops: H = 256 (7 waves), 1024 and 2048 (more candidates than threads; 73.9 KB of LDS) ------------------------------------------
@pytest.mark.parametrize("ratio", pc.WIDE_RATIOS)
@pytest.mark.parametrize("hz", pc.WIDE_RATES)
def test_wide_decisions_without_cascades_and_pinned_ties(wide, wide_judged, hz, ratio):
    a, b = ratio
    x, n, names = pc.wide_rows(hz)
    p = pr.plan(hz, pc.WIDE_W[hz], a, b)
    assert p["H"] == {24000: 256, 96000: 1024, 192000: 2048}[hz] and 11 <= p["M"] <= 27
    y, delta, score = wide(hz, a, b)
    assert delta.shape == (len(names), p["M"]) and y.shape == (len(names), p["Ws"])
    assert np.all(delta[:, 0] == 0) and np.all(score[:, 0] == 0) and np.all(np.abs(delta) <= p["delta"])
    worst = 0.0
    for r, name in enumerate(names):
        j = wide_judged(hz, a, b)[r]
        bad = np.flatnonzero(j["gap"] > j["margin"])
        assert bad.size == 0, (name, bad[:5], j["gap"][bad[:5]], j["margin"][bad[:5]], delta[r, bad[:5]], j["pick"][bad[:5]])
        worst = max(worst, float(np.max(j["gap"] / np.maximum(j["margin"], 1e-300))))
        assert all(delta[r, m] == 0 for m in j["ties"]), (name, [m for m in j["ties"] if delta[r, m] != 0][:5])
        if name == "zero":
            assert len(j["ties"]) == p["M"] - 1 and not delta[r].any() and not score[r].any() and not y[r].any()
    print(f"{hz} Hz {a}/{b}: largest gap / margin {worst:.3g}")
    assert len(wide_judged(hz, a, b)[names.index("vowel")]["ties"]) >= 1
    assert np.any(delta[names.index("noise")] != 0)


@pytest.mark.parametrize("hz", pc.WIDE_RATES)
def test_wide_decisions_on_noise_are_the_reference_picks_wherever_the_lead_settles_them(wide, wide_judged, hz):
    """On the noise row one candidate leads (pitch_cases.noise).  Where its float64 score leads every other by more than twice the
    margin, the device's offset must be the reference's given the device's own previous one: that is asked of at least 3/4 of the
    frames at 8/5 and 1/2 at 4/7 (the reference's own tables give 25/26, 26/26, 24/26 and 10/10, 10/10, 6/10 at 24, 96 and 192 kHz).
    The tables hold d = +D (8/5, frame 2) and d = -D (4/7, frame 1), and at 96 and 192 kHz winners in every slice of T candidates:
    every trip of the candidate loop, the last one's single candidate included, has produced a winner that was checked."""
    x, n, names = pc.wide_rows(hz)
    r = names.index("noise")
    T, C = pc.search_threads(hz)
    D = (C - 1) // 2
    slices = set()
    for (a, b), share in (((8, 5), 0.75), ((4, 7), 0.5)):
        delta = wide(hz, a, b)[1][r]
        j = wide_judged(hz, a, b)[r]
        settled = np.flatnonzero(j["lead"][1:] > 2.0 * j["margin"][1:]) + 1
        print(f"{hz} Hz {a}/{b}: {len(settled)} of {len(delta) - 1} frames judged exactly; offsets {delta.tolist()}")
        assert len(settled) >= share * (len(delta) - 1), (a, b, len(settled), len(delta) - 1)
        wrong = [int(m) for m in settled if delta[m] != j["pick"][m]]
        assert not wrong, (a, b, wrong[:5], delta[wrong[:5]], j["pick"][wrong[:5]])
        assert (D if a > b else -D) in delta[1:], (a, b, delta)
        slices |= {int(d + D) // T for d in delta[1:]}
    assert slices == set(range(-(-C // T))), (sorted(slices), T, C)


@pytest.mark.parametrize("ratio", pc.WIDE_RATIOS)
@pytest.mark.parametrize("hz", pc.WIDE_RATES)
def test_wide_overlap_add_at_the_device_table(wide, hz, ratio):
    a, b = ratio
    x, n, names = pc.wide_rows(hz)
    y, delta, _ = wide(hz, a, b)
    for r, name in enumerate(names):
        want = pr.ola(x[r], n[r], hz, a, b, delta[r])
        peak = float(np.max(np.abs(x[r, :n[r]]), initial=0.0))
        assert np.all(np.isfinite(y[r])), name
        assert np.max(np.abs(y[r].astype(np.float64) - want), initial=0.0) <= 4 * 2.0 ** -24 * peak, name


@pytest.mark.parametrize("hz", pc.WIDE_RATES)
def test_wide_span_discipline_bit_for_bit(eng, wide, hz):
    x, n, names = pc.wide_rows(hz)
    for a, b in ((3, 2), (4, 7)):
        y, delta, score = wide(hz, a, b)
        cut_rows = [r for r in range(len(names)) if n[r] != pc.WIDE_W[hz]]
        assert len(cut_rows) == 3
        for r in cut_rows:
            cut = np.where(np.isnan(x[r, :n[r]]), 0.0, x[r, :n[r]]).astype(np.float32)
            yc, dc, sc = eng.op_time_stretch(cut, hz, a, b)
            Ws, M = yc.shape[1], dc.shape[1]
            assert _same(np.ascontiguousarray(y[r:r + 1, :Ws]), yc), (names[r], a, b)
            assert np.array_equal(delta[r:r + 1, :M], dc) and _same(np.ascontiguousarray(score[r:r + 1, :M]), sc), (names[r], a, b)
            assert Ws == -(-int(n[r]) * a // b) and not y[r, Ws:].any()


@pytest.mark.parametrize("hz,semitones", [(16000, 4.0), (16000, -5.0), (16000, 12.0), (16000, -12.0), (16000, 0.37), (96000, 4.0), (192000, 4.0)],
                         ids=["4.0", "-5.0", "12.0", "-12.0", "0.37", "96000-4.0", "192000-4.0"])
def test_pitch_is_the_resample_of_the_stretch_bit_for_bit(eng, hz, semitones):
    x, n, _ = pc.rows(hz) if hz in pc.W else pc.wide_rows(hz)
    width = x.shape[1]
    a, b = binding.pitch_ratio(semitones)
    k = pr.rate_scale(a, b)
    assert 8000 <= min(a, b) * k and max(a, b) * k <= 192000
    ys, _, _ = _by_four(lambda lo, hi: eng.op_time_stretch(x[lo:hi], hz, a, b, n=n[lo:hi]), len(x))
    want = _by_four(lambda lo, hi: eng.op_resample(ys[lo:hi], a * k, b * k), len(x))
    assert want.shape[1] >= width
    got = _by_four(lambda lo, hi: eng.op_pitch(x[lo:hi], hz, semitones, n=n[lo:hi]), len(x))
    assert got.shape == x.shape and _same(got, np.ascontiguousarray(want[:, :width]))


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
