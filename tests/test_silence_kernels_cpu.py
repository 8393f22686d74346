"""That the bounds of tests/test_gpu_silence_kernels.py bite and that its references stay within them, on the CPU: the float32
sequential restatement of the frame pass and the row pass (tests/silence_cases.py: f32_shares, recombine) against every bound on every
case; six float64 models of the decomposition with one fault each, every one of which must break a bound at every rate where it can
occur; the conditions the near-threshold rows are built to; and the required spans.

The restatement's worst |error| / bound over all cases: 0.50 for a share (bound (L + 1) * 2^-24 of the share; 11.025 kHz) and 0.12 for a
level (bound 34 * 2^-24 of the level; the long case at 8 kHz).  The faults break their bound by factors of 1e4 and more.

The three faults that need a chunk straddling a frame boundary (silence_cases.SPLIT_MUTANTS: the split off by one sample, the second
share given to the frame after the right one, the straddling first chunk of a frame left out) cannot occur at 16, 48, 96 and 192 kHz
(F = 160, 480, 960, 1920, multiples of the 32-sample chunk): there the models must change nothing, which is asserted too."""
import numpy as np
import pytest

import silence_cases as sc
import silence_ref as ref

WORST = {}


def _worst(c, pa, pb, lev):
    ra, rb = sc.share_ratios(c, pa, pb)
    return max(float(ra.max()), float(rb.max())), max(float(v.max()) if v.size else 0.0 for v in sc.level_ratios(c, lev))


@pytest.mark.parametrize("key", sc.KEYS)
def test_spans_signals_and_padding(key):
    c = sc.get(key)
    assert c.W % 4 == 0 and c.W > 2 * sc.SPAN and c.Kf >= 12 and c.x.shape == (c.R, c.W + 1)
    assert set(sc.required_spans(c.F, c.W)) <= set(c.n.tolist())
    assert {s for s, _ in c.rows} == {sc.NOISE, sc.TONE, sc.ZERO, sc.QUARTER, sc.LAST_LOUD, sc.NEAR}
    for r in range(c.R):
        n = int(c.n[r])
        assert np.isnan(c.x[r, n:]).all() and not np.isnan(c.x[r, :n]).any()
        inside = c.x[r, :n]
        assert np.all((inside == 0) | (np.abs(inside) >= np.float32(1e-6))), c.names[r]  # no square underflows
        if c.rows[r][0] == sc.LAST_LOUD:  # the loudest sample is the single sample of the last frame
            assert n % c.F == 1 and int(np.abs(inside).argmax()) == n - 1 and int(c.lev64[r].argmax()) == c.frames[r] - 1
    if c.long:
        assert c.frames.max() > sc.ROW_THREADS and any(s == sc.LAST_LOUD and n // c.F >= sc.ROW_THREADS for s, n in c.rows)
    assert (c.F % sc.CHUNK == 0) == (c.hz in sc.ALIGNED)


def test_the_rates_frames_and_widths():
    F = [ref.frame(hz) for hz in sc.RATES]  # (the GPU file holds RATES against test_gpu_silence.RATES)
    assert F == [80, 110, 160, 221, 441, 480, 882, 960, 1764, 1920]
    assert sum(f % 32 == 0 for f in F) == 4 and sum(f % 2 for f in F) == 2
    assert [sc.width(hz) for hz in sc.RATES] == [16424] * 8 + [21176, 23048] and sc.LONG_W == 82440


@pytest.mark.parametrize("key", sc.KEYS)
def test_float32_restatement_stays_inside_every_bound(key):
    c = sc.get(key)
    share, level = _worst(c, c.pa32, c.pb32, c.lev32)
    WORST[key] = (share, level)
    assert share <= 1.0 and level <= 1.0, (key, share, level)
    # the exact zeros: a share without samples is +0.0, and pb has samples exactly where a frame boundary cuts a chunk inside the span
    for p, L in ((c.pa32, c.La), (c.pb32, c.Lb)):
        assert np.all(p.view(np.uint32)[L == 0] == 0)
    for r in range(c.R):
        assert np.count_nonzero(c.Lb[r]) == sc.pb_cuts(c.n[r], c.F), (key, c.names[r])
    if c.hz in sc.ALIGNED:
        assert not c.Lb.any()
    # the +-0.25 rows are exact in every frame, the short last one included, and the all-zero row is zero
    for r, (sig, n) in enumerate(c.rows):
        if sig == sc.QUARTER:
            assert np.all(c.lev32[r] == 0.0625) and np.all(c.lev64[r] == 0.0625) and c.lev32[r].size == -(-n // c.F)
        if sig == sc.ZERO:
            assert not c.lev32[r].any() and not c.pa32[r].any()
    # the float64 reference is its own decomposition recombined
    for r in range(c.R):
        assert np.allclose(sc.recombine(c.pa64[r], c.pb64[r], c.n[r], c.F), c.lev64[r], rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", sc.MUTANTS)
@pytest.mark.parametrize("key", sc.KEYS)
def test_every_fault_breaks_a_bound_where_it_can_occur(key, name):
    c = sc.get(key)
    pa, pb, lev = sc.mutant(c, name)
    share, level = _worst(c, pa, pb, lev)
    if sc.can_occur(c, name):
        assert max(share, level) > 100.0, (key, name, share, level)
    else:  # no chunk straddles a frame boundary: the model is the float64 reference again
        assert c.hz in sc.ALIGNED and name in sc.SPLIT_MUTANTS
        assert share == 0.0 and level < 1e-6, (key, name, share, level)


@pytest.mark.parametrize("key", sc.KEYS)
def test_near_threshold_rows_are_what_they_claim(key):
    c = sc.get(key)
    assert sorted(c.near) == [c.NEAR_EDGES, c.NEAR_PAUSE]
    for r, d in c.near.items():
        m = c.lev64[r]
        thr = float(m.max()) * 10.0 ** (-float(np.float32(sc.TOP_DB)) / 10.0)
        assert thr == d["thr"] and float(m.max()) == d["mx"] and int(m.argmax()) not in d["picked"]
        e = m[d["picked"]] / thr - 1.0
        assert d["picked"].size >= 8 and np.all(np.abs(e) <= 2e-5) and 2e-5 <= 10 * sc.LEVEL_BOUND
        assert set(np.round(np.abs(d["want"]), 9)) == {0.0, 1e-7, 1e-6, 1e-5} and np.all(np.abs(e - d["want"]) <= 2e-8)
        # every other frame is far from the threshold: what the device decides there is what float64 decides
        others = np.setdiff1d(np.arange(m.size), d["picked"])
        assert np.all(np.abs(10.0 * np.log10(m[others] / thr)) > 10.0)
        # with all picked frames inactive the pause pass would cut between the loud frames; with all active it would not
        F, Mp = c.F, ref.samples(c.hz, sc.MAX_PAUSE_MS)
        loud = np.flatnonzero(m >= 10.0 * thr)
        assert np.all(np.diff(loud)[:1] * F - F > Mp)


def test_zz_report_worst_ratios():
    print("\ncase        share / bound   level / bound   (float32 restatement)")
    for key in sc.KEYS:
        if key in WORST:
            print(f"{key:<12}{WORST[key][0]:<16.2f}{WORST[key][1]:.3f}")
