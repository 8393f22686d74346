"""The formant correction's kernels on an MI355X at op level (kernels_formant.hip through stn_op_formant_ex; include/stn.h "formant";
DESIGN.md section 26) against tests/formant_ref.py on the rows of tests/formant_cases.py.

The tables are judged against the float64 reference's; the filter against the float64 reference run on the device's own tables, so that
a coefficient difference is not judged twice, per sample, within 4 x the deviation of the float32 numpy restatement from float64 on the
same row (formant_cases.FP32_DEVIATION, measured on the CPU; section 18's method).  The shifted rows are the reference's, so the
device's pitch stage is no part of these tests.  tests/test_formant_cpu.py shows that four mutants of the reference land outside
these bounds.

Cost on an MI355X: the file takes 6 s of wall time with the runtime's start, most of it the float64 pitch reference's shifts of the
wide rows on the host (1.2 s at 192 kHz, +4), computed once and shared; every other test is under 0.4 s."""
import numpy as np
import pytest

from supertonic_amd import binding
import formant_cases as fc
import formant_ref as fr
import pitch_ref as pr

pytestmark = pytest.mark.gpu

CASES = [(hz, s) for hz in fc.RATES for s in sorted(fc.SHIFTS)]


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


def _by_four(fn, rows):
    parts = [fn(lo, min(lo + 4, rows)) for lo in range(0, rows, 4)]
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k != "guard_ok"}
    out["guard_ok"] = all(p["guard_ok"] for p in parts)
    return out


@pytest.fixture(scope="module")
def ran(eng):
    """(hz, semitones) -> stn_op_formant_ex of all the rows of fc.rows(hz), four rows a call, computed once"""
    cache = {}

    def get(hz, s):
        if (hz, s) not in cache:
            x, n, _ = fc.rows(hz)
            y = fc.shifted(hz, s)
            cache[hz, s] = _by_four(lambda lo, hi: eng.op_formant(x[lo:hi], y[lo:hi], hz, n=n[lo:hi], ex=True), len(x))
        return cache[hz, s]
    return get


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("hz,semitones", CASES)
def test_tables_against_the_reference(ran, hz, semitones):
    """|d| <= 2^-23 |ref| + 1e-6 max|ref| per frame: one float32 ulp for a rounding at a boundary, and 20 x the 5.6e-8 that another
    summation order of N = 1024 double products can move a solution of condition 4.9e5; g to 1e-6 relative; silent frames exactly."""
    x, n, names = fc.rows(hz)
    y = fc.shifted(hz, semitones)
    d = ran(hz, semitones)
    P = fr.plan(hz, fc.WIDTH[hz])
    assert d["ax"].shape == (len(names), P["frames"], P["p"] + 1) and d["cy"].shape == d["ax"].shape and d["g"].shape == (len(names), P["frames"])
    assert d["guard_ok"]
    worst = 0.0
    silent_frames = 0
    for r, name in enumerate(names):
        t = fr.tables(x[r], y[r], n[r], hz)
        for key in ("ax", "cy"):
            ref = t[key].astype(np.float64)
            tol = 2.0 ** -23 * np.abs(ref) + 1e-6 * np.max(np.abs(ref), axis=1, keepdims=True)
            err = np.abs(d[key][r].astype(np.float64) - ref)
            assert np.all(np.isfinite(d[key][r])), (name, key)
            bad = np.argwhere(err > tol)
            assert bad.size == 0, (name, key, bad[:3], err[err > tol][:3])
            worst = max(worst, float(np.max(err / tol)))
        assert np.all(np.abs(d["g"][r] - t["g"]) <= 1e-6 * t["g"]), name
        for key in ("ex", "ey"):
            assert np.all(np.abs(d[key][r] - t[key]) <= 1e-6 * t[key]), (name, key)
        silent = (t["ex"] == 1e-9) & (t["ey"] == 1e-9)
        silent_frames += int(silent.sum())
        unit = np.zeros(P["p"] + 1, np.float32)
        unit[0] = 1.0
        assert np.all(d["ax"][r][silent] == unit) and np.all(d["cy"][r][silent] == unit) and np.all(d["g"][r][silent] == 1.0), name
        if name in ("zero", "harmonic[:0]"):
            assert silent.all()
    print(f"{hz} Hz {semitones:+g}: largest table error / bound {worst:.3g}; {silent_frames} silent frames")
    assert silent_frames > 2 * P["frames"]  # (the zero rows, and the vowel's gaps produce some)


@pytest.mark.parametrize("hz,semitones", CASES)
def test_filter_on_the_device_tables_and_spans(ran, hz, semitones):
    x, n, names = fc.rows(hz)
    y = fc.shifted(hz, semitones)
    d = ran(hz, semitones)
    failed = []
    for r, name in enumerate(names):
        got = d["out"][r]
        assert np.all(np.isfinite(got)), name  # (NaN behind a span never comes through)
        assert not got[n[r]:].any(), name
        want = fr.apply_tables(y[r], n[r], hz, d["ax"][r], d["cy"][r])
        err = float(np.max(np.abs(got.astype(np.float64) - want), initial=0.0))
        bound = 4.0 * fc.FP32_DEVIATION[hz, semitones][r]
        print(f"{hz} Hz {semitones:+g} {name}: device {err:.3g}, bound {bound:.3g} (fp32 restatement {fc.FP32_DEVIATION[hz, semitones][r]:.3g})")
        if not err <= bound:
            failed.append((name, err, bound))
    assert not failed, failed
    assert d["guard_ok"]


@pytest.mark.parametrize("hz", (16000, 44100, 24000))
def test_a_row_does_not_depend_on_its_batch_or_its_width(eng, ran, hz):
    x, n, names = fc.rows(hz)
    y = fc.shifted(hz, 4.0)
    W = fc.WIDTH[hz]
    v = names.index("vowel")
    alone = eng.op_formant(x[v], y[v], hz)
    assert _same(alone, np.ascontiguousarray(ran(hz, 4.0)["out"][v:v + 1]))
    order = [names.index("noise"), names.index("zero"), names.index("harmonic"), v]
    four = eng.op_formant(x[order], y[order], hz, n=n[order])
    assert _same(np.ascontiguousarray(four[3:4]), alone)
    wider = W + 3 * pr.hop(hz) + 17
    xw, yw = np.full((1, wider), np.nan, np.float32), np.full((1, wider), np.nan, np.float32)
    xw[0, :W], yw[0, :W] = x[v], y[v]
    wide = eng.op_formant(xw, yw, hz, n=[W])
    assert _same(np.ascontiguousarray(wide[:, :W]), alone) and not wide[:, W:].any()


@pytest.mark.parametrize("hz", (8000, 16000, 44100, 96000))
def test_no_state_crosses_a_frame(eng, ran, hz):
    """one sample of x and y at q set to another value, or to NaN: every out[j] with j < q - N or j >= q + 2 N stays bit-identical"""
    x, n, names = fc.rows(hz)
    y = fc.shifted(hz, -5.0)
    h = names.index("harmonic")
    N = 2 * pr.hop(hz)
    W = fc.WIDTH[hz]
    q = W // 2 + 13
    base = ran(hz, -5.0)["out"][h]
    for value in (0.5, np.nan):
        xq, yq = x[h].copy(), y[h].copy()
        xq[q] = yq[q] = value
        got = eng.op_formant(xq, yq, hz)[0]
        keep = np.r_[0:max(q - N, 0), min(q + 2 * N, W):W]
        assert keep.size > 0 and _same(np.ascontiguousarray(got[keep]), np.ascontiguousarray(base[keep])), (hz, value)
        assert not _same(got, base)


@pytest.mark.parametrize("hz", fc.RATES)
def test_the_correction_of_a_row_by_itself_is_the_row(eng, hz):
    """ax == cy then, and the FIR and the IIR start on the same sample: v == y0 in exact arithmetic.  Within 4 x the float32
    restatement's deviation on the same rows (formant_cases.IDENTITY_DEVIATION)."""
    x, n, names = fc.rows(hz)
    for name in fc.IDENTITY_ROWS:
        r = names.index(name)
        d = eng.op_formant(x[r], x[r], hz, ex=True)
        assert _same(d["ax"], d["cy"]) and np.all(d["g"] == 1.0)
        err = float(np.max(np.abs(d["out"][0].astype(np.float64) - x[r].astype(np.float64))))
        bound = 4.0 * fc.IDENTITY_DEVIATION[hz][name]
        print(f"{hz} Hz {name}: device {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (name, err, bound)


def test_refusals(eng):
    x = np.zeros((1, 1024), np.float32)
    with pytest.raises(binding.StnError):
        eng.op_formant(x, x, 7999)
    with pytest.raises(binding.StnError):
        eng.op_formant(x, x, 16000, n=[1025])
    with pytest.raises(ValueError):
        eng.op_formant(x, x[:, :1000], 16000)
