"""The eight launches of the fetch-time de-esser on an MI355X, through stn_op_deesser_ex (Engine::ds_enqueue itself: the band's chunk pass
and scan, chunk pass 1, the (max, x) scan, chunk pass 2, the linear scan, the write pass, the row maxima; kernels_dynamics.hip; DESIGN.md
section 21), its scratch poisoned with NaN and laid open: the band's and both detector stages' chunk end values and start values, h, yL
and y against the contract's recurrence in float64 on the same fp32 coefficients (tests/deesser_ref.py), on the rows, settings, widths
and bounds of tests/deesser_cases.py; both staging forms, a row alone / as row 5 of 8 / at a wider W, and in place against out of place,
bit for bit; h against stn_op_filter of the two high-passes and yL against stn_op_compressor_ex on that band, bit for bit; the guards
around x and y.

Bounds: 4 x the deviation of the float32 sequential restatement from float64, per setting and over all its rows; the rows whose band
stays under the knee get none (tests/deesser_cases.py).  None comes from a kernel.  Every call is held against the reference of the
widest call cut at its W: a row's first n samples do not depend on W.

(test_zz_report_measured prints measured over bound per setting.)"""
import numpy as np
import pytest

from supertonic_amd import binding
import deesser_cases as dc
import deesser_ref as dr

pytestmark = pytest.mark.gpu
MEASURED = {}
KEYS = dc.STATES + ("band", "gr_db", "y")
WHAT = {"gr_db": "yl", "band": "h"}


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


_runs = {}


def _run(eng, name, W, misalign=0, in_place=0, rows=None):
    """one call per (setting, W, alignment, in place, rows), shared by the tests and left unchanged"""
    key = (name, W, misalign, in_place, rows)
    if key not in _runs:
        c = dc.case(name)
        x = c.x[:, :W] if rows is None else c.x[list(rows), :W]
        o = eng.op_deesser_ex(np.ascontiguousarray(x), c.rate, c.setting, x_misalign=misalign, in_place=in_place)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _runs[key] = o
    return _runs[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _form(W, misalign):
    return "vec" if W % 4 == 0 and not misalign else "scalar"


def _check(c, o, W, form, rows=None):
    """every array of one call against the float64 reference cut at W; the failure names the array, the row, the place and the ratio"""
    sel = slice(None) if rows is None else list(rows)
    names = dc.NAMES if rows is None else [dc.NAMES[r] for r in rows]
    ref = dict(c.ref.states(c.f, W), band=c.ref.h[:, :W], gr_db=c.ref.yl[:, :W], y=c.ref.y[:, :W])
    for key in KEYS:
        got, what = o[key], WHAT.get(key, key)
        assert not np.isnan(got).any(), (c.name, key, f"W {W}", form, "poison left in what the launches own", np.argwhere(np.isnan(got))[:4].tolist())
        d = np.abs(got.astype(np.float64) - ref[key][sel])
        if what in dc.REL:
            d = d / c.peak[sel].reshape((-1,) + (1,) * (d.ndim - 1))
        d = d.reshape(d.shape[0], -1)
        b = c.bound[what][sel][:, None]
        bad = np.argwhere(d > b)
        per = dr.CHUNK if key in ("band", "gr_db", "y") else 4 if key in dr.BAND_STATES else 1  # entries per chunk
        assert bad.size == 0, (c.name, key, f"W {W}", form,
                               [(names[i], f"index {j}", f"chunk {j // per}", f"scan tile {j // per // dr.SCAN}", f"{d[i, j]:.2e} over {b[i, 0]:.2e}") for i, j in bad[:6]])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(d == 0, 0.0, d / b).max()
        MEASURED[(c.name, what)] = max(MEASURED.get((c.name, what), 0.0), float(ratio))
    for key in ("st_start", "s1_start", "s2_start"):  # every row starts the band and both stages from +0.0
        assert np.all(_bits(o[key][:, 0]) == 0), key
    if c.f["split"]:  # a row whose band never reaches the knee comes back as it went in, the sign of a zero included
        still = [i for i, r in enumerate(range(8) if rows is None else rows) if r in dc.STILL]
        x = c.x[:, :W] if rows is None else c.x[list(rows), :W]
        assert np.array_equal(_bits(o["y"][still]), _bits(x[still])), (c.name, W, form)


@pytest.mark.parametrize("name", list(dc.SETTINGS))
def test_states_and_output_against_float64(eng, name):
    c = dc.case(name)
    dc.conditions(c)  # (on the float64 reference alone, before the GPU is consulted)
    for W in dc.widths():
        for mis in ((0, 1) if W == dc.W_MAX else (0,)):
            o = _run(eng, name, W, mis)
            form = _form(W, mis)
            assert o["form"] == form, (name, W, mis, o["form"])
            assert o["guard_ok"], (name, W, form, "a launch wrote outside x or y")
            assert o["s1_end"].shape == (8, dr.chunks(W)) and o["st_end"].shape == (8, dr.chunks(W), 4)
            _check(c, o, W, form)
        one = _run(eng, name, W, rows=(dc.NOISE,))  # rows = 1
        assert one["guard_ok"]
        _check(c, one, W, _form(W, 0), rows=(dc.NOISE,))


@pytest.mark.parametrize("name", list(dc.SETTINGS))
def test_staging_forms_agree_bit_for_bit(eng, name):
    v, s = _run(eng, name, dc.W_MAX, 0), _run(eng, name, dc.W_MAX, 1)
    assert (v["form"], s["form"]) == ("vec", "scalar")
    for key in KEYS:
        assert np.array_equal(_bits(v[key]), _bits(s[key])), (name, key)


@pytest.mark.parametrize("name", list(dc.SETTINGS))
def test_in_place_is_out_of_place_bit_for_bit(eng, name):
    for W, mis in ((dc.W_MAX, 0), (dc.W_MAX, 1), (dc.SPAN + 1, 0)):
        a, b = _run(eng, name, W, mis), _run(eng, name, W, mis, in_place=1)
        assert b["guard_ok"] and b["form"] == a["form"]
        for key in KEYS:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), (name, W, mis, key)


@pytest.mark.parametrize("name", list(dc.SETTINGS))
def test_a_row_alone_in_a_batch_and_at_a_wider_width_bit_for_bit(eng, name):
    c = dc.case(name)
    rng = np.random.default_rng(3)
    for r, n in ((dc.NOISE, dc.SPAN + 1), (dc.ESS, dc.TILE + dr.CHUNK), (dc.SPEECHLIKE, 1500 * dr.CHUNK + dr.CHUNK + 2)):
        row = np.ascontiguousarray(c.x[r:r + 1, :n])
        alone = eng.op_deesser(row, c.rate, c.setting)
        batch = (0.3 * rng.standard_normal((8, n))).astype(np.float32)
        batch[5] = row[0]
        wide = np.concatenate([row, (0.3 * rng.standard_normal((1, 4099))).astype(np.float32)], axis=1)
        assert np.array_equal(_bits(eng.op_deesser(batch, c.rate, c.setting)[5]), _bits(alone[0])), (name, dc.NAMES[r], n, "as row 5 of 8")
        assert np.array_equal(_bits(eng.op_deesser(wide, c.rate, c.setting)[0, :n]), _bits(alone[0])), (name, dc.NAMES[r], n, "at a wider W")
        assert np.array_equal(_bits(alone[0]), _bits(_run(eng, name, dc.W_MAX)["y"][r, :n])), (name, dc.NAMES[r], n, "in the widest call")


@pytest.mark.parametrize("name", list(dc.SETTINGS))
def test_band_is_the_chain_s_section_pass_bit_for_bit(eng, name):
    c = dc.case(name)
    chain = [("highpass", c.setting[0], float(q), 0.0) for q in dr.Q]
    for W, mis in ((dc.W_MAX, 0), (dc.W_MAX, 1), (dc.SPAN + 1, 0)):
        o = _run(eng, name, W, mis)
        f = eng.op_filter_ex(np.ascontiguousarray(c.x[:, :W]), c.rate, chain, x_misalign=mis)
        assert np.array_equal(_bits(o["band"]), _bits(f["y"])), (name, W, mis, "h")
        assert np.array_equal(_bits(o["st_end"]), _bits(f["st_end"][0])) and np.array_equal(_bits(o["st_start"]), _bits(f["st_start"][0])), (name, W, mis)


@pytest.mark.parametrize("name", list(dc.SETTINGS))
def test_detector_is_the_compressor_s_on_the_band_bit_for_bit(eng, name):
    """with a range that does not bind (24 dB, on the rows 20 dB down), yL is stn_op_compressor_ex's yL of the band under the same T,
    ratio, knee, attack and release"""
    c = dc.case(name)
    setting = c.setting[:6] + (24.0,) + c.setting[7:]
    W = dc.TILE + dr.CHUNK
    o = eng.op_deesser_ex((0.1 * c.x[:, :W]).astype(np.float32), c.rate, setting)
    k = eng.op_compressor_ex(o["band"], c.rate, tuple(setting[1:6]) + (0.0,))
    assert 3.0 < k["s1_end"].max() < 24.0  # the wanted reduction never reaches the range, and there is something to compare
    for key in dr.DET_STATES + ("gr_db",):
        assert np.array_equal(_bits(o[key]), _bits(k[key])), (name, key, np.abs(o[key].astype(np.float64) - k[key]).max())


def test_the_plain_op_is_the_same_and_ignores_dirty_scratch(eng):
    name = "default_44k"
    c = dc.case(name)
    W = dc.widths()[-2]
    o = _run(eng, name, W)
    x = np.ascontiguousarray(c.x[:, :W])
    assert np.array_equal(_bits(eng.op_deesser(x, c.rate, c.setting)), _bits(o["y"]))
    # a larger call of other rows and another setting leaves its values all over the scratch and the tables; the smaller call reads none
    eng.op_deesser(np.random.default_rng(1).standard_normal((8, W + 4096)).astype(np.float32), 16000, dc.SETTINGS["wide_16k"][0])
    sub = [dc.CLICKS, dc.NOISE, dc.ZERO]
    assert np.array_equal(_bits(eng.op_deesser(x[sub], c.rate, c.setting)), _bits(o["y"][sub]))
    # the mode is part of the table's key: the same numbers in wide mode give another y
    wide = eng.op_deesser(x[sub], c.rate, c.setting[:7] + ("wide",))
    assert not np.array_equal(wide[1], o["y"][dc.NOISE]) and np.array_equal(_bits(eng.op_deesser(x[sub], c.rate, c.setting)), _bits(o["y"][sub]))


def test_ex_refuses_what_the_op_refuses(eng):
    x = np.zeros((1, 100), np.float32)
    for hz in (7999, 192001, 8000):  # (8000: the speech default's 5500 Hz is above 0.45 x the rate)
        with pytest.raises(binding.StnError):
            eng.op_deesser_ex(x, hz, True)
    for i, (field, bad) in enumerate(zip(dr.FIELDS[:7], (1999.0, -61.0, 0.5, 25.0, 0.05, 5.0, 30.0))):
        s = list(dr.SPEECH)
        s[i] = bad
        with pytest.raises(binding.StnError) as ei:
            eng.op_deesser(x, 44100, tuple(s))
        assert ei.value.code == -1 and field in str(ei.value)
    for kw in (dict(x_misalign=2), dict(in_place=2)):
        with pytest.raises(binding.StnError):
            eng.op_deesser_ex(x, 44100, True, **kw)
    assert eng.op_deesser_ex(x, 44100, True)["form"] == "vec" and eng.op_deesser_ex(x, 44100, True, x_misalign=1)["form"] == "scalar"
    assert eng.op_deesser_ex(x[:, :99], 44100, True)["form"] == "scalar"


def test_zz_report_measured():
    order = dc.STATES + ("h", "yl", "y")
    print("\nsetting      restatement's deviation (" + " / ".join(order) + "; band states, h, y relative to the peak, the rest dB)      measured over bound (same order)")
    for name in dc.SETTINGS:
        c = dc.case(name)
        dev = " / ".join(f"{float(np.max(c.dev[k])):.1e}" for k in order)
        got = " / ".join(f"{MEASURED.get((name, k), float('nan')):.2f}" for k in order)
        print(f"{name:<13}{dev:<100}{got}")
    print("(the bound is 4 x the restatement's deviation, per setting)")
