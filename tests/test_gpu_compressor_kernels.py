"""The five launches of the fetch-time compressor on an MI355X, through stn_op_compressor_ex (Engine::cp_enqueue itself: chunk pass 1, the
(max, x) scan, chunk pass 2, the linear scan, the write pass; kernels_dynamics.hip), its scratch poisoned with
NaN and laid open: both stages' chunk end values and start values, yL and y against the contract's recurrence in float64 on the same
fp32 coefficients (tests/compressor_ref.py), on the rows, settings, widths and bounds of tests/compressor_cases.py; both staging forms,
a row alone / as row 5 of 8 / at a wider W, and in place against out of place, bit for bit; the guards around x and y.

Bounds: 4 x the deviation of the float32 sequential restatement (the contract operation for operation, its two fma included) from
float64, per setting and over all its rows; rows on which the restatement does not deviate at all get the floor
tests/compressor_cases.py justifies (their states must be exactly 0).  None comes from a kernel.  Every call is held against the reference of the widest call cut at its W: a row's first n samples do not depend on W.

(test_zz_report_measured prints measured over bound per setting.)"""
import numpy as np
import pytest

from supertonic_amd import binding
import compressor_cases as cc
import compressor_ref as cr

pytestmark = pytest.mark.gpu
MEASURED = {}
KEYS = cc.STATES + ("gr_db", "y")


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
        c = cc.case(name)
        x = c.x[:, :W] if rows is None else c.x[list(rows), :W]
        o = eng.op_compressor_ex(np.ascontiguousarray(x), c.rate, c.setting, x_misalign=misalign, in_place=in_place)
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
    names = cc.NAMES if rows is None else [cc.NAMES[r] for r in rows]
    st = c.ref.states(c.f, W)
    ref = dict(st, gr_db=c.ref.yl[:, :W], y=c.ref.y[:, :W])
    for key in KEYS:
        got, what = o[key], {"gr_db": "yl"}.get(key, key)
        assert not np.isnan(got).any(), (c.name, key, f"W {W}", form, "poison left in what the launches own", np.argwhere(np.isnan(got))[:4].tolist())
        r = ref[key][sel]
        d = np.abs(got.astype(np.float64) - r)
        if what == "y":
            d = d / np.where(c.peak[sel] > 0, c.peak[sel], 1.0)[:, None]
        b = c.bound[what][sel][:, None]
        bad = np.argwhere(d > b)
        per = cr.CHUNK if what in ("yl", "y") else 1
        assert bad.size == 0, (c.name, key, f"W {W}", form,
                               [(names[i], f"index {j}", f"chunk {j // per}", f"scan tile {j // per // cr.SCAN}", f"{d[i, j]:.2e} over {b[i, 0]:.2e}") for i, j in bad[:6]])
        ratio = np.where(d == 0, 0.0, d / np.where(b > 0, b, 1.0)).max()
        MEASURED[(c.name, what)] = max(MEASURED.get((c.name, what), 0.0), float(ratio))
    assert np.all(_bits(o["s1_start"][:, 0]) == 0) and np.all(_bits(o["s2_start"][:, 0]) == 0)  # every row starts both stages from +0.0


@pytest.mark.parametrize("name", list(cc.SETTINGS))
def test_states_and_output_against_float64(eng, name):
    c = cc.case(name)
    cc.conditions(c)  # (on the float64 reference alone, before the GPU is consulted)
    for W in cc.widths():
        for mis in ((0, 1) if W == cc.W_MAX else (0,)):
            o = _run(eng, name, W, mis)
            form = _form(W, mis)
            assert o["form"] == form, (name, W, mis, o["form"])
            assert o["guard_ok"], (name, W, form, "a launch wrote outside x or y")
            assert o["s1_end"].shape == (8, cr.chunks(W))
            _check(c, o, W, form)
        one = _run(eng, name, W, rows=(cc.NOISE,))  # rows = 1
        assert one["guard_ok"]
        _check(c, one, W, _form(W, 0), rows=(cc.NOISE,))


@pytest.mark.parametrize("name", list(cc.SETTINGS))
def test_staging_forms_agree_bit_for_bit(eng, name):
    v, s = _run(eng, name, cc.W_MAX, 0), _run(eng, name, cc.W_MAX, 1)
    assert (v["form"], s["form"]) == ("vec", "scalar")
    for key in KEYS:
        assert np.array_equal(_bits(v[key]), _bits(s[key])), (name, key)


@pytest.mark.parametrize("name", list(cc.SETTINGS))
def test_in_place_is_out_of_place_bit_for_bit(eng, name):
    for W, mis in ((cc.W_MAX, 0), (cc.W_MAX, 1), (cc.SPAN + 1, 0)):
        a, b = _run(eng, name, W, mis), _run(eng, name, W, mis, in_place=1)
        assert b["guard_ok"] and b["form"] == a["form"]
        for key in KEYS:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), (name, W, mis, key)


@pytest.mark.parametrize("name", list(cc.SETTINGS))
def test_a_row_alone_in_a_batch_and_at_a_wider_width_bit_for_bit(eng, name):
    c = cc.case(name)
    rng = np.random.default_rng(3)
    for r, n in ((cc.NOISE, cc.SPAN + 1), (cc.BURSTS, cc.TILE + cr.CHUNK), (cc.SPEECHLIKE, 1500 * cr.CHUNK + cr.CHUNK + 2)):
        row = np.ascontiguousarray(c.x[r:r + 1, :n])
        alone = eng.op_compressor(row, c.rate, c.setting)
        batch = (0.3 * rng.standard_normal((8, n))).astype(np.float32)
        batch[5] = row[0]
        wide = np.concatenate([row, (0.3 * rng.standard_normal((1, 4099))).astype(np.float32)], axis=1)
        assert np.array_equal(_bits(eng.op_compressor(batch, c.rate, c.setting)[5]), _bits(alone[0])), (name, cc.NAMES[r], n, "as row 5 of 8")
        assert np.array_equal(_bits(eng.op_compressor(wide, c.rate, c.setting)[0, :n]), _bits(alone[0])), (name, cc.NAMES[r], n, "at a wider W")
        assert np.array_equal(_bits(alone[0]), _bits(_run(eng, name, cc.W_MAX)["y"][r, :n])), (name, cc.NAMES[r], n, "in the widest call")


def test_the_plain_op_is_the_same_and_ignores_dirty_scratch(eng):
    name = "speech_44k"
    c = cc.case(name)
    W = cc.widths()[-2]
    o = _run(eng, name, W)
    x = np.ascontiguousarray(c.x[:, :W])
    assert np.array_equal(_bits(eng.op_compressor(x, c.rate, c.setting)), _bits(o["y"]))
    # a larger call of other rows and another setting leaves its values all over the scratch and the table; the smaller call reads none
    eng.op_compressor(np.random.default_rng(1).standard_normal((8, W + 4096)).astype(np.float32), 8000, cc.SETTINGS["hard_8k"][0])
    sub = [cc.CLICKS, cc.NOISE, cc.ZERO]
    assert np.array_equal(_bits(eng.op_compressor(x[sub], c.rate, c.setting)), _bits(o["y"][sub]))


def test_ex_refuses_what_the_op_refuses(eng):
    x = np.zeros((1, 100), np.float32)
    for hz in (7999, 192001):
        with pytest.raises(binding.StnError):
            eng.op_compressor_ex(x, hz, True)
    for i, (field, bad) in enumerate(zip(cr.FIELDS, (-61.0, 0.5, 25.0, 0.05, 5.0, 30.0))):
        s = list(cr.SPEECH)
        s[i] = bad
        with pytest.raises(binding.StnError) as ei:
            eng.op_compressor(x, 44100, tuple(s))
        assert ei.value.code == -1 and field in str(ei.value)
    for kw in (dict(x_misalign=2), dict(in_place=2)):
        with pytest.raises(binding.StnError):
            eng.op_compressor_ex(x, 44100, True, **kw)
    assert eng.op_compressor_ex(x, 44100, True)["form"] == "vec" and eng.op_compressor_ex(x, 44100, True, x_misalign=1)["form"] == "scalar"
    assert eng.op_compressor_ex(x[:, :99], 44100, True)["form"] == "scalar"


def test_zz_report_measured():
    print("\nsetting      restatement's deviation (s1_end / s1_start / s2_end / s2_start / yl dB; y rel.)      measured over bound (same order)")
    order = cc.STATES + ("yl", "y")
    for name in cc.SETTINGS:
        c = cc.case(name)
        dev = " / ".join(f"{float(np.max(c.dev[k])):.1e}" for k in order)
        got = " / ".join(f"{MEASURED.get((name, k), float('nan')):.2f}" for k in order)
        print(f"{name:<13}{dev:<70}{got}")
    print("(the bound is 4 x the restatement's deviation, per setting)")
