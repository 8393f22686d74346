"""The section passes of the fetch-time filter chain on an MI355X, through stn_op_filter_ex (Engine::fl_enqueue itself: per pass of two
biquads the chunk launch from zero state, the scan in double and filter_write_kernel, kernels_filter.hip), its
state buffer poisoned with NaN before every pass and laid open: every pass's chunk end states and start states and the output y against
the float64 recurrence on the same fp32 coefficients (tests/filter_ref.py), on the chains, rows, widths and bounds of
tests/filter_cases.py; both staging forms bit for bit; a row alone, in a batch and at a wider W bit for bit; the guards around x and y.

Bounds: 4 x the deviation of the float32 sequential restatement (no FMA) from float64, normalized as tests/filter_cases.py says; none
comes from a kernel.  Every call is held against the reference of the widest call cut at its W (a row's first n samples do not depend on
W), except the end state of a last, partial chunk, which only the widest call's reference has.

(test_zz_report_measured prints measured over bound per chain.)"""
import numpy as np
import pytest

from supertonic_amd import binding
import filter_cases as fc
import filter_ref as fr

pytestmark = pytest.mark.gpu
COMP = "s1 s2 t1 t2".split()
MEASURED = {}


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


_runs = {}


def _run(eng, name, W, misalign=0):
    """one call per (chain, W, alignment), shared by the tests and left unchanged"""
    key = (name, W, misalign)
    if key not in _runs:
        c = fc.case(name)
        o = eng.op_filter_ex(np.ascontiguousarray(c.x[:, :W]), c.rate, c.filters, x_misalign=misalign)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _runs[key] = o
    return _runs[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _calls():
    return [(W, 0) for W in fc.widths()] + [(fc.w_max(), 1)]


def _form(W, misalign):
    return "vec" if W % 4 == 0 and not misalign else "scalar"


def _worst(name, what, ratio):
    MEASURED[(name, what)] = max(MEASURED.get((name, what), 0.0), ratio)


def _check_states(c, what, got, W, form):
    """|got - ref| <= bound * scale at every chunk of every pass, exact where the scale is 0; the failure names the section pass, the row,
    the chunk, the component and the deviation at every seam"""
    ref = {"start": c.ref[0], "end": c.ref[1]}[what]
    if got.shape[2] == 0:  # (a call narrower than one chunk has no whole chunk)
        return
    assert not np.isnan(got).any(), (c.name, what, f"W {W}", form, "poison left in a chunk the pass owns", np.argwhere(np.isnan(got))[:4].tolist())
    rel, exact = fc.deviation(got, ref, c.scale[what])
    assert exact, (c.name, what, f"W {W}", form, "a row whose scale is 0 is not exactly 0")
    for p in range(rel.shape[0]):
        bound = c.bound[what][p]
        bad = np.argwhere(rel[p] > bound)
        seams = {k: float(rel[p][:, k].max()) for k in fc.seams(rel.shape[2])}
        assert bad.size == 0, (c.name, what, f"W {W}", form, f"section pass {p}", f"bound {bound:.2e}",
                               [(fc.NAMES[r], f"chunk {k}", COMP[q], f"{rel[p, r, k, q]:.2e}") for r, k, q in bad[:6]], "at the seams", seams)
        if bound > 0:
            _worst(c.name, what, float(rel[p].max() / bound))


def _check_y(c, got, W, form):
    assert not np.isnan(got).any(), (c.name, "y", f"W {W}", form)
    rel, exact = fc.deviation(got, c.ref[2], c.scale["y"])
    assert exact and not got[fc.ZERO].any(), (c.name, "y", f"W {W}", form, "the zero row is not exactly zero")
    bad = np.argwhere(rel > c.bound["y"])
    chunk, _, tile, _ = fc.geometry()
    assert bad.size == 0, (c.name, "y", f"W {W}", form, f"bound {c.bound['y']:.2e}",
                           [(fc.NAMES[r], f"sample {i}", f"chunk {i // chunk}", f"scan tile {i // chunk // tile}", f"{rel[r, i]:.2e}") for r, i in bad[:6]],
                           "at the seams", {k: float(rel[:, k * chunk:(k + 1) * chunk].max()) for k in fc.seams(fr.chunks(W))})
    _worst(c.name, "y", float(rel.max() / c.bound["y"]))


@pytest.mark.parametrize("name", list(fc.CHAINS))
def test_states_and_output_against_float64(eng, name):
    c = fc.case(name)
    chunk, span, tile, per = fc.geometry()
    assert (chunk, per) == (fr.CHUNK, 2) and c.W == 3 * tile * chunk + 40 and c.passes.shape[0] == (len(c.filters) + 1) // 2
    assert c.x[fc.IMPULSES, 0] == 1 and c.x[fc.IMPULSES, 1500 * chunk + chunk - 1] == 1 and tile < 1500 < 2 * tile
    for W, mis in _calls():
        o = _run(eng, name, W, mis)
        form = _form(W, mis)
        assert o["form"] == form, (name, W, mis, o["form"])
        assert o["guard_ok"], (name, W, form, "a launch wrote outside x or y")
        K, whole = fr.chunks(W), W // chunk if W < c.W else fr.chunks(W)
        assert o["st_start"].shape == (c.passes.shape[0], 5, K, 4)
        _check_states(c, "start", o["st_start"], W, form)
        _check_states(c, "end", o["st_end"][:, :, :whole], W, form)
        _check_y(c, o["y"], W, form)
        assert np.all(_bits(o["st_start"][:, :, 0]) == 0)  # every pass starts every row from +0.0
    K = fr.chunks(c.W)
    assert K > 3 * tile and set(fc.seams(K)) >= {span // chunk, tile, 2 * tile, 3 * tile}  # the widest call crosses every seam


@pytest.mark.parametrize("name", list(fc.CHAINS))
def test_staging_forms_agree_bit_for_bit(eng, name):
    v, s = _run(eng, name, fc.w_max(), 0), _run(eng, name, fc.w_max(), 1)
    assert (v["form"], s["form"]) == ("vec", "scalar")
    for key in ("st_end", "st_start", "y"):
        assert np.array_equal(_bits(v[key]), _bits(s[key])), (name, key)


@pytest.mark.parametrize("name", ["odd_44k", "full_44k", "hp_lowest_192k"])
def test_a_row_alone_in_a_batch_and_at_a_wider_width_bit_for_bit(eng, name):
    c = fc.case(name)
    chunk, span, tile, _ = fc.geometry()
    rng = np.random.default_rng(3)
    for r, n in ((fc.NOISE, span + 1), (fc.DC_TONE, (tile + 1) * chunk), (fc.IMPULSES, 1500 * chunk + chunk + 2)):
        row = np.ascontiguousarray(c.x[r:r + 1, :n])
        alone = eng.op_filter(row, c.rate, c.filters)
        batch = (0.3 * rng.standard_normal((8, n))).astype(np.float32)
        batch[5] = row[0]
        wide = np.concatenate([row, (0.3 * rng.standard_normal((1, 4099))).astype(np.float32)], axis=1)
        assert np.array_equal(_bits(eng.op_filter(batch, c.rate, c.filters)[5]), _bits(alone[0])), (name, fc.NAMES[r], n, "as row 5 of 8")
        assert np.array_equal(_bits(eng.op_filter(wide, c.rate, c.filters)[0, :n]), _bits(alone[0])), (name, fc.NAMES[r], n, "at a wider W")
        assert np.array_equal(_bits(alone[0]), _bits(_run(eng, name, c.W)["y"][r, :n])), (name, fc.NAMES[r], n, "in the widest call")


def test_the_plain_op_is_the_same_and_ignores_dirty_scratch(eng):
    name = "telephone_8k"
    c = fc.case(name)
    W = fc.widths()[-2]
    o = _run(eng, name, W)
    x = np.ascontiguousarray(c.x[:, :W])
    assert np.array_equal(_bits(eng.op_filter(x, c.rate, c.filters)), _bits(o["y"]))
    # a larger call of other rows and another chain leaves its values all over the scratch and the tables; the smaller call reads none
    eng.op_filter(np.random.default_rng(1).standard_normal((8, W + 4096)).astype(np.float32), 44100, fc.FULL)
    sub = [fc.CORNER, fc.NOISE, fc.ZERO]
    assert np.array_equal(_bits(eng.op_filter(x[sub], c.rate, c.filters)), _bits(o["y"][sub]))


def test_ex_refuses_what_the_op_refuses(eng):
    x = np.zeros((1, 100), np.float32)
    hp = [("highpass", 80.0)]
    for hz in (7999, 192001):
        with pytest.raises(binding.StnError):
            eng.op_filter_ex(x, hz, hp)
    for bad, field in (([("highpass", 10.0)], "freq_hz"), ([("peak", 1000.0, 9.0, 0.0)], "q"), ([("peak", 1000.0, 1.0, 19.0)], "gain_db")):
        with pytest.raises(binding.StnError) as ei:
            eng.op_filter(x, 44100, bad)
        assert ei.value.code == -1 and field in str(ei.value)
    with pytest.raises(binding.StnError):
        eng.op_filter(x, 44100, [])
    with pytest.raises(binding.StnError):
        eng.op_filter_ex(x, 44100, hp, x_misalign=2)
    assert eng.op_filter_ex(x, 44100, hp)["form"] == "vec" and eng.op_filter_ex(x, 44100, hp, x_misalign=1)["form"] == "scalar"
    assert eng.op_filter_ex(x[:, :99], 44100, hp)["form"] == "scalar"


def test_zz_report_measured():
    print("\nchain            restatement's deviation (start / end / y, worst pass)      measured over bound (start / end / y)")
    for name in fc.CHAINS:
        c = fc.case(name)
        dev = " / ".join(f"{float(np.max(c.f32[k])):.1e}" for k in ("start", "end", "y"))
        got = " / ".join(f"{MEASURED.get((name, k), float('nan')):.2f}" for k in ("start", "end", "y"))
        print(f"{name:<17}{dev:<60}{got}")
    print("(the bound is 4 x the restatement's deviation, per pass)")
