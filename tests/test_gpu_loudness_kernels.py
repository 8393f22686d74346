"""The four loudness launches (kernels_loudness.hip) pass by pass on an MI355X, through stn_op_loudness_ex
(Engine::lo_measure itself, its scratch poisoned with NaN and laid open), against the float64 reference of each pass
(tests/loudness_ref.py) on the rows, lengths and bounds of tests/loudness_cases.py: pass 1's chunk end states and peaks, the scan's
start states at every chunk (tile and workgroup-span seams named), the energy shares pa / pb with their exact zeros and the segment
sums, the gate from the device's own shares, L end to end, and the exact properties: both staging forms bit for bit, a row alone
against the row in its batch, the poison kept behind every row, no NaN from behind n[r], stn_op_loudness on the same call and on a
dirty scratch.  Every test asserts the staging form that ran first.

Bounds: 4 x the deviation of the float32 sequential restatement (no FMA) from float64, normalized as tests/loudness_cases.py says; none
comes from a kernel.  The restatement's own deviation / the largest the MI355X showed, same normalization, per rate:

    rate     end states           start states         pa / pb              segments
    8000     3.0e-05 / 2.5e-05    6.8e-05 / 4.2e-05    1.8e-05 / 1.6e-05    1.9e-06 / 2.4e-06
    11025    5.5e-05 / 3.7e-05    1.0e-04 / 8.1e-05    1.5e-05 / 1.6e-05    1.4e-06 / 1.3e-06
    22050    1.0e-04 / 7.9e-05    4.4e-04 / 3.5e-04    1.2e-04 / 1.1e-04    1.6e-05 / 1.0e-05
    44100    2.3e-04 / 1.9e-04    1.5e-03 / 1.2e-03    4.7e-04 / 3.3e-04    3.1e-05 / 2.4e-05
    48000    2.8e-04 / 2.3e-04    1.8e-03 / 1.2e-03    3.8e-04 / 3.7e-04    4.8e-05 / 4.3e-05
    88200    4.4e-04 / 2.9e-04    7.1e-03 / 4.3e-03    1.0e-03 / 1.5e-03    7.8e-05 / 1.4e-04
    96000    5.2e-04 / 3.1e-04    9.6e-03 / 5.9e-03    1.0e-03 / 1.1e-03    1.6e-04 / 1.2e-04
    176400   8.7e-04 / 5.2e-04    2.1e-02 / 1.6e-02    2.9e-03 / 2.7e-03    1.5e-04 / 5.9e-04
    192000   1.1e-03 / 6.9e-04    2.5e-02 / 1.8e-02    3.1e-03 / 3.6e-03    2.8e-04 / 3.6e-04

and |dL| against the float64 L under the same coefficients at most 2.2e-05 LU up to 48 kHz (48 kHz, the tone row) and 4.5e-05, 1.5e-04,
3.3e-04 and 7.7e-05 LU at 88.2, 96, 176.4 and 192 kHz (the tone row each time; allowed there 1.4e-03 to 4.8e-03).  Measured over bound
at the four rates above 48 kHz, worst pass: 0.45, 0.27, 0.96 and 0.32.  The 0.96 is the segment sums at 176.4 kHz (5.9e-04 of the tone
row's largest segment against 4 x 1.5e-04): the kernels' error there is 3.8 x the restatement's although pa / pb stay at its level, the
closest any pass comes to its bound.  Above 48 kHz W is per rate (loudness_cases.width: 6 * 32768 + 40 at 176.4 and 192 kHz, seven
scan tiles, WIDE_SEAMS), and pb must be nonzero at exactly the chunks a segment boundary cuts (9, 9, 8, 2 on the four live rows at
88.2 kHz; 8, 6, 8, 2 at 176.4 kHz).

These tests found a fault.  With the scan in fp32, pa on the tone row (0.1 DC offset) was 2.23e-03 at 44.1 kHz and 2.12e-03 at 48 kHz,
4.7 and 5.5 x the restatement, and L of that row was off by 8.5e-04 LU, although the start states were within their bound component by
component: the powers of M hold entries near +-27 that almost cancel (the high-pass's pole is nearly double), and the fp32 rounding of
P o fell on the combination of t1 and t2 the output is most sensitive to.  A float32 numpy model of the scan reproduced it (2.0e-03 at
48 kHz) and showed double arithmetic on a double table bringing it to the restatement's own level; the scan kernel now runs that way.

(test_zz_report_measured prints the table.)"""
import math

import numpy as np
import pytest

from supertonic_amd import binding
import loudness_cases as lc
from loudness_ref import CHUNK, chunks, gate_from_segments, integrated_loudness, segments_from_shares

pytestmark = pytest.mark.gpu
POISON = 0x7FC00000
SEAMS = (255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)  # chunks around a workgroup span's end and the scan's tile ends
WIDE_SEAMS = SEAMS + (3071, 3072, 3073, 4095, 4096, 4097, 5119, 5120, 5121, 6143, 6144, 6145)  # at 176.4 and 192 kHz: seven tiles
FORMS = ("vec", "scalar_w1", "scalar_misaligned")
TARGET, CEIL = -20.0, -1.0
MEASURED = {}


def _seams(c):
    return WIDE_SEAMS if c.W == lc.W_WIDE else SEAMS


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


_runs = {}


def _run(eng, hz, form):
    """one call per (rate, form), shared by the tests and left unchanged: W with 16-byte loads, W + 1, and W uploaded 4 bytes off"""
    if (hz, form) not in _runs:
        c = lc.case(hz)
        x = c.x if form == "scalar_w1" else np.ascontiguousarray(c.x[:, : c.W])
        o = eng.op_loudness_ex(x, hz, c.n, on=True, target_lufs=TARGET, ceiling_dbfs=CEIL, x_misalign=int(form == "scalar_misaligned"))
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _runs[(hz, form)] = o
    return _runs[(hz, form)]


def _form_ran(o, form):
    assert o["form"] == ("vec" if form == "vec" else "scalar"), (form, o["form"])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _live(c, Ks):
    """[6, Ks]: chunk k of row r holds samples of the row"""
    return np.arange(Ks)[None, :] < ((c.n + CHUNK - 1) // CHUNK)[:, None]


def _worst(name, hz, value):
    MEASURED[(name, hz)] = max(MEASURED.get((name, hz), 0.0), value)


def _check_states(c, got, ref, scale, bound, what, hz, form):
    """|got - ref| <= bound * scale at every live chunk, exact where the scale is 0; the failure names row, chunk and any seam"""
    K = ref.shape[1]
    live = ~np.isnan(ref)
    d = np.abs(np.where(live, got[:, :K].astype(np.float64) - np.nan_to_num(ref), 0.0))
    assert not np.isnan(got[:, :K][live]).any(), (what, hz, form)
    s = np.broadcast_to(scale, d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(s > 0, d / s, np.where(d > 0, np.inf, 0.0))
    bad = np.argwhere(rel > bound)
    seams = {k: float(rel[:, k].max()) for k in _seams(c) if k < K}
    assert bad.size == 0, (what, hz, form, f"bound {bound:.2e}", [(lc.NAMES[r], f"chunk {k}", "s1 s2 t1 t2".split()[q], f"{rel[r, k, q]:.2e}")
                                                                 for r, k, q in bad[:6]], "at the seams", seams)
    _worst(what, hz, float(rel.max()))
    return seams


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hz", lc.RATES)
def test_pass1_end_states_and_peaks(eng, hz, form):
    c, o = lc.case(hz), _run(eng, hz, form)
    _form_ran(o, form)
    _check_states(c, o["st_end"], c.ref["end"], c.scale["end"], c.bound["end"], "end", hz, form)
    Ks = o["pk"].shape[1]
    W = Ks * CHUNK
    xs = np.abs(np.pad(np.nan_to_num(c.x), ((0, 0), (0, W - c.x.shape[1]))).reshape(6, -1, CHUNK)[:, :Ks])
    live = _live(c, Ks)
    assert np.array_equal(o["pk"][live], xs.max(axis=2)[live])  # exact: max is order-independent
    for r in range(6):
        want = np.abs(c.x[r, : c.n[r]]).max() if c.n[r] else 0.0
        assert o["peak"][r] == np.float32(want), (hz, form, r)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hz", lc.RATES)
def test_scan_start_states_at_every_chunk(eng, hz, form):
    c, o = lc.case(hz), _run(eng, hz, form)
    _form_ran(o, form)
    K = c.ref["start"].shape[1]
    assert all(not np.isnan(c.ref["start"][:, k]).all() for k in _seams(c)), "a row reaches every seam"
    # a row in the last tile and the last span: at W = 3 * 32768 + 40 four scan tiles and 13 workgroup spans, at 6 * 32768 + 40 seven and 25
    assert K > c.W // lc.TILE * 1024 and (c.n > c.W // lc.SPAN * lc.SPAN).any()
    seams = _check_states(c, o["st_start"], c.ref["start"], c.scale["start"], c.bound["start"], "start", hz, form)
    assert set(seams) == set(_seams(c))
    assert np.all(_bits(o["st_start"][:, 0])[c.n > 0] == 0)  # the first chunk starts from +0.0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hz", lc.RATES)
def test_energy_shares_and_segments(eng, hz, form):
    c, o = lc.case(hz), _run(eng, hz, form)
    _form_ran(o, form)
    K = c.ref["pa"].shape[1]
    live = _live(c, K)
    # the samples a share sums: pa's run from the chunk's first sample, pb's from the next segment's first, both below the whole segments
    k0 = np.arange(K)[None, :] * CHUNK
    full = (c.n // c.hop * c.hop)[:, None]
    nxt = (k0 // c.hop + 1) * c.hop
    has = {"pa": live & (k0 < full), "pb": live & (nxt < np.minimum(k0 + CHUNK, full))}
    for key in ("pa", "pb"):
        got, ref = o[key][:, :K], c.ref[key]
        assert not np.isnan(got[live]).any(), (key, hz, form)
        none = live & ~has[key]
        assert np.all(ref[none] == 0) and np.all(_bits(got)[none] == 0), (key, hz, form)  # no samples: +0.0, bit for bit
        d = np.where(live, np.abs(got.astype(np.float64) - ref), 0.0)
        s = np.broadcast_to(c.scale["share"], d.shape)
        assert np.all(d[s == 0] == 0), (key, hz, form)
        rel = np.where(s > 0, d / np.where(s > 0, s, 1.0), 0.0)
        bad = np.argwhere(rel > c.bound["share"])
        assert bad.size == 0, (key, hz, form, f"bound {c.bound['share']:.2e}", [(lc.NAMES[r], f"chunk {q}", f"{rel[r, q]:.2e}") for r, q in bad[:6]])
        _worst("share", hz, float(rel.max()))
    # pb is nonzero exactly where a chunk straddles into a whole segment (and the row is not silent there)
    nz = live & (o["pb"][:, :K] != 0)
    assert np.all(has["pb"][nz]) and np.all(nz[has["pb"] & (c.ref["pb"] > 0)]), (hz, form)
    if hz in lc.STRADDLING:
        # the segment boundaries inside a row's whole segments that fall inside a chunk: 20 or more on the longest row up to 48 kHz, all
        # there are above (9 of 10 at 88.2 kHz, where 8 hop is a multiple of 32; 8 of 10 at 176.4 kHz, where 4 hop and 8 hop are)
        cuts = np.array([sum(j * c.hop % CHUNK != 0 for j in range(1, int(c.n[r]) // c.hop)) for r in range(6)])
        assert np.array_equal(nz.sum(axis=1)[: lc.ZERO], cuts[: lc.ZERO]), (hz, nz.sum(axis=1), cuts)
        assert nz.sum(axis=1).max() >= (8 if hz in lc.HIGH else 20) and (nz.sum(axis=1) >= 2).sum() >= 3, (hz, nz.sum(axis=1))
    else:
        assert not has["pb"].any() and not nz.any()
    for r in range(6):
        seg = segments_from_shares(o["pa"][r], o["pb"][r], c.n[r], c.hop)
        ref, s = c.ref["seg"][r], c.scale["seg"][r]
        assert seg.shape == ref.shape
        if s == 0:
            assert not seg.any(), (hz, form, r)
            continue
        rel = np.abs(seg - ref) / s
        assert rel.max() <= c.bound["seg"], (hz, form, lc.NAMES[r], f"segment {int(rel.argmax())}", f"{rel.max():.2e}", f"bound {c.bound['seg']:.2e}")
        _worst("seg", hz, float(rel.max()))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hz", lc.RATES)
def test_gate_from_the_devices_own_shares(eng, hz, form):
    c, o = lc.case(hz), _run(eng, hz, form)
    _form_ran(o, form)
    off = eng.op_loudness_ex(np.ascontiguousarray(c.x[:, : c.W]), hz, c.n, on=False, target_lufs=TARGET, ceiling_dbfs=CEIL)
    assert np.all(_bits(off["gain"]) == _bits(np.float32(1.0))) and np.array_equal(_bits(off["lufs"]), _bits(_run(eng, hz, "vec")["lufs"]))
    defined = capped = 0
    for r in range(6):
        seg = segments_from_shares(o["pa"][r], o["pb"][r], c.n[r], c.hop)
        L, gain, margin = gate_from_segments(seg, c.hop, True, TARGET, CEIL, float(o["peak"][r]))
        assert margin >= 1e-4, (hz, form, lc.NAMES[r], margin)
        if math.isinf(L):
            assert o["lufs"][r] == -np.inf and _bits(o["gain"][r:r + 1])[0] == _bits(np.float32(1.0)), (hz, form, r)
            continue
        defined += 1
        capped += 10 ** (CEIL / 20) / float(o["peak"][r]) < 10 ** ((TARGET - L) / 20)
        assert abs(float(o["lufs"][r]) - L) <= 1e-5, (hz, form, lc.NAMES[r], o["lufs"][r], L)
        assert abs(float(o["gain"][r]) - gain) <= 2e-7 * gain, (hz, form, lc.NAMES[r], o["gain"][r], gain)
    assert defined >= 2 and all(o["lufs"][r] == -np.inf for r in (lc.SHORT, lc.ZERO, lc.EMPTY))
    MEASURED[("capped", hz)] = capped


@pytest.mark.parametrize("hz", lc.RATES)
def test_end_to_end_against_float64(eng, hz):
    """L against the float64 L of the same rows under the same fp32 coefficients, held to what the segment bound allows
    (loudness_cases.dl_bound); the distance from the all-float64 BS.1770-4 reading and from the suite's older 0.01 LU is printed"""
    c, o = lc.case(hz), _run(eng, hz, "vec")
    _form_ran(o, "vec")
    out = []
    for r in range(6):
        L = c.gate[r][0]
        if math.isinf(L):
            assert o["lufs"][r] == -np.inf
            continue
        assert c.gate[r][2] >= 1e-4
        dl, allowed = abs(float(o["lufs"][r]) - L), lc.dl_bound(c, r) + 2.0 ** -20  # (+ half an ulp of an fp32 L below 32 in magnitude)
        std = abs(float(o["lufs"][r]) - integrated_loudness(c.x[r, : c.n[r]].astype(np.float64), hz))
        out.append(f"{lc.NAMES[r]} {dl:.1e} (allowed {allowed:.1e}; {std:.1e} from float64 BS.1770, {0.01 / max(std, 1e-12):.0f} x under 0.01)")
        assert dl <= allowed, (hz, lc.NAMES[r], dl, allowed)
        _worst("dL", hz, dl)
    assert out
    print(f"\n{hz} Hz |dL|: " + "; ".join(out))


@pytest.mark.parametrize("hz", lc.RATES)
def test_forms_and_batches_agree_bit_for_bit(eng, hz):
    c = lc.case(hz)
    v, w1, mis = (_run(eng, hz, f) for f in FORMS)
    _form_ran(v, "vec"), _form_ran(w1, "scalar_w1"), _form_ran(mis, "scalar_misaligned")
    Ks = v["pk"].shape[1]
    assert w1["pk"].shape[1] == chunks(c.W + 1) == Ks
    live = _live(c, Ks)
    for key in ("st_end", "st_start", "pk", "pa", "pb", "lufs", "peak", "gain"):
        assert np.array_equal(_bits(v[key]), _bits(mis[key])), (hz, key)  # the same W: the whole buffers, poison included
        a, b = v[key], w1[key][:, :Ks] if w1[key].ndim > 1 else w1[key]
        sel = live if a.ndim > 1 else slice(None)
        assert np.array_equal(_bits(a)[sel], _bits(b)[sel]), (hz, key)
    # a row alone (n = None: the whole of its W) against the row in the batch, in both forms where its length allows
    for r in (lc.TONE, lc.NOISE, lc.QUIET_LOUD, lc.SHORT):
        n = int(c.n[r])
        one = eng.op_loudness_ex(c.x[r:r + 1, :n], hz)
        assert one["form"] == ("vec" if n % 4 == 0 else "scalar")
        K = chunks(n)
        for key in ("st_end", "st_start", "pk", "pa", "pb"):
            assert np.array_equal(_bits(one[key][0, :K]), _bits(v[key][r, :K])), (hz, lc.NAMES[r], key)
        for key in ("lufs", "peak"):
            assert _bits(one[key])[0] == _bits(v[key][r:r + 1])[0], (hz, lc.NAMES[r], key)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hz", lc.RATES)
def test_poison_stays_behind_every_row_and_no_nan_comes_in(eng, hz, form):
    c, o = lc.case(hz), _run(eng, hz, form)
    _form_ran(o, form)
    Ks = o["pk"].shape[1]
    live = _live(c, Ks)
    assert (~live).any() and (~live[lc.EMPTY]).all()
    for key in ("st_end", "st_start", "pk", "pa", "pb"):
        b = _bits(o[key])
        assert np.all(b[~live] == POISON), (hz, form, key)  # nothing written behind lo_chunks(n_r)
        assert not np.isnan(o[key][live]).any(), (hz, form, key)  # x behind n[r] is NaN: none of it reached a written element
    for key in ("lufs", "peak", "gain"):
        assert not np.isnan(o[key]).any(), (hz, form, key)


@pytest.mark.parametrize("hz", lc.RATES)
def test_the_plain_op_is_the_same_measurement_and_ignores_dirty_scratch(eng, hz):
    c, o = lc.case(hz), _run(eng, hz, "vec")
    _form_ran(o, "vec")
    x = np.ascontiguousarray(c.x[:, : c.W])
    lufs, peak = eng.op_loudness(x, hz, c.n)
    assert np.array_equal(_bits(lufs), _bits(o["lufs"])) and np.array_equal(_bits(peak), _bits(o["peak"]))
    # a larger call of other rows leaves its values all over the grow-only scratch; the smaller call after it reads none of them
    rng = np.random.default_rng(hz)
    eng.op_loudness(rng.standard_normal((8, c.W + 4096)).astype(np.float32), hz)
    sub = [lc.NOISE, lc.QUIET_LOUD, lc.SHORT, lc.TONE]
    l2, p2 = eng.op_loudness(x[sub], hz, c.n[sub])
    assert np.array_equal(_bits(l2), _bits(o["lufs"][sub])) and np.array_equal(_bits(p2), _bits(o["peak"][sub]))


def test_ex_refuses_what_the_op_refuses(eng):
    x = np.zeros((1, 100), np.float32)
    for hz in (7999, 192001):
        with pytest.raises(binding.StnError):
            eng.op_loudness_ex(x, hz)
    with pytest.raises(binding.StnError):
        eng.op_loudness_ex(x, 16000, [101])
    with pytest.raises(binding.StnError):
        eng.op_loudness_ex(x, 16000, [-1])
    with pytest.raises(binding.StnError):
        eng.op_loudness_ex(x, 16000, x_misalign=2)
    assert eng.op_loudness_ex(x, 16000)["form"] == "vec" and eng.op_loudness_ex(x, 16000, x_misalign=1)["form"] == "scalar"
    assert eng.op_loudness_ex(x[:, :99], 16000)["form"] == "scalar"


def test_zz_report_measured():
    print("\nrate     " + "".join(f"{k:<22}" for k in ("end states", "start states", "pa / pb", "segments")) + "max |dL| LU   rows at the ceiling")
    for hz in lc.RATES:
        c = lc.case(hz)
        cells = "".join(f"{c.f32[k]:.1e} / {MEASURED.get((k, hz), float('nan')):.1e}   " for k in ("end", "start", "share", "seg"))
        print(f"{hz:<9}{cells}{MEASURED.get(('dL', hz), float('nan')):.1e}       {MEASURED.get(('capped', hz), '-')}")
    print("(float32 restatement / measured, each normalized by the row's scale; the bound is 4 x the first)")
