"""The launches of kernels_edges.hip (DESIGN.md sections 14 and 17) pass by pass on an MI355X, through stn_op_silence_edges_ex
(Engine::ed_enqueue itself, every word of its scratch poisoned with 0x7FC00000 and the scratch laid open), against the float64
references of tests/silence_cases.py on its rows, spans and bounds: the frame pass's chunk shares pa / pb with their exact zeros, the
row pass's levels (bit for bit the double recombination of the device's own shares, and within the bound of float64), the decisions
of the row pass and the pause pass without any margin (exactly the host rule stn_pause_plan on the device's own levels, frames built
to lie within 1e-5 of the threshold included), and the exact properties: the three staging forms bit for bit, a row alone against the
row in its batch, the poison kept behind every row, no NaN from behind n[r], the plain ops on the same operands and on a dirty
scratch.  Every test asserts the staging form that ran first.

Bounds (derived in tests/silence_cases.py, none taken from a kernel): a share within (L + 1) * 2^-24 of its float64 value, L <= 32 its
number of samples; a level within 34 * 2^-24 = 2.03e-6 of its float64 value (under 1e-5 dB).  tests/test_silence_kernels_cpu.py shows
that six faults of the decomposition each break them.  The largest |error| / bound the MI355X showed, per case, over the three forms,
and the picked frames of the two near-threshold rows (top_db 40) that the device put on the other side of the threshold than float64
does.  The float32 sequential restatement without FMA gives the same figures: on these rows the kernels' shares equal it bit for bit
(the build does not contract, -ffp-contract=off), which the report prints and nothing asserts.

    case        pa / pb    lev      picked frames decided against float64
    8000        0.25       0.084    29 of 273
    11025       0.50       0.070    26 of 198
    16000       0.24       0.070    11 of 136
    22050       0.39       0.075    16 of 98
    44100       0.39       0.047    6 of 49
    48000       0.37       0.043    8 of 45
    88200       0.30       0.054    3 of 24
    96000       0.21       0.100    1 of 22
    176400      0.23       0.091    1 of 16
    192000      0.16       0.061    1 of 16
    8000 long   0.27       0.117    158 of 1373

No test found a fault in the kernels.  The poison is 0x7FC00000 in every 32-bit word; read as a double two such words are not a NaN
but 2^1021 * 1.0000005, so the levels behind a row are compared as bits (POISON64) and the levels in front must be at most 1.

pb is nonzero at exactly the chunks a frame boundary cuts inside the span (PB_COUNTS: per rate, on the noise rows of spans W, 8192 and
2 F) and +0.0, bit for bit, everywhere else: at every chunk of the four rates whose frame is a multiple of 32.

(test_zz_report_measured prints the table.)"""
import itertools

import numpy as np
import pytest

from supertonic_amd import binding
import pause_ref as pz
import silence_cases as sc

pytestmark = pytest.mark.gpu
POISON = 0x7FC00000
POISON64 = 0x7FC000007FC00000
FORMS = ("vec", "scalar_w1", "scalar_misaligned")
KEEP_MS, FADE_MS = 20.0, 5.0
CAP = binding.PAUSE_MAX_CUTS
SEAMS = (255, 256, 257, 511, 512, 513)  # chunks around the ends of the frame pass's first two workgroup spans
# chunks with a nonzero pb on the noise rows of spans W, 8192 and 2 F (the others, F, 33, 31 and 0, have none): the frame boundaries
# j F < n that are no multiple of 32
PB_COUNTS = {"8000": (103, 51, 1), "11025": (140, 70, 1), "16000": (0, 0, 0), "22050": (72, 36, 1), "44100": (36, 18, 1), "48000": (0, 0, 0),
             "88200": (17, 9, 1), "96000": (0, 0, 0), "176400": (11, 4, 1), "192000": (0, 0, 0), sc.LONG: (515, 51, 1)}
MEASURED = {}


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


_runs = {}


def _operand(c, form):
    return c.x if form == "scalar_w1" else np.ascontiguousarray(c.x[:, : c.W])


def _run(eng, key, form):
    """one call per (case, form), shared by the tests and left unchanged: W with 16-byte loads, W + 1, and W uploaded 4 bytes off"""
    if (key, form) not in _runs:
        c = sc.get(key)
        o = eng.op_silence_edges_ex(_operand(c, form), c.hz, c.n, sc.TOP_DB, KEEP_MS, FADE_MS, sc.MAX_PAUSE_MS,
                                    x_misalign=int(form == "scalar_misaligned"), cap_pairs=CAP)
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _runs[(key, form)] = o
    return _runs[(key, form)]


def _form_ran(o, form):
    assert o["form"] == ("vec" if form == "vec" else "scalar"), (form, o["form"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _worst(name, key, value):
    MEASURED[(name, key)] = max(MEASURED.get((name, key), 0.0), value)


def test_the_rates_are_those_of_the_decision_tests():
    import test_gpu_silence
    assert list(sc.RATES) == test_gpu_silence.RATES


# ---- the frame pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", sc.KEYS)
def test_frame_pass_shares(eng, key, form):
    c, o = sc.get(key), _run(eng, key, form)
    _form_ran(o, form)
    pa, pb = o["pa"][:, : c.Ks], o["pb"][:, : c.Ks]
    assert not np.isnan(pa[c.live]).any() and not np.isnan(pb[c.live]).any(), (key, form)
    ra, rb = sc.share_ratios(c, pa, pb)
    for name, rel in (("pa", ra), ("pb", rb)):
        bad = np.argwhere(rel > 1.0)
        assert bad.size == 0, (name, key, form, [(c.names[r], f"chunk {k}", f"{rel[r, k]:.3g} x the bound") for r, k in bad[:6]],
                               "at the seams", {k: float(rel[:, k].max()) for k in SEAMS})
        _worst("share", key, float(rel.max()))
    assert all(c.live[:, k].any() for k in SEAMS), "a row reaches both workgroup seams"
    # no samples, no share: +0.0 bit for bit; at the rates whose frame is a multiple of 32 that is every pb
    assert np.all(c.La[c.live] > 0) and np.all(_bits(pb)[c.live & (c.Lb == 0)] == 0), (key, form)
    if c.hz in sc.ALIGNED:
        assert np.all(_bits(pb)[c.live] == 0)
    # and on the noise rows pb is nonzero at exactly the other chunks
    noise = [r for r, (s, _) in enumerate(c.rows) if s == sc.NOISE]
    for r in noise:
        assert np.array_equal(c.live[r] & (pb[r] != 0), c.Lb[r] > 0), (key, form, c.names[r])
    assert tuple(int(np.count_nonzero(pb[r][c.live[r]])) for r in noise[:3]) == PB_COUNTS[key], (key, form)
    assert all(not np.count_nonzero(pb[r][c.live[r]]) for r in noise[3:])
    same = np.array_equal(_bits(pa)[c.live], _bits(c.pa32)[c.live]) and np.array_equal(_bits(pb)[c.live], _bits(c.pb32)[c.live])
    MEASURED[("restated", key)] = MEASURED.get(("restated", key), True) and same


# ---- the row pass ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", sc.KEYS)
def test_row_pass_levels(eng, key, form):
    c, o = sc.get(key), _run(eng, key, form)
    _form_ran(o, form)
    for r in range(c.R):
        K = int(c.frames[r])
        lev = o["lev"][r, :K]
        assert not np.isnan(lev).any(), (key, form, c.names[r])
        # the device's own shares, summed in double in chunk order and divided once by the frame's own length
        own = sc.recombine(o["pa"][r], o["pb"][r], c.n[r], c.F)
        assert np.array_equal(_bits(lev), _bits(own)), (key, form, c.names[r], np.flatnonzero(lev != own)[:6])
        sig = c.rows[r][0]
        if sig == sc.QUARTER:  # exact squares, exact sums: every frame, the short last one included
            assert np.all(lev == 0.0625), (key, form, c.names[r])
        if sig == sc.ZERO:
            assert np.all(_bits(lev) == 0)
    rel = sc.level_ratios(c, o["lev"])
    for r in range(c.R):
        if rel[r].size:
            k = int(rel[r].argmax())
            assert rel[r][k] <= 1.0, (key, form, c.names[r], f"frame {k} of {rel[r].size}", f"{rel[r][k]:.3g} x the bound")
            _worst("lev", key, float(rel[r][k]))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", sc.KEYS)
def test_poison_stays_behind_every_row_and_no_nan_comes_in(eng, key, form):
    c, o = sc.get(key), _run(eng, key, form)
    _form_ran(o, form)
    Ks, Kf = o["pa"].shape[1], o["lev"].shape[1]
    live = np.arange(Ks)[None, :] < (-(-c.n // sc.CHUNK))[:, None]
    framed = np.arange(Kf)[None, :] < c.frames[:, None]
    empty = int(np.flatnonzero(c.n == 0)[0])
    assert (~live).any() and (~framed).any() and not live[empty].any() and not framed[empty].any()
    for k in ("pa", "pb"):
        assert np.all(_bits(o[k])[~live] == POISON), (key, form, k)  # nothing written at or behind chunk ceil(n / 32)
        assert not np.isnan(o[k][live]).any(), (key, form, k)  # x behind n[r] is NaN: none of it reached a written element
    # (two poison words read as a double are no NaN but 2^1021 * 1.0000005: as unmistakable, and compared as bits)
    assert np.all(_bits(o["lev"])[~framed] == POISON64) and np.all(o["lev"][framed] <= 1.0) and not np.isnan(o["lev"][framed]).any(), (key, form)
    assert np.array([POISON64], np.uint64).view(np.float64)[0] > 2.0 ** 1021


# ---- the decisions, without any margin ---------------------------------------------------------------------------------------------
def _check_decisions(c, o, top_db, keep_ms, what):
    """start, end, n_cuts, len and the cuts: the host rule on the device's own levels, exactly; pause_ref.plan_levels on the same levels;
    and, on the rows that clear MARGIN_DB in float64, the float64 rule.  -> (rows that clear the margin, picked frames the device put on
    the other side of the threshold than float64 does)"""
    clear = flipped = 0
    for r in range(c.R):
        n, K = int(c.n[r]), int(c.frames[r])
        lev = o["lev"][r, :K]
        s, e, cuts, nc = binding.pause_plan(lev, n, c.hz, top_db, keep_ms, sc.MAX_PAUSE_MS, CAP)
        got = (int(o["start"][r]), int(o["end"][r]), int(o["n_cuts"][r]))
        assert got == (s, e, nc), (what, c.names[r], got, (s, e, nc))
        assert np.array_equal(o["cuts"][r, :nc], cuts) and np.all(o["cuts"][r, nc:] == -1), (what, c.names[r])
        assert int(o["len"][r]) == e - s - int((cuts[:, 1] - cuts[:, 0]).sum()), (what, c.names[r])
        s2, e2, cuts2, _ = pz.plan_levels(lev, n, c.hz, top_db, keep_ms, sc.MAX_PAUSE_MS)
        assert (s2, e2, cuts2) == (s, e, [tuple(p) for p in cuts.tolist()]), (what, c.names[r])
        s64, e64, cuts64, margin = pz.plan_levels(c.lev64[r], n, c.hz, top_db, keep_ms, sc.MAX_PAUSE_MS)
        if margin >= pz.MARGIN_DB:
            clear += 1
            assert (s64, e64, cuts64) == (s2, e2, cuts2), (what, c.names[r], margin)
        if r in c.near and top_db == sc.TOP_DB:
            d = c.near[r]
            assert margin < 1e-4
            flipped += int(np.count_nonzero((lev[d["picked"]] >= lev.max() * 10.0 ** (-top_db / 10.0)) != (c.lev64[r][d["picked"]] >= d["thr"])))
    return clear, flipped


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", sc.KEYS)
def test_decisions_equal_the_host_rule_on_the_devices_own_levels(eng, key, form):
    c, o = sc.get(key), _run(eng, key, form)
    _form_ran(o, form)
    clear, flipped = _check_decisions(c, o, sc.TOP_DB, KEEP_MS, (key, form))
    assert clear >= 8, (key, clear)  # (most designed rows are far from the threshold: there float64 decides the same)
    assert o["n_cuts"][c.NEAR_PAUSE] >= 1  # (two picked frames 1e-5 under the threshold beside a quiet one: 30 ms of pause at least)
    MEASURED[("flipped", key)] = flipped
    if form != "vec":
        return
    x = _operand(c, form)
    for top_db, keep_ms in itertools.product((30.0, 40.0, 50.0), (0.0, 20.0)):
        if (top_db, keep_ms) == (sc.TOP_DB, KEEP_MS):
            continue
        other = eng.op_silence_edges_ex(x, c.hz, c.n, top_db, keep_ms, FADE_MS, sc.MAX_PAUSE_MS, cap_pairs=CAP)
        _form_ran(other, form)
        assert np.array_equal(_bits(other["lev"]), _bits(o["lev"]))  # the levels do not depend on the parameters
        _check_decisions(c, other, top_db, keep_ms, (key, top_db, keep_ms))


# ---- exact properties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sc.KEYS)
def test_forms_and_batches_agree_bit_for_bit(eng, key):
    c = sc.get(key)
    v, w1, mis = (_run(eng, key, f) for f in FORMS)
    _form_ran(v, "vec"), _form_ran(w1, "scalar_w1"), _form_ran(mis, "scalar_misaligned")
    for k in ("pa", "pb", "lev", "start", "end", "len", "n_cuts", "cuts"):
        assert v[k].shape == mis[k].shape and v[k].tobytes() == mis[k].tobytes(), (key, k)  # the same W: the whole buffers, poison included
    framed = np.arange(c.Kf)[None, :] < c.frames[:, None]
    assert np.array_equal(_bits(v["pa"])[c.live], _bits(w1["pa"][:, : c.Ks])[c.live]) and np.array_equal(_bits(v["pb"])[c.live], _bits(w1["pb"][:, : c.Ks])[c.live])
    assert np.array_equal(_bits(v["lev"])[framed], _bits(w1["lev"][:, : c.Kf])[framed])
    for k in ("start", "end", "len", "n_cuts", "cuts"):
        assert np.array_equal(v[k], w1[k]), (key, k)
    # a row alone at width n + 13 (NaN behind n) against the row in its batch, over its own chunks and frames
    for r in range(c.R):
        n = int(c.n[r])
        if n == 0:
            continue
        x = np.full((1, n + 13), np.nan, np.float32)
        x[0, :n] = c.x[r, :n]
        one = eng.op_silence_edges_ex(x, c.hz, [n], sc.TOP_DB, KEEP_MS, FADE_MS, sc.MAX_PAUSE_MS, cap_pairs=CAP)
        assert one["form"] == ("vec" if (n + 13) % 4 == 0 else "scalar")
        Kc, K = -(-n // sc.CHUNK), int(c.frames[r])
        for k in ("pa", "pb"):
            assert np.array_equal(_bits(one[k][0, :Kc]), _bits(v[k][r, :Kc])), (key, c.names[r], k)
        assert np.array_equal(_bits(one["lev"][0, :K]), _bits(v["lev"][r, :K])), (key, c.names[r])
        for k in ("start", "end", "len", "n_cuts", "cuts"):
            assert np.array_equal(one[k][0], v[k][r]), (key, c.names[r], k)


@pytest.mark.parametrize("key", sc.KEYS)
def test_the_plain_ops_return_the_same_tables_and_ignore_dirty_scratch(eng, key):
    c, o = sc.get(key), _run(eng, key, "vec")
    _form_ran(o, "vec")
    x = _operand(c, "vec")
    eng.op_silence_edges_ex(x, c.hz, c.n, sc.TOP_DB, KEEP_MS, FADE_MS, sc.MAX_PAUSE_MS, cap_pairs=CAP)  # (leaves poison and its tables behind)
    for again in range(2):  # the second call finds what the first one left
        s, e = eng.op_silence_edges(x, c.hz, c.n, sc.TOP_DB, KEEP_MS)
        assert np.array_equal(s, o["start"]) and np.array_equal(e, o["end"]), (key, again)
        p = eng.op_pause_trim(x, c.hz, c.n, sc.TOP_DB, KEEP_MS, FADE_MS, sc.MAX_PAUSE_MS, None, "f32", cap_pairs=CAP)
        for k in ("start", "end", "len", "n_cuts", "cuts"):
            assert np.array_equal(p[k], o[k]), (key, again, k)
    # without the pause pass: the same edges, no cuts
    plain = eng.op_silence_edges_ex(x, c.hz, c.n, sc.TOP_DB, KEEP_MS, FADE_MS, 0.0, cap_pairs=CAP)
    assert np.array_equal(plain["start"], o["start"]) and np.array_equal(plain["end"], o["end"]) and not plain["n_cuts"].any()
    assert np.array_equal(plain["len"], o["end"] - o["start"]) and np.all(plain["cuts"] == -1)
    assert np.array_equal(_bits(plain["lev"]), _bits(o["lev"]))


def test_ex_refuses_what_the_ops_refuse(eng):
    x = np.zeros((1, 100), np.float32)
    for hz in (7999, 192001):
        with pytest.raises(binding.StnError):
            eng.op_silence_edges_ex(x, hz)
    for kw in (dict(n=[101]), dict(n=[-1]), dict(x_misalign=2), dict(top_db=0.5), dict(top_db=121.0), dict(keep_ms=-1.0), dict(keep_ms=1001.0),
               dict(fade_ms=51.0), dict(max_pause_ms=19.0), dict(max_pause_ms=5001.0), dict(max_pause_ms=-20.0)):
        with pytest.raises(binding.StnError):
            eng.op_silence_edges_ex(x, 16000, **kw)
    assert eng.op_silence_edges_ex(x, 16000)["form"] == "vec" and eng.op_silence_edges_ex(x, 16000, x_misalign=1)["form"] == "scalar"
    assert eng.op_silence_edges_ex(x[:, :99], 16000)["form"] == "scalar"


def test_zz_report_measured():
    print("\ncase        pa / pb    lev      picked frames decided against float64    shares equal the restatement")
    for key in sc.KEYS:
        g = lambda name: MEASURED.get((name, key), float("nan"))
        flipped = f"{MEASURED.get(('flipped', key), '-')} of {sum(d['picked'].size for d in sc.get(key).near.values())}"
        print(f"{key:<12}{g('share'):<11.2f}{g('lev'):<9.3f}{flipped:<41}{MEASURED.get(('restated', key), '-')}")
    print("(largest |error| / bound over the three forms: (L + 1) * 2^-24 of a share, 34 * 2^-24 of a level)")
