"""The look-ahead peak limiter behind the loudness gain on an MI355X (include/stn.h "limiter"; kernels_limiter.hip; DESIGN.md section
15) against the numpy contract of tests/limiter_ref.py: the op on rows whose peaks sit at every place a tile, a halo or a span can get
wrong; a row under the ceiling; independence of the batch; every fetch path of a batch whose waveform stn_dbg_batch_set_wav replaced
with a quiet tone plus clicks, so that today's capped gain binds; trimmed and joined fetches; the off path; the refusals; and the
event-timed cost on a C3-sized batch.

Bounds: s is compared within (A + 8) * 2^-24 (limiter_ref.s_tol: sequential summation of A + 1 non-negative terms of total weight <= 1,
plus the weight, divide and final roundings), y within that times |v| plus 2^-23 |v| (the multiply's and the clamp's roundings).  Where
s == 1, the sample counts and the padding are compared exactly.

Above 48 kHz the op runs limiter_ref.long_case's rows (width max(20011, 20 A + 4096), tests/test_limiter_cpu.py proves what they hold) at
A = 1920 (192 kHz, 10 ms: LM_MAX_A), 960, 441 and 88, the envelope path at A = 1920, and the batch-level tests fetch at 88.2 and 192 kHz
(5 ms, and 10 ms at 192 kHz: the engine's own path to A = 1920).  Measured on an MI355X, worst |y - ref| / bound and |s - ref| / bound per
case: A = 4 0.151 / 0.171, A = 221 0.041 / 0.041, A = 1920 0.014 / 0.014, A = 960 0.026 / 0.018, A = 441 0.027 / 0.024, A = 88 0.058 / 0.057,
A = 1920 with the envelope 0.015 / 0.015; batch fetches 0.027 (88.2 kHz), 0.022 (192 kHz, 5 ms) and 0.014 (192 kHz, 10 ms)."""
import math

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
import join_ref
import limiter_ref as ref
import loudness_ref

pytestmark = pytest.mark.gpu
W_OP = 20011
DURS = np.array([0.71, 0.43, 0.92, 0.64, 0.51, 0.47], np.float32)
TARGET, CEIL, MS = -16.0, -1.0, 5.0


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_rows(got_y, got_s, outs, n, hz, ms, what):
    """device rows against the reference's: exact where the contract is exact, within the bounds elsewhere"""
    tol = ref.s_tol(hz, ms)
    worst_y = worst_s = 0.0
    for b, o in enumerate(outs):
        nb, c = int(n[b]), o["c"]
        y = got_y[b, : o["y"].size]
        assert np.abs(y).max() <= c, (what, b)
        assert _same(y[nb:], np.clip(o["v"][nb:], -c, c)), (what, b)  # the padding: the clamped product
        v = np.abs(o["v"].astype(np.float64))
        err = np.abs(y.astype(np.float64) - o["y"])
        worst_y = max(worst_y, float(np.max(err / (tol * v + 2.0 ** -23 * v + 1e-300))))
        print(f"{what} row {b} (n {nb}): limited {o['limited']}, max |y - ref| / bound {np.max(err / (tol * v + 2.0 ** -23 * v + 1e-300)):.3f}")
        assert np.all(err <= tol * v + 2.0 ** -23 * v), (what, b, float(err.max()))
        if got_s is not None:
            s = got_s[b]
            assert np.array_equal(s == 1.0, o["s"] == 1.0), (what, b)
            serr = np.abs(s.astype(np.float64) - o["s"])
            worst_s = max(worst_s, float(serr.max()) / tol)
            print(f"    max |s - ref| {serr.max():.3g} (bound {tol:.3g})")
            assert np.all(serr <= tol), (what, b, float(serr.max()))
            assert np.all(s[:nb] <= o["r"][:nb]), (what, b)
    return worst_y, worst_s


# ---- 1. the op against the reference ---------------------------------------------------------------------------------------------------
OP_CASES = [(8000, 0.5), (44100, 5.0)] + list(ref.LONG_CASES)  # A = 4, 221, then 1920 (LM_MAX_A), 960, 441, 88 above 48 kHz


def _op_rows(hz, ms, rep):
    """(x, n, g, outs, W): the rows of repeat rep and the reference's results; above 48 kHz the rows that scale with A (limiter_ref.long_case)"""
    if (hz, ms) in ref.LONG_CASES:
        x, n, g, outs = ref.long_case(hz, ms, CEIL, rep)
        return x, n, g, outs, x.shape[1]
    x, n, g = ref.peaky_rows(hz, ms, CEIL, W_OP, rep)
    return x, n, g, ref.limit_rows(x, n, g, CEIL, hz, ms), W_OP


@pytest.mark.parametrize("hz,ms", OP_CASES)
def test_op_equals_the_reference(eng, hz, ms):
    A = ref.samples(hz, ms)
    seen = []
    worst = [0.0, 0.0]
    for rep in (0, 1):
        x, n, g, outs, W = _op_rows(hz, ms, rep)
        seen += n.tolist()
        y, s, red, lim = eng.op_limiter(x, hz, n, g, CEIL, ms)
        worst = np.maximum(worst, _check_rows(y, s, outs, n, hz, ms, f"{hz} Hz rep {rep}")).tolist()
        assert lim.tolist() == [o["limited"] for o in outs]
        for b, o in enumerate(outs):
            smin = 10.0 ** (-o["reduction_db"] / 20.0)
            assert abs(float(red[b]) - o["reduction_db"]) <= 20.0 / math.log(10.0) * ref.s_tol(hz, ms) / smin + 1e-6 * o["reduction_db"], (b, red[b])
    if (hz, ms) in ref.LONG_CASES:
        tiles = range(ref.TILE, W, ref.TILE)
        assert set(seen) >= {0, 1, A, A + 1, 2 * A + 1, W, W - 1}
        assert sum(k - 1 in seen for k in tiles) >= 2 and sum(k + 1 in seen for k in tiles) >= 2
    else:
        assert set(seen) >= {0, 1, A, A + 1, 2 * A + 1, 4096, 4097, 8191, 16385, W_OP}
    # no lengths, no gain, a width that is a multiple of 4 (the 16-byte path of an untouched tile), no curve asked for
    if (hz, ms) in ref.LONG_CASES:
        x = np.pad(_op_rows(hz, ms, 1)[0], ((0, 0), (0, -W % 4)))
    else:
        x = np.ascontiguousarray(ref.peaky_rows(hz, ms, CEIL, W_OP + 1, 1)[0])
    Ww = x.shape[1]
    assert Ww % 4 == 0
    outs = ref.limit_rows(x, None, None, CEIL, hz, ms)
    y = np.empty_like(x)
    lim = np.empty(6, np.int64)
    eng._ck(eng._lib.stn_op_limiter(eng._h, hz, 6, Ww, x, None, None, CEIL, ms, y.ctypes.data, None, None, lim.ctypes.data))
    worst[0] = max(worst[0], _check_rows(y, None, outs, [Ww] * 6, hz, ms, f"{hz} Hz whole rows")[0])
    assert lim.tolist() == [o["limited"] for o in outs]
    print(f"{hz} Hz, {ms} ms (A = {A}): worst |y - ref| / bound {worst[0]:.3f}, worst |s - ref| / bound {worst[1]:.3f}")


def test_op_follows_the_true_peak_envelope_at_the_longest_look_ahead(eng):
    """A = 1920 with r from the envelope (stn_op_limiter_ex, peak mode "true": limiter_kernel<true>): the curve of the reference driven
    by the device's own envelope, within the bounds above; the envelope itself within truepeak_ref's bound."""
    import truepeak_ref as R
    hz, ms = 192000, 10.0
    A = ref.samples(hz, ms)
    seen = []
    wy = ws = 0.0
    for rep in (0, 1):  # the short spans 0, 1, A, A + 1, 2A + 1 and W, then the tile multiples +- 1 and W - 1
        x, n, g, _, W = _op_rows(hz, ms, rep)
        seen += n.tolist()
        op = eng.op_limiter_ex(x, hz, n, g, CEIL, ms, "true")
        outs = []
        for b in range(6):
            assert R.env_violations(op["env"][b], x[b], n[b], g[b]).size == 0, (rep, b)
            outs.append(dict(R.limit_row_env(x[b], n[b], g[b], CEIL, hz, ms, env=op["env"][b])))
            outs[b]["limited"] = int(np.count_nonzero(outs[b]["M"][: n[b]] < 1.0))
        y_s = _check_rows(op["y"], op["s"], outs, n, hz, ms, f"{hz} Hz true-peak envelope rep {rep}")
        wy, ws = max(wy, y_s[0]), max(ws, y_s[1])
        assert op["limited"].tolist() == [o["limited"] for o in outs]
        assert np.array_equal(op["limited"] > 0, n > 0)  # every row with a sample has its peak at sample 0
    assert set(seen) >= {0, 1, A, A + 1, 2 * A + 1, W, W - 1}
    print(f"{hz} Hz, {ms} ms, envelope: worst |y - ref| / bound {wy:.3f}, worst |s - ref| / bound {ws:.3f}")


# ---- 2. a row that never exceeds the ceiling ----------------------------------------------------------------------------------------------
def test_a_row_under_the_ceiling_is_the_plain_product(eng):
    rng = np.random.default_rng(3)
    x = (0.3 * rng.uniform(-1, 1, (3, 9001))).astype(np.float32)
    x[1, 100] = -0.0
    g = np.array([1.0, 2.5, 0.1], np.float32)
    c = ref.ceiling(CEIL)
    x[2, 4000] = c / g[2] * np.float32(0.999)  # close under the ceiling
    assert np.abs(x * g[:, None]).max() <= c
    y, s, red, lim = eng.op_limiter(x, 16000, [9001, 5000, 9001], g, CEIL, MS)
    assert _same(y, (x * g[:, None]).astype(np.float32))
    assert np.all(s == 1.0) and not lim.any() and not red.any()


# ---- 3. independence ---------------------------------------------------------------------------------------------------------------------
def test_a_rows_output_does_not_depend_on_the_batch(eng):
    _alone_equals_batched(eng, 44100, 5.0)


@pytest.mark.parametrize("hz,ms", ref.LONG_CASES)
def test_a_rows_output_does_not_depend_on_the_batch_above_48_khz(eng, hz, ms):
    _alone_equals_batched(eng, hz, ms)


def _alone_equals_batched(eng, hz, ms):
    for rep in (0, 1):
        x, n, g = _op_rows(hz, ms, rep)[:3]
        y, s, red, lim = eng.op_limiter(x, hz, n, g, CEIL, ms)
        for k in range(6):
            nk = int(n[k])
            if nk == 0:
                continue
            y1, s1, red1, lim1 = eng.op_limiter(x[k:k + 1, :nk], hz, None, g[k:k + 1], CEIL, ms)
            assert _same(y1[0], y[k, :nk]) and _same(s1[0], s[k, :nk]), (rep, k)
            assert lim1[0] == lim[k] and red1.tobytes() == red[k:k + 1].tobytes()


# ---- 4. batch level --------------------------------------------------------------------------------------------------------------------------
def _clicky_wav(a, e, seed=5):
    """model-rate rows: a quiet tone between a lead and a tail of floor noise, plus a few clicks, so that the capped gain of section 11
    binds (the tone ends far under the target); quiet noise behind the span"""
    B, L, W = e.batch_dims()
    sr = a.sample_rate
    rng = np.random.default_rng(seed)
    wav = (1e-5 * rng.standard_normal((B, W))).astype(np.float32)
    for b in range(B):
        nb = min(W, int(np.float32(DURS[b] / np.float32(1.05)) * np.float32(sr)))
        lead, tail = int(0.03 * sr), int(0.04 * sr)
        t = np.arange(nb) / sr
        tone = 0.02 * (0.7 + 0.3 * np.sin(2 * np.pi * 3.0 * t + b)) * np.sin(2 * np.pi * (200.0 + 30.0 * b) * t)
        wav[b, lead:nb - tail] += tone[lead:nb - tail].astype(np.float32)
        for p in rng.integers(lead + 100, nb - tail - 100, 5):
            wav[b, p] = (0.3 + 0.1 * b) * (1 if p % 2 else -1)
        wav[b, lead + 2048] = 0.5  # (a tile boundary at the native rate)
        wav[b, lead + 2049] = -0.45
    return wav


def _engine(seed=9):
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 6, 14, [14, 9, 5, 12, 7, 11], seed=2)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=DURS)
    e.batch_run(2, 1.05, seed)
    e.dbg_batch_set_wav(_clicky_wav(a, e))
    return a, e


def _spans(e, dur):
    _, _, Wo = e.batch_dims()
    return np.array([max(0, min(Wo, int(np.float32(d) * np.float32(e.output_rate)))) for d in dur], np.int64)


def _source(e):
    """the rows at the current rate with loudness off (the limiter is then inert), their spans"""
    e.set_loudness(None)
    x, dur = e.batch_fetch()
    e.set_loudness(TARGET, CEIL)
    return x, _spans(e, dur)


@pytest.mark.parametrize("rate", [None, 16000, 88200, 192000])
def test_batch_fetch_equals_the_reference_on_the_source_rows(rate):
    _batch_fetch_case(rate, MS)


def test_batch_fetch_at_192_khz_and_the_longest_look_ahead():
    """the engine's own path to A = 1920 (LM_MAX_A): 10 ms at 192 kHz"""
    _batch_fetch_case(192000, 10.0)


def _batch_fetch_case(rate, ms):
    a, e = _engine()
    e.set_output_rate(rate)
    hz = e.output_rate
    x, n = _source(e)
    off = e.batch_fetch()[0]  # today's fetch: the gain capped
    g_cap = e.batch_loudness()[2]
    assert e.limiter is None and not e.batch_limiter()[0].any()
    e.set_limiter(ms)
    assert e.limiter == ms
    lufs, peak, g = e.batch_loudness()
    want_g = np.array([10.0 ** ((TARGET - float(l)) / 20.0) for l in lufs])
    assert np.all(np.abs(g - want_g) <= 2.0 ** -23 * want_g) and np.all(g > g_cap)  # the gain applied: uncapped (the cap bound before)
    outs = ref.limit_rows(x, n, g, CEIL, hz, ms)
    got, dur = e.batch_fetch()
    _check_rows(got, None, outs, n, hz, ms, f"batch at {hz} Hz")
    for enc in ("pcm16", "mulaw", "pcm24"):
        assert _same(e.batch_fetch_encoded(enc)[0], e.op_encode(got, enc)), enc
    for slot in (0, 1):
        e.fetch_encoded_begin(slot, "f32")
        s_got, s_dur = e.fetch_encoded_end(slot)
        assert _same(np.asarray(s_got).reshape(got.shape), got) and s_dur.tobytes() == dur.tobytes(), slot
        e.fetch_encoded_begin(slot, "pcm16")
        assert _same(np.asarray(e.fetch_encoded_end(slot)[0]).reshape(got.shape), e.op_encode(got, "pcm16")), slot
    red, lim = e.batch_limiter()
    assert lim.tolist() == [o["limited"] for o in outs] and np.all(lim > 0)
    for b, o in enumerate(outs):
        smin = 10.0 ** (-o["reduction_db"] / 20.0)
        assert abs(float(red[b]) - o["reduction_db"]) <= 20.0 / math.log(10.0) * ref.s_tol(hz, ms) / smin + 1e-6 * o["reduction_db"], (b, red[b])
        l_on = loudness_ref.integrated_loudness(got[b, : n[b]], hz)
        l_off = loudness_ref.integrated_loudness(off[b, : n[b]], hz)
        print(f"row {b}: {l_off:.2f} LUFS capped, {l_on:.2f} LUFS limited (target {TARGET}), reduction {red[b]:.2f} dB over {lim[b]} samples")
        assert abs(l_on - TARGET) < abs(l_off - TARGET), (b, l_on, l_off)
    e.close()


# ---- 5. composition --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [None, 16000, 88200, 192000])
def test_trimmed_and_joined_fetches_compose(rate):
    a, e = _engine()
    e.set_output_rate(rate)
    hz = e.output_rate
    e.set_loudness(TARGET, CEIL)
    e.set_limiter(MS)
    whole = e.batch_fetch()[0]
    # a trimmed fetch without a fade: a slice of the untrimmed limited fetch
    e.set_silence_trim((40.0, 20.0, 0.0))
    s, en = e.batch_silence_edges()
    assert np.all(en > s) and np.any(s > 0)
    trimmed = e.batch_fetch()[0]
    want = np.zeros_like(whole)
    for b in range(whole.shape[0]):
        want[b, : en[b] - s[b]] = whole[b, s[b]:en[b]]
    assert _same(trimmed, want)
    # joined, one gain per row: the host concatenation of the per-row limited fetch
    rows, gap_s = [2, 1, 3], [0.3, 0.25, 0.0]
    gap = [int(v * hz) for v in gap_s]
    lens = en - s
    p = join_ref.plan(rows, gap, gap_s, lens, (lens.astype(np.float32) / np.float32(hz)).astype(np.float32), hz)
    for enc in ("f32", "pcm16"):
        per_row = e.batch_fetch_encoded(enc)[0]
        got, plen, _ = e.batch_fetch_joined(rows, gap, gap_s, gain_scope="row", encoding=enc, cut=False)
        assert np.array_equal(plen, p["prog_len"])
        assert _same(got, join_ref.padded(join_ref.join(per_row, lens, rows, gap, 0), p["W_join"], 0)), enc
    e.set_silence_trim(None)
    # joined, one gain per programme: the reference on the joined signal, G rows with their programme gains and spans
    e.set_loudness(None)
    joined, plen, pdur = e.batch_fetch_joined(rows, gap, gap_s, cut=False)
    e.set_loudness(TARGET, CEIL)
    lufs, _, g = e.batch_join_loudness(rows, gap, gap_s)
    want_g = np.array([10.0 ** ((TARGET - float(l)) / 20.0) for l in lufs])
    assert np.all(np.abs(g - want_g) <= 2.0 ** -23 * want_g)
    ng = np.array([max(0, min(int(plen[k]), int(np.float32(pdur[k]) * np.float32(hz)))) for k in range(len(rows))], np.int64)
    outs = ref.limit_rows(joined, ng, g, CEIL, hz, MS)
    assert all(o["limited"] > 0 for o in outs)
    got, _, _ = e.batch_fetch_joined(rows, gap, gap_s, gain_scope="programme", cut=False)
    _check_rows(got, None, outs, ng, hz, MS, f"programmes at {hz} Hz")
    assert _same(e.batch_fetch_joined(rows, gap, gap_s, gain_scope="programme", encoding="mulaw", cut=False)[0], e.op_encode(got, "mulaw"))
    e.close()


# ---- 6. inert when off -----------------------------------------------------------------------------------------------------------------------
def _launches(e, fetch):
    e.profile_enable(True)
    e.launch_log_enable(True)
    fetch()
    log = e.launch_log()
    e.launch_log_enable(False)
    e.profile_enable(False)
    return log


def test_off_is_the_path_without_it_and_toggling_touches_no_graph():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 6, 14, [14, 9, 5, 12, 7, 11], seed=2)

    def make():
        x = binding.Engine(0, "bf16")
        x.load_synthetic(a, 7)
        x.set_vocoder_mode(1)
        x.batch_upload(ids, mask, sttl, sdp, duration_override=DURS)
        for _ in range(3):  # the second sighting captures the shape, the third replays it
            x.batch_run(2, 1.05, 4)
        return x

    e, fresh = make(), make()
    cached, replays = e.graphs_cached, e.graph_replays
    assert cached >= 1 and replays >= 1 and e.limiter is None
    e.set_loudness(-20.0)
    for ms in (5.0, 0.5):  # toggling and re-targeting, with fetches in between
        e.set_limiter(ms)
        fams = [f for f, _ in _launches(e, lambda: e.batch_fetch_encoded("mulaw"))]
        assert "out.limiter" in fams and fams[-1] == "out.loudness_gain"
        e.batch_fetch_joined([6], 100, 0.1, gain_scope="programme")
    e.set_limiter(None)
    e.set_loudness(None)
    assert e.graphs_cached == cached and e.graph_replays == replays
    j = ([2, 4], [100, 7], 0.3)
    for limiter, rate, lo in ((None, None, None), (None, 16000, -20.0), (5.0, None, None), (5.0, 16000, None)):
        e.set_limiter(limiter)  # (on with loudness off: no effect, no launch)
        for x in (e, fresh):
            x.set_output_rate(rate)
            x.set_loudness(lo)
        for enc in ("f32", "pcm16", "mulaw"):
            assert _same(e.batch_fetch_encoded(enc)[0], fresh.batch_fetch_encoded(enc)[0]), (limiter, rate, lo, enc)
            assert _launches(e, lambda: e.batch_fetch_encoded(enc)) == _launches(fresh, lambda: fresh.batch_fetch_encoded(enc))
        for slot in (0, 1):
            e.fetch_encoded_begin(slot, "pcm16")
            fresh.fetch_encoded_begin(slot, "pcm16")
            assert _same(e.fetch_encoded_end(slot)[0], fresh.fetch_encoded_end(slot)[0])
        for scope in ("row", "programme"):
            assert _same(e.batch_fetch_joined(*j, gain_scope=scope, cut=False)[0], fresh.batch_fetch_joined(*j, gain_scope=scope, cut=False)[0])
            assert _launches(e, lambda: e.batch_fetch_joined(*j, gain_scope=scope)) == _launches(fresh, lambda: fresh.batch_fetch_joined(*j, gain_scope=scope))
        assert e.batch_loudness()[2].tobytes() == fresh.batch_loudness()[2].tobytes()
    assert e.graphs_cached == cached and e.graph_replays == replays
    e.batch_run(2, 1.05, 4)
    assert e.graphs_cached == cached and e.graph_replays == replays + 1  # the next run is a replay
    e.close()
    fresh.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_error_codes_with_messages(eng):
    e = binding.Engine(0, "bf16")
    e.load_synthetic(tiny_arch(), 7)
    e.set_limiter(2.0)
    for bad in (0.49, 10.5, float("nan"), -1.0):
        assert e._lib.stn_set_limiter(e._h, 1, bad) == -1 and "must be in [0.5, 10]" in e.last_error()
    assert e.limiter == 2.0  # the previous setting stayed in force
    with pytest.raises(binding.StnError) as ei:
        e.batch_limiter()
    assert "no finished batch" in str(ei.value)
    e.close()
    x = np.zeros((1, 64), np.float32)
    y = np.zeros_like(x)
    assert eng._lib.stn_op_limiter(eng._h, 16000, 0, 64, x, None, None, CEIL, MS, y.ctypes.data, None, None, None) == -1
    assert "rows" in eng.last_error()
    assert eng._lib.stn_op_limiter(eng._h, 16000, 65536, 64, x, None, None, CEIL, MS, y.ctypes.data, None, None, None) == -1
    for kw in (dict(lookahead_ms=0.4), dict(lookahead_ms=11.0), dict(ceiling_dbfs=1.0), dict(ceiling_dbfs=-31.0)):
        with pytest.raises(binding.StnError) as ei:
            eng.op_limiter(x, 16000, None, None, **kw)
        assert ei.value.code == -1 and "must be in" in str(ei.value)
    with pytest.raises(binding.StnError):
        eng.op_limiter(x, 7000)
    with pytest.raises(binding.StnError):
        eng.op_limiter(x, 16000, [65])


# ---- 8. cost ---------------------------------------------------------------------------------------------------------------------------------
def test_timing_report_c3_limiter():
    """Event-timed cost of the PCM16 fetch of a C3-sized batch (128 rows) at the native rate, over 10 fetches after a warm one, in three
    states in one process: loudness alone (the fetch as it was), the limiter on with no row over the ceiling, and the limiter on with
    every row carrying clicks.  Printed, not asserted; DESIGN.md section 15 records the values."""
    from supertonic_amd import host, workload
    from supertonic_amd.arch import default_arch
    a = default_arch()
    texts = workload.utterances(128, min_words=3, max_words=12, seed=11)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * 128)
    sttl, sdp = workload.synthetic_styles(a, list(range(128)))
    durs = workload.forced_durations(texts)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(5, 1.05, 1)
    B, _, W = e.batch_dims()

    def timed(what):
        e.batch_fetch_pcm16()  # warm: scratch, tables
        e.profile_enable(True)
        e.profile_reset()
        for _ in range(10):
            e.batch_fetch_pcm16()
        prof = e.profile()
        e.profile_enable(False)
        per = {k: v["ms"] * 1e3 / 10 for k, v in prof.items() if k.startswith("out.")}
        print(f"\nC3 batch, pcm16, {B} x {W} samples, {what}: " + ", ".join(f"{k} {v:.1f} us" for k, v in sorted(per.items()))
              + f"; total {sum(per.values()):.1f} us per fetch")
        return {k: v["launches"] for k, v in prof.items()}

    wav = e.batch_fetch()[0]
    wav = (wav * np.float32(0.05 / max(float(np.abs(wav).max()), 1e-9))).astype(np.float32)  # peaks at 0.05: a 20 dB crest is out of reach
    e.dbg_batch_set_wav(wav)
    e.set_loudness(-30.0, CEIL)
    launches = timed("loudness alone")
    assert "out.limiter" not in launches
    e.set_limiter(MS)
    assert not e.batch_limiter()[1].any()
    launches = timed("limiter on, no row over the ceiling")
    assert launches.get("out.limiter") == 10 and launches.get("out.limiter_rows") == 10
    wav[:, 3000::23000] = 0.9
    e.dbg_batch_set_wav(wav)
    red, lim = e.batch_limiter()
    launches = timed(f"limiter on, every row with clicks ({int(lim.min())} to {int(lim.max())} samples a row turned down)")
    assert launches.get("out.limiter") == 10 and launches.get("out.limiter_rows") == 10 and np.all(lim > 0)
    e.close()
