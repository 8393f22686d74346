"""The true-peak mode through the output stage on an MI355X (include/stn.h "true peak"): known rows put into the
tiny synthetic engine's finished batch (stn_dbg_batch_set_wav), fetched at the native rate and at 16 kHz, against
tests/truepeak_ref.py.  In sample mode the delivered true peak overshoots the ceiling; in true mode it does not."""
import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
import join_ref
import limiter_ref
import truepeak_ref as R

pytestmark = pytest.mark.gpu
DURS = np.array([0.71, 0.43, 0.92, 0.64, 0.51, 0.47], np.float32)
TARGET, CEIL, MS = -12.0, -1.0, 5.0
C = float(limiter_ref.ceiling(CEIL))
# the delivered true peak against c: the fp32 gain, the per-sample product rounding and the device's tol_u at sum |h| <= 1.95
TP_BOUND = C * (1.0 + 64.0 * 2.0 ** -24)
QUIET, TONE, CLICKY = (0, 3), (1, 4), (2, 5)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _wav(a, e, hz_out):
    """model-rate rows.  Quiet: a low tone (the loudness gain leaves it under the ceiling).  Tone: hz_out / 4 at 45 degrees to the
    output rate's sample instants (sample peak 0.707 of the true peak) in 6 ms bursts every 150 ms, a speech-like envelope whose
    loudness is far under its peaks.  Clicky: limiter_ref.peaky_row.  Quiet noise behind the span."""
    B, L, W = e.batch_dims()
    sr = a.sample_rate
    rng = np.random.default_rng(5)
    wav = (1e-5 * rng.standard_normal((B, W))).astype(np.float32)
    t = np.arange(W) / sr
    for b in range(B):
        nb = min(W, int(np.float32(DURS[b] / np.float32(1.05)) * np.float32(sr)))
        if b in QUIET:
            wav[b, :nb] += (0.02 * np.sin(2 * np.pi * (200.0 + 30.0 * b) * t[:nb])).astype(np.float32)
        elif b in TONE:
            envl = 0.004 + 0.3 * np.exp(-0.5 * (((t % 0.15) - 0.05) / 0.003) ** 2)
            wav[b, :nb] += (envl * np.sin(2 * np.pi * (hz_out / 4.0) * t + np.pi / 4))[:nb].astype(np.float32)
        else:
            wav[b] = limiter_ref.peaky_row(W, nb, 1.0, 0.1, limiter_ref.samples(sr, MS), 40 + b)
    return wav


def _engine(rate):
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 6, 14, [14, 9, 5, 12, 7, 11], seed=2)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=DURS)
    e.batch_run(2, 1.05, 9)
    e.dbg_batch_set_wav(_wav(a, e, rate or a.sample_rate))  # (at the model's rate: before the output rate is set)
    e.set_output_rate(rate)
    return a, e


def _spans(e, dur):
    _, _, Wo = e.batch_dims()
    return np.array([max(0, min(Wo, int(np.float32(d) * np.float32(e.output_rate)))) for d in dur], np.int64)


def _source(e):
    e.set_loudness(None)
    x, dur = e.batch_fetch()
    e.set_loudness(TARGET, CEIL)
    return x, _spans(e, dur)


def _tps(y, n):
    return np.array([R.true_peak(y[b], n[b]) for b in range(y.shape[0])])


@pytest.mark.parametrize("rate", [None, 16000])
def test_sample_mode_overshoots_and_true_mode_holds_the_ceiling(rate):
    a, e = _engine(rate)
    hz = e.output_rate
    x, n = _source(e)
    assert e.peak_mode == "sample"
    # sample mode: the gap
    y = e.batch_fetch()[0]
    tps = _tps(y, n)
    for b in TONE:
        over = 20 * np.log10(tps[b] / C)
        print(f"{hz} Hz, sample mode, row {b}: sample peak {np.abs(y[b, :n[b]]).max():.4f}, true peak {tps[b]:.4f} ({over:+.2f} dB against the ceiling)")
        assert np.abs(y[b, : n[b]]).max() <= C and over > 1.0
    tp_in, tp_out, trim = e.batch_true_peak()  # works in any mode
    assert np.all(trim == 1.0)
    assert np.all(np.abs(tp_out - tps) <= 18 * 2.0 ** -24 * 1.95 * tps + 2.0 ** -24 * tps)  # tol_u at sum |h| <= 1.95 and |x| <= tp
    lufs_s, peak_s, g_s = e.batch_loudness()
    # true mode, loudness only
    e.set_peak_mode("true")
    assert e.peak_mode == "true"
    lufs, peak, g = e.batch_loudness()
    tp_in, tp_out, trim = e.batch_true_peak()
    assert peak.tobytes() == tp_in.tobytes() and lufs.tobytes() == lufs_s.tobytes() and np.all(trim == 1.0)
    src_tp = _tps(x, n)
    assert np.all(np.abs(tp_in - src_tp) <= 18 * 2.0 ** -24 * 1.95 * src_tp + 2.0 ** -24 * src_tp)
    want_g = np.array([min(10.0 ** ((TARGET - float(l)) / 20.0), 10.0 ** (float(np.float32(CEIL)) / 20.0) / float(p)) for l, p in zip(lufs, peak)])
    assert np.all(np.abs(g - want_g) <= 2e-7 * want_g), (g, want_g)
    assert all(g[b] < g_s[b] for b in TONE) and all(g[b] == g_s[b] for b in QUIET)
    y = e.batch_fetch()[0]
    assert _same(y, (x * g[:, None]).astype(np.float32))
    tps = _tps(y, n)
    print(f"{hz} Hz, true mode, loudness only: delivered true peaks {np.round(tps, 5).tolist()} (ceiling {C:.5f})")
    assert np.all(tps <= TP_BOUND)
    assert np.all(tp_out <= TP_BOUND)
    for enc in ("pcm16", "mulaw"):
        assert _same(e.batch_fetch_encoded(enc)[0], e.op_encode(y, enc)), enc
    # true mode with the limiter
    e.set_limiter(MS)
    lufs, _, g = e.batch_loudness()
    want_g = np.array([10.0 ** ((TARGET - float(l)) / 20.0) for l in lufs])
    assert np.all(np.abs(g - want_g) <= 2.0 ** -23 * want_g)
    tp_in, tp_out, trim = e.batch_true_peak()
    y = e.batch_fetch()[0]
    tps = _tps(y, n)
    print(f"{hz} Hz, true mode, limiter: trims {trim.tolist()}, delivered true peaks {np.round(tps, 5).tolist()}")
    assert np.all(trim <= 1.0) and np.all(trim > 0.0)  # (reported, not bounded)
    assert np.all(np.abs(y) <= np.float32(C))
    assert np.all(tps <= TP_BOUND) and np.all(tp_out <= TP_BOUND)
    red, lim = e.batch_limiter()
    assert all(lim[b] > 0 for b in TONE + CLICKY)
    op = e.op_limiter_ex(x, hz, n, g, CEIL, MS, "true")
    assert op["trim"].tobytes() == trim.tobytes()
    assert _same(y, (op["y"] * trim[:, None]).astype(np.float32))
    A = limiter_ref.samples(hz, MS)
    for b in range(x.shape[0]):
        assert R.env_violations(op["env"][b], x[b], n[b], g[b]).size == 0, b
        # the curve from the device's own envelope (the reference's differs from it by tol_u, which c / e magnifies by no more than 1)
        o = R.limit_row_env(x[b], n[b], g[b], CEIL, hz, MS, env=op["env"][b])
        assert np.array_equal(np.asarray(op["s"][b] < 1.0), o["s"] < 1.0), b
        tol_s = limiter_ref.s_tol(hz, MS)
        assert np.all(np.abs(op["s"][b].astype(np.float64) - o["s"]) <= tol_s), b
        tol_y = np.abs(o["v"].astype(np.float64)) * (tol_s + 2.0 ** -23)  # (the bound of tests/test_gpu_limiter.py)
        assert np.all(np.abs(op["y"][b].astype(np.float64) - o["y"]) <= tol_y), b
        tol_d = tol_y * float(trim[b]) + np.abs(o["y"]) * float(trim[b]) * 2.0 ** -24
        assert np.all(np.abs(y[b].astype(np.float64) - o["y"] * float(trim[b])) <= tol_d), b
    # a row with g * tp <= c: byte for byte the loudness-only true-mode fetch
    e.set_limiter(None)
    lo_only = e.batch_fetch()[0]
    g_lo = e.batch_loudness()[2]
    for b in QUIET:
        assert g_lo[b] == g[b] and lim[b] == 0 and trim[b] == 1.0 and _same(y[b], lo_only[b]), b
    e.close()


@pytest.mark.parametrize("rate", [None, 16000, 88200, 192000])
def test_encodings_trimmed_and_joined_fetches_compose(rate):
    a, e = _engine(rate)
    hz = e.output_rate
    e.set_loudness(TARGET, CEIL)
    e.set_peak_mode("true")
    e.set_limiter(MS)
    whole = e.batch_fetch()[0]
    for enc in ("pcm16", "mulaw"):
        assert _same(e.batch_fetch_encoded(enc)[0], e.op_encode(whole, enc)), enc
    for slot in (0, 1):
        e.fetch_encoded_begin(slot, "pcm16")
        assert _same(np.asarray(e.fetch_encoded_end(slot)[0]).reshape(whole.shape), e.op_encode(whole, "pcm16")), slot
    # trimmed without a fade: a slice of the untrimmed fetch
    e.set_silence_trim((40.0, 20.0, 0.0))
    s, en = e.batch_silence_edges()
    trimmed = e.batch_fetch()[0]
    want = np.zeros_like(whole)
    for b in range(whole.shape[0]):
        want[b, : en[b] - s[b]] = whole[b, s[b]:en[b]]
    assert _same(trimmed, want)
    assert _same(e.batch_fetch_encoded("mulaw")[0], e.op_encode(trimmed, "mulaw"))
    # joined, one gain per row: the host concatenation of the per-row fetch
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
    # joined, one gain per programme: the op on the joined signal, G rows with their programme gains and spans
    e.set_loudness(None)
    joined, plen, pdur = e.batch_fetch_joined(rows, gap, gap_s, cut=False)
    e.set_loudness(TARGET, CEIL)
    _, _, g = e.batch_join_loudness(rows, gap, gap_s)
    ng = np.array([max(0, min(int(plen[k]), int(np.float32(pdur[k]) * np.float32(hz)))) for k in range(len(rows))], np.int64)
    op = e.op_limiter_ex(joined, hz, ng, g, CEIL, MS, "true")
    got, _, _ = e.batch_fetch_joined(rows, gap, gap_s, gain_scope="programme", cut=False)
    assert _same(got, (op["y"] * op["trim"][:, None]).astype(np.float32))
    assert np.all(_tps(got, ng) <= TP_BOUND) and np.all(np.abs(got) <= np.float32(C))
    assert _same(e.batch_fetch_joined(rows, gap, gap_s, gain_scope="programme", encoding="mulaw", cut=False)[0], e.op_encode(got, "mulaw"))
    # loudness only, per programme: the gate's peak is the joined row's true peak
    e.set_limiter(None)
    lufs, peak, g = e.batch_join_loudness(rows, gap, gap_s)
    want_tp = _tps(joined, ng)
    assert np.all(np.abs(peak - want_tp) <= 18 * 2.0 ** -24 * 1.95 * want_tp + 2.0 ** -24 * want_tp)
    got, _, _ = e.batch_fetch_joined(rows, gap, gap_s, gain_scope="programme", cut=False)
    assert _same(got, (joined * g[:, None]).astype(np.float32)) and np.all(_tps(got, ng) <= TP_BOUND)
    e.close()


def _launches(e, fetch):
    e.profile_enable(True)
    e.launch_log_enable(True)
    fetch()
    log = e.launch_log()
    e.launch_log_enable(False)
    e.profile_enable(False)
    return log


def test_sample_mode_is_the_path_without_it_and_toggling_touches_no_graph():
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
    assert cached >= 1 and replays >= 1 and e.peak_mode == "sample"
    e.set_loudness(-20.0)
    e.set_peak_mode("true")
    fams = [f for f, _ in _launches(e, lambda: e.batch_fetch_encoded("mulaw"))]
    assert fams.count("out.true_peak") == 1 and fams.count("out.loudness") == 4 and fams[-1] == "out.loudness_gain"  # five launches instead of four
    e.set_limiter(5.0)
    fams = [f for f, _ in _launches(e, lambda: e.batch_fetch_encoded("mulaw"))]
    assert fams.count("out.true_peak") == 2 and fams.count("out.true_peak_rows") == 1 and "out.limiter" in fams and fams[-1] == "out.loudness_gain"
    e.batch_fetch_joined([6], 100, 0.1, gain_scope="programme")
    e.batch_true_peak()
    e.set_limiter(None)
    e.set_loudness(None)
    e.set_peak_mode("sample")
    assert e.graphs_cached == cached and e.graph_replays == replays
    j = ([2, 4], [100, 7], 0.3)
    for mode, rate, lo, limiter in (("sample", None, None, None), ("sample", 16000, -20.0, None), ("sample", None, -20.0, 5.0),
                                    ("true", None, None, None), ("true", 16000, None, 5.0)):  # (true with loudness off: no effect, no launch)
        e.set_peak_mode(mode)
        for x in (e, fresh):
            x.set_output_rate(rate)
            x.set_loudness(lo)
            x.set_limiter(limiter)
        for enc in ("f32", "pcm16", "mulaw"):
            assert _same(e.batch_fetch_encoded(enc)[0], fresh.batch_fetch_encoded(enc)[0]), (mode, rate, lo, enc)
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


def test_op_level_calls_keep_the_sample_peak_on_a_true_mode_handle():
    """stn_op_join, stn_op_loudness_ex and stn_op_limiter depend on their arguments alone: a handle in true mode with loudness (and the
    limiter) on answers byte for byte what a fresh handle answers"""
    a = tiny_arch()
    e, fresh = binding.Engine(0, "bf16"), binding.Engine(0, "bf16")
    for x in (e, fresh):
        x.load_synthetic(a, 7)
    e.set_loudness(TARGET, CEIL)
    e.set_peak_mode("true")
    W = 9000
    x = np.stack([R.tone45(W, 0.4), R.tone45(W, 0.2), (0.1 * np.sin(np.arange(W) / 9.0)).astype(np.float32)])
    n = np.array([9000, 8500, 7000], np.int64)
    for limiter in (None, MS):
        e.set_limiter(limiter)
        for enc in ("f32", "pcm16"):
            got = e.op_join(x, n, [2, 1], [100, 0], 16000, encoding=enc, loudness=(0.0, CEIL))
            want = fresh.op_join(x, n, [2, 1], [100, 0], 16000, encoding=enc, loudness=(0.0, CEIL))
            assert all(_same(g, w) for g, w in zip(got, want)), (limiter, enc)
        # (the tone's programme: the sample-peak contract leaves its true peak over the ceiling, which a true-peak cap would not)
        assert R.true_peak(e.op_join(x, n, [2, 1], [100, 0], 16000, loudness=(0.0, CEIL))[0][0]) > C
        a_, b_ = e.op_loudness_ex(x, 16000, n, on=True, target_lufs=0.0), fresh.op_loudness_ex(x, 16000, n, on=True, target_lufs=0.0)
        assert all(_same(a_[k], b_[k]) for k in ("pk", "lufs", "peak", "gain"))
        assert all(_same(p, q) for p, q in zip(e.op_limiter(x, 16000, n, [2.0, 3.0, 1.0]), fresh.op_limiter(x, 16000, n, [2.0, 3.0, 1.0])))
    e.close()
    fresh.close()


def test_refusals_are_error_codes_with_messages():
    e = binding.Engine(0, "bf16")
    e.load_synthetic(tiny_arch(), 7)
    e.set_peak_mode("true")
    for bad in (2, -1, 7):
        assert e._lib.stn_set_peak_mode(e._h, bad) == -1 and "STN_PEAK_SAMPLE" in e.last_error()
    assert e.peak_mode == "true" and e._lib.stn_get_peak_mode(e._h) == 1  # the previous setting stayed in force
    assert e._lib.stn_get_peak_mode(None) == -1 and e._lib.stn_set_peak_mode(None, 0) == -1
    with pytest.raises(ValueError):
        e.set_peak_mode("peak")
    with pytest.raises(binding.StnError) as ei:
        e.batch_true_peak()
    assert "no finished batch" in str(ei.value)
    x = np.zeros((1, 64), np.float32)
    with pytest.raises(binding.StnError) as ei:
        e.op_limiter_ex(x, 16000, peak_mode=2)
    assert ei.value.code == -1 and "peak mode" in str(ei.value)
    y = np.zeros_like(x)
    assert e._lib.stn_op_limiter_ex(e._h, 16000, 0, 64, x, None, None, CEIL, MS, y.ctypes.data, None, None, None, 1, None, None) == -1
    assert "rows" in e.last_error()
    o = e.op_limiter_ex(x, 16000, peak_mode="sample")  # sample mode: stn_op_limiter, trim 1
    assert np.all(o["trim"] == 1.0) and not o["y"].any()
    e.close()


def test_timing_report_c3_truepeak():
    """Event-timed cost of the PCM16 fetch of a C3-sized batch (128 rows) at the native rate, over 10 fetches after a warm one, in three
    states in one process: sample mode with loudness, true mode with loudness, true mode with the limiter.  Printed, not asserted;
    DESIGN.md section 16 records the values."""
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

    e.set_loudness(-23.0, CEIL)
    timed("sample mode, loudness")
    e.set_peak_mode("true")
    timed("true mode, loudness")
    e.set_limiter(MS)
    timed("true mode, limiter")
    e.close()
