"""The fetch-time expander on an MI355X at the level of the fetches (include/stn.h "expander"; Engine::out_source, engine_batch.cpp;
DESIGN.md section 25), on synthetic weights and the batch of six rows the other fetch tests use, bf16 and f16: every fetch path delivers
stn_op_expander of the fp32 fetch with the expander off, bit for bit (with the de-esser and the compressor behind it: their ops of
that), with the resampler, the filter chain, the de-esser and the compressor on and off; the encodings, the edges, the loudness, the
limiter, the de-esser's and the compressor's reports and the joins see the expanded rows; stn_batch_expander reports the reference's
minimum and count; results cached at fetch time are keyed on the setting; off is the path without the feature; the group, the Python
host, the CLI and the service carry the setting.

The rows ("gated"): a 300 Hz tone whose amplitude alternates between 0.3 (80 ms) and 0.006 (160 ms, 34 dB lower: -44 dBFS) behind 30 ms
of digital silence; the last 100 ms of every row's span are quiet.  MID (threshold -40 dBFS, 4:1, hard knee) turns the quiet stretches
down by 13 dB; GATE20 (20:1, range 60 dB) shuts them; the speech default (threshold -50 dBFS) leaves them alone and only shuts the
leading silence.

The edges tests trim at 40 dB under the loudest frame.  Unexpanded (and under the speech default), the quiet tail lies 34 dB under the
loud stretches (25 dB with the compressor on): no silence, the end edge is the span's end.  Behind GATE20 the tail is shut 70 ms in:
silence, and the end edge lies in front of the span's end."""
import ctypes
import itertools
import json
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
import expander_ref as xr
import g711_ref
import join_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
ENCS = ["f32", "pcm16", "pcm24", "mulaw", "alaw"]
ZERO = {e: binding.ZERO_CODEWORD[binding.ENCODINGS[e]] for e in ENCS}
DURS = np.array([0.71, 0.43, 0.92, 0.64, 0.51, 0.47], np.float32)
SPEECH = binding.EXPANDER_SPEECH
MID = (-40.0, 4.0, 0.0, 30.0, 1.0, 10.0, 40.0)
GATE20 = (-40.0, 20.0, 0.0, 60.0, 0.5, 20.0, 50.0)
DEESS = binding.DEESSER_SPEECH
COMP = binding.COMPRESSOR_SPEECH
HP = (("highpass", 80.0, 0.7071, 0.0),)
TRIM = (40.0, 20.0, 0.0)
FAMILIES = ["out.expander_chunks1", "out.expander_scan1", "out.expander_chunks2", "out.expander_scan2", "out.expander_write", "out.expander_rows"]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _tiny_batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 6, 14, [14, 9, 5, 12, 7, 11], seed=2)
    return a, ids, mask, sttl, sdp, DURS


def _spans(e, dur):
    _, _, Wo = e.batch_dims()
    return np.array([max(0, min(Wo, int(np.float32(d) * np.float32(e.output_rate)))) for d in dur], np.int64)


def _gated_wav(a, e):
    B, _, W = e.batch_dims()
    sr = a.sample_rate
    t = np.arange(W) / sr
    wav = np.zeros((B, W), np.float32)
    for b in range(B):
        amp = np.where((t * 1000.0 + 11.0 * b) % 240.0 < 80.0, 0.3, 0.006) * (t >= 0.03)
        nb = min(W, int(np.float32(DURS[b] / np.float32(1.05)) * np.float32(sr)))
        amp[max(0, nb - int(0.1 * sr)):] = 0.006  # (the last 100 ms of the span: quiet)
        wav[b] = amp * np.sin(2 * np.pi * (300.0 + 20.0 * b) * t)
    return wav


def _engine(dtype, seed=9):
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    e = binding.Engine(0, dtype)
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, seed)
    e.dbg_batch_set_wav(_gated_wav(a, e))
    return a, e


def _f32(setting):
    return tuple(np.float32(v) for v in setting)


def _behind(e, x, hz, deess, comp):
    """what the stages behind the expander make of the rows x: their own ops, in the stage's order"""
    if deess:
        x = e.op_deesser(x, hz, deess)
    if comp:
        x = e.op_compressor(x, hz, comp)
    return x


# ---- 1. identity: every fetch path delivers the expanded rows -------------------------------------------------------------------------------
COMBOS = [(None, None, None, None), (16000, HP, DEESS, COMP), (None, HP, None, COMP), (16000, None, DEESS, None)]  # every stage on and off


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_fetch_path_delivers_op_expander_of_the_fetch_without_it(dtype):
    from hip_util import DeviceBuffer
    a, e = _engine(dtype)
    assert e.get_expander() is None and e.expander is None
    exact = 0
    for i, (rate, chain, deess, comp) in enumerate(COMBOS):
        setting = (MID, GATE20)[i % 2]
        e.set_output_rate(rate)
        e.set_filters(chain)
        e.set_deesser(None)
        e.set_compressor(None)
        e.set_expander(None)
        att, closed = e.batch_expander()
        assert not att.any() and not closed.any() and closed.dtype == np.int64
        plain, dur = e.batch_fetch()
        hz = e.output_rate
        xp = e.op_expander(plain, hz, setting)
        # it only ever turns down: a gain of at most 1, within the power of ten's 2 ulp and the product's rounding, and within the few
        # fp32 spacings of R by which a start value the linear scan formed (E s + c, c rounded to fp32) may leave yL above R
        top = (1 + 3 * 2.0 ** -23) * 10.0 ** (4 * float(np.spacing(np.float32(setting[3]))) / 20.0)
        assert np.abs(xp - plain).max() > 0.001 and np.abs(xp).max() > 0.25 and np.all(np.abs(xp) <= np.abs(plain) * top)
        want = _behind(e, xp, hz, deess, comp)
        e.set_deesser(deess)
        e.set_compressor(comp)
        off, _ = e.batch_fetch()
        assert _same(off, _behind(e, plain, hz, deess, comp))  # (the stages behind it alone: their own identities)
        e.set_expander(setting)
        assert e.get_expander() == _f32(setting) == e.expander
        got, gdur = e.batch_fetch()
        assert _same(got, want) and gdur.tobytes() == dur.tobytes(), (dtype, rate, chain, deess, comp, setting)
        if not deess and not comp:
            assert _same(got, e.op_expander(off, hz, setting))  # the identity as the header states it
        B, _, Wo = e.batch_dims()
        for enc in ENCS:
            enc_want = want if enc == "f32" else e.op_encode(want, enc)
            assert _same(e.batch_fetch_encoded(enc)[0], enc_want), (dtype, rate, chain, enc)
            for slot in (0, 1):
                e.fetch_encoded_begin(slot, enc)
                assert _same(np.asarray(e.fetch_encoded_end(slot)[0]).reshape(enc_want.shape), enc_want), (dtype, rate, chain, enc, slot)
            for stride in (Wo + 32 - Wo % 16, Wo + 3 - Wo % 2):  # wide and aligned; odd
                like = binding.encoded_empty(enc, B, stride)
                like[...] = 0x5A if like.dtype == np.uint8 else -7
                d = DeviceBuffer(like)
                e.batch_copy_encoded_device(enc, d.ptr, stride)
                e.sync()
                back = d.to_host()
                assert _same(np.ascontiguousarray(back[:, :Wo]), enc_want) and np.all(back[:, Wo:] == like[:, Wo:]), (enc, stride)
        for enc in ENCS:  # the encodings against the host rules on the delivered fp32 rows
            assert _same(e.batch_fetch_encoded(enc)[0], g711_ref.encode(binding.ENCODINGS[enc], want)), (dtype, rate, enc)
        assert _same(e.batch_fetch_pcm16()[0], g711_ref.pcm16(want))
        # the report: the float64 reference's minimum of R - yL over the rows' valid samples within 4 x the float32 restatement's
        # deviation in yL, and its count of yL <= R / 2, exact where no sample of the reference lies within that bound of R / 2
        f = xr.coefs(setting, hz)
        r64, r32 = xr.Ref(plain, f, np.float64), xr.Ref(plain, f, np.float32)
        bound = 4 * np.abs(r32.yl - r64.yl).max()
        n = _spans(e, dur)
        ref_att, ref_closed = r64.report(f, n)
        R = float(f["R"])
        near = np.array([int((np.abs(r64.yl[b, : n[b]] - R / 2) <= bound).sum()) for b in range(B)])
        att, closed = e.batch_expander()
        assert bound > 0 and np.abs(att - ref_att).max() <= bound, (dtype, rate, chain, setting, att, ref_att, bound)
        assert np.all(np.abs(closed - ref_closed) <= near) and ref_closed.min() > 0.02 * hz and np.all(ref_closed < n), (closed, ref_closed, near)
        exact += int((near == 0).sum())
        assert ref_att.max() < 0.01  # (the loud stretches open the gate)
        # the de-esser's and the compressor's reports are those of the expanded rows
        if deess:
            assert _same(e.batch_deesser(), _report(e, "deesser", xp, hz, deess, n))
        if comp:
            assert _same(e.batch_compressor(), _report(e, "compressor", _behind(e, xp, hz, deess, None), hz, comp, n))
        # the batch's own waveform is untouched
        e.set_expander(None)
        assert _same(e.batch_fetch()[0], off)
    assert exact > 0  # (the exact comparison of the count did happen)
    e.close()


def _report(e, which, x, hz, setting, n):
    """the row maxima of yL over the valid samples, from the op's own probe on the rows x"""
    o = e.op_deesser_ex(x, hz, setting) if which == "deesser" else e.op_compressor_ex(x, hz, setting)
    return np.array([o["gr_db"][b, : n[b]].max() if n[b] else 0.0 for b in range(len(n))], np.float32)


# ---- 2. order: everything behind the expander sees the expanded rows --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_the_level_based_steps_run_on_the_expanded_rows(dtype):
    for rate, chain in ((None, None), (16000, HP)):
        a, e = _engine(dtype)
        e.set_output_rate(rate)
        e.set_filters(chain)
        hz = e.output_rate
        plain, dur = e.batch_fetch()
        n = _spans(e, dur)
        e.set_expander(GATE20)
        xg = e.batch_fetch()[0]
        assert _same(xg, e.op_expander(plain, hz, GATE20))
        e.set_silence_trim(TRIM)
        s1, e1 = e.batch_silence_edges()
        e.set_silence_trim(None)
        os_, oe = e.op_silence_edges(xg, hz, n, TRIM[0], TRIM[1])
        assert np.array_equal(s1, os_) and np.array_equal(e1, oe), (rate, s1, os_)
        ps_, pe = e.op_silence_edges(plain, hz, n, TRIM[0], TRIM[1])
        assert np.all(e1 < pe)  # (trimming's levels are those of the gated signal: the quiet tail is silence now)
        lufs, peak, _ = e.batch_loudness()
        ol, op = e.op_loudness(xg, hz, n)
        assert _same(lufs, ol) and _same(peak, op), rate
        assert _same(e.batch_true_peak()[0], e.op_true_peak(xg, hz, n)["tp"]), rate
        e.set_loudness(-6.0, -1.0)
        e.set_limiter(5.0)
        g = e.batch_loudness()[2]
        red, lim = e.batch_limiter()
        y, s, ored, olim = e.op_limiter(xg, hz, n, g, -1.0, 5.0)
        assert _same(red, ored) and np.array_equal(lim, olim) and lim.any(), rate
        lim_rows = e.batch_fetch()[0]
        assert all(_same(lim_rows[b, : n[b]], y[b, : n[b]]) for b in range(len(n))), rate
        e.close()


def _apply(e, setting, trim):
    e.set_silence_trim(trim)
    e.set_compressor(COMP)
    e.set_expander(setting)


def test_cached_edges_and_maxima_are_keyed_on_the_setting():
    """trimming and the compressor on throughout (edges and row maxima are cached per batch and setting): the expander off, on, changed,
    off again, each against a fresh handle; a cache that ignored the setting would hand the edges or maxima of other rows on"""
    a, e = _engine("bf16")
    seen = []
    for setting in (None, MID, SPEECH, MID, GATE20, None):
        _apply(e, setting, TRIM)
        _, fresh = _engine("bf16")
        _apply(fresh, setting, TRIM)
        for fetch in (lambda x: x.batch_fetch_encoded("pcm16")[0], lambda x: x.batch_fetch()[0],
                      lambda x: x.batch_fetch_joined([2, 1, 3], [100, 7, 0], [0.3, 0.1, 0.0], cut=False, encoding="pcm16")[0]):
            assert _same(fetch(e), fetch(fresh)), setting  # (the fetch first: a stale key would cut by the edges of the setting before)
        edges, fe = np.stack(e.batch_silence_edges()), np.stack(fresh.batch_silence_edges())
        assert np.array_equal(edges, fe) and _same(e.batch_compressor(), fresh.batch_compressor()), setting
        assert all(_same(p, q) for p, q in zip(e.batch_expander(), fresh.batch_expander())), setting
        seen.append((edges, e.batch_compressor()))
        fresh.close()
    assert np.array_equal(seen[0][0], seen[5][0]) and np.array_equal(seen[1][0], seen[3][0])
    assert np.all(seen[4][0][1] < seen[0][0][1])  # (the gate shuts the quiet tail: the end edges do depend on the setting, so a stale key would show)
    e.close()


# ---- 3. joined fetches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_joined_fetch_is_the_host_join_of_the_expanded_rows(dtype):
    import math
    a, e = _engine(dtype)
    rows, gap_s = [2, 1, 3], [0.3, 0.25, 0.0]
    cs = a.base_chunk_size * a.chunk_compress_factor
    # (every stage in front of and behind the expander on and off)
    for rate, chain, deess, comp, trim in ((None, None, None, None, None), (16000, HP, DEESS, COMP, None), (None, HP, None, COMP, TRIM),
                                           (16000, None, DEESS, None, TRIM)):
        e.set_deesser(None)  # (off across the change of rate: its band is checked against the rate in force)
        e.set_output_rate(rate)
        e.set_filters(chain)
        e.set_expander(MID)
        e.set_deesser(deess)
        e.set_compressor(comp)
        e.set_silence_trim(trim)
        e.set_loudness(None)
        hz = e.output_rate
        gap = [int(s * hz) for s in gap_s]
        B, _, Wo = e.batch_dims()
        dur = e.batch_fetch_encoded("pcm16")[1]
        if trim is None:  # a member's whole wave at the output rate
            g_ = math.gcd(hz, a.sample_rate)
            P, Q = hz // g_, a.sample_rate // g_
            whole = [min(Wo, -(-((int(np.float32(d) * np.float32(a.sample_rate)) + cs - 1) // cs) * cs * P // Q)) for d in dur]
            lens = np.asarray(join_ref.member_lengths(whole, dur, hz, join_ref.WHOLE))
            p = join_ref.plan(rows, gap, gap_s, whole, dur, hz, join_ref.WHOLE)
        else:
            s, en = e.batch_silence_edges()
            lens = en - s
            p = join_ref.plan(rows, gap, gap_s, lens, (lens.astype(np.float32) / np.float32(hz)).astype(np.float32), hz)
        for lo, enc in itertools.product((None, -20.0), ("f32", "pcm16", "mulaw")):
            e.set_loudness(lo)
            per_row, _ = e.batch_fetch_encoded(enc)
            want = join_ref.padded(join_ref.join(per_row, lens, rows, gap, ZERO[enc]), p["W_join"], ZERO[enc])
            got, plen, _ = e.batch_fetch_joined(rows, gap, gap_s, gain_scope="row", encoding=enc, cut=False)
            assert np.array_equal(plen, p["prog_len"]) and _same(got, want), (dtype, rate, chain, deess, comp, trim, lo, enc)
        # one gain per programme: the joined expanded fp32 signal times float32(g_g)
        e.set_loudness(None)
        joined, _, _ = e.batch_fetch_joined(rows, gap, gap_s, cut=False)
        e.set_loudness(-20.0)
        g = e.batch_join_loudness(rows, gap, gap_s)[2]
        got, _, _ = e.batch_fetch_joined(rows, gap, gap_s, gain_scope="programme", cut=False)
        assert _same(got, (joined * g[:, None]).astype(np.float32)), (dtype, rate, chain, deess, comp, trim)
    e.close()


# ---- 4. off is off ------------------------------------------------------------------------------------------------------------------------------
def _launches(e, fetch):
    e.profile_enable(True)
    e.launch_log_enable(True)
    fetch()
    log = e.launch_log()
    e.launch_log_enable(False)
    e.profile_enable(False)
    return log


def test_off_is_the_path_without_it_and_changing_the_setting_touches_no_graph():
    a, ids, mask, sttl, sdp, durs = _tiny_batch()

    def make():
        x = binding.Engine(0, "bf16")
        x.load_synthetic(a, 7)
        x.set_vocoder_mode(1)
        x.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
        for _ in range(3):  # the second sighting captures the shape, the third replays it
            x.batch_run(2, 1.05, 4)
        return x

    e, fresh = make(), make()
    cached, replays = e.graphs_cached, e.graph_replays
    assert cached >= 1 and replays >= 1 and e.get_expander() is None
    ptr = e.batch_wav_device_ptr()
    latent = e.batch_fetch_latent()
    for setting in (True, GATE20, {"threshold_db": -45, "ratio": 2}):  # three changes
        e.set_expander(setting)
        fams = [f for f, _ in _launches(e, lambda: e.batch_fetch_encoded("mulaw"))]
        assert [f for f in fams if "expander" in f] == FAMILIES, fams
        e.batch_fetch_joined([6], 100, 0.1)
        assert e.batch_wav_device_ptr() == ptr and _same(e.batch_fetch_latent(), latent)
    assert e.get_expander() == _f32((-45.0, 2.0) + SPEECH[2:])
    for i, (field, bad) in enumerate(zip(xr.FIELDS, (-5.0, 21.0, -1.0, 81.0, 301.0, 501.0, float("nan")))):
        s = list(GATE20)
        s[i] = bad
        with pytest.raises(binding.StnError) as ei:  # (through the C ABI itself: the binding's own parser would stop the NaN first)
            e._ck(e._lib.stn_set_expander(e._h, 1, ctypes.byref(binding.StnExpander(*s))))
        assert ei.value.code == -1 and field in str(ei.value), (field, str(ei.value))
    assert e.get_expander() == _f32((-45.0, 2.0) + SPEECH[2:])  # the previous setting stayed in force
    for rate in (8000, 192000, None):  # no limit depends on the rate
        e.set_output_rate(rate)
    e.set_expander(False)
    assert e.graphs_cached == cached and e.graph_replays == replays
    for rate, lo, trim in ((None, None, None), (16000, -20.0, None), (None, None, (40.0, 20.0, 5.0)), (16000, -20.0, (40.0, 20.0, 5.0))):
        for x in (e, fresh):
            x.set_output_rate(rate)
            x.set_loudness(lo)
            x.set_silence_trim(trim)
        for enc in ENCS:
            assert _same(e.batch_fetch_encoded(enc)[0], fresh.batch_fetch_encoded(enc)[0]), (rate, lo, trim, enc)
            log = _launches(e, lambda: e.batch_fetch_encoded(enc))
            assert log == _launches(fresh, lambda: fresh.batch_fetch_encoded(enc)) and "expander" not in str(log)
        for slot in (0, 1):
            e.fetch_encoded_begin(slot, "pcm16")
            fresh.fetch_encoded_begin(slot, "pcm16")
            assert _same(e.fetch_encoded_end(slot)[0], fresh.fetch_encoded_end(slot)[0])
        j = ([2, 4], [100, 7], 0.3)
        assert _same(e.batch_fetch_joined(*j, cut=False)[0], fresh.batch_fetch_joined(*j, cut=False)[0])
        assert _launches(e, lambda: e.batch_fetch_joined(*j)) == _launches(fresh, lambda: fresh.batch_fetch_joined(*j))
    e.batch_run(2, 1.05, 4)
    assert e.graphs_cached == cached and e.graph_replays == replays + 1  # the next run is a replay
    e.close()
    fresh.close()


# ---- 5. the group --------------------------------------------------------------------------------------------------------------------------------
LOW = (-20.0, 4.0, 6.0, 30.0, 1.0, 10.0, 40.0)  # (high enough a threshold for what synthetic weights produce)


def test_the_group_of_one_forwards_the_setting():
    from supertonic_amd import host, workload
    from supertonic_amd.arch import default_arch
    arch = default_arch()
    B = 4
    texts = workload.utterances(B, min_words=3, max_words=8, seed=61)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * B)
    sttl, sdp = workload.synthetic_styles(arch, list(range(B)))
    durs = workload.forced_durations(texts)
    g = binding.Group([0], "bf16")
    g.load_synthetic(arch, 7)
    g.set_expander(LOW)
    pcm, dur = g.synthesize(ids, mask, sttl, sdp, 2, 1.05, duration_override=durs, noise_seed=5)
    lengths = mask.sum(axis=(1, 2)).astype(np.int32)
    rank_of, row_of = binding.group_deal(lengths, 1)
    order = np.argsort(row_of)
    eng = binding.Engine(0, "bf16")
    eng.load_synthetic(arch, 7)
    eng.set_expander(LOW)
    eng.batch_upload(ids[order], mask[order], sttl[order], sdp[order], duration_override=durs[order], utt_ids=order.astype(np.int64))
    eng.batch_run(2, 1.05, 5)
    ref, _ = eng.batch_fetch_pcm16()
    assert np.array_equal(pcm[order][:, : ref.shape[1]], ref)
    eng.set_expander(None)
    assert not np.array_equal(eng.batch_fetch_pcm16()[0], ref)
    with pytest.raises(binding.StnError) as ei:
        g.set_expander((-50.0, 30.0, 6.0, 24.0, 1.0, 30.0, 150.0))
    assert "ratio" in str(ei.value)
    g.set_expander(None)
    g.close()
    eng.close()


# ---- 6. the hosts ---------------------------------------------------------------------------------------------------------------------------------
TEXT = "The engine gates every utterance on the device before it measures anything."
LOWD = {"threshold_db": -20.0, "ratio": 4.0, "range_db": 30.0, "hold_ms": 10.0, "release_ms": 40.0}


def _tts(**kw):
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    from supertonic_amd.tts import Style, load_text_to_speech
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, **kw)
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    return tts, Style(sttl, sdp)


def test_python_host_applies_the_expander_per_instance_and_per_call():
    assert binding.expander_args(LOWD) == LOW
    tts, style = _tts(noise_seed=21)
    plain, _ = tts.batch([TEXT], ["en"], style, 2, 1.05)
    tts.noise_seed, tts._calls = 21, 0
    got, _ = tts.batch([TEXT], ["en"], style, 2, 1.05, expander=LOWD)
    assert tts.engine.get_expander() is None  # the call's setting went with the call
    assert _same(got, tts.engine.op_expander(plain, tts.sample_rate, LOW)) and not _same(got, plain)
    with pytest.raises(ValueError):
        tts.batch([TEXT], ["en"], style, 2, 1.05, expander={"threshold": -20})
    with pytest.raises(binding.StnError):
        tts.batch([TEXT], ["en"], style, 2, 1.05, expander={"ratio": 40})
    assert tts.engine.get_expander() is None
    tts.engine.close()
    tts, style = _tts(noise_seed=21, output_rate=8000, expander=LOWD)
    assert tts.engine.get_expander() == _f32(LOW) and tts.settings.expander == LOW
    on, _ = tts.batch([TEXT], ["en"], style, 2, 1.05, encoding="mulaw")
    tts.noise_seed, tts._calls = 21, 0
    off, _ = tts.batch([TEXT], ["en"], style, 2, 1.05, expander=False)
    assert tts.engine.get_expander() == _f32(LOW)  # the instance's setting is back
    assert _same(on, g711_ref.encode(binding.ENC_MULAW, tts.engine.op_expander(off, 8000, LOW)))
    tts.engine.close()
    tts, style = _tts(noise_seed=21, expander=True)
    assert tts.engine.get_expander() == _f32(SPEECH)
    tts.engine.close()


def test_cli_expander_writes_the_bytes_the_binding_produces(tmp_path):
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    from supertonic_amd.tts import Style, load_text_to_speech
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    (tmp_path / "voice.json").write_text(json.dumps({"style_ttl": {"data": sttl.astype(np.float64).tolist(), "dims": list(sttl.shape)},
                                                     "style_dp": {"data": sdp.astype(np.float64).tolist(), "dims": list(sdp.shape)}}))
    args = ["--synthetic", "--text", TEXT, "--n-test", "1", "--seed", "3", "--total-step", "2", "--voice-style", "voice.json", "--save-dir", "out",
            "--sample-rate", "8000", "--encoding", "mulaw", "--expander", "-20:4:6:30:1:10:40"]
    p = subprocess.run([CLI] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    (f,) = os.listdir(tmp_path / "out")
    b = open(tmp_path / "out" / f, "rb").read()
    at = b.index(b"data")
    size = struct.unpack("<I", b[at + 4: at + 8])[0]
    data = np.frombuffer(b[at + 8: at + 8 + size], np.uint8)
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, noise_seed=3, output_rate=8000, expander=LOW)
    got, dur = tts(TEXT, "en", Style(sttl, sdp), 2, 1.05, 0.3, encoding="mulaw")
    tts.noise_seed, tts._calls = 3, 0
    off, _ = tts(TEXT, "en", Style(sttl, sdp), 2, 1.05, 0.3, encoding="mulaw", expander=False)
    tts.engine.close()
    n = min(data.size, got.shape[1])
    assert n > 1000 and abs(data.size - int(8000 * float(dur[0]))) <= 1 and np.array_equal(data[:n], got[0, :n]) and not np.array_equal(got, off)
    # a spelling beside a preset takes what it leaves out from that preset, in either order, as the binding's does
    both = binding.expander_args("-20:4", preset="gate")
    assert both == (-20.0, 4.0) + binding.EXPANDER_GATE[2:]
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, noise_seed=3, output_rate=8000, expander=both)
    want, _ = tts(TEXT, "en", Style(sttl, sdp), 2, 1.05, 0.3, encoding="mulaw")
    tts.engine.close()
    assert not np.array_equal(want, got)
    for k, tail in enumerate((["--expander-preset", "gate", "--expander", "-20:4"], ["--expander", "-20:4", "--expander-preset", "gate"])):
        assert args[-8:-6] == ["--save-dir", "out"] and args[-2] == "--expander"
        p = subprocess.run([CLI] + args[:-7] + ["out%d" % k] + args[-6:-2] + tail, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        (f,) = os.listdir(tmp_path / ("out%d" % k))
        b = open(tmp_path / ("out%d" % k) / f, "rb").read()
        at = b.index(b"data")
        d2 = np.frombuffer(b[at + 8: at + 8 + struct.unpack("<I", b[at + 4: at + 8])[0]], np.uint8)
        assert np.array_equal(d2[:n], want[0, :n]), tail
    # a value outside the limits is refused with the field named; so is a malformed spelling
    p = subprocess.run([CLI] + args[:-1] + ["-20:30"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "ratio" in p.stdout + p.stderr
    p = subprocess.run([CLI] + args[:-1] + ["-20"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "THRESHOLD:RATIO" in p.stdout + p.stderr


def test_service_expander_round_trip_and_unlike_settings_are_not_merged():
    from fastapi.testclient import TestClient
    from supertonic_amd import service
    tts, style = _tts(noise_seed=5)
    b = service.DynamicBatcher(tts, max_batch=16, max_wait_ms=400.0)
    texts = ["Hello there, this is the first request.", "And this one is the second request, a bit longer."]
    out = {}

    def go(i, c):
        out[i] = b.submit([texts[i % 2]], "en", style, 2, 1.05, expander=c)

    th = [threading.Thread(target=go, args=(i, c)) for i, c in enumerate((True, SPEECH, None, LOWD))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert sorted(b.batches) == [1, 1, 2]  # the two like requests (True is the speech default) shared a batch; the two others ran apart
    assert tts.engine.get_expander() is None and all(out[i][0][0].size > 1000 for i in range(4))
    with pytest.raises(ValueError) as ei:
        b.submit([texts[0]], "en", style, 2, 1.05, expander={"knee_db": 30})
    assert "knee_db" in str(ei.value)
    b.close()
    # the HTTP field: validated, handed to the engine for the request, gone after it
    app = service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=lambda paths: style)
    with TestClient(app) as c:
        for body in (True, LOWD):
            r = c.post("/tts", json={"text": texts[0], "expander": body, "filter_preset": "rumble", "sample_rate": 8000, "encoding": "mulaw"})
            assert r.status_code == 200 and r.content[:4] == b"RIFF" and len(r.content) > 1000
        r = c.post("/tts", json={"text": texts[0], "expander": {"attack_ms": 0.01}})
        assert r.status_code == 400 and "attack_ms" in r.json()["detail"]
        r = c.post("/tts", json={"text": texts[0], "expander": {"attack": 1}})
        assert r.status_code == 400 and "attack" in r.json()["detail"]
    assert tts.engine.get_expander() is None and tts.engine.output_rate == tts.sample_rate
    tts.engine.close()


# ---- 7. cost -----------------------------------------------------------------------------------------------------------------------------------------
CP_FAMILIES = ["out.compressor_chunks1", "out.compressor_scan1", "out.compressor_chunks2", "out.compressor_scan2", "out.compressor_write"]


def test_timing_report_c3_expander():
    """Event-timed cost on a C3-sized batch (128 rows) at the native rate, over 10 fetches after a warm one: the expander's five
    launches and its row results, beside the compressor's five launches on the same rows (the yardstick: the same bytes read and
    written, one transcendental pair per sample) in the same process and run.  Printed, not asserted; DESIGN.md section 25 records the
    values."""
    from supertonic_amd import host, workload
    from supertonic_amd.arch import default_arch
    from hip_util import DeviceBuffer
    a = default_arch()
    texts = workload.utterances(128, min_words=3, max_words=12, seed=11)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * 128)
    sttl, sdp = workload.synthetic_styles(a, list(range(128)))
    durs = workload.forced_durations(texts)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(5, 1.05, 1)

    def timed(fetch):
        fetch()  # warm: scratch, tables
        e.profile_enable(True)
        e.profile_reset()
        for _ in range(10):
            fetch()
        prof = e.profile()
        e.profile_enable(False)
        return {k: (v["ms"] * 1e3 / max(v["launches"], 1), v["launches"]) for k, v in prof.items() if k.startswith("out.")}

    B, _, W = e.batch_dims()
    dst = DeviceBuffer(np.zeros((B, W), np.float32))
    fetch = lambda: (e.batch_copy_wav_device(dst.ptr, W), e.sync())
    e.set_compressor(COMP)
    t = timed(fetch)
    yard = sum(t[k][0] for k in CP_FAMILIES)
    print(f"\nC3 batch, {B} x {W} samples at {a.sample_rate} Hz: the compressor's five launches "
          + ", ".join(f"{k} {t[k][0]:.1f} us" for k in CP_FAMILIES) + f": {yard:.1f} us")
    e.set_compressor(None)
    for name, setting in (("speech", SPEECH), ("gate", binding.EXPANDER_GATE), ("slow", (-40.0, 2.0, 12.0, 12.0, 300.0, 500.0, 3000.0))):
        e.set_expander(setting)
        t = timed(fetch)
        assert all(t[k][1] == 10 for k in FAMILIES), t
        five = sum(t[k][0] for k in FAMILIES[:5])
        print(f"{name}: " + ", ".join(f"{k} {us:.1f} us" for k, (us, n) in sorted(t.items()))
              + f"; the five launches {five:.1f} us, {five / yard:.2f} x the compressor's")
    e.set_expander(None)
    e.close()
