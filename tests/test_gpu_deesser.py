"""The fetch-time de-esser on an MI355X at the level of the fetches (include/stn.h "de-esser"; Engine::out_source, engine_batch.cpp;
DESIGN.md section 21), on synthetic weights and the batch of six rows the other fetch tests use, bf16 and f16: every fetch path delivers
stn_op_deesser of the fp32 fetch with the de-esser off, bit for bit, with the resampler, the filter chain and the compressor each on and
off (chain -> de-esser -> compressor is the three ops composed on the host); the encodings, the compressor, the edges, the loudness, the
limiter and the joins see the de-essed rows; stn_batch_deesser reports the reference's row maxima; results cached at fetch time (the
compressor's maxima, the edges) are keyed on the setting; off is the path without the feature; a rate at which the setting in force
breaks a limit is refused; the group, the Python host, the CLI and the service carry the setting.

The rows ("ess"): a 300 Hz tone at 0.4 behind 30 ms of silence with white noise on top, whose level alternates between 0.15 and 0.0005
every 50 ms: the band above 5.5 kHz is turned down by about 12 dB while the noise is there and not at all at the start of the row.
The rows of the cached-edges test ("tail"): the tone alone, and the last 60 ms of every row's span noise alone at 0.2, 5 dB under the
tone's frames behind a mild compressor: kept by a trim at 22 dB.  Behind WIDE (everything above 4 kHz, 10:1, up to 24 dB, on the whole
signal) that tail lies 25 dB under the tone and is silence, so the end edge depends on the setting; and the compressor's largest
reduction is the 2 dB it takes off the tone instead of the 4 dB it takes off the tail's peaks."""
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
import deesser_ref as dr
import g711_ref
import join_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
ENCS = ["f32", "pcm16", "pcm24", "mulaw", "alaw"]
ZERO = {e: binding.ZERO_CODEWORD[binding.ENCODINGS[e]] for e in ENCS}
DURS = np.array([0.71, 0.43, 0.92, 0.64, 0.51, 0.47], np.float32)
SPEECH = binding.DEESSER_SPEECH
WIDE = (4000.0, -36.0, 10.0, 0.0, 0.1, 10.0, 24.0, "wide")
COMP = binding.COMPRESSOR_SPEECH
HP = (("highpass", 80.0, 0.7071, 0.0),)
TRIM = (40.0, 20.0, 0.0)
FAMILIES = ["out.deesser_band_chunks", "out.deesser_band_scan", "out.deesser_chunks1", "out.deesser_scan1", "out.deesser_chunks2",
            "out.deesser_scan2", "out.deesser_write", "out.deesser_rowmax"]


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _tiny_batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 6, 14, [14, 9, 5, 12, 7, 11], seed=2)
    return a, ids, mask, sttl, sdp, DURS


def _spans(e, dur):
    _, _, Wo = e.batch_dims()
    return np.array([max(0, min(Wo, int(np.float32(d) * np.float32(e.output_rate)))) for d in dur], np.int64)


def _wav(a, e, kind="ess"):
    B, _, W = e.batch_dims()
    sr = a.sample_rate
    t = np.arange(W) / sr
    rng = np.random.default_rng(5)
    wav = np.zeros((B, W), np.float32)
    for b in range(B):
        tone = 0.4 * np.sin(2 * np.pi * (300.0 + 20.0 * b) * t) * (t >= 0.03)
        hiss = rng.standard_normal(W)
        if kind == "ess":
            on = (((t * 1000.0 + 7.0 * b) // 50.0) % 2 == 0) & (t >= 0.03)
            wav[b] = tone + np.where(on, 0.15, 0.0005) * hiss
        else:
            nb = min(W, int(np.float32(DURS[b] / np.float32(1.05)) * np.float32(sr)))
            at = max(0, nb - int(0.06 * sr))
            wav[b] = tone
            wav[b, at:] = 0.2 * hiss[at:]
    return wav


def _engine(dtype, seed=9, kind="ess"):
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    e = binding.Engine(0, dtype)
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, seed)
    e.dbg_batch_set_wav(_wav(a, e, kind))
    return a, e


def _f32(setting):
    return tuple(np.float32(v) for v in setting[:7]) + (setting[7],)


# ---- 1. identity: every fetch path delivers the de-essed rows, in front of the compressor ------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_fetch_path_delivers_op_deesser_of_the_fetch_without_it(dtype):
    from hip_util import DeviceBuffer
    a, e = _engine(dtype)
    assert e.get_deesser() is None
    combos = list(itertools.product((None, 16000), (None, HP), (None, COMP)))
    for i, (rate, chain, comp) in enumerate(combos):
        setting = (SPEECH, WIDE)[i % 2]
        e.set_output_rate(rate)
        e.set_filters(chain)
        e.set_compressor(None)
        e.set_deesser(None)
        assert not e.batch_deesser().any()
        plain, dur = e.batch_fetch()
        hz = e.output_rate
        want = e.op_deesser(plain, hz, setting)
        assert np.abs(want - plain).max() > 0.05
        if comp:
            want = e.op_compressor(want, hz, comp)
        if chain and comp:  # the order: chain -> de-esser -> compressor, the three ops composed on the host
            e.set_filters(None)
            raw = e.batch_fetch()[0]
            e.set_filters(chain)
            assert _same(want, e.op_compressor(e.op_deesser(e.op_filter(raw, hz, chain), hz, setting), hz, comp)), (dtype, rate)
        e.set_compressor(comp)
        e.set_deesser(setting)
        assert e.get_deesser() == _f32(setting)
        got, gdur = e.batch_fetch()
        assert _same(got, want) and gdur.tobytes() == dur.tobytes(), (dtype, rate, chain, comp, setting)
        B, _, Wo = e.batch_dims()
        for enc in ENCS:
            enc_want = want if enc == "f32" else e.op_encode(want, enc)
            assert _same(e.batch_fetch_encoded(enc)[0], enc_want), (dtype, rate, chain, comp, enc)
            for slot in (0, 1):
                e.fetch_encoded_begin(slot, enc)
                assert _same(np.asarray(e.fetch_encoded_end(slot)[0]).reshape(enc_want.shape), enc_want), (dtype, rate, chain, comp, enc, slot)
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
        # the report: the float64 reference's maxima of yL over the rows' valid samples, within 4 x the float32 restatement's deviation
        # (on the rows in front of the de-esser; once per rate is enough, the chain and the compressor do not enter it)
        n = _spans(e, dur)
        rep = e.batch_deesser()
        if chain is None and comp is None and (rate or dtype == "bf16"):
            f = dr.coefs(setting, hz)
            r64, r32 = dr.Ref(plain, f, np.float64), dr.Ref(plain, f, np.float32)
            bound = 4 * np.abs(r32.yl - r64.yl).max()
            ref_max = np.array([r64.yl[b, : n[b]].max() for b in range(B)])
            assert ref_max.min() >= 6.0 and bound > 0 and np.abs(rep - ref_max).max() <= bound, (dtype, rate, setting, rep, ref_max, bound)
        gr = e.op_deesser_ex(plain, hz, setting)["gr_db"]
        assert _same(rep, np.array([gr[b, : n[b]].max() for b in range(B)], np.float32)), (dtype, rate, chain, comp)
        # the batch's own waveform is untouched
        e.set_compressor(None)
        e.set_deesser(None)
        assert _same(e.batch_fetch()[0], plain)
    e.close()


# ---- 2. order: everything behind the de-esser sees the de-essed rows -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_the_compressor_and_the_level_based_steps_run_on_the_deessed_rows(dtype):
    for rate, chain in ((None, None), (16000, HP)):
        a, e = _engine(dtype)
        e.set_output_rate(rate)
        e.set_filters(chain)
        hz = e.output_rate
        plain, dur = e.batch_fetch()
        n = _spans(e, dur)
        B = len(n)
        e.set_deesser(WIDE)
        xd = e.batch_fetch()[0]
        assert _same(xd, e.op_deesser(plain, hz, WIDE))
        # the compressor's report is that of the de-essed rows
        e.set_compressor(COMP)
        gr = e.op_compressor_ex(xd, hz, COMP)["gr_db"]
        want = np.array([gr[b, : n[b]].max() for b in range(B)], np.float32)
        assert _same(e.batch_compressor(), want) and want.max() > 1.0, (rate, want)
        gr0 = e.op_compressor_ex(plain, hz, COMP)["gr_db"]
        assert not _same(want, np.array([gr0[b, : n[b]].max() for b in range(B)], np.float32))
        e.set_compressor(None)
        e.set_silence_trim(TRIM)
        s1, e1 = e.batch_silence_edges()
        e.set_silence_trim(None)
        os_, oe = e.op_silence_edges(xd, hz, n, TRIM[0], TRIM[1])
        assert np.array_equal(s1, os_) and np.array_equal(e1, oe), (rate, s1, os_)
        lufs, peak, _ = e.batch_loudness()
        ol, op = e.op_loudness(xd, hz, n)
        assert _same(lufs, ol) and _same(peak, op), rate
        assert np.all(e.op_loudness(plain, hz, n)[0] - lufs > 0.5)  # (what is measured was turned down)
        assert _same(e.batch_true_peak()[0], e.op_true_peak(xd, hz, n)["tp"]), rate
        e.set_loudness(-6.0, -1.0)
        e.set_limiter(5.0)
        g = e.batch_loudness()[2]
        red, lim = e.batch_limiter()
        y, s, ored, olim = e.op_limiter(xd, hz, n, g, -1.0, 5.0)
        assert _same(red, ored) and np.array_equal(lim, olim) and lim.any(), rate
        lim_rows = e.batch_fetch()[0]
        assert all(_same(lim_rows[b, : n[b]], y[b, : n[b]]) for b in range(B)), rate
        e.close()


def test_cached_compressor_maxima_and_edges_are_keyed_on_the_setting():
    a, e = _engine("bf16", kind="tail")
    hz = e.output_rate
    plain, dur = e.batch_fetch()
    n = _spans(e, dur)
    B = len(n)
    trim = (22.0, 5.0, 0.0)  # (module docstring)
    comp = (-12.0, 2.0, 0.0, 1.0, 50.0, 0.0)  # (2 dB off the tone, 4 dB off the tail's peaks)
    e.set_silence_trim(trim)
    e.set_compressor(comp)
    first = e.batch_fetch_encoded("pcm16")[0]
    s0, e0 = e.batch_silence_edges()
    r0 = e.batch_compressor()
    seen = []
    for setting in (WIDE, SPEECH, WIDE, None):
        e.set_deesser(setting)
        # the reports first, without a fetch in between: a stale key would hand back those of the setting before
        rep = e.batch_compressor()
        s1, e1 = e.batch_silence_edges()
        xd = plain if setting is None else e.op_deesser(plain, hz, setting)
        o = e.op_compressor_ex(xd, hz, comp)
        assert _same(rep, np.array([o["gr_db"][b, : n[b]].max() for b in range(B)], np.float32)), setting
        ws, we = e.op_silence_edges(o["y"], hz, n, trim[0], trim[1])
        assert np.array_equal(s1, ws) and np.array_equal(e1, we), setting
        got = e.batch_fetch_encoded("pcm16")[0]
        want = np.zeros_like(got)
        pcm = g711_ref.pcm16(o["y"])
        for b in range(B):
            want[b, : we[b] - ws[b]] = pcm[b, ws[b]:we[b]]
        assert _same(got, want), setting
        seen.append((e1.tolist(), rep.tolist()))
        if setting is None:
            assert _same(got, first) and np.array_equal(s1, s0) and np.array_equal(e1, e0) and _same(rep, r0)
    # the end edges and the compressor's maxima depend on the setting: a stale key would show
    assert seen[0] == seen[2] and all(x < y for x, y in zip(seen[0][0], seen[3][0])) and seen[0][1] != seen[3][1]
    e.close()


# ---- 3. joined fetches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_joined_fetch_is_the_host_join_of_the_deessed_rows(dtype):
    import math
    a, e = _engine(dtype)
    rows, gap_s = [2, 1, 3], [0.3, 0.25, 0.0]
    cs = a.base_chunk_size * a.chunk_compress_factor
    for rate, chain, comp, trim in ((None, None, None, None), (16000, HP, COMP, None), (None, HP, None, TRIM), (16000, None, COMP, TRIM)):
        e.set_output_rate(rate)
        e.set_filters(chain)
        e.set_deesser(SPEECH)
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
            assert np.array_equal(plen, p["prog_len"]) and _same(got, want), (dtype, rate, chain, comp, trim, lo, enc)
        # one gain per programme: the joined de-essed fp32 signal times float32(g_g)
        e.set_loudness(None)
        joined, _, _ = e.batch_fetch_joined(rows, gap, gap_s, cut=False)
        e.set_loudness(-20.0)
        g = e.batch_join_loudness(rows, gap, gap_s)[2]
        got, _, _ = e.batch_fetch_joined(rows, gap, gap_s, gain_scope="programme", cut=False)
        assert _same(got, (joined * g[:, None]).astype(np.float32)), (dtype, rate, chain, comp, trim)
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
    assert cached >= 1 and replays >= 1 and e.get_deesser() is None
    ptr = e.batch_wav_device_ptr()
    latent = e.batch_fetch_latent()
    for setting in (True, WIDE, {"freq_hz": 6000, "threshold_db": -28}):  # three changes
        e.set_deesser(setting)
        fams = [f for f, _ in _launches(e, lambda: e.batch_fetch_encoded("mulaw"))]
        assert [f for f in fams if "deesser" in f] == FAMILIES, fams
        e.batch_fetch_joined([6], 100, 0.1)
        assert e.batch_wav_device_ptr() == ptr and _same(e.batch_fetch_latent(), latent)
    last = _f32((6000.0, -28.0) + SPEECH[2:])
    assert e.get_deesser() == last
    for i, (field, bad) in enumerate(zip(dr.FIELDS[:7], (12001.0, 1.0, 21.0, -1.0, 301.0, 3001.0, float("nan")))):
        s = list(WIDE[:7])
        s[i] = bad
        with pytest.raises(binding.StnError) as ei:  # (through the C ABI itself: the binding's own parser would stop the NaN first)
            e._ck(e._lib.stn_set_deesser(e._h, 1, ctypes.byref(binding.StnDeesser(*s, 1))))
        assert ei.value.code == -1 and field in str(ei.value), (field, str(ei.value))
    with pytest.raises(binding.StnError) as ei:
        e._ck(e._lib.stn_set_deesser(e._h, 1, ctypes.byref(binding.StnDeesser(*WIDE[:7], 7))))
    assert "mode" in str(ei.value) and e.get_deesser() == last  # the previous setting stayed in force
    # freq_hz is checked against the rate: a rate at which the setting in force breaks a limit is refused, and the rate stays
    e.set_output_rate(16000)
    for setting in (True, last):
        e.set_deesser(setting)
        with pytest.raises(binding.StnError) as ei:
            e.set_output_rate(8000)
        assert "freq_hz" in str(ei.value) and "0.45" in str(ei.value) and e.output_rate == 16000 and e.get_deesser() == _f32(binding.deesser_args(setting))
    with pytest.raises(binding.StnError) as ei:  # and so is a setting that breaks one at the rate in force
        e.set_deesser({"freq_hz": 8000})
    assert "freq_hz" in str(ei.value) and e.get_deesser() == last
    e.set_deesser(False)
    e.set_output_rate(8000)  # off, nothing stands in the way
    e.set_output_rate(None)
    assert e.graphs_cached == cached and e.graph_replays == replays
    for rate, lo, trim in ((None, None, None), (16000, -20.0, None), (None, None, (40.0, 20.0, 5.0)), (16000, -20.0, (40.0, 20.0, 5.0))):
        for x in (e, fresh):
            x.set_output_rate(rate)
            x.set_loudness(lo)
            x.set_silence_trim(trim)
        for enc in ENCS:
            assert _same(e.batch_fetch_encoded(enc)[0], fresh.batch_fetch_encoded(enc)[0]), (rate, lo, trim, enc)
            log = _launches(e, lambda: e.batch_fetch_encoded(enc))
            assert log == _launches(fresh, lambda: fresh.batch_fetch_encoded(enc)) and "deesser" not in str(log)
        for slot in (0, 1):
            e.fetch_encoded_begin(slot, "pcm16")
            fresh.fetch_encoded_begin(slot, "pcm16")
            assert _same(e.fetch_encoded_end(slot)[0], fresh.fetch_encoded_end(slot)[0])
        j = ([2, 4], [100, 7], 0.3)
        assert _same(e.batch_fetch_joined(*j, cut=False)[0], fresh.batch_fetch_joined(*j, cut=False)[0])
        assert _launches(e, lambda: e.batch_fetch_joined(*j)) == _launches(fresh, lambda: fresh.batch_fetch_joined(*j))
    assert not e.batch_deesser().any()
    e.batch_run(2, 1.05, 4)
    assert e.graphs_cached == cached and e.graph_replays == replays + 1  # the next run is a replay
    e.close()
    fresh.close()


# ---- 5. the group --------------------------------------------------------------------------------------------------------------------------------
LOW = {"freq_hz": 2000.0, "threshold_db": -60.0, "ratio": 20.0, "knee_db": 0.0, "range_db": 24.0, "mode": "wide"}  # (low enough for what
LOW8 = (2000.0, -60.0, 20.0, 0.0, 1.0, 40.0, 24.0, "wide")                                                         # synthetic weights produce)


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
    g.set_deesser(LOW8)
    pcm, dur = g.synthesize(ids, mask, sttl, sdp, 2, 1.05, duration_override=durs, noise_seed=5)
    lengths = mask.sum(axis=(1, 2)).astype(np.int32)
    rank_of, row_of = binding.group_deal(lengths, 1)
    order = np.argsort(row_of)
    eng = binding.Engine(0, "bf16")
    eng.load_synthetic(arch, 7)
    eng.set_deesser(LOW8)
    eng.batch_upload(ids[order], mask[order], sttl[order], sdp[order], duration_override=durs[order], utt_ids=order.astype(np.int64))
    eng.batch_run(2, 1.05, 5)
    ref, _ = eng.batch_fetch_pcm16()
    assert np.array_equal(pcm[order][:, : ref.shape[1]], ref)
    eng.set_deesser(None)
    assert not np.array_equal(eng.batch_fetch_pcm16()[0], ref)
    with pytest.raises(binding.StnError) as ei:
        g.set_deesser(SPEECH[:2] + (30.0,) + SPEECH[3:])
    assert "ratio" in str(ei.value)
    g.set_deesser(None)
    g.close()
    eng.close()


# ---- 6. the hosts ---------------------------------------------------------------------------------------------------------------------------------
TEXT = "She sells sea shells: the engine turns the sibilants of every utterance down on the device."


def _tts(**kw):
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    from supertonic_amd.tts import Style, load_text_to_speech
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, **kw)
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    return tts, Style(sttl, sdp)


def test_python_host_applies_the_deesser_per_instance_and_per_call():
    tts, style = _tts(noise_seed=21)
    plain, _ = tts.batch([TEXT], ["en"], style, 2, 1.05)
    tts.noise_seed, tts._calls = 21, 0
    got, _ = tts.batch([TEXT], ["en"], style, 2, 1.05, deesser=LOW)
    assert tts.engine.get_deesser() is None  # the call's setting went with the call
    assert _same(got, tts.engine.op_deesser(plain, tts.sample_rate, LOW8)) and not _same(got, plain)
    with pytest.raises(ValueError):
        tts.batch([TEXT], ["en"], style, 2, 1.05, deesser={"freq": 6000})
    with pytest.raises(binding.StnError):
        tts.batch([TEXT], ["en"], style, 2, 1.05, deesser={"ratio": 40})
    assert tts.engine.get_deesser() is None
    tts.engine.close()
    tts, style = _tts(noise_seed=21, deesser=True)
    assert tts.engine.get_deesser() == _f32(SPEECH) and tts.settings.deesser == SPEECH
    with pytest.raises(binding.StnError) as ei:  # the instance's default at 8 kHz: refused, and everything is as it was
        tts.batch([TEXT], ["en"], style, 2, 1.05, output_rate=8000)
    assert "freq_hz" in str(ei.value) and tts.engine.output_rate == tts.sample_rate and tts.engine.get_deesser() == _f32(SPEECH)
    tts.engine.close()
    tts, style = _tts(noise_seed=21, output_rate=8000, deesser=dict(LOW, freq_hz=3000.0))
    low8k = (3000.0,) + LOW8[1:]
    assert tts.engine.get_deesser() == _f32(low8k) and tts.settings.deesser == low8k
    on, _ = tts.batch([TEXT], ["en"], style, 2, 1.05, encoding="mulaw")
    tts.noise_seed, tts._calls = 21, 0
    off, _ = tts.batch([TEXT], ["en"], style, 2, 1.05, deesser=False)
    assert tts.engine.get_deesser() == _f32(low8k)  # the instance's setting is back
    assert _same(on, g711_ref.encode(binding.ENC_MULAW, tts.engine.op_deesser(off, 8000, low8k)))
    tts.engine.close()


def test_cli_deesser_writes_the_bytes_the_binding_produces(tmp_path):
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    from supertonic_amd.tts import Style, load_text_to_speech
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    (tmp_path / "voice.json").write_text(json.dumps({"style_ttl": {"data": sttl.astype(np.float64).tolist(), "dims": list(sttl.shape)},
                                                     "style_dp": {"data": sdp.astype(np.float64).tolist(), "dims": list(sdp.shape)}}))
    args = ["--synthetic", "--text", TEXT, "--n-test", "1", "--seed", "3", "--total-step", "2", "--voice-style", "voice.json", "--save-dir", "out",
            "--sample-rate", "16000", "--encoding", "mulaw", "--deesser", "2000:-60:20:0:1:40:24:wide"]
    p = subprocess.run([CLI] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    (f,) = os.listdir(tmp_path / "out")
    b = open(tmp_path / "out" / f, "rb").read()
    at = b.index(b"data")
    size = struct.unpack("<I", b[at + 4: at + 8])[0]
    data = np.frombuffer(b[at + 8: at + 8 + size], np.uint8)
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, noise_seed=3, output_rate=16000, deesser=LOW8)
    got, dur = tts(TEXT, "en", Style(sttl, sdp), 2, 1.05, 0.3, encoding="mulaw")
    tts.noise_seed, tts._calls = 3, 0
    off, _ = tts(TEXT, "en", Style(sttl, sdp), 2, 1.05, 0.3, encoding="mulaw", deesser=False)
    tts.engine.close()
    n = min(data.size, got.shape[1])
    assert n > 1000 and abs(data.size - int(16000 * float(dur[0]))) <= 1 and np.array_equal(data[:n], got[0, :n]) and not np.array_equal(got, off)
    # a value outside the limits is refused with the field named, the corner that depends on the rate included; so is a malformed spelling
    for spec, word in (("2000:-60:30", "ratio"), ("8000:-30", "freq_hz"), ("2000", "FREQ:THRESHOLD")):
        p = subprocess.run([CLI] + args[:-1] + [spec], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode != 0 and word in p.stdout + p.stderr, (spec, p.stdout + p.stderr)
    p = subprocess.run([CLI] + args[:-2] + ["--deesser-preset", "speech"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr


def test_service_deesser_round_trip_and_unlike_settings_are_not_merged():
    from fastapi.testclient import TestClient
    from supertonic_amd import service
    tts, style = _tts(noise_seed=5)
    b = service.DynamicBatcher(tts, max_batch=16, max_wait_ms=400.0)
    texts = ["Hello there, this is the first request.", "And this one is the second request, a bit longer."]
    out = {}

    def go(i, c):
        out[i] = b.submit([texts[i % 2]], "en", style, 2, 1.05, deesser=c)

    th = [threading.Thread(target=go, args=(i, c)) for i, c in enumerate((True, SPEECH, None, LOW))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert sorted(b.batches) == [1, 1, 2]  # the two like requests (True is the speech default) shared a batch; the two others ran apart
    assert tts.engine.get_deesser() is None and all(out[i][0][0].size > 1000 for i in range(4))
    with pytest.raises(ValueError) as ei:
        b.submit([texts[0]], "en", style, 2, 1.05, deesser={"knee_db": 30})
    assert "knee_db" in str(ei.value)
    b.close()
    # the HTTP field: validated against the request's rate, handed to the engine for the request, gone after it
    app = service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=lambda paths: style)
    with TestClient(app) as c:
        for body in (True, LOW):
            r = c.post("/tts", json={"text": texts[0], "deesser": body, "compressor": True, "sample_rate": 16000, "encoding": "mulaw"})
            assert r.status_code == 200 and r.content[:4] == b"RIFF" and len(r.content) > 1000
        r = c.post("/tts", json={"text": texts[0], "deesser": True, "sample_rate": 8000})
        assert r.status_code == 400 and "freq_hz" in r.json()["detail"]
        r = c.post("/tts", json={"text": texts[0], "deesser": {"attack": 1}})
        assert r.status_code == 400 and "attack" in r.json()["detail"]
    assert tts.engine.get_deesser() is None and tts.engine.output_rate == tts.sample_rate
    tts.engine.close()


# ---- 7. cost -----------------------------------------------------------------------------------------------------------------------------------------
def test_timing_report_c3_deesser():
    """Event-timed cost on a C3-sized batch (128 rows) at the native rate, over 10 fetches after a warm one: the de-esser's eight
    launches beside the compressor's five and one section pass of the filter chain (the yardsticks: the same reads of the same rows)
    in the same process and run.  Printed, not asserted; DESIGN.md section 21 records the values."""
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
    e.set_filters([("highpass", 80.0, 0.5412), ("highpass", 80.0, 1.3066)])  # one section pass
    t = timed(fetch)
    e.set_filters(None)
    section = sum(t[k][0] for k in ("out.filter_chunks", "out.filter_scan", "out.filter_write"))
    print(f"\nC3 batch, {B} x {W} samples at {a.sample_rate} Hz: " + ", ".join(f"{k} {us:.1f} us" for k, (us, n) in sorted(t.items()))
          + f"; one section pass {section:.1f} us")
    e.set_compressor(COMP)
    t = timed(fetch)
    e.set_compressor(None)
    cfam = ["out.compressor_chunks1", "out.compressor_scan1", "out.compressor_chunks2", "out.compressor_scan2", "out.compressor_write"]
    five = sum(t[k][0] for k in cfam)
    print("compressor: " + ", ".join(f"{k} {us:.1f} us" for k, (us, n) in sorted(t.items())) + f"; the five launches {five:.1f} us")
    for name, setting in (("speech", SPEECH), ("wide", WIDE[:7] + ("wide",)), ("slow", (8000.0, -30.0, 3.0, 12.0, 20.0, 300.0, 6.0, "split"))):
        e.set_deesser(setting)
        t = timed(fetch)
        assert all(t[k][1] == 10 for k in FAMILIES), t
        eight = sum(t[k][0] for k in FAMILIES)
        print(f"{name}: " + ", ".join(f"{k} {t[k][0]:.1f} us" for k in FAMILIES)
              + f"; the eight launches {eight:.1f} us, {eight / (section + five):.2f} x one section pass plus the compressor's five ({section + five:.1f} us)")
    e.set_deesser(None)
    e.close()
