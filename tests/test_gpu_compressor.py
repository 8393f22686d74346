"""The fetch-time compressor on an MI355X at the level of the fetches (include/stn.h "compressor"; Engine::out_source, engine_batch.cpp;
DESIGN.md section 20), on synthetic weights and the batch of six rows the other fetch tests use, bf16 and f16: every fetch path delivers
stn_op_compressor of the fp32 fetch with the compressor off, bit for bit, with the resampler and the filter chain on and off; the
encodings, the edges, the loudness, the limiter and the joins see the compressed rows; stn_batch_compressor reports the reference's row
maxima; results cached at fetch time are keyed on the setting; off is the path without the feature; the group, the Python host, the
CLI and the service carry the setting.

The rows ("dyn"): a 300 Hz tone whose amplitude alternates between 0.6 and 0.03 every 50 ms behind 30 ms of silence, so that the
compressor (threshold -24 dBFS) turns the loud halves down by more than 6 dB and leaves the start of the row alone; the last 60 ms of
every row's span are quiet.

The cached-edges test trims at 22 dB under the loudest frame.  Uncompressed, the quiet tail (26 dB under the loud halves) is silence and
the end edge lies in front of it.  Behind FAST (8:1, release 10 ms) the loud halves come down by 17 dB and the tail, released within
its first 20 ms, lies 9 dB under them, 16.5 dB under the frame of the first attack: no silence, the end edge is the span's end."""
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
import compressor_ref as cr
import g711_ref
import join_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
ENCS = ["f32", "pcm16", "pcm24", "mulaw", "alaw"]
ZERO = {e: binding.ZERO_CODEWORD[binding.ENCODINGS[e]] for e in ENCS}
DURS = np.array([0.71, 0.43, 0.92, 0.64, 0.51, 0.47], np.float32)
SPEECH = binding.COMPRESSOR_SPEECH
HARD = (-30.0, 8.0, 0.0, 1.0, 50.0, 6.0)
FAST = (-24.0, 8.0, 6.0, 1.0, 10.0, 0.0)
HP = (("highpass", 80.0, 0.7071, 0.0),)
TRIM = (40.0, 20.0, 0.0)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _tiny_batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 6, 14, [14, 9, 5, 12, 7, 11], seed=2)
    return a, ids, mask, sttl, sdp, DURS


def _spans(e, dur):
    _, _, Wo = e.batch_dims()
    return np.array([max(0, min(Wo, int(np.float32(d) * np.float32(e.output_rate)))) for d in dur], np.int64)


def _dyn_wav(a, e):
    B, _, W = e.batch_dims()
    sr = a.sample_rate
    t = np.arange(W) / sr
    wav = np.zeros((B, W), np.float32)
    for b in range(B):
        amp = np.where(((t * 1000.0 + 7.0 * b) // 50.0) % 2 == 0, 0.6, 0.03) * (t >= 0.03)
        nb = min(W, int(np.float32(DURS[b] / np.float32(1.05)) * np.float32(sr)))
        amp[max(0, nb - int(0.06 * sr)):] = 0.03  # (the last 60 ms of the span: quiet)
        wav[b] = amp * np.sin(2 * np.pi * (300.0 + 20.0 * b) * t)
    return wav


def _engine(dtype, seed=9):
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    e = binding.Engine(0, dtype)
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, seed)
    e.dbg_batch_set_wav(_dyn_wav(a, e))
    return a, e


def _f32(setting):
    return tuple(np.float32(v) for v in setting)


# ---- 1. identity: every fetch path delivers the compressed rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_fetch_path_delivers_op_compressor_of_the_uncompressed_fetch(dtype):
    from hip_util import DeviceBuffer
    a, e = _engine(dtype)
    assert e.get_compressor() is None
    for rate, chain, setting in itertools.product((None, 16000), (None, HP), (SPEECH, HARD)):
        e.set_output_rate(rate)
        e.set_filters(chain)
        e.set_compressor(None)
        assert not e.batch_compressor().any()
        plain, dur = e.batch_fetch()
        want = e.op_compressor(plain, e.output_rate, setting)
        assert np.abs(want - plain).max() > 0.05
        e.set_compressor(setting)
        assert e.get_compressor() == _f32(setting)
        got, gdur = e.batch_fetch()
        assert _same(got, want) and gdur.tobytes() == dur.tobytes(), (dtype, rate, chain, setting)
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
        for enc in ENCS:  # the encodings against the host rules on the compressed fp32 rows
            assert _same(e.batch_fetch_encoded(enc)[0], g711_ref.encode(binding.ENCODINGS[enc], want)), (dtype, rate, enc)
        assert _same(e.batch_fetch_pcm16()[0], g711_ref.pcm16(want))
        # the report: the float64 reference's maxima of yL over the rows' valid samples, within 4 x the float32 restatement's deviation
        f = cr.coefs(setting, e.output_rate)
        r64, r32 = cr.Ref(plain, f, np.float64), cr.Ref(plain, f, np.float32)
        bound = 4 * np.abs(r32.yl - r64.yl).max()
        n = _spans(e, dur)
        ref_max = np.array([r64.yl[b, : n[b]].max() for b in range(B)])
        rep = e.batch_compressor()
        assert ref_max.min() >= 6.0 and bound > 0 and np.abs(rep - ref_max).max() <= bound, (dtype, rate, chain, setting, rep, ref_max, bound)
        # the batch's own waveform is untouched
        e.set_compressor(None)
        assert _same(e.batch_fetch()[0], plain)
    e.close()


# ---- 2. order: everything behind the compressor sees the compressed rows ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_the_level_based_steps_run_on_the_compressed_rows(dtype):
    for rate, chain in ((None, None), (16000, HP)):
        a, e = _engine(dtype)
        e.set_output_rate(rate)
        e.set_filters(chain)
        hz = e.output_rate
        plain, dur = e.batch_fetch()
        n = _spans(e, dur)
        e.set_compressor(SPEECH)
        xc = e.batch_fetch()[0]
        assert _same(xc, e.op_compressor(plain, hz, SPEECH))
        e.set_silence_trim(TRIM)
        s1, e1 = e.batch_silence_edges()
        e.set_silence_trim(None)
        os_, oe = e.op_silence_edges(xc, hz, n, TRIM[0], TRIM[1])
        assert np.array_equal(s1, os_) and np.array_equal(e1, oe), (rate, s1, os_)
        lufs, peak, _ = e.batch_loudness()
        ol, op = e.op_loudness(xc, hz, n)
        assert _same(lufs, ol) and _same(peak, op), rate
        assert np.all(e.op_loudness(plain, hz, n)[0] - lufs > 3.0)  # (what is measured was turned down)
        assert _same(e.batch_true_peak()[0], e.op_true_peak(xc, hz, n)["tp"]), rate
        e.set_loudness(-6.0, -1.0)
        e.set_limiter(5.0)
        g = e.batch_loudness()[2]
        red, lim = e.batch_limiter()
        y, s, ored, olim = e.op_limiter(xc, hz, n, g, -1.0, 5.0)
        assert _same(red, ored) and np.array_equal(lim, olim) and lim.any(), rate
        lim_rows = e.batch_fetch()[0]
        assert all(_same(lim_rows[b, : n[b]], y[b, : n[b]]) for b in range(len(n))), rate
        e.close()


def test_cached_edges_are_keyed_on_the_setting():
    a, e = _engine("bf16")
    hz = e.output_rate
    plain, dur = e.batch_fetch()
    n = _spans(e, dur)
    trim = (22.0, 5.0, 0.0)  # (module docstring)
    e.set_silence_trim(trim)
    first = e.batch_fetch_encoded("pcm16")[0]
    s0, e0 = e.batch_silence_edges()
    seen = []
    for setting in (FAST, SPEECH, FAST, None):
        e.set_compressor(setting)
        got = e.batch_fetch_encoded("pcm16")[0]  # (the fetch first: a stale key would cut by the edges of the setting before)
        s1, e1 = e.batch_silence_edges()
        xc = plain if setting is None else e.op_compressor(plain, hz, setting)
        ws, we = e.op_silence_edges(xc, hz, n, trim[0], trim[1])
        assert np.array_equal(s1, ws) and np.array_equal(e1, we), setting
        want = np.zeros_like(got)
        pcm = g711_ref.pcm16(xc)
        for b in range(len(n)):
            want[b, : we[b] - ws[b]] = pcm[b, ws[b]:we[b]]
        assert _same(got, want), setting
        seen.append((s1.tolist(), e1.tolist()))
        if setting is None:
            assert _same(got, first) and np.array_equal(s1, s0) and np.array_equal(e1, e0)
    assert seen[0] == seen[2] and all(a > b for a, b in zip(seen[0][1], seen[3][1]))  # (the end edges depend on the setting: a stale key would show)
    e.close()


# ---- 3. joined fetches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_joined_fetch_is_the_host_join_of_the_compressed_rows(dtype):
    import math
    a, e = _engine(dtype)
    rows, gap_s = [2, 1, 3], [0.3, 0.25, 0.0]
    cs = a.base_chunk_size * a.chunk_compress_factor
    for rate, chain, trim in ((None, None, None), (16000, HP, None), (None, HP, TRIM), (16000, None, TRIM)):
        e.set_output_rate(rate)
        e.set_filters(chain)
        e.set_compressor(SPEECH)
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
            assert np.array_equal(plen, p["prog_len"]) and _same(got, want), (dtype, rate, chain, trim, lo, enc)
        # one gain per programme: the joined compressed fp32 signal times float32(g_g)
        e.set_loudness(None)
        joined, _, _ = e.batch_fetch_joined(rows, gap, gap_s, cut=False)
        e.set_loudness(-20.0)
        g = e.batch_join_loudness(rows, gap, gap_s)[2]
        got, _, _ = e.batch_fetch_joined(rows, gap, gap_s, gain_scope="programme", cut=False)
        assert _same(got, (joined * g[:, None]).astype(np.float32)), (dtype, rate, chain, trim)
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


FAMILIES = ["out.compressor_chunks1", "out.compressor_scan1", "out.compressor_chunks2", "out.compressor_scan2", "out.compressor_write",
            "out.compressor_rowmax"]


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
    assert cached >= 1 and replays >= 1 and e.get_compressor() is None
    ptr = e.batch_wav_device_ptr()
    latent = e.batch_fetch_latent()
    for setting in (True, HARD, {"threshold_db": -18, "ratio": 2}):  # three changes
        e.set_compressor(setting)
        fams = [f for f, _ in _launches(e, lambda: e.batch_fetch_encoded("mulaw"))]
        assert [f for f in fams if "compressor" in f] == FAMILIES, fams
        e.batch_fetch_joined([6], 100, 0.1)
        assert e.batch_wav_device_ptr() == ptr and _same(e.batch_fetch_latent(), latent)
    assert e.get_compressor() == _f32((-18.0, 2.0) + SPEECH[2:])
    for i, (field, bad) in enumerate(zip(cr.FIELDS, (1.0, 21.0, -1.0, 301.0, 3001.0, float("nan")))):
        s = list(HARD)
        s[i] = bad
        with pytest.raises(binding.StnError) as ei:  # (through the C ABI itself: the binding's own parser would stop the NaN first)
            e._ck(e._lib.stn_set_compressor(e._h, 1, ctypes.byref(binding.StnCompressor(*s))))
        assert ei.value.code == -1 and field in str(ei.value), (field, str(ei.value))
    assert e.get_compressor() == _f32((-18.0, 2.0) + SPEECH[2:])  # the previous setting stayed in force
    for rate in (8000, 192000, None):  # no limit depends on the rate
        e.set_output_rate(rate)
    e.set_compressor(False)
    assert e.graphs_cached == cached and e.graph_replays == replays
    for rate, lo, trim in ((None, None, None), (16000, -20.0, None), (None, None, (40.0, 20.0, 5.0)), (16000, -20.0, (40.0, 20.0, 5.0))):
        for x in (e, fresh):
            x.set_output_rate(rate)
            x.set_loudness(lo)
            x.set_silence_trim(trim)
        for enc in ENCS:
            assert _same(e.batch_fetch_encoded(enc)[0], fresh.batch_fetch_encoded(enc)[0]), (rate, lo, trim, enc)
            log = _launches(e, lambda: e.batch_fetch_encoded(enc))
            assert log == _launches(fresh, lambda: fresh.batch_fetch_encoded(enc)) and "compressor" not in str(log)
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
    setting = (-40.0, 8.0, 6.0, 1.0, 50.0, 3.0)  # (low enough for what synthetic weights produce)
    g.set_compressor(setting)
    pcm, dur = g.synthesize(ids, mask, sttl, sdp, 2, 1.05, duration_override=durs, noise_seed=5)
    lengths = mask.sum(axis=(1, 2)).astype(np.int32)
    rank_of, row_of = binding.group_deal(lengths, 1)
    order = np.argsort(row_of)
    eng = binding.Engine(0, "bf16")
    eng.load_synthetic(arch, 7)
    eng.set_compressor(setting)
    eng.batch_upload(ids[order], mask[order], sttl[order], sdp[order], duration_override=durs[order], utt_ids=order.astype(np.int64))
    eng.batch_run(2, 1.05, 5)
    ref, _ = eng.batch_fetch_pcm16()
    assert np.array_equal(pcm[order][:, : ref.shape[1]], ref)
    eng.set_compressor(None)
    assert not np.array_equal(eng.batch_fetch_pcm16()[0], ref)
    with pytest.raises(binding.StnError) as ei:
        g.set_compressor((-24.0, 30.0, 6.0, 5.0, 120.0, 0.0))
    assert "ratio" in str(ei.value)
    g.set_compressor(None)
    g.close()
    eng.close()


# ---- 6. the hosts ---------------------------------------------------------------------------------------------------------------------------------
TEXT = "The engine compresses every utterance on the device before it measures anything."
LOW = {"threshold_db": -40.0, "ratio": 8.0, "makeup_db": 3.0}  # (low enough for what synthetic weights produce)
LOW6 = (-40.0, 8.0) + SPEECH[2:5] + (3.0,)


def _tts(**kw):
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    from supertonic_amd.tts import Style, load_text_to_speech
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, **kw)
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    return tts, Style(sttl, sdp)


def test_python_host_applies_the_compressor_per_instance_and_per_call():
    tts, style = _tts(noise_seed=21)
    plain, _ = tts.batch([TEXT], ["en"], style, 2, 1.05)
    tts.noise_seed, tts._calls = 21, 0
    got, _ = tts.batch([TEXT], ["en"], style, 2, 1.05, compressor=LOW)
    assert tts.engine.get_compressor() is None  # the call's setting went with the call
    assert _same(got, tts.engine.op_compressor(plain, tts.sample_rate, LOW6)) and not _same(got, plain)
    with pytest.raises(ValueError):
        tts.batch([TEXT], ["en"], style, 2, 1.05, compressor={"threshold": -20})
    with pytest.raises(binding.StnError):
        tts.batch([TEXT], ["en"], style, 2, 1.05, compressor={"ratio": 40})
    assert tts.engine.get_compressor() is None
    tts.engine.close()
    tts, style = _tts(noise_seed=21, output_rate=8000, compressor=LOW)
    assert tts.engine.get_compressor() == _f32(LOW6) and tts.settings.compressor == LOW6
    on, _ = tts.batch([TEXT], ["en"], style, 2, 1.05, encoding="mulaw")
    tts.noise_seed, tts._calls = 21, 0
    off, _ = tts.batch([TEXT], ["en"], style, 2, 1.05, compressor=False)
    assert tts.engine.get_compressor() == _f32(LOW6)  # the instance's setting is back
    assert _same(on, g711_ref.encode(binding.ENC_MULAW, tts.engine.op_compressor(off, 8000, LOW6)))
    tts.engine.close()


def test_cli_compressor_writes_the_bytes_the_binding_produces(tmp_path):
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    from supertonic_amd.tts import Style, load_text_to_speech
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    (tmp_path / "voice.json").write_text(json.dumps({"style_ttl": {"data": sttl.astype(np.float64).tolist(), "dims": list(sttl.shape)},
                                                     "style_dp": {"data": sdp.astype(np.float64).tolist(), "dims": list(sdp.shape)}}))
    args = ["--synthetic", "--text", TEXT, "--n-test", "1", "--seed", "3", "--total-step", "2", "--voice-style", "voice.json", "--save-dir", "out",
            "--sample-rate", "8000", "--encoding", "mulaw", "--compressor", "-40:8:6:5:120:3"]
    p = subprocess.run([CLI] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    (f,) = os.listdir(tmp_path / "out")
    b = open(tmp_path / "out" / f, "rb").read()
    at = b.index(b"data")
    size = struct.unpack("<I", b[at + 4: at + 8])[0]
    data = np.frombuffer(b[at + 8: at + 8 + size], np.uint8)
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, noise_seed=3, output_rate=8000, compressor=LOW6)
    got, dur = tts(TEXT, "en", Style(sttl, sdp), 2, 1.05, 0.3, encoding="mulaw")
    tts.noise_seed, tts._calls = 3, 0
    off, _ = tts(TEXT, "en", Style(sttl, sdp), 2, 1.05, 0.3, encoding="mulaw", compressor=False)
    tts.engine.close()
    n = min(data.size, got.shape[1])
    assert n > 1000 and abs(data.size - int(8000 * float(dur[0]))) <= 1 and np.array_equal(data[:n], got[0, :n]) and not np.array_equal(got, off)
    # a value outside the limits is refused with the field named; so is a malformed spelling
    p = subprocess.run([CLI] + args[:-1] + ["-40:30"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "ratio" in p.stdout + p.stderr
    p = subprocess.run([CLI] + args[:-1] + ["-40"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "THRESHOLD:RATIO" in p.stdout + p.stderr


def test_service_compressor_round_trip_and_unlike_settings_are_not_merged():
    from fastapi.testclient import TestClient
    from supertonic_amd import service
    tts, style = _tts(noise_seed=5)
    b = service.DynamicBatcher(tts, max_batch=16, max_wait_ms=400.0)
    texts = ["Hello there, this is the first request.", "And this one is the second request, a bit longer."]
    out = {}

    def go(i, c):
        out[i] = b.submit([texts[i % 2]], "en", style, 2, 1.05, compressor=c)

    th = [threading.Thread(target=go, args=(i, c)) for i, c in enumerate((True, SPEECH, None, LOW))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert sorted(b.batches) == [1, 1, 2]  # the two like requests (True is the speech default) shared a batch; the two others ran apart
    assert tts.engine.get_compressor() is None and all(out[i][0][0].size > 1000 for i in range(4))
    with pytest.raises(ValueError) as ei:
        b.submit([texts[0]], "en", style, 2, 1.05, compressor={"knee_db": 30})
    assert "knee_db" in str(ei.value)
    b.close()
    # the HTTP field: validated, handed to the engine for the request, gone after it
    app = service.create_app(tts, max_batch=8, max_wait_ms=1.0, style_loader=lambda paths: style)
    with TestClient(app) as c:
        for body in (True, LOW):
            r = c.post("/tts", json={"text": texts[0], "compressor": body, "filter_preset": "telephone", "sample_rate": 8000, "encoding": "mulaw"})
            assert r.status_code == 200 and r.content[:4] == b"RIFF" and len(r.content) > 1000
        r = c.post("/tts", json={"text": texts[0], "compressor": {"attack_ms": 0.01}})
        assert r.status_code == 400 and "attack_ms" in r.json()["detail"]
        r = c.post("/tts", json={"text": texts[0], "compressor": {"attack": 1}})
        assert r.status_code == 400 and "attack" in r.json()["detail"]
    assert tts.engine.get_compressor() is None and tts.engine.output_rate == tts.sample_rate
    tts.engine.close()


# ---- 7. cost -----------------------------------------------------------------------------------------------------------------------------------------
def test_timing_report_c3_compressor():
    """Event-timed cost on a C3-sized batch (128 rows) at the native rate, over 10 fetches after a warm one: the compressor's five
    launches and its row maxima, beside the loudness measurement's four launches (the yardstick: the same reads of the same rows) in the
    same process and run.  Printed, not asserted; DESIGN.md section 20 records the values."""
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
    lo = timed(lambda: e.batch_loudness())
    yard = sum(us * n / 10 for k, (us, n) in lo.items() if k == "out.loudness")  # (chunk, scan, energy and the gate: one family)
    print(f"\nC3 batch, {B} x {W} samples at {a.sample_rate} Hz: " + ", ".join(f"{k} {us:.1f} us x {n // 10}" for k, (us, n) in sorted(lo.items()))
          + f"; the loudness measurement's launches together {yard:.1f} us")
    for name, setting in (("speech", SPEECH), ("3 s release", (-30.0, 8.0, 12.0, 0.1, 3000.0, 0.0))):
        e.set_compressor(setting)
        t = timed(lambda: (e.batch_copy_wav_device(dst.ptr, W), e.sync()))
        assert all(t[k][1] == 10 for k in FAMILIES), t
        five = sum(t[k][0] for k in FAMILIES[:5])
        print(f"{name}: " + ", ".join(f"{k} {us:.1f} us" for k, (us, n) in sorted(t.items()))
              + f"; the five launches {five:.1f} us, {five / yard:.2f} x the loudness measurement")
    e.set_compressor(None)
    e.close()
