"""Trimming leading and trailing silence by level at fetch time on an MI355X (include/stn.h "silence trimming"; kernels_edges.hip,
join_trim_rows_kernel): the detection against the float64 rules of tests/silence_ref.py, exactly, on rows whose
margin is asserted; the trimmed store against the host slice of stn_op_encode's rows and against the float32 fade; every fetch path of
a batch whose waveform stn_dbg_batch_set_wav replaced with rows of known silences, against the slice of the untrimmed fetch; the joined
fetches; position independence; the off path; and the event-timed cost beside the store and the join on the same batch.

Why the edges may be compared exactly: the device sums a frame's squares in fp32 chunks of 32 and the chunk shares in double, so a
level is within 34 * 2^-24 relative, under 1e-5 dB, of the float64 mean at every F (tests/test_gpu_silence_kernels.py checks that bound
on every frame); a row whose frames all lie 0.01 dB or more from the threshold,
and whose loudest frame lies that far from the -70 dBFS floor, decides every frame as float64 does.  MARGIN_DB is that bound, and every
row of every input here is asserted to clear it."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
import join_ref
import silence_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
ENCS = ["f32", "pcm16", "pcm24", "mulaw", "alaw"]
ZERO = {e: binding.ZERO_CODEWORD[binding.ENCODINGS[e]] for e in ENCS}
RATES = [8000, 11025, 16000, 22050, 44100, 48000, 88200, 96000, 176400, 192000]  # frames of 80 to 1920 samples
MARGIN_DB = 0.01


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


def _same(a, b):
    """byte equality (float rows included: -0.0 and 0.0 differ)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _slices(rows_enc, start, end, zero):
    """each row's [start, end) from column 0, `zero` behind it"""
    y = np.empty_like(rows_enc)
    y[...] = zero
    for r in range(rows_enc.shape[0]):
        y[r, : int(end[r] - start[r])] = rows_enc[r, int(start[r]):int(end[r])]
    return y


# ---- 1. the detection against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", RATES)
def test_op_edges_equal_the_float64_rules(eng, hz):
    x, n = ref.speech_rows(hz, 6, 2.4, hz)
    for top_db, keep_ms in itertools.product((30.0, 40.0, 50.0), (20.0, 0.0)):
        want_s, want_e, margin = ref.batch_edges(x, n, hz, top_db, keep_ms)
        print(f"{hz} Hz, top_db {top_db}, keep {keep_ms} ms: worst margin {margin.min():.2f} dB")
        assert margin.min() >= MARGIN_DB, (hz, top_db, margin)
        got_s, got_e = eng.op_silence_edges(x, hz, n, top_db, keep_ms)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_e, want_e), (hz, top_db, keep_ms, got_s, want_s, got_e, want_e)
        assert want_s[0] == 0 and want_e[1] == n[1]  # the row without a lead, the row without a tail
    # rows of an odd width (the scalar loads), and no lengths given
    xo = np.ascontiguousarray(x[:, : x.shape[1] - 1])
    want_s, want_e, margin = ref.batch_edges(xo, None, hz, 40.0, 20.0)
    if margin.min() >= MARGIN_DB:  # (the loud padding now counts: whatever it gives, the rule is the same)
        got_s, got_e = eng.op_silence_edges(xo, hz, None, 40.0, 20.0)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_e, want_e)


def test_op_edges_without_speech(eng):
    hz = 16000
    x = np.zeros((4, 4000), np.float32)
    x[1] = 1e-4 * np.random.default_rng(0).standard_normal(4000)  # -80 dBFS: below the floor
    x[2, :1000] = 0.5
    x[3, 100:130] = 0.5  # n < F below
    n = np.array([4000, 3999, 0, 130], np.int64)
    want_s, want_e, margin = ref.batch_edges(x, n, hz, 40.0, 20.0)
    assert margin.min() >= MARGIN_DB
    got_s, got_e = eng.op_silence_edges(x, hz, n, 40.0, 20.0)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_e, want_e)
    assert got_s.tolist() == [0, 0, 0, 0] and got_e.tolist() == [4000, 3999, 0, 130]
    for kw in (dict(top_db=0.5), dict(top_db=121.0), dict(keep_ms=-1.0), dict(keep_ms=1001.0)):
        with pytest.raises(binding.StnError) as ei:
            eng.op_silence_edges(x, hz, n, **kw)
        assert ei.value.code == -1 and "must be in" in str(ei.value)
    with pytest.raises(binding.StnError):
        eng.op_silence_trim(x, hz, n, fade_ms=51.0)
    with pytest.raises(binding.StnError):
        eng.op_silence_edges(x, 7000, n)


# ---- 2. the trimmed store ----------------------------------------------------------------------------------------------------------
def _store_rows(hz):
    """speech rows plus a short burst (len < 2 Fd), a row of nothing but floor noise and an empty row; samples beyond +-1 for the clamp"""
    x, n = ref.speech_rows(hz, 4, 1.2, 7 + hz)
    x = np.concatenate([x, np.zeros((3, x.shape[1]), np.float32)])
    n = np.concatenate([n, [x.shape[1], x.shape[1] - 3, 0]]).astype(np.int64)
    F = ref.frame(hz)
    x[4, 20 * F:21 * F] = 0.4 * np.sign(np.sin(np.arange(F)))  # one frame of speech
    x[5] = 1e-5
    x[:4] *= 4.0
    x[0, 3::11] = -0.0
    return x, n


@pytest.mark.parametrize("hz", [8000, 44100])
def test_trimmed_op_without_a_fade_is_a_slice_of_the_encoded_rows(eng, hz):
    x, n = _store_rows(hz)
    g = np.array([0.5, 1.0, 1.7, 0.25, 2.0, 1.0, 3.0], np.float32)
    for keep_ms, gain in itertools.product((20.0, 0.0), (None, g)):
        want_s, want_e, margin = ref.batch_edges(x, n, hz, 40.0, keep_ms)
        assert margin.min() >= MARGIN_DB
        xg = x if gain is None else (x * gain[:, None]).astype(np.float32)  # one float32 multiply, as the store's
        for enc in ENCS:
            got, s, e = eng.op_silence_trim(x, hz, n, 40.0, keep_ms, 0.0, gain, enc)
            assert np.array_equal(s, want_s) and np.array_equal(e, want_e)
            assert _same(got, _slices(eng.op_encode(xg, enc), s, e, ZERO[enc])), (hz, keep_ms, gain is not None, enc)
    assert (want_e - want_s)[4] == ref.frame(hz) and (want_e - want_s)[6] == 0


@pytest.mark.parametrize("hz", [8000, 22050, 48000])
def test_trimmed_op_with_a_fade_equals_the_float32_reference(eng, hz):
    x, n = _store_rows(hz)
    g = np.array([0.5, 1.0, 1.7, 0.25, 2.0, 1.0, 3.0], np.float32)
    for (keep_ms, fade_ms), gain in itertools.product(((20.0, 5.0), (0.0, 50.0), (3.0, 0.4)), (None, g)):
        want, want_s, want_e, margin = ref.trim_rows(x, n, hz, 40.0, keep_ms, fade_ms, gain)
        assert margin.min() >= MARGIN_DB
        if fade_ms == 50.0:
            assert (want_e - want_s)[4] < 2 * ref.samples(hz, fade_ms)  # the burst: both fades overlap
        for enc in ENCS:
            got, s, e = eng.op_silence_trim(x, hz, n, 40.0, keep_ms, fade_ms, gain, enc)
            assert np.array_equal(s, want_s) and np.array_equal(e, want_e)
            assert _same(got, want if enc == "f32" else eng.op_encode(want, enc)), (hz, keep_ms, fade_ms, gain is not None, enc)


def test_fade_window_is_the_float64_formula_rounded():
    for hz, ms in itertools.product(RATES, (0.0, 0.4, 5.0, 50.0)):
        assert _same(binding.silence_fade_window(hz, ms), ref.fade_window(hz, ms)), (hz, ms)


# ---- 3. every fetch path ---------------------------------------------------------------------------------------------------------------
DURS = np.array([0.71, 0.43, 0.92, 0.64, 0.51, 0.47], np.float32)


def _tiny_batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 6, 14, [14, 9, 5, 12, 7, 11], seed=2)
    return a, ids, mask, sttl, sdp, DURS


def _speech_wav(a, e, seed=5, loud_padding=True):
    """model-rate rows with known silences inside each row's span: a modulated tone plus noise between a lead and a tail of floor noise
    (row 0 has no lead, row 1 no tail); loud noise from 2000 samples behind the span on (never measured; the distance keeps the
    resampler's taps from carrying it into the span), or exact zeros behind the span"""
    B, L, W = e.batch_dims()
    sr = a.sample_rate
    assert e.output_rate == sr
    rng = np.random.default_rng(seed)
    wav = np.zeros((B, W), np.float32)
    for b in range(B):
        nb = min(W, int(np.float32(DURS[b] / np.float32(1.05)) * np.float32(sr)))
        lead = 0 if b == 0 else int(rng.uniform(0.05, 0.15) * sr)
        tail = 0 if b == 1 else int(rng.uniform(0.05, 0.15) * sr)
        t = np.arange(nb) / sr
        tone = (2.0 if b == 3 else 1.0) * 0.3 * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t + b)) * np.sin(2 * np.pi * (180.0 + 40.0 * b) * t)
        row = 1e-4 * rng.standard_normal(nb)
        row[lead:nb - tail] += tone[lead:nb - tail] + 0.01 * rng.standard_normal(nb - tail - lead)
        wav[b, :nb] = row
        if loud_padding:
            wav[b, nb:] = 1e-4 * rng.standard_normal(W - nb)
            wav[b, nb + 2000:] = 0.2 * rng.standard_normal(max(0, W - nb - 2000))
    return wav


def _engine(dtype, seed=9):
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    e = binding.Engine(0, dtype)
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, seed)
    e.dbg_batch_set_wav(_speech_wav(a, e))
    return a, e


def _spans(e, dur):
    _, _, Wo = e.batch_dims()
    return np.array([max(0, min(Wo, int(np.float32(d) * np.float32(e.output_rate)))) for d in dur], np.int64)


def _expected_edges(e, trim):
    """the float64 rules on the untrimmed fp32 fetch at the current rate, before any gain"""
    lo = e.loudness
    e.set_silence_trim(None)
    e.set_loudness(None)
    x, dur = e.batch_fetch()
    e.set_loudness(lo)
    n = _spans(e, dur)
    s, en, margin = ref.batch_edges(x, n, e.output_rate, trim[0], trim[1])
    assert margin.min() >= MARGIN_DB, (e.output_rate, margin)
    return x, n, s, en


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_fetch_path_delivers_the_slice_of_the_untrimmed_fetch(dtype):
    from hip_util import DeviceBuffer
    a, e = _engine(dtype)
    trim = (40.0, 20.0, 0.0)
    checked = 0
    for rate, lo in itertools.product((None, 8000, 16000, 48000), (None, -20.0)):
        e.set_output_rate(rate)
        e.set_loudness(lo)
        _, n, s, en = _expected_edges(e, trim)
        assert s[0] == 0 and en[1] == n[1] and np.all(s[2:] > 0) and np.all(en[2:] < n[2:])
        plain = {enc: e.batch_fetch_encoded(enc) for enc in ENCS}
        e.set_silence_trim(trim)
        gs, ge = e.batch_silence_edges()
        assert np.array_equal(gs, s) and np.array_equal(ge, en), (dtype, rate, lo, gs, s, ge, en)
        B, _, Wo = e.batch_dims()
        for enc in ENCS:
            want = _slices(plain[enc][0], s, en, ZERO[enc])
            got, dur = e.batch_fetch_encoded(enc)
            assert _same(got, want), (dtype, rate, lo, enc)
            assert dur.tobytes() == plain[enc][1].tobytes()  # the durations stay the model's
            checked += 1
            if (rate, lo) in ((16000, -20.0), (None, None), (48000, None)):
                for slot in (0, 1):
                    e.fetch_encoded_begin(slot, enc)
                    s_got, s_dur = e.fetch_encoded_end(slot)
                    assert _same(s_got, want) and s_dur.tobytes() == dur.tobytes(), (slot, enc)
                for stride in (Wo + 32 - Wo % 16, Wo + 3 - Wo % 2):  # wide and aligned; odd
                    like = binding.encoded_empty(enc, B, stride)
                    like[...] = 0x5A if like.dtype == np.uint8 else -7
                    d = DeviceBuffer(like)
                    e.batch_copy_encoded_device(enc, d.ptr, stride)
                    e.sync()
                    back = d.to_host()
                    assert _same(np.ascontiguousarray(back[:, :Wo]), want) and np.all(back[:, Wo:] == like[:, Wo:]), (enc, stride)
        if lo is None:
            assert _same(e.batch_fetch()[0], _slices(plain["f32"][0], s, en, 0)) and _same(e.batch_fetch_pcm16()[0], _slices(plain["pcm16"][0], s, en, 0))
        e.set_silence_trim(None)
    assert checked == 4 * 2 * 5
    e.close()


def test_fetch_with_a_fade_equals_the_float32_reference():
    a, e = _engine("bf16")
    for rate, lo, trim in ((None, None, (40.0, 20.0, 5.0)), (16000, -20.0, (30.0, 10.0, 50.0)), (48000, -18.0, (50.0, 0.0, 2.0))):
        e.set_output_rate(rate)
        e.set_loudness(lo)
        x, n, s, en = _expected_edges(e, trim)
        g = e.batch_loudness()[2]
        e.set_silence_trim(trim)
        want = np.zeros_like(x)
        for b in range(x.shape[0]):
            seg = ref.trimmed_row(x[b], n[b], int(s[b]), int(en[b]), e.output_rate, trim[2], None if lo is None else g[b])
            want[b, : seg.size] = seg
        assert _same(e.batch_fetch()[0], want), (rate, lo, trim)
        assert e.silence_trim == trim
        for enc in ("pcm16", "mulaw", "pcm24"):
            assert _same(e.batch_fetch_encoded(enc)[0], e.op_encode(want, enc)), (rate, lo, trim, enc)
        e.set_silence_trim(None)
    e.close()


# ---- 4. joined fetches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_joined_fetch_joins_the_trimmed_rows(dtype):
    a, e = _engine(dtype)
    rows, gap_s = [2, 1, 3], [0.3, 0.25, 0.0]
    for rate, lo, trim in itertools.product((None, 16000), (None, -20.0), ((40.0, 20.0, 0.0), (40.0, 20.0, 5.0))):
        e.set_output_rate(rate)
        e.set_loudness(lo)
        hz = e.output_rate
        gap = [int(s * hz) for s in gap_s]
        _, n, s, en = _expected_edges(e, trim)
        e.set_silence_trim(trim)
        lens = en - s
        dur = (lens.astype(np.float32) / np.float32(hz)).astype(np.float32)
        p = join_ref.plan(rows, gap, gap_s, lens, dur, hz)
        for enc, mode in itertools.product(ENCS, ("whole", "trim")):
            per_row, _ = e.batch_fetch_encoded(enc)
            want = join_ref.padded(join_ref.join(per_row, lens, rows, gap, ZERO[enc]), p["W_join"], ZERO[enc])
            got, plen, pdur = e.batch_fetch_joined(rows, gap, gap_s, mode=mode, gain_scope="row", encoding=enc, cut=False)
            assert np.array_equal(plen, p["prog_len"]) and pdur.tobytes() == p["prog_dur"].tobytes(), (rate, lo, trim, mode)
            assert _same(got, want), (dtype, rate, lo, trim, enc, mode)
        wj, plen, pdur = e.batch_join_dims(rows, gap, gap_s)
        assert wj == p["W_join"] and np.array_equal(plen, p["prog_len"])
        with pytest.raises(binding.StnError):
            e.batch_fetch_joined(rows, gap, gap_s, mode=2)
        if lo is not None:  # one gain per programme: the joined, faded fp32 signal times float32(g_g)
            e.set_loudness(None)
            joined, _, _ = e.batch_fetch_joined(rows, gap, gap_s, cut=False)
            e.set_loudness(lo)
            g = e.batch_join_loudness(rows, gap, gap_s)[2]
            got, _, _ = e.batch_fetch_joined(rows, gap, gap_s, gain_scope="programme", cut=False)
            assert _same(got, (joined * g[:, None]).astype(np.float32)), (rate, trim)
        if trim[2] == 0.0 and lo is None:
            # the pause between two members' speech is the gap plus twice the keep, within one frame (the frame grid of a trimmed row
            # starts at its cut)
            F, keep = ref.frame(hz), ref.samples(hz, trim[1])
            per_row, _ = e.batch_fetch()
            a0, b0, _ = ref.batch_edges(per_row, lens, hz, trim[0], 0.0)
            i = 0
            for g_, k in enumerate(rows):
                for m in range(k - 1):
                    if en[i + m] < n[i + m] and s[i + m + 1] > 0:  # (an edge that reached the row's end kept less)
                        pause = (lens[i + m] - b0[i + m]) + gap[g_] + a0[i + m + 1]
                        assert abs(pause - (gap[g_] + 2 * keep)) <= F, (rate, g_, m, pause, gap[g_], keep, F)
                i += k
        e.set_silence_trim(None)
    e.close()


# ---- 5. position independence ----------------------------------------------------------------------------------------------------------
def test_a_rows_edges_and_bytes_do_not_depend_on_the_batch():
    a, e = _engine("bf16")
    wav = _speech_wav(a, e, loud_padding=False)  # (zeros behind every span: what the resampler sees there does not depend on the row's width)
    e.dbg_batch_set_wav(wav)
    trim = (40.0, 20.0, 5.0)
    ids, mask, sttl, sdp = make_inputs(a, 6, 14, [14, 9, 5, 12, 7, 11], seed=2)
    for rate in (None, 16000):
        e.set_output_rate(rate)
        e.set_silence_trim(trim)
        s, en = e.batch_silence_edges()
        rows, _ = e.batch_fetch_encoded("pcm16")
        for b in (1, 4):
            one = binding.Engine(0, "bf16")
            one.load_synthetic(a, 7)
            one.set_vocoder_mode(1)
            one.batch_upload(ids[b:b + 1], mask[b:b + 1], sttl[b:b + 1], sdp[b:b + 1], duration_override=DURS[b:b + 1])
            one.batch_run(2, 1.05, 9)
            _, _, W1 = one.batch_dims()
            assert W1 < wav.shape[1]
            one.dbg_batch_set_wav(wav[b:b + 1, :W1])
            one.set_output_rate(rate)
            one.set_silence_trim(trim)
            s1, e1 = one.batch_silence_edges()
            assert (s1[0], e1[0]) == (s[b], en[b]), (rate, b)
            r1, _ = one.batch_fetch_encoded("pcm16")
            k = int(en[b] - s[b])
            assert _same(r1[0, :k], rows[b, :k]) and not r1[0, k:].any() and not rows[b, k:].any()
            one.close()
    e.close()


# ---- 6. the off path -------------------------------------------------------------------------------------------------------------------
def _launches(e, fetch):
    e.profile_enable(True)
    e.launch_log_enable(True)
    fetch()
    log = e.launch_log()
    e.launch_log_enable(False)
    e.profile_enable(False)
    return log


def test_off_is_the_path_without_it_and_toggling_touches_no_graph():
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
    assert cached >= 1 and replays >= 1 and e.silence_trim is None
    for rate, lo in ((None, None), (16000, -20.0)):
        e.set_output_rate(rate)
        e.set_loudness(lo)
        for trim in ((40.0, 20.0, 5.0), (30.0, 0.0, 0.0)):  # toggling and re-targeting
            e.set_silence_trim(trim)
            e.batch_fetch_encoded("mulaw")
            e.batch_fetch_joined([6], 100, 0.1)
            fams = [f for f, _ in _launches(e, lambda: e.batch_fetch_encoded("pcm16"))]
            assert fams[-1] == "out.trim_rows" and "out.edges_frames" not in fams  # (the edges of this batch and setting are cached)
        e.set_silence_trim(None)
    for bad in ((0.5, 20.0, 5.0), (121.0, 20.0, 5.0), (40.0, -1.0, 5.0), (40.0, 1001.0, 5.0), (40.0, 20.0, 51.0)):
        rc = e._lib.stn_set_silence_trim(e._h, 1, *bad)
        assert rc == -1 and "must be in" in e.last_error()
    assert e.silence_trim is None  # the previous setting stayed in force
    assert e.graphs_cached == cached and e.graph_replays == replays
    for rate, lo in ((None, None), (16000, -20.0)):
        for x in (e, fresh):
            x.set_output_rate(rate)
            x.set_loudness(lo)
        for enc in ENCS:
            assert _same(e.batch_fetch_encoded(enc)[0], fresh.batch_fetch_encoded(enc)[0]), (rate, lo, enc)
            assert _launches(e, lambda: e.batch_fetch_encoded(enc)) == _launches(fresh, lambda: fresh.batch_fetch_encoded(enc))
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


# ---- 7. the hosts -----------------------------------------------------------------------------------------------------------------------
LONG_TEXT = ("The engine synthesizes long passages by splitting them into chunks. Each chunk is synthesized on its own. "
             "The chunks are then joined with a short silence between them. This keeps the memory footprint small! "
             "Does it also keep the prosody natural? Mostly, yes. " * 3).strip()


def _tts(**kw):
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    from supertonic_amd.tts import Style, load_text_to_speech
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, **kw)
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    return tts, Style(sttl, sdp)


def test_python_host_trims_a_long_text_and_its_rows():
    from supertonic_amd import host
    from supertonic_amd.tts import Style
    tts, style = _tts(noise_seed=21, output_rate=16000)
    chunks = host.chunk_text(LONG_TEXT, 300)
    n = len(chunks)
    assert n > 1 and tts.trim_silence is None
    got, dur = tts(LONG_TEXT, "en", style, 2, 1.05, 0.3, trim_silence=40)
    assert tts.engine.silence_trim is None  # the call's setting went with the call
    # the same chunks as rows: solo_batch cuts them at the lengths the GPU found, and their host join is the joined fetch
    tts.noise_seed, tts._calls = 21, 0
    rep = Style(np.repeat(style.ttl, n, axis=0), np.repeat(style.dp, n, axis=0))
    waves, _ = tts.solo_batch(chunks, ["en"] * n, rep, 2, 1.05, trim_silence=40)
    tts.engine.set_silence_trim(40)  # (the batch is still resident: its edges under the call's parameters)
    start, end = tts.engine.batch_silence_edges()
    tts.engine.set_silence_trim(None)
    assert [len(w) for w in waves] == (end - start).tolist()
    gap = np.zeros(int(0.3 * 16000), np.float32)
    want = np.concatenate([p for i, w in enumerate(waves) for p in ((gap, w) if i else (w,))])
    assert got.shape == (1, want.size) and _same(got[0], want)
    d = np.float32(0)
    for i, w in enumerate(waves):
        seg = np.float32(len(w)) / np.float32(16000)
        d = seg if i == 0 else np.float32(d + np.float32(seg + np.float32(0.3)))
    assert float(dur[0]) == float(d)
    # an instance-wide setting; batch() rows hold the segment from column 0
    tts.engine.close()
    tts, style = _tts(noise_seed=21, trim_silence=(40, 10, 0))
    assert tts.engine.silence_trim == (40.0, 10.0, 0.0)
    wav, _, seg = tts.batch([chunks[0]], ["en"], style, 2, 1.05, lengths=True)
    assert seg.shape == (1,) and 0 < seg[0] <= wav.shape[1] and not wav[0, int(seg[0]):].any()
    with pytest.raises(ValueError):
        tts.batch([chunks[0]], ["en"], style, 2, 1.05, trim_silence=0.5)
    tts.engine.close()


def _wav(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[36:40] == b"data"
    return struct.unpack("<i", b[24:28])[0], np.frombuffer(b[44:], dtype="<i2")


def _cli(args, cwd, ok=True):
    p = subprocess.run([CLI, "--synthetic"] + args, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (p.returncode == 0) == ok, p.stdout + p.stderr
    return p.stdout + p.stderr


def test_cli_writes_files_of_the_trimmed_length(tmp_path):
    import json
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    (tmp_path / "voice.json").write_text(json.dumps({"style_ttl": {"data": sttl.astype(np.float64).tolist(), "dims": list(sttl.shape)},
                                                     "style_dp": {"data": sdp.astype(np.float64).tolist(), "dims": list(sdp.shape)}}))
    common = ["--text", LONG_TEXT, "--n-test", "1", "--seed", "3", "--total-step", "2", "--voice-style", "voice.json"]
    _cli(common + ["--save-dir", "trim", "--trim-silence", "40", "--trim-keep", "10", "--trim-fade", "0"], tmp_path)
    (f,) = os.listdir(tmp_path / "trim")
    sr, pcm = _wav(tmp_path / "trim" / f)
    # the Python host on the same seed, style and setting: the file is its joined wave, len_b samples per chunk
    from supertonic_amd.tts import Style, load_text_to_speech
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, noise_seed=3, trim_silence=(40, 10, 0))
    got, _ = tts(LONG_TEXT, "en", Style(sttl, sdp), 2, 1.05, 0.3)
    tts.engine.close()
    assert sr == 44100 and pcm.size == got.shape[1]
    assert np.array_equal(pcm, (np.clip(got[0], -1.0, 1.0) * np.float32(32767.0)).astype(np.int16))
    out = _cli(common + ["--save-dir", "no", "--trim-silence", "40", "--devices", "0,0"], tmp_path, ok=False)
    assert "silence trimming" in out  # a group is refused with a message
    out = _cli(common + ["--save-dir", "no", "--trim-silence", "0.5"], tmp_path, ok=False)
    assert "must be in [1, 120]" in out


def test_service_returns_trimmed_waves_and_keeps_unlike_settings_apart():
    import threading
    from supertonic_amd import service
    tts, style = _tts(noise_seed=5)
    b = service.DynamicBatcher(tts, max_batch=16, max_wait_ms=400.0)
    texts = ["Hello there, this is the first request.", "And this one is the second request, a bit longer."]
    out = {}

    def go(i, ts):
        out[i] = b.submit([texts[i % 2]], "en", style, 2, 1.05, silence_duration=0.3, trim_silence=ts)

    th = [threading.Thread(target=go, args=(i, ts)) for i, ts in enumerate((40, 40, None, (40, 0, 0)))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert sorted(b.batches) == [1, 1, 2]  # the two like requests shared a batch; the two others ran apart
    plain = out[2][0][0]
    for i in (0, 1, 3):
        w = out[i][0][0]
        assert 0 < w.size < plain.size * 2 and out[i][1].shape == (1,)
        assert abs(float(out[i][1][0]) - w.size / 44100.0) < 1e-4  # the duration is the segment's
    with pytest.raises(ValueError):
        b.submit([texts[0]], "en", style, 2, 1.05, silence_duration=0.3, trim_silence=121)
    b.close()
    tts.engine.close()


# ---- 8. cost ---------------------------------------------------------------------------------------------------------------------------
def test_timing_report_c3_trim():
    """Event-timed cost on a C3-sized batch (128 rows) at the native rate, over 10 fetches after a warm one: the detection (its two
    launches, re-run by alternating the keep) and the trimmed PCM16 and mu-law stores, beside out.store_rows and out.join on the same
    batch in the same process.  Printed, not asserted; DESIGN.md section 14 records the values."""
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
    rows, gap = [8] * 16, 13230

    def timed(fetch):
        fetch()  # warm: scratch, tables
        e.profile_enable(True)
        e.profile_reset()
        for _ in range(10):
            fetch()
        prof = e.profile()
        e.profile_enable(False)
        return {k: v["ms"] * 1e3 / max(v["launches"], 1) for k, v in prof.items() if k.startswith("out.")}, {k: v["launches"] for k, v in prof.items()}

    B, _, W = e.batch_dims()
    for enc in ("pcm16", "mulaw"):
        per = {}
        per.update(timed(lambda: e.batch_fetch_encoded(enc))[0])
        per.update(timed(lambda: e.batch_fetch_joined(rows, gap, 0.3, encoding=enc, cut=False))[0])
        e.set_silence_trim((40.0, 20.0, 5.0))
        t, launches = timed(lambda: e.batch_fetch_encoded(enc))
        assert launches.get("out.trim_rows") == 10 and "out.edges_frames" not in launches, launches
        per.update(t)
        flip = [0]

        def redetect():
            flip[0] ^= 1
            e.set_silence_trim((40.0, 20.0 + flip[0], 5.0))
            e.batch_fetch_encoded(enc)

        t, launches = timed(redetect)
        assert launches.get("out.edges_frames") == 10 and launches.get("out.edges_rows") == 10, launches
        per.update({k: v for k, v in t.items() if k.startswith("out.edges")})
        e.set_silence_trim(None)
        print(f"\nC3 batch, {enc}, {B} x {W} samples: " + ", ".join(f"{k} {v:.1f} us" for k, v in sorted(per.items())))
    e.close()
