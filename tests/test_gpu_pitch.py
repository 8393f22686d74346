"""The fetch-time pitch shift through the engine on an MI355X (include/stn.h "pitch"; engine_pitch.cpp): planted
rows (stn_dbg_batch_set_wav) fetched with pitch on against the op-level shift of the same rows, the whole output chain behind it against
a handle whose planted rows are the shifted ones, pitch 0 against a fresh handle, histories of settings, a row alone and in a batch, the
group, the command line, the service and the Python host."""
import os
import struct
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding, host, service, tts as tts_mod, workload
from supertonic_amd.arch import default_arch, tiny_arch
from gpu_util import make_inputs
import fetch_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
UTT = np.array([5, 9, 2, 7], np.int64)
DURS = np.array([0.71, 0.92, 0.64, 0.80], np.float32)  # (row 1 is the longest: alone it has the batch's row length; row 2 alone a shorter one)
JOIN = dict(rows=[3, 1], gap_samples=[100, 100], gap_seconds=np.array([0.01, 0.01], np.float32))
CHAIN = dict(output_rate=16000, loudness=(-16.0, -1.0), limiter=5.0, dither=("tpdf", 7))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _launches(e, fn):
    e.launch_log_enable(True)
    out = fn()
    log = e.launch_log()
    e.launch_log_enable(False)
    return out, [k for _, k in log]


def _batch(rows=slice(None)):
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 4, 14, [9, 14, 5, 11], seed=2)
    return a, ids[rows], mask[rows], sttl[rows], sdp[rows], DURS[rows], UTT[rows]


def _engine(rows=slice(None), wave=None):
    """a finished batch of the rows with a known waveform planted: `wave` [rows][>= W] cut to the batch's width, or fetch_rows' rows"""
    a, ids, mask, sttl, sdp, durs, utt = _batch(rows)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs, utt_ids=utt)
    e.batch_run(2, 1.05, 9)
    B, L, W = e.batch_dims()
    if wave is None:
        spans = [min(W, int(np.float32(d / np.float32(1.05)) * np.float32(a.sample_rate))) for d in durs]
        wave = fetch_rows.rows(a.sample_rate, W, spans, 16000, 5.0, 11)
    wave = np.ascontiguousarray(wave[:, :W])
    e.dbg_batch_set_wav(wave)
    return a, e, wave


def _spans(e, hz):
    """the batch's spans at hz as the engine takes them: (int64)(reported duration * hz) in float32, at most W"""
    W = e.batch_dims()[2]
    dur = e.batch_fetch(want_wav=False)[1]
    return np.minimum(W, (dur.astype(np.float32) * np.float32(hz)).astype(np.int64))


def _apply(e, s):
    e.set_pitch(s.get("pitch"))
    e.set_output_rate(s.get("output_rate", 0))
    e.set_loudness(*s.get("loudness", (None,)))
    e.set_limiter(s.get("limiter"))
    e.set_silence_trim(s.get("trim"))
    e.set_dither(*s.get("dither", (None,)))


@pytest.fixture(scope="module")
def op():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


@pytest.fixture(scope="module")
def planted(op):
    """(the arch, the planted rows, their spans at the model's rate, {semitones: the op-level shifted rows}), computed once"""
    a, e, wave = _engine()
    n = _spans(e, a.sample_rate)
    e.close()
    assert 0 < n.min() and n.max() <= wave.shape[1]
    shifted = {s: op.op_pitch(wave, a.sample_rate, s, n=n) for s in (3.0, -4.0)}
    return a, wave, n, shifted


def test_fp32_fetch_is_the_op_level_shift_of_the_planted_rows(planted):
    a, wave, n, shifted = planted
    _, e, _ = _engine(wave=wave)
    plain = e.batch_fetch()[0]
    assert _same(plain, wave) and e.pitch == (0.0, 1, 1)
    for s, want in shifted.items():
        e.set_pitch(s)
        assert e.pitch == (s,) + binding.pitch_ratio(s)
        (got, dur), ks = _launches(e, lambda: e.batch_fetch())
        assert got.shape == wave.shape and _same(got, want) and not _same(got, wave), s
        assert [k for k in ks if "pitch" in k] == ["pitch_search_kernel", "pitch_ola_kernel"], ks  # (the log keeps names)
        assert sum("resample_kernel" in k for k in ks) == 1, ks
        (again, _), ks = _launches(e, lambda: e.batch_fetch())
        assert _same(again, want) and not any("pitch" in k for k in ks), ks  # the shifted rows are kept per batch and setting
        assert _same(e.batch_fetch_encoded("f32")[0], want)
        e.fetch_encoded_begin(0, binding.ENC_F32)
        assert _same(e.fetch_encoded_end(0)[0], want)
    with pytest.raises(ValueError, match="semitones"):
        e.set_pitch(12.5)
    with pytest.raises(binding.StnError, match="semitones"):
        e._ck(e._lib.stn_set_pitch(e._h, float("nan")))
    assert e.pitch[0] == -4.0  # a refused value leaves the setting in force
    e.close()


def test_the_whole_chain_sees_the_shifted_rows(planted):
    """pitch +3 in front of 16 kHz, loudness -16 with the limiter, pcm16 under TPDF dither: byte for byte the fetch of a handle with
    pitch off whose planted rows are the op-level shifted rows; per row, joined and trimmed"""
    a, wave, n, shifted = planted
    _, e, _ = _engine(wave=wave)
    _, f, _ = _engine(wave=shifted[3.0])
    for name, s in (("chain", CHAIN), ("trimmed", dict(CHAIN, trim=(40.0, 20.0, 5.0)))):
        _apply(e, dict(s, pitch=3.0))
        _apply(f, s)
        got, want = e.batch_fetch_encoded("pcm16"), f.batch_fetch_encoded("pcm16")
        assert _same(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        assert got[0].shape[1] == e.batch_dims()[2] and np.any(got[0])
        for scope in ("row", "programme"):
            gj = e.batch_fetch_joined(cut=False, encoding="pcm16", gain_scope=scope, **JOIN)
            wj = f.batch_fetch_joined(cut=False, encoding="pcm16", gain_scope=scope, **JOIN)
            assert _same(gj[0], wj[0]) and np.array_equal(gj[1], wj[1]) and np.array_equal(gj[2], wj[2]), (name, scope)
        if "trim" in s:
            assert np.array_equal(np.stack(e.batch_silence_edges()), np.stack(f.batch_silence_edges()))
        e.fetch_encoded_begin(1, binding.ENC_PCM16)
        assert _same(e.fetch_encoded_end(1)[0], want[0]), name
    e.close()
    f.close()


def test_pitch_zero_is_a_fresh_handle(planted):
    a, wave, n, shifted = planted
    _, e, _ = _engine(wave=wave)
    _, fresh, _ = _engine(wave=wave)
    for s in (dict(), CHAIN):
        _apply(fresh, s)
        for hist in ((), (2.0,), (2.0, -7.0)):
            _apply(e, s)
            for h in hist:
                e.set_pitch(h)
                e.batch_fetch_encoded("pcm16")
            e.set_pitch(0)
            assert e.pitch == (0.0, 1, 1)
            for enc in ("f32", "pcm16"):
                (got, _), ks = _launches(e, lambda: e.batch_fetch_encoded(enc))
                (want, _), kf = _launches(fresh, lambda: fresh.batch_fetch_encoded(enc))
                assert _same(got, want) and ks == kf and not any("pitch" in k for k in ks), (s, hist, enc, ks)
    e.profile_enable(True)
    e.batch_fetch_encoded("pcm16")
    assert not any("pitch" in str(row) for row in e.profile())
    e.set_pitch(2.0)
    e.profile_reset()
    e.batch_fetch_encoded("pcm16")
    tags = str(e.profile())
    assert all(t in tags for t in ("pitch_search", "pitch_ola", "pitch_resample")), tags
    e.close()
    fresh.close()


def test_any_history_of_pitch_settings_fetches_a_fresh_handles_bytes(planted):
    """trimming on throughout (its edges are cached per batch and setting): pitch off, on, changed, off again; a cache that ignored
    pitch would hand the edges of other rows to the later fetches"""
    a, wave, n, shifted = planted
    base = dict(trim=(40.0, 20.0, 5.0), loudness=(-16.0, -1.0))
    _, e, _ = _engine(wave=wave)
    edges = []
    for p in (None, 3.0, -4.0, None):
        s = dict(base, pitch=p)
        _apply(e, s)
        _, fresh, _ = _engine(wave=wave)
        _apply(fresh, s)
        for fetch in (lambda x: x.batch_fetch_encoded("pcm16")[0], lambda x: x.batch_fetch()[0], lambda x: x.batch_fetch_joined(cut=False, encoding="pcm16", **JOIN)[0]):
            assert _same(fetch(e), fetch(fresh)), p
        assert np.array_equal(np.stack(e.batch_silence_edges()), np.stack(fresh.batch_silence_edges())), p
        edges.append(np.stack(e.batch_silence_edges()))
        fresh.close()
    assert np.array_equal(edges[0], edges[3]) and not np.array_equal(edges[0], edges[1])  # (the shifted rows do have other edges)
    e.close()


def test_a_row_alone_and_in_a_batch_of_four(planted):
    a, wave, n, shifted = planted
    _, e, _ = _engine(wave=wave)
    for r in (1, 2):
        _, one, w1 = _engine(slice(r, r + 1), wave[r:r + 1])  # the same samples, as wide as the row's own length needs
        W1 = one.batch_dims()[2]
        assert one.batch_dims()[0] == 1 and (W1 < wave.shape[1]) == (r == 2) and n[r] <= W1
        for s in (dict(pitch=3.0), dict(CHAIN, pitch=-4.0)):
            _apply(e, s)
            _apply(one, s)
            for enc in ("f32", "pcm16"):
                g4, g1 = e.batch_fetch_encoded(enc)[0], one.batch_fetch_encoded(enc)[0]
                span = int(n[r]) * e.output_rate // a.sample_rate
                assert span > 1000 and _same(g4[r:r + 1, :span], g1[:, :span]), (r, s, enc)
        one.close()
    e.close()


def _c3_like(n, seed):
    arch = default_arch()
    texts = workload.utterances(n, min_words=3, max_words=12, seed=seed)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * n)
    sttl, sdp = workload.synthetic_styles(arch, list(range(n)))
    return arch, ids, mask, sttl, sdp, workload.forced_durations(texts)


@pytest.mark.parametrize("n_ranks", [1, 2])
def test_group_is_the_plain_handle(n_ranks):
    if n_ranks > binding.device_count():
        pytest.skip("the group over several devices needs several devices")
    B = 3
    arch, ids, mask, sttl, sdp, durs = _c3_like(B, 21)
    g = binding.Group(list(range(n_ranks)), "bf16")
    g.load_synthetic(arch, 7)
    g.set_encoding("pcm16")
    g.set_pitch(-2.0)
    got, dur = g.synthesize(ids, mask, sttl, sdp, 2, 1.05, duration_override=durs, noise_seed=5)
    lengths = mask.sum(axis=(1, 2)).astype(np.int32)
    rank_of, row_of = binding.group_deal(lengths, n_ranks)
    eng = binding.Engine(0, "bf16")
    eng.load_synthetic(arch, 7)
    for r in range(n_ranks):
        mine = np.where(rank_of == r)[0]
        order = mine[np.argsort(row_of[mine])]
        Lt = int(lengths[order].max())
        eng.batch_upload(ids[order][:, :Lt], mask[order][:, :, :Lt], sttl[order], sdp[order], duration_override=durs[order], utt_ids=order.astype(np.int64))
        eng.batch_run(2, 1.05, 5)
        eng.set_pitch(None)
        off = eng.batch_fetch_encoded("pcm16")[0]
        eng.set_pitch(-2.0)
        ref, dref = eng.batch_fetch_encoded("pcm16")
        W = ref.shape[1]
        assert np.array_equal(got[order][:, :W], ref) and np.array_equal(dur[order], dref) and not np.array_equal(ref, off), r
    with pytest.raises(ValueError, match="semitones"):
        g.set_pitch(13)
    eng.close()
    g.close()


def _chunks(b):
    out, off = {}, 12
    while off < len(b):
        cid, n = b[off:off + 4], struct.unpack("<I", b[off + 4:off + 8])[0]
        out[cid] = b[off + 8:off + 8 + n]
        off += 8 + n + (n & 1)
    return out


def test_cli_pitch(tmp_path):
    common = ["--synthetic", "--onnx-dir", "no_assets_here", "--n-test", "1", "--seed", "7", "--total-step", "2", "--encoding", "f32", "--text", "A short sentence for the pitch."]
    for d, more in (("plain", []), ("zero", ["--pitch", "0"]), ("up", ["--pitch", "2.5"])):
        p = subprocess.run([CLI] + common + ["--save-dir", d] + more, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
    (f,) = os.listdir(tmp_path / "plain")
    v = {d: np.frombuffer(_chunks(open(tmp_path / d / f, "rb").read())[b"data"], "<f4") for d in ("plain", "zero", "up")}
    assert _same(v["plain"], v["zero"]) and v["up"].shape == v["plain"].shape and not _same(v["up"], v["plain"])
    eng = binding.Engine(0, "bf16")
    n = v["plain"].size  # (the file holds the row's span)
    want = eng.op_pitch(v["plain"][None, :], default_arch().sample_rate, 2.5)[0]
    eng.close()
    # the file's samples are the span's; the engine shifted the whole row, whose samples behind the span the shift never read
    assert _same(v["up"][:n], want[:n])
    for bad in ("12.5", "nan", "high"):
        p = subprocess.run([CLI] + common + ["--save-dir", "bad", "--pitch", bad], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 1 and "semitones" in p.stderr and "[-12, 12]" in p.stderr, (bad, p.stderr)


def test_service_and_python_host_pitch():
    from fastapi.testclient import TestClient
    with pytest.raises(ValueError, match="semitones"):
        tts_mod.load_text_to_speech("no_assets_here", use_gpu=True, allow_synthetic=True, pitch=12.5)
    t = tts_mod.load_text_to_speech("no_assets_here", use_gpu=True, dtype="bf16", noise_seed=11, allow_synthetic=True)
    assert t.settings.pitch is False and t.engine.pitch == (0.0, 1, 1)
    st = tts_mod.load_voice_style(["assets/voice_styles/M1.json"], synthetic_arch=t.engine.arch)

    def call(**kw):
        t.noise_seed, t._calls = 3, 0
        return t.batch(["One sentence."], ["en"], st, 2, 1.05, **kw)
    w, dur = call()
    up, dur_up = call(pitch=-3)
    span = int(t.sample_rate * float(dur[0]))
    assert up.shape == w.shape and np.array_equal(dur, dur_up) and not _same(up, w)
    assert _same(up[:, :span], t.engine.op_pitch(w, t.sample_rate, -3, n=[span])[:, :span])
    assert t.engine.pitch == (0.0, 1, 1) and _same(call()[0], w)  # the call's setting is gone behind it
    with pytest.raises(ValueError, match="semitones"):
        call(pitch=-12.01)
    app = service.create_app(t, max_batch=8, max_wait_ms=5.0)
    with TestClient(app) as c:
        body = {"text": "A short request.", "lang": "en", "voice_style": "assets/voice_styles/M1.json", "total_step": 2, "encoding": "f32"}

        def post(**kw):
            t.noise_seed, t._calls = 5, 0
            return c.post("/tts", json=dict(body, **kw))
        r0, r1, r2 = post(), post(pitch=0), post(pitch=4)
        assert r0.status_code == r1.status_code == r2.status_code == 200, r2.text
        v0, v1, v2 = (np.frombuffer(_chunks(r.content)[b"data"], "<f4") for r in (r0, r1, r2))
        assert _same(v0, v1) and v2.shape == v0.shape and not _same(v2, v0)
        assert r0.headers["x-pitch-cents"] == "0.000" and r1.headers["x-pitch-cents"] == "0.000"
        assert r2.headers["x-pitch-cents"] == f"{binding.pitch_cents(4):.3f}" and abs(float(r2.headers["x-pitch-cents"]) - 400.0) <= 1.36
        bad = post(pitch=12.5)
        assert bad.status_code == 400 and bad.json()["detail"] == binding.pitch_error(12.5)
    t.engine.close()
