"""The dithered PCM16 / PCM24 store on an MI355X (include/stn.h "dither"; store_rows_dither_kernel and the join's dithering entry points
in kernels_output.hip), bit for bit against tests/dither_ref.py: the store kernel's vector and scalar forms on
whole buffers (stn_op_encode_ex), every fetch path against the reference applied to the fp32 fetch of the same path and settings (rows
keyed by utterance id, joined programmes by their index, gaps dithered, padding the zero codeword), an utterance's bytes alone and in a
batch, settings that do not stick, the ceiling under dither, the group gather, the command line and the service."""
import os
import struct
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding, host, service, tts as tts_mod, workload
from supertonic_amd.arch import default_arch, tiny_arch
from gpu_util import make_inputs
import dither_cases as dc
import dither_ref as dr
import fetch_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
MODES = ["round", "tpdf", "tpdf-hp"]
ENCS = [binding.ENC_PCM16, binding.ENC_PCM24]
SEED = dc.SEED
UTT = np.array([5, 9, 2], np.int64)  # utterance ids of the batch of three: the noise is keyed by these, not by the row index
DURS = np.array([0.71, 0.92, 0.64], np.float32)  # (row 1, utterance 9, is the longest: alone it has the batch's row length)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _launches(e, fn):
    e.launch_log_enable(True)
    out = fn()
    log = e.launch_log()
    e.launch_log_enable(False)
    return out, [k for _, k in log]


# ---- 1. the store kernel, both forms, on whole buffers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("enc", ENCS)
def test_op_level_both_forms_bit_for_bit(eng, enc, mode):
    m = dr.MODES[mode]
    ran = {"vec": set(), "scalar": set()}
    for W in dc.WS:
        x = dc.inputs(enc, W)
        for gain in (None, dc.GAIN):
            v = x if gain is None else x * gain[:, None]  # (the kernel's fp32 product)
            want = dr.quantize_rows(enc, m, SEED, dr.ROW, dc.IDS, v)
            for stride in (W, W + 16):
                for mis in (0, 1):
                    got, ks = _launches(eng, lambda: eng.op_encode_ex(x, enc, mode, SEED, gain=gain, row_id=dc.IDS, dst_stride=stride, x_misalign=mis))
                    form = "vec" if dc.vector_form(enc, W, stride, mis) else "scalar"
                    assert ks == ["store_rows_dither_kernel" if form == "vec" else "store_rows_dither1_kernel"], (W, stride, mis, ks)  # (the log keeps names)
                    ran[form].add(W)
                    assert _same(got[:, :W], want), (W, gain is not None, stride, mis)
                    assert np.all(got.view(np.uint8).reshape(3, -1)[:, W * binding.ENCODING_BYTES[enc]:] == 0x5A)  # nothing behind a row
    assert ran["scalar"] == set(dc.WS) and ran["vec"] == {W for W in (8, 16, 48, 1040) if W % dc.VEC[enc] == 0}


def test_op_level_off_and_the_other_encodings_run_the_kernels_without_dither(eng):
    from g711_ref import encode
    x = dc.inputs(dr.PCM16, 48)
    for enc in range(5):
        want = encode(enc, x * dc.GAIN[:, None])
        for mode in ["off"] + (MODES if enc not in ENCS else []):  # a mode is accepted and without effect on f32, mu-law and A-law
            for mis in (0, 1):
                got, ks = _launches(eng, lambda: eng.op_encode_ex(x, enc, mode, SEED, gain=dc.GAIN, row_id=dc.IDS, x_misalign=mis))
                assert ks == ["store_rows_kernel"], ks
                assert _same(got, want), (enc, mode, mis)
    # without ids a row's stream is keyed by its index
    got = eng.op_encode_ex(x, "pcm16", "tpdf", SEED)
    assert _same(got, dr.quantize_rows(dr.PCM16, dr.TPDF, SEED, dr.ROW, [0, 1, 2], x))
    for bad in (dict(dither=4), dict(x_misalign=4), dict(dst_stride=47)):
        with pytest.raises((binding.StnError, ValueError)):
            eng.op_encode_ex(x, "pcm16", **{"dither": "tpdf", **bad})


# ---- 2. every fetch path ------------------------------------------------------------------------------------------------------------------
def _batch(rows=slice(None)):
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 3, 14, [9, 14, 5], seed=2)
    return a, ids[rows], mask[rows], sttl[rows], sdp[rows], DURS[rows], UTT[rows]


def _wave(a, e, hz_out=16000):
    B, L, W = e.batch_dims()
    spans = [min(W, int(np.float32(d / np.float32(1.05)) * np.float32(a.sample_rate))) for d in DURS]
    return fetch_rows.rows(a.sample_rate, W, spans, hz_out, 5.0, 11)


def _engine(rows=slice(None), wave=None):
    a, ids, mask, sttl, sdp, durs, utt = _batch(rows)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs, utt_ids=utt)
    e.batch_run(2, 1.05, 9)
    wave = _wave(a, e) if wave is None else wave
    e.dbg_batch_set_wav(wave[rows])
    return a, e, wave


def _device_copy(e, enc, rows, width, stride, copy):
    from hip_util import DeviceBuffer
    like = binding.encoded_empty(enc, rows, stride)
    d = DeviceBuffer(np.full(like.view(np.uint8).shape, 0x5A, np.uint8))
    copy(d.ptr, stride)
    e.sync()
    got = d.to_host().view(like.dtype).reshape(like.shape)
    assert np.all(got.view(np.uint8).reshape(rows, -1)[:, width * binding.ENCODING_BYTES[enc]:] == 0x5A)
    return np.ascontiguousarray(got[:, :width])


JOIN = dict(rows=[2, 1], gap_samples=[dc.GAP, dc.GAP], gap_seconds=np.array([0.01, 0.01], np.float32))
# what is set on the engine, and how the rows' dithered lengths are read (None: the whole row)
PATHS = {
    "native": dict(),
    "resample_16k": dict(output_rate=16000),
    "loudness_limiter": dict(loudness=(-16.0, -1.0), limiter=5.0),
    "filter_16k": dict(output_rate=16000, filters=[("highpass", 80)]),
    "trim": dict(trim=(40.0, 20.0, 5.0)),
    "trim_pause_loud": dict(trim=(40.0, 20.0, 5.0), pause=60.0, loudness=(-16.0, -1.0)),
}


def _apply(e, s):
    e.set_output_rate(s.get("output_rate", 0))
    e.set_filters(s.get("filters"))
    e.set_loudness(*s.get("loudness", (None,)))
    e.set_limiter(s.get("limiter"))
    e.set_silence_trim(s.get("trim"))
    e.set_pause_limit(s.get("pause"))


def _lengths(e, s):
    if "pause" in s:
        return e.batch_pauses()[0]
    if "trim" in s:
        start, end = e.batch_silence_edges()
        return end - start
    return None


@pytest.mark.parametrize("mode", MODES)
def test_every_per_row_fetch_path_is_the_reference_on_its_fp32_fetch(mode):
    a, e, _ = _engine()
    m = dr.MODES[mode]
    for name, s in PATHS.items():
        _apply(e, s)
        e.set_dither(None)
        f32, dur = e.batch_fetch()
        off = {enc: e.batch_fetch_encoded(enc)[0] for enc in range(5)}
        lens = _lengths(e, s)
        B, _, Wo = e.batch_dims()
        assert lens is None or (0 < lens.min() and lens.max() < Wo and not f32[0, lens[0]:].any())  # (trimmed rows do end inside the row)
        e.set_dither(mode, SEED)
        assert e.dither == (mode, SEED)
        assert _same(e.batch_fetch()[0], f32)
        for enc in (binding.ENC_F32, binding.ENC_MULAW, binding.ENC_ALAW):  # unaffected by any mode, byte for byte
            assert _same(e.batch_fetch_encoded(enc)[0], off[enc]), (name, enc)
        for enc in ENCS:
            want = dr.quantize_rows(enc, m, SEED, dr.ROW, UTT, f32, lengths=lens)
            assert not _same(want, off[enc])
            got, d = e.batch_fetch_encoded(enc)
            assert _same(got, want) and np.array_equal(d, dur), (name, enc, "sync")
            if enc == binding.ENC_PCM16:
                assert _same(e.batch_fetch_pcm16()[0], want), name
            for slot in (0, 1):
                e.fetch_encoded_begin(slot, enc)
            for slot in (0, 1):
                assert _same(e.fetch_encoded_end(slot)[0], want), (name, enc, slot)
            for stride in ((Wo + 15) // 16 * 16 + 16, Wo + 3):  # the store's vector and scalar forms
                got = _device_copy(e, enc, B, Wo, stride, lambda p, st: e.batch_copy_encoded_device(enc, p, st))
                assert _same(got, want), (name, enc, stride)
    e.close()


@pytest.mark.parametrize("mode", MODES)
def test_joined_fetches_key_the_programme_and_dither_the_gaps(mode):
    a, e, _ = _engine()
    m = dr.MODES[mode]
    for name, s, scope in (("plain", dict(), "row"), ("loud_row", dict(loudness=(-16.0, -1.0)), "row"), ("loud_text", dict(loudness=(-16.0, -1.0), limiter=5.0), "programme"),
                           ("trim_16k_text", dict(output_rate=16000, trim=(40.0, 20.0, 5.0), loudness=(-20.0, -1.0)), "programme")):
        _apply(e, s)
        j = dict(JOIN, gain_scope=scope)
        e.set_dither(None)
        f32, plen, pdur = e.batch_fetch_joined(cut=False, **j)
        off = {enc: e.batch_fetch_joined(cut=False, encoding=enc, **j)[0] for enc in range(5)}
        G, Wj = f32.shape
        assert G == 2 and plen.max() == Wj and plen.min() < Wj  # (programme 1 is shorter: padding behind its length)
        e.set_dither(mode, SEED)
        for enc in (binding.ENC_F32, binding.ENC_MULAW, binding.ENC_ALAW):
            assert _same(e.batch_fetch_joined(cut=False, encoding=enc, **j)[0], off[enc]), (name, enc)
        for enc in ENCS:
            want = dr.pack(enc, np.stack([dr.quantize_stream(enc, m, SEED, dr.PROG, g, f32[g], length=plen[g]) for g in range(G)]))
            got, gl, gd = e.batch_fetch_joined(cut=False, encoding=enc, **j)
            assert _same(got, want) and np.array_equal(gl, plen) and np.array_equal(gd, pdur), (name, enc)
            assert not got[1, plen[1]:].any()  # at and behind the programme's length: the zero codeword
            for slot in (0, 1):
                e.fetch_joined_begin(slot, encoding=enc, **j)
            for slot in (0, 1):
                assert _same(e.fetch_encoded_end(slot)[0], want), (name, enc, slot)
            for stride in ((Wj + 15) // 16 * 16 + 16, Wj + 3):
                got = _device_copy(e, enc, G, Wj, stride, lambda p, st: e.batch_copy_joined_device(dst_ptr=p, dst_stride=st, encoding=enc, **j))
                assert _same(got, want), (name, enc, stride)
    e.close()


def test_gaps_are_dithered():
    """between two members the fp32 fetch is exact zeros; the dithered codes there are -1, 0, 1 with about a quarter not 0"""
    a, e, wave = _engine()
    e.set_dither("tpdf", SEED)
    member = e.batch_join_dims([1, 1, 1], [0, 0, 0], np.zeros(3, np.float32))[1]  # (alone, a member is its own programme: its length)
    j = dict(rows=[3], gap_samples=[400], gap_seconds=np.array([0.01], np.float32))
    f32 = e.batch_fetch_joined(cut=False, **j)[0][0]
    got = e.batch_fetch_joined(cut=False, encoding="pcm16", **j)[0][0]
    gap = slice(int(member[0]), int(member[0]) + 400)
    assert not f32[gap].any() and set(np.unique(got[gap])) <= {-1, 0, 1} and 60 <= np.count_nonzero(got[gap]) <= 140
    assert _same(got, dr.pack(dr.PCM16, dr.quantize_stream(dr.PCM16, dr.TPDF, SEED, dr.PROG, 0, f32)))
    e.close()


# ---- 3. invariance, and settings that do not stick -----------------------------------------------------------------------------------------
def test_an_utterance_alone_gets_the_bytes_of_its_row_in_the_batch():
    a, e, wave = _engine()
    _, one, _ = _engine(slice(1, 2), wave)  # utterance 9 alone: B = 1, the same wave
    assert one.batch_dims()[0] == 1 and one.batch_dims()[2] == e.batch_dims()[2]
    for s in (PATHS["native"], PATHS["trim_pause_loud"], PATHS["resample_16k"]):
        for x in (e, one):
            _apply(x, s)
            x.set_dither("tpdf-hp", SEED)
        for enc in ENCS:
            assert _same(one.batch_fetch_encoded(enc)[0], e.batch_fetch_encoded(enc)[0][1:2]), (s, enc)
    # ... because the key is the utterance id: the same wave under another id is other noise
    a1, ids, mask, sttl, sdp, durs, _ = _batch(slice(1, 2))
    _apply(one, {})
    before = one.batch_fetch_encoded("pcm16")[0]
    one.batch_upload(ids, mask, sttl, sdp, duration_override=durs, utt_ids=np.array([10], np.int64))
    one.batch_run(2, 1.05, 9)
    one.dbg_batch_set_wav(wave[1:2])
    after = one.batch_fetch_encoded("pcm16")[0]
    assert not _same(after, before) and _same(after, dr.quantize_rows(dr.PCM16, dr.TPDF_HP, SEED, dr.ROW, [10], one.batch_fetch()[0]))
    e.close()
    one.close()


def test_settings_do_not_stick():
    a, e, wave = _engine()
    _, fresh, _ = _engine(wave=wave)
    for s in (PATHS["native"], PATHS["resample_16k"], PATHS["trim"]):
        _apply(e, s)
        _apply(fresh, s)
        fresh.batch_fetch_encoded("pcm24")  # (the edges are detected once per batch and setting: both handles have them from here)
        for hist, last in (([("tpdf", 1)], None), ([("tpdf", 1)], ("tpdf-hp", 1)), ([("tpdf-hp", 1), None], ("round", 0)), ([("tpdf", 1)], ("tpdf", 2)),
                           ([("round", 0), ("tpdf", 2)], ("tpdf", 1))):
            for h in hist:
                e.set_dither(*(h or (None,)))
                e.batch_fetch_encoded("pcm24")
            e.set_dither(*(last or (None,)))
            fresh.set_dither(*(last or (None,)))
            for enc in ENCS:
                (got, _), ks = _launches(e, lambda: e.batch_fetch_encoded(enc))
                (want, _), kf = _launches(fresh, lambda: fresh.batch_fetch_encoded(enc))
                assert _same(got, want) and ks == kf, (s, hist, last, enc)
                assert any("dither" in k for k in ks) == (last is not None), ks  # off launches the kernels without dither
    with pytest.raises(binding.StnError):
        e._ck(e._lib.stn_set_dither(e._h, 4, 0))
    assert e.dither == ("tpdf", 1)  # a refused mode leaves the setting in force
    e.close()
    fresh.close()


@pytest.mark.parametrize("enc", ENCS)
def test_ceiling_holds_within_the_dither(enc):
    """loudness -16 LUFS under a -1 dBFS ceiling with the limiter: v <= c, so q <= floor(c S + 0.5 + d) with |d| < 1: c S + 1.5 at most"""
    a, e, _ = _engine()
    _apply(e, dict(loudness=(-16.0, -1.0), limiter=5.0))
    S = dr.SCALE[enc]
    f32 = e.batch_fetch()[0]
    assert np.abs(f32).max() > 0.95 * 10 ** (-1 / 20)  # (the limiter is holding the ceiling)
    e.set_dither("tpdf", SEED)
    got = e.batch_fetch_encoded(enc)[0]
    q = got.astype(np.int64) if enc == binding.ENC_PCM16 else ((got[..., 0].astype(np.int64) | got[..., 1].astype(np.int64) << 8 | got[..., 2].astype(np.int64) << 16) ^ 0x800000) - 0x800000
    print(f"enc {enc}: max |q| {np.abs(q).max()}, ceiling {10 ** (-1 / 20) * S:.1f}")
    assert np.abs(q).max() <= int(np.floor(10 ** (-1 / 20) * S)) + 2
    e.close()


# ---- 4. the group, the command line, the service ----------------------------------------------------------------------------------------------
def _c3_like(n, seed):
    arch = default_arch()
    texts = workload.utterances(n, min_words=3, max_words=12, seed=seed)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * n)
    sttl, sdp = workload.synthetic_styles(arch, list(range(n)))
    return arch, ids, mask, sttl, sdp, workload.forced_durations(texts)


def test_group_gather_is_the_single_engines():
    B, n_ranks = 9, 3
    arch, ids, mask, sttl, sdp, durs = _c3_like(B, 21)
    g = binding.Group([0] * n_ranks, "bf16")
    g.load_synthetic(arch, 7)
    g.set_encoding("pcm16")
    g.set_dither("tpdf", SEED)
    got, dur = g.synthesize(ids, mask, sttl, sdp, 2, 1.05, duration_override=durs, noise_seed=5)
    assert got.dtype == np.int16 and got.shape[0] == B
    _, samples = g.last_shards()
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
        eng.set_dither(None)
        f32 = eng.batch_fetch()[0]
        eng.set_dither("tpdf", SEED)
        ref, dref = eng.batch_fetch_encoded("pcm16")
        W = ref.shape[1]
        assert W == samples[r]
        assert np.array_equal(got[order][:, :W], ref) and np.array_equal(dur[order], dref), r
        assert _same(ref, dr.quantize_rows(dr.PCM16, dr.TPDF, SEED, dr.ROW, order, f32)), r  # keyed by the caller's indices
        assert not got[order][:, W:].any(), r  # behind a shorter shard's rows the gather pads with the zero codeword
    eng.close()
    g.close()


def _chunks(b):
    out, off = {}, 12
    while off < len(b):
        cid, n = b[off:off + 4], struct.unpack("<I", b[off + 4:off + 8])[0]
        out[cid] = b[off + 8:off + 8 + n]
        off += 8 + n + (n & 1)
    return out


def test_cli_dither_round_trip(tmp_path):
    common = ["--synthetic", "--onnx-dir", "no_assets_here", "--n-test", "1", "--seed", "7", "--total-step", "2", "--text", "A short sentence for the dither."]
    for d, more in (("f32", ["--encoding", "f32"]), ("tpdf", ["--dither", "tpdf", "--dither-seed", "5"]), ("hp24", ["--dither", "tpdf-hp", "--encoding", "pcm24"]), ("plain", [])):
        p = subprocess.run([CLI] + common + ["--save-dir", d] + more, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
    (f,) = os.listdir(tmp_path / "f32")
    data = {d: _chunks(open(tmp_path / d / f, "rb").read()) for d in ("f32", "tpdf", "hp24", "plain")}
    v = np.frombuffer(data["f32"][b"data"], "<f4")
    assert struct.unpack("<HH", data["tpdf"][b"fmt "][:4]) == (1, 1) and struct.unpack("<H", data["tpdf"][b"fmt "][14:16])[0] == 16
    got = np.frombuffer(data["tpdf"][b"data"], "<i2")
    assert got.size == v.size and np.array_equal(got, dr.pack(dr.PCM16, dr.quantize_stream(dr.PCM16, dr.TPDF, 5, dr.ROW, 0, v)))  # one row, utterance 0
    got = np.frombuffer(data["hp24"][b"data"], np.uint8).reshape(-1, 3)
    assert np.array_equal(got, dr.pack(dr.PCM24, dr.quantize_stream(dr.PCM24, dr.TPDF_HP, 0, dr.ROW, 0, v)))
    assert np.array_equal(np.frombuffer(data["plain"][b"data"], "<i2"), dr.pack(dr.PCM16, dr.quantize(dr.PCM16, dr.OFF, v, None)))  # without the flag: truncation


def test_service_and_python_host_dither_round_trip():
    from fastapi.testclient import TestClient
    t = tts_mod.load_text_to_speech("no_assets_here", use_gpu=True, dtype="bf16", noise_seed=11, allow_synthetic=True)
    assert t.settings.dither is False
    st = tts_mod.load_voice_style(["assets/voice_styles/M1.json"], synthetic_arch=t.engine.arch)

    def call(**kw):
        t.noise_seed, t._calls = 3, 0
        return t.batch(["One sentence."], ["en"], st, 2, 1.05, **kw)[0]
    w = call()
    assert _same(call(encoding="pcm16", dither=("tpdf", 4)), dr.quantize_rows(dr.PCM16, dr.TPDF, 4, dr.ROW, [0], w))
    assert _same(call(dither="tpdf"), w) and t.engine.dither is None  # floats are the same; the call's setting is gone behind it
    assert _same(call(encoding="pcm16"), dr.pack(dr.PCM16, dr.quantize(dr.PCM16, dr.OFF, w, None)))
    app = service.create_app(t, max_batch=8, max_wait_ms=5.0)
    with TestClient(app) as c:
        body = {"text": "A short request.", "lang": "en", "voice_style": "assets/voice_styles/M1.json", "total_step": 2}

        def post(**kw):
            t.noise_seed, t._calls = 5, 0
            r = c.post("/tts", json=dict(body, **kw))
            assert r.status_code == 200, r.text
            return _chunks(r.content)
        v = np.frombuffer(post(encoding="f32")[b"data"], "<f4")
        ch = post(dither="tpdf-hp", dither_seed=6)
        assert struct.unpack("<HH", ch[b"fmt "][:4]) == (1, 1) and struct.unpack("<H", ch[b"fmt "][14:16])[0] == 16
        got = np.frombuffer(ch[b"data"], "<i2")
        # one text is one joined programme of the batch's fetch: keyed as programme 0
        assert got.size == v.size and np.array_equal(got, dr.pack(dr.PCM16, dr.quantize_stream(dr.PCM16, dr.TPDF_HP, 6, dr.PROG, 0, v)))
        assert np.array_equal(np.frombuffer(post()[b"data"], "<i2"), dr.pack(dr.PCM16, dr.quantize(dr.PCM16, dr.OFF, v, None)))
    t.engine.close()
