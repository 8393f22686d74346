"""Fetch encodings on an MI355X (include/stn.h STN_ENC_*; store_rows_kernel in kernels_output.hip, the resampler's epilogue in
kernels_resample.hip, the device rules in kernels_dev.hpp): the op on every int16 cell centre in the vector and the scalar form,
every fetch path byte for byte against the numpy rules applied to the fp32 / PCM16 fetch (three output rates and the native one,
loudness off and on, bf16 and f16), position independence at 8 kHz mu-law, captured graphs kept across encoding switches, one launch
for rate + mu-law, the group gather, the CLI and the service.  Prints the event-timed cost of the stores for a C3-sized batch."""
import os
import struct
import subprocess
import time

import numpy as np
import pytest

from supertonic_amd import binding, host, service, tts as tts_mod, workload
from supertonic_amd.arch import default_arch, tiny_arch
from g711_ref import alaw, encode, pcm16, pcm24, ulaw
from gpu_util import make_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
SR = 44100
ENCS = [binding.ENC_MULAW, binding.ENC_ALAW, binding.ENC_PCM24]


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


def _cells():
    """every int16 cell centre (s +- 0.5) / 32767, the cell edges' neighbours, +-1, beyond +-1 and +-0"""
    s = np.arange(1, 32768, dtype=np.float64)
    v = np.concatenate([(s + 0.5) / 32767, -(s + 0.5) / 32767, s / 32767, -s / 32767, [1.0, -1.0, 1.5, -3.0, 1e9, -1e9, 0.0, -0.0, 1e-30]])
    return v.astype(np.float32)


@pytest.mark.parametrize("enc", [binding.ENC_F32, binding.ENC_PCM16, binding.ENC_PCM24, binding.ENC_MULAW, binding.ENC_ALAW])
def test_op_encode_exhaustive(eng, enc):
    v = _cells()
    for W in (16 * 1024, 16, 32, 7, 1, 4099):  # multiples of 16: the vector form; the rest: the scalar form
        n = (v.size + W - 1) // W * W
        x = np.resize(v, n).reshape(-1, W)
        got = eng.op_encode(x, enc)
        want = encode(enc, x)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (enc, W)
    assert eng.op_encode(np.array([[0.0, -0.0]], np.float32), binding.ENC_MULAW).tolist() == [[0xFF, 0xFF]]
    with pytest.raises(binding.StnError):
        eng._ck(eng._lib.stn_op_encode(eng._h, 5, 1, 4, np.zeros(4, np.float32), np.zeros(4, np.uint8).ctypes.data))


def _tiny_batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 3, 14, [14, 9, 5], seed=2)
    return a, ids, mask, sttl, sdp, np.array([0.41, 0.23, 0.12], np.float32)


def _c3_like(n, seed):
    arch = default_arch()
    texts = workload.utterances(n, min_words=3, max_words=12, seed=seed)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * n)
    sttl, sdp = workload.synthetic_styles(arch, list(range(n)))
    return arch, ids, mask, sttl, sdp, workload.forced_durations(texts)


def _device_copy(e, enc, B, Wo, stride):
    """batch_copy_encoded_device into a device buffer of rows `stride` samples apart; the bytes past each row stay untouched"""
    from hip_util import DeviceBuffer
    like = binding.encoded_empty(enc, B, stride)
    fill = np.full(like.view(np.uint8).shape, 0x5A, np.uint8)
    d = DeviceBuffer(fill)
    e.batch_copy_encoded_device(enc, d.ptr, stride)
    e.sync()
    got = d.to_host().view(like.dtype).reshape(like.shape)
    assert np.all(got.view(np.uint8).reshape(B, -1)[:, Wo * binding.ENCODING_BYTES[enc]:] == 0x5A)
    return got[:, :Wo]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("loud", [False, True])
def test_every_fetch_path_byte_exact(dtype, loud):
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    e = binding.Engine(0, dtype)
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, 9)
    if loud:
        e.set_loudness(-20.0, -1.0)
    for hz in (0, 8000, 16000, 48000):
        e.set_output_rate(hz)
        B, _, Wo = e.batch_dims()
        wav, dur0 = e.batch_fetch()
        pcm, _ = e.batch_fetch_pcm16()
        assert np.abs(pcm.astype(np.int32)).max() > 0
        # F32 and PCM16 through the new calls are the old fetches
        f, d = e.batch_fetch_encoded("f32")
        assert _same(f, wav) and np.array_equal(d, dur0)
        p, _ = e.batch_fetch_encoded("pcm16")
        assert _same(p, pcm)
        assert _same(_device_copy(e, binding.ENC_PCM16, B, Wo, Wo + 3), pcm)
        for enc in ENCS:
            want = pcm24(wav) if enc == binding.ENC_PCM24 else (ulaw if enc == binding.ENC_MULAW else alaw)(pcm)
            got, d = e.batch_fetch_encoded(enc)
            assert _same(got, want) and np.array_equal(d, dur0), (hz, enc, "sync")
            for slot in (0, 1):
                e.fetch_encoded_begin(slot, enc)
            for slot in (0, 1):
                got, d = e.fetch_encoded_end(slot)
                assert _same(got, want) and np.array_equal(d, dur0), (hz, enc, slot)
            with pytest.raises(binding.StnError) as ex:  # a slot begun in another encoding is not a PCM16 slot
                e.fetch_pcm16_end(0)
            assert ex.value.code == -3
            wide = (Wo + 15) // 16 * 16 + 16
            for stride in (wide, Wo + 3):
                assert _same(_device_copy(e, enc, B, Wo, stride), want), (hz, enc, stride)
    e.close()


def test_length_aware_rows_are_position_independent_at_8k_mulaw():
    a, ids, mask, sttl, sdp, durs = _c3_like(24, 5)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, 3)
    native, dur = e.batch_fetch()
    e.set_output_rate(8000)
    got, _ = e.batch_fetch_encoded("mulaw")
    cs = a.chunk_size
    for b in range(len(dur)):
        wl = int(np.float32(dur[b]) * np.float32(SR))
        n_b = -(-wl // cs) * cs
        alone = ulaw(pcm16(e.op_resample(native[b:b + 1, :n_b], SR, 8000)[0]))
        assert np.array_equal(got[b, :len(alone)], alone), b
    e.close()


def _launches(e, fetch):
    e.launch_log_enable(True)
    fetch()
    log = e.launch_log()
    e.launch_log_enable(False)
    return [k for _, k in log]


def test_encoding_switches_keep_graphs_and_rate_mulaw_is_one_launch():
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    for _ in range(4):  # the second sighting captures the shape, the next ones replay it
        e.batch_run(2, 1.05, 4)
    cached, replays = e.graphs_cached, e.graph_replays
    assert cached >= 1 and replays >= 1
    ref = {enc: e.batch_fetch_encoded(enc)[0] for enc in range(5)}
    for enc in (4, 2, 3, 0, 1, 3):
        e.fetch_encoded_begin(enc % 2, enc)
        e.fetch_encoded_end(enc % 2)
        e.batch_fetch_encoded(enc)
    e.set_output_rate(8000)
    e.batch_fetch_encoded("mulaw")
    e.set_output_rate(0)
    assert e.graphs_cached == cached
    e.batch_run(2, 1.05, 4)
    assert e.graphs_cached == cached and e.graph_replays == replays + 1  # a replay: nothing was dropped or re-keyed
    for enc in range(5):
        assert _same(e.batch_fetch_encoded(enc)[0], ref[enc]), enc
    e.set_output_rate(8000)
    ks = _launches(e, lambda: e.batch_fetch_encoded("mulaw"))
    assert len(ks) == 1 and "resample" in ks[0], ks
    e.set_output_rate(0)
    ks = _launches(e, lambda: e.batch_fetch_encoded("alaw"))
    assert len(ks) == 1 and "store_rows" in ks[0], ks
    e.close()


def test_group_rehearsal_mulaw_gather():
    B, n_ranks = 9, 3
    arch, ids, mask, sttl, sdp, durs = _c3_like(B, 21)
    g = binding.Group([0] * n_ranks, "bf16")
    g.load_synthetic(arch, 7)
    g.set_output_rate(8000)
    g.set_encoding("mulaw")
    got, dur = g.synthesize(ids, mask, sttl, sdp, 2, 1.05, duration_override=durs, noise_seed=5)
    assert got.dtype == np.uint8 and got.shape[0] == B
    _, samples = g.last_shards()
    lengths = mask.sum(axis=(1, 2)).astype(np.int32)
    rank_of, row_of = binding.group_deal(lengths, n_ranks)
    eng = binding.Engine(0, "bf16")
    eng.load_synthetic(arch, 7)
    eng.set_output_rate(8000)
    padded = False
    for r in range(n_ranks):
        mine = np.where(rank_of == r)[0]
        order = mine[np.argsort(row_of[mine])]
        Lt = int(lengths[order].max())
        eng.batch_upload(ids[order][:, :Lt], mask[order][:, :, :Lt], sttl[order], sdp[order], duration_override=durs[order],
                         utt_ids=order.astype(np.int64))
        eng.batch_run(2, 1.05, 5)
        ref, dref = eng.batch_fetch_encoded("mulaw")
        W = ref.shape[1]
        assert W == samples[r]
        assert np.array_equal(got[order][:, :W], ref) and np.array_equal(dur[order], dref), r
        assert np.all(got[order][:, W:] == 0xFF), r  # padding: mu-law's zero codeword
        padded |= W < got.shape[1]
    assert padded  # (the shards differ in length: the padding was exercised)
    out = np.empty(got.shape, np.int16)
    rc = g._lib.stn_group_fetch_pcm16(g._g, out.ctypes.data, out.size, None)
    assert rc == -3  # STN_ERR_STATE: the gather was mu-law
    g.set_encoding("pcm16")
    pcm, _ = g.synthesize(ids, mask, sttl, sdp, 2, 1.05, duration_override=durs, noise_seed=5)
    assert pcm.dtype == np.int16 and np.array_equal(ulaw(pcm), got)
    eng.close()
    g.close()


def _chunks(b):
    out, off = {}, 12
    while off < len(b):
        cid, n = b[off:off + 4], struct.unpack("<I", b[off + 4:off + 8])[0]
        out[cid] = b[off + 8:off + 8 + n]
        off += 8 + n + (n & 1)
    return out


def _cli(args, cwd):
    p = subprocess.run([CLI, "--synthetic"] + args, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr


@pytest.mark.parametrize("long_form", [False, True])
def test_cli_mulaw_8k(tmp_path, long_form):
    common = ["--onnx-dir", "no_assets_here", "--n-test", "1", "--seed", "7", "--total-step", "2", "--sample-rate", "8000"]
    if long_form:
        text = ("The engine synthesizes long passages by splitting them into chunks. Each chunk is synthesized on its own. "
                "The chunks are then joined with a short silence between them. This keeps the memory footprint small! " * 3).strip()
        common += ["--text", text]
    _cli(common + ["--save-dir", "pcm"], tmp_path)
    _cli(common + ["--save-dir", "mu", "--encoding", "mulaw"], tmp_path)
    (f,) = os.listdir(tmp_path / "pcm")
    pb, mb = open(tmp_path / "pcm" / f, "rb").read(), open(tmp_path / "mu" / f, "rb").read()
    pc, mc = _chunks(pb), _chunks(mb)
    tag, _, sr = struct.unpack("<HHI", mc[b"fmt "][:8])
    assert tag == 7 and sr == 8000 and struct.unpack("<I", mc[b"fact"])[0] == len(mc[b"data"])
    pcm = np.frombuffer(pc[b"data"], "<i2")
    mu = np.frombuffer(mc[b"data"], np.uint8)
    # the default file is the PCM16 fetch sliced to the duration; the mu-law file is the mu-law fetch: the codewords of those samples
    assert mu.size == pcm.size and np.array_equal(mu, ulaw(pcm))
    if long_form:
        z = (mu == 0xFF).astype(np.int8)
        runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], z, [0]]))))[::2]
        assert runs.size and runs.max() >= int(0.3 * 8000) - 1  # the silence between chunks is the zero codeword
    p = subprocess.run([CLI, "--synthetic", "--encoding", "opus"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "opus" in (p.stdout + p.stderr)


def test_service_alaw_and_python_host():
    from fastapi.testclient import TestClient
    t = tts_mod.load_text_to_speech("no_assets_here", use_gpu=True, dtype="bf16", noise_seed=11, allow_synthetic=True)
    st = tts_mod.load_voice_style(["assets/voice_styles/M1.json"], synthetic_arch=t.engine.arch)
    # the Python host: encoded batches are the float batches' encoding
    t.noise_seed, t._calls = 3, 0
    w, d = t.batch(["One sentence.", "Two sentences here."], ["en", "en"], load_two(t), 2, 1.05)
    t.noise_seed, t._calls = 3, 0
    a, d2 = t.batch(["One sentence.", "Two sentences here."], ["en", "en"], load_two(t), 2, 1.05, encoding="alaw")
    assert a.dtype == np.uint8 and np.array_equal(a, alaw(pcm16(w))) and np.array_equal(d, d2)
    text = ("This sentence is exactly long enough to matter for the chunker, is it not? " * 10).strip()
    t.noise_seed, t._calls = 5, 0
    wf, _ = t(text, "en", st, 2, 1.05, 0.3)
    t.noise_seed, t._calls = 5, 0
    wm, _ = t(text, "en", st, 2, 1.05, 0.3, encoding="mulaw")
    assert np.array_equal(wm, ulaw(pcm16(wf)))
    app = service.create_app(t, max_batch=8, max_wait_ms=5.0)
    with TestClient(app) as c:
        body = {"text": "A short request.", "lang": "en", "voice_style": "assets/voice_styles/M1.json", "total_step": 2}
        r = c.post("/tts", json=dict(body, encoding="alaw", sample_rate=8000))
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
        ch = _chunks(r.content)
        assert struct.unpack("<HHI", ch[b"fmt "][:8]) == (6, 1, 8000) and len(ch[b"data"]) > 0
        assert struct.unpack("<I", ch[b"fact"])[0] == len(ch[b"data"])
        r16 = c.post("/tts", json=dict(body, sample_rate=8000))
        ch16 = _chunks(r16.content)
        assert struct.unpack("<H", ch16[b"fmt "][:2])[0] == 1
        assert c.post("/tts", json=dict(body, encoding="opus")).status_code == 400
        rz = c.post("/tts", json={"text": ["One.", "Two."], "lang": ["en", "en"], "voice_style": ["a.json", "b.json"], "batch": True,
                                  "encoding": "pcm24", "total_step": 2})
        import io
        import zipfile
        with zipfile.ZipFile(io.BytesIO(rz.content)) as zf:
            for name in zf.namelist():
                fc = _chunks(zf.read(name))
                assert struct.unpack("<HH", fc[b"fmt "][:4]) == (1, 1) and struct.unpack("<H", fc[b"fmt "][14:16])[0] == 24
    t.engine.close()


def load_two(t):
    return tts_mod.load_voice_style(["assets/voice_styles/M1.json", "assets/voice_styles/F1.json"], synthetic_arch=t.engine.arch)


def test_timing_report_c3_encoded_stores():
    """Event-timed cost of the encoded stores for a C3-sized batch (128 utterances of the default arch); reported, not asserted."""
    a, ids, mask, sttl, sdp, durs = _c3_like(128, 11)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(5, 1.05, 1)
    B, L, W = e.batch_dims()
    rows = []
    for label, hz, enc in (("mu-law store, 44.1 kHz", 0, "mulaw"), ("PCM24 store, 44.1 kHz", 0, "pcm24"),
                           ("PCM16 store, 44.1 kHz", 0, "pcm16"), ("8 kHz mu-law (resample epilogue)", 8000, "mulaw"),
                           ("8 kHz PCM16 (resample epilogue)", 8000, "pcm16")):
        e.set_output_rate(hz)
        e.batch_fetch_encoded(enc)  # warm: table, scratch
        e.profile_enable(True)
        e.profile_reset()
        for _ in range(10):
            e.batch_fetch_encoded(enc)
        prof = e.profile()
        e.profile_enable(False)
        (fam,) = [k for k in prof if k.startswith("out.")] or [None]
        st = prof[fam] if fam else None
        us = st["ms"] / st["launches"] * 1e3 if st else float("nan")
        rows.append((label, fam, us, st["launches"] if st else 0))
        # host to host: the whole fetch (encode + device->host copy) by wall clock
        t0 = time.perf_counter()
        for _ in range(10):
            e.batch_fetch_encoded(enc)
        rows.append((label + ", host to host", "wall", (time.perf_counter() - t0) / 10 * 1e6, 10))
    e.set_output_rate(0)
    print(f"\nC3 batch ({B} x {W} samples at 44.1 kHz):")
    for label, fam, us, n in rows:
        print(f"  {label:42s} {fam or '-':22s} {us:9.1f} us  ({n} fetches)")
    e.close()
