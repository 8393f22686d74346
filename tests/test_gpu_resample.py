"""Output-rate resampling on an MI355X (include/stn.h, stn_set_output_rate / stn_op_resample; kernels_resample.hip): the op against a
float64 polyphase built from the same taps, tone accuracy, every fetch path at 16 / 24 / 48 kHz against the op applied to the native
fetch, position independence of a length-aware batch's rows, the rate-off path byte for byte with no extra launch, captured graphs
kept across a rate switch, the group, the CLI and the C++ host's long-form join.  Prints the event-timed cost of the resample + PCM
launch for a C3-sized batch (128 utterances) at 16 and 48 kHz."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding, host, workload
from supertonic_amd.arch import default_arch, tiny_arch
from gpu_util import make_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
RATES = binding.SUPPORTED_OUTPUT_RATES
SR = 44100


def _pq(in_hz, out_hz):
    g = math.gcd(in_hz, out_hz)
    return out_hz // g, in_hz // g


def ref_resample(x, in_hz, out_hz):
    """float64 polyphase from the library's own taps: y[n] = sum_j taps[(nQ) mod P][j] * x[floor(nQ/P) - (T/2 - 1) + j], 0 outside."""
    taps = binding.resample_filter(in_hz, out_hz).astype(np.float64)
    P, T = taps.shape
    _, Q = _pq(in_hz, out_hz)
    x = np.atleast_2d(np.asarray(x, np.float64))
    rows, W = x.shape
    Wo = -(-W * P // Q)
    off = T // 2 - 1
    pad = np.zeros((rows, W + 2 * T + Q + 8))
    pad[:, T:T + W] = x
    y = np.empty((rows, Wo))
    for s in range(0, Wo, 4096):
        n = np.arange(s, min(Wo, s + 4096), dtype=np.int64)
        ph, base = (n * Q) % P, (n * Q) // P - off + T
        idx = base[:, None] + np.arange(T)[None, :]
        y[:, s:s + len(n)] = np.einsum("rnt,nt->rn", pad[:, idx], taps[ph])
    return y


def pcm_rule(y):
    """writeWavFile's conversion in fp32: clamp to [-1, 1], * 32767, truncation toward zero."""
    return (np.clip(np.asarray(y, np.float32), -1.0, 1.0) * np.float32(32767.0)).astype(np.int32).astype(np.int16)


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


@pytest.mark.parametrize("out_hz", RATES)
def test_op_against_float64_polyphase(eng, out_hz):
    rng = np.random.default_rng(out_hz)
    P, Q = _pq(SR, out_hz)
    for rows, W in ((3, 1), (3, 7), (2, 4097), (2, 4099), (1, 150528)):
        x = rng.uniform(-1, 1, (rows, W)).astype(np.float32)
        y = eng.op_resample(x, SR, out_hz)
        assert y.shape == (rows, -(-W * P // Q))
        err = np.abs(y - ref_resample(x, SR, out_hz)).max()
        assert err <= 2e-6, (out_hz, W, err)
        if out_hz == SR:
            assert np.array_equal(y, x)  # the unit filter is a copy
        pcm = eng.op_resample(x, SR, out_hz, pcm=True)
        assert np.array_equal(pcm, pcm_rule(y)), (out_hz, W)  # the PCM epilogue = fp32 epilogue + the conversion


def test_op_through_the_caches_when_the_span_exceeds_lds(eng):
    """44.1 kHz -> 8001 Hz reduces to P/Q = 127/700: a workgroup's input span is above 160 KiB, so the kernel reads the row through the
    caches instead of LDS — same arithmetic, same bound."""
    x = np.random.default_rng(1).uniform(-1, 1, (2, 20011)).astype(np.float32)
    y = eng.op_resample(x, SR, 8001)
    assert np.abs(y - ref_resample(x, SR, 8001)).max() <= 2e-6


def test_refused_rates(eng):
    x = np.zeros((1, 16), np.float32)
    for bad in (44101, 7999, 192001, -16000):
        with pytest.raises(binding.StnError):
            eng.op_resample(x, SR, bad)


def _snr_db(y, ref):
    return 10 * np.log10(np.sum(ref ** 2) / np.sum((y - ref) ** 2))


@pytest.mark.parametrize("out_hz", [16000, 48000])
def test_tone_accuracy(eng, out_hz):
    n = np.arange(SR)
    x = (0.5 * np.sin(2 * np.pi * 1000 * n / SR)).astype(np.float32)
    y = eng.op_resample(x, SR, out_hz)[0].astype(np.float64)
    T = binding.resample_filter(SR, out_hz).shape[1]
    m = np.arange(len(y))
    ref = 0.5 * np.sin(2 * np.pi * 1000 * m / out_hz)
    keep = slice(T * 4, len(y) - T * 4)  # away from the ends (the row is zero-extended there)
    snr = _snr_db(y[keep], ref[keep])
    print(f"1 kHz tone 44.1 -> {out_hz / 1000:g} kHz: SNR {snr:.1f} dB")
    assert snr >= 80


def test_tone_above_the_output_nyquist_is_rejected(eng):
    n = np.arange(SR)
    x = (0.5 * np.sin(2 * np.pi * 10000 * n / SR)).astype(np.float32)
    y = eng.op_resample(x, SR, 16000)[0].astype(np.float64)
    T = binding.resample_filter(SR, 16000).shape[1]
    att = 20 * np.log10(np.sqrt(np.mean(y[T * 4:-T * 4] ** 2)) / np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    print(f"10 kHz tone 44.1 -> 16 kHz: {att:.1f} dB")
    assert att <= -80


def _c3_like(n, seed):
    arch = default_arch()
    texts = workload.utterances(n, min_words=3, max_words=12, seed=seed)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * n)
    sttl, sdp = workload.synthetic_styles(arch, list(range(n)))
    return arch, ids, mask, sttl, sdp, workload.forced_durations(texts)


def _tiny_batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 3, 14, [14, 9, 5], seed=2)
    return a, ids, mask, sttl, sdp, np.array([0.41, 0.23, 0.12], np.float32)


def _device_copies(e, B, Wo):
    """copy_wav_device / copy_pcm16_device into device buffers with row strides that are not multiples of 8; the padding is untouched"""
    from hip_util import DeviceBuffer
    sw, sp = Wo + 1, Wo + 3
    dw = DeviceBuffer(np.full((B, sw), -7.0, np.float32))
    dp = DeviceBuffer(np.full((B, sp), -7, np.int16))
    e.batch_copy_wav_device(dw.ptr, sw)
    e.batch_copy_pcm16_device(dp.ptr, sp)
    e.sync()
    w, p = dw.to_host(), dp.to_host()
    assert np.all(w[:, Wo:] == -7.0) and np.all(p[:, Wo:] == -7)
    return w[:, :Wo], p[:, :Wo]


@pytest.mark.parametrize("which", ["tiny", "c3"])
def test_every_fetch_path_at_the_output_rate(which):
    if which == "tiny":
        a, ids, mask, sttl, sdp, durs = _tiny_batch()
        e = binding.Engine(0, "bf16")
        e.load_synthetic(a, 7)
    else:
        a, ids, mask, sttl, sdp, durs = _c3_like(128, 11)
        e = binding.Engine(0, "bf16")
        e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, 9)
    native, dur0 = e.batch_fetch()
    B, L, W = e.batch_dims()
    assert W == L * a.chunk_size and e.output_rate == SR
    for out_hz in (16000, 24000, 48000) + ((176400, 192000) if which == "tiny" else ()):
        P, Q = _pq(SR, out_hz)
        e.set_output_rate(out_hz)
        assert e.output_rate == out_hz
        Bd, Ld, Wo = e.batch_dims()
        assert (Bd, Ld) == (B, L) and Wo == -(-W * P // Q)
        wav, dur = e.batch_fetch()
        assert wav.shape == (B, Wo) and np.array_equal(dur, dur0)
        assert np.array_equal(wav, e.op_resample(native, SR, out_hz)), out_hz  # bit for bit
        pcm, dur = e.batch_fetch_pcm16()
        assert np.array_equal(pcm, pcm_rule(wav)) and np.array_equal(dur, dur0)
        for slot in (0, 1):
            e.fetch_pcm16_begin(slot)
            got, d = e.fetch_pcm16_end(slot)
            assert np.array_equal(got, pcm) and np.array_equal(d, dur0), slot
        w_dev, p_dev = _device_copies(e, B, Wo)
        assert np.array_equal(w_dev, wav) and np.array_equal(p_dev, pcm)
        assert np.abs(pcm.astype(np.int32)).max() > 0
    e.set_output_rate(0)
    assert e.batch_dims()[2] == W and np.array_equal(e.batch_fetch()[0], native)
    e.close()


@pytest.mark.parametrize("out_hz", [16000, 24000, 48000])
def test_length_aware_rows_are_position_independent(out_hz):
    """vocoder mode 1: utterance b's first n_b = llen_b * chunk samples are its own and the rest of its row is zero, so the first
    ceil(n_b * P / Q) output samples of its row are the resampling of those n_b samples alone — whatever it was batched with."""
    a, ids, mask, sttl, sdp, durs = _c3_like(24, 5)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, 3)
    native, dur = e.batch_fetch()
    e.set_output_rate(out_hz)
    wav, _ = e.batch_fetch()
    P, Q = _pq(SR, out_hz)
    cs = a.chunk_size
    for b in range(len(dur)):
        wl = int(np.float32(dur[b]) * np.float32(SR))
        n_b = -(-wl // cs) * cs
        assert np.all(native[b, n_b:] == 0), b  # the premise: a length-aware row is zero behind its own frames
        alone = e.op_resample(native[b:b + 1, :n_b], SR, out_hz)[0]
        assert np.array_equal(wav[b, :len(alone)], alone), b
    e.close()


def _launches(e, fetch):
    e.launch_log_enable(True)
    fetch()
    log = e.launch_log()
    e.launch_log_enable(False)
    return [k for _, k in log]


def test_rate_off_is_the_native_path_and_graphs_survive_a_switch():
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    fresh = binding.Engine(0, "bf16")
    fresh.load_synthetic(a, 7)
    fresh.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    fresh.batch_run(2, 1.05, 4)
    ref_w, ref_d = fresh.batch_fetch()
    ref_p, _ = fresh.batch_fetch_pcm16()
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, 4)
    for _ in range(3):  # the second sighting captures the shape, the third replays it
        e.batch_run(2, 1.05, 4)
    cached, replays = e.graphs_cached, e.graph_replays
    assert cached >= 1 and replays >= 1
    e.batch_fetch_pcm16()  # the first native PCM fetch allocates fetch scratch, which no captured graph reads: nothing is re-keyed
    e.batch_run(2, 1.05, 4)
    assert e.graphs_cached == cached and e.graph_replays == replays + 1
    replays += 1
    e.set_output_rate(16000)
    assert e.graphs_cached == cached  # the rate is fetch-time state: no graph is dropped
    assert any("resample" in k for k in _launches(e, e.batch_fetch_pcm16))
    e.batch_fetch()
    e.fetch_pcm16_begin(0)
    e.fetch_pcm16_end(0)
    e.batch_run(2, 1.05, 4)
    assert e.graph_replays == replays + 1 and e.graphs_cached == cached  # the next run is a replay
    for hz in (0, SR):
        e.set_output_rate(hz)
        assert e.output_rate == SR and e.graphs_cached == cached
        w, d = e.batch_fetch()
        p, _ = e.batch_fetch_pcm16()
        assert np.array_equal(w, ref_w) and np.array_equal(d, ref_d) and np.array_equal(p, ref_p)
        ks = _launches(e, e.batch_fetch_pcm16)
        assert ks and not any("resample" in k for k in ks), ks
    e.close()
    fresh.close()


@pytest.mark.parametrize("n_ranks", [1, 2])
def test_group_at_16k_equals_the_engine(n_ranks):
    B = 9
    arch, ids, mask, sttl, sdp, durs = _c3_like(B, 21)
    g = binding.Group([0] * n_ranks, "bf16")
    g.load_synthetic(arch, 7)
    g.set_output_rate(16000)
    pcm, dur = g.synthesize(ids, mask, sttl, sdp, 2, 1.05, duration_override=durs, noise_seed=5)
    rows, samples = g.last_shards()
    lengths = mask.sum(axis=(1, 2)).astype(np.int32)
    rank_of, row_of = binding.group_deal(lengths, n_ranks)
    eng = binding.Engine(0, "bf16")
    eng.load_synthetic(arch, 7)
    eng.set_output_rate(16000)
    for r in range(n_ranks):
        mine = np.where(rank_of == r)[0]
        order = mine[np.argsort(row_of[mine])]
        Lt = int(lengths[order].max())
        eng.batch_upload(ids[order][:, :Lt], mask[order][:, :, :Lt], sttl[order], sdp[order], duration_override=durs[order], utt_ids=order.astype(np.int64))
        eng.batch_run(2, 1.05, 5)
        ref, dref = eng.batch_fetch_pcm16()
        W = ref.shape[1]
        assert W == samples[r] and W == -(-eng.batch_dims()[1] * arch.chunk_size * 160 // 441)
        assert np.array_equal(pcm[order][:, :W], ref) and np.all(pcm[order][:, W:] == 0) and np.array_equal(dur[order], dref), r
    eng.close()
    g.close()


def _wav(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[36:40] == b"data"
    sr = struct.unpack("<i", b[24:28])[0]
    return sr, np.frombuffer(b[44:], dtype="<i2")


def _cli(args, cwd):
    p = subprocess.run([CLI, "--synthetic"] + args, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr


def test_cli_sample_rate(tmp_path):
    common = ["--onnx-dir", "no_assets_here", "--n-test", "1", "--seed", "7", "--total-step", "2"]
    _cli(common + ["--save-dir", "native"], tmp_path)
    _cli(common + ["--save-dir", "r16", "--sample-rate", "16000"], tmp_path)
    (f,) = os.listdir(tmp_path / "native")
    sr0, pcm0 = _wav(tmp_path / "native" / f)
    sr1, pcm1 = _wav(tmp_path / "r16" / f)
    assert sr0 == SR and sr1 == 16000
    # the file holds int(sr * duration) samples of the same duration at each rate
    assert abs(len(pcm1) - len(pcm0) * 16000 / SR) <= 1.0 + 16000 / SR and np.abs(pcm1).max() > 0
    p = subprocess.run([CLI, "--synthetic", "--sample-rate", "12345", "--n-test", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "12345" in (p.stdout + p.stderr)


def test_host_long_form_joins_chunks_with_silence_at_the_output_rate(tmp_path):
    text = ("The engine synthesizes long passages by splitting them into chunks. Each chunk is synthesized on its own. "
            "The chunks are then joined with a short silence between them. This keeps the memory footprint small! "
            "Does it also keep the prosody natural? Mostly, yes. " * 3).strip()
    _cli(["--text", text, "--n-test", "1", "--save-dir", "res", "--seed", "3", "--total-step", "2", "--sample-rate", "16000"], tmp_path)
    (f,) = os.listdir(tmp_path / "res")
    sr, pcm = _wav(tmp_path / "res" / f)
    assert sr == 16000
    z = (pcm == 0).astype(np.int8)
    runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], z, [0]]))))[::2]
    assert runs.size and runs.max() >= int(0.3 * 16000) - 1


@pytest.mark.parametrize("out_hz", [16000, 48000])
def test_timing_report_c3_resample_pcm(out_hz):
    """Event-timed cost of the resample + PCM launch for a C3-sized batch (128 utterances of the default arch); reported, not asserted."""
    a, ids, mask, sttl, sdp, durs = _c3_like(128, 11)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(5, 1.05, 1)
    e.set_output_rate(out_hz)
    e.batch_fetch_pcm16()  # warm: table, scratch
    e.profile_enable(True)
    e.profile_reset()
    for _ in range(10):
        e.batch_fetch_pcm16()
    prof = e.profile()
    e.profile_enable(False)
    st = prof["out.resample_pcm16"]
    B, L, Wo = e.batch_dims()
    print(f"\nC3 batch ({B} x {L * a.chunk_size} samples at 44.1 kHz) -> {out_hz / 1000:g} kHz PCM: {st['ms'] / st['launches'] * 1e3:.1f} us per launch "
          f"({B * Wo / 1e6:.2f} M outputs, {st['flops'] / st['launches'] / 2e9:.2f} G FMA)")
    assert st["launches"] == 10
    e.close()
