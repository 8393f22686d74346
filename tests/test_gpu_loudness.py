"""Loudness normalization on an MI355X (include/stn.h, stn_set_loudness / stn_batch_loudness / stn_op_loudness; kernels_loudness.hip):
the op against a float64 BS.1770-4 (tests/loudness_ref.py) at six rates, every fetch path with normalization on against the gain
applied to the fetch without it, the peak ceiling, the off path byte for byte with no extra launch, captured graphs kept across
toggles, position independence of a length-aware batch's rows, the group, the CLI, the C++ host's long form and the Python host.
Prints the event-timed cost of measure + PCM gain for a C3-sized batch (128 utterances) at 44.1 kHz and with resampling to 16 kHz."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding, host, workload
from supertonic_amd.arch import default_arch, tiny_arch
from gpu_util import make_inputs
from loudness_ref import hop, integrated_loudness, pcm_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
SR = 44100
CEIL = -1.0


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


def _signals(hz, rng):
    """rows of one call: a tone, coloured noise under an envelope with a DC offset, a quiet-then-loud row (the relative gate), a row
    shorter than one block and an all-zero row; lengths that are multiples of neither the chunk (32) nor the hop"""
    W = int(3.7 * hz) + 13
    t = np.arange(W) / hz
    tone = 0.3 * np.sin(2 * np.pi * 997 * t)
    white = rng.standard_normal(W)
    col = np.convolve(white, np.ones(9) / 3.0, mode="same")  # low-passed (coloured) noise
    env = 0.5 * (1 + np.sin(2 * np.pi * 0.7 * t)) ** 2
    noise = 0.05 * col * env + 0.02
    quiet_loud = np.where(t < 1.5, 1e-3, 0.2) * white
    short = 0.5 * white
    x = np.stack([tone, noise, quiet_loud, short, np.zeros(W)]).astype(np.float32)
    n = np.array([W, W - 1001, int(2.9 * hz) + 7, 4 * hop(hz) - 1, W], np.int64)
    return x, n


@pytest.mark.parametrize("hz", [8000, 11025, 16000, 22050, 44100, 48000, 88200, 96000, 176400, 192000])
def test_op_against_float64(eng, hz):
    rng = np.random.default_rng(hz)
    x, n = _signals(hz, rng)
    lufs, peak = eng.op_loudness(x, hz, n)
    worst = 0.0
    for r in range(x.shape[0]):
        ref = integrated_loudness(x[r, : n[r]].astype(np.float64), hz)
        assert peak[r] == np.abs(x[r, : n[r]]).max(), r  # exact: max is order-independent
        if math.isinf(ref):
            assert lufs[r] == -np.inf, (r, lufs[r])
        else:
            worst = max(worst, abs(float(lufs[r]) - ref))
            assert abs(float(lufs[r]) - ref) <= 0.01, (hz, r, lufs[r], ref)
    assert lufs[3] == -np.inf and lufs[4] == -np.inf and peak[4] == 0.0
    # whole rows (n = None), one row at a time: the same numbers as inside the call with the others
    l1, p1 = eng.op_loudness(x[1:2, : n[1]], hz)
    assert l1[0] == lufs[1] and p1[0] == peak[1]
    print(f"\n{hz} Hz: worst |dL| against float64 {worst:.2e} LU")


def test_op_refuses_bad_arguments(eng):
    x = np.zeros((1, 100), np.float32)
    for hz in (7999, 192001):
        with pytest.raises(binding.StnError):
            eng.op_loudness(x, hz)
    with pytest.raises(binding.StnError):
        eng.op_loudness(x, 16000, [101])


def _c3_like(n, seed):
    arch = default_arch()
    texts = workload.utterances(n, min_words=3, max_words=12, seed=seed)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * n)
    sttl, sdp = workload.synthetic_styles(arch, list(range(n)))
    return arch, ids, mask, sttl, sdp, workload.forced_durations(texts)


def _tiny_batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 3, 14, [14, 9, 5], seed=2)
    return a, ids, mask, sttl, sdp, np.array([0.71, 0.23, 0.52], np.float32)


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


def _spans(dur, hz, Wo):
    return [min(Wo, int(np.float32(d) * np.float32(hz))) for d in dur]


def _ceiling_bound(g, lufs, peak, target, ceil=CEIL):
    """the gain the ceiling allows is the smaller one"""
    return 10 ** (ceil / 20) / float(peak) < 10 ** ((target - float(lufs)) / 20)


@pytest.mark.parametrize("which", ["tiny", "c3"])
def test_every_fetch_path_normalized(which):
    a, ids, mask, sttl, sdp, durs = _tiny_batch() if which == "tiny" else _c3_like(128, 11)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, 9)
    target = -20.0
    normalized = 0
    for rate in (None, 16000, 48000):
        e.set_output_rate(rate)
        hz = e.output_rate
        off, dur = e.batch_fetch()
        B, _, Wo = e.batch_dims()
        lufs0, peak0, gain0 = e.batch_loudness()
        assert np.all(gain0 == 1.0)  # off: the gain the setting applies is 1
        e.set_loudness(target, CEIL)
        assert e.loudness == target and e.loudness_ceiling == CEIL
        lufs, peak, gain = e.batch_loudness()
        assert np.array_equal(lufs, lufs0) and np.array_equal(peak, peak0)  # the measurement does not depend on the setting
        wav, d = e.batch_fetch()
        assert np.array_equal(d, dur) and wav.shape == off.shape
        assert np.array_equal(wav, off * gain[:, None].astype(np.float32)), (which, rate)  # one fp32 multiply per sample
        pcm, _ = e.batch_fetch_pcm16()
        assert np.array_equal(pcm, pcm_rule(wav)), (which, rate)
        for slot in (0, 1):
            e.fetch_pcm16_begin(slot)
            got, dd = e.fetch_pcm16_end(slot)
            assert np.array_equal(got, pcm) and np.array_equal(dd, dur), slot
        w_dev, p_dev = _device_copies(e, B, Wo)
        assert np.array_equal(w_dev, wav) and np.array_equal(p_dev, pcm)
        for b, n in enumerate(_spans(dur, hz, Wo)):
            if not np.isfinite(lufs[b]):
                assert gain[b] == 1.0 and (n < 4 * hop(hz) or integrated_loudness(off[b, :n], hz) == -math.inf), b
                continue
            assert abs(float(lufs[b]) - integrated_loudness(off[b, :n].astype(np.float64), hz)) <= 0.01, b
            assert peak[b] == np.abs(off[b, :n]).max()
            L32 = integrated_loudness(wav[b, :n].astype(np.float64), hz)
            L16 = integrated_loudness(pcm[b, :n].astype(np.float64) / 32767.0, hz)
            if _ceiling_bound(gain[b], lufs[b], peak[b], target):
                assert np.abs(wav[b, :n]).max() <= 10 ** (CEIL / 20) * (1 + 1e-6) and L32 < target, b
            else:
                assert abs(L32 - target) <= 0.01 and abs(L16 - target) <= 0.05, (which, rate, b, L32, L16)
                normalized += 1
        e.set_loudness(None)
    assert normalized > 0
    e.close()


def test_ceiling_binds():
    a, ids, mask, sttl, sdp, durs = _c3_like(16, 3)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, 9)
    off, dur = e.batch_fetch()
    e.set_loudness(-6.0, -1.0)
    lufs, peak, gain = e.batch_loudness()
    wav, _ = e.batch_fetch()
    bound = 0
    for b, n in enumerate(_spans(dur, SR, off.shape[1])):
        if not np.isfinite(lufs[b]):
            continue
        assert np.abs(wav[b, :n]).max() <= 10 ** (-1 / 20) * (1 + 1e-6), b
        want = np.float32(min(10 ** ((-6.0 - float(lufs[b])) / 20), 10 ** (-1 / 20) / float(peak[b])))
        assert abs(float(gain[b]) - float(want)) <= 2e-7 * float(want), (b, gain[b], want)
        bound += _ceiling_bound(gain[b], lufs[b], peak[b], -6.0)
    assert bound > 0  # speech-like rows have a crest factor above 5 dB
    e.close()


def _launches(e, fetch):
    e.launch_log_enable(True)
    fetch()
    log = e.launch_log()
    e.launch_log_enable(False)
    return [k for _, k in log]


def test_off_is_the_native_path_and_graphs_survive_toggles():
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
    e.set_loudness(-16.0)
    assert e.graphs_cached == cached
    assert any("loudness" in k for k in _launches(e, e.batch_fetch_pcm16))
    e.batch_fetch()
    e.fetch_pcm16_begin(0)
    e.fetch_pcm16_end(0)
    e.set_loudness(-30.0, -3.0)  # a new target re-keys nothing either
    e.batch_fetch()
    e.batch_run(2, 1.05, 4)
    assert e.graph_replays == replays + 1 and e.graphs_cached == cached  # the next run is a replay
    for off in ("none", "on0"):
        if off == "none":
            e.set_loudness(None)
        else:
            e.set_loudness(-16.0)
            e._ck(e._lib.stn_set_loudness(e._h, 0, -12.0, -2.0))  # on = 0 with a target set
        assert e.loudness is None and e.graphs_cached == cached
        w, d = e.batch_fetch()
        p, _ = e.batch_fetch_pcm16()
        e.fetch_pcm16_begin(1)
        ps, _ = e.fetch_pcm16_end(1)
        assert np.array_equal(w, ref_w) and np.array_equal(d, ref_d) and np.array_equal(p, ref_p) and np.array_equal(ps, ref_p)
        ks = _launches(e, e.batch_fetch_pcm16) + _launches(e, e.batch_fetch)
        assert ks and not any("loudness" in k for k in ks), ks
    # out of range: refused with a message, the previous setting stays
    e.set_loudness(-18.0, -2.0)
    for bad in ((-61.0, -1.0), (1.0, -1.0), (-16.0, 0.5), (-16.0, -31.0), (float("nan"), -1.0)):
        with pytest.raises(binding.StnError) as ei:
            e.set_loudness(*bad)
        assert "loudness" in str(ei.value)
        assert e.loudness == -18.0 and e.loudness_ceiling == -2.0
    e.close()
    fresh.close()


@pytest.mark.parametrize("rate", [None, 16000, 88200, 192000])
def test_length_aware_rows_are_position_independent(rate):
    """vocoder mode 1: each row's L, peak and gain are those of its own span measured alone, and its normalized span is that gain
    applied to the span: bit for bit, whatever the row was batched with"""
    a, ids, mask, sttl, sdp, durs = _c3_like(24, 5)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.set_output_rate(rate)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, 3)
    off, dur = e.batch_fetch()
    hz = e.output_rate
    e.set_loudness(-20.0)
    lufs, peak, gain = e.batch_loudness()
    wav, _ = e.batch_fetch()
    finite = 0
    for b, n in enumerate(_spans(dur, hz, off.shape[1])):
        l1, p1 = e.op_loudness(off[b:b + 1, :n], hz)
        assert (l1[0] == lufs[b] or (np.isinf(l1[0]) and np.isinf(lufs[b]))) and p1[0] == peak[b], b
        assert np.array_equal(wav[b, :n], off[b, :n] * gain[b]), b
        if np.isfinite(lufs[b]):
            finite += 1
            want = min(10 ** ((-20.0 - float(lufs[b])) / 20), 10 ** (CEIL / 20) / float(peak[b]))
            assert abs(float(gain[b]) - want) <= 2e-7 * want, b
    assert finite > 0
    e.close()


@pytest.mark.parametrize("n_ranks", [1, 2])
def test_group_normalized_equals_the_engine(n_ranks):
    B = 9
    arch, ids, mask, sttl, sdp, durs = _c3_like(B, 21)
    g = binding.Group([0] * n_ranks, "bf16")
    g.load_synthetic(arch, 7)
    g.set_loudness(-20.0)
    pcm, dur = g.synthesize(ids, mask, sttl, sdp, 2, 1.05, duration_override=durs, noise_seed=5)
    lengths = mask.sum(axis=(1, 2)).astype(np.int32)
    rank_of, row_of = binding.group_deal(lengths, n_ranks)
    eng = binding.Engine(0, "bf16")
    eng.load_synthetic(arch, 7)
    eng.set_loudness(-20.0)
    for r in range(n_ranks):
        mine = np.where(rank_of == r)[0]
        order = mine[np.argsort(row_of[mine])]
        Lt = int(lengths[order].max())
        eng.batch_upload(ids[order][:, :Lt], mask[order][:, :, :Lt], sttl[order], sdp[order], duration_override=durs[order], utt_ids=order.astype(np.int64))
        eng.batch_run(2, 1.05, 5)
        ref, dref = eng.batch_fetch_pcm16()
        W = ref.shape[1]
        assert np.array_equal(pcm[order][:, :W], ref) and np.all(pcm[order][:, W:] == 0) and np.array_equal(dur[order], dref), r
        assert np.any(eng.batch_loudness()[2] != 1.0)
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


def _pcm_at_target(pcm, sr, target, ceil=CEIL, tol=0.05):
    """the file's loudness is the target, or below it with the sample peak at the ceiling"""
    L = integrated_loudness(pcm.astype(np.float64) / 32767.0, sr)
    if np.abs(pcm.astype(np.int32)).max() >= int(10 ** (ceil / 20) * 32767) - 1:
        assert L < target + tol, L
    else:
        assert abs(L - target) <= tol, L
    return L


def test_cli_loudness(tmp_path):
    common = ["--onnx-dir", "no_assets_here", "--n-test", "1", "--seed", "7", "--total-step", "2"]
    _cli(common + ["--save-dir", "plain"], tmp_path)
    _cli(common + ["--save-dir", "lo", "--loudness", "-16"], tmp_path)
    _cli(common + ["--save-dir", "lo16k", "--loudness", "-16", "--sample-rate", "16000", "--peak-ceiling", "-0.5"], tmp_path)
    (f,) = os.listdir(tmp_path / "plain")
    sr0, p0 = _wav(tmp_path / "plain" / f)
    sr1, p1 = _wav(tmp_path / "lo" / f)
    sr2, p2 = _wav(tmp_path / "lo16k" / f)
    assert sr0 == sr1 == SR and sr2 == 16000 and len(p0) == len(p1)
    assert not np.array_equal(p0, p1)
    print(f"\nCLI: plain {integrated_loudness(p0 / 32767.0, SR):.2f} LUFS -> {_pcm_at_target(p1, SR, -16.0):.2f}; "
          f"16 kHz {_pcm_at_target(p2, 16000, -16.0, ceil=-0.5):.2f}")
    p = subprocess.run([CLI, "--synthetic", "--loudness", "-70", "--n-test", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "loudness" in (p.stdout + p.stderr)


def test_host_long_form_normalizes_each_chunk(tmp_path):
    """The C++ long form: every chunk is its own row with its own gain.  The file holds each chunk's untrimmed wave (up to 70 ms past
    the measured span), so each piece between the silences is held to 0.3 LU here; the Python host below checks the spans exactly."""
    text = ("The engine synthesizes long passages by splitting them into chunks. Each chunk is synthesized on its own. "
            "The chunks are then joined with a short silence between them. This keeps the memory footprint small! "
            "Does it also keep the prosody natural? Mostly, yes. " * 3).strip()
    _cli(["--text", text, "--n-test", "1", "--save-dir", "res", "--seed", "3", "--total-step", "2", "--loudness", "-16"], tmp_path)
    (f,) = os.listdir(tmp_path / "res")
    sr, pcm = _wav(tmp_path / "res" / f)
    z = np.concatenate([[0], (pcm == 0).astype(np.int8), [0]])
    edges = np.flatnonzero(np.diff(z))
    starts, ends = edges[::2], edges[1::2]
    gaps = [(s, e) for s, e in zip(starts, ends) if e - s >= int(0.3 * sr) - 1]
    assert len(gaps) >= 1
    bounds = [0] + [x for s, e in gaps for x in (s, e)] + [len(pcm)]
    pieces = [pcm[bounds[i]:bounds[i + 1]] for i in range(0, len(bounds), 2)]
    for piece in pieces:
        _pcm_at_target(piece, sr, -16.0, tol=0.3)


def test_python_host_loudness():
    from supertonic_amd.tts import Style, load_text_to_speech
    a = default_arch()
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, noise_seed=3, loudness=-16)
    sttl, sdp = workload.synthetic_styles(a, [0])
    style = Style(sttl, sdp)
    texts = ["The quick brown fox jumps over the lazy dog.", "A second sentence, a little longer than the first one was.", "Short."]
    waves, durs = tts.solo_batch(texts, ["en"] * 3, Style(np.repeat(sttl, 3, 0), np.repeat(sdp, 3, 0)), 2)
    finite = 0
    for w, d in zip(waves, durs):
        n = min(len(w), int(np.float32(d) * np.float32(SR)))
        L = integrated_loudness(w[:n].astype(np.float64), SR)
        if np.isfinite(L):
            finite += 1
            if np.abs(w[:n]).max() < 10 ** (CEIL / 20) * (1 - 1e-6):
                assert abs(L - (-16.0)) <= 0.01, L
    assert finite > 0
    # per-call override: off for this call, then the instance's setting again
    w_off, _ = tts.solo_batch(texts[:1], ["en"], style, 2, loudness=False)
    w_on, d_on = tts.solo_batch(texts[:1], ["en"], style, 2)
    assert tts.engine.loudness == -16.0
    assert not np.array_equal(w_off[0], w_on[0])
    wav, dur = tts(" ".join(texts * 4), "en", style, 2)
    assert wav.shape[0] == 1 and np.all(np.isfinite(wav))
    tts.engine.close()


@pytest.mark.parametrize("rate", [None, 16000])
def test_timing_report_c3_loudness_pcm(rate):
    """Event-timed cost of measure + PCM gain (and the resample before them at 16 kHz) for a C3-sized batch; a generous bound only."""
    a, ids, mask, sttl, sdp, durs = _c3_like(128, 11)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(5, 1.05, 1)
    e.set_output_rate(rate)
    e.set_loudness(-16.0)
    e.batch_fetch_pcm16()  # warm: tables, scratch, lengths
    e.profile_enable(True)
    e.profile_reset()
    for _ in range(10):
        e.batch_fetch_pcm16()
    prof = e.profile()
    e.profile_enable(False)
    fams = {k: v for k, v in prof.items() if k.startswith("out.")}
    per = {k: v["ms"] * 1e3 / 10 for k, v in fams.items()}
    total = sum(per.values())
    B, L, Wo = e.batch_dims()
    print(f"\nC3 batch ({B} x {Wo} samples at {e.output_rate / 1000:g} kHz): " + ", ".join(f"{k} {v:.1f} us" for k, v in per.items())
          + f"; total {total:.1f} us per fetch")
    assert fams["out.loudness"]["launches"] == 40 and fams["out.loudness_gain"]["launches"] == 10
    assert total <= 1000.0
    e.close()
