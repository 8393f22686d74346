"""The formant-preserving pitch mode through the engine on an MI355X (include/stn.h "formant"; engine_formant.cpp; DESIGN.md section
26): planted rows (stn_dbg_batch_set_wav) fetched under pitch +4 in mode "formant" against the op-level correction of the rows fetched
with pitch off and under pitch +4 in mode "resample"; stn_op_pitch_ex against the composition; the mode with pitch 0 against a fresh
handle; a walk of the mode under silence trimming; the group; and what the correction is for, on the device's own shift."""
import os
import struct
import subprocess

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import default_arch, tiny_arch
from gpu_util import make_inputs
import fetch_rows
import formant_cases as fc
import pitch_cases as pc
import pitch_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
UTT = np.array([5, 9, 2, 7], np.int64)
DURS = np.array([0.71, 0.92, 0.64, 0.80], np.float32)
JOIN = dict(rows=[3, 1], gap_samples=[100, 100], gap_seconds=np.array([0.01, 0.01], np.float32))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _launches(e, fn):
    e.launch_log_enable(True)
    out = fn()
    log = e.launch_log()
    e.launch_log_enable(False)
    return out, [k for _, k in log]


def _engine(wave=None):
    """a finished batch of four rows with a known waveform planted"""
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 4, 14, [9, 14, 5, 11], seed=2)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=DURS, utt_ids=UTT)
    e.batch_run(2, 1.05, 9)
    B, L, W = e.batch_dims()
    if wave is None:
        spans = [min(W, int(np.float32(d / np.float32(1.05)) * np.float32(a.sample_rate))) for d in DURS]
        wave = fetch_rows.rows(a.sample_rate, W, spans, 16000, 5.0, 11)
    wave = np.ascontiguousarray(wave[:, :W])
    e.dbg_batch_set_wav(wave)
    return a, e, wave


def _spans(e, hz):
    W = e.batch_dims()[2]
    dur = e.batch_fetch(want_wav=False)[1]
    return np.minimum(W, (dur.astype(np.float32) * np.float32(hz)).astype(np.int64))


@pytest.fixture(scope="module")
def op():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


def test_fetch_is_the_op_level_correction_of_the_two_fetches(op):
    a, e, wave = _engine()
    n = _spans(e, a.sample_rate)
    assert e.pitch_mode == "resample"
    plain = e.batch_fetch()[0]
    e.set_pitch(4.0)
    shifted = e.batch_fetch()[0]
    want = op.op_formant(plain, shifted, a.sample_rate, n=n)
    e.set_pitch_mode("formant")
    assert e.pitch_mode == "formant"
    (got, _), ks = _launches(e, lambda: e.batch_fetch())
    assert _same(got, want) and not _same(got, shifted) and not _same(got, plain)
    assert [k for k in ks if "formant" in k][0] == "formant_lpc_kernel" and sum("formant_filter_kernel" in k for k in ks) == 1, ks
    assert [k for k in ks if "pitch" in k] == ["pitch_search_kernel", "pitch_ola_kernel"], ks
    (again, _), ks = _launches(e, lambda: e.batch_fetch())
    assert _same(again, want) and not any("formant" in k or "pitch" in k for k in ks), ks  # the rows are kept per batch, shift and mode
    assert _same(e.batch_fetch_encoded("f32")[0], want)
    e.fetch_encoded_begin(0, binding.ENC_F32)
    assert _same(e.fetch_encoded_end(0)[0], want)  # _begin / _end see the corrected rows
    from hip_util import DeviceBuffer
    W = want.shape[1]
    d = DeviceBuffer(np.full((4, W + 3), -7.0, np.float32))
    e.batch_copy_wav_device(d.ptr, W + 3)  # ... and so do the device-to-device copies
    e.sync()
    back = d.to_host()
    assert _same(np.ascontiguousarray(back[:, :W]), want) and np.all(back[:, W:] == -7.0)
    e.profile_enable(True)
    e.set_pitch(-5.0)
    e.batch_fetch()
    tags = str(e.profile())
    assert all(t in tags for t in ("pitch_search", "formant_lpc", "formant_filter")), tags
    with pytest.raises(ValueError, match="pitch_mode"):
        e.set_pitch_mode("vocoder")
    with pytest.raises(binding.StnError):
        e._ck(e._lib.stn_set_pitch_mode(e._h, 2))
    assert e.pitch_mode == "formant"  # a refused value leaves the mode in force
    e.close()


@pytest.mark.parametrize("hz", (16000, 44100, 96000))
def test_op_pitch_ex_is_the_composition_bit_for_bit(op, hz):
    x, n, _ = pc.rows(hz) if hz in pc.W else pc.wide_rows(hz)
    x, n = x[:4], n[:4]
    for s in (4.0, -5.0):
        y = op.op_pitch(x, hz, s, n=n)
        assert _same(op.op_pitch(x, hz, s, n=n, mode="resample"), y)
        assert _same(op.op_pitch(x, hz, s, n=n, mode="formant"), op.op_formant(x, y, hz, n=n)), (hz, s)
    with pytest.raises(ValueError, match="pitch_mode"):
        op.op_pitch(x, hz, 4.0, mode="lpc")


def test_the_mode_without_pitch_is_a_fresh_handle():
    a, e, wave = _engine()
    _, fresh, _ = _engine(wave=wave)
    e.set_pitch(3.0)
    e.set_pitch_mode("formant")
    e.batch_fetch_encoded("pcm16")
    e.set_pitch(0)
    cached, replays = e.graphs_cached, e.graph_replays
    for enc in ("f32", "pcm16"):
        (got, _), ks = _launches(e, lambda: e.batch_fetch_encoded(enc))
        (want, _), kf = _launches(fresh, lambda: fresh.batch_fetch_encoded(enc))
        assert _same(got, want) and ks == kf and not any("formant" in k or "pitch" in k for k in ks), (enc, ks)
    assert (e.graphs_cached, e.graph_replays) == (cached, replays) and e.graphs_cached == fresh.graphs_cached
    e.close()
    fresh.close()


def test_a_walk_of_the_mode_fetches_a_fresh_handles_bytes():
    """trimming on throughout (its edges are cached per batch and setting): off, formant, resample, off; a cache that ignored the
    mode would hand the edges of other rows to the later fetches"""
    a, e, wave = _engine()
    e.set_silence_trim((40.0, 20.0, 5.0))
    e.set_loudness(-16.0, -1.0)
    seen = []
    for pitch, mode in ((None, "resample"), (4.0, "formant"), (4.0, "resample"), (None, "formant"), (None, "resample")):
        e.set_pitch(pitch)
        e.set_pitch_mode(mode)
        _, fresh, _ = _engine(wave=wave)
        fresh.set_silence_trim((40.0, 20.0, 5.0))
        fresh.set_loudness(-16.0, -1.0)
        fresh.set_pitch_mode(mode)
        fresh.set_pitch(pitch)
        for fetch in (lambda x: x.batch_fetch_encoded("pcm16")[0], lambda x: x.batch_fetch()[0], lambda x: x.batch_fetch_joined(cut=False, encoding="pcm16", **JOIN)[0]):
            assert _same(fetch(e), fetch(fresh)), (pitch, mode)
        assert np.array_equal(np.stack(e.batch_silence_edges()), np.stack(fresh.batch_silence_edges())), (pitch, mode)
        seen.append(e.batch_fetch()[0])
        fresh.close()
    assert _same(seen[0], seen[3]) and _same(seen[0], seen[4]) and not _same(seen[1], seen[2]) and not _same(seen[1], seen[0])
    e.close()


def test_a_group_of_one_forwards_the_mode():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 2, 12, [12, 8], seed=3)
    durs = np.array([0.6, 0.5], np.float32)
    out = {}
    for mode in ("resample", "formant"):
        g = binding.Group([0], "bf16")
        g.load_synthetic(a, 7)
        g.set_encoding("pcm16")
        g.set_pitch(4.0)
        g.set_pitch_mode(mode)
        out[mode] = g.synthesize(ids, mask, sttl, sdp, 2, 1.05, duration_override=durs, noise_seed=5)[0]
        with pytest.raises(ValueError, match="pitch_mode"):
            g.set_pitch_mode("x")
        g.close()
    lengths = mask.sum(axis=(1, 2)).astype(np.int32)
    rank_of, row_of = binding.group_deal(lengths, 1)
    order = np.argsort(row_of)
    Lt = int(lengths.max())
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids[order][:, :Lt], mask[order][:, :, :Lt], sttl[order], sdp[order], duration_override=durs[order], utt_ids=order.astype(np.int64))
    e.batch_run(2, 1.05, 5)
    e.set_pitch(4.0)
    for mode in ("resample", "formant"):
        e.set_pitch_mode(mode)
        ref = e.batch_fetch_encoded("pcm16")[0]
        assert np.array_equal(out[mode][order][:, :ref.shape[1]], ref), mode
    assert not np.array_equal(out["resample"], out["formant"])
    e.close()


def _data(path):
    b = open(path, "rb").read()
    off = 12
    while off < len(b):
        cid, n = b[off:off + 4], struct.unpack("<I", b[off + 4:off + 8])[0]
        if cid == b"data":
            return np.frombuffer(b[off + 8:off + 8 + n], "<f4")
        off += 8 + n + (n & 1)
    raise AssertionError("no data chunk")


def test_cli_pitch_mode(op, tmp_path):
    common = ["--synthetic", "--onnx-dir", "no_assets_here", "--n-test", "1", "--seed", "7", "--total-step", "2", "--encoding", "f32", "--text", "A short sentence for the pitch."]
    for d, more in (("plain", []), ("mode-only", ["--pitch-mode", "formant"]), ("formant", ["--pitch", "2.5", "--pitch-mode", "formant"])):
        p = subprocess.run([CLI] + common + ["--save-dir", d] + more, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
    (f,) = os.listdir(tmp_path / "plain")
    v = {d: _data(tmp_path / d / f) for d in ("plain", "mode-only", "formant")}
    assert _same(v["plain"], v["mode-only"])  # the mode without a pitch changes nothing
    n = v["plain"].size
    want = op.op_pitch(v["plain"][None, :], default_arch().sample_rate, 2.5, mode="formant")[0]
    assert _same(v["formant"][:n], want[:n]) and not _same(v["formant"], op.op_pitch(v["plain"][None, :], default_arch().sample_rate, 2.5)[0][:n])


def test_the_envelope_comes_back_on_the_devices_own_shift(op):
    """the steady vowel at 44.1 kHz, +4 semitones, shifted and corrected on the device: the corrected row's envelope distance to the
    original is at most 0.6 of the uncorrected row's and within 0.1 dB of the float64 reference's recorded figure; the period stays"""
    hz, s = 44100, 4.0
    x = fc.property_rows(hz, s)[0]
    y = op.op_pitch(x, hz, s)[0]
    out = op.op_pitch(x, hz, s, mode="formant")[0]
    lo, hi = pc.steady(hz, len(x))
    unc = fc.fr.envelope_distance_db(x, y, hz, lo, hi)
    cor = fc.fr.envelope_distance_db(x, out, hz, lo, hi)
    print(f"{hz} Hz {s:+g}: uncorrected {unc:.3f} dB, corrected {cor:.3f} dB (reference {fc.ENVELOPE_DB[hz, s]})")
    assert cor <= 0.6 * unc
    assert abs(cor - fc.ENVELOPE_DB[hz, s][1]) <= 0.1
    assert pr.autocorr_f0(out, hz, lo, hi, 100.0, 600.0)[1] == pr.autocorr_f0(y, hz, lo, hi, 100.0, 600.0)[1]
