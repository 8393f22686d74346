"""The join of a fetch on an MI355X (include/stn.h "join"; join_rows_kernel, kernels_output.hip): the op against
tests/join_ref.py applied to stn_op_encode's rows, every byte; every fetch path of a length-aware batch against the host join of
batch_fetch_encoded's rows; the per-programme gain against a float64 BS.1770-4 (tests/loudness_ref.py); what the gain scope changes;
the hosts; no side effects on other fetches or on captured graphs; and the event-timed cost against the store kernel on the same batch."""
import itertools
import math
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

from supertonic_amd import binding, host, workload
from supertonic_amd.arch import default_arch, tiny_arch
from gpu_util import make_inputs
from loudness_ref import hop, integrated_loudness
import join_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
SR = 44100
ENCS = ["f32", "pcm16", "pcm24", "mulaw", "alaw"]
ZERO = {e: binding.ZERO_CODEWORD[binding.ENCODINGS[e]] for e in ENCS}


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


def _same(a, b):
    """byte equality (float rows included: -0.0 and 0.0 differ)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the op, byte-exact -------------------------------------------------------------------------------------------------------
def _op_rows(W, B, rng):
    x = (rng.standard_normal((B, W)) * 0.6).astype(np.float32)
    x[:, 1::7] *= 3.0  # beyond +-1: the clamp
    x[:, 3::11] = 0.0
    x[:, 5::13] = -0.0
    x[0, :4] = [1.0, -1.0, 1.5, -2.0]
    n = rng.integers(1, W + 1, B).astype(np.int64)
    n[n % 4 == 0] -= 1  # multiples of neither 4, 16 nor 32
    n[0] = W  # one whole row
    if B > 2:
        n[2] = 0  # an empty member
    return x, np.maximum(n, 0)


@pytest.mark.parametrize("W", [4096, 3001])
@pytest.mark.parametrize("enc", ENCS)
def test_op_is_the_host_join_of_the_encoded_rows(eng, enc, W):
    rng = np.random.default_rng(W + len(enc))
    B = 7
    x, n = _op_rows(W, B, rng)
    rows_enc = eng.op_encode(x, enc)
    for groups, gaps in itertools.product(([B], [3, 1, 3], [1] * B), (0, 1, 13230, 3)):
        G = len(groups)
        gap = [gaps] * G if G == 1 else [gaps, 3, 0, 1, 13230, 7, 2][:G]
        for mode in (join_ref.WHOLE, join_ref.TRIM):
            # the op takes the members' lengths as given; TRIM's lengths are the reference's
            dur = (n / 8000.0 * rng.uniform(0.5, 1.2, B)).astype(np.float32)
            lens = join_ref.member_lengths(n, dur, 8000, mode)
            want = join_ref.padded(join_ref.join(rows_enc, lens, groups, gap, ZERO[enc]), max(1, join_ref.plan(groups, gap, [0.0] * G, lens, dur, 8000)["W_join"]), ZERO[enc])
            got = eng.op_join(x, lens, groups, gap, 8000, encoding=enc)
            assert _same(got, want), (enc, W, groups, gap, mode, np.flatnonzero((got != want).reshape(G, -1).any(0))[:8])


@pytest.mark.parametrize("enc", ENCS)
def test_op_with_more_members_than_the_workgroup_stages(eng, enc):
    """Programmes of more than JOIN_WG = 256 members: the members past the 256 a workgroup stages in LDS are read from the table.  300
    rows of 64 samples as one programme join to 9-10 k samples, more than one tile of every encoding (8192 samples for the 8-bit ones),
    so the search runs past member 256 both in a first tile and in a later one; [257, 43] has one such member, and rows 16 bytes apart
    only by chance (the sample-by-sample store), [1] * 300 none.  Only join_rows_kernel can be driven there: the trimmed entry point's
    ops are one member per programme, and a trimmed batch join would need more than 256 chunks.  Its walk past member 256 is the same
    code (join_walk, kernels_output.hip), and is covered here only through that."""
    B, W = 300, 64
    rng = np.random.default_rng(300 + ENCS.index(enc))  # (other rows and lengths for every encoding)
    x, n = _op_rows(W, B, rng)
    rows_enc = eng.op_encode(x, enc)
    dur = np.zeros(B, np.float32)
    for groups, gaps in itertools.product(([B], [257, 43], [1] * B), (0, 1, 3)):
        G = len(groups)
        gap = [gaps] * G
        want = join_ref.padded(join_ref.join(rows_enc, n, groups, gap, ZERO[enc]), max(1, join_ref.plan(groups, gap, [0.0] * G, n, dur, 8000)["W_join"]), ZERO[enc])
        got = eng.op_join(x, n, groups, gap, 8000, encoding=enc)
        assert _same(got, want), (enc, groups[:2], gaps, np.flatnonzero((got != want).reshape(G, -1).any(0))[:8])


@pytest.mark.parametrize("enc", ENCS)
def test_device_copy_touches_nothing_outside_the_joined_rows(enc):
    """a sentinel-filled device buffer with dst_stride > W_join, even and odd: only [G][W_join] is written"""
    from hip_util import DeviceBuffer
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    e = _engine("bf16", a, ids, mask, sttl, sdp, durs)
    rows, gap = [2, 1, 3], [13230, 5, 0]
    want, plen, _ = e.batch_fetch_joined(rows, gap, 0.3, encoding=enc, cut=False)
    Wj = want.shape[1]
    for stride in (Wj + 32 - Wj % 16, Wj + 5 + Wj % 2):  # wide and a multiple of 16; odd
        like = binding.encoded_empty(enc, 3, stride)
        like[...] = 0x5A if like.dtype == np.uint8 else -7
        d = DeviceBuffer(like)
        e.batch_copy_joined_device(rows, gap, 0.3, d.ptr, stride, encoding=enc)
        e.sync()
        got = d.to_host()
        assert _same(np.ascontiguousarray(got[:, :Wj]), want), (enc, stride)
        assert np.all(got[:, Wj:] == like[:, Wj:]), (enc, stride)
    e.close()


# ---- 2. every fetch path, byte-exact -------------------------------------------------------------------------------------------------
def _tiny_batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 6, 14, [14, 9, 5, 12, 7, 11], seed=2)
    return a, ids, mask, sttl, sdp, np.array([0.71, 0.23, 0.52, 0.64, 0.31, 0.47], np.float32)


def _engine(dtype, a, ids, mask, sttl, sdp, durs, seed=9):
    e = binding.Engine(0, dtype)
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)  # length-aware: the chunks of a long text
    e.set_shape_buckets(True)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(2, 1.05, seed)
    return e


def _member_len(e, a, dur):
    """the whole wave of each member at the output rate: ceil(L_i * chunk * P / Q), at most the row"""
    _, _, Wo = e.batch_dims()
    cs = a.base_chunk_size * a.chunk_compress_factor
    hz = e.output_rate
    g = math.gcd(hz, a.sample_rate)
    P, Q = hz // g, a.sample_rate // g
    out = []
    for d in dur:
        wl = int(np.float32(d) * np.float32(a.sample_rate))
        L = (wl + cs - 1) // cs
        out.append(min(Wo, -(-L * cs * P // Q)))
    return out


def _host_join(e, a, enc, rows, gap, gap_s, mode):
    """the host concatenation of the per-row fetch in the same encoding: what the joined fetch must equal byte for byte"""
    wav, dur = e.batch_fetch_encoded(enc)
    lens = join_ref.member_lengths(_member_len(e, a, dur), dur, e.output_rate, mode)
    p = join_ref.plan(rows, gap, gap_s, _member_len(e, a, dur), dur, e.output_rate, mode)
    return join_ref.join(wav, lens, rows, gap, ZERO[enc]), p


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_fetch_path_equals_the_host_join(dtype):
    from hip_util import DeviceBuffer
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    e = _engine(dtype, a, ids, mask, sttl, sdp, durs)
    rows, gap_s = [2, 1, 3], [0.3, 0.25, 0.0]
    checked = 0
    for rate, lo in itertools.product((None, 8000, 16000, 48000), (None, -20.0)):
        e.set_output_rate(rate)
        e.set_loudness(lo)
        hz = e.output_rate
        gap = [int(s * hz) for s in gap_s]
        for enc, mode in itertools.product(ENCS, (join_ref.WHOLE, join_ref.TRIM)):
            want, p = _host_join(e, a, enc, rows, gap, gap_s, mode)
            got, dur = e.batch_fetch_joined(rows, gap, gap_s, mode=mode, gain_scope="row", encoding=enc)
            assert dur.tobytes() == p["prog_dur"].tobytes()
            for g in range(3):
                assert _same(got[g], want[g]), (dtype, rate, lo, enc, mode, g)
            full, plen, _ = e.batch_fetch_joined(rows, gap, gap_s, mode=mode, encoding=enc, cut=False)
            assert np.array_equal(plen, p["prog_len"]) and full.shape[1] == p["W_join"]
            assert _same(full, join_ref.padded(want, p["W_join"], ZERO[enc]))  # the zero codeword behind every programme's end
            checked += 1
            # the pipelined slots and the device copy: every encoding and both modes at one resampled rate with loudness on, and natively without
            if (rate, lo) in ((16000, -20.0), (None, None)):
                for slot in (0, 1):
                    e.fetch_joined_begin(slot, rows, gap, gap_s, mode=mode, encoding=enc)
                    s_got, s_dur = e.fetch_encoded_end(slot)
                    assert _same(s_got, full) and s_dur.tobytes() == p["prog_dur"].tobytes(), (slot, enc, mode)
                Wj = p["W_join"]
                for stride in (Wj + 32 - Wj % 16, Wj + 3 - Wj % 2):  # wide and aligned; odd
                    like = binding.encoded_empty(enc, 3, stride)
                    like[...] = 0x5A if like.dtype == np.uint8 else -7
                    d = DeviceBuffer(like)
                    e.batch_copy_joined_device(rows, gap, gap_s, d.ptr, stride, mode=mode, encoding=enc)
                    e.sync()
                    back = d.to_host()
                    assert _same(np.ascontiguousarray(back[:, :Wj]), full) and np.all(back[:, Wj:] == like[:, Wj:]), (enc, mode, stride)
    assert checked == 4 * 2 * 5 * 2
    e.close()


def test_refused_arguments_and_states():
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    with pytest.raises(binding.StnError) as ei:
        e.batch_fetch_joined([6], 0, 0.0)
    assert ei.value.code == -3  # STN_ERR_STATE: no finished batch
    e.close()
    e = _engine("bf16", a, ids, mask, sttl, sdp, durs)
    ref, _ = e.batch_fetch_joined([6], 100, 0.1, encoding="pcm16")
    for kw in (dict(rows=[5]), dict(rows=[3, 4]), dict(rows=[6, 0]), dict(gap_samples=-1), dict(mode=2), dict(gain_scope=3), dict(encoding=9)):
        args = dict(rows=[6], gap_samples=100, gap_seconds=0.1)
        args.update(kw)
        with pytest.raises((binding.StnError, ValueError)) as ei:
            e.batch_fetch_joined(**args)
        if isinstance(ei.value, binding.StnError):
            assert ei.value.code == -1, kw
    import ctypes
    j, keep = binding._join([6], 100, 0.1)
    wj, _, _ = e.batch_join_dims([6], 100, 0.1)
    small = np.empty(wj - 1, np.int16)
    rc = e._lib.stn_batch_fetch_joined(e._h, ctypes.byref(j), binding.ENC_PCM16, small.ctypes.data, small.nbytes, None, None)
    assert rc == -1 and str(wj * 2) in e._lib.stn_last_error(e._h).decode()  # the message states the bytes needed
    from hip_util import DeviceBuffer
    d = DeviceBuffer(np.zeros((1, wj), np.int16))
    with pytest.raises(binding.StnError) as ei:
        e.batch_copy_joined_device([6], 100, 0.1, d.ptr, wj - 1, encoding="pcm16")
    assert ei.value.code == -1 and "dst_stride" in str(ei.value)
    again, _ = e.batch_fetch_joined([6], 100, 0.1, encoding="pcm16")
    assert _same(again[0], ref[0])  # nothing was left half-done
    e.close()


# ---- 3. programme loudness against float64 ---------------------------------------------------------------------------------------------------
def _signals(hz, rng):
    """test_gpu_loudness._signals: a tone, coloured noise under an envelope with a DC offset, a quiet-then-loud row (the relative gate), a
    row shorter than one block and an all-zero row; lengths that are multiples of neither the chunk (32) nor the hop"""
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


TONE, NOISE, QUIET_LOUD = 0, 1, 2
TARGET, CEIL = -16.0, -1.0


def _programmes(hz):
    """(member rows, member lengths, members per programme, gaps) of the four programmes of the check"""
    x, n = _signals(hz, np.random.default_rng(hz))
    members = [TONE, NOISE, QUIET_LOUD, NOISE, TONE, QUIET_LOUD, TONE, TONE]
    groups, gaps = [3, 2, 1, 2], [int(0.3 * hz)] * 3 + [0]
    return x[members], n[members], groups, gaps


@pytest.mark.parametrize("hz", [8000, 16000, 44100, 48000])
def test_programme_gain_against_float64(eng, hz):
    x, n, groups, gaps = _programmes(hz)
    y, lufs, peak, gain = eng.op_join(x, n, groups, gaps, hz, loudness=(TARGET, CEIL))
    plain = eng.op_join(x, n, groups, gaps, hz)
    progs = join_ref.join(x, n, groups, gaps, 0.0)
    for g, p in enumerate(progs):
        ref = integrated_loudness(p.astype(np.float64), hz)
        print(f"\n{hz} Hz programme {g}: {float(lufs[g]):.4f} LUFS (float64 {ref:.4f}), peak {float(peak[g]):.4f}, gain {float(gain[g]):.4f}")
        assert math.isfinite(ref) and abs(float(lufs[g]) - ref) <= 0.01, (hz, g, lufs[g], ref)
        assert peak[g] == np.abs(p).max(), (hz, g)  # exact: max is order-independent
        want = min(10 ** ((TARGET - float(lufs[g])) / 20), 10 ** (CEIL / 20) / float(peak[g]))
        assert abs(float(gain[g]) - want) <= 2e-7 * want
        assert _same(y[g, : len(p)], p * np.float32(gain[g])), (hz, g)  # join * float32(g), bit for bit
        assert _same(plain[g, : len(p)], p) and np.all(y[g, len(p):] == 0)


# ---- 4. the scope matters ------------------------------------------------------------------------------------------------------------
def test_scope_programme_keeps_the_dynamics_scope_row_does_not(eng):
    hz = 48000
    x, n = _signals(hz, np.random.default_rng(hz))
    x, n = x[[NOISE, TONE]], n[[NOISE, TONE]]
    gap = int(0.3 * hz)
    L_in = [integrated_loudness(x[i, : n[i]].astype(np.float64), hz) for i in range(2)]
    assert 8.0 <= abs(L_in[0] - L_in[1]) <= 10.0, L_in
    # one gain for the programme: its loudness is the target, the difference between its two segments is the input's
    y, lufs, peak, gain = eng.op_join(x, n, [2], [gap], hz, loudness=(TARGET, CEIL))
    total = n[0] + gap + n[1]
    assert abs(integrated_loudness(y[0, :total].astype(np.float64), hz) - TARGET) <= 0.01
    seg = [y[0, : n[0]], y[0, n[0] + gap: total]]
    L_out = [integrated_loudness(s.astype(np.float64), hz) for s in seg]
    assert abs((L_out[0] - L_out[1]) - (L_in[0] - L_in[1])) <= 0.01, (L_in, L_out)
    # one gain per member (each its own programme: the same launches, the gains a GAIN_ROW fetch applies): every segment at the target,
    # the joined programme not
    _, _, _, g_row = eng.op_join(x, n, [1, 1], [0, 0], hz, loudness=(TARGET, CEIL))
    rowwise = np.concatenate([x[0, : n[0]] * np.float32(g_row[0]), np.zeros(gap, np.float32), x[1, : n[1]] * np.float32(g_row[1])])
    for s in (rowwise[: n[0]], rowwise[n[0] + gap:]):
        assert abs(integrated_loudness(s.astype(np.float64), hz) - TARGET) <= 0.01
    assert abs(integrated_loudness(rowwise.astype(np.float64), hz) - TARGET) > 0.05


# ---- 5. the hosts ----------------------------------------------------------------------------------------------------------------------
LONG_TEXT = ("The engine synthesizes long passages by splitting them into chunks. Each chunk is synthesized on its own. "
             "The chunks are then joined with a short silence between them. This keeps the memory footprint small! "
             "Does it also keep the prosody natural? Mostly, yes. " * 3).strip()  # the text of test_host_long_form_normalizes_each_chunk


def _tts(**kw):
    from supertonic_amd.tts import Style, load_text_to_speech
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, **kw)
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    return tts, Style(sttl, sdp)


def test_python_host_text_scope_normalizes_the_text_as_one():
    """Target -23 LUFS (EBU R 128's programme level; the issue fixes no figure for this host): noise-like synthetic speech has a crest
    factor that can put -16 at the ceiling, and the un-capped branch is the one that shows the programme gain."""
    target, ceil = -23.0, -1.0
    uncapped = 0
    for seed in (3, 4):
        tts, style = _tts(noise_seed=seed, loudness=(target, ceil))
        chunks = host.chunk_text(LONG_TEXT, 300)
        assert len(chunks) >= 3
        wav, dur = tts(LONG_TEXT, "en", style, 2, loudness_scope="text")
        assert wav.shape[0] == 1 and dur.shape == (1,)
        n = min(wav.shape[1], int(np.float32(SR) * np.float32(dur[0])))
        L = integrated_loudness(wav[0, :n].astype(np.float64), SR)
        peak = float(np.abs(wav[0, :n]).max())
        B, _, W = tts.engine.batch_dims()
        print(f"\nseed {seed}: {len(chunks)} chunks -> {L:.3f} LUFS, peak {peak:.4f}; joined fetch {wav.shape[1] * 4} bytes over PCIe against "
              f"{B * W * 4} for the {B} x {W} rows it replaces")
        if abs(L - target) <= 0.01:
            uncapped += 1
        else:
            assert L < target and abs(peak - 10 ** (ceil / 20)) <= 1e-6 * 10 ** (ceil / 20), (seed, L, peak)
        # per chunk, the same text reads otherwise: the scope is what changed
        tts.noise_seed, tts._calls = seed, 0
        w_chunk, d_chunk = tts(LONG_TEXT, "en", style, 2)
        assert d_chunk[0] == dur[0] and w_chunk.shape == wav.shape and not np.array_equal(w_chunk, wav)
        tts.engine.close()
    assert uncapped >= 1


@pytest.mark.parametrize("rate,enc", [(None, None), (8000, None), (8000, "mulaw")])
def test_python_host_default_call_is_the_host_join_byte_for_byte(rate, enc):
    from supertonic_amd import service
    from supertonic_amd.tts import Style
    tts, style = _tts(noise_seed=21, output_rate=rate, loudness=-20)
    chunks = host.chunk_text(LONG_TEXT, 300)
    n = len(chunks)
    got, dur = tts(LONG_TEXT, "en", style, 2, 1.05, 0.3, encoding=enc)
    tts.noise_seed, tts._calls = 21, 0
    rep = Style(np.repeat(style.ttl, n, axis=0), np.repeat(style.dp, n, axis=0))
    waves, durs = tts.solo_batch(chunks, ["en"] * n, rep, 2, 1.05, encoding=enc)  # the pre-change long form: rows, then the host join
    ref, d = service.join_chunks(waves, durs, 0.3, tts.output_rate, enc)
    assert got.shape[0] == 1 and _same(got[0], ref) and float(dur[0]) == d
    tts.engine.close()


def _wav(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[36:40] == b"data"
    sr = struct.unpack("<i", b[24:28])[0]
    return sr, np.frombuffer(b[44:], dtype="<i2")


def _cli(args, cwd, ok=True):
    p = subprocess.run([CLI, "--synthetic"] + args, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (p.returncode == 0) == ok, p.stdout + p.stderr
    return p.stdout + p.stderr


def test_cli_text_scope_and_trimmed_chunks(tmp_path):
    # the voice as a file, so that the Python host below can run the same style (the CLI's synthetic styles are keyed by name)
    import json
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    (tmp_path / "voice.json").write_text(json.dumps({"style_ttl": {"data": sttl.astype(np.float64).tolist(), "dims": list(sttl.shape)},
                                                     "style_dp": {"data": sdp.astype(np.float64).tolist(), "dims": list(sdp.shape)}}))
    common = ["--text", LONG_TEXT, "--n-test", "1", "--seed", "3", "--total-step", "2", "--voice-style", "voice.json"]
    _cli(common + ["--save-dir", "text", "--loudness", "-16", "--loudness-scope", "text"], tmp_path)
    (f,) = os.listdir(tmp_path / "text")
    sr, pcm = _wav(tmp_path / "text" / f)
    L = integrated_loudness(pcm.astype(np.float64) / 32767.0, sr)
    capped = np.abs(pcm.astype(np.int32)).max() >= int(10 ** (-1 / 20) * 32767) - 1
    print(f"\nCLI --loudness-scope text: the whole file {L:.3f} LUFS" + (" (peak at the ceiling)" if capped else ""))
    assert (L < -16.0 + 0.05) if capped else abs(L - (-16.0)) <= 0.05, L
    # --trim-chunks: the file is as long as the reference's Rust join of the same chunks
    _cli(common + ["--save-dir", "trim", "--trim-chunks"], tmp_path)
    _, trimmed = _wav(tmp_path / "trim" / f)
    _cli(common + ["--save-dir", "whole"], tmp_path)
    _, whole = _wav(tmp_path / "whole" / f)
    tts, style = _tts(noise_seed=3)  # the same weights and text: the durations the CLI's run predicted
    chunks = host.chunk_text(LONG_TEXT, 300)
    n = len(chunks)
    from supertonic_amd.tts import Style
    waves, durs = tts.solo_batch(chunks, ["en"] * n, Style(np.repeat(style.ttl, n, 0), np.repeat(style.dp, n, 0)), 2)
    gap = int(np.float32(0.3) * np.float32(SR))  # the C++ host's rule
    plans = {}
    for mode, pcm_file in ((join_ref.TRIM, trimmed), (join_ref.WHOLE, whole)):
        p = plans[mode] = join_ref.plan([n], [gap], [0.3], [len(w) for w in waves], durs, SR, mode)
        assert len(pcm_file) == min(int(p["prog_len"][0]), int(np.float32(SR) * p["prog_dur"][0])), mode
        # the silences sit where the plan puts them: the gap in front of every later member is zeros
        for d in p["seg_dst"][1:]:
            assert np.all(pcm_file[int(d) - gap: int(d)] == 0), (mode, int(d))
    # (both files end at the text's duration, which is where the trimmed join ends anyway: what trimming moves is every later chunk)
    assert plans[join_ref.TRIM]["prog_len"][0] < plans[join_ref.WHOLE]["prog_len"][0]
    assert np.all(plans[join_ref.TRIM]["seg_dst"][1:] < plans[join_ref.WHOLE]["seg_dst"][1:]) and not np.array_equal(trimmed, whole)
    tts.engine.close()
    out = _cli(common + ["--save-dir", "no", "--loudness", "-16", "--loudness-scope", "text", "--devices", "0,0"], tmp_path, ok=False)
    assert "scope" in out  # a group is refused with a message, not normalized per chunk


def test_service_jobs_with_unlike_silences_share_a_batch():
    from supertonic_amd import service
    from supertonic_amd.tts import Style
    tts, style = _tts(noise_seed=5)
    b = service.DynamicBatcher(tts, max_batch=64, max_wait_ms=1500.0)
    texts = {0.1: host.chunk_text(LONG_TEXT, 300), 0.45: host.chunk_text(LONG_TEXT[: len(LONG_TEXT) // 2], 300)}
    out = {}

    def go(sil):
        out[sil] = b.submit(texts[sil], "en", style, 2, 1.05, silence_duration=sil)

    th = [threading.Thread(target=go, args=(s,)) for s in texts]
    [t.start() for t in th]
    [t.join() for t in th]
    b.close()
    assert b.batches == [sum(len(t) for t in texts.values())], b.batches  # one engine batch for both jobs
    # each job's own result: its rows of the same merged batch (same seed, either queue order), joined on the host with ITS silence
    matched = 0
    for order in ((0.1, 0.45), (0.45, 0.1)):
        tts.noise_seed, tts._calls = 5, 0
        merged = [t for s in order for t in texts[s]]
        n = len(merged)
        waves, durs = tts.solo_batch(merged, ["en"] * n, Style(np.repeat(style.ttl, n, 0), np.repeat(style.dp, n, 0)), 2, 1.05)
        o, ok = 0, True
        for s in order:
            k = len(texts[s])
            ref, d = service.join_chunks(waves[o:o + k], durs[o:o + k], s, SR)
            (w,), dd = out[s]
            ok = ok and _same(w, ref) and float(dd[0]) == d
            o += k
        matched += ok
    assert matched == 1
    tts.engine.close()


# ---- 6. no side effects -------------------------------------------------------------------------------------------------------------------
def _launches(e, fetch):
    """the kernel families of a fetch's launches, in dispatch order (families are named while profiling is on)"""
    e.profile_enable(True)
    e.launch_log_enable(True)
    fetch()
    log = e.launch_log()
    e.launch_log_enable(False)
    e.profile_enable(False)
    return [f for f, _ in log]


def test_joined_fetches_leave_everything_else_alone():
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    fresh = _engine("bf16", a, ids, mask, sttl, sdp, durs, seed=4)
    e = _engine("bf16", a, ids, mask, sttl, sdp, durs, seed=4)
    for _ in range(3):  # the second sighting captures the shape, the third replays it
        e.batch_run(2, 1.05, 4)
    e.batch_fetch_pcm16()
    cached, replays = e.graphs_cached, e.graph_replays
    assert cached >= 1 and replays >= 1
    rows, gap = [2, 4], [13230, 100]
    # the launch logs: one join launch natively with loudness off; join + four measurement launches + the gain store per programme
    fams = _launches(e, lambda: e.batch_fetch_joined(rows, gap, 0.3, encoding="pcm16"))
    assert fams == ["out.join"], fams
    e.set_loudness(-20.0)
    fams = _launches(e, lambda: e.batch_fetch_joined(rows, gap, 0.3, gain_scope="programme", encoding="pcm16"))
    assert fams == ["out.join"] + ["out.loudness"] * 4 + ["out.loudness_gain"], fams
    prog, _ = e.batch_fetch_joined(rows, gap, 0.3, gain_scope="programme")
    row, _ = e.batch_fetch_joined(rows, gap, 0.3, gain_scope="row")
    assert not _same(prog[1], row[1])
    lufs, peak, gain = e.batch_join_loudness(rows, gap, 0.3)
    plain, _ = (lambda: (e.set_loudness(None), e.batch_fetch_joined(rows, gap, 0.3))[1])()
    e.set_loudness(-20.0)
    for g in range(2):
        assert _same(prog[g], plain[g] * np.float32(gain[g])), g  # one gain per programme, bit for bit
    # a single-member programme whose span is the row's span: the same bytes under both scopes
    for mode in ("whole", "trim"):
        one_p, _ = e.batch_fetch_joined([1] * 6, 0, 0.0, mode=mode, gain_scope="programme", encoding="pcm16")
        one_r, _ = e.batch_fetch_joined([1] * 6, 0, 0.0, mode=mode, gain_scope="row", encoding="pcm16")
        same_span = [g for g in range(6) if len(one_r[g]) >= int(np.float32(durs[g] / np.float32(1.05)) * np.float32(SR))]
        assert same_span and all(_same(one_p[g], one_r[g]) for g in same_span), mode
    for slot in (0, 1):
        e.fetch_joined_begin(slot, rows, gap, 0.3, mode="trim", encoding="mulaw")
        e.fetch_encoded_end(slot)
    e.set_loudness(None)
    assert e.graphs_cached == cached and e.graph_replays == replays  # no capture, no drop
    e.batch_run(2, 1.05, 4)
    assert e.graphs_cached == cached and e.graph_replays == replays + 1  # the next run is a replay
    # plain fetches: byte-identical to a handle that never joined, with their own launch logs
    for enc in ENCS:
        w0, d0 = fresh.batch_fetch_encoded(enc)
        w1, d1 = e.batch_fetch_encoded(enc)
        assert _same(w0, w1) and _same(d0, d1), enc
    assert _same(fresh.batch_fetch()[0], e.batch_fetch()[0])
    assert _launches(e, e.batch_fetch_pcm16) == _launches(fresh, fresh.batch_fetch_pcm16) == ["out.store_rows"]
    e.set_loudness(-20.0)
    fresh.set_loudness(-20.0)
    assert _same(fresh.batch_fetch_pcm16()[0], e.batch_fetch_pcm16()[0])
    assert _launches(e, e.batch_fetch_pcm16) == _launches(fresh, fresh.batch_fetch_pcm16)
    e.close()
    fresh.close()


# ---- 7. cost -----------------------------------------------------------------------------------------------------------------------------
def _c3_like(n, seed):
    arch = default_arch()
    texts = workload.utterances(n, min_words=3, max_words=12, seed=seed)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * n)
    sttl, sdp = workload.synthetic_styles(arch, list(range(n)))
    return arch, ids, mask, sttl, sdp, workload.forced_durations(texts)


@pytest.mark.parametrize("enc", ["pcm16", "mulaw"])
def test_timing_report_c3_join(enc):
    """Event-timed cost of the join for a C3-sized batch (128 rows into 16 programmes of 8, 13 230-sample gaps) at the native rate,
    beside out.store_rows on the same batch and encoding in the same process (the per-row fetch: the same bytes, aligned); a generous
    bound only.  DESIGN.md section 13 records the measured pair."""
    a, ids, mask, sttl, sdp, durs = _c3_like(128, 11)
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    e.batch_run(5, 1.05, 1)
    rows, gap = [8] * 16, 13230
    per = {}
    for name, fetch in (("out.store_rows", lambda: e.batch_fetch_encoded(enc)), ("out.join", lambda: e.batch_fetch_joined(rows, gap, 0.3, encoding=enc, cut=False))):
        fetch()  # warm: scratch, tables
        e.profile_enable(True)
        e.profile_reset()
        for _ in range(10):
            fetch()
        prof = e.profile()
        e.profile_enable(False)
        assert prof[name]["launches"] == 10 and [k for k in prof if k.startswith("out.")] == [name], prof.keys()
        per[name] = prof[name]["ms"] * 1e3 / 10
    B, _, W = e.batch_dims()
    Wj, plen, _ = e.batch_join_dims(rows, gap, 0.3)
    eb = binding.ENCODING_BYTES[binding.ENCODINGS[enc]]
    print(f"\nC3 batch, {enc}: out.store_rows {per['out.store_rows']:.1f} us for {B} x {W} samples ({B * W * (4 + eb) / 1e6:.1f} MB moved); "
          f"out.join {per['out.join']:.1f} us for 16 x {Wj} ({(int(plen.sum()) - 16 * 7 * gap) * 4 / 1e6 + 16 * Wj * eb / 1e6:.1f} MB moved); "
          f"ratio {per['out.join'] / per['out.store_rows']:.2f}; host copy {16 * Wj * eb} bytes against {B * W * eb}")
    assert per["out.join"] <= 1000.0
    e.close()
