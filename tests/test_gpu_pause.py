"""The pause limit on an MI355X (include/stn.h "pause limit"; pause_rows_kernel in kernels_edges.hip, join_trim_rows_kernel; DESIGN.md
section 17) against the float64 reference tests/pause_ref.py: edges, cuts and lengths exactly, the fp32 rows bit for bit, every encoding
byte for byte, zero codewords behind len included.

Rows are tone bursts over whole frames on a -80 dBFS noise floor, so every frame lies tens of dB from the threshold; section 14's
0.01 dB margin is asserted over all frames of every row used, on the CPU, and so is the number of cuts designed into each row, before
anything runs on the GPU: no case can pass because nothing was cut."""
import functools
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
import pause_ref as pz
import silence_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "supertonic_amd", "example_native")
ENCS = ["f32", "pcm16", "pcm24", "mulaw", "alaw"]
ZERO = {e: binding.ZERO_CODEWORD[binding.ENCODINGS[e]] for e in ENCS}
RATES = [8000, 11025, 16000, 44100, 48000, 88200, 96000, 176400, 192000]  # frames of 80 to 1920 samples, as the edges run
CAP = 8  # pairs of the cut tables asked for where a row has a handful of cuts


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


def _same(a, b):
    """byte equality (float rows included: -0.0 and 0.0 differ)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _odd(n, F):
    while n % 32 == 0 or n % F == 0:
        n -= 1
    return n


def _want(x, n, hz, top_db, keep_ms, fade_ms, max_pause_ms, cuts, gain=None):
    """the reference on rows whose designed numbers of cuts are `cuts`, margin and counts asserted"""
    w = pz.pause_rows(x, n, hz, top_db, keep_ms, fade_ms, max_pause_ms, gain)
    assert w["margin"].min() >= pz.MARGIN_DB, (hz, w["margin"])
    assert w["n_cuts"].tolist() == list(cuts), (hz, max_pause_ms, w["n_cuts"], cuts)
    return w


def _check_tables(got, want, cap):
    for k in ("start", "end", "len", "n_cuts"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert np.array_equal(got["cuts"], pz.cuts_array(want["cuts"], cap))


# ---- 1. row shapes at nine rates ---------------------------------------------------------------------------------------------------------
# frames: burst (first, count).  Designed for max_pause 20 ms (2 frames) and 100 ms (10 frames); the counts per row are stated beside them
SHAPES = [
    ([(3, 40)], 0, 0),                                  # no pause
    ([(4, 5), (10, 6)], 0, 0),                          # a pause of one frame: shorter than either Mp
    ([(2, 6), (40, 9)], 1, 1),                          # one long pause
    ([(5, 4), (30, 1), (55, 3)], 2, 2),                 # two cuts around a single active frame
    ([(6, 3), (14, 3), (60, 2)], 2, 1),                 # 5 frames, then 43
    ([], 0, 0),                                         # no speech
    ([(1, 2)], 0, 0),                                   # n = 0 (the burst lies behind the span)
]


@functools.lru_cache(maxsize=None)
def _shape_rows(hz):
    F = ref.frame(hz)
    W = 72 * F + 8  # 0.72 s; a multiple of 4
    W += (-W) % 4
    x = np.zeros((len(SHAPES), W), np.float32)
    n = np.zeros(len(SHAPES), np.int64)
    for r, (bursts, _, _) in enumerate(SHAPES):
        n[r] = 0 if r == 6 else _odd(W - 5 - 7 * r, F)
        x[r] = pz.burst_row(hz, W, int(n[r]), bursts if n[r] else [], 100 * r + hz)
    x[0, 5::13] = -0.0
    x[2] *= 4.0  # beyond +-1: the encodings clamp
    return x, n


@pytest.mark.parametrize("hz", RATES)
def test_op_rows_equal_the_reference_in_every_encoding(eng, hz):
    x, n = _shape_rows(hz)
    assert 0.3 <= x.shape[1] / hz <= 2.0 and all(v % 32 and v % ref.frame(hz) for v in n[:6])
    g = np.array([0.5, 1.0, 1.7, 0.25, 2.0, 1.0, 3.0], np.float32)
    for (mp, fade_ms, col), gain in itertools.product(((20.0, 20.0, 1), (100.0, 5.0, 2), (20.0, 0.0, 1)), (None, g)):
        want = _want(x, n, hz, 40.0, 20.0, fade_ms, mp, [s[col] for s in SHAPES], gain)
        if fade_ms == 20.0:  # the single active frame between two cuts: Mp + F samples, shorter than both fades together
            a, b = pz.segments(int(want["start"][3]), int(want["end"][3]), want["cuts"][3])[1]
            assert b - a == pz.pause_samples(hz, mp) + ref.frame(hz) < 2 * ref.samples(hz, fade_ms)
        for enc in ENCS:
            got = eng.op_pause_trim(x, hz, n, 40.0, 20.0, fade_ms, mp, gain, enc, cap_pairs=CAP)
            _check_tables(got, want, CAP)
            assert _same(got["y"], want["y"] if enc == "f32" else eng.op_encode(want["y"], enc)), (hz, mp, fade_ms, gain is not None, enc)
            if fade_ms == 0.0:  # every segment is a byte slice of the untrimmed rows in that encoding
                xg = x if gain is None else (x * gain[:, None]).astype(np.float32)
                plain = eng.op_encode(xg, enc)
                for r in range(x.shape[0]):
                    at = 0
                    for a, b in pz.segments(int(want["start"][r]), int(want["end"][r]), want["cuts"][r]):
                        assert _same(got["y"][r, at:at + b - a], plain[r, a:b]), (hz, enc, r)
                        at += b - a
                    assert at == want["len"][r] and np.all(got["y"][r, at:] == ZERO[enc])
    assert want["len"][6] == 0 and want["len"][5] == n[5]


def test_op_ranges_are_refused(eng):
    x, n = _shape_rows(8000)
    for kw in (dict(max_pause_ms=19.0), dict(max_pause_ms=5001.0), dict(top_db=0.5), dict(fade_ms=51.0)):
        with pytest.raises(binding.StnError) as ei:
            eng.op_pause_trim(x, 8000, n, **kw)
        assert ei.value.code == -1 and "must be in" in str(ei.value)
    assert eng.pause_limit is None
    for bad in (19.9, 5000.5):
        assert eng._lib.stn_set_pause_limit(eng._h, 1, bad) == -1 and "must be in [20, 5000]" in eng.last_error()
    assert eng.pause_limit is None  # the previous setting stayed
    eng.set_pause_limit(250)
    assert eng.pause_limit == 250.0
    assert eng._lib.stn_set_pause_limit(eng._h, 1, 6000.0) == -1 and eng.pause_limit == 250.0
    eng.set_pause_limit(None)
    assert eng.pause_limit is None


# ---- 2. tile seams at 8 kHz: the row workgroup walks 1024 frames at a time -------------------------------------------------------------
SEAMS = [
    (1023, [(5, 3), (300, 2), (700, 1), (1021, 2)], 3),
    (1024, [(5, 3), (300, 2), (700, 1), (1022, 2)], 3),                # closed by the last but one thread of the first tile
    (1025, [(5, 3), (300, 2), (700, 1), (1024, 1)], 3),                # closed by the first thread of the second tile: all three carries
    (2100, [(5, 3), (1020, 2), (1030, 1), (1040, 1), (2000, 2)], 4),   # a pause over frames 1022 .. 1029 straddles the seam; cuts on both sides
    (2100, [(5, 3), (500, 2), (1000, 1), (2060, 3), (2080, 2)], 4),    # a pause of 1059 frames: the second tile holds no active frame
    (2100, [(1023, 1), (1024, 1), (2047, 1), (2049, 1)], 1),           # neighbours across a seam are no pause; one frame at 2048 is, uncut; 1025 .. 2046 is cut
]


@functools.lru_cache(maxsize=None)
def _seam_rows():
    hz, F = 8000, 80
    W = 2100 * F
    x = np.zeros((len(SEAMS), W), np.float32)
    n = np.zeros(len(SEAMS), np.int64)
    for r, (K, bursts, _) in enumerate(SEAMS):
        n[r] = K * F - 13
        assert -(-int(n[r]) // F) == K and n[r] % 32 and n[r] % F
        x[r] = pz.burst_row(hz, W, int(n[r]), bursts, 7 + r)
    want = _want(x, n, hz, 40.0, 20.0, 5.0, 50.0, [s[2] for s in SEAMS])
    return x, n, want


def test_tile_seams_and_carries(eng):
    x, n, want = _seam_rows()
    assert x.shape[1] == 168000
    # the straddling pause and the one longer than a tile are among the cuts
    assert (1022 * 80 + 200, 1030 * 80 - 200) in want["cuts"][3] and (1001 * 80 + 200, 2060 * 80 - 200) in want["cuts"][4]
    assert want["cuts"][5] == [(1025 * 80 + 200, 2047 * 80 - 200)]
    for enc in ("f32", "pcm16"):
        got = eng.op_pause_trim(x, 8000, n, 40.0, 20.0, 5.0, 50.0, None, enc, cap_pairs=CAP)
        _check_tables(got, want, CAP)
        assert _same(got["y"], want["y"] if enc == "f32" else eng.op_encode(want["y"], enc)), enc


def test_a_rows_table_and_bytes_do_not_depend_on_the_batch(eng):
    x, n, want = _seam_rows()
    r = 3
    alone = eng.op_pause_trim(x[r:r + 1], 8000, n[r:r + 1], 40.0, 20.0, 5.0, 50.0, None, "mulaw", cap_pairs=CAP)
    W2 = x.shape[1] + 37  # another width, odd: the scalar loads
    xb = np.zeros((5, W2), np.float32)
    xb[:, :x.shape[1]] = x[[0, 4, 1, r, 2]]
    xb[:, x.shape[1]:] = 0.3
    nb = n[[0, 4, 1, r, 2]]
    many = eng.op_pause_trim(xb, 8000, nb, 40.0, 20.0, 5.0, 50.0, None, "mulaw", cap_pairs=CAP)
    for k in ("start", "end", "len", "n_cuts", "cuts"):
        assert np.array_equal(alone[k][0], many[k][3]) and np.array_equal(alone[k][0], (pz.cuts_array(want["cuts"], CAP) if k == "cuts" else want[k])[r]), k
    k = int(want["len"][r])
    assert _same(alone["y"][0, :k], many["y"][3, :k]) and np.all(alone["y"][0, k:] == 0xFF) and np.all(many["y"][3, k:] == 0xFF)


# ---- 3. the cap ----------------------------------------------------------------------------------------------------------------------------
def test_300_cuttable_pauses_the_first_255_are_cut(eng):
    hz, F = 8000, 80
    K = 1 + 4 * 300 + 5
    n = np.array([K * F - 9], np.int64)
    assert n[0] % 32 and n[0] % F and 90000 < n[0] < 100000
    x = pz.burst_row(hz, K * F, int(n[0]), [(4 * i, 1) for i in range(301)], 11)[None, :]
    want = _want(x, n, hz, 40.0, 20.0, 5.0, 20.0, [255])
    assert want["cuts"][0][-1] == ((4 * 254 + 1) * F + 80, 4 * 255 * F - 80)
    assert want["len"][0] == want["end"][0] - want["start"][0] - 255 * (3 * F - 160)
    for enc in ("f32", "alaw"):
        got = eng.op_pause_trim(x, hz, n, 40.0, 20.0, 5.0, 20.0, None, enc, cap_pairs=255)
        _check_tables(got, want, 255)
        assert _same(got["y"], want["y"] if enc == "f32" else eng.op_encode(want["y"], enc)), enc
    # a caller's table smaller than the count: the count is whole, the table its first pairs
    got = eng.op_pause_trim(x, hz, n, 40.0, 20.0, 5.0, 20.0, None, "f32", cap_pairs=7)
    assert got["n_cuts"][0] == 255 and np.array_equal(got["cuts"], pz.cuts_array(want["cuts"], 7))


# ---- 4. the engine: every fetch path of a batch whose waveform is replaced by designed rows -------------------------------------------
DURS = np.array([0.71, 0.43, 0.92, 0.64, 0.51, 0.47], np.float32)
# bursts in seconds (first, length) inside each row's span; the designed cuts at max_pause 100 ms
BURSTS = [([(0.00, 0.10), (0.30, 0.10), (0.55, 0.05)], 2), ([(0.05, 0.30)], 0), ([(0.10, 0.05), (0.20, 0.20), (0.70, 0.10)], 1),
          ([(0.04, 0.05), (0.30, 0.02), (0.50, 0.05)], 2), ([(0.10, 0.10), (0.28, 0.15)], 0), ([(0.02, 0.08), (0.30, 0.10)], 1)]
MP = 100.0


def _tiny_batch():
    a = tiny_arch()
    ids, mask, sttl, sdp = make_inputs(a, 6, 14, [14, 9, 5, 12, 7, 11], seed=2)
    return a, ids, mask, sttl, sdp, DURS


def _burst_wav(a, e):
    B, L, W = e.batch_dims()
    sr = a.sample_rate
    F = ref.frame(sr)
    wav = np.zeros((B, W), np.float32)
    for b in range(B):
        nb = min(W, int(np.float32(DURS[b] / np.float32(1.05)) * np.float32(sr)))
        bursts = [(int(round(t0 * sr / F)), int(round(t1 * sr / F))) for t0, t1 in BURSTS[b][0]]
        assert all((f + k) * F < nb for f, k in bursts), (b, nb)
        wav[b] = pz.burst_row(sr, W, nb, bursts, 31 + b)
        wav[b, nb:] = 0.0  # (zeros behind the span: the resampler carries nothing into it)
    return wav


def _engine(dtype="bf16", runs=1):
    a, ids, mask, sttl, sdp, durs = _tiny_batch()
    e = binding.Engine(0, dtype)
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=durs)
    for _ in range(runs):
        e.batch_run(2, 1.05, 9)
    e.dbg_batch_set_wav(_burst_wav(a, e))
    return a, e


def _spans(e, dur):
    _, _, Wo = e.batch_dims()
    return np.array([max(0, min(Wo, int(np.float32(d) * np.float32(e.output_rate)))) for d in dur], np.int64)


def _expected(e, trim, mp, gain=None):
    """the reference on the untrimmed fp32 fetch at the current rate, before any gain; the designed cuts asserted"""
    lo, st = e.loudness, e.silence_trim
    e.set_silence_trim(None)
    e.set_loudness(None)
    x, dur = e.batch_fetch()
    e.set_loudness(lo)
    e.set_silence_trim(st)
    n = _spans(e, dur)
    return x, n, _want(x, n, e.output_rate, trim[0], trim[1], trim[2], mp, [b[1] for b in BURSTS], gain)


def _launches(e, fetch):
    e.profile_enable(True)
    e.launch_log_enable(True)
    fetch()
    log = e.launch_log()
    e.launch_log_enable(False)
    e.profile_enable(False)
    return log


def test_every_fetch_path_delivers_the_reference_rows():
    from hip_util import DeviceBuffer
    a, e = _engine()
    for rate, lo, trim in ((None, None, (40.0, 20.0, 5.0)), (16000, -20.0, (40.0, 10.0, 0.0)), (8000, None, (40.0, 20.0, 20.0))):
        e.set_output_rate(rate)
        e.set_loudness(lo)
        g = e.batch_loudness()[2] if lo is not None else None
        x, n, want = _expected(e, trim, MP, g)
        e.set_silence_trim(trim)
        e.set_pause_limit(MP)
        assert e.pause_limit == MP
        B, _, Wo = e.batch_dims()
        # stn_batch_pauses agrees with the reference and with the op on the same rows; the edges are still reported
        ln, nc, cuts = e.batch_pauses(CAP)
        op = e.op_pause_trim(x, e.output_rate, n, trim[0], trim[1], trim[2], MP, g, "f32", cap_pairs=CAP)
        _check_tables(dict(start=e.batch_silence_edges()[0], end=e.batch_silence_edges()[1], len=ln, n_cuts=nc, cuts=cuts), want, CAP)
        _check_tables(op, want, CAP)
        assert _same(op["y"], want["y"])
        for enc in ENCS:
            w = want["y"] if enc == "f32" else e.op_encode(want["y"], enc)
            got, dur = e.batch_fetch_encoded(enc)
            assert _same(got, w), (rate, lo, trim, enc)
            for slot in (0, 1):
                e.fetch_encoded_begin(slot, enc)
                s_got, s_dur = e.fetch_encoded_end(slot)
                assert _same(s_got, w) and s_dur.tobytes() == dur.tobytes(), (slot, enc)
            stride = Wo + 3 - Wo % 2  # odd
            like = binding.encoded_empty(enc, B, stride)
            like[...] = 0x5A if like.dtype == np.uint8 else -7
            d = DeviceBuffer(like)
            e.batch_copy_encoded_device(enc, d.ptr, stride)
            e.sync()
            back = d.to_host()
            assert _same(np.ascontiguousarray(back[:, :Wo]), w) and np.all(back[:, Wo:] == like[:, Wo:]), (enc, stride)
        if lo is None:
            assert _same(e.batch_fetch()[0], want["y"])
        e.set_pause_limit(None)
        e.set_silence_trim(None)
    e.close()


def test_the_pause_left_between_two_bursts_is_exactly_mp():
    a, e = _engine()
    sr = a.sample_rate
    F = ref.frame(sr)
    trim = (40.0, 20.0, 0.0)
    x, n, want = _expected(e, trim, MP)
    e.set_silence_trim(trim)
    e.set_pause_limit(MP)
    y, _ = e.batch_fetch()
    Mp = pz.pause_samples(sr, MP)
    # row 0: bursts over [0, 0.1 s) and [0.3 s, 0.4 s): the pause between them, 0.2 s, is cut to Mp
    a_f = int(round(0.10 * sr / F))
    at = a_f * F - int(want["start"][0])
    assert np.abs(y[0, at - F:at]).max() > 0.1 and np.abs(y[0, at:at + Mp]).max() < 1e-3 and np.abs(y[0, at + Mp:at + Mp + F]).max() > 0.1
    assert _same(y[0, at:at + Mp], np.concatenate([x[0, a_f * F:a_f * F + Mp - Mp // 2], x[0, int(round(0.30 * sr / F)) * F - Mp // 2:int(round(0.30 * sr / F)) * F]]))
    e.close()


def test_joined_fetch_is_the_host_join_of_the_rows():
    a, e = _engine()
    rows, gap_s = [2, 1, 3], [0.3, 0.25, 0.0]
    trim = (40.0, 20.0, 5.0)
    for rate, lo, lim, pk in ((None, None, None, None), (16000, -20.0, None, None), (None, -16.0, 5.0, "true")):
        e.set_output_rate(rate)
        e.set_loudness(lo)
        e.set_limiter(lim)
        e.set_peak_mode(pk or "sample")
        hz = e.output_rate
        gap = [int(s * hz) for s in gap_s]
        _, _, want = _expected(e, trim, MP)
        e.set_silence_trim(trim)
        e.set_pause_limit(MP)
        lens = want["len"]
        dur = (lens.astype(np.float32) / np.float32(hz)).astype(np.float32)
        p = join_ref.plan(rows, gap, gap_s, lens, dur, hz)
        for enc, mode in itertools.product(("f32", "pcm16", "mulaw"), ("whole", "trim")):
            per_row, _ = e.batch_fetch_encoded(enc)
            w = join_ref.padded(join_ref.join(per_row, lens, rows, gap, ZERO[enc]), p["W_join"], ZERO[enc])
            got, plen, pdur = e.batch_fetch_joined(rows, gap, gap_s, mode=mode, gain_scope="row", encoding=enc, cut=False)
            assert np.array_equal(plen, p["prog_len"]) and pdur.tobytes() == p["prog_dur"].tobytes(), (rate, lo, mode)
            assert _same(got, w), (rate, lo, lim, enc, mode)
            if lo is None:  # without loudness a programme has no gain of its own: the same bytes
                got, plen, pdur = e.batch_fetch_joined(rows, gap, gap_s, mode=mode, gain_scope="programme", encoding=enc, cut=False)
                assert np.array_equal(plen, p["prog_len"]) and pdur.tobytes() == p["prog_dur"].tobytes() and _same(got, w)
        wj, plen, pdur = e.batch_join_dims(rows, gap, gap_s)
        assert wj == p["W_join"] and np.array_equal(plen, p["prog_len"]) and pdur.tobytes() == p["prog_dur"].tobytes()
        per_row, _ = e.batch_fetch_encoded("pcm16")
        e.fetch_joined_begin(0, rows, gap, gap_s, encoding="pcm16")
        assert _same(e.fetch_encoded_end(0)[0], join_ref.padded(join_ref.join(per_row, lens, rows, gap, 0), p["W_join"], 0))
        if lo is not None and lim is None:  # one gain per programme: the joined, faded fp32 signal times float32(g_g)
            e.set_loudness(None)
            joined, _, _ = e.batch_fetch_joined(rows, gap, gap_s, cut=False)
            e.set_loudness(lo)
            g = e.batch_join_loudness(rows, gap, gap_s)[2]
            got, plen, pdur = e.batch_fetch_joined(rows, gap, gap_s, gain_scope="programme", cut=False)
            assert _same(got, (joined * g[:, None]).astype(np.float32)) and np.array_equal(plen, p["prog_len"]) and pdur.tobytes() == p["prog_dur"].tobytes()
        e.set_pause_limit(None)
        e.set_silence_trim(None)
    e.close()


def test_off_is_the_path_without_it_and_toggling_touches_no_graph():
    a, e = _engine(runs=3)  # the second sighting captures the shape, the third replays it
    _, fresh = _engine(runs=3)
    cached, replays = e.graphs_cached, e.graph_replays
    assert cached >= 1 and replays >= 1 and e.pause_limit is None
    trim = (40.0, 20.0, 5.0)
    wav = _burst_wav(a, e)  # (the model-rate rows: set again below to force a re-detection)
    # on: one more launch behind the detection, cached with the edges; toggling and re-targeting
    e.set_silence_trim(trim)
    for mp in (MP, 50.0):
        e.set_pause_limit(mp)
        fams = [f for f, _ in _launches(e, lambda: e.batch_fetch_encoded("mulaw"))]
        assert fams[-4:] == ["out.edges_frames", "out.edges_rows", "out.pause_rows", "out.trim_rows"], fams
        e.batch_fetch_joined([6], 100, 0.1)
        fams = [f for f, _ in _launches(e, lambda: e.batch_fetch_encoded("pcm16"))]
        assert fams == ["out.trim_rows"], fams  # (the edges and cuts of this batch and setting are cached)
    assert e.graphs_cached == cached and e.graph_replays == replays
    j = ([2, 4], [100, 7], 0.3)
    # the limit off under trimming, and the limit on without trimming: bytes and launch log of a handle that never set it
    for limit, st in ((None, trim), (MP, None)):
        e.set_pause_limit(limit)
        for x in (e, fresh):
            x.set_silence_trim(st)
        for rate, lo in ((None, None), (16000, -20.0)):
            for x in (e, fresh):
                x.set_output_rate(rate)
                x.set_loudness(lo)
            for enc in ENCS:
                assert _same(e.batch_fetch_encoded(enc)[0], fresh.batch_fetch_encoded(enc)[0]), (limit, rate, lo, enc)
                assert _launches(e, lambda: e.batch_fetch_encoded(enc)) == _launches(fresh, lambda: fresh.batch_fetch_encoded(enc))
            for slot in (0, 1):
                e.fetch_encoded_begin(slot, "pcm16")
                fresh.fetch_encoded_begin(slot, "pcm16")
                assert _same(e.fetch_encoded_end(slot)[0], fresh.fetch_encoded_end(slot)[0])
            assert _same(e.batch_fetch_joined(*j, cut=False)[0], fresh.batch_fetch_joined(*j, cut=False)[0])
            assert _launches(e, lambda: e.batch_fetch_joined(*j)) == _launches(fresh, lambda: fresh.batch_fetch_joined(*j))
            # re-detection under the same setting launches the same kernels on both
            for x in (e, fresh):
                x.dbg_batch_set_wav(wav)
            assert _launches(e, lambda: e.batch_fetch_encoded("pcm16")) == _launches(fresh, lambda: fresh.batch_fetch_encoded("pcm16"))
    e.set_pause_limit(None)
    e.batch_run(2, 1.05, 9)
    assert e.graphs_cached == cached and e.graph_replays == replays + 1  # the next run is a replay
    e.close()
    fresh.close()


def test_the_group_refuses_the_setting():
    g = binding.Group([0])
    try:
        with pytest.raises(binding.StnError) as ei:
            g.set_pause_limit(250)
        assert ei.value.code == -1 and "does not trim" in str(ei.value)
        g.set_pause_limit(None)  # off: nothing to refuse
    finally:
        g.close()


# ---- 5. the hosts ---------------------------------------------------------------------------------------------------------------------------
def test_python_host_cuts_solo_rows_at_len_b():
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    from supertonic_amd.tts import Style, load_text_to_speech
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, noise_seed=21, output_rate=16000, trim_silence=40, max_pause=20)
    assert tts.engine.pause_limit == 20.0
    sttl, sdp = workload.synthetic_styles(default_arch(), [0, 1])
    waves, _ = tts.solo_batch(["Hello there, this is one.", "And this, well, is the other one."], ["en", "en"], Style(sttl, sdp), 2, 1.05)
    ln, nc, _ = tts.engine.batch_pauses(1)
    start, end = tts.engine.batch_silence_edges()
    assert [len(w) for w in waves] == ln.tolist() and np.all(ln <= end - start)
    wav, _, seg = tts.batch(["Hello there."], ["en"], Style(sttl[:1], sdp[:1]), 2, 1.05, lengths=True, max_pause=False)
    s1, e1 = tts.engine.batch_silence_edges()
    assert seg.tolist() == (e1 - s1).tolist() and tts.engine.pause_limit == 20.0  # this call's setting went with the call
    with pytest.raises(ValueError):
        tts.batch(["Hello there."], ["en"], Style(sttl[:1], sdp[:1]), 2, 1.05, max_pause=5)
    tts.engine.close()


def _wav(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[36:40] == b"data"
    return struct.unpack("<i", b[24:28])[0], np.frombuffer(b[44:], dtype="<i2")


def _cli(args, cwd, ok=True):
    p = subprocess.run([CLI, "--synthetic"] + args, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert (p.returncode == 0) == ok, p.stdout + p.stderr
    return p.stdout + p.stderr


def test_cli_writes_the_python_hosts_wave_and_refuses_what_it_must(tmp_path):
    import json
    from supertonic_amd import workload
    from supertonic_amd.arch import default_arch
    from supertonic_amd.tts import Style, load_text_to_speech
    sttl, sdp = workload.synthetic_styles(default_arch(), [0])
    (tmp_path / "voice.json").write_text(json.dumps({"style_ttl": {"data": sttl.astype(np.float64).tolist(), "dims": list(sttl.shape)},
                                                     "style_dp": {"data": sdp.astype(np.float64).tolist(), "dims": list(sdp.shape)}}))
    text = "The chunks are then joined, with a short silence between them. Does it keep the prosody natural? Mostly, yes."
    common = ["--text", text, "--n-test", "1", "--seed", "3", "--total-step", "2", "--voice-style", "voice.json"]
    _cli(common + ["--save-dir", "out", "--trim-silence", "40", "--trim-keep", "10", "--trim-fade", "0", "--max-pause", "20"], tmp_path)
    (f,) = os.listdir(tmp_path / "out")
    sr, pcm = _wav(tmp_path / "out" / f)
    # the Python host on the same seed, style and settings: the file is its wave, len_b samples
    tts = load_text_to_speech("no_assets_here", allow_synthetic=True, noise_seed=3, trim_silence=(40, 10, 0), max_pause=20)
    got, _ = tts(text, "en", Style(sttl, sdp), 2, 1.05, 0.3)
    ln, nc, _ = tts.engine.batch_pauses(1)
    tts.engine.close()
    assert sr == 44100 and pcm.size == got.shape[1] == int(ln.sum())
    assert np.array_equal(pcm, (np.clip(got[0], -1.0, 1.0) * np.float32(32767.0)).astype(np.int16))
    out = _cli(common + ["--save-dir", "no", "--max-pause", "100"], tmp_path, ok=False)
    assert "--max-pause needs --trim-silence" in out
    out = _cli(common + ["--save-dir", "no", "--trim-silence", "40", "--max-pause", "100", "--devices", "0,0"], tmp_path, ok=False)
    assert "does not trim" in out  # a group is refused with a message
    out = _cli(common + ["--save-dir", "no", "--trim-silence", "40", "--max-pause", "5"], tmp_path, ok=False)
    assert "must be in [20, 5000]" in out


# ---- 6. cost --------------------------------------------------------------------------------------------------------------------------------
def test_timing_report_c3_pause():
    """Event-timed cost on the C3-shaped batch of test_gpu_silence.py's test_timing_report_c3_trim (128 rows, native rate), over 10
    fetches after a warm one: out.pause_rows beside out.edges_rows (the detection re-run by alternating the keep), and out.trim_rows
    with and without the limit.  Printed, not asserted; DESIGN.md section 17 records the values."""
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
    B, _, W = e.batch_dims()
    # rows with pauses to cut: every row's span in bursts of 150 ms, 250 ms apart
    sr, F = a.sample_rate, ref.frame(a.sample_rate)
    wav = np.zeros((B, W), np.float32)
    one = pz.burst_row(sr, W, W, [(f, 15) for f in range(2, W // F - 16, 40)], 5)
    for b in range(B):
        nb = min(W, int(np.float32(durs[b] / np.float32(1.05)) * np.float32(sr)))
        wav[b, :nb] = one[:nb]
    e.dbg_batch_set_wav(wav)

    def timed(fetch):
        fetch()  # warm: scratch, tables
        e.profile_enable(True)
        e.profile_reset()
        for _ in range(10):
            fetch()
        prof = e.profile()
        e.profile_enable(False)
        return {k: v["ms"] * 1e3 / max(v["launches"], 1) for k, v in prof.items() if k.startswith("out.")}, {k: v["launches"] for k, v in prof.items()}

    flip = [0]

    def redetect():
        flip[0] ^= 1
        e.set_silence_trim((40.0, 20.0 + flip[0], 5.0))
        e.batch_fetch_encoded("pcm16")

    e.set_silence_trim((40.0, 20.0, 5.0))
    per = {"out.trim_rows (limit off)": timed(lambda: e.batch_fetch_encoded("pcm16"))[0]["out.trim_rows"]}
    e.set_pause_limit(100.0)
    t, launches = timed(lambda: e.batch_fetch_encoded("pcm16"))
    assert launches.get("out.trim_rows") == 10 and "out.pause_rows" not in launches, launches
    per["out.trim_rows (limit on)"] = t["out.trim_rows"]
    t, launches = timed(redetect)
    assert launches.get("out.edges_rows") == 10 and launches.get("out.pause_rows") == 10, launches
    per.update({k: v for k, v in t.items() if k in ("out.edges_frames", "out.edges_rows", "out.pause_rows")})
    ln, nc, _ = e.batch_pauses(1)
    s, en = e.batch_silence_edges()
    print(f"\nC3 batch, pcm16, {B} x {W} samples, {int(nc.sum())} cuts, {int(ln.sum())} of {int((en - s).sum())} trimmed samples delivered: "
          + ", ".join(f"{k} {v:.1f} us" for k, v in sorted(per.items())))
    assert nc.sum() > B  # (the report is about rows that are cut)
    e.close()
