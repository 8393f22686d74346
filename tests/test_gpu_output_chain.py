"""All nine fetch-time stages on at once on an MI355X, against the engine's own ops composed on the host in the documented order
(DESIGN.md sections 11 to 21; Engine::out_source and enqueue_output, engine_batch.cpp): an output rate, a two-filter chain, the
de-esser, the compressor, loudness, the limiter at its longest look-ahead (10 ms), the true-peak mode, silence trimming with a fade and a
pause limit, at 16000 Hz, the native rate and 192000 Hz, on output_walk.busy_rows.  Every op is held against float64 by its own file,
so everything here is byte for byte: a mismatch can only come from order, spans or inputs.

The composition: op_resample, op_filter, op_deesser, op_compressor; the edges and the cuts detected on those rows over the reported
spans (op_silence_edges_ex with the pause limit); loudness measured on the same untrimmed rows over the same spans; the limiter on
(rows x gain) along the true-peak envelope (op_limiter_ex), then its trim gain; the trimmed, faded, pause-cut rows (pause_ref) and their
join (join_ref) on the host; op_encode.  The one hand-off no op expresses is the uncapped gain (with the limiter active the gate's
ceiling is infinite): it is the engine's own, from batch_loudness, checked against 10^((target - LUFS of op_loudness) / 20) within 2^-23
relative and passed on as given.  With one gain per programme, loudness and the limiter run on the joined signal.

Order, on data: at 16000 Hz the composition with two adjacent stages swapped, for every adjacent pair, differs from the engine's bytes
on these rows.

Measured on an MI355X (six rows; samples limited, deepest reductions in dB, cuts, rows with both edges inside, largest gain, true over
sample peak; wall time against the clock alone, the first case with the process's runtime start):
  16000 Hz, 6 x 20063: 3788 limited, limiter 10.4 dB, compressor 12.4 dB, de-esser 11.8 dB, 1 cut, 2 inside, gain 10.3, 1.47 dB; 0.34 s
  44100 Hz, 6 x 55296: 15760 limited, 15.9 dB, 15.1 dB, 12.0 dB, 1 cut, 2 inside, gain 11.8, 2.38 dB; 0.05 s
  192000 Hz, 6 x 240745: 68554 limited, 16.0 dB, 15.0 dB, 12.0 dB, 1 cut, 2 inside, gain 12.2, 0.08 dB; 0.13 s
  the swaps at 16000 Hz: 0.07 s."""
import time

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
import join_ref
import output_walk as ow
import pause_ref

pytestmark = pytest.mark.gpu
BATCH = ow.BATCHES[2]  # six rows: two of each kind of busy_rows
CHAIN = (("highpass", 100.0, 0.7071, 0.0), ("peak", 3000.0, 1.0, 4.0))
DEESS = (5500.0, -30.0, 4.0, 6.0, 1.0, 40.0, 12.0, "split")
COMP = (-24.0, 3.0, 6.0, 5.0, 120.0, 0.0)
TARGET, CEIL, MS = -12.0, -1.0, 10.0
TRIM, PAUSE = (40.0, 20.0, 5.0), 60.0
ENCS = ("pcm16", "mulaw")
JOIN = tuple(ow.join_spec(len(BATCH[0])))
ZERO = {e: binding.ZERO_CODEWORD[binding.ENCODINGS[e]] for e in binding.ENCODINGS}
STAGES = ("resample", "filter", "deesser", "compressor", "edges", "loudness", "limiter", "cut", "encode")


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _engine(rate):
    """the batch with busy_rows as its waveform and every stage on -> (arch, handle, the model-rate rows)"""
    a = tiny_arch()
    lens, durs, seed = BATCH
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    ids, mask, sttl, sdp = make_inputs(a, len(lens), max(lens), lens, seed=seed)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=np.asarray(durs, np.float32))
    e.batch_run(2, ow.SPEED, 9)
    B, L, _ = e.batch_dims()
    W = L * a.base_chunk_size * a.chunk_compress_factor
    raw = ow.busy_rows(a.sample_rate, W, ow.spans(a.sample_rate, W, durs), 43, tone_hz=min(rate, a.sample_rate) / 4.0)
    e.dbg_batch_set_wav(raw)
    e.set_output_rate(None if rate == a.sample_rate else rate)
    e.set_filters(list(CHAIN))
    e.set_deesser(DEESS)
    e.set_compressor(COMP)
    e.set_loudness(TARGET, CEIL)
    e.set_limiter(MS)
    e.set_peak_mode("true")
    e.set_silence_trim(TRIM)
    e.set_pause_limit(PAUSE)
    return a, e, raw


def _front(e, raw, sr, hz, order=STAGES[:4]):
    """the four stages in front, in `order` -> (the rows behind them, the rows in front of the last one and of the last two)"""
    x, rate, before = raw, sr, []
    for stage in order:
        before.append(x)
        if stage == "resample":
            x, rate = (e.op_resample(x, sr, hz) if hz != sr else x), hz
        elif stage == "filter":
            x = e.op_filter(x, rate, list(CHAIN))
        elif stage == "deesser":
            x = e.op_deesser(x, rate, DEESS)
        else:
            x = e.op_compressor(x, rate, COMP)
    return x, before


def _gain(lufs):
    return np.array([np.float32(10.0 ** ((TARGET - float(v)) / 20.0)) for v in lufs], np.float32)


def _cut(x, n, ed, hz, gain=None):
    """pause_ref's delivered rows from the op's edges and cuts -> ([rows, W] float32 with +0.0 behind, the lengths)"""
    y = np.zeros_like(x)
    lens = np.zeros(x.shape[0], np.int64)
    for b in range(x.shape[0]):
        cuts = [tuple(int(v) for v in c) for c in ed["cuts"][b, : ed["n_cuts"][b]]]
        row = pause_ref.delivered_row(x[b], n[b], int(ed["start"][b]), int(ed["end"][b]), cuts, hz, TRIM[2], None if gain is None else gain[b])
        y[b, : row.size], lens[b] = row, row.size
    return y, lens


def _edges(e, x, hz, n):
    return e.op_silence_edges_ex(x, hz, n, TRIM[0], TRIM[1], TRIM[2], max_pause_ms=PAUSE)


def _limit(e, x, hz, n, g):
    return e.op_limiter_ex(x, hz, n, g, CEIL, MS, "true")


def _rows(e, x, hz, n, g, swap=None, detect_on=None):
    """stages 5 to 8 on the rows behind the compressor -> (the delivered fp32 rows, their lengths, the pieces on the way).  swap: the
    first of two adjacent stages that change places."""
    ed = _edges(e, x if detect_on is None else detect_on, hz, n)
    if swap == "loudness":  # the limiter in front of the loudness gain
        lim = _limit(e, x, hz, n, None)
        y = (lim["y"] * lim["trim"][:, None]).astype(np.float32)
        return _cut(y, n, ed, hz, g) + (dict(ed=ed, lim=lim),)
    if swap == "limiter":  # cut first, then limited over what is left
        t, lens = _cut(x, n, ed, hz)
        lim = _limit(e, t, hz, lens, g)
        return (lim["y"] * lim["trim"][:, None]).astype(np.float32), lens, dict(ed=ed, lim=lim)
    lim = _limit(e, x, hz, n, g)
    y, lens = _cut(lim["y"], n, ed, hz, lim["trim"])
    return y, lens, dict(ed=ed, lim=lim)


def _rowmax(gr, n):
    return np.array([gr[b, : n[b]].max() for b in range(len(n))], np.float32)


@pytest.mark.parametrize("rate", [16000, 44100, 192000])
def test_every_fetch_path_is_the_nine_stages_composed_in_the_documented_order(rate):
    t0 = time.perf_counter()
    a, e, raw = _engine(rate)
    sr, hz = a.sample_rate, e.output_rate
    assert hz == rate
    got, dur = e.batch_fetch()
    B, _, Wo = e.batch_dims()
    n = np.array([max(0, min(Wo, int(np.float32(d) * np.float32(hz)))) for d in dur], np.int64)
    # 1 to 4: the rows the level-based steps see, and the two reports on the way
    x, before = _front(e, raw, sr, hz)
    assert x.shape == (B, Wo)
    assert _same(e.batch_deesser(), _rowmax(e.op_deesser_ex(before[2], hz, DEESS)["gr_db"], n))
    assert _same(e.batch_compressor(), _rowmax(e.op_compressor_ex(before[3], hz, COMP)["gr_db"], n))
    # 6: loudness of the untrimmed rows over the spans; the gain is the engine's, held to the formula
    lufs, peak, g = e.batch_loudness()
    op_lufs, op_peak = e.op_loudness(x, hz, n)
    tp = e.op_true_peak(x, hz, n)["tp"]
    assert _same(lufs, op_lufs) and _same(peak, op_peak)  # (with the limiter active the gate keeps the sample peak: nothing caps the gain)
    assert np.all(np.abs(g / _gain(op_lufs).astype(np.float64) - 1.0) <= 2.0 ** -23), (g, _gain(op_lufs))
    # 5, 7, 8: edges and cuts, the limiter on rows x gain, the delivered rows
    want, lens, o = _rows(e, x, hz, n, g)
    ed, lim = o["ed"], o["lim"]
    s_, e_ = e.batch_silence_edges()
    plen, ncut, cuts = e.batch_pauses()
    assert np.array_equal(s_, ed["start"]) and np.array_equal(e_, ed["end"])
    assert np.array_equal(plen, ed["len"]) and np.array_equal(ncut, ed["n_cuts"]) and np.array_equal(cuts, ed["cuts"]) and np.array_equal(plen, lens)
    red, limited = e.batch_limiter()
    assert _same(red, lim["reduction_db"]) and np.array_equal(limited, lim["limited"])
    tp_in, tp_out, trim = e.batch_true_peak()
    assert _same(tp_in, tp) and _same(trim, lim["trim"]) and np.all(tp_out <= 10.0 ** (CEIL / 20.0) * (1.0 + 2.0 ** -20))
    assert _same(got, want), [b for b in range(B) if got[b].tobytes() != want[b].tobytes()]
    # every stage had work to do
    sp = np.array([np.abs(x[b, : n[b]]).max() for b in range(B)])
    figures = dict(limited=int(limited.max()), limiter_db=float(red.max()), compressor_db=float(e.batch_compressor().max()),
                   deesser_db=float(e.batch_deesser().max()), cuts=int(ncut.max()), inside=int(np.sum((s_ > 0) & (e_ < n))), gain=float(g.max()),
                   true_over_sample_db=float((20 * np.log10(tp / sp)).max()))
    assert figures["limited"] > 0 and figures["compressor_db"] > 1.0 and figures["deesser_db"] > 1.0 and figures["cuts"] > 0 and figures["inside"] > 0
    # (a tone at a quarter of the rate: output_walk.busy_rows has the 0.69 dB; rows resampled upwards hold nothing above a quarter of 192 kHz)
    assert np.all(g != 1.0) and figures["true_over_sample_db"] > (0.5 if rate <= sr else 0.0) and np.all(tp >= sp), figures
    # 9: two encodings of the delivered rows, per row and joined with one gain per row
    gap = JOIN[1]
    p = join_ref.plan(JOIN[0], gap, JOIN[2], lens, (lens.astype(np.float32) / np.float32(hz)).astype(np.float32), hz)
    for enc in ("f32",) + ENCS:
        rows = want if enc == "f32" else e.op_encode(want, enc)
        assert _same(e.batch_fetch_encoded(enc)[0], rows), enc
        joined = join_ref.padded(join_ref.join(rows, lens, JOIN[0], gap, ZERO[enc]), p["W_join"], ZERO[enc])
        gj, gl, _ = e.batch_fetch_joined(*JOIN, mode="trim", gain_scope="row", encoding=enc, cut=False)
        assert np.array_equal(gl, p["prog_len"]) and _same(gj, joined), enc
    # one gain per programme: the cut rows joined without a gain, measured and limited as G rows
    plain, _ = _cut(x, n, ed, hz)
    J = join_ref.padded(join_ref.join(plain, lens, JOIN[0], gap, 0.0), p["W_join"], 0.0)
    ng = np.array([max(0, min(int(l), int(np.float32(d) * np.float32(hz)))) for l, d in zip(p["prog_len"], p["prog_dur"])], np.int64)
    jl, jp, jg = e.batch_join_loudness(*JOIN, mode="trim")
    op_jl, op_jp = e.op_loudness(J, hz, ng)
    assert _same(jl, op_jl) and _same(jp, op_jp)
    assert np.all(np.abs(jg / _gain(op_jl).astype(np.float64) - 1.0) <= 2.0 ** -23)
    jlim = _limit(e, J, hz, ng, jg)
    want_prog = (jlim["y"] * jlim["trim"][:, None]).astype(np.float32)
    for enc in ("f32", ENCS[1]):
        gj, gl, _ = e.batch_fetch_joined(*JOIN, mode="trim", gain_scope="programme", encoding=enc, cut=False)
        assert np.array_equal(gl, p["prog_len"]) and _same(gj, want_prog if enc == "f32" else e.op_encode(want_prog, enc)), enc
    assert jlim["limited"].max() > 0
    e.close()
    print(f"\n{rate} Hz, {B} x {Wo}: {figures}; programmes: {int(jlim['limited'].max())} samples limited; {time.perf_counter() - t0:.2f} s")


def test_swapping_two_adjacent_stages_changes_the_bytes():
    """(module docstring) a composition that commutes on these rows would prove nothing about the order: none does"""
    rate = 16000
    a, e, raw = _engine(rate)
    sr, hz = a.sample_rate, e.output_rate
    got, dur = e.batch_fetch()
    got_enc = e.batch_fetch_encoded("mulaw")[0]
    B, _, Wo = e.batch_dims()
    n = np.array([max(0, min(Wo, int(np.float32(d) * np.float32(hz)))) for d in dur], np.int64)
    g = e.batch_loudness()[2]
    x, before = _front(e, raw, sr, hz)
    assert _same(got, _rows(e, x, hz, n, g)[0])  # (the order as it is gives the engine's bytes)
    # 1-2, 2-3, 3-4: two of the four in front change places; the gain is then the formula's, of the rows that come out
    for k in range(3):
        order = list(STAGES[:4])
        order[k], order[k + 1] = order[k + 1], order[k]
        xs, _ = _front(e, raw, sr, hz, order)
        assert xs.shape == x.shape and not _same(xs, x), order
        gs = _gain(e.op_loudness(xs, hz, n)[0])
        assert not _same(_rows(e, xs, hz, n, gs)[0], got), order
    # 4-5: the edges and cuts detected in front of the compressor
    y, lens, o = _rows(e, x, hz, n, g, detect_on=before[3])
    assert not _same(y, got) and not (np.array_equal(o["ed"]["start"], e.batch_silence_edges()[0]) and np.array_equal(o["ed"]["len"], e.batch_pauses()[0]))
    # 5-6: loudness measured behind the cut, on what is left
    ed = _edges(e, x, hz, n)
    t, lens = _cut(x, n, ed, hz)
    gs = _gain(e.op_loudness(t, hz, lens)[0])
    assert not _same(gs, g) and not _same(_rows(e, x, hz, n, gs)[0], got)
    # 6-7 and 7-8: the limiter in front of the gain; the cut in front of the limiter
    for swap in ("loudness", "limiter"):
        assert not _same(_rows(e, x, hz, n, g, swap=swap)[0], got), swap
    # 8-9: encoded first, then cut (a codeword cannot be faded)
    lim = _limit(e, x, hz, n, g)
    enc = e.op_encode((lim["y"] * lim["trim"][:, None]).astype(np.float32), "mulaw")
    late = np.full_like(enc, ZERO["mulaw"])
    for b in range(B):
        cuts = [tuple(int(v) for v in c) for c in ed["cuts"][b, : ed["n_cuts"][b]]]
        row = np.concatenate([enc[b, lo:hi] for lo, hi in pause_ref.segments(int(ed["start"][b]), int(ed["end"][b]), cuts)])
        late[b, : row.size] = row
    assert not _same(late, got_enc)
    e.close()
