"""The output stage's kept state under histories of settings on an MI355X (output_walk.py has the model, the steps and the walks;
test_output_walk_cpu.py shows that a key short of one field fails them): a fetch depends on the finished waveform and the settings in
force, and on nothing the handle did before.  One live handle (tiny arch, bf16, length-aware vocoder) plays a walk; after every step a
fresh handle is created, loaded, given the step's batch and waveform and the step's settings once, in a fixed order, and everything the
two deliver must be equal in dtype, shape and bytes: batch_fetch, two encodings that rotate through the five, a pipelined slot fetch, a
device copy into a sentinel-filled buffer of odd stride, the joined fetch in both gain scopes, batch_join_loudness,
batch_join_loudness_range and all eight reports (a refused report must be refused by both with one code; the rows are about a second
long, short against the loudness range's 3 s window, which both handles then report alike).  A refused set call must raise and change nothing; graphs_cached and
graph_replays of the live handle move on a batch step only.  A failure prints the seed, the walk, the step and the history up to it as
a list that output_walk's steps replay, with the output and the row that differ.

Over each walk the fresh handles' own results show every stage a walk enables at work (samples limited, dB taken off by the compressor
and the de-esser, edges inside a span, pauses cut, a gain other than 1, a true peak over the sample peak); every walk prints its figures.
Two figures are taken at every step that enables them, on the fresh handle once the comparison is over: `shifted`, the largest |fp32
fetch - the same fetch with pitch off|, and `dithered`, the PCM16 samples that differ from the same fetch with dither off (at the steps
whose encoded fetches hold a PCM encoding); either must be above 0 at every such step.

Cost, measured on an MI355X against the clock alone: a fresh handle is 7 ms to create and load, 1.2 ms to upload and run its batch and
2 ms to take (the process's first handle adds 1.7 s of runtime start, once); a step with both takes and the host's comparison comes to
20 to 45 ms, a walk of 16 steps to 0.55 to 0.75 s, and the file's five walks to 4.1 s of wall time with the start.  With pitch, dither
and the loudness-range outputs in every comparison: the seven walks take 0.65 to 0.80 s each (walk 5, whose every fresh handle shifts
its batch and whose two op steps stretch 2 x 120011 samples, 0.80 s; walk 6 0.77 s), and the file 6.5 s of wall time with the start.
A fresh handle per step fits: every step is compared.  The five walks of then were played the same way for 25 more seeds (2000
steps), walks 5 and 6 for 12 more (384 steps, 0.25 to 0.41 s a walk once the process is warm), and met no difference."""
import time

import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.arch import tiny_arch
from gpu_util import make_inputs
import output_walk as ow

pytestmark = pytest.mark.gpu
SEED = 0
_SETTERS = dict(
    rate=lambda e, v: e.set_output_rate(v),
    filters=lambda e, v: e.set_filters(list(v) or None),
    deesser=lambda e, v: e.set_deesser(v),
    compressor=lambda e, v: e.set_compressor(v),
    loudness=lambda e, v: e.set_loudness(None) if v is None else e.set_loudness(*v),
    limiter=lambda e, v: e.set_limiter(v),
    peak=lambda e, v: e.set_peak_mode(v),
    trim=lambda e, v: e.set_silence_trim(v),
    pause=lambda e, v: e.set_pause_limit(v),
    pitch=lambda e, v: e.set_pitch(v),
    dither=lambda e, v: e.set_dither(v),
)
# the five whose out-of-range values the binding's own parsers stop: through the C ABI itself, so that the engine is the one to refuse
_RAW = dict(
    limiter=lambda e, v: e._ck(e._lib.stn_set_limiter(e._h, 1, float(v))),
    trim=lambda e, v: e._ck(e._lib.stn_set_silence_trim(e._h, 1, *(float(x) for x in v))),
    pause=lambda e, v: e._ck(e._lib.stn_set_pause_limit(e._h, 1, float(v))),
    pitch=lambda e, v: e._ck(e._lib.stn_set_pitch(e._h, float(v))),
    dither=lambda e, v: e._ck(e._lib.stn_set_dither(e._h, int(v[0]), int(v[1]))),
)
_WAVS = {}


def _handle(a):
    e = binding.Engine(0, "bf16")
    e.load_synthetic(a, 7)
    e.set_vocoder_mode(1)
    return e


def _run_batch(a, e, index):
    lens, durs, seed = ow.BATCHES[index]
    ids, mask, sttl, sdp = make_inputs(a, len(lens), max(lens), lens, seed=seed)
    e.batch_upload(ids, mask, sttl, sdp, duration_override=np.asarray(durs, np.float32))
    e.batch_run(2, ow.SPEED, 9)


def _set_wav(a, e, state):
    B, L, _ = e.batch_dims()
    W = L * a.base_chunk_size * a.chunk_compress_factor
    key = (state["batch"], state["wav"], W)
    if key not in _WAVS:
        _WAVS[key] = ow.busy_rows(a.sample_rate, W, ow.spans(a.sample_rate, W, ow.BATCHES[state["batch"]][1]), state["wav"])
        _WAVS[key].setflags(write=False)
    e.dbg_batch_set_wav(_WAVS[key])


def _fresh(a, state):
    """a handle that has done nothing but reach the state"""
    e = _handle(a)
    _run_batch(a, e, state["batch"])
    _set_wav(a, e, state)
    for name in ow.SETTINGS:
        _SETTERS[name](e, state[name])
    return e


def _op_rows(variant, most=7):
    rows, W = ((3, 5000), (min(most, 7), 120011))[variant]
    t = np.arange(W)
    x = np.stack([(0.2 + 0.1 * r) * np.sin(t / (7.0 + r)) * ((t // 1500) % 3 != 1) for r in range(rows)]).astype(np.float32)
    x[:, ::997] = 0.95
    return x, np.array([W - 17 * r for r in range(rows)], np.int64)


def _op(e, family, variant):
    """one op-level call on rows that have nothing to do with the batch"""
    # (the two stretches search their rows frame by frame, a workgroup per row: two rows in variant 1, about 295 and 200 frames each)
    x, n = _op_rows(variant, most=2 if family in ("time_stretch", "pitch") else 7)
    hz = (16000, 48000)[variant]
    rows = x.shape[0]
    if family == "resample":
        e.op_resample(x, 44100, hz)
    elif family == "filter":
        e.op_filter(x, hz, [("highpass", 100.0), ("peak", 2000.0, 1.0, 3.0), ("lowpass", 6000.0)])
    elif family == "deesser":
        e.op_deesser(x, hz, binding.DEESSER_SPEECH)
    elif family == "compressor":
        e.op_compressor(x, hz, binding.COMPRESSOR_SPEECH)
    elif family == "loudness":
        e.op_loudness(x, hz, n)
    elif family == "true_peak":
        e.op_true_peak(x, hz, n)
    elif family == "limiter":
        e.op_limiter_ex(x, hz, n, np.full(rows, 1.5, np.float32), -1.0, 3.0, "true")
    elif family == "edges":
        if variant:
            e.op_pause_trim(x, hz, n, 30.0, 10.0, 2.0, 40.0)
        else:
            e.op_silence_edges(x, hz, n, 30.0, 10.0)
    elif family == "join":
        e.op_join(x, n, [rows - 1, 1], 50, hz, encoding="pcm16", loudness=(-20.0, -1.0))
    elif family == "encode":
        e.op_encode(x, "mulaw")
    elif family == "time_stretch":
        e.op_time_stretch(x, hz, 5, 4, n=n)
    elif family == "pitch":
        e.op_pitch(x, hz, -3.0, n=n)
    elif family == "loudness_range":
        e.op_loudness_range(x, hz, n)
    elif family == "encode_ex":
        e.op_encode_ex(x, "pcm16", dither="tpdf-hp", seed=3, gain=np.full(rows, 0.5, np.float32))
    else:
        raise KeyError(family)


def _copy(e, enc, B, Wo):
    """batch_copy_encoded_device into a sentinel-filled buffer of odd stride -> the rows; the sentinel behind every row is checked here"""
    from hip_util import DeviceBuffer
    stride = Wo + 3 - Wo % 2
    like = binding.encoded_empty(enc, B, stride)
    like[...] = 0x5A if like.dtype == np.uint8 else -7
    d = DeviceBuffer(like)
    e.batch_copy_encoded_device(enc, d.ptr, stride)
    e.sync()
    back = d.to_host()
    assert np.array_equal(back[:, Wo:], like[:, Wo:]), "the device copy wrote behind a row"
    return np.ascontiguousarray(back[:, :Wo])


def _one(e, name, i, state):
    B, _, Wo = e.batch_dims()
    join = ow.join_spec(B)
    mode = "trim" if state["trim"] else "whole"
    encs = ow.encodings(i)
    if name == "f32":
        return e.batch_fetch()
    if name in ("enc0", "enc1"):
        return e.batch_fetch_encoded(encs[int(name[-1])])
    if name == "slot":
        e.fetch_encoded_begin(i % 2, encs[1])
        return e.fetch_encoded_end(i % 2)
    if name == "copy":
        return (_copy(e, encs[0], B, Wo),)
    if name in ow.JOINED:
        return e.batch_fetch_joined(*join, mode=mode, gain_scope=name[5:], encoding=encs[0] if name == "join_row" else None, cut=False)
    if name == "join_loudness":
        return e.batch_join_loudness(*join, mode=mode)
    if name == "join_loudness_range":
        return e.batch_join_loudness_range(*join, mode=mode)
    r = getattr(e, "batch_" + name)()
    return (r,) if isinstance(r, np.ndarray) else r


def _take(e, i, state):
    """every output of take_order(i), as name -> tuple of arrays, or ("refused", code)"""
    out = {}
    for name in ow.take_order(i):
        try:
            out[name] = tuple(np.asarray(v) for v in _one(e, name, i, state))
        except binding.StnError as err:
            out[name] = ("refused", err.code)
    return out


def _first_difference(got, want):
    """(output, part, row) of the first output that differs, or None"""
    assert got.keys() == want.keys()
    for k in want:
        g, w = got[k], want[k]
        if g and isinstance(g[0], str) or w and isinstance(w[0], str):
            if g != w:
                return k, g, w
            continue
        for part, (x, y) in enumerate(zip(g, w)):
            if x.shape != y.shape or x.dtype != y.dtype:
                return k, part, (x.shape, x.dtype, y.shape, y.dtype)
            if x.tobytes() != y.tobytes():
                rows = [r for r in range(x.shape[0]) if x[r].tobytes() != y[r].tobytes()] if x.ndim else []
                return k, part, rows
    return None


def _fetch_step(e, path, state):
    name = {"enc": "enc0", "join_programme": "join_programme", "join_row": "join_row"}.get(path, path)
    _one(e, name, 0, state)


def _play(a, e, state, step):
    """one step on the live handle -> the state behind it"""
    kind = step[0]
    if kind == "set":
        _SETTERS[step[1]](e, step[2])
    elif kind == "batch":
        _run_batch(a, e, step[1])
        _set_wav(a, e, ow.apply(state, step))
    elif kind == "wav":
        _set_wav(a, e, ow.apply(state, step))
    elif kind == "op":
        _op(e, step[1], step[2])
    elif kind == "refuse":
        with pytest.raises(binding.StnError) as ei:
            _RAW.get(step[1], _SETTERS[step[1]])(e, step[2])
        assert ei.value.code == -1, (step, str(ei.value))
    elif kind == "fetch":
        _fetch_step(e, step[1], state)
    return ow.apply(state, step)


def _busy(busy, state, want, f, i):
    """what the fresh handle's results show of the stages the state enables (the comparison is over: the fresh handle is asked once
    more with one setting off, for the figures that need the other fetch)"""
    on = lambda n: state[n] != ow.OFF[n]  # noqa: E731
    B, _, Wo = f.batch_dims()
    if on("dither") and {"pcm16", "pcm24"} & set(ow.encodings(i)):
        with_dither = f.batch_fetch_encoded("pcm16")[0]
        f.set_dither(None)
        n = int(np.count_nonzero(with_dither != f.batch_fetch_encoded("pcm16")[0]))
        assert n > 0, "dither on and no PCM16 sample differs from the fetch without"
        busy["dithered"] = max(busy.get("dithered", 0), n)
    if on("pitch"):
        with_pitch = f.batch_fetch()[0]
        f.set_pitch(None)
        d = float(np.abs(with_pitch - f.batch_fetch()[0]).max())
        f.set_pitch(state["pitch"])  # (the figures below are the shifted rows')
        assert d > 0.0, "pitch on and the fp32 fetch is the one without"
        busy["shifted"] = max(busy.get("shifted", 0.0), d)
    if on("loudness"):
        busy["gain"] = max(busy.get("gain", 0.0), float(np.abs(want["loudness"][2] - 1.0).max()))
        if on("limiter"):
            busy["limited"] = max(busy.get("limited", 0), int(want["limiter"][1].max()))
        if on("peak") and "true_peak_over_sample_db" not in busy:
            tp = want["true_peak"][0]
            f.set_peak_mode("sample")  # (once more, for the sample peaks)
            sp = f.batch_loudness()[1]
            busy["true_peak_over_sample_db"] = float((20 * np.log10(tp / sp)).max())
    if on("compressor"):
        busy["compressor_db"] = max(busy.get("compressor_db", 0.0), float(want["compressor"][0].max()))
    if on("deesser"):
        busy["deesser_db"] = max(busy.get("deesser_db", 0.0), float(want["deesser"][0].max()))
    if on("trim"):
        start, end = want["silence_edges"]
        n = np.array([min(Wo, int(np.float32(d) * np.float32(f.output_rate))) for d in want["f32"][1]])
        busy["edges_inside"] = max(busy.get("edges_inside", 0), int(np.sum((start > 0) & (end < n) & (end > start))))
        if on("pause"):
            busy["cuts"] = max(busy.get("cuts", 0), int(want["pauses"][1].max()))


_NEEDS = dict(gain=("loudness",), limited=("loudness", "limiter"), true_peak_over_sample_db=("loudness", "peak"), compressor_db=("compressor",),
              deesser_db=("deesser",), edges_inside=("trim",), cuts=("trim", "pause"), shifted=("pitch",), dithered=("dither",))


def _walk(w, walk):
    a = tiny_arch()
    e = _handle(a)
    state = ow.start()
    _run_batch(a, e, state["batch"])
    _set_wav(a, e, state)
    busy = {}
    enabled = set()
    t0 = time.perf_counter()
    for i, step in enumerate(walk):
        counters = (e.graphs_cached, e.graph_replays)
        state = _play(a, e, state, step)
        got = _take(e, i, state)
        after = (e.graphs_cached, e.graph_replays)
        f = _fresh(a, state)
        want = _take(f, i, state)
        diff = _first_difference(got, want)
        history = f"seed {SEED}, walk {w}, step {i} {step!r}; replay with output_walk's steps:\n{walk[:i + 1]!r}"
        assert diff is None, f"output {diff[0]!r}, part {diff[1]}, rows {diff[2]} differ from a fresh handle's\n{history}"
        assert after == counters or step[0] == "batch", f"graphs_cached / graph_replays went {counters} -> {after}\n{history}"
        _busy(busy, state, want, f, i)
        for k, needs in _NEEDS.items():
            if all(state[n] != ow.OFF[n] for n in needs) and (k != "dithered" or {"pcm16", "pcm24"} & set(ow.encodings(i))):
                enabled.add(k)
        f.close()
    e.close()
    print(f"\nwalk {w}: {len(walk)} steps in {time.perf_counter() - t0:.2f} s; at work: {busy}")
    idle = [k for k in enabled if not busy.get(k, 0) > 0]
    assert not idle, f"walk {w}: enabled and never at work: {idle}; {busy}"


@pytest.mark.parametrize("w", list(range(ow.N_WALKS)) + sorted(ow.REGRESSIONS))
def test_a_history_of_settings_fetches_what_a_fresh_handle_fetches(w):
    """the seeded walks, and by name the histories that once failed (output_walk.REGRESSIONS)"""
    _walk(w, ow.REGRESSIONS[w] if w in ow.REGRESSIONS else ow.walks(SEED)[w])


def test_every_setting_and_every_trim_field_changes_what_a_fresh_handle_delivers():
    """(the comparison has something to see: on these rows, with everything on, a fresh handle one value away delivers other bytes, so
    a handle that kept the value before would be found out)"""
    a = tiny_arch()
    base = dict(ow.start(), batch=2, rate=24000, peak="true", pause=60.0,
                **{n: ow.VALUES[n][0] for n in ("filters", "deesser", "compressor", "loudness", "limiter", "trim", "pitch", "dither")})
    f = _fresh(a, base)
    want = _take(f, 0, base)
    f.close()
    others = [(n, [v for v in ow.VALUES[n] + (ow.OFF[n],) if v != base[n]][0]) for n in ow.SETTINGS] + [("trim", v) for v in ow.VALUES["trim"][2:]] + [("wav", 77)]
    for name, value in others:
        state = dict(base, **{name: value})
        f = _fresh(a, state)
        assert _first_difference(_take(f, 0, state), want) is not None, (name, value)
        f.close()
