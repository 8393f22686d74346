"""No op-level entry's result depends on what an earlier call left in the engine's arena.

Every output-stage entry runs once on a fresh engine, on 2 rows of W = one workgroup span of chunks + one chunk + three samples
(filter_geometry(): 256 chunks of 32 samples, so W = 8192 + 35), and once more right behind a probing _ex call of another entry on 4
rows of 2 W, which leaves the quiet NaN across a larger arena than the entry takes.  The two results must be equal as bytes: an entry
that read a word no launch of its own wrote, or whose result moved with an address, differs."""
import numpy as np
import pytest

from supertonic_amd import binding

pytestmark = pytest.mark.gpu

HZ = 24000
CHUNK, WG_SPAN = binding.filter_geometry()[:2]
W = WG_SPAN + CHUNK + 3
ROWS = 2


def _rows(rows, width, seed):
    """speech-like rows: voiced bursts (a 140 Hz buzz under a 5.8 kHz hiss) with pauses between them and quiet edges"""
    rng = np.random.default_rng(seed)
    t = np.arange(width) / HZ
    x = np.zeros((rows, width), np.float32)
    for r in range(rows):
        buzz = np.sign(np.sin(2 * np.pi * (140 + 15 * r) * t)) * 0.3 + 0.2 * np.sin(2 * np.pi * 5800 * t)
        on = ((np.arange(width) // (width // 7)) % 2 == 1).astype(np.float64)
        x[r] = (buzz * on * (0.9 - 0.2 * r) + 1e-4 * rng.standard_normal(width)).astype(np.float32)
    return x


X = _rows(ROWS, W, 1)
X.setflags(write=False)
BIG = _rows(4, 2 * W, 2)
BIG.setflags(write=False)
N = np.array([W, W - 2 * CHUNK - 5], np.int64)
FILTERS = [("highpass", 80), ("peak", 3000, 1.0, 4.0), ("highshelf", 6000, 0.7, -3.0)]


def _disturb(eng):
    eng.op_compressor_ex(BIG, HZ, binding.COMPRESSOR_SPEECH, x_misalign=1)


def _disturb_compressor(eng):
    eng.op_silence_edges_ex(BIG, HZ, max_pause_ms=60.0, x_misalign=1)


ENTRIES = {
    "loudness": lambda e: e.op_loudness(X, HZ, N),
    "loudness_range": lambda e: e.op_loudness_range(X, HZ, N),
    "silence_trim": lambda e: e.op_silence_trim(X, HZ, N, gain=[0.5, 1.5], encoding="pcm16"),
    "pause_trim": lambda e: e.op_pause_trim(X, HZ, N, max_pause_ms=20.0, gain=[0.5, 1.5]),
    "true_peak": lambda e: e.op_true_peak(X, HZ, N, gain=[0.5, 1.5]),
    "limiter_sample": lambda e: e.op_limiter(X, HZ, N, gain=[3.0, 4.0]),
    "limiter_true": lambda e: e.op_limiter_ex(X, HZ, N, gain=[3.0, 4.0], peak_mode="true"),
    "filter": lambda e: e.op_filter(X, HZ, FILTERS),
    "compressor": lambda e: e.op_compressor(X, HZ, binding.COMPRESSOR_SPEECH),
    "deesser": lambda e: e.op_deesser(X, HZ, binding.DEESSER_SPEECH),
    "expander": lambda e: e.op_expander(X, HZ, binding.EXPANDER_SPEECH),
    "time_stretch": lambda e: e.op_time_stretch(X, HZ, 9, 8, N),
    "pitch_resample": lambda e: e.op_pitch(X, HZ, 2.0, N),
    "pitch_formant": lambda e: e.op_pitch(X, HZ, 2.0, N, mode="formant"),
    "formant": lambda e: e.op_formant(X, X[::-1], HZ, N),
    "f0": lambda e: e.op_f0(X, HZ, N),
    "resample": lambda e: (e.op_resample(X, HZ, 44100), e.op_resample(X, HZ, 16000, pcm=True)),
    "encode": lambda e: e.op_encode(X, "pcm24"),
    "join": lambda e: e.op_join(X, N, [2], [CHUNK + 1], HZ, encoding="pcm16", loudness=(-23.0, -1.0)),
}


def _arrays(o, path="out"):
    """every array (and string) of a result, named by its place in it"""
    if isinstance(o, dict):
        for k in sorted(o):
            yield from _arrays(o[k], f"{path}[{k!r}]")
    elif isinstance(o, (tuple, list)):
        for i, v in enumerate(o):
            yield from _arrays(v, f"{path}[{i}]")
    elif o is not None:
        yield path, np.ascontiguousarray(o)


def _bytes(o):
    return [(p, a.dtype.str, a.shape, a.tobytes()) for p, a in _arrays(o)]


@pytest.mark.parametrize("name", list(ENTRIES))
def test_result_independent_of_arena_history(name):
    eng = binding.Engine(0, "bf16")
    try:
        fresh = _bytes(ENTRIES[name](eng))
        (_disturb_compressor if name == "compressor" else _disturb)(eng)
        again = _bytes(ENTRIES[name](eng))
    finally:
        eng.close()
    assert len(fresh) == len(again) and fresh
    for (p, dt, shape, a), (_, dt2, shape2, b) in zip(fresh, again):
        assert (dt, shape) == (dt2, shape2), (name, p)
        if a != b:
            u, v = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
            at = np.flatnonzero(u != v)
            pytest.fail(f"{name}: {p} ({dt}, {shape}) differs behind a probing call in {at.size} bytes, the first at byte {int(at[0])}")
