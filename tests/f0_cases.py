"""The pitch report's case rows: one launch of rows per rate at 8, 16, 44.1, 48 and 192 kHz (k = 1, 1, 2, 3, 12),
each row at most 0.6 s, W padded behind the longest span and everything behind each span poisoned with NaN.  case_rows(hz, G) takes the
track kernel's group size G (binding.f0_group()[0]) for the rows that sit on the workgroup seam; refs(hz, G) is the float64 reference
of every row, computed once."""
import functools

import numpy as np

import f0_ref as ref

RATES = (8000, 16000, 44100, 48000, 192000)
NAMES = ("span 0", "one sample short of a frame", "exactly one frame", "G frames", "G + 1 frames", "n not a multiple of k", "sine 70 Hz", "sine 150 Hz",
         "sine 450 Hz", "octave trap 120 Hz", "glide 100-300 Hz", "noise", "200 Hz, last third silent")
TONES = {6: 70.0, 7: 150.0, 8: 450.0}  # row -> the pure tone's frequency
GLIDE, NOISE = 10, 11
PAD = 37
_ROWS, _REFS = {}, {}


def harmonic(hz, n, f, amps=(0.2, 0.07, 0.03)):
    t = np.arange(n) / hz
    return sum(a * np.sin(2 * np.pi * f * (h + 1) * t) for h, a in enumerate(amps))


def case_rows(hz, G):
    """(x [13, W] float32 with NaN behind each span, n [13] int64)"""
    if (hz, G) in _ROWS:
        return _ROWS[hz, G]
    g = ref.plan(hz, 0)
    k, hop, T = g["k"], g["hop"], g["tau_max"]
    full = int(0.6 * hz)
    frame = 2 * T * k  # the samples of exactly one frame

    def frames(c):  # the shortest span of c frames
        return ((c - 1) * hop + 2 * T) * k

    t = np.arange(full) / hz
    glide_T = full / hz
    phase = 2 * np.pi * 100.0 * glide_T / np.log(3.0) * (3.0 ** (t / glide_T) - 1.0)
    tone200 = 0.3 * np.sin(2 * np.pi * 200.0 * t)
    tone200[2 * full // 3:] = 0.0
    odd = (int(0.3 * hz) // k) * k + (k - 1)
    rows = [
        (np.zeros(0), 0),
        (harmonic(hz, frame - 1, 110.0), frame - 1),
        (harmonic(hz, frame, 110.0), frame),
        (harmonic(hz, frames(G), 110.0), frames(G)),
        (harmonic(hz, frames(G + 1), 110.0), frames(G + 1)),
        (harmonic(hz, odd, 130.0), odd),
        (0.3 * np.sin(2 * np.pi * 70.0 * t), full),
        (0.3 * np.sin(2 * np.pi * 150.0 * t), full),
        (0.3 * np.sin(2 * np.pi * 450.0 * t), full),
        (0.075 * np.sin(2 * np.pi * 120.0 * t) + 0.225 * np.sin(2 * np.pi * 240.0 * t), full),
        (0.3 * np.sin(phase) + 0.1 * np.sin(2 * phase), full),
        (0.1 * np.random.default_rng(hz).standard_normal(full), full),
        (tone200, full),
    ]
    assert len(rows) == len(NAMES) and all(c <= full for _, c in rows)
    n = np.array([c for _, c in rows], np.int64)
    x = np.full((len(rows), int(n.max()) + PAD), np.nan, np.float32)
    for r, (v, c) in enumerate(rows):
        x[r, :c] = v[:c]
    x.setflags(write=False)
    n.setflags(write=False)
    _ROWS[hz, G] = (x, n)
    return x, n


def refs(hz, G):
    """per row: dict f0, ap, lag (float64 / int32 [frames]), det (f0_ref.track's detail), plan"""
    if (hz, G) not in _REFS:
        x, n = case_rows(hz, G)
        out = []
        for r in range(len(n)):
            f0, ap, lag, det = ref.track(x[r, : n[r]], hz, detail=True)
            out.append({"f0": f0, "ap": ap, "lag": lag, "det": det, "plan": ref.plan(hz, int(n[r]))})
        _REFS[hz, G] = out
    return _REFS[hz, G]


PITCH_HZ, PITCH_F = 44100, 150.0  # the row the pitch stage is measured on: a 150 Hz harmonic tone of 0.6 s at 44.1 kHz


def pitch_row():
    return harmonic(PITCH_HZ, int(0.6 * PITCH_HZ), PITCH_F).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pitch_chain(semitones):
    """the float64 chain: tests/pitch_ref.py's shift of the row (the library's ratio and taps), rounded to float32 -> (y, (a, b))"""
    from supertonic_amd import binding
    import formant_cases
    import pitch_ref as pr
    a, b = binding.pitch_ratio(semitones)
    y, _ = pr.pitch(pitch_row(), None, PITCH_HZ, a, b, formant_cases.taps(a, b))
    return y.astype(np.float32), (a, b)


def undecidable(hz, G):
    """per row the frames that are not decidable (f0_ref.decidable)"""
    return [[t for t in range(len(w["lag"])) if not ref.decidable(w["det"][t], int(w["lag"][t]), w["plan"])] for w in refs(hz, G)]
