"""Histories of the output stage for the walk tests (test_output_walk_cpu.py, test_gpu_output_walk.py, test_gpu_output_chain.py): a model
of everything a fetch may depend on (the state), the steps that change it or must not, a seeded generator of fixed histories (walks) that
hold every cached-reuse situation of the stage, the order in which a comparison takes a handle's outputs, and rows that keep all the
fetch-time stages busy.  No GPU and no library: plain Python and numpy.

A state is a dict: batch (index into BATCHES), wav (the seed of the rows dbg_batch_set_wav is given) and the eleven SETTINGS.  A step is a
tuple:
    ("set", name, value)      one setting to another valid value, to OFF[name], or back to an earlier value
    ("batch", index)          upload and run BATCHES[index], then dbg_batch_set_wav with the state's seed
    ("wav", seed)             dbg_batch_set_wav alone
    ("op", family, variant)   one op-level call on unrelated rows (OPS); variant 0: few short rows at 16 kHz, 1: more and longer rows
                              than any batch's at 48 kHz (every grow-only buffer the op shares with the batch path moves)
    ("refuse", name, value)   a set call the engine must refuse: the state stays
    ("fetch", path)           one fetch by one path (PATHS), nothing changed
After every step the GPU walk compares the live handle with a fresh one, taking the outputs in the order take_order(i) gives for step i:
the reports in front of the fetches on even steps (a report is then the first to meet whatever the step left stale), behind them on odd
ones.  In every order a joined fetch of each gain scope stands directly behind one per-row fetch and directly in front of another.
walks(seed) deals the settings, the op families, the batches and the other steps over N_WALKS histories, draws values and the
interleaving from the seed, and keeps the first draw in which the situations _wanted() names occur.  Walks 0 to 4 are step for step
what they were before pitch, dither and the loudness-range outputs existed (test_output_walk_cpu.py pins them); walk 5 plays the pitch
under compressor, de-esser, trimming and loudness, walk 6 dither beside the rate with loudness going off and on."""
import math
import random

import numpy as np

import limiter_ref

NATIVE_HZ = 44100  # the tiny arch's rate: the refused low-pass of a walk is placed by it
SPEED = 1.05
# (token lengths, forced durations, seed), of unlike B and W; the first two of one W (their longest rows are equally long), so that going
# from one to the other changes the row count alone.  Every first row of three is long enough for busy_rows' phrase.
BATCHES = (
    ([9, 6], (0.97, 0.72), 3),
    ([7, 11, 5], (0.97, 0.78, 0.84), 5),
    ([14, 9, 5, 12, 7, 11], (1.30, 1.10, 0.88, 1.21, 1.02, 0.91), 2),
)
SETTINGS = ("rate", "filters", "deesser", "compressor", "loudness", "limiter", "peak", "trim", "pause", "pitch", "dither")
OFF = dict(rate=None, filters=(), deesser=None, compressor=None, loudness=None, limiter=None, peak="sample", trim=None, pause=None, pitch=None,
           dither=None)
# the ratios a / b the three shifts are realised with (include/stn.h "pitch": the closest fraction to 2^(s / 12) with terms up to 640; the
# shifts are the ratios' own semitones, so the fractions are exact).  None of them is an octave.  The first shares its b with the second and its a
# with the third: the resample table of the way back is kept per (a, b), and a walk goes from the first to either neighbour, so that a
# table looked up by one term alone is a wrong one
PITCH_RATIOS = ((5, 4), (3, 4), (5, 3))
# the values a walk draws (include/stn.h's ranges; every chain and de-esser is valid at every rate drawn, so that no rate change is refused).
# trim[1:] each differ from trim[0] in one field; the largest pause limit is shorter than busy_rows' pause
VALUES = dict(
    rate=(16000, 24000, 48000),
    filters=((("highpass", 80.0, 0.7071, 0.0),),
             (("highpass", 120.0, 0.7071, 0.0), ("peak", 3000.0, 1.0, 4.0)),
             (("lowshelf", 200.0, 0.7071, -3.0), ("lowpass", 7000.0, 0.7071, 0.0), ("notch", 1000.0, 2.0, 0.0))),
    deesser=((5500.0, -30.0, 4.0, 6.0, 1.0, 40.0, 12.0, "split"), (4000.0, -36.0, 10.0, 0.0, 0.1, 10.0, 24.0, "wide"),
             (6000.0, -28.0, 4.0, 6.0, 1.0, 40.0, 12.0, "split")),
    compressor=((-24.0, 3.0, 6.0, 5.0, 120.0, 0.0), (-12.0, 2.0, 0.0, 1.0, 50.0, 0.0), (-20.0, 4.0, 6.0, 5.0, 120.0, 3.0)),
    loudness=((-12.0, -1.0), (-14.0, -2.0), (-10.0, -1.5)),  # (every target above busy_rows' loudness: a gain above 1, and clicks to limit)
    limiter=(5.0, 2.0, 10.0),
    peak=("true",),
    trim=((40.0, 20.0, 5.0), (30.0, 20.0, 5.0), (40.0, 10.0, 5.0), (40.0, 20.0, 0.0)),
    pause=(60.0, 150.0),
    pitch=tuple(12.0 * math.log2(a / b) for a, b in PITCH_RATIOS),  # +3.86, -4.98 and +8.84 semitones
    dither=(("tpdf", 7), ("tpdf", 8), ("round", 0), ("tpdf-hp", 7)),  # (mode, seed): the first two differ in the seed alone
)
PAUSE_S = 0.26  # busy_rows' pause: longer than max(VALUES["pause"]) ms plus twice the longest keep
# what the engine refuses (include/stn.h); the low-pass is placed above Nyquist of the rate in force by refused()
REFUSED = dict(rate=7000, limiter=11.0, loudness=(1.0, -1.0), trim=(0.5, 20.0, 5.0), pause=10.0,
               compressor=(-24.0, 30.0, 6.0, 5.0, 120.0, 0.0), deesser=(13000.0, -30.0, 4.0, 6.0, 1.0, 40.0, 12.0, "split"),
               pitch=12.5, dither=(4, 7))  # (semitones outside [-12, 12]; a mode behind the last, STN_DITHER_TPDF_HP = 3, with a seed)
# the first ten are shuffled and dealt over walks 0 to 4 two each, the last four go to walks 5 and 6 as they stand
OPS = ("resample", "filter", "deesser", "compressor", "loudness", "true_peak", "limiter", "edges", "join", "encode",
       "time_stretch", "pitch", "loudness_range", "encode_ex")
N_SHUFFLED_OPS = 10
PATHS = ("f32", "enc", "slot", "copy", "join_programme", "join_row")
ENCODINGS = ("f32", "pcm16", "pcm24", "mulaw", "alaw")
REPORTS = ("compressor", "deesser", "silence_edges", "pauses", "loudness", "limiter", "true_peak", "loudness_range")
FETCHES = ("f32", "join_programme", "enc0", "join_row", "enc1", "slot", "copy", "join_loudness", "join_loudness_range")
PER_ROW, JOINED = ("f32", "enc0", "enc1", "slot", "copy"), ("join_programme", "join_row")
N_WALKS = 7


def take_order(i):
    """The outputs a comparison takes after step i, in order.  Even steps: the reports, then the fetches.  The compressor's and the
    de-esser's report read maxima that every other output computes afresh on its way, and either one, when it finds nothing kept,
    refreshes the other's: they come first, the compressor's in front on every fourth step and the de-esser's on the others.  Odd steps:
    the fetches, then the reports the other way round, so that whatever reads the edges last in one comparison reads them first in the
    next under the same pause limit (batch_pauses asks for the cuts whether the limit is on or off, and one set of edges is kept)."""
    if i % 2:
        return FETCHES + REPORTS[::-1]
    return (REPORTS[1::-1] if i % 4 else REPORTS[:2]) + REPORTS[2:] + FETCHES


def encodings(i):
    """the two encodings of step i's encoded fetches: both rotate through the five along a walk"""
    return ENCODINGS[i % 5], ENCODINGS[(i + 2) % 5]


def join_spec(B):
    """(rows, gap_samples, gap_seconds) of the joined fetches of a batch of B rows: two programmes"""
    return [B - B // 2, B // 2], [120, 60], [0.1, 0.05]


def start():
    s = dict(OFF)
    s.update(batch=0, wav=41)
    return s


def rate_of(state):
    return state["rate"] or NATIVE_HZ


def pitch_ratio(value):
    """(a, b) of a pitch value of VALUES (1, 1 for off)"""
    return (1, 1) if value is None else PITCH_RATIOS[VALUES["pitch"].index(value)]


def refused(state, name):
    """the value of a ("refuse", name, value) step in this state"""
    if name == "filters":
        return (("lowpass", 0.5 * rate_of(state) + 100.0, 0.7071, 0.0),)
    return REFUSED[name]


def apply(state, step):
    """the state behind a step (a new dict); ValueError for a step that is none"""
    s = dict(state)
    kind = step[0]
    if kind == "set":
        if step[1] not in SETTINGS:
            raise ValueError(step)
        s[step[1]] = step[2]
    elif kind == "batch":
        s["batch"] = step[1]
    elif kind == "wav":
        s["wav"] = step[1]
    elif kind not in ("op", "refuse", "fetch"):
        raise ValueError(step)
    return s


def states(walk):
    """the state behind every step of a walk"""
    out, s = [], start()
    for step in walk:
        s = apply(s, step)
        out.append(s)
    return out


def frozen(state):
    return tuple(sorted((k, repr(v)) for k, v in state.items()))


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
def _script(name, rng, pairs):
    """one setting's steps as atoms (lists of steps that stay together, in order): on, `pairs` times (another value, back), off, on again"""
    vals = list(VALUES[name])
    a = vals[0] if name == "trim" else rng.choice(vals)
    others = [v for v in vals if v != a] or [OFF[name]]
    if name != "trim":
        rng.shuffle(others)
    atoms = [[("set", name, a)]]
    for k in range(pairs):
        atoms.append([("set", name, others[k % len(others)]), ("set", name, a)])
    atoms.append([("set", name, OFF[name])])
    atoms.append([("set", name, rng.choice(vals))])
    return atoms


def _pitch_script(rng):
    """pitch: on, to another value, to a third, off, on again with the third (the state comes back).  The value in the middle is the one
    that shares a term of its ratio with either neighbour (PITCH_RATIOS).  -> (atoms, the two that go from one on-value to another)"""
    mid, ends = VALUES["pitch"][0], list(VALUES["pitch"][1:])
    rng.shuffle(ends)
    atoms = [[("set", "pitch", v)] for v in (ends[0], mid, ends[1], None, ends[1])]
    return atoms, atoms[1:3]


def _dither_script(rng):
    """dither: on, the seed alone changed, another mode, off, on again -> (atoms, the one that changes the seed alone)"""
    tpdf = list(VALUES["dither"][:2])
    rng.shuffle(tpdf)
    atoms = [[("set", "dither", v)] for v in (tpdf[0], tpdf[1], rng.choice(VALUES["dither"][2:]), None, rng.choice(VALUES["dither"]))]
    return atoms, atoms[1:2]


# which walk plays which settings: what depends on another setting shares its walk, so that a walk meets it with that one on and off
_PLAN = (("deesser", "compressor"), ("loudness", "limiter"), ("trim",), ("pause", "peak"), ("rate", "filters"), ("pitch",), ("dither", "rate"))
_PAIRS = dict(trim=3, limiter=1, pause=1, compressor=1, deesser=1)
# every walk starts on batch 0: grows, shrinks, and 1 -> 0 changes the row count alone
_BATCH_STEPS = ((2,), (1, 0), (2, 0), (1,), (1, 0), (2, 1, 0), (2,))
_WAV_WALKS = (0, 1, 5)
_FETCH_WALKS = (0, 1, 2)
# what a walk needs around its own settings to give them something to do: set in front of everything else
_CONTEXT = {1: (("peak", "true"),), 2: (("loudness", (-12.0, -1.0)),), 3: (("trim", (40.0, 20.0, 5.0)), ("loudness", (-12.0, -1.0))),
            4: (("loudness", (-14.0, -2.0)), ("limiter", 5.0), ("compressor", VALUES["compressor"][1]), ("deesser", VALUES["deesser"][1]),
                ("trim", (40.0, 20.0, 5.0))),
            5: (("compressor", VALUES["compressor"][0]), ("deesser", VALUES["deesser"][0]), ("trim", (40.0, 20.0, 5.0)), ("loudness", (-12.0, -1.0))),
            6: (("loudness", (-12.0, -1.0)), ("limiter", 5.0))}
# the setting whose refused call walks 5 and 6 hold (walks 0 to 4 draw theirs from the seed)
_REFUSED_BY = {5: "pitch", 6: "dither"}


def _merge(scripts, rng, even=(), at=0):
    """the scripts' atoms in one random order that keeps every script's own.  even: atoms (by identity) to put at even steps of a walk
    in which the merged steps start at step `at`, wherever the scripts' orders leave the choice: such an atom is drawn at an even step
    when one is at the head of a script, and another kind at an odd one (_wanted decides whether the draw did it)"""
    left = [list(s) for s in scripts if s]
    out = []
    while left:
        pick = left
        if even:
            want = (at + len(out)) % 2 == 0
            pick = [s for s in left if any(s[0] is e for e in even) == want] or left
        s = rng.choice(pick)
        out.extend(s.pop(0))
        if not s:
            left.remove(s)
    return out


def _on(state, name):
    return state[name] != OFF[name]


def _wanted(w, walk):
    """the situations walk w must hold beyond its steps' mere presence (test_output_walk_cpu.py states them, and that every key field's
    omission is caught): each is met with the reports in front (an even step)"""
    st = states(walk)
    prev = [start()] + st[:-1]
    even = [(i, p, s, walk[i]) for i, (p, s) in enumerate(zip(prev, st)) if i % 2 == 0]
    both = lambda p, s, n: all(_on(x, n) for x in (p, s))  # noqa: E731
    if w == 0:  # with the compressor's report in front (take_order): the de-esser changed under the compressor, and another waveform
        return (any(k[0] == "set" and k[1] == "deesser" and _on(p, "deesser") and p["deesser"] != s["deesser"] and both(p, s, "compressor")
                    for i, p, s, k in even if i % 4 == 0)
                and any(k[0] == "set" and k[1] == "deesser" and both(p, s, "deesser") and p["deesser"] != s["deesser"] for i, p, s, k in even if i % 4 == 2)
                and any(k[0] == "wav" and _on(s, "compressor") for i, p, s, k in even if i % 4 == 0))
    if w == 4:
        # a chain changed under the de-esser and the compressor, with either report in front, and other rows of one width with the
        # de-esser's in front; with a chain on, fewer rows of one width, and narrower rows
        chain = [i % 4 for i, p, s, k in even if k[0] == "set" and k[1] == "filters" and p["filters"] != s["filters"]
                 and both(p, s, "compressor") and both(p, s, "deesser")]
        return (0 in chain and 2 in chain
                and any(k == ("batch", 0) and p["batch"] == 1 and _on(s, "deesser") for i, p, s, k in even if i % 4 == 2)
                and any(k == ("batch", 0) and p["batch"] == 1 and _on(s, "filters") for p, s, k in zip(prev, st, walk))
                and any(k[0] == "set" and k[1] == "rate" and rate_of(s) < rate_of(p) and _on(s, "filters") for p, s, k in zip(prev, st, walk)))
    if w == 1:
        lim = [(p, s) for p, s, k in zip(prev, st, walk) if k[0] == "set" and k[1] == "limiter"]
        return (any(_on(p, "limiter") and _on(s, "limiter") and _on(s, "loudness") for p, s in lim)  # the window's milliseconds, in use
                and any(_on(s, "limiter") and not _on(s, "loudness") for s in st) and any(_on(s, "limiter") and _on(s, "loudness") for s in st))
    if w == 3:
        return any(_on(s, "pause") and not _on(s, "trim") for s in st) and any(_on(s, "pause") and _on(s, "trim") for s in st)
    if w == 5:
        # the shift goes from one on-value to another under the compressor and the de-esser, with either one's report in front (the two
        # keep maxima of the shifted rows), and under trimming (the edges are the shifted rows' too).  Those two and the other waveform
        # are met at even steps; the three batch steps under a shift at whatever step: the context takes steps 0 to 3, the first shift
        # step 4 at the earliest, off and on again take or leave without a shift one more even step, so of the five even steps left in a
        # walk of 16 at most four hold a situation, and a report in front of a fetch is what tells the two maxima's keys from each other,
        # not the shifted rows' own (every output starts from those)
        moved = {i % 4 for i, p, s, k in even if k[0] == "set" and k[1] == "pitch" and both(p, s, "pitch") and p["pitch"] != s["pitch"]
                 and both(p, s, "compressor") and both(p, s, "deesser") and both(p, s, "trim")}
        rows = lambda b: len(BATCHES[b][0])  # noqa: E731
        wide = lambda b: max(BATCHES[b][1])  # noqa: E731
        shifted = [(p, s, k) for p, s, k in zip(prev, st, walk) if _on(p, "pitch") and _on(s, "pitch")]
        # pitch on, off and on again with the value it had: the state comes back, and the kept rows are those of another setting by then
        vals = [k[2] for k in walk if k[0] == "set" and k[1] == "pitch"]
        back = any(a is not None and b is None and c == a for a, b, c in zip(vals, vals[1:], vals[2:]))
        return (moved == {0, 2} and back
                and any(k[0] == "wav" and _on(s, "pitch") for i, p, s, k in even)                  # another waveform under the same shift
                and any(k == ("batch", 0) and p["batch"] == 1 for p, s, k in shifted)              # the row count alone
                and any(k[0] == "batch" and rows(k[1]) > rows(p["batch"]) and wide(k[1]) > wide(p["batch"]) for p, s, k in shifted)   # the scratch moves
                and any(k[0] == "batch" and rows(k[1]) < rows(p["batch"]) and wide(k[1]) < wide(p["batch"]) for p, s, k in shifted))  # and is reused dirty
    if w == 6:
        # every one at a step whose encoded fetches hold a PCM encoding (encodings(i) holds none at i % 5 == 3: the dither would be idle)
        pcm = [(i, p, s, k) for i, (p, s, k) in enumerate(zip(prev, st, walk)) if i % 5 != 3]
        others = [n for n in SETTINGS if n not in ("dither", "rate", "limiter")]  # (the limiter without loudness does nothing)
        return (any(_on(s, "dither") and _on(s, "rate") and not any(_on(s, n) for n in others) for i, p, s, k in pcm)  # the resampler alone in front of the dithered store
                and any(_on(s, "dither") and _on(s, "loudness") and _on(s, "limiter") for i, p, s, k in pcm)
                and any(_on(s, "dither") and not _on(s, "rate") for i, p, s, k in pcm)
                and any(i % 2 == 0 and k[0] == "set" and k[1] == "dither" and both(p, s, "dither") and p["dither"][0] == s["dither"][0]
                        and p["dither"][1] != s["dither"][1] for i, p, s, k in pcm))                                     # the seed alone, the reports in front
    return True


def walks(seed):
    """N_WALKS histories, the same for the same seed: lists of steps, each played from start()"""
    out = []
    ops = list(OPS[:N_SHUFFLED_OPS])
    random.Random(seed).shuffle(ops)
    ops += OPS[N_SHUFFLED_OPS:]
    for w in range(N_WALKS):
        for attempt in range(10000):
            rng = random.Random(seed * 1000003 + w * 10007 + attempt)
            even = []  # the atoms _wanted(w) asks for at even steps
            if w == 5:
                script, even = _pitch_script(rng)
                scripts = [script[1:]]  # (the first shift goes directly behind the context, below)
            elif w == 6:  # loudness, the context of the dithered store's gain and limiter, goes off and on again beside dither and rate
                script, even = _dither_script(rng)
                scripts = [script, _script("rate", rng, 0), [[("set", "loudness", None)], [("set", "loudness", VALUES["loudness"][0])]]]
            else:
                scripts = [_script(n, rng, _PAIRS.get(n, 0)) for n in _PLAN[w]]
            if w == 3:  # trim, the context of this walk's pause limit, goes off and on again beside it
                scripts.append([[("set", "trim", None)], [("set", "trim", VALUES["trim"][0])]])
            scripts.append([[("batch", b)] for b in _BATCH_STEPS[w]])
            scripts.append([[("op", f, rng.randrange(2))] for f in ops[2 * w:2 * w + 2]])
            extra = [[("fetch", PATHS[(2 * w + seed) % len(PATHS)])]] if w in _FETCH_WALKS else []
            if w in _WAV_WALKS:
                extra.append([("wav", 50 + 7 * w + seed % 5)])
            if w == 5:  # (and the other waveform under a shift)
                even = even + extra[-1:]
            # the refused call: an atom of its own (it never parts a value from the step back to it); its value is the state's there
            name = _REFUSED_BY.get(w) or ("filters", "limiter", "trim", "pause", "deesser", "rate", "loudness", "compressor")[(w + seed) % 8]
            extra.append([("refuse", name, None)])
            scripts.extend([atom] for atom in extra)  # (each free of the others)
            context = [("set", n, v) for n, v in _CONTEXT.get(w, ())] + (script[0] if w == 5 else [])
            walk = context + _merge(scripts, rng, even, len(context))
            at = walk.index(("refuse", name, None))
            walk[at] = ("refuse", name, refused(states(walk[:at] or [("fetch", "f32")])[-1], name))
            if _wanted(w, walk):
                break
        else:
            raise RuntimeError(f"no walk {w} for seed {seed}")
        out.append(walk)
    return out


# regression walks: histories that once failed on the GPU, by name (none so far)
REGRESSIONS = {}


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------------
def spans(sr, W, durs):
    """row b's span at the model's rate: its reported duration, after the speed, inside [0, W]"""
    return [min(W, int(np.float32(d / np.float32(SPEED)) * np.float32(sr))) for d in durs]


def busy_rows(sr, W, spans, seed, tone_hz=None, ms=5.0):
    """float32 [len(spans), W] at the model's rate sr, row b's signal inside its first spans[b] samples and quiet noise everywhere, three
    kinds in turn; what fetch_rows.rows has, and what it lacks.  Phrase (a span of 0.9 s and more): a 220 Hz tone at 0.35, above every
    compressor threshold drawn, behind 60 ms and in front of 80 ms of silence, with PAUSE_S of silence from 0.35 s on (longer than every
    pause limit drawn), white noise at 0.12 from 0.15 to 0.21 s (a sibilant: most of it above every de-esser's split frequency) and two
    clicks at 0.9 (the limiter turns them down once the loudness gain is above 1).  Tone: tone_hz (None: sr / 4) in 6 ms bursts every 150 ms, at 45
    degrees and in the next such row at 90 (loudness far under its peaks; at a rate of 4 tone_hz the true peak is 3 dB over the sample peak
    at 45 degrees, and whatever phase a filter in front adds, one of two such rows keeps 1 / cos(22.5 degrees), 0.69 dB).  Clicky:
    limiter_ref.peaky_row (peaks the limiter turns down, none of it silent).  The rows depend on the seed alone, not on the settings."""
    rng = np.random.default_rng(seed)
    wav = (1e-5 * rng.standard_normal((len(spans), W))).astype(np.float32)
    t = np.arange(W) / sr
    tone_hz = sr / 4.0 if tone_hz is None else tone_hz
    for b, nb in enumerate(int(n) for n in spans):
        if b % 3 == 0:
            lo, hi = min(nb, int(0.06 * sr)), max(0, nb - int(0.08 * sr))
            voiced = (t < 0.35) | (t >= 0.35 + PAUSE_S)
            voiced[:lo] = False
            voiced[hi:] = False
            x = 0.35 * np.sin(2 * np.pi * (220.0 + 30.0 * b) * t) * voiced
            ess = (t >= 0.15) & (t < 0.21) & voiced
            x = x + 0.12 * rng.standard_normal(W) * ess
            for at in (0.10, 0.30):
                if int(at * sr) < hi:
                    x[int(at * sr)] = 0.9
            wav[b] += x.astype(np.float32)
        elif b % 3 == 1:
            envl = 0.004 + 0.3 * np.exp(-0.5 * (((t % 0.15) - 0.05) / 0.003) ** 2)
            wav[b, :nb] += (envl * np.sin(2 * np.pi * tone_hz * t + np.pi / 4 * (1 + b // 3)))[:nb].astype(np.float32)
        else:
            wav[b] = limiter_ref.peaky_row(W, nb, 1.0, 0.1, limiter_ref.samples(sr, ms), seed + b)
    return wav
