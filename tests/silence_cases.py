"""The rows, spans, references and bounds that tests/test_silence_kernels_cpu.py and tests/test_gpu_silence_kernels.py share: the frame
pass and the row pass of kernels_edges.hip and the pause pass behind them (section 17), pass by pass.

Rates: the ten of tests/test_gpu_silence.py, frames F = 80, 110, 160, 221, 441, 480, 882, 960, 1764, 1920; four are multiples of the
32-sample chunk (ALIGNED: no chunk straddles a frame boundary there, so pb is +0.0 everywhere), two are odd.  Width: width(hz) =
max(2 * 8192 + 40, 12 F + 8) rounded up to a multiple of 4 (16424 up to 96 kHz, 21176 and 23048 above): two workgroup seams of the
frame pass (samples 8192 and 16384) and at least 12 frames, the smallest width that still crosses a workgroup span twice.  One more
case, long_case(), at 8 kHz with W = 1030 * 80 + 40: more than 1024 frames, so the row workgroup walks a second stride and its block
reductions run over both; there the loudest frame of the last-loud row, the last active frame of the near-threshold rows and cuts of
the pause pass all lie behind frame 1023.  x has one column more than W (NaN), the GPU test's W + 1 form.

Rows (rows_of: signal and span).  Signals: modulated noise; a tone on a DC offset; an all-zero row; a row of +-0.25 (its squares and every
fp32 sum of them are exact: every frame's level, the short last one included, must be exactly 0.0625); a row whose loudest sample is
the single sample of its last frame (n = 2 F + 1); and two near-threshold rows (below).  Spans: required_spans, every one at every
rate.  Every sample behind n[r] is NaN; inside the span |x| >= 1e-6 or x == 0, so no square underflows.

Near-threshold rows (NEAR_EDGES, then NEAR_PAUSE).  Full frames of loud noise (one in twelve), quiet frames 60 dB below them (every
frame k with k % 4 == 3 that is not loud, and the short last frame) and, everywhere else, picked frames: each rescaled in float32, then
moved by single ulps, until its float64 level is thr * (1 + e), thr the float64 threshold of the row for top_db = 40 and e running
through 0, +-1e-7, +-1e-6, +-1e-5 (_near_row has the two orders).  In NEAR_EDGES the loud frames are 6, 18, ...: the first and the last
active frame are picked ones, and start and end (with keep = 0) hinge on them.  In NEAR_PAUSE they are 0, 12, ... and the last full
frame: the picked frames lie between two loud frames 120 ms apart with only quiet frames beside them, and where the pause pass cuts
depends on which side of the threshold the device puts each of them; two neighbours at e = -1e-5 beside a quiet frame make one cut
certain.  Asserted here, on the CPU: at least eight picked frames, none the loudest, each within 2e-5 relative of the threshold (ten
times the device bound below is 2.0e-5), the achieved e within 2e-8 of the wanted one, and mx unchanged by the rescaling.

References, per row: the float64 shares of every chunk in the kernel's decomposition (a chunk's samples inside the span before the
next frame boundary, and from it on) with the number of samples in each; the float64 levels of silence_ref.levels; and a float32
sequential restatement of both in numpy float32 without FMA (f32_shares: square rounded, then added, in sample order; recombine: the
row pass, a sequential double sum of the shares in chunk order and one division by the frame's own length).

Bounds, none taken from a kernel.  A share is a sequential fp32 sum of L <= 32 non-negative squares, each square rounded once: relative
error at most gamma(L + 1), about (L + 1) * 2^-24 (share_bound).  The row pass adds at most 61 such floats in double and divides once,
under 2^-45 relative: (ED_CHUNK + 2) * 2^-24 = 34 * 2^-24 = 2.03e-6 (LEVEL_BOUND, under 1e-5 dB) covers a level.  A share or level
whose reference is 0 must be 0."""
import functools

import numpy as np

import silence_ref as ref

CHUNK, SPAN, ROW_THREADS = 32, 8192, 1024
RATES = (8000, 11025, 16000, 22050, 44100, 48000, 88200, 96000, 176400, 192000)
ALIGNED = (16000, 48000, 96000, 192000)  # F = 160, 480, 960, 1920: multiples of 32
U = 2.0 ** -24
LEVEL_BOUND = (CHUNK + 2) * U
TOP_DB, MAX_PAUSE_MS = 40.0, 20.0
E_WANTED = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5)
# the order along the picked frames (eight to every twelve frames), see _near_row
E_EDGES = (0.0, -1e-7, 1e-7, -1e-6, 1e-6, -1e-5, 1e-5, 0.0)
E_PAUSE = (1e-5, 0.0, 1e-7, -1e-7, 1e-6, -1e-5, -1e-5, -1e-6)
SEED = 14
NOISE, TONE, ZERO, QUARTER, LAST_LOUD, NEAR = "noise", "tone", "zero", "quarter", "last_loud", "near"
LONG = "8000 long"  # the key of long_case() where a rate keys a table


def width(hz):
    w = max(2 * SPAN + 40, 12 * ref.frame(hz) + 8)
    return w + (-w) % 4


LONG_W = 1030 * 80 + 40


def rows_of(F, W, long=False):
    """[(signal, span)]; the last two rows are the near-threshold ones"""
    rows = [(NOISE, W), (TONE, W - 1), (QUARTER, 8193), (NOISE, 8192), (TONE, 8191), (NOISE, 2 * F), (LAST_LOUD, 2 * F + 1), (TONE, F + 1),
            (NOISE, F), (QUARTER, F - 1), (NOISE, 33), (TONE, 32), (NOISE, 31), (QUARTER, 1), (NOISE, 0), (ZERO, W - 2)]
    if long:
        rows += [(LAST_LOUD, 1029 * F + 1), (QUARTER, W - 6)]
    return rows + [(NEAR, W), (NEAR, W - 3)]


def required_spans(F, W):
    return (0, 1, 31, 32, 33, F - 1, F, F + 1, 2 * F, 2 * F + 1, 8191, 8192, 8193, W - 1, W)


def _floor(x):
    """|x| >= 1e-6 wherever x != 0: no square underflows"""
    small = (x != 0) & (np.abs(x) < 1e-6)
    return np.where(small, np.where(x < 0, -1e-6, 1e-6), x)


def _near_row(rng, n, hz, edges):
    """one near-threshold row -> (x [n] float32, dict of what it was built to).  edges: the loud frames are 6, 18, 30, ..., so the first
    and the last active frame are picked ones (e = 0 first) and start and end hinge on them; else they are 0, 12, 24, ... and the last
    full frame, and frames 8 and 9 of every twelve (e = -1e-5) with the quiet frame 7 make a pause of 30 ms at least: one certain cut"""
    F = ref.frame(hz)
    Kfull = n // F
    k = np.arange(Kfull)
    loud = (k % 12 == 6) if edges else ((k % 12 == 0) | (k == Kfull - 1))
    quiet = ~loud & (k % 4 == 3)
    picked = np.flatnonzero(~loud & ~quiet)
    amp = np.where(loud, 0.3, np.where(quiet, 3e-4, 4.5e-3))
    first = int(np.flatnonzero(loud)[0])
    amp[first] = 0.45  # one loudest frame, by design
    x = np.full(n, 3e-4) * rng.standard_normal(n)
    x[: Kfull * F] = (rng.standard_normal((Kfull, F)) * amp[:, None]).reshape(-1)
    x = _floor(x).astype(np.float32)
    before = ref.levels(x, n, hz)
    mx = float(before.max())
    assert int(before.argmax()) == first
    thr = mx * 10.0 ** (-float(np.float32(TOP_DB)) / 10.0)
    order = E_EDGES if edges else E_PAUSE
    want = np.array([order[i % len(order)] for i in range(picked.size)])
    for f, e in zip(picked, want):
        seg = x[f * F:(f + 1) * F].astype(np.float64)
        target = thr * (1.0 + e)
        seg = _floor(seg * np.sqrt(target / np.mean(seg ** 2))).astype(np.float32)
        x[f * F:(f + 1) * F] = _nudge(seg, target * F)
    # the frames beside the first loud one: before it (edges) or up to the next loud one
    stretch = np.arange(0, first) if edges else np.arange(1, int(np.flatnonzero(loud)[1]))
    return x, dict(picked=picked, want=want, mx=mx, thr=thr, loudest=first, stretch=stretch)


def _nudge(seg, total):
    """float32 samples moved by single ulps, one sample at a time, until the float64 sum of their squares is as close to `total` as such
    steps bring it (a rescaled frame lands within about 1e-7 relative by its float32 rounding alone; this brings it under 1e-9)"""
    seg = seg.copy()
    for _ in range(64):
        s = seg.astype(np.float64)
        left = total - float(np.sum(s ** 2))
        up = np.nextafter(seg, np.float32(np.inf)).astype(np.float64) ** 2 - s ** 2
        dn = np.nextafter(seg, np.float32(-np.inf)).astype(np.float64) ** 2 - s ** 2
        ok = np.abs(s) > 1e-5  # (the floor of 1e-6 stays far away)
        cand = np.where(ok[None, :], np.abs(left - np.stack([up, dn])), np.inf)
        way, i = np.unravel_index(int(cand.argmin()), cand.shape)
        if cand[way, i] >= abs(left):
            break
        seg[i] = np.nextafter(seg[i], np.float32(np.inf if way == 0 else -np.inf))
    return seg


def signals(hz, W, long=False):
    """x [rows, W + 1] float32 with NaN behind n[r], n, and what the near-threshold rows were built to"""
    F = ref.frame(hz)
    rows = rows_of(F, W, long)
    rng = np.random.default_rng(SEED + hz + (1 if long else 0))
    N = W + 1
    t = np.arange(N) / hz
    x = np.full((len(rows), N), np.nan, np.float32)
    n = np.array([s for _, s in rows], np.int64)
    near = {}
    for r, (sig, span) in enumerate(rows):
        if sig == NOISE:
            row = (0.02 + 0.25 * (0.5 + 0.5 * np.sin(2 * np.pi * 7.0 * t + r)) ** 2) * rng.standard_normal(N)
        elif sig == TONE:
            row = 0.25 * np.sin(2 * np.pi * 997.0 * t + 0.1 * r) + 0.1
        elif sig == ZERO:
            row = np.zeros(N)
        elif sig == QUARTER:
            row = np.where(rng.integers(0, 2, N) == 1, 0.25, -0.25)
        elif sig == LAST_LOUD:
            row = 0.05 * rng.standard_normal(N)
            row[span - 1] = 0.9
        else:
            row = np.zeros(N)
            xr, near[r] = _near_row(rng, span, hz, edges=not near)
            row[:span] = xr
        x[r, :span] = _floor(row[:span]).astype(np.float32)
    return x, n, near


def decomposition(n, F, Ks):
    """the kernel's split of a row of n samples into chunk shares: in_a, in_b [Ks, 32] bool (the sample belongs to the chunk's first /
    second share) and fc [Ks], the frame each chunk starts in"""
    i = np.arange(Ks * CHUNK).reshape(Ks, CHUNK)
    fc = i[:, 0] // F
    inside = i < n
    first = (i // F) == fc[:, None]
    return inside & first, inside & ~first, fc


def f64_shares(x, n, F, Ks):
    """float64 pa, pb [Ks] of one row and the number of samples in each"""
    a, b, _ = decomposition(n, F, Ks)
    xx = np.zeros(Ks * CHUNK)
    xx[:n] = x[:n].astype(np.float64) ** 2
    xx = xx.reshape(Ks, CHUNK)
    return np.where(a, xx, 0.0).sum(axis=1), np.where(b, xx, 0.0).sum(axis=1), a.sum(axis=1), b.sum(axis=1)


def f32_shares(x, n, F, Ks, in_a=None, in_b=None):
    """the frame pass restated in numpy float32, sequential in sample order: the square rounded, then added (no FMA)"""
    if in_a is None:
        in_a, in_b, _ = decomposition(n, F, Ks)
    xs = np.zeros(Ks * CHUNK, np.float32)
    m = min(len(x), Ks * CHUNK)
    xs[:m] = np.nan_to_num(x[:m])
    xs = (xs * xs).reshape(Ks, CHUNK)
    a, b, zero = np.zeros(Ks, np.float32), np.zeros(Ks, np.float32), np.float32(0.0)
    for i in range(CHUNK):
        a = a + np.where(in_a[:, i], xs[:, i], zero)
        b = b + np.where(in_b[:, i], xs[:, i], zero)
    return a, b


def recombine(pa, pb, n, F):
    """the row pass: frame k's level from the shares of the chunks that touch it, a sequential double sum in chunk order (a chunk that
    starts in the frame gives its first share, the one that started in the frame before its second), one division by the frame's own
    length.  No multiply: numpy reproduces the device's doubles bit for bit."""
    n = int(n)
    K = -(-n // F)
    k = np.arange(K)
    lo = k * F
    hi = np.minimum(lo + F, n)
    c0, c1 = lo // CHUNK, (hi - 1) // CHUNK
    s = np.zeros(K)
    pa, pb = np.asarray(pa, np.float64), np.asarray(pb, np.float64)
    for j in range(int((c1 - c0).max()) + 1 if K else 0):
        c = np.minimum(c0 + j, c1)
        term = np.where(c * CHUNK // F == k, pa[c], pb[c])
        s = s + np.where(c0 + j <= c1, term, 0.0)
    return s / (hi - lo).astype(np.float64)


def share_bound(L):
    return (L + 1) * U


def pb_cuts(n, F):
    """the chunks of a row of n samples that a frame boundary cuts inside the span: boundaries j F < n that are no multiple of 32"""
    j = np.arange(1, -(-int(n) // F))
    return int(np.count_nonzero(j * F % CHUNK))


class Case:
    pass


def _case(hz, W, long):
    c = Case()
    c.hz, c.F, c.W, c.long = hz, ref.frame(hz), W, long
    c.rows = rows_of(c.F, W, long)
    c.R = len(c.rows)
    c.names = [f"{s}[{n}]" for s, n in c.rows]
    c.x, c.n, c.near = signals(hz, W, long)
    c.NEAR_EDGES, c.NEAR_PAUSE = c.R - 2, c.R - 1
    assert set(required_spans(c.F, W)) <= set(int(v) for v in c.n), (hz, sorted(set(required_spans(c.F, W)) - set(int(v) for v in c.n)))
    c.Ks, c.Kf = -(-W // CHUNK), -(-W // c.F)
    c.pa64, c.pb64 = np.zeros((c.R, c.Ks)), np.zeros((c.R, c.Ks))
    c.La, c.Lb = np.zeros((c.R, c.Ks), np.int64), np.zeros((c.R, c.Ks), np.int64)
    c.pa32, c.pb32 = np.zeros((c.R, c.Ks), np.float32), np.zeros((c.R, c.Ks), np.float32)
    c.lev64, c.lev32 = [], []
    for r in range(c.R):
        nr = int(c.n[r])
        c.pa64[r], c.pb64[r], c.La[r], c.Lb[r] = f64_shares(c.x[r], nr, c.F, c.Ks)
        c.pa32[r], c.pb32[r] = f32_shares(c.x[r], nr, c.F, c.Ks)
        c.lev64.append(ref.levels(c.x[r], nr, hz))
        c.lev32.append(recombine(c.pa32[r], c.pb32[r], nr, c.F))
    c.live = np.arange(c.Ks)[None, :] < (-(-c.n // CHUNK))[:, None]  # chunk k of row r holds samples of the row
    c.frames = -(-c.n // c.F)
    # the near-threshold rows: what the module docstring promises
    for r, d in c.near.items():
        m = c.lev64[r]
        assert d["picked"].size >= 8 and float(m.max()) == d["mx"] and int(m.argmax()) == d["loudest"], (hz, r)
        got_e = m[d["picked"]] / d["thr"] - 1.0
        assert np.all(np.abs(got_e) <= 2e-5) and np.all(np.abs(got_e - d["want"]) <= 2e-8), (hz, r, np.abs(got_e - d["want"]).max())
        assert set(E_WANTED) <= set(d["want"].tolist())
        d["got"] = got_e
        # picked frames inside a stretch that is otherwise inactive and longer than the pause limit: the frames between two loud ones
        stretch = d["stretch"]
        quiet = np.setdiff1d(stretch, d["picked"])
        assert quiet.size and np.all(m[quiet] < 1e-1 * d["thr"]) and np.intersect1d(d["picked"], stretch).size >= 5
        assert stretch.size * c.F > ref.samples(hz, MAX_PAUSE_MS) and m[stretch[-1] + 1] > 1e3 * d["thr"]
    for a in (c.x, c.n, c.pa64, c.pb64, c.La, c.Lb, c.pa32, c.pb32, c.live, c.frames, *c.lev64, *c.lev32):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case(hz):
    """x, n and every reference at hz, computed once per process and handed out read-only"""
    return _case(hz, width(hz), False)


@functools.lru_cache(maxsize=None)
def long_case():
    return _case(8000, LONG_W, True)


def all_cases():
    return [(str(hz), case(hz)) for hz in RATES] + [(LONG, long_case())]


def get(key):
    return long_case() if key == LONG else case(int(key))


KEYS = tuple(str(hz) for hz in RATES) + (LONG,)


def share_ratios(c, pa, pb):
    """|p - p64| / ((L + 1) 2^-24 p64) over the live chunks of every row, [R, Ks] each; a share whose reference is 0 must be 0 (inf if not)"""
    out = []
    for got, want, L in ((pa, c.pa64, c.La), (pb, c.pb64, c.Lb)):
        got = np.asarray(got, np.float64)[:, : c.Ks]
        d = np.abs(np.where(c.live, got - want, 0.0))
        lim = share_bound(L) * want
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.where(lim > 0, d / lim, np.where(d > 0, np.inf, 0.0)))
    return out


def level_ratios(c, lev):
    """per row |lev - lev64| / (34 * 2^-24 lev64) over its frames; a level whose reference is 0 must be 0"""
    out = []
    for r in range(c.R):
        K = int(c.frames[r])
        want = c.lev64[r]
        d = np.abs(np.asarray(lev[r], np.float64)[:K] - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.where(want > 0, d / (LEVEL_BOUND * want), np.where(d > 0, np.inf, 0.0)))
    return out


# ---- the faults the tests must be sharp enough to see: the decomposition gone wrong, in float64 ------------------------------------
MUTANTS = ("split_off_by_one", "seam_chunk_dropped", "tail_summed_to_32", "second_share_to_next_frame", "short_frame_by_F",
           "straddling_first_chunk_left_out")
SPLIT_MUTANTS = ("split_off_by_one", "second_share_to_next_frame", "straddling_first_chunk_left_out")  # need a chunk that straddles


def mutant(c, name):
    """(pa, pb [R, Ks], lev [R][K]) of a float64 model of both passes with one fault"""
    pa, pb, lev = np.zeros((c.R, c.Ks)), np.zeros((c.R, c.Ks)), []
    F = c.F
    for r in range(c.R):
        n = int(c.n[r])
        K = -(-n // F)
        a, b, fc = decomposition(n, F, c.Ks)
        xr = np.zeros(c.Ks * CHUNK)
        xr[:n] = c.x[r, :n]
        if name == "split_off_by_one":  # the first sample of the next frame counted into the first share
            i = np.arange(c.Ks * CHUNK).reshape(c.Ks, CHUNK)
            first = ((i - 1) // F <= fc[:, None]) & (i < n)
            a, b = first, (i < n) & ~first
        if name == "tail_summed_to_32" and n % CHUNK:  # the span's last chunk over a finite, loud padding
            xr[n:(n // CHUNK + 1) * CHUNK] = 0.5
            i = np.arange(c.Ks * CHUNK).reshape(c.Ks, CHUNK)
            inside = i < (n // CHUNK + 1) * CHUNK
            first = (i // F) == fc[:, None]
            a, b = inside & first, inside & ~first
        xx = (xr ** 2).reshape(c.Ks, CHUNK)
        pa[r], pb[r] = np.where(a, xx, 0.0).sum(axis=1), np.where(b, xx, 0.0).sum(axis=1)
        if name == "seam_chunk_dropped" and n > SPAN:
            pa[r, SPAN // CHUNK] = pb[r, SPAN // CHUNK] = 0.0
        m = np.zeros(K)
        for k in range(K):
            lo, hi = k * F, min(k * F + F, n)
            c0, c1 = lo // CHUNK, (hi - 1) // CHUNK
            for ch in range(c0, c1 + 1):
                own = ch * CHUNK // F == k
                if name == "straddling_first_chunk_left_out" and not own:
                    continue
                if name == "second_share_to_next_frame" and not own:
                    continue  # (given away below)
                m[k] += pa[r, ch] if own else pb[r, ch]
            if name == "second_share_to_next_frame" and k >= 2:  # what belonged to frame k - 1 arrives here
                ch = (k - 1) * F // CHUNK
                if ch * CHUNK // F != k - 1:
                    m[k] += pb[r, ch]
            m[k] /= F if name == "short_frame_by_F" else hi - lo
        lev.append(m)
    return pa, pb, lev


def can_occur(c, name):
    if name in SPLIT_MUTANTS:
        return c.F % CHUNK != 0
    return True
