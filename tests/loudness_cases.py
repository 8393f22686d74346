"""The rows, lengths, references and bounds that tests/test_loudness_kernels_cpu.py and tests/test_gpu_loudness_kernels.py share.

Rows (six per call, the same at every rate): a 30 Hz + 997 Hz tone on a 0.1 DC offset (the high-pass states are large at every chunk
boundary), coloured noise under an envelope, a quiet-then-loud row (the relative gate), a row of 4 hop - 1 samples (one short of a
block), an all-zero row and a row of n = 0.  Behind n[r] every row is NaN.  W = 3 * 32768 + 40: three full scan tiles of 1024 chunks
and the start of a fourth, 13 workgroup spans of 8192 samples; the GPU tests run it as W (16-byte loads), W + 1 and W uploaded 4 bytes
off alignment (scalar loads).  At 176.4 and 192 kHz W = 6 * 32768 + 40 (width(hz)): 7 gating blocks at 192 kHz as at 96 kHz, seven scan
tiles, 25 spans.  The lengths walk every boundary of the decomposition (lengths() below).

Everything is computed once per process (case(hz)) and handed out read-only.  The restatement loops over the samples in Python with the
six rows side by side; case(hz) takes about 3.5 s up to 96 kHz and 6 to 6.5 s at 176.4 and 192 kHz (twice the samples) on one CPU core, so the
rows stay as they are and W is not shrunk.

Bounds.  None is taken from a kernel.  Each comes from the float32 restatement of the same recurrence (loudness_ref.cascade_states and
chunk_shares with dtype = float32: sequential from sample 0, every product and sum rounded, no fused multiply-add) held against the
float64 reference on these rows with the same fp32 coefficients: its largest deviation, normalized by the row's scale, times 4 (the
kernels contract to FMAs and the scan sums in another tree).  The scales, per row: for the states, per component, the largest |value|
of that component over the row's chunks in the float64 reference (end states for pass 1, true states for the scan); for pa / pb the
row's largest chunk energy pa + pb; for the segment sums the row's largest segment.  A row whose scale is 0 must match exactly."""
import functools
import math

import numpy as np

from loudness_ref import CHUNK, cascade_states, chunk_shares, chunks, gate_from_segments, hop, segments_from_shares

HIGH = (88200, 96000, 176400, 192000)
RATES = (8000, 11025, 22050, 44100, 48000) + HIGH
STRADDLING = (11025, 22050, 44100, 88200, 176400)  # hop 1103, 2205, 4410, 8820, 17640: no multiple of 32, so chunks straddle segments
W = 3 * 32768 + 40
W_WIDE = 6 * 32768 + 40
SPAN, TILE = 8192, 32768  # samples per workgroup of the chunk passes, per scan tile
TONE, NOISE, QUIET_LOUD, SHORT, ZERO, EMPTY = range(6)
NAMES = ("tone", "noise", "quiet_loud", "short", "zero", "empty")
SAFETY = 4.0
SEED = 20


def width(hz):
    """W at hz: up to 96 kHz three full scan tiles and the start of a fourth (7 gating blocks at 96 kHz); at 176.4 and 192 kHz six and the
    start of a seventh (7 blocks at 192 kHz), or the quiet-then-loud row has too few blocks for the relative gate to decide anything."""
    return W if hz <= 96000 else W_WIDE


def lengths(hz):
    """n[6] at hz.  Over the rates up to 48 kHz: 0, 1, 31, 32, 33, 8191, 8192, 8193, 32767, 32768, 32769, 65536 + 5, a multiple of hop and
    one more and one less, n % 4 in {1, 2, 3}, and at every rate a row that runs into the last scan tile.  Each of the four HIGH rates has
    all of these by itself: the last tile (w - 2, n % 4 = 2), m hop, m hop + 1 and m hop - 1 (n % 4 = 0, 1, 3: these hops are multiples of
    4), and they change rows from rate to rate, so that the tone, the noise and the quiet-then-loud row each end on a whole segment, one
    sample past one and one sample short of one at some rate.  The quiet-then-loud row keeps at least 9 segments everywhere."""
    h, w = hop(hz), width(hz)
    free = {8000: (W, 65536 + 5, 32769, 1),
            11025: (31, W - 1, 60 * h, 8192),
            22050: (W - 2, 32, 40 * h + 1, 32767),
            44100: (32768, W - 3, W, 33),
            48000: (W, 8193, W - 1, 8191),
            88200: (w - 2, 11 * h, 10 * h + 1, 9 * h - 1),
            96000: (10 * h - 1, w - 2, 10 * h, 9 * h + 1),
            176400: (11 * h + 1, 10 * h - 1, w - 2, 11 * h),
            192000: (10 * h, 9 * h + 1, 10 * h - 1, w - 2)}[hz]
    return np.array([free[0], free[1], free[2], 4 * h - 1, free[3], 0], np.int64)


REQUIRED_LENGTHS = (0, 1, 31, 32, 33, 8191, 8192, 8193, 32767, 32768, 32769, 65536 + 5)


def signals(hz):
    """x [6, width(hz) + 1] float32 with NaN behind n[r], and n."""
    rng = np.random.default_rng(SEED + hz)
    N = width(hz) + 1
    t = np.arange(N) / hz
    n = lengths(hz)
    white = rng.standard_normal(N)
    tone = 0.25 * np.sin(2 * np.pi * 30 * t) + 0.25 * np.sin(2 * np.pi * 997 * t) + 0.1
    col = np.convolve(rng.standard_normal(N), np.ones(9) / 3.0, mode="same")
    env = 0.5 * (1 + np.sin(2 * np.pi * 0.7 * t)) ** 2
    noise = 0.05 * col * env + 0.02
    quiet_loud = np.where(np.arange(N) < n[QUIET_LOUD] // 2, 1e-3, 0.2) * white
    short = 0.5 * rng.standard_normal(N)
    x = np.stack([tone, noise, quiet_loud, short, np.zeros(N), white]).astype(np.float32)
    x[np.arange(N)[None, :] >= n[:, None]] = np.nan
    return x, n


class Case:
    pass


def _measure(c, coef, dtype, reset_every=0):
    """one restatement of the whole measurement on the case's rows: states, shares, segments"""
    start, end, y = cascade_states(c.x, coef, c.n, dtype=dtype, reset_every=reset_every)
    K = start.shape[1]
    pa, pb = np.zeros((6, K), dtype), np.zeros((6, K), dtype)
    seg = []
    for r in range(6):
        pa[r], pb[r] = chunk_shares(np.nan_to_num(y[r]), c.n[r], c.hop, dtype=dtype)
        seg.append(segments_from_shares(pa[r], pb[r], c.n[r], c.hop))
    return dict(start=start, end=end, y=y, pa=pa, pb=pb, seg=seg)


def _dev(got, ref, scale):
    """largest |got - ref| / scale over the entries the reference defines; an entry whose scale is 0 must be equal"""
    live = ~np.isnan(ref)
    d = np.abs(np.where(live, got.astype(np.float64) - ref, 0.0))
    s = np.broadcast_to(scale, d.shape)
    assert np.all(d[s == 0] == 0)
    return float((d[s > 0] / s[s > 0]).max()) if np.any(s > 0) else 0.0


def scales(ref):
    """the rows' scales of the module docstring, from a float64 measurement"""
    with np.errstate(invalid="ignore"):
        return dict(end=np.nan_to_num(np.nanmax(np.abs(ref["end"]), axis=1, initial=0.0))[:, None, :],
                    start=np.nan_to_num(np.nanmax(np.abs(ref["start"]), axis=1, initial=0.0))[:, None, :],
                    share=(ref["pa"] + ref["pb"]).max(axis=1)[:, None],
                    seg=[float(s.max()) if len(s) else 0.0 for s in ref["seg"]])


def deviations(c, got):
    """normalized deviations of a measurement (dict as _measure's: end, start, pa, pb, seg) from the case's float64 reference"""
    sc = c.scale
    seg = 0.0
    for r in range(6):
        if len(c.ref["seg"][r]):
            seg = max(seg, _dev(np.asarray(got["seg"][r]), c.ref["seg"][r], sc["seg"][r]))
    return dict(end=_dev(got["end"], c.ref["end"], sc["end"]), start=_dev(got["start"], c.ref["start"], sc["start"]),
                share=max(_dev(got["pa"], c.ref["pa"], sc["share"]), _dev(got["pb"], c.ref["pb"], sc["share"])), seg=seg)


@functools.lru_cache(maxsize=None)
def case(hz):
    """x, n, the table, the float64 reference of every pass, the float32 restatement's deviations and the bounds at hz"""
    from supertonic_amd import binding
    c = Case()
    c.hz, c.hop, c.W = hz, hop(hz), width(hz)
    c.coef, c.mpow, table_hop = binding.loudness_table(hz)
    assert table_hop == c.hop
    c.x, c.n = signals(hz)
    c.ref = _measure(c, c.coef.astype(np.float64), np.float64)
    c.scale = scales(c.ref)
    c.f32 = deviations(c, _measure(c, c.coef, np.float32))
    c.bound = {k: SAFETY * v for k, v in c.f32.items()}
    c.gate = [gate_from_segments(s, c.hop) for s in c.ref["seg"]]  # (L, 1.0, margin) of the float64 reference
    for a in (c.x, c.n, c.coef, c.mpow, *[v for v in c.ref.values() if isinstance(v, np.ndarray)], *c.ref["seg"]):
        a.setflags(write=False)
    return c


def dl_bound(c, r):
    """what the segment bound allows row r's L to move by while no block changes side of a gate: every 400 ms block mean moves by at most
    eps * S / hop (S the row's largest segment), so the gated mean z moves by as much and dL <= 10 log10(1 + eps * S / (hop * z))"""
    L = c.gate[r][0]
    z = 10.0 ** ((L + 0.691) / 10.0)
    return 10.0 * math.log10(1.0 + c.bound["seg"] * c.scale["seg"][r] / (c.hop * z))


# ---- the faults the tests must be sharp enough to see (float64 models of the decomposition gone wrong) -------------------------------
def fault_lost_carry(c, period):
    """the running state zeroed every `period` samples: the scan's carry lost at every tile (32768) or beyond a workgroup span (8192)"""
    return _measure(c, c.coef.astype(np.float64), np.float64, reset_every=period)


def fault_pb_dropped(c):
    got = dict(c.ref)
    got["pb"] = np.zeros_like(c.ref["pb"])
    got["seg"] = [segments_from_shares(got["pa"][r], got["pb"][r], c.n[r], c.hop) for r in range(6)]
    return got


def fault_last_chunk_dropped(c):
    """the last chunk that holds samples of the last whole segment contributes nothing"""
    got = dict(c.ref)
    got["pa"], got["pb"] = c.ref["pa"].copy(), c.ref["pb"].copy()
    for r in range(6):
        full = c.n[r] // c.hop * c.hop
        if full:
            got["pa"][r, (full - 1) // CHUNK] = 0.0
            got["pb"][r, (full - 1) // CHUNK] = 0.0
    got["seg"] = [segments_from_shares(got["pa"][r], got["pb"][r], c.n[r], c.hop) for r in range(6)]
    return got


def loudness_of(c, got, r):
    return gate_from_segments(got["seg"][r], c.hop)[0]

