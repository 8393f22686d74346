"""The chains, rows, widths, references and bounds that tests/test_filter_cpu.py and tests/test_gpu_filter_kernels.py share.

Chains (name -> rate, filters): the worst-conditioned corner allowed, a high-pass at rate / 2400, at 8, 44.1 and 192 kHz; an odd chain
(the identity pad); the telephone preset at 8 kHz; a narrow peak; a full chain of 8 biquads.  Rows (five per call): white noise; a
0.05 DC offset plus a 220 Hz tone; a tone at the chain's first corner; a unit impulse at sample 0 and one at the last sample of a chunk;
an all-zero row.  The widest call is W = 3 scan tiles + 40 samples (the lengths come from stn_dbg_filter_geometry); a row's first n
samples do not depend on W, so the narrower calls (widths()) are held against the same reference cut at their W.

Bounds.  None is taken from a kernel.  Each is 4 x the largest deviation of the float32 sequential restatement (filter_ref.chain_states
with dtype float32: every product and sum rounded, no fused multiply-add) from the float64 recurrence on the same fp32 coefficients,
normalized as tests/loudness_cases.py normalizes: per row and state component by the largest |value| of that component over the row's
chunks in the float64 reference (per pass), for y by the row's largest |y|.  The 4 is the margin for the one fp32 rounding of a start
state per chunk and the kernels' fused multiply-adds.  A row whose scale is 0 must match exactly."""
import functools

import numpy as np

import filter_ref as fr

SAFETY = 4.0
NAMES = ("noise", "dc_tone", "corner_tone", "impulses", "zero")
NOISE, DC_TONE, CORNER, IMPULSES, ZERO = range(5)
TELEPHONE = (("highpass", 300.0, 0.541, 0.0), ("highpass", 300.0, 1.307, 0.0), ("lowpass", 3400.0, 0.541, 0.0), ("lowpass", 3400.0, 1.307, 0.0))
FULL = (("highpass", 300.0, 0.7071, 0.0), ("lowshelf", 400.0, 0.7071, 3.0), ("peak", 1000.0, 2.0, -4.0), ("peak", 3000.0, 1.0, 4.0),
        ("notch", 5000.0, 4.0, 0.0), ("highshelf", 8000.0, 0.7071, -3.0), ("peak", 12000.0, 0.5, 2.0), ("lowpass", 16000.0, 0.7071, 0.0))


def lowest_corner(rate):
    """the smallest float32 frequency that is not below rate / 2400"""
    f = np.float32(rate / 2400.0)
    return float(f if float(f) >= rate / 2400.0 else np.nextafter(f, np.float32(np.inf)))


CHAINS = {
    "hp_lowest_8k": (8000, (("highpass", lowest_corner(8000), 0.7071, 0.0),)),
    "hp_lowest_44k": (44100, (("highpass", lowest_corner(44100), 0.7071, 0.0),)),
    "hp_lowest_192k": (192000, (("highpass", lowest_corner(192000), 0.7071, 0.0),)),
    "odd_44k": (44100, (("highpass", 80.0, 0.7071, 0.0), ("peak", 3000.0, 1.0, 4.0), ("highshelf", 8000.0, 0.7071, -3.0))),
    "telephone_8k": (8000, TELEPHONE),
    "peak_q8_44k": (44100, (("peak", 200.0, 8.0, 12.0),)),
    "full_44k": (44100, FULL),
}
# what the numpy model of the decomposition was also run on (test_filter_cpu.py)
MODEL_ONLY = {"notch_shelf_16k": (16000, (("notch", 50.0, 8.0, 0.0), ("lowshelf", 150.0, 0.7071, 6.0)))}


@functools.lru_cache(maxsize=None)
def geometry():
    from supertonic_amd import binding
    return binding.filter_geometry()  # chunk, workgroup span, scan tile in chunks, biquads per section pass


def w_max():
    chunk, _, tile, _ = geometry()
    return 3 * tile * chunk + 40


def widths():
    """W of every call: 1, chunk - 1, chunk, chunk + 1, span - 1, span + 1, one scan tile - 1 chunk, one scan tile + 1 chunk, and the
    widest; W % 4 == 0 takes the 16-byte staging (chunk, tile -+ chunk, the widest), the others the scalar one."""
    chunk, span, tile, _ = geometry()
    return (1, chunk - 1, chunk, chunk + 1, span - 1, span + 1, (tile - 1) * chunk, (tile + 1) * chunk, w_max())


def seams(K):
    """the chunks around a workgroup span's end and the scan's tile ends"""
    chunk, span, tile, _ = geometry()
    g = span // chunk
    return tuple(k for k in (g - 1, g, g + 1, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 3 * tile - 1, 3 * tile, 3 * tile + 1) if k < K)


def signals(rate, first_corner, N, seed=18):
    rng = np.random.default_rng(seed + rate)
    t = np.arange(N) / rate
    imp = np.zeros(N)
    imp[0] = 1.0
    if N > 1500 * fr.CHUNK + fr.CHUNK - 1:
        imp[1500 * fr.CHUNK + fr.CHUNK - 1] = 1.0  # the last sample of chunk 1500, in the second scan tile
    x = np.stack([0.25 * rng.standard_normal(N), 0.05 + 0.4 * np.sin(2 * np.pi * 220.0 * t), 0.5 * np.sin(2 * np.pi * first_corner * t), imp, np.zeros(N)])
    return x.astype(np.float32)


class Case:
    pass


def _scales(ref):
    start, end, y = ref
    return dict(start=np.abs(start).max(axis=2, keepdims=True), end=np.abs(end).max(axis=2, keepdims=True), y=np.abs(y).max(axis=1, keepdims=True))


def deviation(got, ref, scale):
    """largest |got - ref| / scale over the entries whose scale is not 0 and whether every entry whose scale is 0 is equal; got may be
    narrower than ref along the last axes (a narrower call): ref is cut to it"""
    ref = ref[tuple(slice(0, n) for n in got.shape)]
    d = np.abs(got.astype(np.float64) - ref)
    s = np.broadcast_to(scale, ref.shape)
    exact = bool(np.all(d[s == 0] == 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(s > 0, d / s, 0.0)
    return rel, exact


def deviations(c, got):
    """the three normalized deviations of (start, end, y) from the case's float64 reference: start and end per pass [P], y a number"""
    out = {}
    for key, g, r in zip(("start", "end", "y"), got, c.ref):
        rel, exact = deviation(g, r, c.scale[key])
        assert exact, key
        out[key] = rel.reshape(rel.shape[0], -1).max(axis=1) if key != "y" else float(rel.max())
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """x, the fp32 coefficients as section passes, the float64 reference, the float32 restatement's deviations and the bounds"""
    from supertonic_amd import binding
    c = Case()
    c.name = name
    c.rate, c.filters = (CHAINS.get(name) or MODEL_ONLY[name])
    c.W = w_max()
    c.c32 = np.stack([binding.filter_coefs(f, c.rate)[1] for f in c.filters])
    c.passes = fr.passes_of(c.c32)
    c.x = signals(c.rate, c.filters[0][1], c.W)
    c.ref = fr.chain_states(c.x, c.passes, np.float64)
    c.scale = _scales(c.ref)
    c.f32 = deviations(c, fr.chain_states(c.x, c.passes, np.float32))
    c.bound = {k: SAFETY * v for k, v in c.f32.items()}
    for a in (c.x, c.c32, c.passes, *c.ref):
        a.setflags(write=False)
    return c


def over_bound(c, got):
    """measured over bound per kind: the largest over the passes for the states"""
    d = deviations(c, got)
    out = {}
    for k in d:
        v, b = np.atleast_1d(d[k]), np.atleast_1d(c.bound[k])
        out[k] = float(np.max(np.where(b > 0, v / np.where(b > 0, b, 1.0), np.where(v > 0, np.inf, 0.0))))
    return out
