"""A float64 statement of ITU-R BS.1770-4 integrated loudness (one channel, weight 1.0), written from the standard's text and
independent of the engine's kernels: the K-weighting biquads derived at any rate from the analog prototypes of the standard's 48 kHz
table, filtered with scipy.signal.lfilter, then the 400 ms / 100 ms gating.

Below it, the same measurement restated pass by pass for the kernel tests (tests/test_gpu_loudness_kernels.py): the cascade as the
sample-by-sample recurrence of two transposed-direct-form-II sections with its state at every 32-sample chunk boundary
(cascade_states), each chunk's energy split at the 100 ms segment boundary (chunk_shares), and the gate on segment sums
(gate_from_segments).  tests/test_loudness_kernels_cpu.py holds the three together to integrated_loudness above."""
import math

import numpy as np


def kweighting(hz):
    """(shelf_b, shelf_a, hp_b, hp_a) in float64 at hz."""
    fs = float(hz)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf_b = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    shelf_a = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp_b = np.array([1.0, -2.0, 1.0])
    hp_a = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return shelf_b, shelf_a, hp_b, hp_a


def hop(hz):
    return (int(hz) + 5) // 10


def integrated_loudness(x, hz):
    """BS.1770-4 integrated loudness of x (1-D) in LUFS, -inf when x is shorter than one 400 ms block or every block is gated out."""
    from scipy.signal import lfilter
    x = np.asarray(x, np.float64)
    sb, sa, hb, ha = kweighting(hz)
    y = lfilter(hb, ha, lfilter(sb, sa, x))
    h = hop(hz)
    nseg = len(x) // h
    if nseg < 4:
        return -math.inf
    seg = (y[: nseg * h] ** 2).reshape(nseg, h).sum(axis=1)
    z = (seg[:-3] + seg[1:-2] + seg[2:-1] + seg[3:]) / (4 * h)
    with np.errstate(divide="ignore"):
        lj = -0.691 + 10.0 * np.log10(z)
    g = lj > -70.0
    if not g.any():
        return -math.inf
    rel = -0.691 + 10.0 * math.log10(z[g].mean()) - 10.0
    g &= lj > rel
    if not g.any():
        return -math.inf
    return -0.691 + 10.0 * math.log10(z[g].mean())


CHUNK = 32  # samples per chunk of the kernels' decomposition (LO_CHUNK)


def chunks(n):
    return (int(n) + CHUNK - 1) // CHUNK


def coef_of(hz):
    """kweighting(hz) in the order the kernels take it: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 (float64)."""
    sb, sa, hb, ha = kweighting(hz)
    return np.array([sb[0], sb[1], sb[2], sa[1], sa[2], hb[0], hb[1], hb[2], ha[1], ha[2]])


def cascade_states(x, coef, n=None, dtype=np.float64, reset_every=0):
    """The K-weighting cascade as its recurrence, one sample at a time, every product and sum rounded to dtype (no fused multiply-add):
        v = b0 u + s1;  s1 = (b1 u + s2) - a1 v;  s2 = b2 u - a2 v        (shelf, coef[0:5])
        y = c0 v + t1;  t1 = (c1 v + t2) - d1 y;  t2 = c2 v - d2 y        (high-pass, coef[5:10])
    x [N] or [rows, N]; coef [10] or [rows, 10]; n (rows, default N): row r's samples at or past n[r] are not read.
    Returns (start, end, y): start [rows, K, 4] the state (s1, s2, t1, t2) before sample 32 k, NaN for k >= chunks(n); end [rows, K, 4]
    the state chunk k ends in when it starts from zero state (after its last sample below n), NaN likewise; y [rows, N], NaN at or past
    n.  K = chunks(N).  A 1-D x returns the three without the row axis.  reset_every = P > 0 models a lost carry: the running state is
    zeroed before every sample that is a multiple of P (the tests' injected faults; start and y then carry the fault)."""
    x = np.asarray(x)
    one = x.ndim == 1
    x = np.atleast_2d(x)
    R, N = x.shape
    n = np.full(R, N, np.int64) if n is None else np.broadcast_to(np.asarray(n, np.int64), (R,))
    K = chunks(N)
    c = np.broadcast_to(np.asarray(coef), (R, 10)).astype(dtype).T.copy()  # [10][R]
    xt = np.where(np.arange(K * CHUNK)[None, :] < n[:, None], np.pad(x, ((0, 0), (0, K * CHUNK - N))), 0).astype(dtype).T.copy()  # [K*32][R]
    start = np.empty((K, R, 4), dtype)
    y = np.empty((N, R), dtype)
    s1, s2, t1, t2 = (np.zeros(R, dtype) for _ in range(4))
    for i in range(N):
        if reset_every and i % reset_every == 0:
            s1, s2, t1, t2 = (np.zeros(R, dtype) for _ in range(4))
        if i % CHUNK == 0:
            k = i // CHUNK
            start[k, :, 0], start[k, :, 1], start[k, :, 2], start[k, :, 3] = s1, s2, t1, t2
        u = xt[i]
        v = c[0] * u + s1
        s1 = (c[1] * u + s2) - c[3] * v
        s2 = c[2] * u - c[4] * v
        yy = c[5] * v + t1
        t1 = (c[6] * v + t2) - c[8] * yy
        t2 = c[7] * v - c[9] * yy
        y[i] = yy
    # every chunk from zero state: the same recurrence, the chunks side by side
    xc = xt.T.reshape(R, K, CHUNK)
    cc = c[:, :, None]
    e = np.zeros((4, R, K), dtype)
    for i in range(CHUNK):
        live = (np.arange(K)[None, :] * CHUNK + i) < n[:, None]
        u = xc[:, :, i]
        v = cc[0] * u + e[0]
        a = (cc[1] * u + e[1]) - cc[3] * v
        b = cc[2] * u - cc[4] * v
        yy = cc[5] * v + e[2]
        p = (cc[6] * v + e[3]) - cc[8] * yy
        q = cc[7] * v - cc[9] * yy
        e = np.where(live[None], np.stack([a, b, p, q]), e)
    dead = np.arange(K)[None, :] >= ((n + CHUNK - 1) // CHUNK)[:, None]
    start = np.where(dead[:, :, None], np.nan, start.transpose(1, 0, 2))
    end = np.where(dead[:, :, None], np.nan, e.transpose(1, 2, 0))
    y = np.where(np.arange(N)[None, :] < n[:, None], y.T, np.nan)
    return (start[0], end[0], y[0]) if one else (start, end, y)


def chunk_shares(y, n, hop, dtype=np.float64):
    """(pa, pb) [K] each for one row y [N] of which the first n count: pa[k] the sum of y^2 over chunk k's samples that lie in the 100 ms
    segment the chunk starts in, pb[k] over those in the next segment; both over samples below n // hop * hop only (whole segments).
    Each sum runs over the chunk's samples in order, in dtype.  Chunks without such samples get 0."""
    y = np.asarray(y)
    N, K = y.shape[0], chunks(y.shape[0])
    full = int(n) // int(hop) * int(hop)
    g = np.arange(K * CHUNK).reshape(K, CHUNK)
    yy = np.where(g < full, np.pad(y, (0, K * CHUNK - N)).reshape(K, CHUNK), 0).astype(dtype)
    yy = yy * yy
    first = (g // hop) == (g[:, :1] // hop)
    pa, pb = np.zeros(K, dtype), np.zeros(K, dtype)
    for i in range(CHUNK):
        pa = pa + np.where(first[:, i], yy[:, i], 0).astype(dtype)
        pb = pb + np.where(first[:, i], 0, yy[:, i]).astype(dtype)
    return pa, pb


def segments_from_shares(pa, pb, n, hop):
    """The 100 ms segment sums [n // hop] as the gate forms them: over the chunks that touch the segment, pa of a chunk that starts in it,
    else pb, in float64."""
    nseg = int(n) // int(hop)
    seg = np.zeros(nseg, np.float64)
    for j in range(nseg):
        k = np.arange(j * hop // CHUNK, ((j + 1) * hop - 1) // CHUNK + 1)
        seg[j] = np.where(k * CHUNK // hop == j, np.asarray(pa, np.float64)[k], np.asarray(pb, np.float64)[k]).sum()
    return seg


def gate_from_segments(seg, hop, on=False, target=-23.0, ceiling=-1.0, peak=0.0):
    """BS.1770-4 gating on 100 ms segment sums of y^2 -> (L, gain, margin): L in LUFS (-inf when undefined); the gain of
    stn_set_loudness, min(10^((target - L) / 20), 10^(ceiling / 20) / peak) with L rounded to float32 first as the engine reports it
    (1.0 with on false, L undefined or peak 0); margin, the distance in LU of the nearest 400 ms block from the absolute threshold or,
    among the blocks above it, from the relative one (inf without blocks)."""
    seg = np.asarray(seg, np.float64)
    if len(seg) < 4:
        return -math.inf, 1.0, math.inf
    z = ((seg[:-3] + seg[1:-2]) + (seg[2:-1] + seg[3:])) / (4.0 * hop)
    with np.errstate(divide="ignore"):
        lj = -0.691 + 10.0 * np.log10(z)
    margin = float(np.abs(lj + 70.0).min())
    g = lj > -70.0
    if not g.any():
        return -math.inf, 1.0, margin
    rel = -0.691 + 10.0 * math.log10(z[g].mean()) - 10.0
    margin = min(margin, float(np.abs(lj[g] - rel).min()))
    g &= lj > rel
    if not g.any():
        return -math.inf, 1.0, margin
    L = -0.691 + 10.0 * math.log10(z[g].mean())
    gain = 1.0
    if on and peak > 0:
        gain = min(10.0 ** ((float(target) - float(np.float32(L))) / 20.0), 10.0 ** (float(ceiling) / 20.0) / float(peak))
    return L, gain, margin


def pcm_rule(y):
    """writeWavFile's conversion in fp32: clamp to [-1, 1], * 32767, truncation toward zero."""
    return (np.clip(np.asarray(y, np.float32), -1.0, 1.0) * np.float32(32767.0)).astype(np.int32).astype(np.int16)
