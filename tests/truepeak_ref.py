"""The true-peak contract (include/stn.h "true peak") in numpy / float64: the 4x oversampling filter, the
envelope, the per-chunk peaks, and the limiter's curve driven by the envelope."""
import numpy as np

import limiter_ref

F32 = np.float32
P, T, OFF, BETA = 4, 16, 7, 8.0
CHUNK = 32
EPS = 2.0 ** -24


def design():
    """float32 [4, 16]: Kaiser-windowed sinc (beta 8, cutoff at the input Nyquist), every phase normalized in float64 to DC gain 1;
    sinc is exactly 0 at the non-zero integers"""
    taps = np.zeros((P, T), F32)
    for p in range(P):
        d = p - (np.arange(T) - OFF) * P
        x = d / float(P)
        sinc = np.where(d == 0, 1.0, np.where(d % P == 0, 0.0, np.sin(np.pi * x) / np.where(d == 0, 1.0, np.pi * x)))
        r = d / (T * P / 2.0)
        w = np.where(r * r < 1.0, np.i0(BETA * np.sqrt(np.maximum(1.0 - r * r, 0.0))) / np.i0(BETA), 0.0)
        h = sinc * w
        taps[p] = (h / h.sum()).astype(F32)
    return taps


TAPS = design()


def _windows(x, n, g):
    """v [W] float32 (x * g), and win [n + 1, 16] float64: row e holds v[i - 7 .. i + 8] for i = e - 1, zero outside [0, n)"""
    v = (np.asarray(x, F32) * F32(g)).astype(F32)
    n = int(n)
    xp = np.concatenate([np.zeros(8), v[:n].astype(np.float64), np.zeros(8)])  # xp[k] = x[k - 8]
    return v, np.lib.stride_tricks.sliding_window_view(xp, T)[:n + 1]          # window e starts at x[e - 8] = x[(e - 1) - 7]


def oversampled(x, n, g=1.0, taps=None, phases=(1, 2, 3)):
    """(U [n + 1] float64, tolU [n + 1]): U[e] = max_ph |u[e - 1][ph]| and, per point, the bound tol_u of the phase that attains it
    widened to the largest over the phases (a max of values each within its own bound lies within the largest of them)"""
    taps = TAPS if taps is None else taps
    _, win = _windows(x, n, g)
    h = taps.astype(np.float64)[list(phases)]
    u = np.abs(win @ h.T)                              # [n + 1, phases]
    tol = 18.0 * EPS * (np.abs(win) @ np.abs(h).T)
    return u.max(axis=1), tol.max(axis=1)


def envelope(x, n, g=1.0, taps=None, phases=(1, 2, 3)):
    """(p [W] float64, tol [W] float64): p[i] = max(|v[i]|, U[i-1], U[i]) for i < n, |v[i]| behind (exact there: tol 0)"""
    v, _ = _windows(x, n, g)
    n = int(n)
    p = np.abs(v.astype(np.float64))
    tol = np.zeros(v.size)
    if n:
        U, tU = oversampled(x, n, g, taps, phases)
        p[:n] = np.maximum(p[:n], np.maximum(U[:-1], U[1:]))
        tol[:n] = np.maximum(tU[:-1], tU[1:])
    return p, tol


def true_peak(x, n=None, g=1.0):
    x = np.asarray(x, F32)
    n = x.size if n is None else int(n)
    return float(envelope(x, n, g)[0][:n].max()) if n else 0.0


def chunk_peaks(env, n, W):
    """pk [ceil(W / 32)] of an envelope (any dtype, kept): max over the chunk's samples inside the span, +0.0 when there are none"""
    Ks = (W + CHUNK - 1) // CHUNK
    e = np.zeros(Ks * CHUNK, env.dtype)
    e[:int(n)] = env[:int(n)]
    return e.reshape(Ks, CHUNK).max(axis=1)


def tol_u(x, n, g=1.0):
    """the bound on |env_device - env| per sample: 18 * 2^-24 * sum_j |h_j| |x_j| of the contributing oversampled points"""
    return envelope(x, n, g)[1]


def limit_row_env(x, n, g, ceiling_db, hz, ms, env=None):
    """limiter_ref.limit_row with r formed from the true-peak envelope of v = x * g: r[j] = 1 where env[j] <= c, else c / env[j]
    (float32), 1 outside [0, n).  env: the float32 envelope to use (the device's), or None for the reference's rounded to float32."""
    x = np.asarray(x, F32)
    W = x.size
    n = int(n)
    A = limiter_ref.samples(hz, ms)
    c = limiter_ref.ceiling(ceiling_db)
    w = limiter_ref.window(hz, ms).astype(np.float64)
    v = (x * F32(g)).astype(F32)
    e = envelope(x, n, g)[0].astype(F32) if env is None else np.asarray(env, F32)
    r = np.ones(W, F32)
    over = e[:n] > c
    r[:n][over] = (c / e[:n][over]).astype(F32)
    rp = np.concatenate([np.ones(A, F32), r, np.ones(A, F32)])
    me = np.lib.stride_tricks.sliding_window_view(rp, A + 1).min(axis=1)
    M = np.minimum(me[:W], me[A:])
    tot = np.convolve(me.astype(np.float64), w, mode="valid")
    s = np.where(M == 1.0, 1.0, np.minimum(np.minimum(tot, r.astype(np.float64)), limiter_ref.BELOW_ONE))
    vd = v.astype(np.float64)
    y = np.clip(vd, -float(c), float(c))
    y[:n] = np.clip(vd[:n] * s[:n], -float(c), float(c))
    s_out = s.copy()
    s_out[n:] = 1.0  # (the padding has no curve)
    return dict(y=y, s=s_out, v=v, r=r, M=M, c=c, A=A)


# ---- the rows of the kernel test ------------------------------------------------------------------------------------------------------
SPANS = [0, 1, 7, 8, 9, 31, 32, 33, 8191, 8192, 8193, 2 * 8192 + 5]
POISON = 1e3


def tone45(W, amp=1.0):
    """fs/4 sampled at 45 degrees: sample peak amp / sqrt(2), true peak amp"""
    return (amp * np.sin(2 * np.pi * 0.25 * np.arange(W) + np.pi / 4)).astype(F32)


def kernel_rows(W):
    """(x [R, W] float32, n [R]): for every span the tone, the clicks and +1 +1 pairs (at sample 0, n - 1, across the lane seam 31|32
    and the workgroup seam 8191|8192), single clicks and the alternating burst, and coloured noise with DC; 1e3 behind every span"""
    rng = np.random.default_rng(7)
    rows, spans = [], []
    for n in SPANS:
        kinds = []
        kinds.append(tone45(W, 0.9))
        clicks = np.zeros(W)
        for i in (0, n - 1, 31, 8191):
            if 0 <= i < n:
                clicks[i] = 1.0
                if i + 1 < n:
                    clicks[i + 1] = 1.0      # a +1 +1 pair straddling the seam behind i
        kinds.append(clicks)
        single = np.zeros(W)
        for i in (0, n - 1, 32, 8192, 300):
            if 0 <= i < n:
                single[i] = -1.0 if i % 3 else 1.0
        b = min(max(n - 8, 0), 8188)
        for q, s in enumerate((1, -1, 1, -1)):
            if b + q < n:
                single[b + q] = s
        kinds.append(single)
        z = rng.standard_normal(W)
        col = np.convolve(z, [0.5, 0.3, 0.2, -0.1], mode="same") * 0.4 + 0.1
        col[0] = POISON                      # the row before ends in 1e3 and this one starts with it: a leak across a row shows
        kinds.append(col)
        for k in kinds:
            r = np.asarray(k, np.float64).copy()
            r[n:] = POISON
            rows.append(r.astype(F32))
            spans.append(n)
    return np.stack(rows), np.array(spans, np.int64)


def env_violations(env_dev, x, n, g=1.0):
    """indices where a device envelope (float32 [W]) misses the contract for row x with span n: outside tol_u of the float64 envelope
    inside the span, or not |x * g| bit for bit behind it"""
    ref, tol = envelope(x, n, g)
    e = np.asarray(env_dev, F32)
    n = int(n)
    bad = np.abs(e[:n].astype(np.float64) - ref[:n]) > tol[:n]
    v = np.abs((np.asarray(x, F32) * F32(g)).astype(F32))
    tail = e[n:].view(np.uint32) != v[n:].view(np.uint32)
    return np.concatenate([np.flatnonzero(bad), n + np.flatnonzero(tail)])
