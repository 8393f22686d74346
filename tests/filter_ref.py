"""Float64 statements of the fetch-time biquad chain (include/stn.h "filter chain"), numpy only and independent of
the engine: the designer restated from the RBJ Audio-EQ-Cookbook, the response of a set of coefficients, the chain as its sample-by-
sample recurrence with the state at every 32-sample chunk boundary (in float64: the reference; in float32 without fused multiply-add:
the restatement the bounds come from), and a numpy model of the kernels' decomposition with the faults the tests must be able to see."""
import math

import numpy as np

TYPES = ("highpass", "lowpass", "notch", "peak", "lowshelf", "highshelf")
CHUNK = 32
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0)


def chunks(n):
    return (int(n) + CHUNK - 1) // CHUNK


def design(kind, freq_hz, q, gain_db, rate_hz):
    """b0 b1 b2 a1 a2 (a0 = 1) of the cookbook's section, float64.  freq_hz, q and gain_db are taken as the float32 values the C ABI
    carries.  1 - cos w0 is written 2 sin^2(w0 / 2): the same number, without the cancellation at a low corner."""
    f, q, g = (float(np.float32(v)) for v in (freq_hz, q, gain_db))
    w0 = 2.0 * math.pi * f / float(rate_hz)
    cs, sn, sh = math.cos(w0), math.sin(w0), math.sin(0.5 * w0)
    omc, opc = 2.0 * sh * sh, 1.0 + cs
    alpha = sn / (2.0 * q)
    A = math.pow(10.0, g / 40.0)
    if kind == "highpass":
        b, a = (0.5 * opc, -opc, 0.5 * opc), (1 + alpha, -2 * cs, 1 - alpha)
    elif kind == "lowpass":
        b, a = (0.5 * omc, omc, 0.5 * omc), (1 + alpha, -2 * cs, 1 - alpha)
    elif kind == "notch":
        b, a = (1.0, -2 * cs, 1.0), (1 + alpha, -2 * cs, 1 - alpha)
    elif kind == "peak":
        b, a = (1 + alpha * A, -2 * cs, 1 - alpha * A), (1 + alpha / A, -2 * cs, 1 - alpha / A)
    elif kind == "lowshelf":
        r = 2.0 * math.sqrt(A) * alpha
        b = (A * ((A + 1) - (A - 1) * cs + r), 2 * A * ((A - 1) - (A + 1) * cs), A * ((A + 1) - (A - 1) * cs - r))
        a = ((A + 1) + (A - 1) * cs + r, -2 * ((A - 1) + (A + 1) * cs), (A + 1) + (A - 1) * cs - r)
    elif kind == "highshelf":
        r = 2.0 * math.sqrt(A) * alpha
        b = (A * ((A + 1) + (A - 1) * cs + r), -2 * A * ((A - 1) + (A + 1) * cs), A * ((A + 1) + (A - 1) * cs - r))
        a = ((A + 1) - (A - 1) * cs + r, 2 * ((A - 1) - (A + 1) * cs), (A + 1) - (A - 1) * cs - r)
    else:
        raise ValueError(kind)
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]])


def response_db(coefs, rate_hz, freq_hz):
    """Magnitude in dB at freq_hz of the cascade of the sections coefs [n, 5] (b0 b1 b2 a1 a2), evaluated in float64."""
    c = np.atleast_2d(np.asarray(coefs, np.float64))
    w = 2.0 * np.pi * np.asarray(freq_hz, np.float64) / float(rate_hz)
    z1, z2 = np.exp(-1j * w), np.exp(-2j * w)
    db = np.zeros(w.shape)
    for b0, b1, b2, a1, a2 in c:
        db = db + 20.0 * np.log10(np.abs((b0 + b1 * z1 + b2 * z2) / (1.0 + a1 * z1 + a2 * z2)))
    return db


def butterworth_band_db(freq_hz, lo_hz, hi_hz, rate_hz, order=4):
    """Closed form: the magnitude in dB of an order-`order` Butterworth high-pass at lo_hz in series with a low-pass at hi_hz, both
    bilinear-transformed with their corners pre-warped (what sections of the cookbook's high- and low-pass make of the Butterworth Qs):
    |H|^2 = 1 / (1 + (W_lo / W)^(2 n)) / (1 + (W / W_hi)^(2 n)), W = tan(pi f / rate)."""
    W = np.tan(np.pi * np.asarray(freq_hz, np.float64) / rate_hz)
    Wl, Wh = math.tan(math.pi * lo_hz / rate_hz), math.tan(math.pi * hi_hz / rate_hz)
    return -10.0 * np.log10(1.0 + (Wl / W) ** (2 * order)) - 10.0 * np.log10(1.0 + (W / Wh) ** (2 * order))


def passes_of(c32):
    """The chain's float32 sections c32 [n, 5] as section passes [P, 10] of two biquads, an odd count padded with the identity."""
    c = [np.asarray(v, np.float32) for v in c32]
    if len(c) % 2:
        c.append(np.asarray(IDENTITY, np.float32))
    return np.stack([np.concatenate(c[i:i + 2]) for i in range(0, len(c), 2)])


def chain_states(x, passes, dtype=np.float64, reset_every=0):
    """The chain as its recurrence, one sample at a time, every product and sum rounded to dtype (no fused multiply-add), per pass p
        v = b0 u + s1;  s1 = (b1 u + s2) - a1 v;  s2 = b2 u - a2 v        (passes[p][0:5])
        y = c0 v + t1;  t1 = (c1 v + t2) - d1 y;  t2 = c2 v - d2 y        (passes[p][5:10])
    with y the next pass's u, every row from zero state at its sample 0.  x [R, N]; passes [P, 10].
    Returns (start, end, y): start [P, R, K, 4] pass p's state (s1, s2, t1, t2) before sample 32 k; end [P, R, K, 4] the state chunk k
    of pass p's input ends in when it starts from zero state (after its last sample below N); y [R, N] the last pass's output.
    K = chunks(N).  reset_every = S > 0 models a lost carry: every pass's state is zeroed before each sample that is a multiple of S.
    (The passes run one sample apart in one loop, pass p at sample i - p, so a chain costs the loop of one pass.)"""
    x = np.atleast_2d(np.asarray(x))
    R, N = x.shape
    c = np.asarray(passes).astype(dtype)
    P, K = c.shape[0], chunks(N)
    cc = [c[:, j][:, None] for j in range(10)]
    xt = np.ascontiguousarray(x.astype(dtype).T)
    s1, s2, t1, t2 = (np.zeros((P, R), dtype) for _ in range(4))
    start = np.zeros((P, R, K, 4), dtype)
    U = np.zeros((N + P, P, R), dtype)  # U[i][p]: pass p's input at sample i - p
    y = np.zeros((N, R), dtype)
    prev = np.zeros((P, R), dtype)
    zero = np.zeros(R, dtype)
    for i in range(N + P - 1):
        u = U[i]
        u[0] = xt[i] if i < N else zero
        u[1:] = prev[:-1]
        for p in range(P):
            j = i - p
            if 0 <= j < N:
                if reset_every and j % reset_every == 0:
                    s1[p] = 0; s2[p] = 0; t1[p] = 0; t2[p] = 0
                if j % CHUNK == 0:
                    st = start[p, :, j // CHUNK]
                    st[:, 0], st[:, 1], st[:, 2], st[:, 3] = s1[p], s2[p], t1[p], t2[p]
        v = cc[0] * u + s1
        s1 = (cc[1] * u + s2) - cc[3] * v
        s2 = cc[2] * u - cc[4] * v
        yy = cc[5] * v + t1
        t1 = (cc[6] * v + t2) - cc[8] * yy
        t2 = cc[7] * v - cc[9] * yy
        prev = yy
        if i >= P - 1:
            y[i - (P - 1)] = yy[P - 1]
    # pass p's input as [R, N]
    ins = [np.ascontiguousarray(U[p:p + N, p].T) for p in range(P)]
    end = np.stack([chunk_ends(ins[p], c[p], dtype) for p in range(P)])
    return start, end, np.ascontiguousarray(y.T)


def _step(cc, u, e):
    v = cc[0] * u + e[0]
    a = (cc[1] * u + e[1]) - cc[3] * v
    b = cc[2] * u - cc[4] * v
    yy = cc[5] * v + e[2]
    p = (cc[6] * v + e[3]) - cc[8] * yy
    q = cc[7] * v - cc[9] * yy
    return yy, (a, b, p, q)


def chunk_ends(u, coef, dtype, start=None, out=None):
    """Every chunk of u [R, N] through one pass (coef [10]) side by side, from zero state or from start [R, K, 4]: the end states
    [R, K, 4] after each chunk's last sample below N; out (or None) [R, K * 32] receives the outputs."""
    R, N = u.shape
    K = chunks(N)
    uc = np.pad(u.astype(dtype), ((0, 0), (0, K * CHUNK - N))).reshape(R, K, CHUNK)
    cc = np.asarray(coef).astype(dtype)
    e = tuple(np.zeros((R, K), dtype) if start is None else start[:, :, j].astype(dtype) for j in range(4))
    for i in range(CHUNK):
        live = (np.arange(K)[None, :] * CHUNK + i) < N
        yy, n = _step(cc, uc[:, :, i], e)
        e = tuple(np.where(live, n[j], e[j]) for j in range(4))
        if out is not None:
            out[:, i::CHUNK] = yy
    return np.stack(e, axis=-1)


def transition(coef):
    """M = A^32 (float64) of the zero-input state transition A the pass's float32 coefficients define, state (s1, s2, t1, t2)."""
    c = np.asarray(coef, np.float32).astype(np.float64)
    A = np.array([[-c[3], 1, 0, 0],
                  [-c[4], 0, 0, 0],
                  [c[6] - c[8] * c[5], 0, -c[8], 1],
                  [c[7] - c[9] * c[5], 0, -c[9], 0]])
    return np.linalg.matrix_power(A, CHUNK)


def decomposed(x, passes, tile=1024, fault=None):
    """A numpy model of the kernels' decomposition: per pass, every chunk from zero state in float32, the start states
    s_{k+1} = M s_k + e_k in float64 stored as float32, every chunk again from its start state in float32, float32 between the passes.
    Returns (start, end, y) shaped as chain_states'.  fault: None; "carry": the scan's carry into a tile is dropped (chunk t * tile
    starts from zero state); "chunk": every start state is taken from the chunk before (chunk k uses s_{k-1})."""
    u = np.atleast_2d(np.asarray(x, np.float32))
    R, N = u.shape
    K = chunks(N)
    starts, ends = [], []
    for coef in np.asarray(passes, np.float32):
        e = chunk_ends(u, coef, np.float32)
        M = transition(coef)
        s = np.zeros((R, K, 4), np.float64)
        run = np.zeros((R, 4))
        for k in range(1, K):
            run = run @ M.T + e[:, k - 1].astype(np.float64)
            if fault == "carry" and k % tile == 0:
                run = np.zeros((R, 4))
            s[:, k] = run
        if fault == "chunk":
            s[:, 1:] = s[:, :-1].copy()
        s32 = s.astype(np.float32)
        out = np.zeros((R, K * CHUNK), np.float32)
        chunk_ends(u, coef, np.float32, start=s32, out=out)
        starts.append(s32)
        ends.append(e)
        u = out[:, :N]
    return np.stack(starts), np.stack(ends), u
