"""Float64 reference of the formant correction behind the pitch shift (include/stn.h "formant"): the geometry, the
windowed lags and their conditioning, Levinson-Durbin, the gain and the float32 tables, the per-frame filter g A_y / A_x from zero state
N samples ahead of the frame, and the Hann cross-fade of two neighbouring frames' outputs.  Written from the rule, not from the kernels:
numpy only.  The chains of all frames of a row are independent and run in lock-step here, one numpy operation per sample index.

`mutant` selects one deliberate mistake (tests/test_formant_cpu.py shows that each lands outside the bounds of the GPU tests):
"no-conditioning", "short-warmup", "ay-both-sides", "swapped-halves"."""
import math

import numpy as np

import pitch_ref as pr

MAX_ORDER = 48
MUTANTS = ("no-conditioning", "short-warmup", "ay-both-sides", "swapped-halves")


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------------
def order(hz):
    return min(MAX_ORDER, max(10, 2 * math.ceil(hz / 2000) + 2))


def plan(hz, W):
    H = pr.hop(hz)
    return dict(H=H, N=2 * H, p=order(hz), frames=-(-W // H) + 1)


def lag_window(hz, p=None):
    """1 at lag 0, exp(-0.5 (2 pi 60 k / hz)^2) at lag k"""
    k = np.arange((order(hz) if p is None else p) + 1, dtype=np.float64)
    return np.exp(-0.5 * (2.0 * np.pi * 60.0 * k / hz) ** 2)


# ---- per frame: lags, conditioning, recursion ---------------------------------------------------------------------------------------------------
def frames32(x, n, hz, W=None):
    """the windowed frames of a row: float32(w[i] x[s_m + i]) widened -> [frames][N] float64"""
    x = np.asarray(x, np.float32)
    W = len(x) if W is None else W
    P = plan(hz, W)
    H, N, F = P["H"], P["N"], P["frames"]
    n = W if n is None else max(0, min(int(n), W))
    pad = np.zeros(H + F * H + N, np.float32)
    pad[H:H + n] = x[:n]
    w = pr.window(hz).astype(np.float32)
    idx = (np.arange(F) * H)[:, None] + np.arange(N)[None, :]  # s_m + H + i into pad
    return (w[None, :] * pad[idx]).astype(np.float64)


def lags(xw, p):
    """R[k] = sum_i xw[i] xw[i + k], k = 0 .. p, in double -> [frames][p + 1]"""
    N = xw.shape[1]
    return np.stack([np.sum(xw[:, :N - k] * xw[:, k:], axis=1) for k in range(p + 1)], axis=1)


def condition(R, hz, mutant=None):
    Rc = np.array(R, np.float64)
    if mutant == "no-conditioning":
        return Rc
    Rc[..., 1:] *= lag_window(hz, Rc.shape[-1] - 1)[1:]
    Rc[..., 0] = 1.0001 * Rc[..., 0] + 1e-9
    return Rc


def levinson(Rc):
    """Levinson-Durbin on conditioned lags [..., p + 1] -> (a [..., p + 1] with a[0] = 1, the final error [...], the reflection
    coefficients [..., p]).  A frame whose R[0] is 0 (only without the conditioning) gives a = (1, 0, ...), E = 1e-9."""
    Rc = np.atleast_2d(np.asarray(Rc, np.float64))
    F, p = Rc.shape[0], Rc.shape[1] - 1
    a = np.zeros((F, p + 1))
    a[:, 0] = 1.0
    refl = np.zeros((F, p))
    dead = Rc[:, 0] == 0.0
    E = np.where(dead, 1.0, Rc[:, 0])
    for i in range(1, p + 1):
        acc = Rc[:, i].copy()
        for j in range(1, i):
            acc += a[:, j] * Rc[:, i - j]
        k = np.where(dead, 0.0, -acc / E)
        a[:, 1:i] = a[:, 1:i] + k[:, None] * a[:, i - 1:0:-1]
        a[:, i] = k
        E = E * (1.0 - k * k)
        refl[:, i - 1] = k
    return a, np.where(dead, 1e-9, E), refl


def lpc(x, n, hz, W=None, mutant=None):
    """-> (a [frames][p + 1], E [frames]) of a row"""
    a, E, _ = levinson(condition(lags(frames32(x, n, hz, W), order(hz)), hz, mutant))
    return a, E


def tables(x, y, n, hz, mutant=None):
    """the stored tables of a row pair -> dict ax, cy (float32 [frames][p + 1]), g, ex, ey (float64 [frames])"""
    a_x, e_x = lpc(x, n, hz, mutant=mutant)
    a_y, e_y = lpc(y, n, hz, mutant=mutant)
    if mutant == "ay-both-sides":
        a_x = a_y
    g = np.clip(np.sqrt(e_x / e_y), 0.5, 2.0)
    return dict(ax=a_x.astype(np.float32), cy=(g[:, None] * a_y).astype(np.float32), g=g, ex=e_x, ey=e_y)


# ---- the filter and the cross-fade --------------------------------------------------------------------------------------------------------------
def chains(y, n, hz, ax, cy, dtype=np.float64, mutant=None):
    """v_m[j] for j in [s_m - N, s_m + N), every frame of a row -> [frames][2 N] of dtype.  float64: the reference.  float32: the
    restatement the bounds of the GPU tests are measured with, every product and every sum rounded, taps in ascending k."""
    y = np.asarray(y, np.float32)
    W = len(y)
    P = plan(hz, W)
    H, N, F, p = P["H"], P["N"], P["frames"], P["p"]
    n = W if n is None else max(0, min(int(n), W))
    L = 2 * N
    lead = 3 * H + p  # pad[lead + j] = y0[j]
    pad = np.zeros(lead + F * H + N + 1, dtype)
    pad[lead:lead + n] = y[:n].astype(dtype)
    n0 = (np.arange(F) - 3) * H
    seg = pad[(n0 + lead - p)[:, None] + np.arange(L + p)[None, :]].copy()  # [frames][p + L]: y0[n0 - p + t]
    seg[:, :p] = 0  # the signal is taken as 0.0 before n0
    if mutant == "short-warmup":
        seg[:, :p + N] = 0  # zero state at s_m: nothing enters before it
    ax = np.asarray(ax).astype(dtype)
    cy = np.asarray(cy).astype(dtype)
    e = cy[:, 0:1] * seg[:, p:p + L]
    for k in range(1, p + 1):
        e = e + cy[:, k:k + 1] * seg[:, p - k:p - k + L]
    v = np.zeros((F, p + L), dtype)
    if dtype == np.float64:
        axr = ax[:, :0:-1]  # tap p first: v[:, t : t + p] holds v[j - p] .. v[j - 1]
        for t in range(L):
            v[:, p + t] = e[:, t] - np.sum(axr * v[:, t:t + p], axis=1)
    else:
        for t in range(L):
            acc = e[:, t]
            for k in range(1, p + 1):
                acc = acc - ax[:, k] * v[:, p + t - k]
            v[:, p + t] = acc
    return v[:, p:]


def crossfade(v, n, hz, W, mutant=None):
    """out[m H + i] = w[H + i] v_m[m H + i] + w[i] v_{m+1}[m H + i], 0 from the span on -> [W] of v's dtype"""
    P = plan(hz, W)
    H, F = P["H"], P["frames"]
    n = W if n is None else max(0, min(int(n), W))
    w = pr.window(hz).astype(np.float32).astype(v.dtype)
    first, second = (w[:H], w[H:]) if mutant == "swapped-halves" else (w[H:], w[:H])
    out = first[None, :] * v[:-1, 3 * H:4 * H] + second[None, :] * v[1:, 2 * H:3 * H]  # [frames - 1][H]
    out = out.reshape(-1)[:W].copy()
    out[n:] = 0
    return out


def apply_tables(y, n, hz, ax, cy, dtype=np.float64, mutant=None):
    """the filter and the cross-fade on given tables -> out [W]"""
    return crossfade(chains(y, n, hz, ax, cy, dtype, mutant), n, hz, len(y), mutant)


def formant(x, y, n, hz, mutant=None):
    """the whole correction in float64 on float32 tables -> (out [W], the tables)"""
    t = tables(x, y, n, hz, mutant)
    return apply_tables(y, n, hz, t["ax"], t["cy"], np.float64, mutant), t


# ---- properties -----------------------------------------------------------------------------------------------------------------------------------
def envelope_db(z, hz, lo, hi, f_lo, f_hi, points=256):
    """the LPC log envelope of z[lo:hi) in dB on `points` frequencies from f_lo to f_hi, its mean over the band removed: the rule's
    order and conditioning on the Hann-windowed segment"""
    seg = np.asarray(z, np.float64)[lo:hi]
    seg = seg * (0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(len(seg)) / len(seg))))
    p = order(hz)
    R = np.array([[seg[:len(seg) - k] @ seg[k:] for k in range(p + 1)]])
    a, _, _ = levinson(condition(R, hz))
    f = np.linspace(f_lo, f_hi, points)
    A = np.exp(-2j * np.pi * f[:, None] * np.arange(p + 1)[None, :] / hz) @ a[0]
    env = -20.0 * np.log10(np.abs(A))
    return env - env.mean()


def period(z, hz, lo, hi, f_lo, f_hi):
    """the period of z[lo:hi) in samples: pitch_ref.autocorr_f0's peak over lags of hz / f_hi .. hz / f_lo, refined by the parabola
    through the peak and its two neighbours (a period half-way between two lags is no tie then) -> (period, the integer lag)"""
    seg = np.asarray(z, np.float64)[lo:hi]
    seg = seg - seg.mean()
    lags_ = np.arange(int(hz / f_hi) - 1, int(hz / f_lo) + 2)
    L = len(seg) - lags_.max()
    r = np.array([seg[:L] @ seg[k:k + L] for k in lags_])
    i = 1 + int(np.argmax(r[1:-1]))
    d = 0.5 * (r[i - 1] - r[i + 1]) / (r[i - 1] - 2.0 * r[i] + r[i + 1])
    return float(lags_[i] + d), int(lags_[i])


def envelope_distance_db(x, z, hz, lo, hi):
    """the RMS over 100 Hz .. min(5 kHz, 0.4 hz) of the difference between the mean-removed envelopes of z and x over [lo, hi)"""
    f_hi = min(5000.0, 0.4 * hz)
    d = envelope_db(z, hz, lo, hi, 100.0, f_hi) - envelope_db(x, hz, lo, hi, 100.0, f_hi)
    return float(np.sqrt(np.mean(d * d)))
