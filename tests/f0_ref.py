"""The pitch report's contract (include/stn.h "f0") in float64 numpy, written from the definitions: YIN steps 1 to
5 on the box-averaged row, the per-row statistics, the decidability of a frame and the first-order error bound of the fp32 device
against this reference.  Nothing here reads the library."""
import math

import numpy as np

DEFAULTS = {"fmin_hz": 60.0, "fmax_hz": 500.0, "threshold": 0.15, "gate_db": -60.0}
U32 = 2.0 ** -24  # unit roundoff of fp32


def params(p=None):
    """the parameter set as the ABI holds it: fp32 fields, read as float64"""
    q = dict(DEFAULTS)
    q.update(p or {})
    return {k: float(np.float32(v)) for k, v in q.items()}


def plan(hz, n, p=None):
    p = params(p)
    k = max(1, hz // 16000)
    ha = hz / k
    hop = int(math.floor(ha / 100.0 + 0.5))
    tau_max = int(math.ceil(ha / p["fmin_hz"]))
    tau_min = int(math.floor(ha / p["fmax_hz"]))
    na = n // k
    frames = 0 if na < 2 * tau_max else (na - 2 * tau_max) // hop + 1
    return {"k": k, "ha": ha, "hop": hop, "tau_min": tau_min, "tau_max": tau_max, "frames": frames, "na": na}


def analysis(x, hz):
    """u[j] = mean of x[jk .. jk + k), j < n div k"""
    x = np.asarray(x, np.float64)
    k = max(1, hz // 16000)
    na = x.size // k
    return x[: na * k].reshape(na, k).sum(axis=1) / k if na else np.zeros(0)


def difference(w, T):
    """d(tau), tau = 0 .. T, of one frame w[0 .. 2T): the direct squared difference"""
    win = np.lib.stride_tricks.sliding_window_view(w[: 2 * T], T)[: T + 1]  # win[tau][j] = w[j + tau]
    v = w[None, :T] - win
    return np.einsum("ij,ij->i", v, v)


def normalise(d):
    """d'(0) = 1, d'(tau) = d(tau) tau / sum_{i = 1 .. tau} d(i), 1 where that sum is 0"""
    T = d.size - 1
    run = np.concatenate(([0.0], np.cumsum(d[1:])))
    dp = np.ones(T + 1)
    ok = run > 0.0
    ok[0] = False
    tau = np.arange(T + 1, dtype=np.float64)
    dp[ok] = d[ok] * tau[ok] / run[ok]
    return dp, run


def decide(dp, tau_min, T, threshold):
    """tau^ (0: no lag in [tau_min, T) is under the threshold)"""
    below = np.nonzero(dp[tau_min:T] < threshold)[0]
    if below.size == 0:
        return 0
    lag = tau_min + int(below[0])
    while lag + 1 < T and dp[lag + 1] < dp[lag]:
        lag += 1
    return lag


def refine(dp, lag, ha):
    a, b, c = dp[lag - 1], dp[lag], dp[lag + 1]
    den = a - 2.0 * b + c
    off = min(1.0, max(-1.0, 0.5 * (a - c) / den)) if den > 0.0 else 0.0
    return ha / (lag + off), b


def track(x, hz, p=None, detail=False):
    """(f0, ap, lag) [frames] of one row; with detail also a list of per-frame dicts: d, dp, run (float64 [T + 1]), e2 (the sum of u^2
    over the frame's 2T samples), gated"""
    p = params(p)
    g = plan(hz, np.asarray(x).size, p)
    T, F = g["tau_max"], g["frames"]
    u = analysis(x, hz)
    f0, ap, lag, det = np.zeros(F), np.ones(F), np.zeros(F, np.int32), []
    gate = 10.0 ** (p["gate_db"] / 10.0)
    for t in range(F):
        w = u[t * g["hop"]: t * g["hop"] + 2 * T]
        gated = float(np.dot(w[:T], w[:T])) / T < gate
        d = difference(w, T)
        dp, run = normalise(d)
        if not gated:
            lag[t] = decide(dp, g["tau_min"], T, p["threshold"])
            if lag[t]:
                f0[t], ap[t] = refine(dp, int(lag[t]), g["ha"])
        if detail:
            det.append({"d": d, "dp": dp, "run": run, "e2": float(np.dot(w, w)), "gated": gated})
    return (f0, ap, lag, det) if detail else (f0, ap, lag)


def stats(f0):
    """the statistics of a track (0 = unvoiced): lower median, geometric mean, min, max over the voiced frames"""
    f0 = np.asarray(f0, np.float64)
    v = np.sort(f0[f0 > 0.0])
    out = {"frames": int(f0.size), "voiced": int(v.size), "median_hz": 0.0, "mean_hz": 0.0, "min_hz": 0.0, "max_hz": 0.0}
    if v.size:
        out.update(median_hz=float(v[(v.size - 1) // 2]), mean_hz=float(2.0 ** np.mean(np.log2(f0[f0 > 0.0]))), min_hz=float(v[0]), max_hz=float(v[-1]))
    return out


def decidable(det, lag, g, p=None):
    """A frame is decidable when the reference's voicing and tau^ are the same at thresholds 0.15 (1 +- 1e-3) (the parameter's own value
    in place of 0.15) and d'(tau^) lies at least 1e-5 under both neighbours.  A gated frame is decidable: its level decides."""
    p = params(p)
    if det["gated"]:
        return True
    T = g["tau_max"]
    for s in (1.0 - 1e-3, 1.0 + 1e-3):
        if decide(det["dp"], g["tau_min"], T, p["threshold"] * s) != lag:
            return False
    if lag == 0:
        return True
    dp = det["dp"]
    return bool(dp[lag] + 1e-5 <= dp[lag - 1] and dp[lag] + 1e-5 <= dp[lag + 1])


def moved(det, lag, g, step):
    """the reference's (f0, ap) with tau^ moved by step lags (None when that leaves [tau_min, T))"""
    m = lag + step
    if lag == 0 or m < max(1, g["tau_min"]) or m >= g["tau_max"]:
        return None
    return refine(det["dp"], m, g["ha"])


def device_bound(det, lag, g, terms=False):
    """(bound of |f0_dev - f0_ref| / f0_ref, bound of |ap_dev - ap_ref|) for a decidable voiced frame (terms=True: the curvature D and
    the error sum S below instead): DESIGN.md section 27's derivation
    evaluated on the reference's own d, running sum and curvature.  With u = 2^-24:
      the staged sample is the exact box average rounded once to fp32 (nothing for k = 1): |du_j| <= eta |u_j|, eta = u (0 for k = 1), so
        the exact d of the staged samples is within 4 eta sqrt(d E2) + 4 eta^2 E2 of d (E2 the frame's sum of u^2, Cauchy-Schwarz);
      a term (fl(a - b))^2 carries (1 + u)^3 and the sequential sum of T non-negative terms (1 + u)^(T - 1): relative (T + 2) u;
      the running sum C adds non-negative terms through a wave scan (6 levels) and the carries of at most ceil(T / 64) tiles: relative
        (6 + ceil(T / 64)) u on top of its terms' own (T + 2) u;
      d' = fl(fl(d tau) / C): 2 u more.
    So |dd'| <= d' (2T + 12 + ceil(T / 64)) u + d' sum_i abs(d(i)) / C + tau abs(d) / C to first order (two sums of T fp32 terms), the
    second-order remainder covered by 1 / (1 - (2T + 12 + ceil(T / 64)) u).  The parabola is evaluated in double on those fp32 d', so with
    S = |da| + 2 |db| + |dc| < D = a - 2b + c the offset moves by at most (0.5 (|da| + |dc|) + |off| S) / (D - S), and f0 = ha / tau*
    is rounded once to fp32."""
    T = g["tau_max"]
    eta = 0.0 if g["k"] == 1 else U32
    d, run, dp = det["d"], det["run"], det["dp"]
    abs_d = 4.0 * eta * np.sqrt(d * det["e2"]) + 4.0 * eta * eta * det["e2"]
    abs_run = np.concatenate(([0.0], np.cumsum(abs_d[1:])))
    rounding = (2 * T + 12 + -(-T // 64)) * U32
    grow = 1.0 / (1.0 - rounding)

    def err(tau):
        if run[tau] <= 0.0:
            return 0.0
        return grow * (dp[tau] * (rounding + abs_run[tau] / run[tau]) + tau * abs_d[tau] / run[tau])

    a, b, c = dp[lag - 1], dp[lag], dp[lag + 1]
    da, db, dc = err(lag - 1), err(lag), err(lag + 1)
    D, S = a - 2.0 * b + c, da + 2.0 * db + dc
    if terms:
        return D, S
    if not D > S:
        return math.inf, db + U32 * b
    off = min(1.0, max(-1.0, 0.5 * (a - c) / D))
    doff = (0.5 * (da + dc) + abs(off) * S) / (D - S)
    tau_star = lag + off
    return doff / (tau_star - doff) + 2.0 * U32, db + U32 * b


def cents(f, ref):
    return 1200.0 * math.log2(f / ref)
