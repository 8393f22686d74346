"""The fetch-time expander in numpy (include/stn.h "expander"): the reference of every numeric statement, which is
the contract's recurrence sample by sample in float64 on the fp32-rounded T, S, K, R, kA, delta and Bh; the same in float32, operation
for operation with the contract's fma (the restatement whose deviation from float64 sets the tests' bounds); and a model of the GPU's
decomposition (fp32 chunks of 32 samples, scans in double, fp32 start values) with the faults a scan can have.  Nothing here calls the
library."""
import numpy as np

CHUNK, WG, SCAN = 32, 256, 1024  # samples per chunk, chunks per workgroup, chunks per scan tile
FIELDS = ("threshold_db", "ratio", "knee_db", "range_db", "attack_ms", "hold_ms", "release_ms")
SPEECH = (-50.0, 3.0, 6.0, 24.0, 1.0, 30.0, 150.0)
GATE = (-45.0, 20.0, 0.0, 60.0, 0.5, 50.0, 100.0)


def chunks(W):
    return (W + CHUNK - 1) // CHUNK


def hold_samples(c, rate):
    return int(np.floor(float(np.float32(c[5])) * float(rate) / 1000.0 + 0.5))


def coefs(c, rate):
    """the seven fp32 values the GPU computes with (and the float64 reference is given), as a dict of np.float32; each is formed in
    double from the fp32 fields of the setting and rounded once"""
    t, r, k, rng, a, h, rl = (np.float32(v) for v in c)
    kA = np.float32(-np.expm1(-1000.0 / (float(a) * float(rate))))
    delta = np.float32(float(rng) * 1000.0 / (float(rl) * float(rate)))
    Bh = np.float32(float(delta) * hold_samples(c, rate))
    return dict(T=t, S=np.float32(float(r) - 1.0), K=k, R=rng, kA=kA, delta=delta, Bh=Bh)


def _as(f, dt):
    return {n: dt(v) for n, v in f.items()}


def want(x, f, dt=np.float64):
    """z in [0, R], the attenuation the gain computer wants at every sample, in dB"""
    f = _as(f, dt)
    xg = dt(20) * np.log10(np.maximum(np.abs(np.asarray(x, np.float32).astype(dt)), dt(np.float32(1e-6))))
    d = f["T"] - xg
    d2 = dt(2) * d
    t = d + dt(0.5) * f["K"]
    with np.errstate(divide="ignore", invalid="ignore"):
        knee = (f["S"] * (t * t)) / (dt(2) * f["K"])
    in_knee = (np.abs(d2) <= f["K"]) & (f["K"] > 0)  # (the quadratic only where there is a knee: K = 0 is the hard corner)
    z = np.where(d2 < -f["K"], dt(0), np.where(in_knee, knee, f["S"] * d)).astype(dt)
    return np.minimum(z, f["R"])


def target(z, f, dt=np.float64, boost_partly_open=False):
    """t: the openness R - z, with the hold boost on the fully open samples (fault: on every sample that is open at all)"""
    f = _as(f, dt)
    o = f["R"] - z
    full = (o > 0) if boost_partly_open else (z == 0)
    return np.where(full, o + f["Bh"], o).astype(dt)


def _fma(a, b, c, dt):
    """fma(a, b, c) in dt.  float32: the product of two fp32 values is exact in float64, and the sum is rounded to fp32 from there."""
    if dt is np.float32:
        return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    return a * b + c


def detect(t, f, dt=np.float64, u=None, yl=None):
    """u and yL at every sample of t [rows, W], from zero or from the given start values [rows]"""
    f = _as(f, dt)
    rows, W = t.shape
    u = np.zeros(rows, dt) if u is None else u.astype(dt)
    yl = np.zeros(rows, dt) if yl is None else yl.astype(dt)
    ou, ol = np.empty((W, rows), dt), np.empty((W, rows), dt)
    tt = np.ascontiguousarray(t.T)
    kA, delta, R = f["kA"], f["delta"], f["R"]
    for n in range(W):
        u = np.maximum(tt[n], u - delta)
        yl = _fma(kA, np.minimum(u, R) - yl, yl, dt)
        ou[n] = u
        ol[n] = yl
    return np.ascontiguousarray(ou.T), np.ascontiguousarray(ol.T)


def apply(x, yl, f, dt=np.float64):
    f = _as(f, dt)
    return (np.asarray(x, np.float32).astype(dt) * np.power(dt(10), (yl - f["R"]) / dt(20))).astype(dt)


def _chunked(a, fill=0.0):
    """[rows, W] -> [rows, K, CHUNK] (the last chunk padded) and the chunks' lengths [K]"""
    rows, W = a.shape
    K = chunks(W)
    p = np.full((rows, K * CHUNK), fill, a.dtype)
    p[:, :W] = a
    ln = np.full(K, CHUNK)
    if W % CHUNK:
        ln[-1] = W % CHUNK
    return p.reshape(rows, K, CHUNK), ln


def chunk_run(t, f, dt, u_start=None, yl_start=None):
    """every chunk of t [rows, W] on its own from the start values [rows, K] (None: zero) -> (u at the chunks' ends, yL at their ends,
    yL at every sample [rows, W]); all chunks advance together, a short last chunk stops at its length"""
    f = _as(f, dt)
    rows, W = t.shape
    tc, ln = _chunked(t.astype(dt))
    K = tc.shape[1]
    u = np.zeros((rows, K), dt) if u_start is None else u_start.astype(dt)
    yl = np.zeros((rows, K), dt) if yl_start is None else yl_start.astype(dt)
    out = np.zeros((rows, K, CHUNK), dt)
    for i in range(CHUNK):
        live = (i < ln)[None, :]
        nu = np.maximum(tc[:, :, i], u - f["delta"])
        nl = _fma(f["kA"], np.minimum(nu, f["R"]) - yl, yl, dt)
        u = np.where(live, nu, u)
        yl = np.where(live, nl, yl)
        out[:, :, i] = yl
    return u, yl, out.reshape(rows, K * CHUNK)[:, :W]


class Ref:
    """the contract on x [rows, W] in dt: z, t, u, yL, y per sample, and the four per-chunk arrays the GPU's launches hand on"""

    def __init__(self, x, f, dt=np.float64):
        self.z = want(x, f, dt)
        self.t = target(self.z, f, dt)
        self.u, self.yl = detect(self.t, f, dt)
        self.y = apply(x, self.yl, f, dt)
        self.W = x.shape[1]

    def states(self, f, W, dt=np.float64):
        """s1_end, s1_start, s2_end, s2_start [rows, chunks(W)] of the first W samples"""
        K = chunks(W)
        first = np.arange(K) * CHUNK
        zero = np.zeros((self.t.shape[0], 1), dt)
        s1_start = np.concatenate([zero, self.u[:, first[1:] - 1]], axis=1)
        s2_start = np.concatenate([zero, self.yl[:, first[1:] - 1]], axis=1)
        s1_end, _, _ = chunk_run(self.t[:, :W], f, dt)
        _, s2_end, _ = chunk_run(self.t[:, :W], f, dt, u_start=s1_start)
        return dict(s1_end=s1_end, s1_start=s1_start, s2_end=s2_end, s2_start=s2_start)

    def report(self, f, n):
        """(min of R - yL, count of yL <= R / 2) over each row's first n[row] samples, in this precision"""
        R = self.yl.dtype.type(f["R"])
        att = np.array([float((R - self.yl[r, :k]).min()) if k else float(R) for r, k in enumerate(n)])
        closed = np.array([int((self.yl[r, :k] <= R / 2).sum()) for r, k in enumerate(n)], np.int64)
        return att, closed


def scan(e, combine, drop_carry_at=(), neighbour=False):
    """the chunks' start values [rows, K] from their end values from zero, in double, stored as fp32: s_0 = 0, s_{k+1} = combine(e_k,
    s_k), combine applying one whole chunk to the running value.  Faults: drop_carry_at (chunk indices at which the running value is
    lost, as a tile's carry would be), neighbour (every chunk takes the start value of the chunk in front of it)."""
    rows, K = e.shape
    s = np.zeros((rows, K), np.float64)
    run = np.zeros(rows, np.float64)
    for k in range(K):
        if k in drop_carry_at:
            run = np.zeros(rows, np.float64)
        s[:, k] = run
        run = combine(e[:, k].astype(np.float64), run)
    s = s.astype(np.float32)
    if neighbour:
        s = np.concatenate([np.zeros((rows, 1), np.float32), s[:, :-1]], axis=1)
    return s


def model(x, f, fault=None):
    """The GPU's decomposition in numpy: fp32 chunks, scans in double, fp32 start values -> dict of yl, y and the four state arrays.
    fault: None, ("carry1" | "carry2", chunk index), "neighbour1", "neighbour2" or "boost" (the hold boost on partly open samples)."""
    dt = np.float32
    t = target(want(x, f, dt), f, dt, boost_partly_open=fault == "boost")
    c = float(CHUNK) * float(f["delta"])
    E = (1.0 - float(f["kA"])) ** CHUNK
    drop = {1: (), 2: ()}
    nb = {1: False, 2: False}
    if isinstance(fault, tuple):
        drop[int(fault[0][-1])] = (fault[1],)
    elif fault in ("neighbour1", "neighbour2"):
        nb[int(fault[-1])] = True
    s1_end, _, _ = chunk_run(t, f, dt)
    s1_start = scan(s1_end, lambda e, run: np.maximum(e, run - c), drop[1], nb[1])
    _, s2_end, _ = chunk_run(t, f, dt, u_start=s1_start)
    s2_start = scan(s2_end, lambda e, run: e + E * run, drop[2], nb[2])
    _, _, yl = chunk_run(t, f, dt, u_start=s1_start, yl_start=s2_start)
    return dict(yl=yl, y=apply(x, yl, f, dt), s1_end=s1_end, s1_start=s1_start, s2_end=s2_end, s2_start=s2_start)
