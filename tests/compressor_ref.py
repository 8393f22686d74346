"""The fetch-time compressor in numpy (include/stn.h "compressor"): the reference of every numeric statement, which
is the contract's recurrence sample by sample in float64 on the fp32-rounded T, S, K, kA, kR and makeup; the same in float32, operation
for operation with the contract's two fma (the restatement whose deviation from float64 sets the tests' bounds); and a model of the
GPU's decomposition (fp32 chunks of 32 samples, scans in double, fp32 start values) with the faults a scan can have.  Nothing here calls the library."""
import numpy as np

CHUNK, WG, SCAN = 32, 256, 1024  # samples per chunk, chunks per workgroup, chunks per scan tile
FIELDS = ("threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "makeup_db")
SPEECH = (-24.0, 3.0, 6.0, 5.0, 120.0, 0.0)


def chunks(W):
    return (W + CHUNK - 1) // CHUNK


def k_of(ms, rate):
    """k = -expm1(-1000 / (ms rate)) in double, ms as the fp32 the setting holds"""
    return -np.expm1(-1000.0 / (float(np.float32(ms)) * float(rate)))


def coefs(c, rate):
    """the six fp32 values the GPU computes with (and the float64 reference is given), as a dict of np.float32"""
    t, r, k, a, rl, m = (np.float32(v) for v in c)
    return dict(T=t, S=np.float32(1.0 / float(r) - 1.0), K=k, kA=np.float32(k_of(a, rate)), kR=np.float32(k_of(rl, rate)), mk=m)


def _as(f, dt):
    return {n: dt(v) for n, v in f.items()}


def want(x, f, dt=np.float64):
    """z >= 0, the reduction the gain computer wants at every sample, in dB"""
    f = _as(f, dt)
    xg = dt(20) * np.log10(np.maximum(np.abs(np.asarray(x, np.float32).astype(dt)), dt(np.float32(1e-6))))
    d = xg - f["T"]
    d2 = dt(2) * d
    t = d + dt(0.5) * f["K"]
    with np.errstate(divide="ignore", invalid="ignore"):
        knee = (-f["S"] * (t * t)) / (dt(2) * f["K"])
    in_knee = (np.abs(d2) <= f["K"]) & (f["K"] > 0)  # (the quadratic only where there is a knee: K = 0 is the hard corner)
    return np.where(d2 < -f["K"], dt(0), np.where(in_knee, knee, -f["S"] * d)).astype(dt)


def _fma(a, b, c, dt):
    """fma(a, b, c) in dt.  float32: the product of two fp32 values is exact in float64, and the sum is rounded to fp32 from there."""
    if dt is np.float32:
        return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    return a * b + c


def detect(z, f, dt=np.float64, y1=None, yl=None):
    """y1 and yL at every sample of z [rows, W], from zero or from the given start values [rows]"""
    f = _as(f, dt)
    rows, W = z.shape
    y1 = np.zeros(rows, dt) if y1 is None else y1.astype(dt)
    yl = np.zeros(rows, dt) if yl is None else yl.astype(dt)
    o1, ol = np.empty((W, rows), dt), np.empty((W, rows), dt)
    zt = np.ascontiguousarray(z.T)
    kA, kR = f["kA"], f["kR"]
    for n in range(W):
        y1 = np.maximum(zt[n], _fma(-kR, y1, y1, dt))
        yl = _fma(kA, y1 - yl, yl, dt)
        o1[n] = y1
        ol[n] = yl
    return np.ascontiguousarray(o1.T), np.ascontiguousarray(ol.T)


def apply(x, yl, f, dt=np.float64):
    f = _as(f, dt)
    return (np.asarray(x, np.float32).astype(dt) * np.power(dt(10), (f["mk"] - yl) / dt(20))).astype(dt)


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


def chunk_run(z, f, dt, y1_start=None, yl_start=None):
    """every chunk of z [rows, W] on its own from the start values [rows, K] (None: zero) -> (y1 at the chunks' ends, yL at their
    ends, yL at every sample [rows, W]); all chunks advance together, a short last chunk stops at its length"""
    f = _as(f, dt)
    rows, W = z.shape
    zc, ln = _chunked(z.astype(dt))
    K = zc.shape[1]
    y1 = np.zeros((rows, K), dt) if y1_start is None else y1_start.astype(dt)
    yl = np.zeros((rows, K), dt) if yl_start is None else yl_start.astype(dt)
    out = np.zeros((rows, K, CHUNK), dt)
    for i in range(CHUNK):
        live = (i < ln)[None, :]
        n1 = np.maximum(zc[:, :, i], _fma(-f["kR"], y1, y1, dt))
        nl = _fma(f["kA"], n1 - yl, yl, dt)
        y1 = np.where(live, n1, y1)
        yl = np.where(live, nl, yl)
        out[:, :, i] = yl
    return y1, yl, out.reshape(rows, K * CHUNK)[:, :W]


class Ref:
    """the contract on x [rows, W] in dt: z, y1, yL, y per sample, and the four per-chunk arrays the GPU's launches hand on"""

    def __init__(self, x, f, dt=np.float64):
        self.z = want(x, f, dt)
        self.y1, self.yl = detect(self.z, f, dt)
        self.y = apply(x, self.yl, f, dt)
        self.W = x.shape[1]

    def states(self, f, W, dt=np.float64):
        """s1_end, s1_start, s2_end, s2_start [rows, chunks(W)] of the first W samples"""
        K = chunks(W)
        first = np.arange(K) * CHUNK
        zero = np.zeros((self.z.shape[0], 1), dt)
        s1_start = np.concatenate([zero, self.y1[:, first[1:] - 1]], axis=1)
        s2_start = np.concatenate([zero, self.yl[:, first[1:] - 1]], axis=1)
        s1_end, _, _ = chunk_run(self.z[:, :W], f, dt)
        _, s2_end, _ = chunk_run(self.z[:, :W], f, dt, y1_start=s1_start)
        return dict(s1_end=s1_end, s1_start=s1_start, s2_end=s2_end, s2_start=s2_start)


def scan(e, P, combine, drop_carry_at=(), neighbour=False):
    """the chunks' start values [rows, K] from their end values from zero, in double, stored as fp32: s_0 = 0, s_{k+1} = combine(e_k,
    P s_k) with P the factor of one whole chunk.  Faults: drop_carry_at (chunk indices at which the running value is lost, as a tile's
    carry would be), neighbour (every chunk takes the start value of the chunk in front of it)."""
    rows, K = e.shape
    s = np.zeros((rows, K), np.float64)
    run = np.zeros(rows, np.float64)
    for k in range(K):
        if k in drop_carry_at:
            run = np.zeros(rows, np.float64)
        s[:, k] = run
        run = combine(e[:, k].astype(np.float64), P * run)
    s = s.astype(np.float32)
    if neighbour:
        s = np.concatenate([np.zeros((rows, 1), np.float32), s[:, :-1]], axis=1)
    return s


def model(x, f, fault=None):
    """The GPU's decomposition in numpy: fp32 chunks, scans in double, fp32 start values -> dict of yl, y and the four state arrays.
    fault: None, ("carry1" | "carry2", chunk index), "neighbour1" or "neighbour2"."""
    dt = np.float32
    z = want(x, f, dt)
    D = (1.0 - float(f["kR"])) ** CHUNK
    E = (1.0 - float(f["kA"])) ** CHUNK
    drop = {1: (), 2: ()}
    nb = {1: False, 2: False}
    if isinstance(fault, tuple):
        drop[int(fault[0][-1])] = (fault[1],)
    elif fault:
        nb[int(fault[-1])] = True
    s1_end, _, _ = chunk_run(z, f, dt)
    s1_start = scan(s1_end, D, np.maximum, drop[1], nb[1])
    _, s2_end, _ = chunk_run(z, f, dt, y1_start=s1_start)
    s2_start = scan(s2_end, E, np.add, drop[2], nb[2])
    _, _, yl = chunk_run(z, f, dt, y1_start=s1_start, yl_start=s2_start)
    return dict(yl=yl, y=apply(x, yl, f, dt), s1_end=s1_end, s1_start=s1_start, s2_end=s2_end, s2_start=s2_start)
