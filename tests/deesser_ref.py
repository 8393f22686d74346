"""The fetch-time de-esser in numpy (include/stn.h "de-esser"), built on filter_ref (the band) and compressor_ref
(the detector): the reference of every numeric statement, which is the contract's recurrence sample by sample in float64 on the
fp32-rounded coefficients; the same in float32 (the band as filter_ref.chain_states runs it, the detector with the contract's two fma:
the restatement whose deviation from float64 sets the tests' bounds); and a model of the GPU's decomposition (fp32 chunks of 32 samples,
scans in double, fp32 start values) with the faults a scan can have, the band's scan included.  Nothing here calls the library."""
import numpy as np

import compressor_ref as cr
import filter_ref as fr

CHUNK, WG, SCAN = cr.CHUNK, cr.WG, cr.SCAN
FIELDS = ("freq_hz", "threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "range_db", "mode")
SPEECH = (5500.0, -30.0, 4.0, 6.0, 1.0, 40.0, 12.0, "split")
Q = (np.float32(0.54119610), np.float32(1.30656296))  # 4th-order Butterworth
BAND_STATES, DET_STATES = ("st_end", "st_start"), ("s1_end", "s1_start", "s2_end", "s2_start")
chunks = cr.chunks


def band(c, rate):
    """the section pass [10] float32: the two high-passes designed in double and rounded to fp32"""
    return np.concatenate([fr.design("highpass", c[0], q, 0.0, rate) for q in Q]).astype(np.float32)


def coefs(c, rate):
    """what the GPU computes with (and the float64 reference is given): the detector's fp32 values as compressor_ref.coefs names them
    (mk = 0), the range R, the band's section pass, and whether only the band is turned down"""
    f = cr.coefs(tuple(c[1:6]) + (0.0,), rate)
    return dict(f, R=np.float32(c[6]), band=band(c, rate), split=c[7] in ("split", 0))


def _det(f):
    return {k: f[k] for k in ("T", "S", "K", "kA", "kR", "mk")}


def want(h, f, dt=np.float64):
    """z >= 0: the compressor's gain computer on the band's level (h as it is, in dt), capped at the range"""
    d = {k: dt(f[k]) for k in ("T", "S", "K", "R")}
    hg = dt(20) * np.log10(np.maximum(np.abs(h.astype(dt)), dt(np.float32(1e-6))))
    x = hg - d["T"]
    x2 = dt(2) * x
    t = x + dt(0.5) * d["K"]
    with np.errstate(divide="ignore", invalid="ignore"):
        knee = (-d["S"] * (t * t)) / (dt(2) * d["K"])
    in_knee = (np.abs(x2) <= d["K"]) & (d["K"] > 0)
    z = np.where(x2 < -d["K"], dt(0), np.where(in_knee, knee, -d["S"] * x))
    return np.minimum(d["R"], z).astype(dt)


def apply(x, h, yl, f, dt=np.float64):
    """split: y = fma(-(1 - g), h, x), x itself where g == 1; wide: y = x g"""
    x = np.asarray(x, np.float32).astype(dt)
    g = np.power(dt(10), -yl / dt(20)).astype(dt)
    if not f["split"]:
        return (x * g).astype(dt)
    return np.where(g == 1, x, cr._fma(-(dt(1) - g), h.astype(dt), x, dt)).astype(dt)


class Ref:
    """the contract on x [rows, W] in dt: h, z, y1, yL, y per sample and the band's state at every chunk's start"""

    def __init__(self, x, f, dt=np.float64):
        self.x, self.dt = np.asarray(x, np.float32), dt
        start, _, h = fr.chain_states(self.x, f["band"][None, :], dt)
        self.st_start, self.h = start[0], h
        self.z = want(h, f, dt)
        self.y1, self.yl = cr.detect(self.z, _det(f), dt)
        self.y = apply(self.x, h, self.yl, f, dt)

    def states(self, f, W):
        """st_end, st_start [rows, chunks(W), 4] and s1_end, s1_start, s2_end, s2_start [rows, chunks(W)] of the first W samples"""
        dt, K = self.dt, chunks(W)
        first = np.arange(K) * CHUNK
        zero = np.zeros((self.z.shape[0], 1), dt)
        s1_start = np.concatenate([zero, self.y1[:, first[1:] - 1]], axis=1)
        s2_start = np.concatenate([zero, self.yl[:, first[1:] - 1]], axis=1)
        z = self.z[:, :W]
        s1_end, _, _ = cr.chunk_run(z, _det(f), dt)
        _, s2_end, _ = cr.chunk_run(z, _det(f), dt, y1_start=s1_start)
        st_end = fr.chunk_ends(self.x[:, :W], f["band"], dt)
        return dict(st_end=st_end, st_start=self.st_start[:, :K], s1_end=s1_end, s1_start=s1_start, s2_end=s2_end, s2_start=s2_start)


def model(x, f, fault=None):
    """The GPU's decomposition in numpy: the band's chunks from zero in fp32, their scan in double, h regenerated from the fp32 start
    states; the detector's two stages likewise on z(h) -> dict of h, yl, y and the six state arrays.
    fault: None, "band_carry" (the band's scan drops its carry at every tile), "band_neighbour" (every chunk takes the band state of
    the chunk in front of it), ("carry1" | "carry2", chunk index), "neighbour1" or "neighbour2" (compressor_ref.model's)."""
    dt = np.float32
    x = np.asarray(x, np.float32)
    bf = {"band_carry": "carry", "band_neighbour": "chunk"}.get(fault) if isinstance(fault, str) else None
    start, end, h = fr.decomposed(x, f["band"][None, :], tile=SCAN, fault=bf)
    z = want(h, f, dt)
    d = _det(f)
    D = (1.0 - float(f["kR"])) ** CHUNK
    E = (1.0 - float(f["kA"])) ** CHUNK
    drop = {1: (), 2: ()}
    nb = {1: False, 2: False}
    if isinstance(fault, tuple):
        drop[int(fault[0][-1])] = (fault[1],)
    elif fault and bf is None:
        nb[int(fault[-1])] = True
    s1_end, _, _ = cr.chunk_run(z, d, dt)
    s1_start = cr.scan(s1_end, D, np.maximum, drop[1], nb[1])
    _, s2_end, _ = cr.chunk_run(z, d, dt, y1_start=s1_start)
    s2_start = cr.scan(s2_end, E, np.add, drop[2], nb[2])
    _, _, yl = cr.chunk_run(z, d, dt, y1_start=s1_start, yl_start=s2_start)
    return dict(h=h, yl=yl, y=apply(x, h, yl, f, dt), st_end=end[0], st_start=start[0], s1_end=s1_end, s1_start=s1_start, s2_end=s2_end,
                s2_start=s2_start)
