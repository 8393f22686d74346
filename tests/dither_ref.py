"""The dithered PCM quantizer in numpy (include/stn.h "dither"), as the definition states it and nothing else:
Philox4x32-10 in uint64 arithmetic, the stream's counter and key, the three modes' dither values, the quantizer in float64 and the two
encodings.  The device (tests/test_gpu_dither.py) and the host functions (tests/test_dither_cpu.py) are held to it bit for bit.
`fault` names one deliberate deviation each, for the tests that show the bound catches it."""
import numpy as np

OFF, ROUND, TPDF, TPDF_HP = 0, 1, 2, 3
MODES = {"off": OFF, "round": ROUND, "tpdf": TPDF, "tpdf-hp": TPDF_HP}
ROW, PROG = 0, 1
PCM16, PCM24 = 1, 2  # STN_ENC_*
SCALE = {PCM16: 32767, PCM24: 8388607}
M32 = np.uint64(0xFFFFFFFF)
FAULTS = ("same_block_predecessor", "first_predecessor_zero", "fp32_sum", "id_high_dropped")  # ("gaps_undithered" is quantize_prog's)


def philox4x32_10(c, k):
    """c uint64 [..., 4] (32-bit values), k (k0, k1) -> uint64 [..., 4]: ten rounds of Philox4x32 (Random123)"""
    c = [np.asarray(c[..., i], np.uint64) & M32 for i in range(4)]
    k0, k1 = np.uint64(k[0]) & M32, np.uint64(k[1]) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=-1)


def words(seed, kind, id, n):
    """the 32-bit word of every sample index in n (int64 array) of stream (kind, id) under seed -> uint64 array"""
    n = np.asarray(n, np.int64)
    assert n.size == 0 or (n.min() >= 0 and n.max() < 1 << 34)
    seed, id = int(seed) & (1 << 64) - 1, int(id) & (1 << 64) - 1
    c = np.empty(n.shape + (4,), np.uint64)
    c[..., 0] = (n >> 2).astype(np.uint64)
    c[..., 1], c[..., 2], c[..., 3] = id & 0xFFFFFFFF, id >> 32, 0xD17E0000 | kind
    out = philox4x32_10(c, (seed & 0xFFFFFFFF, seed >> 32))
    return np.take_along_axis(out, (n & 3).astype(np.int64)[..., None], axis=-1)[..., 0]


def noise(mode, seed, kind, id, n0, n, fault=None):
    """the dither d of samples n0 .. n0 + n in LSB, float64 (exact: multiples of 2^-16 below 1 in magnitude)"""
    idx = n0 + np.arange(n, dtype=np.int64)
    if mode in (OFF, ROUND) or n == 0:
        return np.zeros(n)
    if fault == "id_high_dropped":
        id = int(id) & 0xFFFFFFFF
    w = words(seed, kind, id, idx)
    a, b = (w & np.uint64(0xFFFF)).astype(np.int64), (w >> np.uint64(16)).astype(np.int64)
    if mode == TPDF:
        return (a - b) / 65536.0
    pw = words(seed, kind, id, np.maximum(idx - 1, 0))  # the predecessor's word: for n % 4 == 0 it lies in the previous block
    prev = (pw & np.uint64(0xFFFF)).astype(np.int64)
    if fault == "same_block_predecessor":  # the word in front of a block's first taken from the same block (its last)
        wrong = words(seed, kind, id, idx | 3)
        prev = np.where(idx % 4 == 0, (wrong & np.uint64(0xFFFF)).astype(np.int64), prev)
    prev = np.where(idx == 0, 0 if fault == "first_predecessor_zero" else b, prev)  # a_{-1} := b_0
    return (a - prev) / 65536.0


def quantize(enc, mode, v, d, fault=None):
    """the codes (int64) of fp32 samples v under dither d (float64, LSB).  OFF: the truncating store."""
    S = SCALE[enc]
    vc = np.minimum(np.float32(1), np.maximum(np.float32(-1), np.asarray(v, np.float32)))
    if mode == OFF:
        return (vc * np.float32(S)).astype(np.int64)  # fp32 product, toward zero
    if fault == "fp32_sum":
        t = vc * np.float32(S) + np.float32(0.5) + d.astype(np.float32)
    else:
        t = vc.astype(np.float64) * float(S) + 0.5 + d
    return np.clip(np.floor(t).astype(np.int64), -S, S)


def pack(enc, q):
    """codes -> int16 [...] or little-endian uint8 [..., 3]"""
    q = np.asarray(q, np.int64)
    if enc == PCM16:
        return q.astype(np.int16)
    u = (q & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=-1).astype(np.uint8)


def quantize_stream(enc, mode, seed, kind, id, v, n0=0, length=None, fault=None):
    """one row: v[i] is sample n0 + i of stream (kind, id); samples at and behind `length` (None: none) are the zero codeword -> codes"""
    v = np.asarray(v, np.float32)
    q = quantize(enc, mode, v, noise(mode, seed, kind, id, n0, v.size, fault), fault)
    if length is not None and mode != OFF:
        q[max(0, int(length) - n0):] = 0
    return q


def quantize_rows(enc, mode, seed, kind, ids, v, lengths=None, fault=None):
    """rows v [R, W] fp32, row r the stream (kind, ids[r]) from sample 0 -> packed samples [R, W] (int16) or [R, W, 3] (uint8)"""
    v = np.atleast_2d(np.asarray(v, np.float32))
    return pack(enc, np.stack([quantize_stream(enc, mode, seed, kind, ids[r], v[r], 0, None if lengths is None else lengths[r], fault)
                               for r in range(v.shape[0])]))


def quantize_prog(enc, mode, seed, g, v, length, members, fault=None):
    """one joined programme row v (fp32) of index g with the members' (start, end) spans; fault "gaps_undithered": only the members'
    samples draw dither, the gaps are quantized without -> packed"""
    q = quantize_stream(enc, mode, seed, PROG, g, v, 0, length, None if fault == "gaps_undithered" else fault)
    if fault == "gaps_undithered":
        inside = np.zeros(len(v), bool)
        for s, e in members:
            inside[s:e] = True
        q = np.where(inside, q, quantize(enc, ROUND if mode != OFF else OFF, v, np.zeros(len(v))))
    return pack(enc, q)
