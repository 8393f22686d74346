"""The shapes and inputs the dither tests share: tests/test_gpu_dither.py runs them on the GPU, tests/test_dither_cpu.py shows on the same
shapes that every fault it names breaks the bit-exact comparison."""
import numpy as np

import dither_ref as dr

SEED = 0x9E3779B97F4A7C15  # (a non-zero high word: the key's second half)
IDS = np.array([0, 7, (1 << 32) + 5], np.int64)  # row ids of the op-level test: the last has a high word
WS = (1, 3, 4, 5, 8, 9, 15, 16, 17, 33, 48, 1040)
GAIN = np.array([1.0, 0.5, 1.75], np.float32)
VEC = {dr.PCM16: 8, dr.PCM24: 16}  # samples per thread of the store's vector form
GAP = 100  # samples of silence between the members of the joined fetch


def inputs(enc, W):
    """float32 [3, W]: by (column + row) % 4 a ramp through +-1.25 (the clamp), an exact zero, a tie +-(k + 0.5) / S, and a value under
    one LSB; every row holds every kind as soon as W >= 4, and the three rows differ at every column"""
    S = dr.SCALE[enc]
    j = np.arange(W)
    rows = []
    for r in range(3):
        kind = (j + r) % 4
        ramp = -1.25 + 2.5 * ((j * 37 + r * 11) % 101) / 100.0
        tie = np.where(j % 2 == 0, 1.0, -1.0) * (((7 * j + r) % 50) + 0.5) / S
        sub = (((j + 2 * r) % 9) - 4) / 10.0 / S
        rows.append(np.select([kind == 0, kind == 1, kind == 2], [ramp, 0.0, tie], sub))
    return np.asarray(rows, np.float64).astype(np.float32)


def vector_form(enc, W, stride, misalign):
    """whether launch_store_rows takes the vector form (the buffers themselves are 16-byte aligned)"""
    V = VEC[enc]
    return misalign == 0 and W % V == 0 and stride % V == 0
