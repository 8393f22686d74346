"""numpy restatements of the tables csrc/host/len_tables.cpp builds, written from what the kernels they replace are documented to write
(row_map_kernel, hs_pairs_kernel, trim_len_kernel, scale_len_kernel) — shared by tests/test_len_tables_cpu.py and tests/test_gpu_len_tables.py."""
import numpy as np


def bucket_up(n, q):
    return (n + q - 1) // q * q


def row_map(llen, rows_padded):
    llen = np.asarray(llen, np.int64)
    off = np.concatenate([[0], np.cumsum(llen)]).astype(np.int32)
    row_b = np.zeros(max(int(off[-1]), rows_padded), np.int32)  # dead rows behind the last utterance: sequence 0
    row_b[:off[-1]] = np.repeat(np.arange(len(llen), dtype=np.int32), llen)
    return off, row_b[:rows_padded] if rows_padded else row_b


def hs_pairs(llen):
    """ascending rank with index tie-break; the k-th longest with the k-th shortest; -1 for the odd one out; B + 2 words, the rest 0"""
    B = len(llen)
    order = sorted(range(B), key=lambda i: (int(llen[i]), i))
    out = np.zeros(B + 2, np.int32)
    for i in range((B + 1) // 2):
        out[2 * i] = order[B - 1 - i]
        out[2 * i + 1] = order[i] if B - 1 - i > i else -1
    return out


def vo_extents(llen, form, ccf, T, rf):
    """form 1: the 2rf trim (n = l6 + 2rf, valid = l6 + rf where l6 + 2rf <= T, else both T); 2: the tail form (both min(l6 + rf, T));
    3: lengths scaled by ccf"""
    l6 = np.asarray(llen, np.int64) * ccf
    if form == 3:
        n = valid = l6
    elif form == 2:
        n = valid = np.minimum(l6 + rf, T)
    else:
        trim = l6 + 2 * rf <= T
        n = np.where(trim, l6 + 2 * rf, T)
        valid = np.where(trim, l6 + rf, T)
    off = np.concatenate([[0], np.cumsum(n)])
    return n.astype(np.int32), valid.astype(np.int32), off.astype(np.int32)


def cases():
    """(name, llen): all lengths equal (every tie), strictly descending, one length of 1, odd B, B in {1, 2, 3, 128, 1024}"""
    rng = np.random.default_rng(5)
    out = []
    for B in (1, 2, 3, 128, 1024):
        out.append((f"equal B{B}", np.full(B, 57, np.int32)))
        out.append((f"descending B{B}", (np.arange(B, 0, -1) + 3).astype(np.int32)))
        r = rng.integers(20, 79, B).astype(np.int32)
        r[B // 2] = 1
        out.append((f"random with a 1 B{B}", r))
        t = rng.integers(40, 44, B).astype(np.int32)  # many ties
        out.append((f"ties B{B}", t))
    out.append(("odd B 5", np.array([9, 3, 9, 1, 7], np.int32)))
    return out
