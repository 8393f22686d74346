"""The layout kernels between the GEMMs (csrc/kernels_layout.hip: row_map_kernel, ncl_to_rows_kernel, euler_ncl_kernel<ZT>, unpack_rows_kernel,
embed_kernel, masked_mean_kernel, vocoder_im2col_kernel<OutT, FIXED>, vocoder_in_kernel), one at a time through stn_op_layout, against numpy
statements of what each does.  Most only move or round data and are compared bit for bit; every destination is a buffer full of NaN (or -7)
sentinels that comes back whole, so a row or column a kernel must not touch is seen; sources carry NaN where a kernel must not read.

Not exact, with the reason for each bound:
  * euler_ncl: with r = prev + dt * v in float64, |got - r| <= 0.5 ulp32(r) + 0.5 ulp32(dt * v): one rounding of the sum, and one of the
    product unless the compiler contracts the multiply-add.
  * masked_mean: |got - mean64| <= (len + 1) 2^-24 mean|x|: the kernel adds len terms serially in fp32, each addition rounds a partial sum
    of at most len mean|x| by 2^-24 relative, the division by len brings that to len 2^-24 mean|x| and rounds once more.  len = 0 gives 0.
  * vocoder_in (fp32 fmaf chain of ld * k terms) against float64: max |d| <= VI_REL rms(ref).  Measured 1.8e-6 (ld = 24, k = 7: 168 terms; 5.5e-7 at 40 terms); bound 6e-6
    (under 4x the measurement).  The same bound ties it to the fp32 im2col times the same weights in float64.

Wall time on an MI355X: 1 s (52 tests)."""
import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.binding import (LAYOUT_EMBED, LAYOUT_EULER_NCL, LAYOUT_IM2COL, LAYOUT_MASKED_MEAN, LAYOUT_NCL_TO_ROWS, LAYOUT_ROW_MAP,
                                    LAYOUT_UNPACK_ROWS, LAYOUT_VOCODER_IN)

pytestmark = pytest.mark.gpu

SENTINEL_BITS = 0x7FC00000  # the canonical quiet NaN: survives the round trip through bf16 / half bit for bit
SENTINEL = np.array([SENTINEL_BITS], np.uint32).view(np.float32)[0]
FMTS = ("f32", "bf16", "f16")
VI_REL = 6e-6
STATS = {}


@pytest.fixture(scope="module")
def eng():
    return binding.Engine(0, "bf16")


def rnd(x, fmt):
    """round-to-nearest-even to the format, as float32"""
    x = np.ascontiguousarray(x, np.float32)
    if fmt == "bf16":
        u = x.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
        return u.astype(np.uint32).view(np.float32)
    if fmt == "f16":
        return x.astype(np.float16).astype(np.float32)
    return x


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def sent(*shape):
    return np.full(shape, SENTINEL, np.float32)


def ulp32(x):
    return np.exp2(np.maximum(np.floor(np.log2(np.maximum(np.abs(x), 1e-300))), -126) - 23)


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ---- row_map --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 2, 127, 1023, 1024))
def test_row_map(eng, B):
    rng = np.random.default_rng(B)
    lens = rng.integers(0, 6, B).astype(np.int32)
    lens[rng.integers(0, B, max(B // 4, 1))] = 0
    if B == 2:
        lens[:] = (0, 3)
    tot = int(lens.sum())
    off = offsets(lens)
    for rows_padded in (0, tot + 37):
        n = max(tot, rows_padded)
        io = eng.op_layout(LAYOUT_ROW_MAP, [B, rows_padded, 1], length=lens, iout=np.full(B + 1 + n + 5, -7, np.int32))[2]
        assert np.array_equal(io[:B + 1], off)
        assert np.array_equal(io[B + 1:B + 1 + tot], np.repeat(np.arange(B), lens))
        assert np.all(io[B + 1 + tot:B + 1 + n] == 0)  # dead rows map to sequence 0
        assert np.all(io[B + 1 + n:] == -7)
    io = eng.op_layout(LAYOUT_ROW_MAP, [B, 0, 0], length=lens, iout=np.full(B + 1 + 5, -7, np.int32))[2]  # row_b = NULL
    assert np.array_equal(io[:B + 1], off) and np.all(io[B + 1:] == -7)


def test_row_map_refuses_more_than_1024_sequences(eng):
    with pytest.raises(binding.StnError) as ei:
        eng.op_layout(LAYOUT_ROW_MAP, [1025, 0, 0], length=np.ones(1025, np.int32), iout=np.full(1026, -7, np.int32))
    assert ei.value.code == -1


# ---- ncl_to_rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("ldo", (37, 64))
def test_ncl_to_rows(eng, fmt, ldo):
    B, C, L = 3, 37, 45
    rng = np.random.default_rng(ldo)
    x = rng.standard_normal((B, C, L)).astype(np.float32)
    rows = np.zeros((B, L, ldo), np.float32)
    rows[:, :, :C] = rnd(x, fmt).transpose(0, 2, 1)
    out = eng.op_layout(LAYOUT_NCL_TO_ROWS, [B, C, L, ldo], a=x, out=sent(B * L + 2, ldo), dtype=fmt)[0]
    assert same(out[:B * L], rows.reshape(B * L, ldo)) and np.all(bits(out[B * L:]) == SENTINEL_BITS)
    lens = np.array([45, 0, 17], np.int32)
    out = eng.op_layout(LAYOUT_NCL_TO_ROWS, [B, C, L, ldo], a=x, length=lens, packed=True, out=sent(int(lens.sum()) + 2, ldo), dtype=fmt)[0]
    assert same(out[:62], np.concatenate([rows[0], rows[2, :17]])) and np.all(bits(out[62:]) == SENTINEL_BITS)


# ---- euler_ncl --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zfmt", (None,) + FMTS)
@pytest.mark.parametrize("packed", (False, True), ids=("padded", "packed"))
@pytest.mark.parametrize("ldz", (37, 64))
def test_euler_ncl(eng, zfmt, packed, ldz):
    B, D, L = 3, 37, 45
    rng = np.random.default_rng(ldz + packed)
    for lens in (None, np.array([0, 1, 45], np.int32), np.array([45, 20, 33], np.int32)):
        if packed and lens is None:
            continue  # (packed rows need lengths)
        n = np.full(B, L) if lens is None else lens
        prev = rng.standard_normal((B, D, L)).astype(np.float32)
        v = rng.standard_normal((B, L, D)).astype(np.float32)
        dt = np.array([0.2, 1.0 / 3.0, 0.125], np.float32)
        valid = np.arange(L)[None, :] < n[:, None]
        if packed:
            vin = np.concatenate([v[b, :n[b]] for b in range(B)] + [sent(3, D)])  # rows beyond the packed total: NaN
            zrows = int(n.sum())
        else:
            vin = v.copy()
            vin[~valid] = np.nan  # velocity rows beyond a sequence's own: NaN, and they change nothing
            vin = vin.reshape(B * L, D)
            zrows = B * L
        out, z, _ = eng.op_layout(LAYOUT_EULER_NCL, [B, D, L, int(zfmt is not None), ldz], a=prev, b=vin, c=dt, length=lens, packed=packed,
                                  out=sent(B * D * L + 5), out2=None if zfmt is None else sent(zrows + 2, ldz), dtype=zfmt or "f32")
        assert np.all(bits(out[B * D * L:]) == SENTINEL_BITS)
        out = out[:B * D * L].reshape(B, D, L)
        vm = valid[:, None, :] & np.ones((1, D, 1), bool)
        assert np.all(bits(out)[~vm] == 0), "frames at t >= len[b] must be exactly +0"
        prod = dt.astype(np.float64)[:, None, None] * v.transpose(0, 2, 1).astype(np.float64)
        r = prev.astype(np.float64) + prod
        assert np.all((np.abs(out - r) <= 0.5 * ulp32(r) + 0.5 * ulp32(prod))[vm])
        if zfmt is None:
            continue
        # the z rows are the rounding of the RETURNED latent, bit for bit: what ncl_to_rows makes of it, asserted through that entry too
        want = rnd(out, zfmt).transpose(0, 2, 1)  # [B, L, D]
        via = eng.op_layout(LAYOUT_NCL_TO_ROWS, [B, D, L, ldz], a=out, length=lens, packed=packed, out=sent(zrows + 2, ldz), dtype=zfmt)[0]
        zw = np.concatenate([want[b, :n[b]] for b in range(B)]) if packed else want.reshape(B * L, D)
        assert same(z[:zrows, :D], zw) and same(via[:zrows, :D], zw)
        assert np.all(bits(z[:zrows, D:]) == SENTINEL_BITS) and np.all(bits(z[zrows:]) == SENTINEL_BITS)


# ---- unpack_rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (4, 512))
def test_unpack_rows(eng, W):
    B, T = 3, 9
    lens = np.array([9, 0, 4], np.int32)
    rng = np.random.default_rng(W)
    src = rng.standard_normal((13, W)).astype(np.float32)
    out = eng.op_layout(LAYOUT_UNPACK_ROWS, [B, T, W], a=np.concatenate([src, sent(2, W)]), length=lens, out=sent(B * T * W + 8))[0]
    want = np.zeros((B, T, W), np.float32)
    want[0], want[2, :4] = src[:9], src[9:]
    assert same(out[:B * T * W], want.reshape(-1)) and np.all(bits(out[B * T * W:]) == SENTINEL_BITS)


# ---- embed --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", (False, True), ids=("padded", "packed"))
def test_embed(eng, packed):
    vocab, B, L, C = 11, 3, 7, 8
    rng = np.random.default_rng(3)
    table = rng.standard_normal((vocab, C)).astype(np.float32)
    ids = rng.integers(0, vocab, (B, L)).astype(np.int64)
    ids[0, 1], ids[0, 2], ids[0, 3], ids[2, 0], ids[2, 1] = -1, vocab, vocab + 5, 10, 0
    lens = np.array([7, 0, 3], np.int32)
    want = np.zeros((B, L, C), np.float32)
    for b in range(B):
        for t in range(lens[b]):
            if 0 <= ids[b, t] < vocab:
                want[b, t] = table[ids[b, t]]
    rows = int(lens.sum()) if packed else B * L
    out = eng.op_layout(LAYOUT_EMBED, [vocab, B, L, C], a=table, ids=ids, length=lens, packed=packed, out=sent(rows + 2, C))[0]
    assert same(out[:rows], np.concatenate([want[b, :lens[b]] for b in range(B)]) if packed else want.reshape(B * L, C))
    assert np.all(bits(out[rows:]) == SENTINEL_BITS)


# ---- masked_mean ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("packed", (False, True), ids=("padded", "packed"))
def test_masked_mean(eng, fmt, packed):
    B, L, C = 4, 50, 20
    lens = np.array([50, 0, 1, 33], np.int32)
    rng = np.random.default_rng(9)
    x = rnd(rng.standard_normal((B, L, C)) + 0.25, fmt)
    valid = np.arange(L)[None, :] < lens[:, None]
    if packed:
        xin = np.concatenate([x[b, :lens[b]] for b in range(B)] + [sent(2, C)])
    else:
        xin = x.copy()
        xin[~valid] = np.nan  # never read
        xin = xin.reshape(B * L, C)
    out = eng.op_layout(LAYOUT_MASKED_MEAN, [B, L, C], a=xin, length=lens, packed=packed, out=sent(B * C + 3), dtype=fmt)[0]
    assert np.all(bits(out[B * C:]) == SENTINEL_BITS)
    out = out[:B * C].reshape(B, C)
    for b in range(B):
        if lens[b] == 0:
            assert np.all(bits(out[b]) == 0)  # 0 / max(len, 1)
            continue
        xs = x[b, :lens[b]].astype(np.float64)
        assert np.all(np.abs(out[b] - xs.mean(axis=0)) <= (lens[b] + 1) * 2.0 ** -24 * np.abs(xs).mean(axis=0))


# ---- the vocoder fronts -----------------------------------------------------------------------------------------------------------------
def frames_of(latent, ld, ccf):
    """[B, ld*ccf, L] -> vocoder frames [B, T = L*ccf, ld]: frame l*ccf + q, channel c <- latent[b, q*ld + c, l]"""
    B, D, L = latent.shape
    return latent.reshape(B, ccf, ld, L).transpose(0, 3, 1, 2).reshape(B, L * ccf, ld)


def im2col_ref(latent, ld, ccf, k, kp, n):
    fr = frames_of(latent, ld, ccf)
    B, T, _ = fr.shape
    half = (k - 1) // 2
    cols = np.zeros((B, T, kp), np.float32)
    for b in range(B):
        for j in range(k):
            for t in range(T):
                tt = t + j - half
                if 0 <= tt < n[b]:
                    cols[b, t, j:ld * k:k] = fr[b, tt]
    return cols


IM2COL_SHAPES = {"fixed": (24, 6, 7, 192, 7), "generic_small": (8, 3, 5, 48, 15), "fixed_kp200": (24, 6, 7, 200, 7)}  # ld, ccf, k, kp, L


def run_im2col(eng, fmt, latent, ld, ccf, k, kp, lens, packed):
    B, _, L = latent.shape
    T = L * ccf
    rows = int(np.sum(lens)) if packed else B * T
    out = eng.op_layout(LAYOUT_IM2COL, [B, L, ld, ccf, k, kp], a=latent, length=lens, packed=packed, out=sent(rows + 2, kp), dtype=fmt)[0]
    assert np.all(bits(out[rows:]) == SENTINEL_BITS)
    return out[:rows]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", sorted(IM2COL_SHAPES))
def test_vocoder_im2col(eng, fmt, name):
    ld, ccf, k, kp, L = IM2COL_SHAPES[name]
    B, T = 3, L * ccf
    assert T % 32
    rng = np.random.default_rng(ld + kp)
    latent = rng.standard_normal((B, ld * ccf, L)).astype(np.float32)
    for lens in (None, np.array([T, 1, T // 2 - 1], np.int32), np.array([2, T, 0], np.int32)):
        n = np.full(B, T) if lens is None else lens
        want = rnd(im2col_ref(latent, ld, ccf, k, kp, n), fmt)
        assert np.all(want[:, :, ld * k:] == 0)
        got = run_im2col(eng, fmt, latent, ld, ccf, k, kp, lens, False)
        assert same(got, want.reshape(B * T, kp)), (name, fmt, lens)
        if lens is not None:
            got_p = run_im2col(eng, fmt, latent, ld, ccf, k, kp, lens, True)
            assert same(got_p, np.concatenate([want[b, :n[b]] for b in range(B)])), (name, fmt, lens, "packed")
        if name == "fixed_kp200":  # the generic template on the FIXED numbers: the compile-time form's 192 columns
            assert same(run_im2col(eng, fmt, latent, ld, ccf, k, 192, lens, False), got[:, :192])


def test_vocoder_im2col_long(eng):
    """several 32-frame tiles per sequence: tiles that start inside the first `half` frames, inside the sequence and end at T"""
    ld, ccf, k, kp = 24, 6, 7, 192
    B, L = 2, 17  # T = 102: tiles at 0, 32, 64, 96 (the last of 6 frames)
    latent = np.random.default_rng(1).standard_normal((B, ld * ccf, L)).astype(np.float32)
    for fmt in FMTS:
        for lens in (None, np.array([102, 65], np.int32), np.array([33, 96], np.int32)):
            n = np.full(B, 102) if lens is None else lens
            want = rnd(im2col_ref(latent, ld, ccf, k, kp, n), fmt)
            assert same(run_im2col(eng, fmt, latent, ld, ccf, k, kp, lens, False), want.reshape(-1, kp))
            if lens is not None:
                assert same(run_im2col(eng, fmt, latent, ld, ccf, k, kp, lens, True), np.concatenate([want[b, :n[b]] for b in range(B)]))


@pytest.mark.parametrize("shape", [(8, 3, 5, 20, 5), (24, 6, 7, 64, 3)], ids=str)
def test_vocoder_in(eng, shape):
    ld, ccf, k, C, L = shape
    B, T = 2, L * ccf
    assert T % 8
    rng = np.random.default_rng(C)
    latent = rng.standard_normal((B, ld * ccf, L)).astype(np.float32)
    w_t = (rng.standard_normal((ld * k, C)) / np.sqrt(ld * k)).astype(np.float32)  # [(ci, j), co]
    bias = (rng.standard_normal(C) * 0.3).astype(np.float32)
    for lens in (None, np.array([T, T // 2], np.int32)):
        n = np.full(B, T) if lens is None else lens
        got = eng.op_layout(LAYOUT_VOCODER_IN, [B, L, ld, ccf, C, k], a=latent, b=w_t, c=bias, length=lens, out=sent(B * T + 2, C))[0]
        assert np.all(bits(got[B * T:]) == SENTINEL_BITS)
        got = got[:B * T].astype(np.float64)
        ref = im2col_ref(latent, ld, ccf, k, ld * k, n).reshape(B * T, ld * k).astype(np.float64) @ w_t.astype(np.float64) + bias.astype(np.float64)
        rms = np.sqrt(np.mean(ref ** 2))
        rel = float(np.abs(got - ref).max() / rms)
        # the other front on the same data: the fp32 im2col (exact) times the same weights
        cols = run_im2col(eng, "f32", latent, ld, ccf, k, ld * k, lens, False).astype(np.float64)
        rel2 = float(np.abs(got - (cols @ w_t.astype(np.float64) + bias.astype(np.float64))).max() / rms)
        STATS[str(shape)] = max(STATS.get(str(shape), 0.0), rel, rel2)
        print(f"vocoder_in {shape} lens {None if lens is None else lens.tolist()}: max|d|/rms = {rel:.3e} (float64), {rel2:.3e} (im2col x W)")
        assert rel <= VI_REL and rel2 <= VI_REL, (shape, rel, rel2)


def test_entry_refuses_buffers_that_are_too_small(eng):
    x = np.zeros((2, 5, 7), np.float32)
    with pytest.raises(binding.StnError):
        eng.op_layout(LAYOUT_NCL_TO_ROWS, [2, 5, 7, 5], a=x, out=sent(13, 5))
    with pytest.raises(binding.StnError):
        eng.op_layout(LAYOUT_NCL_TO_ROWS, [2, 5, 7, 5], a=x, packed=True, out=sent(14, 5))  # packed without lengths
    with pytest.raises(binding.StnError):
        eng.op_layout(LAYOUT_UNPACK_ROWS, [2, 3, 4], a=np.zeros((3, 4), np.float32), length=np.array([3, 4], np.int32), out=sent(24))


def test_zz_report_measured():
    """not a check: prints the largest deviations seen in this session (run with -s)"""
    for kname, v in sorted(STATS.items()):
        print(f"vocoder_in {kname}: max|d|/rms = {v:.3e} (bound {VI_REL:.1e})")
