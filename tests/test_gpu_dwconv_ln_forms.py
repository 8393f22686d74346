"""Every form of the depthwise-conv + LayerNorm family (csrc/kernels_dwconv_ln.hip: dwconv_ln_v3_kernel<OutT, K, R> for (K, R) in {(5,2), (5,4),
(5,8), (7,4)}, dwconv_ln_v3_occ4_kernel, dwconv_ln_v2_kernel<OutT, K, 2>, dwconv_ln_kernel<OutT, true / false>; csrc/kernels_fold.hip: fold_ln_kernel<OutT, F16, RV,
S>) against float64, through stn_op_dwconv_ln_ex and stn_op_fold_ln.  Each case first asserts the form it expects (binding.dwconv_ln_form
pins the same strings without a GPU in tests/test_dwconv_ln_form_cpu.py), then the values.  The reference is plain numpy in float64:
zero-padded dilated depthwise convolution inside each sequence (taps at t >= seqlen[b] read zero), bias, LayerNorm with eps = 1e-6 over
C, gain and shift.  All weights are random, so a mirrored tap order or a wrong channel map cannot pass.

Bounds ("measured" = the largest value over every case of this file on an MI355X, printed by test_zz_report_measured):
  * fp32 outputs (and fold_ln's updated residual): max |got - ref| <= F32_REL rms(ref): fp32 sums in another order than float64.
    Measured 1.7e-6 (v2<5>; every form and fold_ln between 0.5e-6 and 1.7e-6); bound 6e-6 (under 4x the measurement, and under the 2e-5
    tests/test_gpu_ops.py asserts).
  * 16-bit outputs: the only 16-bit rounding is the store: |got - ref| <= 0.5 ulp_fmt(ref) + F32_REL rms(ref), every element.
  * Exact (bits): rows at t >= seqlen[b] of a padded batch are +0.0 in every form — the sign IS pinned: the v2 and generic kernels
    used to write `0 * value`, i.e. -0.0 for a negative value and NaN for a NaN one, and are now selects; NaN in every input row at
    t >= seqlen[b] changes no bit of any output (the v2 / v3 kernels used to multiply the clamped padding load by 0, which let 0 * NaN
    into the valid rows next to a sequence's end: fixed by selects); rows outside the launch keep their NaN sentinels; packed against
    padded of the same form; a sequence's bits across batch positions and neighbours.

Wall time on an MI355X: 6 s (122 tests)."""
import numpy as np
import pytest

from supertonic_amd import binding

pytestmark = pytest.mark.gpu

SENTINEL_BITS = 0x7FC00000  # the canonical quiet NaN: survives the round trip through bf16 / half bit for bit
SENTINEL = np.array([SENTINEL_BITS], np.uint32).view(np.float32)[0]
F32_REL = 6e-6
FMTS = ("f32", "bf16", "f16")
DILS = (1, 2, 4, 8)
EPS = 1e-6
STATS = {}


@pytest.fixture(scope="module")
def eng():
    return binding.Engine(0, "bf16")


def ulp(x, fmt):
    e = np.floor(np.log2(np.maximum(np.abs(x), 1e-300)))
    if fmt == "bf16":
        return np.exp2(np.maximum(e, -126) - 7)
    return np.exp2(np.maximum(e, -14) - 10)


def rnd(x, fmt):
    if fmt == "bf16":
        u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
        return u.astype(np.uint32).view(np.float32)
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def layernorm64(h, g, bt):
    mean = h.mean(axis=-1, keepdims=True)
    var = ((h - mean) ** 2).mean(axis=-1, keepdims=True)
    return (h - mean) / np.sqrt(var + EPS) * g + bt


def ref64(x, w, bias, g, bt, dil, lens):
    """x [B, L, C]; w [C, k]; lens [B].  Rows at t >= lens[b] come back as zeros."""
    B, L, C = x.shape
    k = w.shape[1]
    half = (k - 1) // 2
    mask = np.arange(L)[None, :] < np.asarray(lens)[:, None]
    xz = np.where(mask[:, :, None], x.astype(np.float64), 0.0)
    h = np.broadcast_to(bias.astype(np.float64), (B, L, C)).copy()
    for j in range(k):
        s = (j - half) * dil
        if abs(s) >= L:
            continue
        wj = w[:, j].astype(np.float64)
        if s >= 0:
            h[:, :L - s] += wj * xz[:, s:]
        else:
            h[:, -s:] += wj * xz[:, :L + s]
    y = layernorm64(h, g.astype(np.float64), bt.astype(np.float64))
    return np.where(mask[:, :, None], y, 0.0)


def check_vals(got, ref, fmt, form, what):
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), what
    if ref.size == 0:
        return
    rms = np.sqrt(np.mean(ref ** 2)) + 1e-30
    d = np.abs(got - ref)
    if fmt == "f32":
        rel = float(d.max() / rms)
        STATS[(form, fmt)] = max(STATS.get((form, fmt), 0.0), rel)
        print(f"{what}: max|d|/rms = {rel:.3e}")
        assert rel <= F32_REL, (what, rel)
        return
    need = float(np.max((d - 0.5 * ulp(ref, fmt)) / rms))  # the share of rms(ref) that half an ulp at |ref| leaves to cover
    STATS[(form, fmt)] = max(STATS.get((form, fmt), 0.0), need)
    print(f"{what}: max(|d| - ulp/2)/rms = {need:.3e}")
    assert need <= F32_REL, (what, need)


class Params:
    def __init__(self, C, k, seed):
        rng = np.random.default_rng(seed)
        self.C, self.k = C, k
        self.w = (rng.standard_normal((C, k)) * 0.5).astype(np.float32)
        self.bias = (rng.standard_normal(C) * 0.3).astype(np.float32)
        self.g = (1.0 + 0.3 * rng.standard_normal(C)).astype(np.float32)
        self.bt = (rng.standard_normal(C) * 0.3).astype(np.float32)


def expect_form(fmt, B, L, C, k, packed):
    """the form by the rules the issue states, written out independently of the library"""
    if C > 512 or k not in (5, 7):
        return "generic"
    M = B * L
    if M < 4096 and not packed:
        return f"v2<{k}>"
    if k == 7:
        return "v3<7,4>" if fmt == "f16" else "v3occ4<7,4>"
    if M >= 32768:
        return "v3<5,8>"
    if M >= 16384:
        return "v3<5,4>"
    if M >= 4096:
        return "v3<5,2>"
    return "v3<5,2>" if M < 1024 else "v3<5,4>"


def run(eng, fmt, x, p, dil, lens=None, packed=False, tail=3):
    """x [B, L, C] padded.  Returns (out [B, L, C] with the rows a packed run does not have as zeros, form).  Asserts the sentinels."""
    B, L, C = x.shape
    n = [L] * B if lens is None else [int(v) for v in lens]
    if packed:
        xin = np.concatenate([x[b, :n[b]] for b in range(B)] + [np.zeros((0, C), np.float32)]).reshape(-1, C)
        rows = xin.shape[0]
        xin = np.concatenate([xin, np.full((tail, C), SENTINEL, np.float32)])
    else:
        xin = x.reshape(B * L, C)
        rows = B * L
    buf = np.full((rows + tail, C), SENTINEL, np.float32)
    out, form = eng.op_dwconv_ln_ex(xin, p.w, p.bias, p.g, p.bt, dil, buf, B, L, seqlen=None if lens is None else np.asarray(lens, np.int32),
                                    packed=packed, dtype=fmt)
    assert np.all(bits(out[rows:]) == SENTINEL_BITS), "rows past the launch were written"
    if not packed:
        return out[:rows].reshape(B, L, C), form
    full = np.zeros((B, L, C), np.float32)
    r = 0
    for b in range(B):
        full[b, :n[b]] = out[r:r + n[b]]
        r += n[b]
    return full, form


def check_run(eng, fmt, x, p, dil, lens=None, packed=False, what=""):
    B, L, C = x.shape
    exp = expect_form(fmt, B, L, C, p.k, packed)
    assert binding.dwconv_ln_form(fmt, B, L, C, p.k, packed) == exp, what
    out, form = run(eng, fmt, x, p, dil, lens, packed)
    assert form == exp, (what, form, exp)
    n = np.full(B, L) if lens is None else np.asarray(lens)
    ref = ref64(x, p.w, p.bias, p.g, p.bt, dil, n)
    mask = np.arange(L)[None, :] < n[:, None]
    assert np.all(bits(out)[~mask] == 0), (what, "rows past a sequence's end must be +0.0")
    check_vals(out[mask], ref[mask], fmt, form, f"{what} {form} {fmt} B{B} L{L} C{C} k{p.k} dil{dil}{' packed' if packed else ''}")
    return out, form


# ---- every form just past its threshold ----------------------------------------------------------------------------------------------
# (rows, B, C, k, packed): L = rows / B is odd, so never a multiple of R * dil for dil in {2, 4, 8}; for dil = 1 it is checked below
THRESH = [
    (4100, 4, 100, 5, False),    # v3<5,2>
    (16388, 4, 64, 5, False),    # v3<5,4>
    (32772, 4, 100, 5, False),   # v3<5,8>
    (4100, 4, 388, 7, False),    # v3occ4<7,4> / v3<7,4>
    (4092, 4, 512, 5, False),    # v2<5>: the last row count below the threshold
    (4092, 4, 388, 7, False),    # v2<7>
    (1023, 1, 384, 5, True),     # packed: v3<5,2>
    (1025, 1, 384, 5, True),     # packed: v3<5,4>
    (1025, 1, 512, 7, True),     # packed: v3 7,4
    (4100, 4, 516, 5, False),    # generic (width)
    (4100, 4, 64, 9, False),     # generic (taps)
]


@pytest.mark.parametrize("case", THRESH, ids=lambda c: "M%d_B%d_C%d_k%d_%s" % (c[0], c[1], c[2], c[3], "packed" if c[4] else "padded"))
def test_forms_past_their_thresholds(eng, case):
    M, B, C, k, packed = case
    L = M // B
    rng = np.random.default_rng(M + C + k)
    x = rng.standard_normal((B, L, C)).astype(np.float32)
    p = Params(C, k, 7)
    lens = np.full(B, L, np.int32) if packed else None
    for dil in DILS:
        for R in (2, 4, 8):
            assert L % (R * dil), (L, R, dil)
        for fmt in FMTS:
            check_run(eng, fmt, x, p, dil, lens, packed, "threshold")


# ---- edges of one sequence ---------------------------------------------------------------------------------------------------------------
def edge_lengths(k, dil, R):
    reach = (k - 1) // 2 * dil
    return sorted({v for v in (1, dil - 1, dil, R * dil - 1, R * dil + 1, reach - 1, reach + 1) if v >= 1})


@pytest.mark.parametrize("k,dil", [(5, 1), (5, 4), (7, 2), (7, 8), (3, 4)])
@pytest.mark.parametrize("fmt", FMTS)
def test_sequence_edges(eng, fmt, k, dil):
    C = 8
    p = Params(C, k, 11)
    rng = np.random.default_rng(k * 100 + dil)
    for R in ((2, 4, 8) if k == 5 else (4,)):
        for L in edge_lengths(k, dil, R):
            # one sequence alone: v2 / generic padded, v3 packed; then as many sequences as put the padded launch on the v3 form with this R
            x1 = rng.standard_normal((1, L, C)).astype(np.float32)
            check_run(eng, fmt, x1, p, dil, None, False, "edge")
            if k != 3:
                check_run(eng, fmt, x1, p, dil, np.array([L], np.int32), True, "edge")
            if k == 3 and R != 4:
                continue
            rows = {2: 4096, 4: 16384 if k == 5 else 4096, 8: 32768}[R]
            B = -(-rows // L)
            x = rng.standard_normal((B, L, C)).astype(np.float32)
            lens = rng.integers(0, L + 1, B).astype(np.int32)
            lens[:3] = (L, 0, L)
            out, form = check_run(eng, fmt, x, p, dil, lens, False, "edge")
            if k != 3:
                assert form.split("<")[1] == f"{k},{R}>", form


# ---- channel widths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (4, 64, 100, 388, 512, 516, 1024))
@pytest.mark.parametrize("fmt", FMTS)
def test_channel_widths(eng, fmt, C):
    rng = np.random.default_rng(C)
    for k, dil in ((5, 2), (7, 1)):
        p = Params(C, k, C + k)
        lens = np.array([19, 0, 23, 1, 23], np.int32)
        x = rng.standard_normal((5, 23, C)).astype(np.float32)
        check_run(eng, fmt, x, p, dil, lens, False, "width")                   # v2 / generic
        if C <= 512:
            check_run(eng, fmt, x, p, dil, lens, True, "width")                # v3, combs of 2 / 4
            xb = rng.standard_normal((180, 23, C)).astype(np.float32)          # 4140 padded rows: v3
            check_run(eng, fmt, xb, p, dil, rng.integers(0, 24, 180).astype(np.int32), False, "width")


# ---- ragged batches: zeros in the padding, NaN in the padding, packed against padded --------------------------------------------------
RAGGED = {  # form family -> (L, C, k)
    "v2<5>": (37, 64, 5), "v2<7>": (37, 100, 7), "v3<5,2>": (900, 16, 5), "v3<5,4>": (3300, 8, 5), "v3<5,8>": (6600, 8, 5),
    "v3<7,4>": (900, 16, 7), "generic_wide": (37, 516, 5), "generic_k3": (37, 64, 3),
}


def ragged_lens(L):
    return np.array([L, 0, L, 1, L // 2], np.int32)  # a zero-length sequence between two full ones


@pytest.mark.parametrize("name", sorted(RAGGED))
@pytest.mark.parametrize("fmt", FMTS)
def test_ragged_padded_nan_padding_and_packed(eng, fmt, name):
    L, C, k = RAGGED[name]
    rng = np.random.default_rng(L + C + k)
    p = Params(C, k, 3)
    lens = ragged_lens(L)
    x = rng.standard_normal((5, L, C)).astype(np.float32)
    pad = np.arange(L)[None, :] >= lens[:, None]
    for dil in (1, 8):
        out, form = check_run(eng, fmt, x, p, dil, lens, False, "ragged")
        if not name.startswith("generic"):
            assert form.replace("occ4", "") == name, form
        # NaN in every input row past a sequence's end: no bit of any output changes (check_run has pinned the padding rows to +0.0)
        xn = x.copy()
        xn[pad] = np.nan
        out_n, form_n = run(eng, fmt, xn, p, dil, lens, False)
        assert form_n == form
        assert np.array_equal(bits(out_n), bits(out)), ("NaN padding reached the output", name, fmt, dil,
                                                        int(np.sum(bits(out_n) != bits(out))), int(np.sum(np.isnan(out_n))))
        if name.startswith("generic"):
            with pytest.raises(binding.StnError):
                run(eng, fmt, x, p, dil, lens, True)
            continue
        # the packed layout of the same batch: float64 always, the padded run's bits where both take the same form
        out_p, form_p = check_run(eng, fmt, x, p, dil, lens, True, "ragged")
        if form_p == form:
            assert np.array_equal(bits(out_p), bits(out)), (name, fmt, dil)
        else:
            assert form.startswith("v2") and form_p.startswith("v3"), (form, form_p)


@pytest.mark.parametrize("fmt", FMTS)
def test_packed_matches_padded_where_v2_cannot(eng, fmt):
    """below 4096 rows the padded form is v2 and the packed one v3: compare the packed small batch with the same sequences inside a padded
    batch large enough for v3 with the same comb (same form asserted), bit for bit"""
    rng = np.random.default_rng(5)
    L, C = 37, 64
    lens = ragged_lens(L)
    x = rng.standard_normal((5, L, C)).astype(np.float32)
    for k, dil in ((5, 2), (7, 4)):
        p = Params(C, k, 9)
        out_p, form_p = check_run(eng, fmt, x, p, dil, lens, True, "small packed")
        Bb = 120  # 4440 padded rows
        xb = rng.standard_normal((Bb, L, C)).astype(np.float32)
        lb = rng.integers(0, L + 1, Bb).astype(np.int32)
        xb[50:55], lb[50:55] = x, lens
        out_b, form_b = check_run(eng, fmt, xb, p, dil, lb, False, "large padded")
        assert form_b == form_p
        assert np.array_equal(bits(out_b[50:55]), bits(out_p))


# ---- position independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 37, 64, 5, False), (3, 37, 64, 5, True), (3, 37, 516, 7, False), (3, 1400, 16, 5, False),
                                   (3, 1400, 16, 7, True), (3, 1400, 16, 7, False)], ids=str)
@pytest.mark.parametrize("fmt", FMTS)
def test_position_and_neighbours_do_not_matter(eng, fmt, shape):
    B, L, C, k, packed = shape
    rng = np.random.default_rng(L + C)
    p = Params(C, k, 13)
    n = L - 5
    seq = rng.standard_normal((L, C)).astype(np.float32)
    res = []
    for pos, lens in ((0, [n, L, 3]), (2, [0, L - 1, n]), (1, [L, n, L])):
        x = (rng.standard_normal((B, L, C)) * (1 + pos)).astype(np.float32)
        x[pos] = seq
        x[pos, n:] = rng.standard_normal((L - n, C))  # what lies behind the sequence in its own padding differs too
        out, form = run(eng, fmt, x, p, 2, np.asarray(lens, np.int32), packed)
        res.append((out[pos, :n], form))
    assert res[0][1] == res[1][1] == res[2][1] == expect_form(fmt, B, L, C, k, packed)
    assert np.array_equal(bits(res[0][0]), bits(res[1][0])) and np.array_equal(bits(res[0][0]), bits(res[2][0]))


# ---- plain LayerNorm --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (4, 144, 512, 1024))
@pytest.mark.parametrize("fmt", FMTS)
def test_layernorm_only(eng, fmt, C):
    p = Params(C, 1, C)
    for M in (1, 3, 4, 5, 1000):
        rng = np.random.default_rng(M + C)
        x = (rng.standard_normal((M, C)) * 2 + 0.5).astype(np.float32)
        buf = np.full((M + 2, C), SENTINEL, np.float32)
        out, form = eng.op_dwconv_ln_ex(x, None, None, p.g, p.bt, 1, buf, M, 1, ln_only=True, dtype=fmt)
        assert form == "layernorm"
        assert np.all(bits(out[M:]) == SENTINEL_BITS)
        check_vals(out[:M], layernorm64(x.astype(np.float64), p.g.astype(np.float64), p.bt.astype(np.float64)), fmt, form, f"layernorm M{M} C{C}")


# ---- fold + LayerNorm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (4, 8, 12, 24))
@pytest.mark.parametrize("rv", (False, True), ids=("norowvec", "rowvec"))
@pytest.mark.parametrize("fmt", ("bf16", "f16"))
def test_fold_ln(eng, fmt, rv, S):
    for M, C in ((37, 384), (5, 100), (130, 1024)):
        rng = np.random.default_rng(S * 1000 + M)
        p = Params(C, 1, S)
        x = rng.standard_normal((M, C)).astype(np.float32)
        part = rnd(rng.standard_normal((S, M, C)) * 0.5, fmt)  # exactly representable: the entry's rounding changes nothing
        b2 = (rng.standard_normal(C) * 0.2).astype(np.float32)
        gamma = (rng.standard_normal(C) * 0.5).astype(np.float32)
        nseq = 3
        rowvec = (rng.standard_normal((nseq, C)) * 0.3).astype(np.float32) if rv else None
        row_b = np.sort(rng.integers(0, nseq, M)).astype(np.int32) if rv else None
        x_new, y = eng.op_fold_ln(x, part, b2, gamma, p.g, p.bt, rowvec=rowvec, row_b=row_b, dtype=fmt)
        ref_x = x.astype(np.float64) + gamma.astype(np.float64) * (part.astype(np.float64).sum(axis=0) + b2.astype(np.float64))
        if rv:
            ref_x = ref_x + rowvec.astype(np.float64)[row_b]
        form = f"fold_ln<S{S}{',rv' if rv else ''}>"
        check_vals(x_new, ref_x, "f32", form, f"{form} residual {fmt} M{M} C{C}")
        check_vals(y, layernorm64(ref_x, p.g.astype(np.float64), p.bt.astype(np.float64)), fmt, form, f"{form} M{M} C{C}")


def test_entry_refuses_bad_arguments(eng):
    p = Params(8, 5, 1)
    x = np.zeros((10, 8), np.float32)
    with pytest.raises(binding.StnError):  # fewer rows than the launch addresses
        eng.op_dwconv_ln_ex(x, p.w, p.bias, p.g, p.bt, 1, x, 2, 6, dtype="f32")
    with pytest.raises(binding.StnError):  # packed rows without lengths
        eng.op_dwconv_ln_ex(x, p.w, p.bias, p.g, p.bt, 1, x, 2, 5, packed=True, dtype="f32")
    with pytest.raises(binding.StnError):  # a length beyond L
        eng.op_dwconv_ln_ex(x, p.w, p.bias, p.g, p.bt, 1, x, 2, 5, seqlen=np.array([6, 1], np.int32), dtype="f32")


def test_zz_report_measured():
    """not a check: prints the largest deviations seen in this session (run with -s)"""
    for (form, fmt), v in sorted(STATS.items()):
        print(f"{form:16s} {fmt:5s}: {'max|d|/rms' if fmt == 'f32' else 'max(|d| - ulp/2)/rms'} = {v:.3e}")
    f32 = [v for (_, fmt), v in STATS.items() if fmt == "f32"]
    if f32:
        print(f"F32_REL measured: {max(f32):.3e} (bound {F32_REL:.1e})")
