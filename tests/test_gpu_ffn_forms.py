"""Every form of the fused pointwise pair (csrc/kernels_ffn.hip: ffn_fused_kernel<384 | 512>, bf16 and IEEE half, and its hidden-split form)
against float64, through stn_op_ffn_ex, which goes through Engine::ffn_launch on the caller's whole buffers.  Each case first asserts the
form that ran ("k4", "k4splitS", "gemms"), then the values.  The reference is plain numpy in float64 at the kernel's declared rounding points:
xn, W1 and W2 rounded to the format; h = xn . W1^T + b1; GELU in the form the kernel declares, x / (1 + exp2(x (x^2 * -0.10294324 -
2.30220819))), rounded once to the format (K4 takes it for half too; the tiled pw1 of the two-launch form takes erf there: act_ref of
test_gpu_gemm_epilogues.py); y = g . W2^T; K4: (x + gamma (y + b2) + rowvec[seq]) * keep; K4-split: each share's y as a 16-bit value.  All
operands are random, so a permuted fragment order, a wrong k permutation of W2 or a wrong accumulator map cannot pass.

What is left between kernel and reference is fp32 summation order and hidden values that land on the other side of a 16-bit rounding
midpoint (v_exp_f32 / v_rcp_f32 are 1-ulp instructions).  Bounds ("measured" = the largest value over every case of this file on an
MI355X, printed by test_zz_report_measured; each bound is at most 4x its measurement):
  * K4 update: max |(got - x_in) - upd_ref| / rms(upd_ref) over every element <= K4_REL.
    Measured bf16 2.6e-3, f16 1.0e-3; bounds 9e-3 / 3.5e-3.  The maximum is ONE hidden value on the other side of a midpoint: the worst
    element (C = 384, I = 192, 1100 rows) is unit 154 of row 844, GELU 1.2460933 against the midpoint 1.2460938 (0.49994 ulp from its
    rounding); undoing that one step leaves 7e-7 in the row, and 7 of the 1100 rows deviate by more than 1e-5 at all.  One step is
    ulp(g) |W2| gamma / rms, so the maximum cannot come much below 1e-3 whatever the kernel does; the rms over all elements does:
    rms(d) / rms(upd_ref) <= K4_RMS, measured 3.6e-5 / 4.0e-5, bounds 1.25e-4 / 1.4e-4 (tests/test_gpu_ffn.py asserts 3e-3).
  * two launches on the same operands against their own reference <= GEMMS_REL, and K4 against the two launches <= CROSS_REL (half: the
    erf form against the exp2 form, up to 4.73e-4 apart before the hidden rounding).
    Measured 1.5e-3 / 3.9e-4 and 1.4e-3 / 2.6e-3; bounds 5e-3 / 1.4e-3 and 4.8e-3 / 9e-3.
  * partial sums: |got - ref| <= 1 ulp_fmt(ref) + PART_FLOOR rms(ref), every element, and the share of elements that differ from
    rnd(ref) at all <= PART_DIFFER sqrt(q), q = the hidden units of a share (that many roundings per element can fall on the other
    side; their summed effect grows with sqrt(q)).  Measured floor 4.9e-3 / 8.4e-4, bounds 1.7e-2 / 2.9e-3; measured share / sqrt(q)
    7.5e-5 / 3.7e-4 (0.16 % of bf16 and 1.6 % of half elements at q = 2048), bounds 2.6e-4 / 1.3e-3.
  * Exact (bits): masked rows are zeros of either sign; x rows >= M and the gap columns of a wider ldo keep their NaN sentinels; part rows
    >= M rounded up to 32 of every share, the gap between shares and everything past S * part_stride keep theirs; a K4-split launch
    returns x as it went in; NaN in the gap columns of xn and rowvec and in x rows >= M changes no bit; a row's result does not depend
    on M, slab or wave (K4, and K4-split for a fixed S).

Wall time on an MI355X: 10 s (72 tests)."""
import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.binding import ACT_GELU
from test_gpu_gemm_epilogues import SENTINEL, SENTINEL_BITS, act_ref, rnd, ulp

pytestmark = pytest.mark.gpu

FMTS = ("bf16", "f16")
K4_REL = {"bf16": 9e-3, "f16": 3.5e-3}        # max |d| / rms(upd_ref)
K4_RMS = {"bf16": 1.25e-4, "f16": 1.4e-4}     # rms(d) / rms(upd_ref)
GEMMS_REL = {"bf16": 5e-3, "f16": 1.4e-3}
CROSS_REL = {"bf16": 4.8e-3, "f16": 9e-3}
PART_FLOOR = {"bf16": 1.7e-2, "f16": 2.9e-3}
PART_DIFFER = {"bf16": 2.6e-4, "f16": 1.3e-3}  # times sqrt(hidden units per share)
STATS = {}


def note(key, v):
    STATS[key] = max(STATS.get(key, 0.0), float(v))


@pytest.fixture(scope="module")
def engs():
    e = {fmt: binding.Engine(0, fmt) for fmt in FMTS}
    yield e
    for v in e.values():
        v.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gelu_k4(x):
    return x / (1.0 + np.exp2(x * (x * x * -0.10294324 - 2.30220819)))


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)) + 1e-30)


class Ops:
    """seeded operands of one block shape and the float64 reference of any leading row count"""

    def __init__(self, M, C, I, fmt, seed, nseq=0):
        rng = np.random.default_rng(seed)
        self.M, self.C, self.I, self.fmt = M, C, I, fmt
        self.xn = rng.standard_normal((M, C), dtype=np.float32)
        self.W1 = (rng.standard_normal((I, C)) / np.sqrt(C)).astype(np.float32)
        self.W2 = (rng.standard_normal((C, I)) / np.sqrt(I)).astype(np.float32)
        self.b1 = (0.3 * rng.standard_normal(I)).astype(np.float32)
        self.b2 = (0.3 * rng.standard_normal(C)).astype(np.float32)
        self.gamma = (0.5 + 0.2 * rng.standard_normal(C)).astype(np.float32)
        self.x = rng.standard_normal((M, C), dtype=np.float32)
        self.rowvec = (0.3 * rng.standard_normal((max(nseq, 1), C))).astype(np.float32)
        self.xr, self.W1r, self.W2r = rnd(self.xn, fmt), rnd(self.W1, fmt), rnd(self.W2, fmt)
        self._g = {}

    def hidden(self, M, erf_form=False):
        """the GELU'd hidden activation of rows [0, M) as the kernel's MFMA operand: rounded once to the format"""
        if erf_form not in self._g:
            h = self.xr @ self.W1r.T + self.b1.astype(np.float64)
            self._g = {erf_form: rnd(act_ref(h, ACT_GELU, self.fmt) if erf_form else gelu_k4(h), self.fmt)}  # (one entry: the large cases are large)
        return self._g[erf_form][:M]

    def y(self, M, gemms=False):
        return self.hidden(M, gemms) @ self.W2r.T

    def shares(self, M, S):
        g, q = self.hidden(M), self.I // S
        return np.stack([g[:, s * q:(s + 1) * q] @ self.W2r[:, s * q:(s + 1) * q].T for s in range(S)])

    def update(self, M, b2=True, gamma=True, rv_rows=None, gemms=False):
        u = self.y(M, gemms)
        if b2:
            u = u + self.b2.astype(np.float64)
        if gamma:
            u = u * self.gamma.astype(np.float64)
        if rv_rows is not None:
            u = u + self.rowvec.astype(np.float64)[rv_rows]
        return u


def padded(a, ld, fill):
    """a [rows, C] in the first columns of a [rows, ld] array whose gap columns hold `fill`"""
    out = np.full((a.shape[0], ld), fill, np.float32)
    out[:, :a.shape[1]] = a
    return out


def run_pair(eng, o, M, mode, b2=True, gamma=True, rowvec=False, len_=None, L=None, row_b=None, ldx=None, ldo=None, rv_ld=None, extra_rows=3,
             tail_fill=SENTINEL, rows=None):
    """modes 0 / 1 on rows [0, M) (or the rows `rows`).  Returns (x_out [M, C], form) after checking the sentinels around the written region."""
    C = o.C
    ldx, ldo, rv_ld = ldx or C, ldo or C, rv_ld or C
    rows = np.arange(M) if rows is None else rows
    M = len(rows)
    xin = np.full((M + extra_rows, ldo), SENTINEL, np.float32)
    xin[:M, :C] = o.x[rows]
    xin[M:, :C] = tail_fill
    rv = padded(o.rowvec, rv_ld, np.nan) if rowvec else None
    got, _, form = eng.op_ffn_ex(padded(o.xn[rows], ldx, np.nan), o.W1, o.b1, o.W2, xin, mode=mode, b2=o.b2 if b2 else None,
                                 gamma=o.gamma if gamma else None, len=len_, L=L, row_b=row_b, rowvec=rv, M=M)
    assert got.shape == xin.shape
    assert np.array_equal(bits(got[M:]), bits(xin[M:])), "x rows at or past M were written"
    assert np.all(bits(got[:M, C:]) == SENTINEL_BITS), "x columns past C were written"
    return got[:M, :C], form


def check_update(got, o, M, upd_ref, bound, key, what, keep=None):
    upd = got.astype(np.float64) - o.x[:M].astype(np.float64)
    if keep is not None:
        assert np.all((bits(got)[~keep] & 0x7FFFFFFF) == 0), (what, "masked rows must come back as zeros")
        upd, upd_ref = upd[keep], upd_ref[keep]
    assert np.all(np.isfinite(upd)), what
    d = float(np.abs(upd - upd_ref).max() / rms(upd_ref))
    r = rms(upd - upd_ref) / rms(upd_ref)
    note(key, d)
    print(f"{what}: max|d|/rms = {d:.3e}, rms(d)/rms = {r:.3e}")
    assert d <= bound, (what, d, bound)
    if key[0] == "k4":
        note(("k4_rms", key[1]), r)
        assert r <= K4_RMS[key[1]], (what, r)


def run_split(eng, o, M, S, want, ldx=None, stride_extra=0, tail=7, rows=None):
    """mode 2 on rows [0, M) (or the rows `rows`), S ways (0: the launcher's choice; `want` = the S expected to run).  Returns part
    [want, M, C] after checking the form, that x came back as it went in, and the sentinels around every share's written rows."""
    C = o.C
    xn = o.xn[:M] if rows is None else o.xn[rows]
    M = xn.shape[0]
    rows128, rows32 = (M + 127) // 128 * 128, (M + 31) // 32 * 32
    stride = rows128 * C + stride_extra
    part = np.full(want * stride + tail, SENTINEL, np.float32)
    xin = np.full((M + 1, C + 4), SENTINEL, np.float32)  # a split launch has no use for x: all NaN
    x_out, p, form = eng.op_ffn_ex(padded(xn, ldx or C, np.nan), o.W1, o.b1, o.W2, xin, mode=2, split=S, part=part, part_stride=stride, M=M,
                                   b2=o.b2, gamma=o.gamma)
    assert form == f"k4split{want}", (form, want)
    assert np.array_equal(bits(x_out), bits(xin)), "a K4-split launch touched x"
    assert np.all(bits(p[want * stride:]) == SENTINEL_BITS), "part past S * part_stride was written"
    sh = p[:want * stride].reshape(want, stride)
    assert np.all(bits(sh[:, rows32 * C:]) == SENTINEL_BITS), "part rows past M rounded up to 32 (or the gap between shares) were written"
    written = sh[:, :rows32 * C].reshape(want, rows32, C)
    assert np.all(np.isfinite(written))
    return written[:, :M]


def check_part(got, ref, fmt, q, what):
    """q = hidden units per share: that many hidden roundings can fall on the other side of a midpoint per element, and their summed
    effect grows with sqrt(q); the cap on the share of elements that differ from rnd(ref) at all is PART_DIFFER sqrt(q)"""
    got = np.asarray(got, np.float64)
    r = rms(ref)
    d = np.abs(got - ref)
    need = float(np.max((d - ulp(ref, fmt)) / r))  # the share of rms(ref) that one ulp at |ref| leaves to cover
    frac = float(np.mean(got != rnd(ref, fmt))) / np.sqrt(q)
    note(("part_floor", fmt), need)
    note(("part_differ", fmt), frac)
    print(f"{what}: max(|d| - ulp)/rms = {need:.3e}, differ / sqrt({q}) = {frac:.3e}")
    assert need <= PART_FLOOR[fmt], (what, need)
    assert frac <= PART_DIFFER[fmt], (what, frac)


# ---- K4: every ring schedule, row edge and both widths --------------------------------------------------------------------------------------
ROWS = (1, 31, 32, 33, 127, 128, 129, 300, 1100)
SHAPES = [(384, I) for I in (128, 192, 1024, 1536, 2304)] + [(512, I) for I in (128, 1024, 2048)]
CEILINGS = [(384, 8192), (512, 7168)]  # the LDS ceilings: at C = 384 the fifth buffer sits behind 8192 + 768 floats of biases


@pytest.mark.parametrize("C,I", SHAPES + CEILINGS, ids=lambda v: str(v))
@pytest.mark.parametrize("fmt", FMTS)
def test_k4_shapes_and_rows(engs, fmt, C, I):
    ceiling = (C, I) in CEILINGS
    assert binding.load().stn_ffn_fused_forms(binding._DTYPES[fmt], C, I) == (2 if C == 384 and I >= 1024 and (I // 32) % 8 == 0 else 1)
    rows = (1, 129, 300) if ceiling else ROWS
    o = Ops(max(rows), C, I, fmt, C + I)
    for M in rows:
        got, form = run_pair(engs[fmt], o, M, 1)
        assert form == "k4"
        check_update(got, o, M, o.update(M), K4_REL[fmt], ("k4", fmt), f"k4 {fmt} C{C} I{I} M{M}")


@pytest.mark.parametrize("C,I", CEILINGS)
@pytest.mark.parametrize("fmt", FMTS)
def test_one_step_past_the_lds_ceiling_is_refused(engs, fmt, C, I):
    assert binding.load().stn_ffn_fused_forms(binding._DTYPES[fmt], C, I) >= 1
    assert binding.load().stn_ffn_fused_forms(binding._DTYPES[fmt], C, I + 64) == 0
    o = Ops(4, C, I + 64, fmt, 1)
    with pytest.raises(binding.StnError):
        run_pair(engs[fmt], o, 4, 1)


@pytest.mark.parametrize("C,I", [(384, 128), (384, 1536), (512, 2048)])
@pytest.mark.parametrize("fmt", FMTS)
def test_k4_row_bits_do_not_depend_on_position(engs, fmt, C, I):
    o = Ops(700, C, I, fmt, 5)
    full, _ = run_pair(engs[fmt], o, 700, 1)
    sel = np.r_[3:40, 129:300, 511:700]
    part, _ = run_pair(engs[fmt], o, 0, 1, rows=sel)
    assert np.array_equal(bits(full[sel]), bits(part))
    one, _ = run_pair(engs[fmt], o, 1, 1)
    assert np.array_equal(bits(full[:1]), bits(one))


# ---- the row mask and the choice of rowvec -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,I", [(384, 192), (512, 1024)])
@pytest.mark.parametrize("fmt", FMTS)
def test_mask_and_rowvec_selection(engs, fmt, C, I):
    L = 70
    lens = np.array([0, 1, L - 1, L, 33, L], np.int32)
    B = len(lens)
    M = B * L
    o = Ops(M, C, I, fmt, 11, nseq=B)
    seq, t = np.arange(M) // L, np.arange(M) % L
    keep = t < lens[seq]
    res = {}
    for mode, form, bound, key in ((1, "k4", K4_REL, "k4"), (0, "gemms", GEMMS_REL, "gemms")):
        # padded rows: the mask by length, rowvec by m / L
        got, f = run_pair(engs[fmt], o, M, mode, rowvec=True, len_=lens, L=L)
        assert f == form
        check_update(got, o, M, o.update(M, rv_rows=seq, gemms=mode == 0), bound[fmt], (key, fmt), f"{form} masked {fmt} C{C}", keep=keep)
        res[mode] = got
        # the mask alone
        got, f = run_pair(engs[fmt], o, M, mode, len_=lens, L=L)
        check_update(got, o, M, o.update(M, gemms=mode == 0), bound[fmt], (key, fmt), f"{form} masked, no rowvec {fmt} C{C}", keep=keep)
        # rowvec by m / L without a mask: no row is zeroed
        got, f = run_pair(engs[fmt], o, M, mode, rowvec=True, L=L)
        check_update(got, o, M, o.update(M, rv_rows=seq, gemms=mode == 0), bound[fmt], (key, fmt), f"{form} rowvec by m/L {fmt} C{C}")
        # packed rows: rowvec by row_b, sequences of unequal length in an order m / L cannot give
        row_b = np.sort(np.random.default_rng(3).integers(0, B, M)).astype(np.int32)[::-1].copy()
        assert not np.array_equal(row_b, seq)
        got, f = run_pair(engs[fmt], o, M, mode, rowvec=True, row_b=row_b)
        check_update(got, o, M, o.update(M, rv_rows=row_b, gemms=mode == 0), bound[fmt], (key, fmt), f"{form} rowvec by row_b {fmt} C{C}")
    # the two forms zero the same rows (check_update has pinned both to zeros of either sign there)
    z1, z0 = (bits(res[1]) & 0x7FFFFFFF) == 0, (bits(res[0]) & 0x7FFFFFFF) == 0
    assert np.array_equal(z1.all(axis=1), z0.all(axis=1)) and np.array_equal(z1.all(axis=1), ~keep)


# ---- optional operands ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,I", [(384, 192), (512, 128)])
@pytest.mark.parametrize("fmt", FMTS)
def test_optional_operands(engs, fmt, C, I):
    M = 129
    o = Ops(M, C, I, fmt, 13, nseq=1)
    for b2 in (False, True):
        for gamma in (False, True):
            for rv in (False, True):
                got, form = run_pair(engs[fmt], o, M, 1, b2=b2, gamma=gamma, rowvec=rv, L=M)
                assert form == "k4"
                ref = o.update(M, b2=b2, gamma=gamma, rv_rows=np.zeros(M, np.int64) if rv else None)
                check_update(got, o, M, ref, K4_REL[fmt], ("k4", fmt), f"k4 {fmt} C{C} b2={b2} gamma={gamma} rowvec={rv}")


# ---- strides, gap columns, rows past M -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,I", [(384, 1024), (512, 1024)])
@pytest.mark.parametrize("fmt", FMTS)
def test_strides_gaps_and_rows_past_m(engs, fmt, C, I):
    L, B = 43, 5
    M = L * B
    o = Ops(M, C, I, fmt, 17, nseq=B)
    seq = np.arange(M) // L
    plain = {}
    for mode, form, bound, key in ((1, "k4", K4_REL, "k4"), (0, "gemms", GEMMS_REL, "gemms")):
        plain[mode], f = run_pair(engs[fmt], o, M, mode, rowvec=True, L=L)
        assert f == form
        # wider rows everywhere, NaN in the gap columns of xn and rowvec (run_pair fills them), sentinels in the gap of x and in the rows past M
        wide, f = run_pair(engs[fmt], o, M, mode, rowvec=True, L=L, ldx=C + 8, ldo=C + 4, rv_ld=C + 4)
        assert f == form
        check_update(wide, o, M, o.update(M, rv_rows=seq, gemms=mode == 0), bound[fmt], (key, fmt), f"{form} wide rows {fmt} C{C}")
        assert np.array_equal(bits(wide), bits(plain[mode])), "the strides changed a bit"
        # finite values in the rows past M instead of NaN: nothing changes
        fin, f = run_pair(engs[fmt], o, M, mode, rowvec=True, L=L, ldx=C + 8, ldo=C + 4, rv_ld=C + 4, tail_fill=1.5)
        assert np.array_equal(bits(fin), bits(wide)), "x rows past M reached the result"


# ---- the two launches on the same operands ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,I,M", [(384, 1536, 300), (512, 2048, 300), (384, 128, 33), (512, 1024, 1100)])
@pytest.mark.parametrize("fmt", FMTS)
def test_two_launches_against_their_reference_and_k4(engs, fmt, C, I, M):
    o = Ops(M, C, I, fmt, 19)
    k4, f1 = run_pair(engs[fmt], o, M, 1)
    two, f0 = run_pair(engs[fmt], o, M, 0)
    assert (f1, f0) == ("k4", "gemms")
    check_update(k4, o, M, o.update(M), K4_REL[fmt], ("k4", fmt), f"k4 {fmt} C{C} I{I} M{M}")
    check_update(two, o, M, o.update(M, gemms=True), GEMMS_REL[fmt], ("gemms", fmt), f"gemms {fmt} C{C} I{I} M{M}")
    cross = two.astype(np.float64) - o.x[:M].astype(np.float64)
    check_update(k4, o, M, cross, CROSS_REL[fmt], ("cross", fmt), f"k4 vs gemms {fmt} C{C} I{I} M{M}")


# ---- K4-split --------------------------------------------------------------------------------------------------------------------------------
SPLIT_M = (129, 1000, 1100, 1536, 1664, 4224)  # 2, 8, 9, 12, 13 and 33 slabs: both sides of a multiple of 8, of 12 and of 32
_SPLIT_OPS = {}


def split_ops(fmt, I=1536, M=4224):
    if (fmt, I) not in _SPLIT_OPS:
        _SPLIT_OPS.clear()  # (one entry: consecutive cases share it)
        _SPLIT_OPS[(fmt, I)] = Ops(M, 384, I, fmt, 23 + I)
    return _SPLIT_OPS[(fmt, I)]


@pytest.mark.parametrize("S", (4, 8, 12))
@pytest.mark.parametrize("fmt", FMTS)
def test_split_forced_ways_at_every_slab_count(engs, fmt, S):
    """S forced at each row count: every element of every share against float64, and a row's partial sums bit for bit whatever M, slab or
    wave it sits in."""
    o = split_ops(fmt)
    ref = o.shares(max(SPLIT_M), S)
    base = None
    for M in sorted(SPLIT_M, reverse=True):
        got = run_split(engs[fmt], o, M, S, S)
        check_part(got, ref[:, :M], fmt, o.I // S, f"k4split{S} {fmt} M{M}")
        if base is None:
            base = got
        else:
            assert np.array_equal(bits(got), bits(base[:, :M])), (S, M, "a row's partial sums depend on the launch's row count")
    sel = np.r_[5:6, 37:170, 1000:1290, 4000:4224]  # other waves, other slabs, another slab count
    got = run_split(engs[fmt], o, 0, S, S, rows=sel)
    assert np.array_equal(bits(got), bits(base[:, sel]))


@pytest.mark.parametrize("fmt", FMTS)
def test_split_the_launchers_choice(engs, fmt):
    o = split_ops(fmt)
    for M, want in ((1536, 12), (1537, 8), (4096, 8), (4097, 4)):  # 12 / 13 and 32 / 33 slabs
        assert binding.ffn_form(fmt, binding.FFN_ESTIMATOR, 384, 1536, M) == f"k4split{want}"
        got = run_split(engs[fmt], o, M, 0, want)
        check_part(got, o.shares(M, want), fmt, o.I // want, f"k4split (chosen {want}) {fmt} M{M}")


@pytest.mark.parametrize("I,M,want", [(1024, 1000, 4), (1024, 2000, 8), (2304, 1000, 12), (2304, 2000, 4), (8192, 300, 4), (8192, 2000, 8)])
@pytest.mark.parametrize("fmt", FMTS)
def test_split_fall_backs_and_short_shares(engs, fmt, I, M, want):
    """I = 1024 does not split 12 ways and I = 2304 not 8 ways ((I / 32) % (2 S) != 0): the launcher falls back to 4.  8 ways at I = 1024
    are T = 4 tiles per share (one LIVE trip and the TAIL trip), as 12 ways at I = 1536; I = 8192 is the LDS ceiling."""
    assert binding.ffn_form(fmt, binding.FFN_ESTIMATOR, 384, I, M) == f"k4split{want}"
    o = split_ops(fmt, I, 2000)
    got = run_split(engs[fmt], o, M, 0, want, ldx=384 + 8, stride_extra=64)
    check_part(got, o.shares(M, want), fmt, I // want, f"k4split{want} {fmt} I{I} M{M}")
    forced = run_split(engs[fmt], o, M, want, want)
    assert np.array_equal(bits(forced), bits(got))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments(engs):
    eng = engs["bf16"]
    M, C, I = 40, 384, 1024
    o = Ops(M, C, I, "bf16", 29, nseq=2)
    xin = o.x.copy()

    def call(e=eng, **kw):
        a = dict(xn=o.xn, W1=o.W1, b1=o.b1, W2=o.W2, x=xin, mode=1)
        a.update(kw)
        return e.op_ffn_ex(a.pop("xn"), a.pop("W1"), a.pop("b1"), a.pop("W2"), a.pop("x"), **a)

    part = np.zeros(4 * 128 * C, np.float32)
    assert call()[2] == "k4" and call(mode=0)[2] == "gemms" and call(mode=2, part=part, part_stride=128 * C)[2] == "k4split4"
    f32 = binding.Engine(0, "f32")
    for kw in (dict(e=f32, dtype="bf16"), dict(e=f32), dict(dtype="f16"), dict(e=f32, mode=0)):  # fp32 engines, another format than the engine's
        with pytest.raises(binding.StnError):
            call(**kw)
    f32.close()
    for Ib in (64, 96, 160):  # I = 64, I % 64 != 0
        with pytest.raises(binding.StnError):
            call(W1=np.zeros((Ib, C), np.float32), b1=np.zeros(Ib, np.float32), W2=np.zeros((C, Ib), np.float32))
    with pytest.raises(binding.StnError):  # C = 256
        call(xn=np.zeros((M, 256), np.float32), W1=np.zeros((I, 256), np.float32), W2=np.zeros((256, I), np.float32), x=np.zeros((M, 256), np.float32))
    for S in (1, 2, 5, 12, 16, 24):  # an S outside FFN_SPLITS, or one I = 1024 does not run with
        with pytest.raises(binding.StnError):
            call(mode=2, split=S, part=np.zeros(24 * 128 * C, np.float32), part_stride=128 * C)
    with pytest.raises(binding.StnError):  # no K4-split at C = 512
        call(xn=np.zeros((M, 512), np.float32), W1=np.zeros((I, 512), np.float32), W2=np.zeros((512, I), np.float32), x=np.zeros((M, 512), np.float32),
             mode=2, split=4, part=np.zeros(4 * 128 * 512, np.float32), part_stride=128 * 512)
    for kw in (dict(M=M + 1),                                                        # xn and x hold fewer rows than M
               dict(xn=o.xn[:M - 1], M=M), dict(x=xin[:M - 1], M=M),
               dict(mode=2, part=part[:-1], part_stride=128 * C),                    # part smaller than S * part_stride
               dict(mode=2, part=part, part_stride=127 * C),                         # shares closer than the padded rows
               dict(mode=2, part=np.zeros(4 * (128 * C + 4), np.float32), part_stride=128 * C + 4),  # shares not 16-byte aligned
               dict(mode=2), dict(mode=1, part=part, part_stride=128 * C), dict(mode=1, split=4),
               dict(len=np.array([20, 20], np.int32), L=20, row_b=np.zeros(M, np.int32)),           # len together with row_b
               dict(len=np.array([21, 20], np.int32), L=20), dict(len=np.array([20], np.int32), L=20),
               dict(rowvec=o.rowvec[:1], L=20), dict(rowvec=o.rowvec, row_b=np.full(M, 2, np.int32)),
               dict(xn=padded(o.xn, C + 4, 0.0)), dict(x=padded(xin, C + 2, 0.0)), dict(rowvec=padded(o.rowvec, C + 2, 0.0), L=20),
               dict(mode=3)):
        with pytest.raises(binding.StnError):
            call(**kw)


def test_zz_report_measured():
    """not a check: prints the largest deviations seen in this session (run with -s)"""
    for key, v in sorted(STATS.items(), key=str):
        print(f"{key[0]:12s} {key[1]:5s}: {v:.3e}")
