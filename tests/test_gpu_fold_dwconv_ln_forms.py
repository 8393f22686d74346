"""Every form of fold_dwconv_ln_kernel<OutT / F16, K, RV, NSLOT, S> (csrc/kernels_fold.hip: 2 formats x K {5, 7} x rowvec on / off x NSLOT {3, 4}
x S {4, 8, 12, 24} = 64 instantiations) and every run length (8, 32, 40, 48 frames per workgroup) against float64, through
stn_op_fold_dwconv_ln_ex.  Each case first asserts the form it expects (binding.fold_dwconv_ln_form pins the same strings without a GPU in
tests/test_fold_dwconv_ln_form_cpu.py), then the values.  No case sets an environment switch: the run lengths are reached the way the launcher
chooses them (few sequences, many sequences, many with FoldArgs::run_frames).

The reference (tests/test_fold_dwconv_ln_form_cpu.py) is plain numpy.  The fold follows the one order kernels_fold.hpp defines — fp32,
(((p0 + p1) + p2) + ...), then x + gamma * (sum + b2) + rowvec[b] — on partial sums rounded to the format; the zero-padded dilated depthwise
conv inside each sequence, its bias and the LayerNorm (eps 1e-6) then run in float64 on that fp32 residual.  All weights are random, so no tap,
channel or split order can be mirrored unnoticed.

Unless a case says otherwise the operands have the engine's layout: the partial sums `part_stride` = (M rounded up to 128 rows) * C apart with
NaN in the gap, rowvec rows C + 4 apart with NaN in the gap, NaN rows behind the last sequence of x_in, and NaN sentinels behind the last
sequence of x_out and y — which must keep their bits.

Bounds ("measured" = the largest value over every case of this file on an MI355X, printed by test_zz_report_measured):
  * x_out: bit-equal to the fp32 numpy fold, every case.
  * y: every element |got - ref| <= 0.5 ulp_fmt(ref) + F32_REL rms(ref), F32_REL = 6e-6 (tests/test_gpu_dwconv_ln_forms.py).  Every case asserts
    on its own inputs that a float32 numpy restatement of conv + LayerNorm in another summation order stays within F32_REL rms(ref) of the
    float64 reference (largest 2.9e-6), so the margin belongs to fp32 arithmetic, not to the kernel.
    Measured max(|d| - ulp/2) / rms, the largest of each group of instantiations (all 64 lie between 0.5e-7 and 1.0e-6, under a fifth of the
    bound): bf16 U3 2.9e-7, bf16 U2 2.9e-7, bf16 U1 3.1e-7 (K5, norv, ns4, S12); f16 U3 5.4e-7, f16 U2 1.0e-6 (K7, norv, ns3, S4), f16 U1 5.9e-7.
    The existing assertion on this kernel (tests/test_gpu_ffn.py) is rms < 4e-3.
  * Exact (bits): the same sequences across run lengths 8 / 32 / 40 / 48; across launch shapes (L, part_stride, rv_ld, zero-length
    neighbours); NaN in every row of another sequence (x and partial sums); position in the batch; x_out against stn_op_fold_ln.

Wall time on an MI355X: 5 s (143 tests)."""
import functools
import time

import numpy as np
import pytest

from supertonic_amd import binding
from test_fold_dwconv_ln_form_cpu import F32_REL, conv_ln32_alt, conv_ln64, expect_form, fold_ref, lds_bytes, max_dil
from test_gpu_dwconv_ln_forms import SENTINEL, SENTINEL_BITS, bits, rnd, ulp

pytestmark = pytest.mark.gpu

STN_ERR_INVALID = -1  # include/stn.h

FMTS = ("bf16", "f16")
STATS = {}        # instantiation -> max(|d| - ulp/2) / rms over the cases that ran it
ALT = [0.0]       # the largest float32-restatement margin
RUNS = set()      # run lengths compared with float64
T0 = [None]


@pytest.fixture(scope="module")
def eng():
    T0[0] = time.time()
    return binding.Engine(0, "bf16")  # (the entry takes its format per call, whatever the engine's)


class Params:
    def __init__(self, C, k, seed):
        rng = np.random.default_rng(seed)
        self.C, self.k = C, k
        self.w = (rng.standard_normal((C, k)) * 0.5).astype(np.float32)
        self.bias = (rng.standard_normal(C) * 0.3).astype(np.float32)
        self.g = (1.0 + 0.3 * rng.standard_normal(C)).astype(np.float32)
        self.bt = (rng.standard_normal(C) * 0.3).astype(np.float32)
        self.b2 = (rng.standard_normal(C) * 0.2).astype(np.float32)
        self.gamma = (rng.standard_normal(C) * 0.5).astype(np.float32)


X_POOL, PART_POOL = 1400 * 512, 24 * 1200 * 512


@functools.lru_cache(maxsize=None)
def _x_pool():
    return np.random.default_rng(1).standard_normal(X_POOL, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _part_pool(fmt):
    return rnd(np.random.default_rng(2).standard_normal(PART_POOL, dtype=np.float32) * np.float32(0.5), fmt)  # values of the format: the entry's rounding changes nothing


def _slice(pool, n, seed):
    """n values of a pool of random numbers, from an offset the seed picks (drawing 7 M normals per case would dominate the file's time)"""
    assert n <= len(pool), n
    o = (seed * 7919) % (len(pool) - n + 1)
    return pool[o:o + n].copy()


class Ops:
    """operands of one launch: x [M, C], part [S, M, C] (values of the format), rowvec [B, C] or None"""
    def __init__(self, fmt, lens, C, S, rv, seed):
        self.fmt, self.lens, self.C, self.S = fmt, [int(v) for v in lens], C, S
        M = self.M = int(sum(self.lens))
        self.x = _slice(_x_pool(), M * C, seed + 1).reshape(M, C)
        self.part = _slice(_part_pool(fmt), S * M * C, seed).reshape(S, M, C)
        self.rowvec = (np.random.default_rng(seed + 2).standard_normal((len(self.lens), C)) * 0.3).astype(np.float32) if rv else None

    def take(self, seqs):
        """the operands of a subset of the sequences, in the given order"""
        off = np.r_[0, np.cumsum(self.lens)]
        rows = np.concatenate([np.arange(off[b], off[b] + self.lens[b]) for b in seqs] + [np.zeros(0, np.int64)]).astype(np.int64)
        o = object.__new__(Ops)
        o.fmt, o.C, o.S = self.fmt, self.C, self.S
        o.lens = [self.lens[b] for b in seqs]
        o.M = len(rows)
        o.x = self.x[rows].copy()
        o.part = np.ascontiguousarray(self.part[:, rows])
        o.rowvec = None if self.rowvec is None else self.rowvec[list(seqs)].copy()
        return o


def launch(eng, ops, p, dil, L=None, run_frames=0, tight=False, tail=3, b2=True, gamma=True):
    """-> (x_out [M, C], y [M, C], form).  Asserts that nothing outside the M rows was written."""
    M, C, S, B = ops.M, ops.C, ops.S, len(ops.lens)
    L = max(ops.lens) if L is None else L
    stride = M * C if tight else -(-M // 128) * 128 * C
    part = np.full((S, stride), np.nan, np.float32)
    part[:, :M * C] = ops.part.reshape(S, M * C)
    part = part.reshape(-1)[:(S - 1) * stride + M * C] if tight else part
    rv = ops.rowvec
    if rv is not None and not tight:
        rv = np.full((B, C + 4), np.nan, np.float32)
        rv[:, :C] = ops.rowvec
    x_in = np.concatenate([ops.x, np.full((tail, C), np.nan, np.float32)])
    buf = np.full((M + tail, C), SENTINEL, np.float32)
    xo, y, form = eng.op_fold_dwconv_ln_ex(np.asarray(ops.lens, np.int32), L, x_in, part, stride, S, p.b2 if b2 else None, p.gamma if gamma else None,
                                           rv, p.w, p.bias, p.g, p.bt, dil, buf, buf, run_frames=run_frames, dtype=ops.fmt)
    assert np.all(bits(xo[M:]) == SENTINEL_BITS) and np.all(bits(y[M:]) == SENTINEL_BITS), "rows past the launch were written"
    return xo[:M], y[:M], form


def check(eng, ops, p, dil, what, L=None, run_frames=0, **kw):
    """form first, then x_out (bits) and y (float64) of one launch"""
    B, C, fmt = len(ops.lens), ops.C, ops.fmt
    Lc = max(ops.lens) if L is None else L
    exp = expect_form(fmt, B, Lc, C, p.k, dil, ops.S, ops.rowvec is not None, run_frames)
    assert binding.fold_dwconv_ln_form(fmt, B, Lc, C, p.k, dil, ops.S, ops.rowvec is not None, run_frames) == exp, what
    xo, y, form = launch(eng, ops, p, dil, L, run_frames, **kw)
    assert form == exp, (what, form, exp)
    b2 = p.b2 if kw.get("b2", True) else np.zeros(C, np.float32)
    gamma = p.gamma if kw.get("gamma", True) else np.ones(C, np.float32)
    rxo = fold_ref(ops.x, ops.part, b2, gamma, ops.rowvec, ops.lens)
    assert np.array_equal(bits(xo), bits(rxo)), (what, form, "x_out differs from the fp32 fold", int(np.sum(bits(xo) != bits(rxo))))
    ref = conv_ln64(rxo, ops.lens, p.w, p.bias, p.g, p.bt, dil)
    rms = np.sqrt(np.mean(ref ** 2)) + 1e-30
    alt = float(np.abs(conv_ln32_alt(rxo, ops.lens, p.w, p.bias, p.g, p.bt, dil).astype(np.float64) - ref).max() / rms)
    ALT[0] = max(ALT[0], alt)
    assert alt <= F32_REL, (what, "the float32 restatement itself leaves the bound", alt)
    assert np.all(np.isfinite(y)), (what, form)
    need = float(np.max((np.abs(y.astype(np.float64) - ref) - 0.5 * ulp(ref, fmt)) / rms))
    inst, run = form.split(" run ")
    STATS[inst] = max(STATS.get(inst, -1.0), need)
    RUNS.add(int(run.split()[0]))
    print(f"{what} {form} C{C} dil{dil} B{B} M{ops.M}: max(|d| - ulp/2)/rms = {need:.3e} (float32 restatement {alt:.3e})")
    assert need <= F32_REL, (what, form, need)
    return xo, y, form


def trips(lens, C, k, dil, U, run=32):
    """phase-1 trips of every workgroup of a launch: a window of nw rows takes ceil(nw / (rpp U)) trips, rpp = 1024 / (C / 8) rows per pass"""
    rpp, half, out = 1024 // (C // 8), (k - 1) // 2, set()
    for n in lens:
        if n == 0:
            continue
        nch = -(-n // run)
        per = -(-n // nch)
        for c in range(nch):
            t0, t1 = c * per, min(c * per + per, n)
            if t0 < t1:
                out.add(-(-(min(t1 + half * dil, n) - max(t0 - half * dil, 0)) // (rpp * U)))
    return out


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------------------
# Dilations per (K, C), chosen so that phase 1 takes both ONE trip and SEVERAL for every U (a window of nw rows against rpp * U; the middle
# run of the 96-frame sequence is 32 frames with both halos, nw = 32 + (K - 1) dil):
#   U = 3 (S 4, K 5, C 384: rpp 21, 63 rows per trip): dil 1 -> nw 36, one trip; dil 8 -> nw 64, two
#   U = 2 (S 4, K 7, C 384: 42 rows per trip):         dil 1 -> nw 38, one trip; dil 2 -> nw 44, two
#   U = 2 (S 4, C 512: rpp 16, 32 rows per trip):      the sequences of up to 32 frames are one window of nw = length <= 32: one trip; every
#                                                      run with a halo (nw >= 32 + dil): two or more
#   U = 1 (S > 4: rpp 21 / 16 rows per trip):          the sequences of 1, 2 and HALF dil +- 1 frames (<= 16): one trip; the rest: several
DILS = {(5, 384): (1, 8), (7, 384): (1, 2), (5, 512): (1, 8), (7, 512): (1, 2)}


def ragged_lens(k, dil):
    half = (k - 1) // 2 * dil
    return [1, 2, max(half - 1, 1), half + 1, 31, 32, 33, 64, 65, 96, 203]


@pytest.mark.parametrize("C", (384, 512))
@pytest.mark.parametrize("S", (4, 8, 12, 24))
@pytest.mark.parametrize("rv", (True, False), ids=("rv", "norv"))
@pytest.mark.parametrize("k", (5, 7))
@pytest.mark.parametrize("fmt", FMTS)
def test_every_instantiation(eng, fmt, k, rv, S, C):
    p = Params(C, k, 100 * k + C)
    U = int(expect_form(fmt, 1, 1, C, k, 1, S, rv).split(",U")[1][0])
    seen = set()
    for dil in DILS[(k, C)]:
        lens = ragged_lens(k, dil)
        assert len(lens) * -(-max(lens) // 32) >= 64  # runs of 32
        seen |= trips(lens, C, k, dil, U)
        check(eng, Ops(fmt, lens, C, S, rv, 7 * S + dil), p, dil, "instantiation")
    assert 1 in seen and max(seen) >= 2, seen


# ---- 2. every run length ------------------------------------------------------------------------------------------------------------------------
# probe sequences: 33 (runs of 40 / 48: ONE run whose second phase-2 pass has one live frame), 66 (runs of 40: two runs of 33), 65 (runs of 32:
# per = ceil(65 / 3) = 22, the last run 21), 81 (runs of 40: per 27), 3 and 1 (shorter than one halo of dil 8), 49, 96, 45 (runs of 48: one run)
PROBE = [33, 66, 65, 81, 3, 1, 49, 96, 45]


@pytest.mark.parametrize("k,C,S,dils", [(5, 384, 4, (1, 8)), (7, 512, 4, (1, 3)), (5, 384, 12, (2, 12)), (7, 384, 24, (7,)), (5, 512, 8, (5,))], ids=str)
@pytest.mark.parametrize("fmt", FMTS)
def test_every_run_length(eng, fmt, k, C, S, dils):
    rng = np.random.default_rng(k + C + S)
    many = PROBE + [int(v) for v in rng.integers(20, 91, 13)]
    n = len(PROBE)
    assert n * -(-max(PROBE) // 32) < 64 <= len(many) * -(-max(many) // 32)
    p = Params(C, k, 3)
    ops_many = Ops(fmt, many, C, S, True, 31 + S)
    ops_few = ops_many.take(range(n))
    m = ops_few.M
    for dil in dils:
        assert lds_bytes(C, k, dil, 48) <= 160 * 1024
        res = {}
        xo, y, form = check(eng, ops_few, p, dil, "run length (few)")
        res[8] = (xo, y)
        for rf, run in ((0, 32), (40, 40), (48, 48)):
            xo, y, form = check(eng, ops_many, p, dil, "run length (many)", run_frames=rf)
            assert f" run {run} " in form, form
            res[run] = (xo[:m], y[:m])
        for run in (32, 40, 48):
            assert np.array_equal(bits(res[run][0]), bits(res[8][0])) and np.array_equal(bits(res[run][1]), bits(res[8][1])), (run, dil)


# ---- 3. other widths -----------------------------------------------------------------------------------------------------------------------------
# C 8: one 8-channel group (C8 = 1, rpp = 1024 rows per pass, more than any window); 64, 96: rpp 128 / 85 > window, one lane group of NSLOT 3
# partly masked; 128, 256: NSLOT 3 with masked slots; 392 (C8 = 49, rpp 20, 44 idle threads), 448: NSLOT 4 with masked slots
@pytest.mark.parametrize("C", (8, 64, 96, 128, 256, 392, 448))
@pytest.mark.parametrize("fmt", FMTS)
def test_other_widths(eng, fmt, C):
    lens = [1, 2, 5, 31, 32, 33, 65, 130]
    for k, S, dil, rv in ((5, 4, 2, True), (7, 12, 1, False), (7, 4, 3, True)):
        p = Params(C, k, C + k)
        ops = Ops(fmt, lens, C, S, rv, C + S)
        a = check(eng, ops, p, dil, "width")                 # 8 x 5 runs: few -> runs of 8
        b = check(eng, ops, p, dil, "width", L=256)          # 8 x 8 = 64: runs of 32, and placeholder workgroups
        assert " run 8 " in a[2] and " run 32 " in b[2]
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


# ---- 4. the largest admitted dilation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,k", [(384, 5), (512, 5), (384, 7), (512, 7)])
@pytest.mark.parametrize("fmt", FMTS)
def test_largest_dilation(eng, fmt, C, k):
    p = Params(C, k, 17)
    for dil, rf, run in ((max_dil(C, k), 0, 32), (max_dil(C, k), 48, 32), (max_dil(C, k, 48), 48, 48), (max_dil(C, k, 40), 40, 40)):
        half = (k - 1) // 2 * dil
        lens = [1, half - 1, half, half + 1, 2 * half + 1, 40, 97, 130, 33, 64, 7, 48, 96]
        assert len(lens) * -(-max(lens) // 32) >= 64
        xo, y, form = check(eng, Ops(fmt, lens, C, 4, True, dil), p, dil, "largest dilation", run_frames=rf)
        assert f" run {run} " in form, form
    with pytest.raises(binding.StnError):
        launch(eng, Ops(fmt, [40, 3], C, 4, True, 1), p, max_dil(C, k) + 1)


# ---- 5. launch shape -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,C,S", [(5, 384, 4), (7, 512, 8), (5, 96, 12)], ids=str)
@pytest.mark.parametrize("fmt", FMTS)
def test_launch_shape(eng, fmt, k, C, S):
    p = Params(C, k, 23)
    rng = np.random.default_rng(C)
    lens = [int(v) for v in rng.integers(1, 100, 24)]
    lens[3], lens[10] = 99, 1
    ops = Ops(fmt, lens, C, S, True, 5)
    dil = 2
    base = check(eng, ops, p, dil, "shape: engine layout")
    off = np.r_[0, np.cumsum(lens)]
    # tight buffers (part_stride = M * C, rv_ld = C, no rows behind the last sequence), and L far beyond every length (placeholder workgroups)
    for kw in (dict(tight=True, tail=0), dict(L=112), dict(L=400), dict(L=400, run_frames=48)):
        got = check(eng, ops, p, dil, f"shape: {kw}", **kw)
        assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(bits(got[1]), bits(base[1])), kw
    # zero-length sequences at the front, in the middle and at the end: the others keep their bits
    order = list(range(len(lens)))
    zl = Ops(fmt, [0, 0] + lens[:9] + [0] + lens[9:] + [0, 0], C, S, True, 5)
    src = ops.take(order)
    zl.x, zl.part = src.x, src.part
    zl.rowvec = np.concatenate([np.full((2, C), 9.0, np.float32), ops.rowvec[:9], np.full((1, C), 9.0, np.float32), ops.rowvec[9:], np.full((2, C), 9.0, np.float32)])
    got = check(eng, zl, p, dil, "shape: zero-length sequences")
    assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(bits(got[1]), bits(base[1]))
    # b2 / gamma left out (0 / 1)
    check(eng, ops, p, dil, "shape: no b2, no gamma", b2=False, gamma=False)
    # one sequence alone, of every probe kind; its bits are those it has in the batch
    for b in (3, 10, 0):
        one = check(eng, ops.take([b]), p, dil, "shape: B = 1")
        assert " run 8 " in one[2]
        assert np.array_equal(bits(one[0]), bits(base[0][off[b]:off[b + 1]])) and np.array_equal(bits(one[1]), bits(base[1][off[b]:off[b + 1]]))


@pytest.mark.parametrize("fmt", FMTS)
def test_1024_sequences(eng, fmt):
    rng = np.random.default_rng(1024)
    lens = [int(v) for v in rng.integers(0, 7, 1024)]
    lens[0], lens[511], lens[1023] = 0, 40, 6
    C, k, S = 64, 5, 4
    p = Params(C, k, 29)
    xo, y, form = check(eng, Ops(fmt, lens, C, S, True, 11), p, 1, "B = 1024")
    assert form.endswith(" run 32 cps 2")
    with pytest.raises(binding.StnError):
        launch(eng, Ops(fmt, [1] * 1025, C, S, True, 11), p, 1)


# ---- 6. isolation --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,C,S,dil,rf", [(5, 384, 4, 8, 0), (5, 384, 4, 8, 40), (7, 384, 4, 2, 0), (5, 512, 4, 1, 48), (7, 512, 12, 6, 0), (5, 64, 24, 4, 0)], ids=str)
@pytest.mark.parametrize("fmt", FMTS)
def test_nan_in_a_neighbour_stays_out(eng, fmt, k, C, S, dil, rf):
    """NaN in every row of one sequence, in x and in its partial sums: every other sequence keeps its bits (a tap outside a sequence is a
    select of the zero row, never 0 * value; a thread past the window's end re-reads a row of its own sequence)"""
    lens = [37, 1, 64, 5, 33, 2, 96, 31, 70, 9, 65, 32, 17, 41, 3, 80, 12, 50, 8, 66, 90, 24]
    assert len(lens) * -(-max(lens) // 32) >= 64
    p = Params(C, k, 37)
    ops = Ops(fmt, lens, C, S, True, 13)
    base = check(eng, ops, p, dil, "isolation", run_frames=rf)
    off = np.r_[0, np.cumsum(lens)]
    for bad in (0, 1, 6, 11, len(lens) - 1):
        o = ops.take(range(len(lens)))
        o.x[off[bad]:off[bad + 1]] = np.nan
        o.part[:, off[bad]:off[bad + 1]] = np.nan
        o.rowvec[bad] = np.nan
        xo, y, form = launch(eng, o, p, dil, run_frames=rf)
        assert form == base[2]
        keep = np.ones(ops.M, bool)
        keep[off[bad]:off[bad + 1]] = False
        assert np.array_equal(bits(xo[keep]), bits(base[0][keep])) and np.array_equal(bits(y[keep]), bits(base[1][keep])), (
            "NaN crossed a sequence boundary", bad, int(np.sum(np.isnan(y[keep]))))
        assert np.all(np.isnan(xo[~keep]))


@pytest.mark.parametrize("k,C,S,dil", [(5, 384, 4, 8), (7, 512, 4, 2), (5, 384, 12, 1), (7, 392, 8, 4)], ids=str)
@pytest.mark.parametrize("fmt", FMTS)
def test_position_and_neighbours_do_not_matter(eng, fmt, k, C, S, dil):
    lens = [70, 33, 9, 96, 1, 45, 64, 20, 81, 31, 58, 7, 66, 32, 90, 3, 40, 77, 12, 65, 50, 88]
    assert len(lens) * -(-max(lens) // 32) >= 64
    p = Params(C, k, 41)
    ops = Ops(fmt, lens, C, S, True, 19)
    base = check(eng, ops, p, dil, "position")
    off = np.r_[0, np.cumsum(lens)]
    rng = np.random.default_rng(S)
    for _ in range(2):
        order = [int(v) for v in rng.permutation(len(lens))]
        sub = ops.take(order)
        xo, y, form = launch(eng, sub, p, dil)
        assert form == base[2]
        r = 0
        for b in order:
            assert np.array_equal(bits(xo[r:r + lens[b]]), bits(base[0][off[b]:off[b + 1]])) and np.array_equal(bits(y[r:r + lens[b]]), bits(base[1][off[b]:off[b + 1]])), b
            r += lens[b]


# ---- 7. the unfused pair ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (4, 8, 12, 24))
@pytest.mark.parametrize("rv", (True, False), ids=("rv", "norv"))
@pytest.mark.parametrize("fmt", FMTS)
def test_x_out_is_fold_ln_s_x(eng, fmt, rv, S):
    """the contract that lets the engine fold a pending update with either kernel: the same residual, bit for bit"""
    for C, k in ((384, 5), (512, 7), (96, 5)):
        lens = [37, 1, 64, 0, 5, 33, 96, 2]
        p = Params(C, k, 43)
        ops = Ops(fmt, lens, C, S, rv, 3 * S)
        xo, y, form = launch(eng, ops, p, 2, L=640)  # (8 x 20 runs: runs of 32)
        row_b = np.repeat(np.arange(len(lens)), lens).astype(np.int32)
        x_new, _ = eng.op_fold_ln(ops.x, ops.part, p.b2, p.gamma, p.g, p.bt, rowvec=ops.rowvec, row_b=row_b if rv else None, dtype=fmt)
        assert np.array_equal(bits(xo), bits(x_new)), (fmt, rv, S, C)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments(eng):
    C, k, S = 64, 5, 4
    p = Params(C, k, 1)
    lens = np.array([5, 0, 7], np.int32)
    M = 12
    x = np.zeros((M, C), np.float32)
    part = np.zeros(S * M * C, np.float32)
    rvec = np.zeros((3, C), np.float32)

    def call(dtype="bf16", lens=lens, L=7, x_in=x, part=part, stride=M * C, S=S, rv=rvec, w=p.w, dil=1, xo=x, y=x):
        return eng.op_fold_dwconv_ln_ex(lens, L, x_in, part, stride, S, p.b2, p.gamma, rv, w, p.bias, p.g, p.bt, dil, xo, y, dtype=dtype)

    call()
    bad = [dict(dtype="f32"), dict(L=6), dict(lens=np.array([5, -1, 8], np.int32)), dict(x_in=x[:11]), dict(xo=x[:11]), dict(y=x[:11]),
           dict(stride=M * C - 8), dict(stride=M * C + 4), dict(part=part[:-1]), dict(S=5), dict(S=2), dict(dil=0), dict(dil=150),
           dict(w=np.zeros((C, 3), np.float32)), dict(rv=np.zeros((3, C + 2), np.float32)), dict(lens=np.zeros(3, np.int32)),
           dict(lens=np.ones(1025, np.int32), L=1)]
    for kw in bad:
        with pytest.raises(binding.StnError) as ei:
            call(**kw)
        assert ei.value.code == STN_ERR_INVALID, kw
    with pytest.raises(binding.StnError):  # a width outside the kernel: C % 8
        eng.op_fold_dwconv_ln_ex(lens, 7, np.zeros((M, 12), np.float32), np.zeros(S * M * 12, np.float32), M * 12, S, None, None, None,
                                 np.zeros((12, k), np.float32), np.zeros(12, np.float32), np.ones(12, np.float32), np.zeros(12, np.float32), 1,
                                 np.zeros((M, 12), np.float32), np.zeros((M, 12), np.float32), dtype="bf16")
    xo, y, form = call()  # the engine is usable afterwards
    assert form == expect_form("bf16", 3, 7, C, k, 1, S, True) and np.all(np.isfinite(y))


# ---- the whole family was covered ------------------------------------------------------------------------------------------------------------------
def test_zz_every_instantiation_and_run_length_ran():
    want = {f"fold_dwconv_ln<{fmt},K{k},{rv},ns{ns},S{S},U{1 if S > 4 else 3 if (k == 5 and ns == 3) else 2}>"
            for fmt in FMTS for k in (5, 7) for rv in ("rv", "norv") for ns in (3, 4) for S in (4, 8, 12, 24)}
    assert len(want) == 64
    assert want == set(STATS), (sorted(want - set(STATS)), sorted(set(STATS) - want))
    assert RUNS == {8, 32, 40, 48}, RUNS


def test_zz_report_measured():
    """not a check: prints the largest deviations seen in this session (run with -s)"""
    for inst, v in sorted(STATS.items()):
        print(f"{inst:44s}: max(|d| - ulp/2)/rms = {v:.3e}")
    if STATS:
        print(f"largest over {len(STATS)} instantiations: {max(STATS.values()):.3e}; float32 restatement: {ALT[0]:.3e} (bound {F32_REL:.1e})")
    if T0[0] is not None:
        print(f"wall time since the first case: {time.time() - T0[0]:.1f} s")
