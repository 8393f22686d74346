"""Every form of the engine's GEMM launcher (csrc/kernels_gemm.hip) and every fused epilogue, against float64 on operands rounded to the
engine's format, through stn_op_gemm_ex.  Each case first asserts the form it expects (stn_dbg_gemm_form's string, as the launch reports it),
so a heuristic change that moves a shape to another kernel fails here instead of silently losing coverage.

Bounds (one reason each):
  * fp32 outputs: max |d| <= 2e-5 rms(ref), as the GEMM tests of test_gpu_ops.py: fp32 accumulation in another order than float64.
  * 16-bit outputs: |got - ref| <= 1 ulp of the output format at |ref| plus that same fp32 floor (the accumulator is rounded once), and
    the share of elements that differ from the rounded float64 value at all <= FRAC_DIFFER (fp32 summation order moves a value across a
    rounding midpoint; measured on an MI355X over every case here: at most 0.013 % of bf16 and 0.22 % of half outputs).
  * EPI_RESID: the update (out - resid_in) within 2e-5 of its rms: the same fp32 accumulation, plus the rounding of resid + update.
  * Masked rows, sentinels around the written region, transposed-image vs slab store, nt on / off and a row's bits across M: exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.special import erf

from supertonic_amd import binding
from supertonic_amd.binding import ACT_GELU, ACT_GELU_TANH, ACT_NONE, ACT_SILU, EPI_RESID, EPI_STORE, EPI_STORE_T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL_BITS = 0x7FC00000           # the canonical quiet NaN: survives the round trip through bf16 / half bit for bit
SENTINEL = np.array([SENTINEL_BITS], np.uint32).view(np.float32)[0]
FRAC_DIFFER = {"bf16": 0.001, "f16": 0.01}


# ---- float64 model of the engine's arithmetic ------------------------------------------------------------------------------------------
def rnd(x, fmt):
    """Round to the engine's format: bf16 round-to-nearest-even, IEEE half, or fp32 (float64 out)."""
    x = np.asarray(x)
    if fmt == "bf16":
        u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
        return u.astype(np.uint32).view(np.float32).astype(np.float64)
    if fmt == "f16":
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)
    return np.asarray(x, np.float32).astype(np.float64)


def act_ref(x, act, out_fmt):
    """kernels_dev.hpp: fp32 / half outputs take GELU in the erf form and GELU-tanh as the sigmoid form; bf16 outputs take gelu_bf16_f for both."""
    if act == ACT_NONE:
        return x
    if act == ACT_SILU:
        return x / (1.0 + np.exp(-x))
    if out_fmt == "bf16":
        return x / (1.0 + np.exp2(x * (x * x * -0.10294324 - 2.30220819)))
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))
    return x / (1.0 + np.exp(-1.5957691216057308 * x * (1.0 + 0.044715 * x * x)))


def ulp(x, fmt):
    """spacing of the output format at |x| (normal range; half's subnormal step below 2^-14)"""
    e = np.floor(np.log2(np.maximum(np.abs(x), 1e-300)))
    if fmt == "bf16":
        return np.exp2(np.maximum(e, -126) - 7)
    return np.exp2(np.maximum(e, -14) - 10)


def check_store(got, ref, out_fmt, what):
    """got (fp32 or widened 16-bit) against the float64 reference after the activation"""
    got = np.asarray(got, np.float64)
    floor = 2e-5 * (np.sqrt(np.mean(ref ** 2)) + 1e-30)
    d = np.abs(got - ref)
    if out_fmt == "f32":
        assert d.max() <= floor, (what, d.max() / floor)
        return 0.0
    assert np.all(d <= ulp(ref, out_fmt) + floor), (what, float(np.max(d - ulp(ref, out_fmt))))
    frac = float(np.mean(got != rnd(ref, out_fmt)))
    assert frac <= FRAC_DIFFER[out_fmt], (what, frac)
    return frac


def check_update(got, resid_in, upd_ref, what):
    upd = np.asarray(got, np.float64) - np.asarray(resid_in, np.float64)
    d = np.abs(upd - upd_ref).max() / (np.sqrt(np.mean(upd_ref ** 2)) + 1e-30)
    assert d <= 2e-5, (what, d)


def sentinel_ok(buf, M, N):
    """every element outside [:M, :N] still holds the sentinel's bits"""
    bits = np.ascontiguousarray(buf, np.float32).view(np.uint32)
    outside = np.ones(bits.shape, bool)
    outside[:M, :N] = False
    return bool(np.all(bits[outside] == SENTINEL_BITS))


def sample_rows(M, tile, n=256, seed=0):
    """all rows of small launches; else the first and the last row tile in full plus a seeded sample"""
    if M <= 2048:
        return np.arange(M)
    last = (M - 1) // tile * tile
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(tile), np.arange(last, M), rng.integers(0, M, n)]))


class Case:
    """seeded operands of one shape, rounded to the engine's format, and the float64 accumulator of any row subset"""

    def __init__(self, M, N, K, fmt, seed):
        rng = np.random.default_rng(seed)
        self.M, self.N, self.K, self.fmt = M, N, K, fmt
        self.A = rng.standard_normal((M, K), dtype=np.float32)
        self.W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        self.bias = (0.5 * rng.standard_normal(N)).astype(np.float32)
        self.gamma = (1.0 + 0.2 * rng.standard_normal(N)).astype(np.float32)
        self.Ar, self.Wr = rnd(self.A, fmt), rnd(self.W, fmt)
        self.rng = rng

    def acc(self, rows):
        return self.Ar[rows] @ self.Wr.T


def buffer(M, N, ldo, extra_rows, fill=None):
    """the caller's [M + extra_rows][ldo] destination: sentinels everywhere, `fill` in [:M, :N]"""
    buf = np.full((M + extra_rows, ldo), SENTINEL, np.float32)
    if fill is not None:
        buf[:M, :N] = fill
    return buf


@pytest.fixture(scope="module")
def eng():
    from supertonic_amd.arch import tiny_arch
    e = binding.Engine(0, "f32")
    e.load_synthetic(tiny_arch(), 7)
    yield e
    e.close()


def run_store(eng, c, act, out_fmt, ldo, tr=-1, nt=0, len_=None, L=1, extra_rows=2):
    got, form = eng.op_gemm_ex(c.A, c.W, buffer(c.M, c.N, ldo, extra_rows), mode=EPI_STORE, act=act, out_dtype=out_fmt, ldo=ldo,
                               bias=c.bias, len=len_, L=L, nt=nt, tr=tr, dtype=c.fmt)
    return got, form


def ref_store(c, rows, act, out_fmt, len_=None, L=1):
    ref = act_ref(c.acc(rows) + c.bias, act, out_fmt)
    if len_ is not None:
        ref[(rows % L) >= np.asarray(len_)[rows // L]] = 0.0
    return ref


# ---- forms x epilogues, 16-bit engines ---------------------------------------------------------------------------------------------------
# (M, N, K) -> the form launch_gemm takes for a 16-bit engine (EPI_STORE, fp32 output)
FORMS = [
    ((300, 384, 384), "tiled<128,128,2,4,4,64,2> cfg8", (ACT_GELU, ACT_SILU)),
    ((49, 384, 1536), "tiled<64,64,2,2,4,64,2> cfg12", (ACT_GELU_TANH, ACT_NONE)),
    ((9000, 1536, 384), "tiled<256,256,4,4,4,32,2> cfg11", (ACT_GELU, ACT_NONE)),
    ((7436, 1536, 384), "tiled<192,256,3,4,4,32,2> cfg18", (ACT_GELU_TANH, ACT_SILU)),
    ((22000, 1536, 384), "tiled<256,256,2,4,4,32,2> cfg1", (ACT_GELU, ACT_GELU_TANH)),
    ((44000, 1536, 384), "tiled<256,128,4,2,3,32,2> cfg17", (ACT_SILU, ACT_NONE)),
    ((300, 384, 96), "ring_vec", (ACT_GELU, ACT_GELU_TANH)),
    ((300, 130, 96), "ring", (ACT_SILU, ACT_GELU)),
    ((257, 130, 72), "reg", (ACT_GELU_TANH, ACT_NONE)),
]


def epi_of(form_base, want):
    """the 16-bit store form a variant must report: tiled kernels honour `want`, ring_vec always uses its slab, the others store per lane"""
    if form_base.startswith("tiled"):
        return want
    return "slab" if form_base == "ring_vec" else "lane"


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("shape,form,acts", FORMS, ids=[f[1].split(" ")[-1].split("<")[0] for f in FORMS])
def test_form_epilogues(eng, fmt, shape, form, acts):
    M, N, K = shape
    c = Case(M, N, K, fmt, seed=M + 7 * N + K + (1 if fmt == "f16" else 0))
    tile = int(form.split("<")[1].split(",")[0]) if form.startswith("tiled") else 128
    rows = sample_rows(M, tile)
    ldo = N + 8 if N % 8 == 0 else N + 2           # gap columns that a 16-byte store past N would hit
    L = max(16, M // 40)                              # sequences of L rows (at least three); lengths include 0 and L
    nseq = (M + L - 1) // L
    lens = c.rng.integers(0, L + 1, nseq).astype(np.int32)
    lens[0], lens[-1] = L, 0
    fracs = {}
    for act in acts:
        # fp32 store, ldo == N
        got, f = eng.op_gemm_ex(c.A, c.W, np.zeros((M, N), np.float32), act=act, out_dtype="f32", bias=c.bias, dtype=fmt)
        assert f == form + " " + epi_of(form, "slab"), f
        check_store(got[rows], ref_store(c, rows, act, "f32"), "f32", (form, act, "f32"))
        # 16-bit store: transposed image forced on / off (same accumulator, conversion and activation code: same bits), nt on
        got_tr, f = run_store(eng, c, act, fmt, ldo, tr=1)
        assert f == form + " " + epi_of(form, "tr"), f
        got_sl, f = run_store(eng, c, act, fmt, ldo, tr=0)
        assert f == form + " " + epi_of(form, "slab"), f
        got_nt, _ = run_store(eng, c, act, fmt, ldo, tr=0, nt=1)
        assert sentinel_ok(got_tr, M, N) and sentinel_ok(got_sl, M, N) and sentinel_ok(got_nt, M, N), (form, act)
        assert np.array_equal(got_tr.view(np.uint32), got_sl.view(np.uint32)), (form, act, "tr vs slab")
        assert np.array_equal(got_nt.view(np.uint32), got_sl.view(np.uint32)), (form, act, "nt")
        fracs[act] = check_store(got_tr[rows, :N], ref_store(c, rows, act, fmt), fmt, (form, act, fmt))
        # 16-bit store with a row mask (the slab path in the tiled kernels): masked rows exactly 0
        got, f = run_store(eng, c, act, fmt, ldo, len_=lens, L=L)
        assert f == form + " " + epi_of(form, "slab"), f
        assert sentinel_ok(got, M, N)
        m_all = np.arange(M)
        masked = (m_all % L) >= lens[m_all // L]
        assert np.all(got[:M, :N][masked] == 0.0), (form, act, "masked rows")
        check_store(got[rows, :N], ref_store(c, rows, act, fmt, lens, L), fmt, (form, act, fmt, "len"))
    # EPI_RESID: gamma + bias + rowvec + len, and packed rows (row_b) + rowvec
    resid = c.rng.standard_normal((M, N), dtype=np.float32)
    rowvec = (0.3 * c.rng.standard_normal((nseq, N))).astype(np.float32)
    got, f = eng.op_gemm_ex(c.A, c.W, buffer(M, N, ldo, 2, resid), mode=EPI_RESID, ldo=ldo, bias=c.bias, gamma=c.gamma, len=lens, L=L,
                            rowvec=rowvec, dtype=fmt)
    assert f == form + " " + epi_of(form, "slab"), f
    assert sentinel_ok(got, M, N)
    m_all = np.arange(M)
    masked = (m_all % L) >= lens[m_all // L]
    assert np.all(got[:M, :N][masked] == 0.0), (form, "resid masked rows")
    live = rows[~masked[rows]]
    upd = c.gamma * (c.acc(live) + c.bias) + rowvec[live // L]
    check_update(got[live, :N], resid[live], upd, (form, "resid len"))
    row_b = np.sort(c.rng.integers(0, nseq, M)).astype(np.int32)
    got, f = eng.op_gemm_ex(c.A, c.W, buffer(M, N, ldo, 2, resid), mode=EPI_RESID, ldo=ldo, bias=c.bias, gamma=c.gamma, row_b=row_b,
                            rowvec=rowvec, dtype=fmt)
    assert f == form + " " + epi_of(form, "slab"), f
    assert sentinel_ok(got, M, N)
    upd = c.gamma * (c.acc(rows) + c.bias) + rowvec[row_b[rows]]
    check_update(got[rows, :N], resid[rows], upd, (form, "resid row_b"))
    print(f"[{fmt}] {form}: share of 16-bit outputs off the rounded float64 value: " + ", ".join(f"act {a}: {100 * v:.3f} %" for a, v in fracs.items()))


# ---- fp32 engine forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,form", [
    ((600, 384, 256), "tiled<64,64,2,2,4,32,4> slab"),        # fp32 64x64 tile: < 160 tiles of 128x128
    ((2600, 1024, 512), "tiled<128,128,2,2,3,32,4> slab"),    # fp32 128x128 tile: 21 x 8 = 168 tiles
    ((257, 130, 72), "reg lane"),                              # gemm_f32_kernel: K % 32 != 0
    ((600, 130, 256), "reg lane"),                             # gemm_f32_kernel: N % 8 != 0
    ((300, 384, 384), "splitk3+tiled<64,64,2,2,4,32,4> slab"),  # deterministic split-K
    ((49, 384, 1536), "splitk8+tiled<64,64,2,2,4,32,4> slab"),
], ids=["f32_64", "f32_128", "reg_k72", "reg_n130", "splitk3", "splitk8"])
def test_f32_forms(eng, shape, form):
    M, N, K = shape
    c = Case(M, N, K, "f32", seed=M + N + K)
    ldo = N + 8 if N % 8 == 0 else N
    L = 50 if M >= 200 else max(8, M // 4)            # at least three sequences; lengths include 0 and L
    nseq = (M + L - 1) // L
    lens = c.rng.integers(0, L + 1, nseq).astype(np.int32)
    lens[0], lens[-1] = L, 0
    for act in (ACT_GELU, ACT_GELU_TANH, ACT_SILU):
        got, f = eng.op_gemm_ex(c.A, c.W, buffer(M, N, ldo, 2), act=act, ldo=ldo, bias=c.bias, len=lens, L=L, dtype="f32")
        assert f == form, f
        assert sentinel_ok(got, M, N)
        check_store(got[:M, :N], ref_store(c, np.arange(M), act, "f32", lens, L), "f32", (form, act))
    resid = c.rng.standard_normal((M, N), dtype=np.float32)
    rowvec = (0.3 * c.rng.standard_normal((nseq, N))).astype(np.float32)
    got, f = eng.op_gemm_ex(c.A, c.W, buffer(M, N, ldo, 2, resid), mode=EPI_RESID, ldo=ldo, bias=c.bias, gamma=c.gamma, len=lens, L=L,
                            rowvec=rowvec, dtype="f32")
    assert f == form, f
    assert sentinel_ok(got, M, N)
    m_all = np.arange(M)
    masked = (m_all % L) >= lens[m_all // L]
    assert np.all(got[:M, :N][masked] == 0.0)
    live = m_all[~masked]
    check_update(got[live, :N], resid[live], c.gamma * (c.acc(live) + c.bias) + rowvec[live // L], (form, "resid"))


# ---- EPI_STORE_T: [B, N, L] placement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,K,form", [("bf16", 256, "ring lane"), ("bf16", 72, "reg lane"), ("f32", 256, "reg lane")],
                         ids=["bf16_ring", "bf16_reg", "f32_reg"])
def test_store_t(eng, fmt, K, form):
    B, L, N = 5, 37, 136
    M = B * L
    c = Case(M, N, K, fmt, seed=K + 3)
    lens = np.array([37, 1, 0, 20, 36], np.int32)
    out = np.full((B, N, L), SENTINEL, np.float32)
    got, f = eng.op_gemm_ex(c.A, c.W, out, mode=EPI_STORE_T, bias=c.bias, len=lens, L=L, dtype=fmt)
    assert f == form, f
    ref = (c.acc(np.arange(M)) + c.bias).reshape(B, L, N).transpose(0, 2, 1)   # [b][n][t]
    t = np.arange(L)
    for b in range(B):
        assert np.all(got[b][:, t >= lens[b]] == 0.0), (b, "rows past len[b]")
    ref = np.where(t[None, None, :] < lens[:, None, None], ref, 0.0)
    check_store(got, ref, "f32", (fmt, K, "store_t"))


# ---- edges -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("M,N,K", [(1, 384, 384), (63, 384, 384), (65, 384, 384), (127, 384, 384), (129, 384, 384), (255, 384, 384),
                                   (257, 384, 384), (300, 8, 384), (300, 136, 384), (300, 264, 384), (300, 384, 32), (300, 136, 8),
                                   (129, 8, 32)])
def test_edges(eng, fmt, M, N, K):
    """M = tile +- 1 and 1, N = 8 and N a multiple of 8 but not of the tile, one K step, K = 8; ldo > N with sentinels in the gap and below"""
    c = Case(M, N, K, fmt, seed=M * 31 + N + K)
    rows = np.arange(M)
    ldo = N + 8
    out_fmt = fmt
    for act in (ACT_GELU, ACT_NONE):
        got, f = eng.op_gemm_ex(c.A, c.W, buffer(M, N, ldo, 3), act=act, out_dtype=out_fmt, ldo=ldo, bias=c.bias, dtype=fmt)
        assert f == binding.gemm_form(fmt, M, N, K, out_dtype=out_fmt, ldo=ldo), f
        assert sentinel_ok(got, M, N), (f, "sentinel overwritten")
        check_store(got[:M, :N], ref_store(c, rows, act, out_fmt), out_fmt, (f, act))
    resid = c.rng.standard_normal((M, N), dtype=np.float32)
    got, f = eng.op_gemm_ex(c.A, c.W, buffer(M, N, ldo, 3, resid), mode=EPI_RESID, ldo=ldo, bias=c.bias, gamma=c.gamma, dtype=fmt)
    assert sentinel_ok(got, M, N), (f, "resid sentinel overwritten")
    check_update(got[:M, :N], resid, c.gamma * (c.acc(rows) + c.bias), (f, "resid"))


# ---- exact properties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("M1,M2,N,K,form", [
    (300, 200, 384, 384, "tiled<128,128,2,4,4,64,2> cfg8 tr"),
    (64, 7, 384, 1536, "tiled<64,64,2,2,4,64,2> cfg12 tr"),
    (9000, 8800, 1536, 384, "tiled<256,256,4,4,4,32,2> cfg11 tr"),
    (300, 130, 384, 96, "ring_vec slab"),
    (300, 65, 136, 72, "reg lane"),
], ids=["cfg8", "cfg12", "cfg11", "ring_vec", "reg"])
def test_row_bits_do_not_depend_on_m(eng, fmt, M1, M2, N, K, form):
    """include/stn.h ("what is bit-identical"): within one form a row's result does not depend on how many rows the launch has"""
    c = Case(M1, N, K, fmt, seed=N + K)
    outs = []
    for M in (M1, M2):
        got, f = eng.op_gemm_ex(c.A[:M], c.W, np.zeros((M, N), np.float32), act=ACT_GELU, out_dtype=fmt, bias=c.bias, dtype=fmt)
        assert f == form, f
        outs.append(got)
    assert np.array_equal(outs[0][:M2].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,form", [(300, 384, "tiled<128,128,2,4,4,64,2> cfg8 tr"), (64, 128, "tiled<64,64,2,2,4,64,2> cfg12 tr"),
                                      (9000, 1536, "tiled<256,256,4,4,4,32,2> cfg11 tr")], ids=["cfg8", "cfg12", "cfg11"])
def test_asymmetric_identity_16bit_out(eng, fmt, M, N, form):
    """test_gpu_ops.py::test_gemm_asymmetric_identity with a 16-bit output through the transposed image: A stacks identities, W holds
    integers below 256, so every output is an exact integer and a swapped row / column / 4x4 block of the image shows"""
    K = 128
    A = np.zeros((M, K), np.float32)
    A[np.arange(M), np.arange(M) % K] = 1.0
    W = (np.arange(N * K, dtype=np.float32).reshape(N, K) * 7 % 251)
    got, f = eng.op_gemm_ex(A, W, np.zeros((M, N), np.float32), out_dtype=fmt, dtype=fmt)
    assert f == form, f
    assert np.array_equal(got, W.T[np.arange(M) % K]), fmt


# ---- the experiment-only tile configurations (STN_GEMM_CFG=n, bf16) -------------------------------------------------------------------------
CFG_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from supertonic_amd import binding
from supertonic_amd.binding import ACT_GELU, EPI_RESID
from supertonic_amd.arch import tiny_arch
import test_gpu_gemm_epilogues as t
cfg = int(sys.argv[2])
eng = binding.Engine(0, "bf16")
eng.load_synthetic(tiny_arch(), 7)
M, N, K = 301, 264, 384                 # edge tiles in M and N for every tile shape; K % 64 == 0 for the 64-deep configurations
c = t.Case(M, N, K, "bf16", seed=cfg)
rows = np.arange(M)
ldo = N + 8
forms = []
for tr in (0, 1):
    got, f = eng.op_gemm_ex(c.A, c.W, t.buffer(M, N, ldo, 2), act=ACT_GELU, out_dtype="bf16", ldo=ldo, bias=c.bias, tr=tr, dtype="bf16")
    forms.append(f)
    assert (" cfg%d " % cfg) in f, f
    assert t.sentinel_ok(got, M, N), f
    t.check_store(got[:M, :N], t.ref_store(c, rows, ACT_GELU, "bf16"), "bf16", f)
resid = c.rng.standard_normal((M, N), dtype=np.float32)
got, f = eng.op_gemm_ex(c.A, c.W, t.buffer(M, N, ldo, 2, resid), mode=EPI_RESID, ldo=ldo, bias=c.bias, gamma=c.gamma, dtype="bf16")
forms.append(f)
assert t.sentinel_ok(got, M, N), f
t.check_update(got[:M, :N], resid, c.gamma * (c.acc(rows) + c.bias), f)
eng.close()
print("RESULT " + json.dumps(forms))
"""

EXPERIMENT_CFGS = [2, 3, 4, 5, 6, 7, 9, 10, 13, 14, 15, 16]


def test_experiment_tile_configs():
    """The documented tile sweeps (tools/gemm_phases.py, STN_DEV_SWITCHES=1 STN_GEMM_CFG=n): one fresh process per configuration, one at a
    time, each under a time limit; a configuration's results must be right even though the heuristic never picks it."""
    for cfg in EXPERIMENT_CFGS:
        env = dict(os.environ, STN_DEV_SWITCHES="1", STN_GEMM_CFG=str(cfg))
        env.pop("STN_GEMM_TR", None)
        r = subprocess.run([sys.executable, "-c", CFG_CHILD, ROOT, str(cfg)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (cfg, r.stdout[-2000:], r.stderr[-4000:])
        forms = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        assert forms[0].endswith(" slab") and forms[1].endswith(" tr") and forms[2].endswith(" slab"), (cfg, forms)
