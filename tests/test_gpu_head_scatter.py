"""The vocoder's exit without a copy of the waveform: the head GEMM stores its packed rows where they belong (the packed-row destination map of
the tiled kernels' fp32 slab epilogue, csrc/kernels_gemm.hip, through stn_op_gemm_rows) and fill_rows_kernel (csrc/kernels_layout.hip, through
stn_op_layout) writes the rows the GEMM leaves out.

Shape: B = 5 sequences in rows of T = 70, valid = [70, 1, 33, 64, 70] — 238 packed rows, so a sequence straddles the 128-row tile edge, one
sequence has a single row, two are untrimmed.  N = 512 and N = 200 (not a multiple of the 128-column tile), K = 64.  Everything is bits:
  * after the GEMM alone every row t < valid[b] equals the plain-store GEMM's packed row, every other row of the destination and the guard
    behind it still hold the sentinel;
  * a sequence that owns more rows than it stores (the 2rf trim form: rows = valid + rf), dead rows behind the last sequence (a row count
    rounded up to a shape bucket) and an empty sequence change nothing of that;
  * after the fill rows t >= valid[b] equal numpy's restatement of the rule — edge[t - (T - rf)] for t >= T - rf, else quiet (rf = 3 and 0),
    or zeros — and the rows below are unchanged."""
import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.binding import LAYOUT_FILL_ROWS

pytestmark = pytest.mark.gpu

SENTINEL_BITS = 0x7FC00000
SENTINEL = np.array([SENTINEL_BITS], np.uint32).view(np.float32)[0]
B, T, K = 5, 70, 64
VALID = np.array([70, 1, 33, 64, 70], np.int32)
GUARD = 16


@pytest.fixture(scope="module")
def eng():
    return binding.Engine(0, "bf16")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sent(*shape):
    return np.full(shape, SENTINEL, np.float32)


def operands(N, M):
    rng = np.random.default_rng(N + M)
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = (rng.standard_normal((N, K)) * 0.2).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    return A, W, bias


def check_scatter(eng, fmt, N, rows, valid, M):
    A, W, bias = operands(N, M)
    plain, form_plain = eng.op_gemm_ex(A, W, sent(M, N), bias=bias, dtype=fmt)
    assert np.all(np.isfinite(plain))
    dst = sent(B * T * N + GUARD)
    got, form = eng.op_gemm_rows(A, W, dst, rows, valid, T, bias=bias, dtype=fmt)
    assert form == form_plain and "tiled" in form and form.endswith("slab")
    assert np.all(bits(got[B * T * N:]) == SENTINEL_BITS)
    got = got[:B * T * N].reshape(B, T, N)
    off = np.concatenate([[0], np.cumsum(rows)])
    for b in range(B):
        v = int(valid[b])
        assert np.array_equal(bits(got[b, :v]), bits(plain[off[b]:off[b] + v])), (fmt, N, b)
        assert np.all(bits(got[b, v:]) == SENTINEL_BITS), (fmt, N, b)
    return got


@pytest.mark.parametrize("N", (512, 200))
@pytest.mark.parametrize("fmt", ("bf16", "f16", "f32"))
def test_gemm_stores_rows_where_they_belong(eng, fmt, N):
    assert int(VALID.sum()) == 238
    check_scatter(eng, fmt, N, VALID, VALID, 238)


@pytest.mark.parametrize("N", (512, 200))
def test_owned_rows_beyond_valid_dead_rows_and_an_empty_sequence(eng, N):
    rf = 3
    rows = np.minimum(VALID + rf, T).astype(np.int32)  # the 2rf trim form computes rf more rows than it keeps
    check_scatter(eng, "bf16", N, rows, VALID, int(rows.sum()))
    check_scatter(eng, "bf16", N, VALID, VALID, 238 + 146)  # 384 rows: dead ones fill the second tile and all of a third
    v0 = VALID.copy()
    v0[1] = 0
    check_scatter(eng, "bf16", N, v0, v0, int(v0.sum()))


def fill_ref(dst, valid, rf, quiet, edge):
    ref = dst.copy()
    for b in range(B):
        for t in range(int(valid[b]), T):
            ref[b, t] = 0.0 if quiet is None else (edge[t - (T - rf)] if t >= T - rf else quiet)
    return ref


@pytest.mark.parametrize("W", (512, 200))
@pytest.mark.parametrize("rule", ("quiet_rf3", "quiet_rf0", "zeros"))
def test_fill_writes_the_rest_and_nothing_else(eng, rule, W):
    rng = np.random.default_rng(W)
    rf = 3 if rule == "quiet_rf3" else 0
    quiet = None if rule == "zeros" else rng.standard_normal(W).astype(np.float32)
    edge = None if rule == "zeros" or rf == 0 else rng.standard_normal((rf, W)).astype(np.float32)
    dst = rng.standard_normal((B, T, W)).astype(np.float32)  # stands for what the GEMM stored (and, past valid, for stale samples)
    buf = np.concatenate([dst.reshape(-1), sent(GUARD)])
    for valid in (VALID, np.array([0, 70, 69, 68, 1], np.int32)):  # the second: the rest begins inside the edge tail, and a whole row of rest
        out = eng.op_layout(LAYOUT_FILL_ROWS, [B, T, W, rf, int(quiet is None)], a=quiet, b=edge, length=valid, out=buf)[0]
        assert np.all(bits(out[B * T * W:]) == SENTINEL_BITS)
        assert np.array_equal(bits(out[:B * T * W].reshape(B, T, W)), bits(fill_ref(dst, valid, rf, quiet, edge))), (rule, W)


def test_scatter_then_fill_covers_every_row(eng):
    N, rf = 512, 3
    got = check_scatter(eng, "bf16", N, VALID, VALID, 238)
    rng = np.random.default_rng(1)
    quiet = rng.standard_normal(N).astype(np.float32)
    edge = rng.standard_normal((rf, N)).astype(np.float32)
    out = eng.op_layout(LAYOUT_FILL_ROWS, [B, T, N, rf, 0], a=quiet, b=edge, length=VALID, out=got)[0].reshape(B, T, N)
    assert np.all(np.isfinite(out))
    assert np.array_equal(bits(out), bits(fill_ref(got, VALID, rf, quiet, edge)))


def test_refusals(eng):
    A, W, bias = operands(20, 238)  # N % 8 != 0: no vector epilogue, no map
    with pytest.raises(binding.StnError):
        eng.op_gemm_rows(A, W[:20], sent(B * T * 20), VALID, VALID, T, bias=bias[:20], dtype="bf16")
    A, W, bias = operands(64, 238)
    with pytest.raises(binding.StnError):
        eng.op_gemm_rows(A, W, sent(B * T * 64), VALID, VALID + 1, T, dtype="bf16")  # valid beyond the rows a sequence owns
    with pytest.raises(binding.StnError):
        eng.op_gemm_rows(A, W, sent(B * T * 64 - 1), VALID, VALID, T, dtype="bf16")  # destination too small
    with pytest.raises(binding.StnError):
        eng.op_layout(LAYOUT_FILL_ROWS, [B, T, 64, 3, 0], a=np.zeros(64, np.float32), length=VALID, out=sent(B * T * 64))  # no edge tail
