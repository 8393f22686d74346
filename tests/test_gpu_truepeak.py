"""The true-peak kernel (kernels_truepeak.hip) on an MI355X through stn_op_true_peak, against the float64
statement of the contract in tests/truepeak_ref.py: every span around a lane seam (32) and a workgroup seam (8192), both staging forms,
1e3 behind every span and in front of the next row.  tests/test_truepeak_cpu.py shows that the bounds used here catch a dropped phase,
a zeroed halo and a shift by one sample."""
import numpy as np
import pytest

from supertonic_amd import binding

import truepeak_ref as R

pytestmark = pytest.mark.gpu
W_VEC, W_SCALAR = 16400, 16401


@pytest.fixture(scope="module")
def eng():
    e = binding.Engine(0, "bf16")
    yield e
    e.close()


@pytest.fixture(scope="module")
def rows():
    """the rows at both widths (the scalar width has one more poisoned column), their spans and the float64 envelopes, computed once"""
    x, n = R.kernel_rows(W_VEC)
    xs = np.concatenate([x, np.full((x.shape[0], 1), R.POISON, np.float32)], axis=1)
    for a in (x, xs):
        a.setflags(write=False)
    return {W_VEC: x, W_SCALAR: xs}, n


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(o, x, n, g=None):
    rowsn, W = x.shape
    Ks = (W + 31) // 32
    assert o["pk"].shape == (rowsn, Ks) and not np.isnan(o["pk"]).any() and not np.isnan(o["env"]).any() and not np.isnan(o["tp"]).any()
    for r in range(rowsn):
        gr = 1.0 if g is None else g[r]
        bad = R.env_violations(o["env"][r], x[r], n[r], gr)
        assert bad.size == 0, (r, int(n[r]), bad[:8], o["env"][r][bad[:8]])
        want_pk = R.chunk_peaks(o["env"][r], n[r], W)  # of the device's own envelope: bit for bit
        assert np.array_equal(_bits(o["pk"][r]), _bits(want_pk)), (r, int(n[r]))
        assert not np.signbit(o["pk"][r]).any()
        assert _bits(o["tp"][r]) == _bits(o["pk"][r].max()), (r, int(n[r]))


@pytest.mark.parametrize("W,misalign,form", [(W_VEC, 0, "vec"), (W_SCALAR, 0, "scalar"), (W_VEC, 1, "scalar")])
def test_envelope_chunk_peaks_and_true_peak(eng, rows, W, misalign, form):
    xs, n = rows
    x = xs[W]
    o = eng.op_true_peak(x, 44100, n, x_misalign=misalign)
    assert o["form"] == form
    _check(o, x, n)
    o8 = eng.op_true_peak(x, 8000, n, x_misalign=misalign)  # the filter lives in normalized frequency: the rate changes nothing
    for k in ("tp", "env", "pk"):
        assert np.array_equal(_bits(o[k]), _bits(o8[k])), k
    nopk = eng.op_true_peak(x, 44100, n, x_misalign=misalign, env=False)  # the launch without an envelope: the same peaks
    assert np.array_equal(_bits(nopk["pk"]), _bits(o["pk"])) and np.array_equal(_bits(nopk["tp"]), _bits(o["tp"]))


def test_the_tone_reads_three_db_over_its_sample_peak(eng, rows):
    xs, n = rows
    x = xs[W_VEC]
    o = eng.op_true_peak(x, 44100, n)
    seen = 0
    for r in range(0, x.shape[0], 4):  # (the tone is every span's first row)
        if n[r] >= 8191:
            sp = float(np.abs(x[r, : n[r]]).max())
            db = 20 * np.log10(float(o["tp"][r]) / sp)
            print(f"tone, n = {int(n[r])}: sample peak {sp:.5f}, true peak {float(o['tp'][r]):.5f} (+{db:.2f} dB)")
            assert db > 2.9
            seen += 1
    assert seen == 4
    assert float(o["tp"][0]) == 0.0 and not o["pk"][0].any()  # n = 0


def test_gain_is_the_premultiplied_row(eng, rows):
    xs, n = rows
    for W in (W_VEC, W_SCALAR):
        x = xs[W]
        g = np.linspace(0.37, 2.9, x.shape[0]).astype(np.float32)
        a = eng.op_true_peak(x, 44100, n, gain=g)
        b = eng.op_true_peak((x * g[:, None]).astype(np.float32), 44100, n)
        for k in ("tp", "env", "pk"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (W, k)
        _check(a, x, n, g)


def test_a_row_does_not_depend_on_the_batch_or_the_width(eng, rows):
    xs, n = rows
    x = xs[W_VEC]
    whole = eng.op_true_peak(x, 44100, n)
    for r in (3, 22, 35, 44, 47):
        Wn = max(int(n[r]), 1) + 13  # another W, alone: another tiling of the padding, scalar or vec as it falls
        alone = eng.op_true_peak(np.ascontiguousarray(x[r:r + 1, :Wn]), 44100, n[r:r + 1])
        assert _bits(alone["tp"][0]) == _bits(whole["tp"][r]), r
        assert np.array_equal(_bits(alone["env"][0]), _bits(whole["env"][r, :Wn])), r
        Kn = (int(n[r]) + 31) // 32
        assert np.array_equal(_bits(alone["pk"][0, :Kn]), _bits(whole["pk"][r, :Kn])), r


def test_refusals_are_error_codes_with_messages(eng):
    x = np.zeros((1, 64), np.float32)
    tp = np.zeros(1, np.float32)
    L = eng._lib
    assert L.stn_op_true_peak(eng._h, 16000, 0, 64, x, None, None, 0, tp.ctypes.data, None, None, None, 0) == -1 and "rows" in eng.last_error()
    assert L.stn_op_true_peak(eng._h, 16000, 65536, 64, x, None, None, 0, tp.ctypes.data, None, None, None, 0) == -1
    assert L.stn_op_true_peak(eng._h, 16000, 1, 64, x, None, None, 2, tp.ctypes.data, None, None, None, 0) == -1 and "x_misalign" in eng.last_error()
    for hz in (7999, 192001):
        with pytest.raises(binding.StnError) as ei:
            eng.op_true_peak(x, hz)
        assert ei.value.code == -1 and "sample rate" in str(ei.value)
    with pytest.raises(binding.StnError) as ei:
        eng.op_true_peak(x, 16000, [65])
    assert "outside [0, W]" in str(ei.value)
