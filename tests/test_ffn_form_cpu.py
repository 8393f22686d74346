"""The ConvNeXt pointwise pair's choice of form (ffn_form in csrc/kernels_ffn.hip, reported by stn_dbg_ffn_form without a device), pinned on
both sides of every threshold: two GEMMs, K4 or K4-split.  tests/test_gpu_ffn.py checks each form's results; this file keeps a shape from
drifting to another form unnoticed.  tests/test_gpu_ffn_forms.py runs every K4 and K4-split form against float64 with the GELU form pinned here."""
import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.binding import FFN_ESTIMATOR, FFN_TEXT, FFN_VOCODER

VO = (512, 2048)  # the vocoder's C, I
VE = (384, 1536)  # the estimator's


def form(dtype, stage, shape, M, **kw):
    return binding.ffn_form(dtype, stage, *shape, M, **kw)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_vocoder_k4_from_min_rows(dtype):
    assert form(dtype, FFN_VOCODER, VO, 18431, packed=False) == "gemms"
    assert form(dtype, FFN_VOCODER, VO, 18432, packed=False) == "k4"
    assert form(dtype, FFN_VOCODER, VO, 18432) == "k4"  # packed rows too; never split outside the estimator
    assert form(dtype, FFN_VOCODER, VO, 200, min_rows=200) == "k4" and form(dtype, FFN_VOCODER, VO, 199, min_rows=200) == "gemms"


def test_gate_rows_decide_k4():
    # a trimmed vocoder decides on its dense B*T, not on the packed rows it launches
    assert form("bf16", FFN_VOCODER, VO, 10000, gate_rows=18432) == "k4"
    assert form("bf16", FFN_VOCODER, VO, 10000, gate_rows=18431) == "gemms"
    assert form("bf16", FFN_VOCODER, VO, 20000, gate_rows=18431) == "gemms"
    assert form("bf16", FFN_VOCODER, VO, 20000, gate_rows=0) == "k4"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_estimator_split_needs_packed_rows(dtype):
    assert form(dtype, FFN_ESTIMATOR, VE, 1) == "k4split12"
    for M in (1, 1000, 20000):
        assert form(dtype, FFN_ESTIMATOR, VE, M, packed=False) == "gemms", M
    assert form(dtype, FFN_ESTIMATOR, VE, 20000, packed=False, mask=15) == "k4"  # padded: K4 by the estimator's own bit
    assert form(dtype, FFN_ESTIMATOR, VE, 100, split_min_rows=100) == "k4split12"
    assert form(dtype, FFN_ESTIMATOR, VE, 99, split_min_rows=100) == "gemms"


def test_split_ways_by_row_count():
    # 12 ways up to 12 slabs of 128 rows, 8 ways up to 32 slabs, 4 beyond
    assert form("bf16", FFN_ESTIMATOR, VE, 1536) == "k4split12"
    assert form("bf16", FFN_ESTIMATOR, VE, 1537) == "k4split8"
    assert form("bf16", FFN_ESTIMATOR, VE, 4096) == "k4split8"
    assert form("bf16", FFN_ESTIMATOR, VE, 4097) == "k4split4"
    assert form("bf16", FFN_ESTIMATOR, VE, 200000) == "k4split4"
    # the hidden width must split into an even number of 32-unit tiles per share: I = 1024 (32 tiles) takes 4 and 8 ways, not 12
    assert form("bf16", FFN_ESTIMATOR, (384, 1024), 1000) == "k4split4"
    assert form("bf16", FFN_ESTIMATOR, (384, 1024), 2000) == "k4split8"


def test_split_fall_backs_and_lds_ceilings():
    """ffn_split_choose / ffn_split_valid: a share is an even number of 32-unit tiles, (I / 32) % (2 S) == 0, else the launch falls back to 4 ways."""
    lib = binding.load()
    for dtype in ("bf16", "f16"):
        # I = 1024 (32 tiles): no 12 ways; I = 2304 (72 tiles): no 8 ways; I = 1536 (48 tiles): all three
        for I, ways in ((1024, (4, 4, 8, 8, 4)), (2304, (12, 12, 4, 4, 4)), (1536, (12, 12, 8, 8, 4)), (8192, (4, 4, 8, 8, 4))):
            got = tuple(form(dtype, FFN_ESTIMATOR, (384, I), M) for M in (1, 1536, 1537, 4096, 4097))
            assert got == tuple(f"k4split{w}" for w in ways), (dtype, I, got)
        # the LDS ceilings (ring + biases + at C = 384 the fifth buffer <= 160 KiB; I <= 8192): K4 up to them, nothing one step of 64 past them
        d = binding._DTYPES[dtype]
        assert lib.stn_ffn_fused_forms(d, 384, 8192) == 2 and lib.stn_ffn_fused_forms(d, 384, 8256) == 0
        assert lib.stn_ffn_fused_forms(d, 512, 7168) == 1 and lib.stn_ffn_fused_forms(d, 512, 7232) == 0
        assert form(dtype, FFN_TEXT, (384, 8192), 4000, mask=15, min_rows=1) == "k4" and form(dtype, FFN_TEXT, (384, 8256), 4000, mask=15, min_rows=1) == "gemms"
        assert form(dtype, FFN_VOCODER, (512, 7168), 4000, min_rows=1) == "k4" and form(dtype, FFN_VOCODER, (512, 7232), 4000, min_rows=1) == "gemms"
        assert form(dtype, FFN_ESTIMATOR, (384, 8256), 1000) == "gemms"
        # the smallest ring schedule and the floor: I = 128 runs K4 (no split: fewer than 1024 hidden units), I = 64 does not
        assert lib.stn_ffn_fused_forms(d, 384, 128) == 1 and lib.stn_ffn_fused_forms(d, 512, 128) == 1
        assert lib.stn_ffn_fused_forms(d, 384, 64) == 0 and lib.stn_ffn_fused_forms(d, 384, 160) == 0
        assert form(dtype, FFN_ESTIMATOR, (384, 128), 1000) == "gemms" and form(dtype, FFN_ESTIMATOR, (384, 128), 1000, mask=2, min_rows=1) == "k4"


def test_gelu_form_against_erf():
    """The GELU form K4 computes in both formats and the tiled pw1 for bf16 outputs (gelu_bf16_f, kernels_dev.hpp; the asm blocks of
    kernels_ffn_body.inc), x / (1 + exp2(x (x^2 * -0.10294324 - 2.30220819))), against the erf form in float64 on [-12, 12], grid 1e-5: the
    largest deviation is 4.73e-4, at x = -2.70 and, both forms being x times a sigmoid-like factor, at +2.70.  The upper bound is what the kernels' comments promise; the lower one keeps the constants
    from drifting unnoticed."""
    from scipy.special import erf
    x = np.arange(-1200000, 1200001) * 1e-5
    got = x / (1.0 + np.exp2(x * (x * x * -0.10294324 - 2.30220819)))
    err = np.abs(got - 0.5 * x * (1.0 + erf(x / np.sqrt(2.0))))
    assert 4.5e-4 < err.max() <= 4.8e-4, err.max()
    assert abs(abs(x[err.argmax()]) - 2.70) < 0.01, x[err.argmax()]


def test_split_shapes():
    # K4-split exists for C = 384 only: the estimator's C = 512, I = 2048 never splits
    assert form("bf16", FFN_ESTIMATOR, VO, 1000) == "gemms"
    assert form("bf16", FFN_ESTIMATOR, VO, 1000, mask=15, min_rows=1) == "k4"
    # the fold kernel must take the stage's conv: k = 5 or 7, and an image of 32 + (k-1) * dil + k + 4 rows of C floats within 160 KiB
    assert form("bf16", FFN_ESTIMATOR, VE, 1000, k=3) == "gemms"
    assert form("bf16", FFN_ESTIMATOR, VE, 1000, k=7) == "k4split12"
    assert form("bf16", FFN_ESTIMATOR, VE, 1000, max_dil=16) == "k4split12"  # (32 + 64 + 9) * 1536 = 161280 bytes
    assert form("bf16", FFN_ESTIMATOR, VE, 1000, max_dil=17) == "gemms"      # (32 + 68 + 9) * 1536 = 167424 bytes
    assert form("bf16", FFN_ESTIMATOR, VE, 1000, k=7, max_dil=10) == "k4split12"
    assert form("bf16", FFN_ESTIMATOR, VE, 1000, k=7, max_dil=11) == "gemms"
    assert form("bf16", FFN_ESTIMATOR, VE, 1000, max_dil=17, mask=15, min_rows=1) == "k4"  # falls back to K4 where its bit is set
    # K4 takes C = 384 and 512 only
    assert form("bf16", FFN_TEXT, (256, 1024), 40000, mask=15) == "gemms"
    assert form("bf16", FFN_TEXT, VE, 40000, mask=15) == "k4"


def test_stage_mask():
    big = 30000
    # the default 9: the vocoder's K4 and the estimator's K4-split
    assert form("bf16", FFN_VOCODER, VO, big) == "k4"
    assert form("bf16", FFN_ESTIMATOR, VE, big) == "k4split4"
    assert form("bf16", FFN_ESTIMATOR, VE, big, packed=False) == "gemms"
    assert form("bf16", FFN_TEXT, VE, big) == "gemms"
    for mask in (0, 2):
        assert form("bf16", FFN_VOCODER, VO, big, mask=mask) == "gemms", mask
        assert form("bf16", FFN_TEXT, VE, big, mask=mask) == "gemms", mask
    assert form("bf16", FFN_ESTIMATOR, VE, big, mask=0) == "gemms"
    assert form("bf16", FFN_ESTIMATOR, VE, big, mask=2) == "k4"
    assert form("bf16", FFN_ESTIMATOR, VE, big, mask=2, packed=False) == "k4"
    assert form("bf16", FFN_VOCODER, VO, big, mask=15) == "k4"
    assert form("bf16", FFN_ESTIMATOR, VE, big, mask=15) == "k4split4"
    assert form("bf16", FFN_ESTIMATOR, VE, big, mask=15, packed=False) == "k4"
    assert form("bf16", FFN_TEXT, VE, big, mask=15) == "k4"
    assert form("bf16", FFN_TEXT, VE, big, mask=8) == "gemms"


def test_fp32_engines_take_two_gemms():
    for stage, shape in ((FFN_VOCODER, VO), (FFN_ESTIMATOR, VE), (FFN_TEXT, VE)):
        for M in (1, 20000, 100000):
            assert form("f32", stage, shape, M, mask=15, min_rows=1) == "gemms", (stage, M)


def test_offset_bound():
    # M * C * 2 < 2^31 - 1 (the kernels' 32-bit buffer offsets): C = 384 fits 2796202 rows, C = 512 2097151
    assert form("bf16", FFN_ESTIMATOR, VE, 2796202) == "k4split4"
    assert form("bf16", FFN_ESTIMATOR, VE, 2796203) == "gemms nt"
    assert form("bf16", FFN_VOCODER, VO, 2097151) == "k4"
    assert form("bf16", FFN_VOCODER, VO, 2097152) == "gemms nt"


def test_nt_boundary():
    # two GEMMs store a hidden activation of M * I * 2 bytes > 128e6 non-temporally (16-bit engines with the hints on)
    assert form("bf16", FFN_VOCODER, VO, 31250, mask=0) == "gemms"        # 128 000 000 bytes
    assert form("bf16", FFN_VOCODER, VO, 31251, mask=0) == "gemms nt"
    assert form("f16", FFN_TEXT, VE, 41667) == "gemms nt" and form("f16", FFN_TEXT, VE, 41666) == "gemms"
    assert form("bf16", FFN_VOCODER, VO, 31251, mask=0, nt_hints=False) == "gemms"
    assert form("f32", FFN_VOCODER, VO, 100000) == "gemms"


def test_invalid_arguments():
    for kw in ({"stage": 3}, {"stage": 8}, {"M": 0}, {"k": 0}, {"max_dil": 0}):
        args = {"dtype": "bf16", "stage": FFN_VOCODER, "C": 512, "I": 2048, "M": 100}
        args.update(kw)
        with pytest.raises(binding.StnError):
            binding.ffn_form(**args)
