"""The ConvNeXt pointwise pair's choice of form (ffn_form in csrc/kernels_ffn.hip, reported by stn_dbg_ffn_form without a device), pinned on
both sides of every threshold: two GEMMs, K4 or K4-split.  tests/test_gpu_ffn.py checks each form's results; this file keeps a shape from
drifting to another form unnoticed."""
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
