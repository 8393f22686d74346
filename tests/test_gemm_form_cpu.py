"""The GEMM launcher's choice of form (gemm_form in csrc/kernels_gemm.hip, reported by stn_dbg_gemm_form without a device), pinned on
both sides of every threshold of its heuristic.  tests/test_gpu_gemm_epilogues.py checks each form's results; this file keeps a shape
from drifting to another form unnoticed."""
import pytest

from supertonic_amd import binding
from supertonic_amd.binding import EPI_RESID, EPI_STORE, EPI_STORE_T

T8 = "tiled<128,128,2,4,4,64,2> cfg8"
T12 = "tiled<64,64,2,2,4,64,2> cfg12"
T11 = "tiled<256,256,4,4,4,32,2> cfg11"
T18 = "tiled<192,256,3,4,4,32,2> cfg18"
T1 = "tiled<256,256,2,4,4,32,2> cfg1"
T17 = "tiled<256,128,4,2,3,32,2> cfg17"
F64 = "tiled<64,64,2,2,4,32,4>"
F128 = "tiled<128,128,2,2,3,32,4>"


def form(dtype, M, N, K, **kw):
    return binding.gemm_form(dtype, M, N, K, **kw)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_tile_thresholds(dtype):
    K = 384
    # N >= 256 and t256 = ceil(M/256) * ceil(N/256) >= 160 selects the big tiles; at N = 256, t256 = ceil(M / 256)
    assert form(dtype, 159 * 256, 256, K) == T8 + " slab"          # t256 = 159
    assert form(dtype, 159 * 256 + 1, 256, K) == T18 + " slab"      # t256 = 160, t192 = 213
    assert form(dtype, 300, 248, K) == T8 + " slab" and form(dtype, 320 * 256, 248, K) == T8 + " slab"  # N < 256: never a big tile
    # config 18 while t192 = ceil(M/192) * ceil(N/256) <= 256 (and t256 < 208, implied: t256 <= t192)
    assert form(dtype, 256 * 192, 256, K) == T18 + " slab"          # t192 = 256
    assert form(dtype, 256 * 192 + 1, 256, K) == T11 + " slab"      # t192 = 257
    assert form(dtype, 207 * 256, 256, K) == T11 + " slab" and form(dtype, 208 * 256, 256, K) == T11 + " slab"
    # config 11 below t256 = 512
    assert form(dtype, 511 * 256, 256, K) == T11 + " slab"
    assert form(dtype, 511 * 256 + 1, 256, K) == T1 + " slab"       # t256 = 512
    # config 17 from t256 = 1024 on, for K <= 512 only
    assert form(dtype, 1023 * 256, 256, 512) == T1 + " slab"
    assert form(dtype, 1024 * 256, 256, 512) == T17 + " slab"
    assert form(dtype, 1024 * 256, 256, 576) == T1 + " slab"
    # small launches: 64x64 tiles up to M = 64, 128x128 beyond
    assert form(dtype, 64, 384, K) == T12 + " slab" and form(dtype, 1, 384, K) == T12 + " slab"
    assert form(dtype, 65, 384, K) == T8 + " slab"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_k_n_ldo_and_alignment_forms(dtype):
    # K % 64 == 0: tiled; K % 32 == 0 only: the LDS-DMA ring kernel; otherwise the register-staged kernel
    assert form(dtype, 300, 384, 128) == T8 + " slab"
    assert form(dtype, 300, 384, 96) == "ring_vec slab"
    assert form(dtype, 300, 384, 32) == "ring_vec slab"
    assert form(dtype, 300, 384, 72) == "reg lane" and form(dtype, 300, 384, 8) == "reg lane"
    # a big tile needs K % 32 only
    assert form(dtype, 9000, 1536, 96) == T11 + " slab"
    # the vector epilogues need N % 8 == 0 and ldo % 8 == 0
    assert form(dtype, 300, 136, 384) == T8 + " slab" and form(dtype, 300, 8, 384) == T8 + " slab"
    assert form(dtype, 300, 132, 384) == "ring lane"
    assert form(dtype, 300, 384, 384, ldo=388) == "ring lane"
    assert form(dtype, 300, 384, 384, ldo=392) == T8 + " slab"
    assert form(dtype, 300, 384, 96, ldo=388) == "ring lane"
    assert form(dtype, 300, 132, 72) == "reg lane"
    # operands the launcher refuses: K not a multiple of 8
    with pytest.raises(binding.StnError):
        form(dtype, 300, 384, 36)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_transposed_image_store(dtype):
    """the transposed-image epilogue: 16-bit stores of configurations 8, 11, 12 and 18 without a row mask; the tr override either way"""
    for M, N, base, tr in ((300, 384, T8, True), (49, 384, T12, True), (9000, 1536, T11, True), (7436, 1536, T18, True),
                           (22000, 1536, T1, False), (44000, 1536, T17, False)):
        want = " tr" if tr else " slab"
        assert form(dtype, M, N, 384, out_dtype=dtype) == base + want, (M, N)
        assert form(dtype, M, N, 384) == base + " slab"                                 # fp32 output
        assert form(dtype, M, N, 384, out_dtype=dtype, masked=True) == base + " slab"   # row mask: the slab path
        assert form(dtype, M, N, 384, out_dtype=dtype, tr=1) == base + " tr"
        assert form(dtype, M, N, 384, out_dtype=dtype, tr=0) == base + " slab"
        assert form(dtype, M, N, 384, out_dtype=dtype, masked=True, tr=1) == base + " slab"
        assert form(dtype, M, N, 384, mode=EPI_RESID, tr=1) == base + " slab"
    # forms without a tile: the override changes nothing
    assert form(dtype, 300, 384, 96, out_dtype=dtype, tr=1) == "ring_vec slab"
    assert form(dtype, 300, 384, 72, out_dtype=dtype, tr=1) == "reg lane"


def test_f32_forms_and_split_k():
    # exact-fp32 tiles: 64x64 up to M = 64 or below 160 tiles of 128x128, else 128x128; K % 32 != 0 or N % 8 != 0: gemm_f32_kernel
    assert form("f32", 600, 384, 256) == F64 + " slab"
    assert form("f32", 53 * 128, 384, 256) == F64 + " slab"          # 159 tiles of 128x128
    assert form("f32", 53 * 128 + 1, 384, 256) == F128 + " slab"      # 162
    assert form("f32", 2600, 1024, 512) == F128 + " slab"
    assert form("f32", 64, 30000, 256) == F64 + " slab"
    assert form("f32", 257, 130, 72) == "reg lane" and form("f32", 600, 130, 256) == "reg lane"
    assert form("f32", 600, 384, 36) == "reg lane"
    # deterministic split-K: fp32, M <= 512, K >= 384, K % 32 == 0, N % 8 == 0, ldo % 4 == 0, a store or residual epilogue
    assert form("f32", 512, 384, 384) == "splitk3+" + F64 + " slab"
    assert form("f32", 513, 384, 384) == F64 + " slab"
    assert form("f32", 300, 384, 352) == F64 + " slab"
    assert form("f32", 300, 384, 384) == "splitk3+" + F64 + " slab"
    assert form("f32", 49, 384, 1536) == "splitk8+" + F64 + " slab"
    assert form("f32", 64, 256, 1152) == "splitk6+" + F64 + " slab"
    assert form("f32", 300, 384, 384, mode=EPI_RESID) == "splitk3+" + F64 + " slab"
    assert form("f32", 300, 384, 384, ldo=390) == "reg lane"         # ldo % 4 != 0: neither split nor vector epilogue
    assert form("f32", 300, 384, 384, ldo=388) == "splitk3+" + F64 + " slab"  # ldo % 4 == 0: splits (the partials have their own stride)
    assert form("f32", 300, 384, 384, mode=EPI_STORE_T) == "reg lane"
    # the 16-bit engines never split (a row's bits must not depend on the launch's row count)
    assert form("bf16", 49, 384, 1536) == T12 + " slab"


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_transposing_store(dtype):
    want = "reg lane" if dtype == "f32" else "ring lane"
    assert form(dtype, 185, 136, 256, mode=EPI_STORE_T) == want
    assert form(dtype, 185, 136, 72, mode=EPI_STORE_T) == "reg lane"
    assert form(dtype, 185, 136, 256, mode=EPI_STORE) != want
