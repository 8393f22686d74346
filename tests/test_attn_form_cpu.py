"""The attention launchers' choice of form (attn_form in csrc/kernels_attn.hip, xattn_hs_form in csrc/kernels_xattn_hs.hip, reported by
stn_dbg_attn_form without a device), pinned on both sides of every threshold of their heuristics.  tests/test_gpu_attention_forms.py
checks each form's results; this file keeps a shape from drifting to another form unnoticed."""
import pytest

from supertonic_amd import binding

MIS_Q, MIS_K, MIS_V = 1, 2, 4


def form(dtype, B, Lq, Lk, H, dh, **kw):
    return binding.attn_form(dtype, B, Lq, Lk, H, dh, **kw)


def hs(dtype, B, L, Lk, H=4, dh=96, ldk=3072):
    return binding.attn_form(dtype, B, L, Lk, H, dh, ldk=ldk, kind=1)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_mfma_head_dims_and_key_chunks(dtype):
    for dh in (32, 64, 96):
        assert form(dtype, 2, 70, 50, 4, dh) == f"mfma<{dh},{dtype}> kc64 nch1"
    for dh in (8, 16, 40, 48, 56, 80, 88):
        assert form(dtype, 2, 70, 50, 4, dh) == f"scalar<{dtype},TPR32>"
    # kc = Lk rounded up to 32, at most 128; nch = ceil(Lk / kc)
    for Lk, kc, nch in [(1, 32, 1), (32, 32, 1), (33, 64, 1), (64, 64, 1), (65, 96, 1), (96, 96, 1), (97, 128, 1), (128, 128, 1),
                        (129, 128, 2), (256, 128, 2), (257, 128, 3), (311, 128, 3), (385, 128, 4)]:
        assert form(dtype, 2, 70, Lk, 4, 64) == f"mfma<64,{dtype}> kc{kc} nch{nch}", Lk


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_mfma_strides_alignment_and_size(dtype):
    C = 4 * 64
    mf = f"mfma<64,{dtype}> kc64 nch1"
    sc = f"scalar<{dtype},TPR32>"
    # ld % 8 == 0 for q and for k / v (the engine's 3C fused QKV and nb*2C K/V rows qualify)
    assert form(dtype, 2, 70, 50, 4, 64, ldq=3 * C, ldk=3 * C) == mf
    assert form(dtype, 2, 70, 50, 4, 64, ldq=C + 8, ldk=8 * C) == mf
    assert form(dtype, 2, 70, 50, 4, 64, ldq=C + 4) == sc and form(dtype, 2, 70, 50, 4, 64, ldq=C + 1) == sc
    assert form(dtype, 2, 70, 50, 4, 64, ldk=C + 4) == sc
    # 16-byte aligned q, k and v
    for bit in (MIS_Q, MIS_K, MIS_V):
        assert form(dtype, 2, 70, 50, 4, 64, misaligned=bit) == sc, bit
    # 32-bit buffer offsets: B*Lq*ldq*2 and B*Lk*ldk*2 below 2^31 - 1 (ld = 256: 2^22 - 1 rows of 512 bytes fit, 2^22 do not)
    n = (0x7FFFFFFF // (2 * C))  # 4194303
    assert form(dtype, 1, n, 50, 4, 64) == mf
    assert form(dtype, 1, n + 1, 50, 4, 64) == f"scalar<{dtype},TPR8>"
    assert form(dtype, 1, 70, n, 4, 64) == f"mfma<64,{dtype}> kc128 nch{(n + 127) // 128}"
    assert form(dtype, 1, 70, n + 1, 4, 64) == sc
    assert form(dtype, 2, 70, n // 2, 4, 64).startswith("mfma") and form(dtype, 2, 70, n // 2 + 1, 4, 64) == sc


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_scalar_threads_per_row(dtype):
    suffix = " vec" if dtype == "f32" else ""
    dh = 48  # no MFMA form at this head dim
    # TPR = 32 while ceil(Lq / 32) * H * B < 96 workgroups of 32 query rows, else 8
    assert form(dtype, 2, 352, 50, 4, dh) == f"scalar<{dtype},TPR32>{suffix}"  # 11 * 4 * 2 = 88
    assert form(dtype, 2, 353, 50, 4, dh) == f"scalar<{dtype},TPR8>{suffix}"   # 12 * 4 * 2 = 96
    assert form(dtype, 2, 384, 50, 4, dh) == f"scalar<{dtype},TPR8>{suffix}"
    assert form(dtype, 95, 1, 50, 1, dh) == f"scalar<{dtype},TPR32>{suffix}"
    assert form(dtype, 96, 1, 50, 1, dh) == f"scalar<{dtype},TPR8>{suffix}"
    assert form(dtype, 8, 100, 50, 4, dh) == f"scalar<{dtype},TPR8>{suffix}"   # 4 * 4 * 8 = 128
    assert form(dtype, 2, 7, 11, 2, dh) == f"scalar<{dtype},TPR32>{suffix}"


def test_f32_staging():
    C = 4 * 32
    # fp32 never takes the MFMA kernel; each operand is staged with 16-byte loads when its ld % 4 == 0 and its pointer is aligned
    assert form("f32", 2, 70, 50, 4, 32) == "scalar<f32,TPR32> vec"
    assert form("f32", 2, 70, 50, 4, 32, ldq=C + 4, ldk=3 * C) == "scalar<f32,TPR32> vec"
    assert form("f32", 2, 70, 50, 4, 32, ldq=C + 2) == "scalar<f32,TPR32> vec kv"
    assert form("f32", 2, 70, 50, 4, 32, ldk=C + 1) == "scalar<f32,TPR32> vec q"
    assert form("f32", 2, 70, 50, 4, 32, ldq=C + 3, ldk=C + 6) == "scalar<f32,TPR32> elem"
    assert form("f32", 2, 70, 50, 4, 32, misaligned=MIS_Q) == "scalar<f32,TPR32> vec kv"
    assert form("f32", 2, 70, 50, 4, 32, misaligned=MIS_K) == "scalar<f32,TPR32> vec qv"
    assert form("f32", 2, 70, 50, 4, 32, misaligned=MIS_V) == "scalar<f32,TPR32> vec qk"
    assert form("f32", 2, 70, 50, 4, 32, misaligned=MIS_Q | MIS_K | MIS_V) == "scalar<f32,TPR32> elem"
    assert form("f32", 8, 100, 50, 4, 96, ldk=3 * 4 * 96 + 1) == "scalar<f32,TPR8> vec q"


def test_unsupported_head_dims_are_refused():
    for dh in (0, 4, 12, 100, 104, 128):
        with pytest.raises(binding.StnError):
            form("bf16", 2, 70, 50, 4, dh)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_head_split_supported_shapes(dtype):
    ok = f"xattn_hs<{dtype},U1> kc64"
    assert hs(dtype, 2, 70, 50) == ok
    # C = 384 in 4 heads of 96 only
    for H, dh in [(4, 88), (8, 48), (2, 96), (4, 104)]:
        with pytest.raises(binding.StnError):
            hs(dtype, 2, 70, 50, H=H, dh=dh)
    # 1 <= L <= 256, 1 <= Lk <= 128, ldk % 8 == 0
    assert hs(dtype, 2, 256, 50) == ok and hs(dtype, 2, 1, 50) == ok
    with pytest.raises(binding.StnError):
        hs(dtype, 2, 257, 50)
    assert hs(dtype, 2, 70, 128) == f"xattn_hs<{dtype},U1> kc128"
    with pytest.raises(binding.StnError):
        hs(dtype, 2, 70, 129)
    assert hs(dtype, 2, 70, 50, ldk=768 + 8) == ok
    for ldk in (768 + 4, 3071):
        with pytest.raises(binding.StnError):
            hs(dtype, 2, 70, 50, ldk=ldk)
    with pytest.raises(binding.StnError):
        hs("f32", 2, 70, 50)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_head_split_group(dtype):
    # two utterances per workgroup once one per workgroup needs more than 256 workgroups (B * 4 > 256) ...
    assert hs(dtype, 64, 100, 50) == f"xattn_hs<{dtype},U1> kc64"
    assert hs(dtype, 65, 100, 50) == f"xattn_hs<{dtype},U2> kc64"
    assert hs(dtype, 1024, 100, 50) == f"xattn_hs<{dtype},U2> kc64"
    # ... if a pair's tiles fit the two a wave can own (L <= 128) ...
    assert hs(dtype, 65, 128, 50) == f"xattn_hs<{dtype},U2> kc64"
    assert hs(dtype, 65, 129, 50) == f"xattn_hs<{dtype},U1> kc64"
    # ... and two key slots fit beside Wo_h in LDS (kc <= 96)
    assert hs(dtype, 65, 100, 96) == f"xattn_hs<{dtype},U2> kc96"
    assert hs(dtype, 65, 100, 97) == f"xattn_hs<{dtype},U1> kc128"
    # kc = Lk rounded up to 32
    for Lk, kc in [(1, 32), (31, 32), (32, 32), (33, 64), (50, 64), (64, 64), (65, 96), (127, 128), (128, 128)]:
        assert hs(dtype, 3, 40, Lk) == f"xattn_hs<{dtype},U1> kc{kc}", Lk
