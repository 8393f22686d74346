"""dwconv_ln_form (csrc/kernels_dwconv_ln.hip), the one decision launch_dwconv_ln executes, on both sides of every threshold — through
stn_dbg_dwconv_ln_form, which needs no device.  tests/test_gpu_dwconv_ln_forms.py asserts the same strings before it compares values, so a
threshold that moves fails here first and there second.

The forms the production launches take (test_production_shapes; B*L is the PADDED product of the call, also for packed rows):
  * bench config (128 utterances of 10 words, speed 1.05, bf16, packed rows): vector estimator C = 384, k = 5, B*L = 128 x ~60 latent
    frames -> v3<5,2>; vocoder C = 512, k = 7, B*T = 6 B*L >= 32768 -> v3occ4<7,4>; text encoder (C = 256) and duration predictor
    (C = 128), k = 5, 128 x 32..127 tokens -> v3<5,2>.
  * a single utterance (workload.C1_SENTENCE), packed rows: estimator 1 x 49 frames -> v3<5,2> (the "below 1024 packed" branch); vocoder
    1 x 294 frames -> v3occ4<7,4> (bf16) / v3<7,4> (IEEE half); text stages -> v3<5,2>.  An fp32 engine runs its vocoder on padded rows:
    v2<7>."""
import numpy as np
import pytest

from supertonic_amd import binding, workload
from supertonic_amd.arch import default_arch

DTYPES = ("f32", "bf16", "f16")


def form(dt, M, C, k, packed=False, B=1):
    assert M % B == 0
    return binding.dwconv_ln_form(dt, B, M // B, C, k, packed)


def v3_74(dt):
    return "v3<7,4>" if dt == "f16" else "v3occ4<7,4>"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", (4, 384, 512))
def test_thresholds_on_rows(dt, C):
    # packed, k = 5: combs of 2 below 1024 rows, of 4 from there
    assert form(dt, 1023, C, 5, True) == "v3<5,2>"
    assert form(dt, 1024, C, 5, True) == "v3<5,4>"
    assert form(dt, 4095, C, 5, True) == "v3<5,4>"
    # padded below 4096 rows: v2, whatever k
    for M in (1, 1023, 1024, 4095):
        assert form(dt, M, C, 5) == "v2<5>" and form(dt, M, C, 7) == "v2<7>"
    # from 4096 rows the layout no longer matters
    for packed in (False, True):
        assert form(dt, 4096, C, 5, packed) == "v3<5,2>"
        assert form(dt, 16383, C, 5, packed) == "v3<5,2>"
        assert form(dt, 16384, C, 5, packed) == "v3<5,4>"
        assert form(dt, 32767, C, 5, packed) == "v3<5,4>"
        assert form(dt, 32768, C, 5, packed) == "v3<5,8>"
        for M in (4096, 16383, 16384, 32767, 32768):
            assert form(dt, M, C, 7, packed) == v3_74(dt)
    # packed k = 7: combs of 4 at any row count
    for M in (1, 1023, 1024, 4095):
        assert form(dt, M, C, 7, True) == v3_74(dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_rows_are_the_product_of_batch_and_length(dt):
    assert form(dt, 4096, 384, 5, B=64) == "v3<5,2>" and form(dt, 4032, 384, 5, B=64) == "v2<5>"
    assert form(dt, 32768, 512, 5, B=128) == "v3<5,8>" and form(dt, 32768 - 128, 512, 5, B=128) == "v3<5,4>"
    assert form(dt, 1024, 384, 5, True, B=8) == "v3<5,4>" and form(dt, 1016, 384, 5, True, B=8) == "v3<5,2>"


@pytest.mark.parametrize("dt", DTYPES)
def test_generic_and_refusals(dt):
    for M in (100, 4096, 40000):
        for k in (3, 9):
            assert form(dt, M, 384, k) == "generic"
            with pytest.raises(binding.StnError):
                form(dt, M, 384, k, True)
        for C in (516, 1024):
            for k in (5, 7):
                assert form(dt, M, C, k) == "generic"
                with pytest.raises(binding.StnError):
                    form(dt, M, C, k, True)
        for packed in (False, True):
            for C in (1028, 6, 510, 1):
                with pytest.raises(binding.StnError):
                    form(dt, M, C, 5, packed)


def test_bad_arguments_are_error_codes():
    L = binding.load()
    assert L.stn_dbg_dwconv_ln_form(1, 0, 10, 384, 5, 0, None, 0) < 0
    assert L.stn_dbg_dwconv_ln_form(1, 1, 0, 384, 5, 0, None, 0) < 0
    assert L.stn_dbg_dwconv_ln_form(1, 1, 10, 384, 4, 0, None, 0) < 0
    assert L.stn_dbg_dwconv_ln_form(7, 1, 10, 384, 5, 0, None, 0) < 0
    assert L.stn_dbg_dwconv_ln_form(1, 1, 10, 384, 5, 0, None, 0) == len("v2<5>")  # the length without a buffer


def latent_geometry(a, dur):
    """Engine::latent_geometry (engine_batch.cpp): float32 products, truncation"""
    cs = a.base_chunk_size * a.chunk_compress_factor
    dur = np.asarray(dur, np.float32)
    L = int((np.float32(dur.max()) * np.float32(a.sample_rate) + np.float32(cs) - np.float32(1.0)) / np.float32(cs))
    llen = [int((int(np.float32(d) * np.float32(a.sample_rate)) + cs - 1) // cs) for d in dur]
    return L, llen


def test_production_shapes():
    a = default_arch()
    ccf = a.chunk_compress_factor
    # the bench: 128 utterances of 10 words at speed 1.05 (bench.py's defaults), packed rows, 16-bit engines
    texts = workload.utterances(128, 10)
    L, llen = latent_geometry(a, workload.forced_durations(texts) / np.float32(1.05))
    assert 4096 <= 128 * L < 16384 and 128 * L * ccf >= 32768 and max(llen) == L
    for dt in ("bf16", "f16"):
        assert binding.dwconv_ln_form(dt, 128, L, a.ve_dim, a.ve_kernel, True) == "v3<5,2>"
        assert binding.dwconv_ln_form(dt, 128, L * ccf, a.vo_dim, a.vo_kernel, True) == v3_74(dt)
        for Lt in (32, len(max(texts, key=len)), 127):  # token rows of the longest utterance: well inside the bracket
            assert binding.dwconv_ln_form(dt, 128, Lt, a.te_dim, a.te_kernel, True) == "v3<5,2>"
            assert binding.dwconv_ln_form(dt, 128, Lt, a.dp_dim, a.dp_kernel, True) == "v3<5,2>"
    assert 32 <= len(max(texts, key=len)) <= 127
    # a single utterance
    L1, l1 = latent_geometry(a, workload.forced_durations([workload.C1_SENTENCE]) / np.float32(1.05))
    assert L1 == l1[0] == 49
    for dt in ("bf16", "f16"):
        assert binding.dwconv_ln_form(dt, 1, L1, a.ve_dim, a.ve_kernel, True) == "v3<5,2>"
        assert binding.dwconv_ln_form(dt, 1, L1 * ccf, a.vo_dim, a.vo_kernel, True) == v3_74(dt)
        assert binding.dwconv_ln_form(dt, 1, len(workload.C1_SENTENCE), a.te_dim, a.te_kernel, True) == "v3<5,2>"
    assert binding.dwconv_ln_form("f32", 1, L1 * ccf, a.vo_dim, a.vo_kernel, False) == "v2<7>"  # (fp32 vocoder: padded rows)
