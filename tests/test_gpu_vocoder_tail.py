"""The dense vocoder trimmed to ONE receptive field (the "tail form"): every utterance is computed on its first min(len*ccf + rf, T) frames
and the convolutions read the frames beyond from per-layer tail tables cached at load, so every computed row is exact.

1. The kernel (dwconv_ln_v3_body<..., TAIL = true> through stn_op_dwconv_ln_tail): bit for bit against the existing kernel
   (stn_op_dwconv_ln_ex, packed) on a buffer in which the halo rows are materialised as real rows, and against the float64 statement of
   tests/test_gpu_dwconv_ln_forms.py at that file's bound for 16-bit stores (|d| <= ulp/2 + F32_REL rms(ref), F32_REL = 6e-6); rows outside
   the written ones keep their sentinels.  Measured on an MI355X: max(|d| - ulp/2)/rms = 1.1e-7 (bf16) and 2.3e-7 (f16) over every case.
2. The engine: the default layout against set_packed_rows(False), whole [B, W] arrays equal, eager, capture and replay, on batches the
   len*ccf + 2 rf form leaves dense; the row counts through eng.vo_rows.  Paddings of exactly rf = 57 and of 56 frames need a latent that
   is not compressed sixfold (the default stack's paddings are multiples of 6): those two batches run the default stack with
   chunk_compress_factor = 1 (latent_dim = 144: the same 144 latent channels), whose receptive field is the same 57 frames."""
import numpy as np
import pytest

from supertonic_amd import binding, host
from supertonic_amd.arch import default_arch
from gpu_util import make_inputs
from test_gpu_dwconv_ln_forms import F32_REL, SENTINEL, SENTINEL_BITS, Params, bits, ref64, ulp

pytestmark = pytest.mark.gpu

C, K, RF = 512, 7, 57
LENS = (1, 2, 3, 7, 12, 13, 29)
PADS = (0, 1, 3, 11, 12, 13, 57, 58, 200)


@pytest.fixture(scope="module")
def op_eng():
    return binding.Engine(0, "bf16")


def materialise(x_seqs, lens, tail, T, halo):
    """[B, max(len) + halo, C]: a sequence's own rows, then `halo` rows holding what the tail-reading kernel reads there."""
    B, Lm = len(lens), max(lens) + halo
    buf = np.zeros((B, Lm, tail.shape[1]), np.float32)
    for b, n in enumerate(lens):
        buf[b, :n] = x_seqs[b]
        for tt in range(n, n + halo):
            if tt < T:
                buf[b, tt] = tail[min(T - 1 - tt, tail.shape[0] - 1)]
    return buf


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("dil", [1, 2, 4])
def test_tail_kernel_equals_materialised_halo(op_eng, fmt, dil):
    rng = np.random.default_rng(100 + dil)
    p = Params(C, K, 7 + dil)
    tail = rng.standard_normal((RF + 1, C)).astype(np.float32)
    halo = (K - 1) // 2 * dil
    worst = 0.0
    for T in sorted({n + d for n in LENS for d in PADS}):
        lens = [n for n in LENS if n <= T]  # every length whose row fits T, mixed in one call; T - len covers PADS for each length over the loop
        L = max(lens)
        xs = [rng.standard_normal((n, C)).astype(np.float32) for n in lens]
        rows = sum(lens)
        x_packed = np.concatenate(xs)
        out0 = np.full((rows + 3, C), SENTINEL, np.float32)
        got, form = op_eng.op_dwconv_ln_tail(x_packed, p.w, p.bias, p.g, p.bt, dil, out0, L, lens, tail, T, dtype=fmt)
        assert form == ("v3<7,4>" if fmt == "f16" else "v3occ4<7,4>"), form
        assert np.all(bits(got[rows:]) == SENTINEL_BITS), ("rows past the packed ones were written", T)
        # the existing kernel on materialised halo rows
        buf = materialise(xs, lens, tail, T, halo)
        mlens = [n + halo for n in lens]
        m_packed = np.concatenate([buf[b, :mlens[b]] for b in range(len(lens))])
        ref_out, ref_form = op_eng.op_dwconv_ln_ex(m_packed, p.w, p.bias, p.g, p.bt, dil, np.zeros((sum(mlens), C), np.float32), len(lens), L + halo,
                                                   seqlen=mlens, packed=True, dtype=fmt)
        assert ref_form == form, (ref_form, form)
        ref = ref64(buf, p.w, p.bias, p.g, p.bt, dil, mlens)
        o = om = 0
        for b, n in enumerate(lens):
            np.testing.assert_array_equal(bits(got[o:o + n]), bits(ref_out[om:om + n]), err_msg=f"T={T} len={n} dil={dil}")
            r64 = ref[b, :n]
            rms = np.sqrt(np.mean(r64 ** 2)) + 1e-30
            need = float(np.max((np.abs(got[o:o + n].astype(np.float64) - r64) - 0.5 * ulp(r64, fmt)) / rms))
            worst = max(worst, need)
            assert need <= F32_REL, (T, n, dil, need)
            o += n
            om += mlens[b]
    print(f"tail kernel {fmt} dil={dil}: max(|d| - ulp/2)/rms = {worst:.3e}")


def arch_ccf1():
    a = default_arch()
    a.chunk_compress_factor, a.latent_dim = 1, 144
    return a


_ENGINES = {}


def engine(arch_name, dtype):
    key = (arch_name, dtype)
    if key not in _ENGINES:
        eng = binding.Engine(0, dtype)
        eng.load_synthetic(default_arch() if arch_name == "default" else arch_ccf1(), 7)
        eng.set_fused_ffn(1)  # the same estimator kernels in both layouts (K4-split exists on packed rows only)
        _ENGINES[key] = eng
    return _ENGINES[key]


def durations(a, frames):
    """durations that give exactly these latent lengths (half a latent frame below each boundary)"""
    chunk = a.base_chunk_size * a.chunk_compress_factor
    return np.array([(n - 0.5) * chunk / a.sample_rate for n in frames], np.float32)


def run_layouts(eng, a, lat_lens, seed):
    B = len(lat_lens)
    ids, mask, sttl, sdp = make_inputs(a, B, 12, np.array([12] + [5 + (i % 7) for i in range(B - 1)]), seed=seed)
    durs = durations(a, lat_lens)
    outs = {}
    for packed in (False, True):
        eng.set_packed_rows(packed)
        for _ in range(3):  # eager, capture, replay
            w, d = eng.synthesize(ids, mask, sttl, sdp, 2, 1.0, duration_override=durs, noise_seed=4)
            if packed in outs:
                np.testing.assert_array_equal(w, outs[packed][0])
            outs[packed] = (w, eng.vo_rows)
        lens = host.latent_geometry(d, a.sample_rate, a.base_chunk_size, a.chunk_compress_factor, a.latent_dim)[2]
        assert list(lens) == list(lat_lens), lens
    eng.set_packed_rows(True)
    return outs


CASES = {
    # paddings of 60 and 108 frames, all below 2 x 57; the 20-frame row's extent 177 has taps beyond T = 180
    "default_60_108": ("default", [30, 20, 12, 12, 12, 12]),
    # chunk_compress_factor = 1: a padding of exactly 57 frames (extent == T, no tap reads a tail) and four of 110
    "pad_57": ("ccf1", [180, 123, 70, 70, 70, 70]),
    # a padding of 56 frames: len + 57 > T, the extent is clamped to T
    "pad_56": ("ccf1", [180, 124, 70, 70, 70, 70]),
}


@pytest.mark.parametrize("dtype16", ["bf16", "f16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_tail_form_is_bit_identical_to_dense(case, dtype16):
    arch_name, lat_lens = CASES[case]
    a = default_arch() if arch_name == "default" else arch_ccf1()
    ccf, T = a.chunk_compress_factor, max(lat_lens) * a.chunk_compress_factor
    B = len(lat_lens)
    assert not any(n * ccf + 2 * RF <= T for n in lat_lens)  # the len*ccf + 2 rf form leaves this batch dense
    want = sum(min(n * ccf + RF, T) for n in lat_lens)
    assert want * 10 <= B * T * 9  # ... and the tail form clears the bar
    outs = run_layouts(engine(arch_name, dtype16), a, lat_lens, seed=31)
    np.testing.assert_array_equal(outs[True][0], outs[False][0])
    assert outs[False][1] == B * T, outs[False][1]
    assert outs[True][1] == want, (outs[True][1], want)


@pytest.mark.parametrize("dtype16", ["bf16", "f16"])
def test_tail_form_below_the_bar_stays_dense(dtype16):
    a = default_arch()
    lat_lens = [30, 30, 30, 30, 30, 12]  # extents 5 x 180 + 129 = 1029 of 1080 frames: the one short row removes 4.7 %, less than the bar
    T, B = 180, len(lat_lens)
    want = sum(min(n * 6 + RF, T) for n in lat_lens)
    assert want * 10 > B * T * 9
    outs = run_layouts(engine("default", dtype16), a, lat_lens, seed=32)
    np.testing.assert_array_equal(outs[True][0], outs[False][0])
    assert outs[True][1] == B * T and outs[False][1] == B * T, (outs[True][1], outs[False][1])


def test_tail_form_not_on_fp32_engines():
    a = default_arch()
    lat_lens = CASES["default_60_108"][1]
    outs = run_layouts(engine("default", "f32"), a, lat_lens, seed=31)
    assert outs[True][1] == len(lat_lens) * 180 and outs[False][1] == len(lat_lens) * 180, (outs[True][1], outs[False][1])
