"""fold_dwconv_ln_form (csrc/kernels_fold.hip), the one decision launch_fold_dwconv_ln executes — kernel instantiation, run length, workgroups per
sequence — and fold_dwconv_ln_supported, the gate behind it, on both sides of every limit, through stn_dbg_fold_dwconv_ln_form, which needs no
device.  tests/test_gpu_fold_dwconv_ln_forms.py asserts the same strings before it compares values, and takes its reference (fold_ref,
conv_ln64) from here.

Gate agreement: the one place where engine code leaves an update pending for this kernel is ffn_form (csrc/kernels_ffn.hip), which returns
K4-split only where fold_dwconv_ln_supported(C, k, max_dil) holds; the head-split cross-attention (Engine::ve_step_dev) leaves its partial
sums pending only inside a stage whose blocks are K4-split, i.e. behind the same decision.  ffn_form is reachable from the host
(stn_dbg_ffn_form), so test_pending_updates_agree_with_the_gate pins it.

The bound the GPU file puts on y (F32_REL rms(ref) beside half an ulp of the store) is checked here to belong to fp32 arithmetic: a float32
numpy restatement of conv + LayerNorm in ANOTHER summation order (taps reversed, separately rounded products, pairwise mean) stays within it
of the float64 reference (test_f32_restatement_stays_within_the_bound; the GPU file asserts the same on every case's own inputs)."""
import numpy as np
import pytest

from supertonic_amd import binding, workload
from supertonic_amd.arch import default_arch
from supertonic_amd.binding import FFN_ESTIMATOR

F32_REL = 6e-6  # tests/test_gpu_dwconv_ln_forms.py
EPS = 1e-6
LDS_LIMIT = 160 * 1024
FMTS = ("bf16", "f16")


# ---- the rules, written out independently of the library ---------------------------------------------------------------------------------
def lds_bytes(C, k, dil, run=32):
    """image of run + (k-1) dil frames, a row of zeros, k taps + conv bias + LayerNorm gain and shift: fp32 rows of C"""
    return (run + (k - 1) * dil + k + 4) * C * 4


def max_dil(C, k, run=32):
    """the largest dilation whose image of `run` frames fits 160 KiB (0: none)"""
    d = 0
    while lds_bytes(C, k, d + 1, run) <= LDS_LIMIT:
        d += 1
    return d


def expect_form(fmt, B, L, C, k, dil, S, rv, run_frames=0):
    ns = 3 if C <= 384 else 4
    U = (3 if k == 5 and ns == 3 else 2) if S == 4 else 1  # the kernel comment: three rows per trip for four partial sums, two for the wider variants
    run = 8 if B * -(-L // 32) < 64 else 32
    if run == 32 and run_frames in (40, 48) and lds_bytes(C, k, dil, run_frames) <= LDS_LIMIT:
        run = run_frames
    return f"fold_dwconv_ln<{fmt},K{k},{'rv' if rv else 'norv'},ns{ns},S{S},U{U}> run {run} cps {-(-L // run)}"


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def fold_ref(x, part16, b2, gamma, rowvec, lens):
    """kernels_fold.hpp: fp32, (((p0 + p1) + p2) + ...), then (x + gamma * (sum + b2)) + rowvec[b]; part16 [S, M, C] already rounded to the format"""
    acc = part16[0].astype(np.float32)
    for s in range(1, part16.shape[0]):
        acc = (acc + part16[s]).astype(np.float32)
    xo = (x + (gamma * (acc + b2).astype(np.float32)).astype(np.float32)).astype(np.float32)
    rv = np.zeros_like(xo) if rowvec is None else rowvec[np.repeat(np.arange(len(lens)), lens)]
    return (xo + rv).astype(np.float32)


def _layernorm64(h, g, bt):
    mean = h.mean(axis=-1, keepdims=True)
    var = ((h - mean) ** 2).mean(axis=-1, keepdims=True)
    return (h - mean) / np.sqrt(var + EPS) * g + bt


def conv_ln64(xo, lens, w, bias, g, bt, dil):
    """xo [M, C] fp32 packed rows; zero-padded dilated depthwise conv inside each sequence, bias, LayerNorm (eps 1e-6): float64"""
    k = w.shape[1]
    half = (k - 1) // 2
    out = np.zeros(xo.shape, np.float64)
    r = 0
    for n in lens:
        xs = xo[r:r + n].astype(np.float64)
        h = np.tile(bias.astype(np.float64), (n, 1))
        for j in range(k):
            s = (j - half) * dil
            lo, hi = max(0, -s), min(n, n - s)
            if hi > lo:
                h[lo:hi] += w[:, j].astype(np.float64) * xs[lo + s:hi + s]
        out[r:r + n] = _layernorm64(h, g.astype(np.float64), bt.astype(np.float64))
        r += n
    return out


def _pairwise_sum32(a):
    """sum over the last axis as a float32 binary tree"""
    a = np.asarray(a, np.float32)
    n = 1 << int(np.ceil(np.log2(max(a.shape[-1], 1))))
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (n - a.shape[-1],), np.float32)], axis=-1)
    while a.shape[-1] > 1:
        a = (a[..., 0::2] + a[..., 1::2]).astype(np.float32)
    return a


def conv_ln32_alt(xo, lens, w, bias, g, bt, dil):
    """the same in float32, in another order than the kernel's: taps from last to first, products rounded before they are added, tree sums"""
    k = w.shape[1]
    half = (k - 1) // 2
    C = xo.shape[1]
    out = np.zeros(xo.shape, np.float32)
    r = 0
    for n in lens:
        xs = xo[r:r + n]
        h = np.tile(bias.astype(np.float32), (n, 1))
        for j in reversed(range(k)):
            s = (j - half) * dil
            lo, hi = max(0, -s), min(n, n - s)
            if hi > lo:
                h[lo:hi] = (h[lo:hi] + (w[:, j] * xs[lo + s:hi + s]).astype(np.float32)).astype(np.float32)
        mean = (_pairwise_sum32(h) / np.float32(C)).astype(np.float32)
        d = (h - mean).astype(np.float32)
        var = (_pairwise_sum32(d * d) / np.float32(C)).astype(np.float32)
        out[r:r + n] = (d / np.sqrt(var + np.float32(EPS), dtype=np.float32) * g + bt).astype(np.float32)
        r += n
    return out


def f32_margin(xo, lens, w, bias, g, bt, dil, ref=None):
    """max |float32 restatement - float64| / rms(float64): what fp32 arithmetic in another order costs on these inputs"""
    ref = conv_ln64(xo, lens, w, bias, g, bt, dil) if ref is None else ref
    return float(np.abs(conv_ln32_alt(xo, lens, w, bias, g, bt, dil).astype(np.float64) - ref).max() / (np.sqrt(np.mean(ref ** 2)) + 1e-30))


# ---- the gate ----------------------------------------------------------------------------------------------------------------------------------
def refused(*a, **kw):
    try:
        binding.fold_dwconv_ln_form(*a, **kw)
    except binding.StnError:
        return True
    return False


def test_gate_on_width_and_taps():
    for C in (8, 96, 384, 392, 512):
        for k in (5, 7):
            assert not refused("bf16", 4, 50, C, k, 1, 4)
    for C in (4, 12, 100, 390, 516, 520, 1024):  # C % 8, C <= 512
        assert refused("bf16", 4, 50, C, 5, 1, 4), C
    for k in (1, 3, 4, 6, 9):
        assert refused("bf16", 4, 50, 384, k, 1, 4), k
    assert refused("bf16", 4, 50, 384, 5, 0, 4) and refused("bf16", 4, 50, 384, 5, -1, 4)
    for S in (0, 1, 2, 3, 5, 16, 48):
        assert refused("bf16", 4, 50, 384, 5, 1, S), S
    assert refused("f32", 4, 50, 384, 5, 1, 4)
    assert refused("bf16", 0, 50, 384, 5, 1, 4) and refused("bf16", 4, 0, 384, 5, 1, 4)


@pytest.mark.parametrize("C,k,dmax", [(384, 5, 16), (512, 5, 9), (384, 7, 10), (512, 7, 6)])
def test_gate_on_the_largest_dilation(C, k, dmax):
    """(32 + (k-1) dil + k + 4) C 4 <= 160 KiB: 106 rows of 384 channels, 80 rows of 512"""
    assert max_dil(C, k) == dmax
    assert lds_bytes(C, k, dmax) <= LDS_LIMIT < lds_bytes(C, k, dmax + 1)
    for fmt in FMTS:
        assert binding.fold_dwconv_ln_form(fmt, 128, 64, C, k, dmax, 4) == expect_form(fmt, 128, 64, C, k, dmax, 4, True)
        assert refused(fmt, 128, 64, C, k, dmax + 1, 4)
        assert refused(fmt, 1, 8, C, k, dmax + 1, 4)  # (the gate is on the 32-frame image, whatever run the launch would take)


def test_pending_updates_agree_with_the_gate():
    """ffn_form leaves an update pending (K4-split) exactly where the fold kernel takes the stage's taps and largest dilation"""
    for fmt in FMTS:
        for k in (3, 5, 7, 9):
            for d in (1, 8, 10, 11, 16, 17, 32, 128):
                pending = binding.ffn_form(fmt, FFN_ESTIMATOR, 384, 1536, 7424, 0, True, k, d).startswith("k4split")
                assert pending == (not refused(fmt, 128, 58, 384, k, d, 4)), (fmt, k, d)


# ---- run length ----------------------------------------------------------------------------------------------------------------------------------
def run_of(form):
    return int(form.split(" run ")[1].split()[0])


def cps_of(form):
    return int(form.split(" cps ")[1])


def test_run_length_few_against_many():
    f = lambda B, L, **kw: binding.fold_dwconv_ln_form("bf16", B, L, 384, 5, 1, 4, **kw)
    for B, L in ((63, 32), (9, 200), (1, 63 * 32), (21, 96), (7, 288)):  # B * ceil(L / 32) = 63
        assert B * -(-L // 32) == 63
        assert run_of(f(B, L)) == 8 and cps_of(f(B, L)) == -(-L // 8), (B, L)
        assert run_of(f(B, L, run_frames=40)) == 8  # run_frames is honoured only where the base choice is 32
    for B, L in ((64, 32), (32, 33), (32, 64), (1, 63 * 32 + 1), (16, 97), (1024, 1)):  # ... = 64 and beyond
        assert B * -(-L // 32) >= 64
        assert run_of(f(B, L)) == 32 and cps_of(f(B, L)) == -(-L // 32), (B, L)


def test_run_frames_is_honoured_where_the_image_fits():
    f = lambda C, k, d, rf: run_of(binding.fold_dwconv_ln_form("f16", 128, 78, C, k, d, 12, run_frames=rf))
    assert (f(384, 5, 8, 0), f(384, 5, 8, 40), f(384, 5, 8, 48)) == (32, 40, 48)
    # (C, k) = (384, 5): 49 + 4 dil <= 106 rows for runs of 40, 57 + 4 dil for runs of 48
    assert max_dil(384, 5, 40) == 14 and max_dil(384, 5, 48) == 12
    assert (f(384, 5, 12, 40), f(384, 5, 12, 48)) == (40, 48)
    assert (f(384, 5, 13, 40), f(384, 5, 13, 48)) == (40, 32)   # 40 fits, 48 does not
    assert (f(384, 5, 14, 40), f(384, 5, 14, 48)) == (40, 32)
    assert (f(384, 5, 15, 40), f(384, 5, 15, 48)) == (32, 32)   # neither fits: the default
    assert (f(384, 5, 16, 40), f(384, 5, 16, 48)) == (32, 32)
    for C, k in ((384, 5), (512, 5), (384, 7), (512, 7)):
        for rf in (40, 48):
            d = max_dil(C, k, rf)
            assert d >= 1 and f(C, k, d, rf) == rf and f(C, k, d + 1, rf) == 32, (C, k, rf)
    # values that are no multiple of 8 or lie outside (32, 48] are ignored
    for rf in (-8, 1, 8, 16, 24, 31, 32, 33, 36, 39, 41, 44, 47, 49, 56, 64, 80, 1 << 20):
        assert f(384, 5, 1, rf) == 32, rf
    form = binding.fold_dwconv_ln_form("f16", 128, 78, 384, 5, 8, 12, run_frames=40)
    assert form == "fold_dwconv_ln<f16,K5,rv,ns3,S12,U1> run 40 cps 2" == expect_form("f16", 128, 78, 384, 5, 8, 12, True, 40)


# ---- instantiation -----------------------------------------------------------------------------------------------------------------------------
def test_u_and_nslot():
    for fmt in FMTS:
        for rv in (True, False):
            for C, ns in ((8, 3), (128, 3), (376, 3), (384, 3), (392, 4), (448, 4), (512, 4)):
                for k in (5, 7):
                    for S in (4, 8, 12, 24):
                        U = 1 if S > 4 else 3 if (k == 5 and ns == 3) else 2
                        got = binding.fold_dwconv_ln_form(fmt, 128, 64, C, k, 2, S, rv)
                        assert got == f"fold_dwconv_ln<{fmt},K{k},{'rv' if rv else 'norv'},ns{ns},S{S},U{U}> run 32 cps 2", got
                        assert got == expect_form(fmt, 128, 64, C, k, 2, S, rv)


def test_bad_arguments_are_error_codes():
    L = binding.load()
    assert L.stn_dbg_fold_dwconv_ln_form(1, 0, 10, 384, 5, 1, 4, 1, 0, None, 0) < 0
    assert L.stn_dbg_fold_dwconv_ln_form(0, 1, 10, 384, 5, 1, 4, 1, 0, None, 0) < 0
    assert L.stn_dbg_fold_dwconv_ln_form(7, 1, 10, 384, 5, 1, 4, 1, 0, None, 0) < 0
    assert L.stn_dbg_fold_dwconv_ln_form(1, 1, 10, 384, 5, 1, 4, 1, 0, None, 0) == len("fold_dwconv_ln<bf16,K5,rv,ns3,S4,U3> run 8 cps 2")


# ---- the shapes production launches take ---------------------------------------------------------------------------------------------------------
def latent_lengths(a, dur):
    """Engine::latent_geometry (engine_batch.cpp): float32 products, truncation"""
    cs = a.base_chunk_size * a.chunk_compress_factor
    return [int((int(np.float32(d) * np.float32(a.sample_rate)) + cs - 1) // cs) for d in np.asarray(dur, np.float32)]


def test_production_shapes():
    a = default_arch()
    C, k = a.ve_dim, a.ve_kernel
    dils = [1 << j for j in range(a.ve_dilated)]
    assert (C, k, dils) == (384, 5, [1, 2, 4, 8])
    # the bench: 128 utterances of 10 words at speed 1.05 on 256 CUs: 128 x 3 runs of <= 32 frames are two rounds, 128 x 2 runs of <= 40 one
    llen = latent_lengths(a, workload.forced_durations(workload.utterances(128, 10)) / np.float32(1.05))
    Lmax = max(llen)
    assert 64 < Lmax <= 80 and binding.fold_run_frames(llen, 256) == 40
    for fmt in FMTS:
        for L in (Lmax, -(-Lmax // 16) * 16):  # the exact longest length (injected noise) and the bucketed one
            for d in dils:
                # K4-split of 7 k rows leaves 4 partial sums with the time vector (S4, rv: U3); the head-split cross-attention 4 without (norv)
                assert binding.fold_dwconv_ln_form(fmt, 128, L, C, k, d, 4, True, 40) == f"fold_dwconv_ln<{fmt},K5,rv,ns3,S4,U3> run 40 cps 2"
            assert binding.fold_dwconv_ln_form(fmt, 128, L, C, k, 1, 4, False, 40) == f"fold_dwconv_ln<{fmt},K5,norv,ns3,S4,U3> run 40 cps 2"
    # a single utterance: 49 frames, 12 splits (one slab), runs of 8
    l1 = latent_lengths(a, workload.forced_durations([workload.C1_SENTENCE]) / np.float32(1.05))
    assert l1 == [49] and binding.fold_run_frames(l1, 256) == 0
    for fmt in FMTS:
        for L in (49, 64):
            for d in dils:
                assert binding.fold_dwconv_ln_form(fmt, 1, L, C, k, d, 12, True, 0) == f"fold_dwconv_ln<{fmt},K5,rv,ns3,S12,U1> run 8 cps {L // 8 + (L % 8 > 0)}"
    # mixed lengths (128 utterances of 4..40 words): no run length up to 48 brings the grid into one round: the default
    lm = latent_lengths(a, workload.forced_durations(workload.utterances(128, min_words=4, max_words=40)) / np.float32(1.05))
    Lm = max(lm)
    assert 128 * -(-Lm // 48) > 256 and binding.fold_run_frames(lm, 256) == 0
    for fmt in FMTS:
        for d in dils:
            assert binding.fold_dwconv_ln_form(fmt, 128, Lm, C, k, d, 4, True, 0) == f"fold_dwconv_ln<{fmt},K5,rv,ns3,S4,U3> run 32 cps {-(-Lm // 32)}"


# ---- the bound belongs to fp32 arithmetic --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,k,dil", [(8, 5, 1), (96, 7, 2), (384, 5, 8), (384, 5, 16), (512, 7, 6), (512, 5, 9), (392, 7, 1)])
def test_f32_restatement_stays_within_the_bound(C, k, dil):
    rng = np.random.default_rng(C + k + dil)
    lens = [1, 2, dil * (k // 2) + 1, 33, 203]
    xo = (rng.standard_normal((sum(lens), C)) * 1.3).astype(np.float32)
    w = (rng.standard_normal((C, k)) * 0.5).astype(np.float32)
    bias = (rng.standard_normal(C) * 0.3).astype(np.float32)
    g = (1.0 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    bt = (rng.standard_normal(C) * 0.3).astype(np.float32)
    m = f32_margin(xo, lens, w, bias, g, bt, dil)
    print(f"C{C} k{k} dil{dil}: float32 restatement max|d|/rms = {m:.3e}")
    assert m <= F32_REL
