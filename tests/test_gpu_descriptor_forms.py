"""The engine against the CPU oracle, stage by stage and as the RESIDENT latent, over the descriptors of tests/descriptor_cases.py: each
is the default descriptor at the smallest depths with one change that moves a stage from one kernel form to another (K4-split and its
split count, head-split or four-launch cross-attention, MFMA or scalar attention, fold K5 / K7 or no fold reader, comb or generic
dwconv + LayerNorm, K4 per stage, fixed or run-time im2col), so that the mixtures of fused and generic forms a loaded graph can land on
run together and are compared with the oracle where the forms meet: the latent batch_run keeps on the device.

Per descriptor and engine mode (fresh engine, load_synthetic(a, 7); B = 3, 14 / 9 / 5 tokens, 10 / 5 / 1 latent frames, 3 Euler steps):
  1. duration against the oracle, rtol 2e-5 (the predictor is fp32 in every mode)
  2. text_enc against the oracle; padded tokens exactly zero
  3. batch_upload + batch_set_noise + batch_run + batch_fetch_latent against the oracle's Euler loop on the oracle's own text embedding;
     frames past each utterance's length exactly zero; 16-bit engines once more with K4 allowed at any row count (mask 15)
  4. vocoder(oracle latent) against the oracle's vocoder; the batch's waveform against the oracle's synthesis
  5. the launch log holds the kernel families the table promises and none it excludes (the log names kernels without their template
     arguments: the split count and the fold's K are the host decision functions' answers for the engine's own row count, which
     tests/test_descriptor_cases_cpu.py pins to the table; the im2col variant is the launcher's condition restated in
     descriptor_cases.forms, and here only its result is checked, by the vocoder's parity on ld16ccf4)
  6. the logged (eager), eager, captured and replayed runs give the same latent bit for bit
Bounds: descriptor_cases.bound() — fp32 gpu_util.CEILING; 16-bit 2 x measured, never above CEILING nor above a quarter of the smallest
ablation distance of the stage (tests/test_descriptor_cases_cpu.py asserts that of every committed bound).

Measured on an MI355X: the 63 cases take 27 s in all with the oracle's runs, 0.1 to 1.1 s each; every check of every descriptor passes
in all three modes and no form condition had to change.  Worst latent error per descriptor (max / rms, relative to the rms of the
oracle's latent; the worse of the default run and the K4 run) and its share of the bound and of the cap:
  base          f32 2.3e-06 / 3.9e-07; bf16 1.6e-02 / 2.8e-03 (51 % / 51 % of its bound, 19 % / 15 % of the cap); f16 1.9e-03 / 3.5e-04 (50 % / 50 % of its bound, 2 % / 2 % of the cap)
  main2         f32 2.1e-06 / 3.7e-07; bf16 1.5e-02 / 2.8e-03 (51 % / 51 % of its bound, 17 % / 17 % of the cap); f16 1.7e-03 / 3.6e-04 (51 % / 50 % of its bound, 2 % / 2 % of the cap)
  ve_dh64       f32 1.9e-06 / 3.9e-07; bf16 1.6e-02 / 2.8e-03 (51 % / 51 % of its bound, 19 % / 15 % of the cap); f16 1.7e-03 / 3.4e-04 (51 % / 50 % of its bound, 2 % / 2 % of the cap)
  ve_dh48       f32 1.9e-06 / 3.9e-07; bf16 1.6e-02 / 2.8e-03 (50 % / 51 % of its bound, 18 % / 16 % of the cap); f16 1.6e-03 / 3.5e-04 (51 % / 51 % of its bound, 2 % / 2 % of the cap)
  ve_k7         f32 2.4e-06 / 3.8e-07; bf16 1.3e-02 / 2.9e-03 (51 % / 51 % of its bound, 15 % / 16 % of the cap); f16 1.9e-03 / 3.7e-04 (50 % / 50 % of its bound, 2 % / 2 % of the cap)
  ve_k3         f32 1.9e-06 / 3.9e-07; bf16 1.3e-02 / 2.9e-03 (49 % / 51 % of its bound, 14 % / 15 % of the cap); f16 1.7e-03 / 3.6e-04 (49 % / 50 % of its bound, 2 % / 2 % of the cap)
  ve_k9         f32 2.0e-06 / 3.9e-07; bf16 1.3e-02 / 2.8e-03 (55 % / 50 % of its bound, 15 % / 15 % of the cap); f16 1.7e-03 / 3.6e-04 (46 % / 51 % of its bound, 2 % / 2 % of the cap)
  fold_edge     f32 2.2e-06 / 3.8e-07; bf16 1.4e-02 / 2.8e-03 (50 % / 50 % of its bound, 17 % / 16 % of the cap); f16 1.8e-03 / 3.6e-04 (50 % / 50 % of its bound, 2 % / 2 % of the cap)
  fold_over     f32 1.9e-06 / 3.9e-07; bf16 1.7e-02 / 2.8e-03 (54 % / 50 % of its bound, 21 % / 16 % of the cap); f16 1.7e-03 / 3.6e-04 (52 % / 52 % of its bound, 2 % / 2 % of the cap)
  ve_dil128     f32 1.8e-06 / 3.9e-07; bf16 1.5e-02 / 2.8e-03 (54 % / 51 % of its bound, 19 % / 16 % of the cap); f16 1.6e-03 / 3.6e-04 (48 % / 51 % of its bound, 2 % / 2 % of the cap)
  ve512         f32 2.4e-06 / 4.1e-07; bf16 1.5e-02 / 2.8e-03 (50 % / 50 % of its bound, 14 % / 14 % of the cap); f16 1.9e-03 / 3.5e-04 (51 % / 51 % of its bound, 2 % / 2 % of the cap)
  ve_i1024      f32 2.2e-06 / 3.8e-07; bf16 1.3e-02 / 2.8e-03 (52 % / 50 % of its bound, 16 % / 15 % of the cap); f16 1.6e-03 / 3.6e-04 (51 % / 50 % of its bound, 2 % / 2 % of the cap)
  ve_i1152      f32 2.1e-06 / 3.8e-07; bf16 1.3e-02 / 2.8e-03 (50 % / 50 % of its bound, 15 % / 15 % of the cap); f16 1.8e-03 / 3.5e-04 (48 % / 51 % of its bound, 2 % / 2 % of the cap)
  vo384k5       f32 2.3e-06 / 3.9e-07; bf16 1.6e-02 / 2.8e-03 (51 % / 51 % of its bound, 19 % / 15 % of the cap); f16 1.9e-03 / 3.5e-04 (50 % / 50 % of its bound, 2 % / 2 % of the cap)
  vo1024        f32 2.3e-06 / 3.9e-07; bf16 1.6e-02 / 2.8e-03 (51 % / 51 % of its bound, 19 % / 15 % of the cap); f16 1.9e-03 / 3.5e-04 (50 % / 50 % of its bound, 2 % / 2 % of the cap)
  vo520         f32 2.3e-06 / 3.9e-07; bf16 1.6e-02 / 2.8e-03 (51 % / 51 % of its bound, 19 % / 15 % of the cap); f16 1.9e-03 / 3.5e-04 (50 % / 50 % of its bound, 2 % / 2 % of the cap)
  ld16ccf4      f32 1.7e-06 / 4.1e-07; bf16 1.3e-02 / 3.0e-03 (51 % / 51 % of its bound, 14 % / 15 % of the cap); f16 1.5e-03 / 3.5e-04 (51 % / 50 % of its bound, 2 % / 2 % of the cap)
  te384         f32 2.0e-06 / 4.2e-07; bf16 1.7e-02 / 3.0e-03 (57 % / 52 % of its bound, 17 % / 16 % of the cap); f16 1.8e-03 / 3.8e-04 (46 % / 53 % of its bound, 2 % / 2 % of the cap)
  vo_dil64      f32 2.3e-06 / 3.9e-07; bf16 1.6e-02 / 2.8e-03 (51 % / 51 % of its bound, 19 % / 15 % of the cap); f16 1.9e-03 / 3.5e-04 (50 % / 50 % of its bound, 2 % / 2 % of the cap)
  min8          f32 1.6e-06 / 2.5e-07; bf16 1.7e-02 / 2.8e-03 (51 % / 50 % of its bound, 18 % / 16 % of the cap); f16 2.4e-03 / 3.4e-04 (51 % / 50 % of its bound, 2 % / 2 % of the cap)
  base_zero_len f32 2.2e-06 / 3.7e-07; bf16 1.5e-02 / 2.9e-03 (51 % / 50 % of its bound, 15 % / 16 % of the cap); f16 2.0e-03 / 3.4e-04 (50 % / 50 % of its bound, 2 % / 2 % of the cap)
(16-bit bounds are 2 x these figures by construction; fp32 is held to CEILING e2e 2e-3 / 5e-4, of which it uses about a thousandth.)
No bf16 case of this table is over its cap; the one that is, the full default stack, is in tests/test_gpu_xattn.py."""
import numpy as np
import pytest

from supertonic_amd import binding
import descriptor_cases as dc

pytestmark = pytest.mark.gpu


def _run(eng, x):
    eng.batch_upload(x["ids"], x["mask"], x["sttl"], x["sdp"], duration_override=x["durs"])
    eng.batch_set_noise(x["noise"])
    eng.batch_run(dc.STEPS, 1.0, 1234)
    return eng.batch_fetch_latent().copy()


def _logged(eng, x):
    """one eager run with the launch log on -> (latent, {family: set of kernel names})"""
    eng.profile_enable(True)
    eng.launch_log_enable(True)
    eng.profile_reset()
    lat = _run(eng, x)
    log = eng.launch_log()
    eng.launch_log_enable(False)
    eng.profile_enable(False)
    fam = {}
    for f, k in log:
        fam.setdefault(f, set()).add(k)
    return lat, fam


def _padding_is_zero(lat, lens):
    return all(np.all(lat[b, :, n:] == 0) for b, n in enumerate(lens))


def _same(got, want, what, name):
    assert got == want, f"{name}: {what}: the engine ran {got!r}, the table says {want!r}"


def _generic(kernels):
    return kernels == {"dwconv_ln_kernel"}


def _forms_default(name, dtype, eng, fam, x):
    a, e = dc.arch(name), dc.expected(name)
    half = dtype != "f32"
    ve = e["ve"] if half else "gemms"
    split = ve.startswith("k4split")
    hs = e["hs"] and half
    _same("ve.ffn_split" in fam, split, "K4-split", name)
    _same("ve.ffn_fused" in fam, False, "estimator K4 at the default mask", name)
    _same("ve.xattn_hs" in fam, hs, "head-split cross-attention", name)
    _same("ve.attention" in fam, not hs, "four-launch cross-attention", name)
    _same("ve.gemm_q" in fam and "ve.gemm_attn_out" in fam, not hs, "q and output projections of the four launches", name)
    _same("ve.fold_dwconv_ln" in fam, split, "fold_dwconv_ln", name)
    _same("ve.fold_ln" in fam, split, "fold_ln", name)
    _same(_generic(fam["ve.dwconv_ln"]), e["conv"] == "generic", "generic estimator dwconv + LayerNorm", name)
    _same(_generic(fam["vo.dwconv_ln"]), e["vo_conv"] == "generic", "generic vocoder dwconv + LayerNorm", name)
    _same("vo.im2col" in fam, half, "im2col + GEMM vocoder entry", name)
    _same("vo.vocoder_in" in fam, not half, "direct vocoder entry", name)
    if half:
        if not hs:
            _same(fam["ve.attention"], {"attn_mfma_kernel" if e["attn"].startswith("mfma") else "attn_kernel"}, "attention kernel", name)
        # the engine's own row count through the host's decision function: the split count the launches took
        rows = int(eng.ve_rows)
        _same(rows, x["rows"] if e["packed"] else x["B"] * x["L"], "estimator rows", name)
        f = dc.forms(name, dtype, rows)
        _same(f["ve"], e["ve"], "estimator pointwise form at the engine's rows", name)
        _same(f["fold"], e["fold"], "fold instantiation", name)
    else:
        _same(fam["ve.attention"], {"attn_kernel"}, "fp32 attention kernel", name)
    for f in ("vo.ffn_fused", "te.ffn_fused", "dp.ffn_fused"):  # K4 below its row threshold
        _same(f in fam, False, f, name)
    assert a.ve_dim == 384 or not split


def _forms_k4(name, fam):
    e = dc.expected(name)
    _same("vo.ffn_fused" in fam, e["vo_k4"] == "k4", "vocoder K4 under mask 15", name)
    _same("te.ffn_fused" in fam, e["te_k4"] == "k4", "text-encoder K4 under mask 15", name)
    _same("ve.ffn_fused" in fam, e["ve_k4"] == "k4", "estimator K4 under mask 15", name)
    _same("ve.ffn_split" in fam, e["ve_k4"].startswith("k4split"), "K4-split under mask 15", name)
    _same("ve.xattn_hs" in fam, e["hs"], "head-split under mask 15", name)
    for stage, key in (("vo", "vo_k4"), ("ve", "ve_k4")):  # (the text encoder's self-attention blocks keep a two-GEMM feed-forward of their own)
        _same(f"{stage}.gemm_pw1_gelu" in fam, e[key] == "gemms", f"{stage} pointwise pair as two GEMMs under mask 15", name)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", dc.NAMES)
def test_descriptor_against_the_oracle(name, dtype):
    a, x, o = dc.arch(name), dc.inputs(name), dc.oracle(name)
    eng = binding.Engine(0, dtype)
    try:
        eng.load_synthetic(a, dc.SEED)
        # 1. durations
        np.testing.assert_allclose(eng.duration(x["ids"], x["sdp"], x["mask"]), o["dur"], rtol=2e-5)
        # 2. text embedding
        emb = eng.text_enc(x["ids"], x["sttl"], x["mask"])
        dc.check(name, "text_emb", dtype, emb, o["text_emb"])
        tokens = dc.CASES[name].get("tokens", dc.TOKENS)
        assert _padding_is_zero(emb, tokens)
        # 3. + 5. the resident latent and the forms that made it
        lat, fam = _logged(eng, x)
        wav, dur = eng.batch_fetch()
        assert lat.shape == o["latent"].shape and wav.shape == o["e2e_wav"].shape
        dc.check(name, "latent", dtype, lat, o["latent"])
        assert _padding_is_zero(lat, x["lens"])
        _forms_default(name, dtype, eng, fam, x)
        # 4. the batch's waveform, and the vocoder alone on the oracle's latent
        dc.check(name, "e2e_wav", dtype, wav, o["e2e_wav"])
        dc.check(name, "vocoder_wav", dtype, eng.vocoder(o["latent"]), o["vocoder_wav"])
        # 6. eager, captured, replayed
        for _ in range(3):
            assert np.array_equal(_run(eng, x), lat)
        if dtype != "f32":
            eng.set_fused_ffn_min_rows(1, 1)
            eng.set_fused_ffn(15)
            lat4, fam4 = _logged(eng, x)
            wav4, _ = eng.batch_fetch()
            dc.check(name, "latent_k4", dtype, lat4, o["latent"])
            assert _padding_is_zero(lat4, x["lens"])
            dc.check(name, "e2e_wav", dtype, wav4, o["e2e_wav"])
            _forms_k4(name, fam4)
            for _ in range(3):
                assert np.array_equal(_run(eng, x), lat4)
    finally:
        eng.close()
