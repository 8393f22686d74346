"""A table of architecture descriptors inside Engine::load's box, each the default descriptor cut to the smallest depths that keep every
kind of block and every seam between two kernel forms, with ONE change that flips a form; the inputs they all run on; the CPU oracle's
results for them; and, on the oracle alone, how far each stage's output moves when one of its inputs is ablated.  Shared by
tests/test_descriptor_cases_cpu.py and tests/test_gpu_descriptor_forms.py (nothing here touches a device).

Bounds.  An fp32 engine is held to gpu_util.CEILING (stage: text embedding, vocoder; e2e: the 3-step latent and the waveform).  A 16-bit
engine is held to tests/golden/descriptor_bounds.json: 2 x the error measured on an MI355X (tools/parity_record.py --descriptors, raw
figures in profiles/parity_descriptors.json), never looser than CEILING and never looser than the CAP: a quarter of the smallest distance
any ablation of that stage moves the oracle's output, in max and in rms.  A block that is dead or reads another utterance's row moves
the output by at least four bounds, so it cannot pass.  Where bf16 rounding alone measures above the cap the case is listed under
"over_cap" in the bounds file with the ablations it can no longer tell from rounding; f16 never is."""
import functools
import json
import os

import numpy as np

from oracle import host_ref
from oracle.neural_ref import RefModel, randn
from supertonic_amd.arch import default_arch
from gpu_util import CEILING, make_inputs, rel_err

_HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS_PATH = os.path.join(_HERE, "golden", "descriptor_bounds.json")
MEASURED_PATH = os.path.join(os.path.dirname(_HERE), "profiles", "parity_descriptors.json")
SEED = 7                      # weights: load_synthetic(a, SEED) / RefModel(a, SEED)
STEPS = 3
TOKENS = (14, 9, 5)           # B = 3
FRAMES = (10, 5, 1)           # latent lengths
NOISE_SEED = 31
CAP_SHARE = 0.25
KIND = {"text_emb": "stage", "vocoder_wav": "stage", "latent": "e2e", "latent_k4": "e2e", "e2e_wav": "e2e"}
STAGE_OF = {"text_emb": "text_emb", "vocoder_wav": "vocoder_wav", "latent": "latent", "latent_k4": "latent"}  # (e2e_wav: no cap, see cap())


def shallow():
    a = default_arch()
    a.te_conv_blocks = a.te_attn_blocks = a.te_style_blocks = a.dp_conv_blocks = 1
    a.ve_main_blocks, a.ve_dilated, a.ve_tail_blocks = 2, 2, 1
    a.vo_blocks = 3
    for i in range(len(a.vo_dilations)):
        a.vo_dilations[i] = (1, 2, 4)[i] if i < 3 else 1
    a.n_style_ttl = 10
    return a


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            if k == "vo_dilations":
                for i, d in enumerate(v):
                    a.vo_dilations[i] = d
            else:
                setattr(a, k, v)
    return f


def _min8(a):
    a.ve_dim = a.ve_hidden = a.ve_time_dim = a.vo_dim = a.vo_hidden = 8
    a.ve_heads = 1


# What each descriptor is there for, as the host's own decision functions state it for the shapes the descriptor produces (forms() below;
# tests/test_descriptor_cases_cpu.py holds this column to them).  Keys, all for a 16-bit engine on the resident (packed) batch:
#   ve      the estimator's pointwise pair at the engine's defaults          ve_k4   the same with K4 allowed at any row count (mask 15)
#   hs      head-split cross-attention (else four launches)                  attn    kernel of the four launches: mfma<dh> / scalar
#   fold    fold_dwconv_ln instantiation of the widest dilation, or None     conv    estimator dwconv + LayerNorm where nothing is pending: comb<k> / generic
#   packed  the estimator runs on packed rows                                vo_k4 / te_k4  vocoder / text-encoder pointwise pair under mask 15
#   vo_conv vocoder dwconv + LayerNorm kernel                                im2col  fixed (ld 24, ccf 6, k 7) or run-time
_BASE = dict(ve="k4split12", ve_k4="k4split12", hs=True, attn="mfma<96", fold="K5", packed=True, conv="comb5", vo_k4="k4", vo_conv="comb7",
             te_k4="gemms", im2col="fixed")
CASES = {
    "base": dict(change=_set()),
    "main2": dict(change=_set(), inputs_seed=1),  # the seam head-split -> first conv of the next main block, on other inputs
    "ve_dh64": dict(change=_set(ve_heads=6), hs=False, attn="mfma<64"),
    "ve_dh48": dict(change=_set(ve_heads=8), hs=False, attn="scalar"),
    "ve_k7": dict(change=_set(ve_kernel=7), fold="K7", conv="comb7"),
    "ve_k3": dict(change=_set(ve_kernel=3), ve="gemms", ve_k4="k4", hs=False, fold=None, packed=False, conv="generic"),
    "ve_k9": dict(change=_set(ve_kernel=9), ve="gemms", ve_k4="k4", hs=False, fold=None, packed=False, conv="generic"),
    "fold_edge": dict(change=_set(ve_dilated=5)),
    "fold_over": dict(change=_set(ve_dilated=6), ve="gemms", ve_k4="k4", hs=False, fold=None),
    "ve_dil128": dict(change=_set(ve_dilated=8), ve="gemms", ve_k4="k4", hs=False, fold=None),
    "ve512": dict(change=_set(ve_dim=512, ve_hidden=2048, ve_heads=8), ve="gemms", ve_k4="k4", hs=False, attn="mfma<64", fold=None),
    "ve_i1024": dict(change=_set(ve_hidden=1024), ve="k4split4", ve_k4="k4split4"),
    "ve_i1152": dict(change=_set(ve_hidden=1152), ve="gemms", ve_k4="k4", hs=False, fold=None),
    "vo384k5": dict(change=_set(vo_dim=384, vo_hidden=1536, vo_kernel=5), vo_conv="comb5"),
    "vo1024": dict(change=_set(vo_dim=1024), vo_k4="gemms", vo_conv="generic"),
    "vo520": dict(change=_set(vo_dim=520, vo_hidden=1040), vo_k4="gemms", vo_conv="generic"),
    "ld16ccf4": dict(change=_set(latent_dim=16, chunk_compress_factor=4, vo_in_kernel=3), im2col="run-time"),
    "te384": dict(change=_set(te_dim=384, te_out_dim=384, te_hidden=1536, te_ffn=1536), te_k4="k4"),
    "vo_dil64": dict(change=_set(vo_dilations=(3, 64, 1))),
    "min8": dict(change=_min8, ve="gemms", ve_k4="gemms", hs=False, attn="scalar", fold=None, conv="comb5", vo_k4="gemms", vo_conv="comb7"),
    # base once more with an utterance of no latent frame at all (it owns no packed row)
    "base_zero_len": dict(change=_set(), tokens=(14, 9, 5, 3), frames=(10, 5, 1, 0)),
}
NAMES = list(CASES)
FULL = "full_hs"  # not a row of the table: the full default stack on tests/test_gpu_xattn.py::test_head_split_vs_oracle's six utterances


def expected(name):
    e = dict(_BASE)
    e.update({k: v for k, v in CASES[name].items() if k in _BASE})
    return e


def arch(name):
    if name == FULL:
        return default_arch()
    a = shallow()
    CASES[name]["change"](a)
    return a


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The same inputs for every descriptor (its own vocabulary and style shapes apart): B = 3, 14 / 9 / 5 tokens, 10 / 5 / 1 latent frames."""
    a = arch(name)
    if name == FULL:
        return _full_inputs(a)
    c = CASES[name]
    tokens, frames = c.get("tokens", TOKENS), c.get("frames", FRAMES)
    B, Lt = len(tokens), max(tokens)
    ids, mask, sttl, sdp = make_inputs(a, B, Lt, list(tokens), seed=c.get("inputs_seed", 0))
    # half a frame short of `frames` frames; 1e-5 s is no sample, hence no frame
    durs = np.array([(f - 0.5) * a.chunk_size / a.sample_rate if f else 1e-5 for f in frames], np.float32)
    D, L, lens = host_ref.latent_geometry(durs, a.sample_rate, a.base_chunk_size, a.chunk_compress_factor, a.latent_dim)
    assert tuple(int(v) for v in lens) == tuple(frames) and L == max(frames), (name, lens, L)
    lmask = host_ref.length_to_mask(lens, L)
    noise = randn(NOISE_SEED, B, D, L)
    for v in (ids, mask, sttl, sdp, durs, lmask, noise):
        v.setflags(write=False)
    return dict(ids=ids, mask=mask, sttl=sttl, sdp=sdp, durs=durs, D=D, L=L, lens=tuple(int(v) for v in lens), lmask=lmask, noise=noise,
                B=B, Lt=Lt, rows=int(sum(lens)), speed=1.0)


def _full_inputs(a, n=6, speed=np.float32(1.05)):
    from supertonic_amd import host, workload
    texts = workload.utterances(n, min_words=3, max_words=9, seed=5)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * n)
    sttl, sdp = workload.synthetic_styles(a, list(range(n)))
    durs = (workload.forced_durations(texts) / speed * speed).astype(np.float32)  # the override; the run divides it by the speed again
    D, L, lens = host_ref.latent_geometry((durs / speed).astype(np.float32), a.sample_rate, a.base_chunk_size, a.chunk_compress_factor, a.latent_dim)
    lmask = host_ref.length_to_mask(lens, L)
    noise = randn(11, n, D, L)
    return dict(ids=ids, mask=mask, sttl=sttl, sdp=sdp, durs=durs, D=D, L=L, lens=tuple(int(v) for v in lens), lmask=lmask, noise=noise,
                B=n, Lt=ids.shape[1], rows=int(sum(lens)), speed=float(speed))


def euler(ref, x0, emb, sttl, mask, lmask, steps=STEPS, total=STEPS, step_shift=0):
    """The oracle's Euler loop of TextToSpeech::_infer on given inputs: `steps` steps of a schedule of `total`."""
    B = x0.shape[0]
    x = (x0 * lmask).astype(np.float32)
    for s in range(steps):
        x = ref.vector_est(x, emb, sttl, mask, lmask, np.full(B, total, np.float32), np.full(B, s + step_shift, np.float32))
    return x


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The oracle chain for one descriptor: duration, text embedding, the latent after STEPS Euler steps on the oracle's own embedding,
    the waveform of that latent (= RefModel.synthesize's).  Arrays are read-only: every test shares them."""
    a, x = arch(name), inputs(name)
    ref = RefModel(a, SEED)
    dur = ref.duration(x["ids"], x["sdp"], x["mask"])
    emb = ref.text_enc(x["ids"], x["sttl"], x["mask"])
    lat = euler(ref, x["noise"], emb, x["sttl"], x["mask"], x["lmask"])
    wav = ref.vocoder(lat)
    out = dict(dur=dur, text_emb=emb, latent=lat, vocoder_wav=wav, e2e_wav=wav)
    for v in out.values():
        v.setflags(write=False)
    ref.close()
    return out


@functools.lru_cache(maxsize=None)
def ablations(name):
    """{stage: {ablation: (max, rms)}}: how far each ablation moves the oracle's stage output, relative to the output's rms (rel_err)."""
    a, x, o = arch(name), inputs(name), oracle(name)
    ref = RefModel(a, SEED)
    ids, mask, sttl, lmask, emb, noise = x["ids"], x["mask"], x["sttl"], x["lmask"], o["text_emb"], x["noise"]
    B = x["B"]
    run = functools.partial(euler, ref)
    lat = {
        "style zeroed": run(noise, emb, np.zeros_like(sttl), mask, lmask),
        "style rows rotated": run(noise, emb, np.roll(sttl, 1, axis=0), mask, lmask),
        "text embedding zeroed": run(noise, np.zeros_like(emb), sttl, mask, lmask),
        "current_step + 1": run(noise, emb, sttl, mask, lmask, step_shift=1),
        "one Euler step fewer": run(noise, emb, sttl, mask, lmask, steps=STEPS - 1),
    }
    rot = ids.copy()
    for b, n in enumerate(mask[:, 0, :].sum(axis=1).astype(int)):
        rot[b, :n] = np.roll(ids[b, :n], 1)
    te = {
        "style zeroed": ref.text_enc(ids, np.zeros_like(sttl), mask),
        "ids rotated by one position": ref.text_enc(rot, sttl, mask),
    }
    latent = o["latent"]
    vo = {"latent shifted by one frame": ref.vocoder(np.roll(latent, 1, axis=2))} if name != FULL else {}
    if a.chunk_compress_factor > 1 and name != FULL:
        vo["latent channel blocks rotated by one"] = ref.vocoder(np.roll(latent, a.latent_dim, axis=1))
    ref.close()
    ab = {"rotated_style_latent": lat["style rows rotated"]}  # (kept: the CPU test feeds it to check() in place of an engine)
    ab.update({stage: {k: rel_err(v, o[stage]) for k, v in d.items()} for stage, d in (("latent", lat), ("text_emb", te), ("vocoder_wav", vo))})
    assert B == latent.shape[0]
    return ab


def cap(name, what):
    """(max, rms) a bound of `what` may not exceed: CAP_SHARE of the smallest ablation distance of its stage; None for the batch's waveform
    (it is held to the project's end-to-end rule: the latent and the vocoder, each under its cap, are what it is made of)."""
    stage = STAGE_OF.get(what)
    if stage is None:
        return None
    d = ablations(name)[stage]
    if not d:
        return None
    return CAP_SHARE * min(v[0] for v in d.values()), CAP_SHARE * min(v[1] for v in d.values())


@functools.lru_cache(maxsize=None)
def _bounds_file():
    try:
        with open(BOUNDS_PATH) as f:
            return json.load(f)
    except FileNotFoundError:
        return {"bounds": {}, "over_cap": {}}


def bound(name, what, dtype):
    """(max, rms) the engine's `what` of descriptor `name` is held to, and where it comes from."""
    cmax, crms = CEILING[dtype][KIND[what]]
    if dtype == "f32":
        return cmax, crms, "ceiling"
    b = _bounds_file()["bounds"].get(f"desc.{name}.{what}", {}).get(dtype)
    if b:
        return min(b["max"], cmax), min(b["rms"], crms), "recorded"
    return cmax, crms, "ceiling (no record)"


def check(name, what, dtype, got, ref):
    """Engine output against the oracle's: the shape, finite, (max, rms) error within bound().  With STN_PARITY_RECORD=<file> the
    measurement is appended there in gpu_util.parity_check's line format; with STN_PARITY_RECORD_ONLY=1 only the ceiling applies."""
    got = np.asarray(got)
    assert got.shape == np.asarray(ref).shape, (name, what, got.shape, np.asarray(ref).shape)
    assert np.all(np.isfinite(got)), (name, what, dtype)
    mx, rms = rel_err(got, ref)
    bmax, brms, src = bound(name, what, dtype)
    rec = os.environ.get("STN_PARITY_RECORD")
    if rec:
        with open(rec, "a") as f:
            f.write(json.dumps({"case": f"desc.{name}.{what}", "dtype": dtype, "kind": KIND[what], "max": mx, "rms": rms, "n": int(got.size)}) + "\n")
    if os.environ.get("STN_PARITY_RECORD_ONLY") == "1":
        bmax, brms = CEILING[dtype][KIND[what]]
    print(f"desc.{name}.{what} [{dtype}]: max {mx:.3e} ({mx / bmax:.0%} of {bmax:.3g}) rms {rms:.3e} ({rms / brms:.0%} of {brms:.3g}) [{src}]")
    assert mx <= bmax and rms <= brms, f"desc.{name}.{what} [{dtype}]: max {mx:.3e} (bound {bmax:.3g}) rms {rms:.3e} (bound {brms:.3g}) [{src}]"
    return mx, rms


def forms(name, dtype="bf16", rows=None):
    """The table's columns as the host's decision functions give them for this descriptor's shapes (supertonic_amd.binding, no device).
    rows: the estimator's packed row count (default: the sum of the latent lengths)."""
    from supertonic_amd import binding as bd
    a, x = arch(name), inputs(name)
    B, L, Lt = x["B"], x["L"], x["Lt"]
    M = x["rows"] if rows is None else rows
    C, I, k, H = a.ve_dim, a.ve_hidden, a.ve_kernel, a.ve_heads
    max_dil = 1 << max(0, a.ve_dilated - 1)
    packed = a.ve_dilated > 0 and C <= 512 and k in (5, 7)  # Engine::packed_rows_ok
    f = {"packed": packed}
    rows_ve = M if packed else B * L
    f["ve"] = bd.ffn_form(dtype, bd.FFN_ESTIMATOR, C, I, rows_ve, packed=packed, k=k, max_dil=max_dil)
    f["ve_k4"] = bd.ffn_form(dtype, bd.FFN_ESTIMATOR, C, I, rows_ve, packed=packed, k=k, max_dil=max_dil, mask=15, min_rows=1, split_min_rows=1)
    split = f["ve"].startswith("k4split")
    hs = split
    if hs:
        try:
            for Lk in (Lt, a.n_style_ttl):
                bd.attn_form(dtype, B, L, Lk, H, C // H, ldk=a.ve_main_blocks * 2 * C, kind=1)
        except bd.StnError:
            hs = False
    f["hs"] = hs
    af = bd.attn_form(dtype, B, L, Lt, H, C // H, ldk=a.ve_main_blocks * 2 * C)
    f["attn"] = af.split(",")[0] if af.startswith("mfma") else "scalar"
    f["fold"] = None
    if split:
        S = int(f["ve"][len("k4split"):])
        ff = [bd.fold_dwconv_ln_form(dtype, B, L, C, k, 1 << j, S) for j in range(a.ve_dilated)]
        f["fold"] = "K5" if ",K5," in ff[-1] else "K7" if ",K7," in ff[-1] else ff[-1]
        f["fold_full"] = ff[-1]
    comb = lambda form, kk: "generic" if form == "generic" else f"comb{kk}"  # noqa: E731  (v2 / v3 / v3occ4: the comb kernels, by row count)
    f["conv"] = comb(bd.dwconv_ln_form(dtype, B, L, C, k, packed=packed), k)
    T = L * a.chunk_compress_factor
    vo_max = max(a.vo_dilations[:a.vo_blocks])
    f["vo_k4"] = bd.ffn_form(dtype, bd.FFN_VOCODER, a.vo_dim, a.vo_hidden, B * T, packed=False, k=a.vo_kernel, max_dil=vo_max, mask=15, min_rows=1)
    f["vo_conv"] = comb(bd.dwconv_ln_form(dtype, B, T, a.vo_dim, a.vo_kernel), a.vo_kernel)
    f["te_k4"] = bd.ffn_form(dtype, bd.FFN_TEXT, a.te_dim, a.te_hidden, sum(CASES[name].get("tokens", TOKENS)), k=a.te_kernel, mask=15, min_rows=1)
    kp = (a.latent_dim * a.vo_in_kernel + 63) // 64 * 64
    f["im2col"] = "fixed" if (a.latent_dim, a.chunk_compress_factor, a.vo_in_kernel, kp) == (24, 6, 7, 192) else "run-time"  # launch_vocoder_im2col
    return f
