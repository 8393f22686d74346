"""The descriptor table of tests/descriptor_cases.py on the CPU: the oracle runs every descriptor; the table's "what flips" columns are
the host's own decision functions' answers for the shapes each descriptor produces; and the bounds tests/test_gpu_descriptor_forms.py
asserts are tight enough to see a dead or mis-fed block: every committed bound is at most a quarter of the smallest distance any ablation
moves the oracle's stage output (style zeroed / rotated among utterances, text zeroed, a step index off by one, a step missing; ids
rotated; latent shifted by a frame or by a channel block), in max and in rms.  The check function itself is shown to refuse the oracle
run on rotated style rows for every descriptor and mode."""
import json
import os
import time

import numpy as np
import pytest

from gpu_util import CEILING
import descriptor_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dc.NAMES + [dc.FULL]


def _json(path):
    with open(path) as f:
        return json.load(f)


def test_the_oracle_runs_every_descriptor_quickly():
    dc.oracle.cache_clear()
    t0 = time.perf_counter()
    for name in dc.NAMES:
        a, x, o = dc.arch(name), dc.inputs(name), dc.oracle(name)
        B, L = x["B"], x["L"]
        assert o["dur"].shape == (B,) and np.all(o["dur"] > 0)
        assert o["text_emb"].shape == (B, a.te_out_dim, x["Lt"])
        assert o["latent"].shape == (B, a.latent_channels, L) == x["noise"].shape
        assert o["vocoder_wav"].shape == (B, L * a.chunk_size)
        for k, v in o.items():
            assert np.all(np.isfinite(v)), (name, k)
        for b, n in enumerate(x["lens"]):
            assert np.all(o["latent"][b, :, n:] == 0) and (n == 0 or np.any(o["latent"][b, :, :n] != 0))
    took = time.perf_counter() - t0
    print(f"oracle chain over {len(dc.NAMES)} descriptors: {took:.1f} s")
    assert took < 60.0
    assert len(dc.NAMES) >= 20 and {"base", "main2", "fold_edge", "fold_over", "min8", "vo_dil64"} <= set(dc.NAMES)


def test_the_shared_full_depth_chain_is_the_oracles_synthesis():
    """descriptor_cases.oracle(FULL) is what tests/test_gpu_xattn.py::test_head_split_vs_oracle compares the waveform with: the same bits
    as RefModel.synthesize on that test's inputs."""
    from oracle.neural_ref import RefModel
    a, x, o = dc.arch(dc.FULL), dc.inputs(dc.FULL), dc.oracle(dc.FULL)
    wav, _ = RefModel(a, dc.SEED).synthesize(x["ids"], x["mask"], x["sttl"], x["sdp"], dc.STEPS, np.float32(x["speed"]), lambda B, D, L: x["noise"],
                                             duration_override=x["durs"])
    assert np.array_equal(wav, o["e2e_wav"])
    assert x["L"] <= 256 and x["Lt"] <= 128  # inside the head-split kernel's shapes


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name", dc.NAMES)
def test_the_table_is_what_the_host_decides(name, dtype):
    f, e = dc.forms(name, dtype), dc.expected(name)
    assert {k: f[k] for k in e} == e, name
    assert f["hs"] == e["hs"] and (not e["hs"] or (e["ve"].startswith("k4split") and e["fold"]))  # head-split only where a fold reader follows


def test_the_rows_the_table_names_are_where_it_says():
    from supertonic_amd import binding as bd
    x = dc.inputs("base")
    B, L = x["B"], x["L"]
    assert "S12" in dc.forms("base")["fold_full"] and "S4" in dc.forms("ve_i1024")["fold_full"]
    assert ",ns4," in bd.fold_dwconv_ln_form("bf16", B, L, 512, 5, 1, 4)  # (ve512's width folds in four slots where a split reaches it)
    # fold_edge's widest dilation is the last the fold takes at C = 384, k = 5; fold_over's is the first it refuses
    bd.fold_dwconv_ln_form("bf16", B, L, 384, 5, 16, 12)
    with pytest.raises(bd.StnError):
        bd.fold_dwconv_ln_form("bf16", B, L, 384, 5, 32, 12)
    assert dc.arch("fold_edge").ve_dilated == 5 and dc.arch("fold_over").ve_dilated == 6
    # vo_dil64: the receptive field is longer than every utterance's own frames plus twice itself: no row is trimmed
    a = dc.arch("vo_dil64")
    rf = (a.vo_in_kernel - 1) // 2 + sum((a.vo_kernel - 1) // 2 * a.vo_dilations[i] for i in range(a.vo_blocks))
    T = L * a.chunk_compress_factor
    assert all(n * a.chunk_compress_factor + 2 * rf > T for n in x["lens"]) and rf > T
    # ve_dil128: dilations wider than every sequence
    assert 1 << (dc.arch("ve_dil128").ve_dilated - 1) > L


@pytest.mark.parametrize("name", ALL)
def test_every_committed_bound_sees_every_ablation(name):
    """bound <= CAP_SHARE x the smallest ablation distance of its stage (max and rms), for the fp32 ceilings and every recorded 16-bit bound;
    the bf16 cases the bounds file lists as over their cap are exactly those, with exactly the ablations that are closer than four bounds."""
    ab = dc.ablations(name)
    over = dc._bounds_file().get("over_cap", {})
    whats = ["latent"] if name == dc.FULL else [w for w in dc.STAGE_OF]
    for what in whats:
        stage = dc.STAGE_OF[what]
        dist = ab[stage]
        assert len(dist) >= (1 if stage == "vocoder_wav" else 2) and all(d[0] > 0 and d[1] > 0 for d in dist.values()), (name, stage, dist)
        cmax, crms = dc.cap(name, what)
        print(f"{name}.{what}: cap max {cmax:.3g} rms {crms:.3g}  " + ", ".join(f"{k} {d[0]:.3g}/{d[1]:.3g}" for k, d in dist.items()))
        for dtype in ("f32", "bf16", "f16"):
            bmax, brms, src = dc.bound(name, what, dtype)
            listed = over.get(f"desc.{name}.{what}", {}).get(dtype)
            if listed is None:
                assert bmax <= cmax and brms <= crms, f"desc.{name}.{what} [{dtype}] ({src}): bound {bmax:.3g}/{brms:.3g} over cap {cmax:.3g}/{crms:.3g}"
            else:
                assert dtype == "bf16" and src == "recorded" and (bmax > cmax or brms > crms), (name, what, dtype)
                assert listed == sorted(k for k, d in dist.items() if dc.CAP_SHARE * d[0] < bmax or dc.CAP_SHARE * d[1] < brms) and listed


def test_bounds_are_at_most_twice_the_measured_error():
    measured = _json(dc.MEASURED_PATH)["measured"]
    bf = _json(dc.BOUNDS_PATH)
    bounds, over = bf["bounds"], bf["over_cap"]
    want = {f"desc.{n}.{w}" for n in dc.NAMES for w in dc.KIND} | {f"desc.{dc.FULL}.latent"}
    assert set(measured) == want and set(bounds) == want
    for case, per in measured.items():
        assert set(per) >= {"bf16", "f16"} and set(bounds[case]) == {"bf16", "f16"}, case
        for dtype, m in per.items():
            cmax, crms = CEILING[dtype][m["kind"]]
            assert m["max"] <= cmax and m["rms"] <= crms, (case, dtype)
            if dtype == "f32":
                continue
            b = bounds[case][dtype]
            for k in ("max", "rms"):
                assert m[k] <= b[k] <= 2.0 * m[k] * (1 + 1e-12), (case, dtype, k, m[k], b[k])
    assert all(set(v) == {"bf16"} for v in over.values())


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", ALL)
def test_the_latent_check_refuses_the_oracle_on_rotated_style_rows(name, dtype, monkeypatch):
    monkeypatch.delenv("STN_PARITY_RECORD", raising=False)
    monkeypatch.delenv("STN_PARITY_RECORD_ONLY", raising=False)
    o, wrong = dc.oracle(name), dc.ablations(name)["rotated_style_latent"]
    for what in ("latent",) if name == dc.FULL else ("latent", "latent_k4"):
        dc.check(name, what, dtype, o["latent"], o["latent"])  # (the check passes what is right)
        with pytest.raises(AssertionError, match="bound"):
            dc.check(name, what, dtype, wrong, o["latent"])
