"""Measure the engine-vs-oracle error of every named parity case on an MI355X and derive the test bounds from it.

  python tools/parity_record.py [--out-dir gpurun_out/parity]
  python tools/parity_record.py --descriptors [--out-dir DIR]

Runs the oracle-parity tests (tests/test_gpu_stages.py, tests/test_gpu_configs.py, tests/test_gpu_load_dir.py, tests/test_gpu_ffn.py) once with STN_PARITY_RECORD set — the tests'
own inputs, engines and comparison code, so what is recorded is exactly what the tests assert on — and writes
  parity_r04.json     {"measured": {case: {dtype: {"max", "rms", "kind", "n"}}}, "_source_sha": ...}   -> commit as profiles/parity_r04.json
  parity_bounds.json  {"bounds": {case: {dtype: {"max", "rms"}}}}: 2 x measured, rounded DOWN to two digits, not below
                      FLOOR (fp32 summation-order noise)                                                      -> tests/golden/
(max, rms) are relative to the rms of the oracle's output (tests/gpu_util.rel_err).  tests/test_parity_bounds_cpu.py keeps the
two files consistent: no bound looser than 2 x its measurement.

--descriptors runs only tests/test_gpu_descriptor_forms.py and tests/test_gpu_xattn.py::test_head_split_vs_oracle and writes only
  parity_descriptors.json   {"measured": ...} of the "desc.*" cases                                            -> commit under profiles/
  descriptor_bounds.json    {"bounds": ..., "cap": ..., "over_cap": ...}: 16-bit bounds, 2 x measured rounded down to two digits, never
                            above gpu_util.CEILING nor above the cap (tests/descriptor_cases.py: a quarter of the smallest ablation
                            distance of the stage, computed here on the CPU oracle).  A bf16 case whose 2 x measured is above its cap
                            keeps 2 x measured and is listed under "over_cap" with the ablations it no longer tells from rounding; an
                            f16 case never is (its bound stays the cap, and the test fails)                     -> tests/golden/
and leaves parity_r04.json / parity_bounds.json alone."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.src_hash import source_sha  # noqa: E402


FLOOR = {"max": 2e-6, "rms": 5e-7}


def floor2(x):
    """x rounded down to two significant digits (so that 2 x measured stays an upper limit of the bound)."""
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x)) - 1
    return math.floor(x / 10 ** e) * 10 ** e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "gpurun_out", "parity"))
    ap.add_argument("--descriptors", action="store_true", help="only the descriptor table's cases, into parity_descriptors.json / descriptor_bounds.json")
    args = ap.parse_args()
    if args.descriptors:
        return main_descriptors(args.out_dir)
    measured = record(args.out_dir, "records.jsonl",
                      ["tests/test_gpu_stages.py", "tests/test_gpu_configs.py", "tests/test_gpu_load_dir.py", "tests/test_gpu_ffn.py"])
    # an error of a few fp32 ulps is summation-order noise: its bound does not go below FLOOR (16 / 4 ulps of the output's rms)
    bounds = {c: {d: {"max": max(floor2(2 * v["max"]), FLOOR["max"]), "rms": max(floor2(2 * v["rms"]), FLOOR["rms"])} for d, v in per.items()}
              for c, per in measured.items()}
    note = ("relative to the rms of the oracle output (tests/gpu_util.rel_err); tiny = tests' small descriptor, c1/c3/c4/c5 = the 66 M stack on "
            "BASELINE.json's configs; engine through the C ABI vs oracle/stn_ref.c on identical synthetic weights and inputs")
    with open(os.path.join(args.out_dir, "parity_r04.json"), "w") as f:
        json.dump({"_source_sha": source_sha(), "note": note, "measured": measured}, f, indent=1, sort_keys=True)
    with open(os.path.join(args.out_dir, "parity_bounds.json"), "w") as f:
        json.dump({"source": "profiles/parity_r04.json (tools/parity_record.py): bound = max(2 x measured rounded down to two digits, floor)",
                   "floor": FLOOR, "bounds": bounds},
                  f, indent=1, sort_keys=True)
    for c in sorted(measured):
        for d, v in sorted(measured[c].items()):
            print(f"{c:36s} {d:5s} max {v['max']:.3e} rms {v['rms']:.3e}   bound max {bounds[c][d]['max']:.2g} rms {bounds[c][d]['rms']:.2g}")


def record(out_dir, log_name, targets):
    """run `targets` once with STN_PARITY_RECORD set -> {case: {dtype: worst (max, rms), kind, n}}"""
    os.makedirs(out_dir, exist_ok=True)
    log = os.path.join(out_dir, log_name)
    if os.path.exists(log):
        os.remove(log)
    env = dict(os.environ, STN_PARITY_RECORD=log, STN_PARITY_RECORD_ONLY="1")
    rc = subprocess.call([sys.executable, "-m", "pytest", *targets, "-q", "-m", "gpu", "-x"], cwd=ROOT, env=env)
    if rc != 0:
        sys.exit(f"parity tests failed (rc={rc}): nothing recorded")
    measured = {}
    with open(log) as f:
        for line in f:
            r = json.loads(line)
            m = measured.setdefault(r["case"], {}).setdefault(r["dtype"], {"max": 0.0, "rms": 0.0, "kind": r["kind"], "n": r["n"]})
            m["max"], m["rms"] = max(m["max"], r["max"]), max(m["rms"], r["rms"])
    return measured


def descriptor_bounds(measured):
    """(bounds, caps, over_cap) of the "desc.<name>.<what>" cases from their measurements and the oracle's ablation distances"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import descriptor_cases as dc
    from gpu_util import CEILING
    bounds, caps, over = {}, {}, {}
    for case, per in sorted(measured.items()):
        _, name, what = case.split(".")
        cap = dc.cap(name, what)
        if cap:
            caps[case] = {"max": cap[0], "rms": cap[1]}
        for dtype, v in sorted(per.items()):
            if dtype == "f32":
                continue  # held to CEILING
            ceil = CEILING[dtype][v["kind"]]
            b = {k: min(max(floor2(2 * v[k]), FLOOR[k]), ceil[i]) for i, k in enumerate(("max", "rms"))}
            if cap and (b["max"] > cap[0] or b["rms"] > cap[1]):
                if dtype == "bf16":
                    dist = dc.ablations(name)[dc.STAGE_OF[what]]
                    over.setdefault(case, {})[dtype] = sorted(k for k, d in dist.items() if dc.CAP_SHARE * d[0] < b["max"] or dc.CAP_SHARE * d[1] < b["rms"])
                else:
                    b = {"max": min(b["max"], floor2(cap[0])), "rms": min(b["rms"], floor2(cap[1]))}
            bounds.setdefault(case, {})[dtype] = b
    return bounds, caps, over


def main_descriptors(out_dir):
    measured = record(out_dir, "records_descriptors.jsonl", ["tests/test_gpu_descriptor_forms.py", "tests/test_gpu_xattn.py::test_head_split_vs_oracle"])
    measured = {c: v for c, v in measured.items() if c.startswith("desc.")}
    bounds, caps, over = descriptor_bounds(measured)
    note = ("relative to the rms of the oracle output (tests/gpu_util.rel_err); desc.<name>.<what>: descriptor <name> of tests/descriptor_cases.py, "
            "<what> = text_emb, latent (resident, 3 Euler steps), latent_k4 (K4 at any row count), vocoder_wav (on the oracle's latent), e2e_wav")
    with open(os.path.join(out_dir, "parity_descriptors.json"), "w") as f:
        json.dump({"_source_sha": source_sha(), "note": note, "measured": measured}, f, indent=1, sort_keys=True)
    with open(os.path.join(out_dir, "descriptor_bounds.json"), "w") as f:
        json.dump({"source": "profiles/parity_descriptors.json (tools/parity_record.py --descriptors): 16-bit bound = min(2 x measured rounded down to two "
                             "digits, gpu_util.CEILING, cap); cap = a quarter of the smallest ablation distance of the stage on the oracle; over_cap: "
                             "bf16 cases held to 2 x measured above their cap, with the ablations closer than four bounds",
                   "floor": FLOOR, "bounds": bounds, "cap": caps, "over_cap": over}, f, indent=1, sort_keys=True)
    for c in sorted(measured):
        for d, v in sorted(measured[c].items()):
            b = bounds.get(c, {}).get(d)
            print(f"{c:36s} {d:5s} max {v['max']:.3e} rms {v['rms']:.3e}" + (f"   bound max {b['max']:.2g} rms {b['rms']:.2g}" if b else "")
                  + ("   OVER CAP: " + ", ".join(over[c][d]) if d in over.get(c, {}) else ""))


if __name__ == "__main__":
    main()
