#!/usr/bin/env python3
"""What the pitch report costs, from the output stage's own HIP-event spans (stn_profile_*): the family out.f0
(f0_track_kernel + f0_stats_kernel) on (1) a C3-sized batch (128 utterances of the default architecture on synthetic weights, 44.1 kHz),
(2) the case rows of tests/f0_cases.py at 8 and 192 kHz and (3) one row at the report's cap at 8 kHz, and beside each the four launches
of the loudness measurement (out.loudness) and the pitch shift's search kernel (out.pitch_search, +3 semitones) on the same rows.
Medians over the rounds.

    python tools/f0_cost.py [--rounds 9] [--rows 128]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from supertonic_amd import binding, host, workload  # noqa: E402
from supertonic_amd.arch import default_arch  # noqa: E402
import f0_cases  # noqa: E402


def spans(e, rounds, run, families):
    """median ms of each family over `rounds` runs of run()"""
    run()  # warm: tables, scratch
    got = {f: [] for f in families}
    e.profile_enable(True)
    for _ in range(rounds):
        e.profile_reset()
        run()
        p = e.profile()
        for f in families:
            got[f].append(p[f]["ms"] if f in p else float("nan"))
    e.profile_enable(False)
    return {f: round(statistics.median(v) * 1e3, 1) for f, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--rows", type=int, default=128)
    args = ap.parse_args()
    arch = default_arch()
    a, b = binding.pitch_ratio(3.0)
    G, cap = binding.f0_group()
    out = {}
    e = binding.Engine(0, "bf16")
    e.load_synthetic(arch, 7)

    def ops(name, x, hz, n):
        clean = np.nan_to_num(x, nan=0.0)  # (the stretch reads zeros behind a span: no poison for it)
        us = {}
        us.update(spans(e, args.rounds, lambda: e.op_f0(x, hz, n), ["out.f0"]))
        us.update(spans(e, args.rounds, lambda: e.op_loudness(x, hz, n), ["out.loudness"]))
        us.update(spans(e, args.rounds, lambda: e.op_time_stretch(clean, hz, a, b, n=n), ["out.pitch_search"]))
        frames = [binding.f0_plan(hz, int(v))["frames"] for v in n]
        out[name] = dict(rows=len(n), W=int(x.shape[1]), hz=hz, frames=int(sum(frames)), us=us)
        print(f"{name}: {len(n)} rows x {x.shape[1]} at {hz} Hz, {sum(frames)} frames: " + "  ".join(f"{f} {v:.1f} us" for f, v in us.items()))

    for hz in (8000, 192000):
        x, n = f0_cases.case_rows(hz, G)
        ops(f"case rows {hz}", x, hz, n)
    g = binding.f0_plan(8000, 0)
    at_cap = (cap - 1) * g["hop"] + 2 * g["tau_max"]
    t = np.arange(at_cap) / 8000.0
    ops("one row at the cap", (0.3 * np.sin(2 * np.pi * 140.0 * t)).astype(np.float32)[None, :], 8000, np.array([at_cap], np.int64))

    texts = workload.utterances(args.rows, min_words=10, max_words=10, seed=1234)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * args.rows)
    sttl, sdp = workload.synthetic_styles(arch, list(range(args.rows)))
    e.batch_upload(ids, mask, sttl, sdp, duration_override=workload.forced_durations(texts))
    e.batch_run(5, 1.05, 1)
    B, _, Wb = e.batch_dims()
    us = {}
    us.update(spans(e, args.rounds, e.batch_f0, ["out.f0"]))
    us.update(spans(e, args.rounds, e.batch_loudness, ["out.loudness"]))

    def shifted_fetch():
        e.set_pitch(3.0)  # (set again: that drops the shifted rows kept per batch and setting)
        e.batch_fetch_encoded("pcm16")

    us.update(spans(e, args.rounds, shifted_fetch, ["out.pitch_search"]))
    e.set_pitch(None)
    st = e.batch_f0()[2]
    out["C3 batch"] = dict(rows=B, W=int(Wb), hz=arch.sample_rate, frames=int(st["frames"].sum()), us=us)
    print(f"C3 batch: {B} rows x {Wb} at {arch.sample_rate} Hz, {st['frames'].sum()} frames: " + "  ".join(f"{f} {v:.1f} us" for f, v in us.items()))
    print(json.dumps(out))
    e.close()


if __name__ == "__main__":
    main()
