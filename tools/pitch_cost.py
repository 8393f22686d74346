#!/usr/bin/env python3
"""What the fetch-time pitch shift costs: (1) the search kernel's time per frame at 44.1 kHz, from the output
stage's own span (stn_profile_*) of stn_op_time_stretch on one row and on 128 rows (a row is one workgroup's chain of frames, so the
span over the frame count is the time a frame takes whatever the row count, while the rows fit the device); (2) a pcm16 fetch of a
C3-sized batch (128 utterances of the default architecture on synthetic weights) with pitch on against the same fetch with pitch off,
wall clock around the call and the spans per kernel family.  On and off are interleaved round by round and the medians printed; the
shifted rows are kept per batch and setting, so the setting is set again in front of every timed fetch (that drops them).

    python tools/pitch_cost.py [--rounds 15] [--rows 128] [--semitones 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from supertonic_amd import binding, host, workload  # noqa: E402
from supertonic_amd.arch import default_arch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--semitones", type=float, default=3.0)
    args = ap.parse_args()
    arch = default_arch()
    hz = arch.sample_rate
    a, b = binding.pitch_ratio(args.semitones)
    out = {"semitones": args.semitones, "ratio": [a, b], "hz": hz}
    e = binding.Engine(0, "bf16")
    e.load_synthetic(arch, 7)

    # (1) the search kernel per frame
    W = 4 * hz
    rng = np.random.default_rng(3)
    t = np.arange(W) / hz
    for rows in (1, args.rows):
        x = (0.5 * np.sin(2 * np.pi * (150.0 + 5.0 * np.arange(rows))[:, None] * t[None, :]) + 0.05 * rng.standard_normal((rows, W))).astype(np.float32)
        M = binding.pitch_plan(hz, W, a, b)["M"]
        e.op_time_stretch(x, hz, a, b)  # warm
        e.profile_enable(True)
        us = []
        for _ in range(args.rounds):
            e.profile_reset()
            e.op_time_stretch(x, hz, a, b)
            us.append(e.profile()["out.pitch_search"]["ms"] * 1e3)
        e.profile_enable(False)
        med = statistics.median(us)
        out[f"search_rows{rows}"] = dict(frames=M, span_us=round(med, 1), us_per_frame=round(med / (M - 1), 3))
        print(f"search, {rows} row(s) x {W} samples at {hz} Hz, {a}/{b}: {med:.1f} us over {M - 1} searched frames = {med / (M - 1):.2f} us per frame "
              f"(min {min(us):.1f}, max {max(us):.1f} over {args.rounds} rounds)")

    # (2) the fetch
    texts = workload.utterances(args.rows, min_words=3, max_words=12, seed=11)
    ids, mask = host.UnicodeProcessor(host.synthetic_indexer())(texts, ["en"] * args.rows)
    sttl, sdp = workload.synthetic_styles(arch, list(range(args.rows)))
    e.batch_upload(ids, mask, sttl, sdp, duration_override=workload.forced_durations(texts))
    e.batch_run(5, 1.05, 1)
    B, _, Wb = e.batch_dims()
    configs = {"off": None, "on": args.semitones}
    for s in configs.values():  # warm: the table, the scratch
        e.set_pitch(s)
        e.batch_fetch_encoded("pcm16")
    wall = {k: [] for k in configs}
    fam = {k: {} for k in configs}
    for _ in range(args.rounds):
        for k, s in configs.items():
            e.set_pitch(s)
            e.sync()
            t0 = time.perf_counter()
            e.batch_fetch_encoded("pcm16")
            wall[k].append((time.perf_counter() - t0) * 1e6)
    e.profile_enable(True)
    for _ in range(args.rounds):
        for k, s in configs.items():
            e.set_pitch(s)
            e.profile_reset()
            e.batch_fetch_encoded("pcm16")
            for f, st in e.profile().items():
                fam[k].setdefault(f, []).append(st["ms"] * 1e3)
    e.profile_enable(False)
    print(f"pcm16 fetch of {B} rows x {Wb} samples at {hz} Hz; median of {args.rounds} interleaved rounds")
    for k in configs:
        med = {f: statistics.median(v) for f, v in fam[k].items()}
        w = statistics.median(wall[k])
        out[f"fetch_{k}"] = dict(wall_us=round(w, 1), wall_min_us=round(min(wall[k]), 1), wall_max_us=round(max(wall[k]), 1), families={f: round(v, 1) for f, v in med.items()})
        print(f"  pitch {k:3s}: wall {w:9.1f} us (min {min(wall[k]):.1f}, max {max(wall[k]):.1f})   " + "  ".join(f"{f} {v:.1f}" for f, v in med.items()))
    print(json.dumps(out))
    e.close()


if __name__ == "__main__":
    main()
