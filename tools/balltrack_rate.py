#!/usr/bin/env python3
"""Cost of the ball-track launches (include/eagle.h, eagle_op_ball_track / eagle_ball_track; csrc/balltrack.hip): one JSON line.

    python tools/balltrack_rate.py [--frames 30000] [--reps 7] [--context]

Clips of --frames frames with 1, 3 and 8 candidates on every frame (a true path on a random walk under distractors anywhere in a 1280 x 720 picture),
as one shot and cut into 64.  Per clip eagle_op_ball_track runs with either recovery of the chosen nodes, pointer doubling and the single-lane chase:
device events around the recurrence with its chaining, around the recovery and around the row / prefix-sum / tracklet launches, two warm-up calls, then
--reps calls, reported as the median with the minimum and the maximum (milliseconds), the recurrence also per frame.  With one candidate on every frame
a shot is one piece of the timeline and one wave walks it: the recurrence is bound by latency by construction, so the time per frame is what there is
to report and no share of any peak.  --context: records holding the same candidates and two players go through eagle_ball_track and eagle_postprocess
of a handle (wall clock, host staging included), so a reader sees the share.  A report, not a gate: nothing here is compared with a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eagle_amd import lib  # noqa: E402

PARTS = ("recurrence", "recovery", "rows", "all")


def clip(n, cands, seed=0):
    """-> (counts, positions in half pixels, cq): candidate 0.. in descending confidence, the true ball somewhere among them"""
    r = np.random.default_rng(seed)
    path = np.clip(np.cumsum(r.integers(-12, 13, (n, 2)), 0) + (1280, 720), 0, (2560, 1440))
    pos = np.stack([r.integers(0, 2561, (n, cands)), r.integers(0, 1441, (n, cands))], 2)
    pos[np.arange(n), r.integers(0, cands, n)] = path
    cq = -np.sort(-r.integers(300, 1025, (n, cands)), 1)
    return np.full(n, cands, np.int32), pos.reshape(-1, 2).astype(np.int32), cq.reshape(-1).astype(np.int32)


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def measure(counts, pos, cq, p, cuts, recover, reps):
    ms = []
    for k in range(2 + reps):
        fr, tr, cl, t = lib.op_ball_track(counts, pos, cq, p, cuts, recover=recover, times=True)
        if k >= 2:
            ms.append(t.copy())
    ms = np.array(ms)
    out = {name: stats(ms[:, i]) for i, name in enumerate(PARTS)}
    out["recurrence_us_per_frame"] = round(1000.0 * out["recurrence"]["median"] / len(counts), 4)
    return out, (fr, tr, cl)


def records(counts, pos, cq):
    n, c = len(counts), int(counts[0])
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = c + 2, 1, 1
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    d = recs["det"]
    q, conf = pos.reshape(n, c, 2), cq.reshape(n, c) / 1024.0
    for j in range(c):
        d["reported"][:, j], d["in_bounds"][:, j], d["cls"][:, j], d["id"][:, j], d["conf"][:, j] = 1, 1, 2, j, conf[:, j]
        d["bx1"][:, j], d["bx2"][:, j], d["by2"][:, j] = q[:, j, 0] // 2, q[:, j, 0] - q[:, j, 0] // 2, q[:, j, 1] // 2
        d["pitch_x"][:, j], d["pitch_y"][:, j] = q[:, j, 0] * 105 // 2561, q[:, j, 1] * 68 // 1441
    for j, x in ((c, 30), (c + 1, 70)):
        d["reported"][:, j], d["in_bounds"][:, j], d["cls"][:, j], d["id"][:, j], d["conf"][:, j] = 1, 1, 0, j - c + 1, 0.9
        d["bx1"][:, j], d["bx2"][:, j], d["by1"][:, j], d["by2"][:, j], d["pitch_x"][:, j], d["pitch_y"][:, j] = 10 * x, 10 * x + 20, 300, 340, x, 34
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--context", action="store_true")
    a = ap.parse_args()
    n = a.frames
    p = lib.ball_track_params(25, 1280)
    res = {"frames": n, "reps": a.reps, "clips": []}
    for cands in (1, 3, 8):
        counts, pos, cq = clip(n, cands)
        for shots in (1, 64):
            cuts = [k * n // shots for k in range(1, shots)]
            row = {"candidates": cands, "shots": shots}
            for name, recover in (("doubling", lib.BALL_RECOVER_DOUBLING), ("chase", lib.BALL_RECOVER_CHASE)):
                row[name], out = measure(counts, pos, cq, p, cuts, recover, a.reps)
            row.update(frames_chosen=int(out[2][0]["frames_chosen"]), tracklets=int(out[2][0]["tracklets"]))
            res["clips"].append(row)
        if a.context:
            recs = records(counts, pos, cq)
            h = lib.Handle(batch=2, frame_h=720, frame_w=1280)
            try:
                wall = {"ball_track": [], "postprocess": [], "postprocess_ball": []}
                for k in range(4):
                    t0 = time.perf_counter()
                    fr = h.ball_track(recs, p)[0]
                    t1 = time.perf_counter()
                    h.postprocess(recs, 25, 1280, None).close()
                    t2 = time.perf_counter()
                    h.postprocess(recs, 25, 1280, None, ball_det=fr["det"]).close()
                    t3 = time.perf_counter()
                    if k:
                        wall["ball_track"].append(1000 * (t1 - t0)); wall["postprocess"].append(1000 * (t2 - t1)); wall["postprocess_ball"].append(1000 * (t3 - t2))
                res["clips"][-2]["handle_wall_ms"] = {k: stats(v) for k, v in wall.items()}
            finally:
                h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
