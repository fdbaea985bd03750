#!/usr/bin/env python3
"""Cost of the team clustering (include/eagle.h, eagle_team_cluster / eagle_op_team_cluster_ids; csrc/kits.hip): one JSON line.

    python tools/kits_rate.py [--frames 200] [--players 22] [--reps 7]

A clip of --frames frames of 1280 x 720 resident in HBM, --players boxes of about 40 x 100 on every frame (seeded noise frames with two kit colours
painted into the boxes).  Through a handle, wall clock around the synchronous calls (the upload of the crop list, the launches and the download of the
records included): eagle_team_cluster, and in the same run eagle_team_colors, the reference's rule, on the same crops.  Through the operator entry,
device events around the histogram launch and around the four clustering launches.  Then the clustering alone from given sums at 64, 256 and 1024 ids,
all of them voters (device events).  Two warm-up calls, then --reps calls, reported as the median with the minimum and the maximum in milliseconds.
A report, not a gate: nothing here is compared with a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eagle_amd import lib  # noqa: E402

FH, FW = 720, 1280


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def clip(n, players, seed=0):
    r = np.random.default_rng(seed)
    base = r.integers(0, 256, (4, FH, FW, 3), dtype=np.uint8)
    frames = base[np.arange(n) % 4].copy()
    kits = np.array([(125, 44, 22), (235, 170, 90)], np.int64)
    crops, slots = [], []
    for i in range(n):
        for j in range(players):
            w, h = int(r.integers(34, 47)), int(r.integers(90, 111))
            x, y = int(r.integers(0, FW - w)), int(r.integers(0, FH - h))
            frames[i, y:y + h, x:x + w] = np.clip(kits[j % 2] + r.integers(-10, 11, (h, w, 3)), 0, 255)
            crops.append((i, x, y, x + w, y + h))
            slots.append(j)
    return frames, np.array(crops, np.int32), np.array(slots, np.int32)


def ids(n, seed=1):
    r = np.random.default_rng(seed)
    base = np.zeros((2, lib.KIT_BINS), np.int64)
    base[0, [9, 24, 33]], base[1, [0, 15, 31]] = (9000, 2000, 1000), (7000, 3000, 2000)
    used = r.integers(3, 200, n)
    return (base[r.integers(0, 2, n)] + r.integers(0, 100, (n, lib.KIT_BINS))) * used[:, None], used.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--players", type=int, default=22)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    frames, crops, slots = clip(a.frames, a.players)
    res = {"frames": a.frames, "crops": len(crops), "ids": a.players, "reps": a.reps}
    p = lib.kit_params()
    h = lib.Handle(batch=1, frame_h=FH, frame_w=FW)
    try:
        d = h.upload(frames)
        wall = {"team_cluster": [], "team_colors": []}
        for k in range(2 + a.reps):
            t0 = time.perf_counter()
            out = h.team_cluster(d, a.frames, crops, slots, a.players, p)
            t1 = time.perf_counter()
            h.team_colors(d, a.frames, crops)
            t2 = time.perf_counter()
            if k >= 2:
                wall["team_cluster"].append(1000 * (t1 - t0)); wall["team_colors"].append(1000 * (t2 - t1))
        h.free(d)
        res["handle_wall_ms"] = {k: stats(v) for k, v in wall.items()}
        res["crops_used"], res["teams"] = int(out[1]["used"].sum()), [int((out[1]["team"] == k).sum()) for k in (0, 1)]
    finally:
        h.close()
    ms = np.array([lib.op_team_cluster(frames, crops, slots, a.players, p, times=True)[3] for _ in range(1 + min(a.reps, 3))][1:])
    res["device_ms"] = {"histograms": stats(ms[:, 0]), "clustering": stats(ms[:, 1])}
    res["histograms_us_per_crop"] = round(1000.0 * res["device_ms"]["histograms"]["median"] / len(crops), 4)
    res["clustering_alone_ms"] = {}
    for n in (64, 256, 1024):
        sums, used = ids(n)
        t = [lib.op_team_cluster_ids(sums, used, p, times=True)[2][1] for _ in range(2 + a.reps)][2:]
        res["clustering_alone_ms"][str(n)] = stats(t)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
