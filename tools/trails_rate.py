#!/usr/bin/env python3
"""Cost of the minimap's trail, pass-arrow and owner layers (include/eagle.h, eagle_minimap_set_trails; csrc/minimap.hip, csrc/trails.hip): one JSON line.

    python tools/trails_rate.py [--rows 1000] [--batch 100] [--reps 10]

The table of tools/minimap_rate.py (23 pitch columns: 4 corners, 16 players, 2 goalkeepers, the ball) with a possession result; --batch rows at a time are
drawn into HBM as BGR at 8 pixels per metre (872 x 576).  Reported in one process: pictures per second (HIP events of the profiling mode around the
launches of a call, mean of --reps calls after a warm-up) of the plain minimap, of trails over 25 and over 125 rows, of the pass arrows with the owner
ring, and of all layers together.  The trails run on the 19 entity columns (16 players, 2 goalkeepers, the ball): of the table's 23 pitch columns the four
corner columns cannot be selected.  The event span ("minimap" / "minimap_layers") covers the sites and the draw launch only; what a layered call does in
front of them (the uploads, trail_points_kernel, trail_events_kernel and a stream synchronisation) is outside it, so the wall time of a whole call is
reported beside it ("wall_us_per_call", "wall_pictures_per_s"; for the plain minimap too).  The plain figure is the one tools/minimap_rate.py reports as
bgr / plain; the parent commit's plain figure comes from running that tool on a checkout of the parent."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from eagle_amd import lib, weights  # noqa: E402
from minimap_rate import records  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    B = min(a.batch, a.rows)
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    t = h.postprocess(records(a.rows), 25, 1280, {i + 1: i % 2 for i in range(16)})
    _, owner, _, ev = h.possession(t, lib.possession_params(25))
    sel = [c for c, k in enumerate(t.columns) if not k["video"] and int(k["kind"]) in (lib.POST_PLAYER, lib.POST_GOALKEEPER, lib.POST_BALL)]
    w, hh = lib.minimap_size(lib.minimap_params(8))
    res = {"rows": len(t.rows), "selected_columns": len(sel), "events": len(ev), "owned_rows": int((owner >= 0).sum()), "batch": B, "frame": [hh, w], "reps": a.reps}
    d_out = h.upload(np.zeros(B * hh * w * 3, np.uint8))
    first = max(len(t.rows) - B, 0)                       # the last rows of the table: every trail has its whole window behind it
    try:
        for name, layers, window in (("plain", 0, 25), ("trails_25", 1, 25), ("trails_125", 1, 125), ("passes_owner", 6, 25), ("all", 7, 25)):
            h.minimap_set_trails(t, lib.trail_params(window=window, pass_hold=25), sel)
            par = lib.minimap_params(8, layers=layers)
            h.minimap_device(t, d_out, par, first, B, "bgr")                    # warm-up
            h.set_profiling(1)
            for _ in range(a.reps):
                h.minimap_device(t, d_out, par, first, B, "bgr")
            row = [x for x in h.kernel_times() if x[0] == ("minimap_layers" if layers else "minimap")][0]
            h.set_profiling(0)
            us = 1e3 * row[1] / row[2]
            t0 = time.perf_counter()
            for _ in range(a.reps):
                h.minimap_device(t, d_out, par, first, B, "bgr")                # (the entry returns when the pictures are complete)
            wall = (time.perf_counter() - t0) / a.reps * 1e6
            res[name] = {"us_per_call": round(us, 1), "pictures_per_s": round(B / (us * 1e-6)), "wall_us_per_call": round(wall, 1),
                         "wall_pictures_per_s": round(B / (wall * 1e-6))}
    finally:
        h.free(d_out)
        t.close()
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
