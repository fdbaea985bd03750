#!/usr/bin/env python3
"""Cost of the team-shape kernels and of the minimap's hull layer (include/eagle.h, eagle_post_team_shape / eagle_minimap_set_hulls; csrc/shape.hip,
csrc/minimap.hip): one JSON line.

    python tools/shape_rate.py [--rows 30000] [--players 20] [--reps 10] [--mm-rows 1000] [--batch 100]

A processed table of --rows rows is built by eagle_postprocess from constructed records (--players players split over two teams, 2 goalkeepers and the
ball on a random walk: tools/occupancy_rate.py's table) and eagle_post_team_shape is called --reps times after a warm-up call.  Each launch is timed
separately (HIP events of the profiling mode around the launch of ONE call): median, minimum and maximum; the statistics kernel also in GB/s against the
16 bytes a member cell reads.  The wall time of a whole call (upload of the member list, two launches, one wait) is reported beside them, and so are
eagle_post_possession and eagle_post_occupancy (R = 1, sigma 2 m, default selections) on the same table, summed over their launches.  The rows, columns
and members used are in the output.  Then the layered minimap at --mm-rows rows, --batch pictures per call as BGR at 8 pixels per metre, layers = 7
against layers = 15 (tools/trails_rate.py's "all" configuration, and the same with the hulls under it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from eagle_amd import lib, occupancy as oc, shape, weights  # noqa: E402
from control_rate import records, timed  # noqa: E402


def wall_us(call, reps):
    call()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return round((time.perf_counter() - t0) / reps * 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--players", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mm-rows", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=100)
    a = ap.parse_args()
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    tm = {i + 1: i % 2 for i in range(a.players)}
    res = {"reps": a.reps}
    t = h.postprocess(records(a.rows, a.players, 2), 25, 1280, tm)
    try:
        groups = shape.member_columns(t.columns, t.team_mapping)
        members, n = len(groups[0]) + len(groups[1]), len(t.rows)
        res.update(rows=n, columns=len(t.columns), members=[len(groups[0]), len(groups[1])])
        call = lambda: h.L.eagle_post_team_shape(h._h, t._t)
        st = timed(h, "shape_stats", a.reps, call)
        st["GB_per_s"] = round(16.0 * members * n / (st["ms_median"] * 1e-3) / 1e9, 1)
        res["shape_stats"], res["shape_hull"] = st, timed(h, "shape_hull", a.reps, call)
        res["team_shape_wall_us_per_call"] = wall_us(call, a.reps)
        rec, _ = h.team_shape(t)
        res["hull_n_mean"] = round(float(rec["hull_n"].mean()), 2)
        pp = lib.possession_params(25)
        pcall = lambda: h.L.eagle_post_possession(h._h, t._t, pp)
        res["possession"] = {k: timed(h, k, a.reps, pcall) for k in ("possession_cand", "possession_scan")}
        res["possession_wall_us_per_call"] = wall_us(pcall, a.reps)
        off, sc, _ = oc.default_selections(t.columns, t.team_mapping)
        off_a, sc_a = np.array(off, np.int32), np.array(sc, np.int32)
        op = lib.occupancy_params(25, 1, 2.0)
        ocall = lambda: h.L.eagle_post_occupancy(h._h, t._t, op, off_a.ctypes.data, sc_a.ctypes.data, len(off) - 1)
        res["occupancy_R1_sigma2"] = {k: timed(h, k, a.reps, ocall) for k in ("occupancy_hist", "occupancy_blur_x", "occupancy_blur_y", "occupancy_norm")}
        res["occupancy_wall_us_per_call"] = wall_us(ocall, a.reps)
    finally:
        t.close()
    # ---- the layered minimap with and without the hulls ----
    B = min(a.batch, a.mm_rows)
    t = h.postprocess(records(a.mm_rows, a.players, 2), 25, 1280, tm)
    d_out = None
    try:
        h.possession(t, lib.possession_params(25))
        h.team_shape(t)
        h.set_hulls(t, 1)
        sel = [c for c, k in enumerate(t.columns) if not k["video"] and int(k["kind"]) in (lib.POST_PLAYER, lib.POST_GOALKEEPER, lib.POST_BALL)]
        h.minimap_set_trails(t, lib.trail_params(window=25, pass_hold=25), sel)
        w, hh = lib.minimap_size(lib.minimap_params(8))
        d_out = h.upload(np.zeros(B * hh * w * 3, np.uint8))
        first = max(len(t.rows) - B, 0)
        res["minimap"] = {"rows": len(t.rows), "batch": B, "frame": [hh, w]}
        for name, layers in (("layers_7", 7), ("layers_15", 15)):
            par = lib.minimap_params(8, layers=layers)
            draw = lambda: h.minimap_device(t, d_out, par, first, B, "bgr")
            ev = timed(h, "minimap_layers", a.reps, draw)
            ev.update(pictures_per_s=round(B / (ev["ms_median"] * 1e-3)), wall_us_per_call=wall_us(draw, a.reps))
            res["minimap"][name] = ev
    finally:
        if d_out is not None:
            h.free(d_out)
        t.close()
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
