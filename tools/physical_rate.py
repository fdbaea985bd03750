#!/usr/bin/env python3
"""Cost of the physical-report kernels (include/eagle.h, eagle_post_physical; csrc/physical.hip): one JSON line.

    python tools/physical_rate.py [--rows 30000] [--players 20] [--reps 10]

A processed table of --rows rows is built by eagle_postprocess from constructed records (--players players split over two teams, 2 goalkeepers and the
ball on a random walk: tools/occupancy_rate.py's table), its velocities are computed and eagle_post_physical is called --reps times after a warm-up call,
with thresholds low enough for the random walk to make efforts.  Each of the three launches is timed separately (HIP events of the profiling mode around
the launch of ONE call): median, minimum and maximum; the rows kernel also in GB/s against the 42 bytes it moves per person and row (16 read, 26 written).
Next to them: post_velocity on the same table, in GB/s against its 32 bytes per cell (the bandwidth yardstick: the rows kernel has its access pattern), the
wall time of a whole eagle_post_physical call (uploads, three launches, two waits, the records fetched), and the numpy restatement of the contract
(tests/physical_ref.py, scan formulation) on the host over the same velocities.  The rows, columns, persons and efforts used are in the output."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eagle_amd import lib, weights  # noqa: E402
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
    a = ap.parse_args()
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    tm = {i + 1: i % 2 for i in range(a.players)}
    res = {"reps": a.reps}
    t = h.postprocess(records(a.rows, a.players, 2), 25, 1280, tm)
    try:
        n, cols = len(t.rows), len(t.columns)
        kp = lib.kinematics_params(25)
        vcall = lambda: h.L.eagle_post_velocities(h._h, t._t, kp)
        vel = timed(h, "post_velocity", a.reps, vcall)
        vel["GB_per_s"] = round(32.0 * cols * n / (vel["ms_median"] * 1e-3) / 1e9, 1)
        res["post_velocity"] = vel
        args = dict(zone_edges=(0.5, 1.0, 2.0, 4.0), effort_speed=(2.0, 4.0), accel=1.0, min_frames=5)
        p = lib.load_params(25, **args)
        call = lambda: h.L.eagle_post_physical(h._h, t._t, p)
        _, _, _, totals, efforts = h.physical(t, p)
        persons = len(totals)
        res.update(rows=n, columns=cols, persons=persons, efforts=len(efforts), params={k: list(v) if isinstance(v, tuple) else v for k, v in args.items()})
        rk = timed(h, "physical_rows", a.reps, call)
        rk["GB_per_s"] = round(42.0 * persons * n / (rk["ms_median"] * 1e-3) / 1e9, 1)
        res["physical_rows"], res["physical_scan"], res["physical_effort"] = rk, timed(h, "physical_scan", a.reps, call), timed(h, "physical_effort", a.reps, call)
        res["physical_wall_us_per_call"] = wall_us(call, a.reps)
        # the numpy restatement on the host, over the velocities the library computed
        import physical_ref as PR
        v = h.velocities(t, 25)
        columns = [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in t.columns]
        t0 = time.perf_counter()
        ref = PR.physical(v, t.rows, columns, 25, None, args["zone_edges"], args["effort_speed"], args["accel"], (args["min_frames"],) * 2)
        res["numpy_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["equal_to_restatement"] = bool(ref["totals"].tobytes() == totals.tobytes() and ref["efforts"].tobytes() == efforts.tobytes())
    finally:
        t.close()
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
