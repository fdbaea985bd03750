#!/usr/bin/env python3
"""Cost of the possession kernels (include/eagle.h, eagle_post_possession; csrc/possession.hip): one JSON line.

    python tools/possession_rate.py [--rows 16384 131072] [--players 24] [--reps 10]
    python tools/possession_rate.py --op-rows 1048576 [--reps 5]          # under a kernel trace: the operator entry on a constructed table

For each --rows value a processed table is built by eagle_postprocess from constructed records (--players players, 2 goalkeepers and the ball on a
random walk: 26 person columns by default) and eagle_post_possession is called --reps times after a warm-up call.  The two stages are timed separately:
HIP events of the profiling mode around the launch of ONE call, reported as the median with the minimum and the maximum.  The candidate stage is given
in GB/s against the bytes it moves (the ball's and the persons' 16-byte cells read once, 13 bytes per row written), next to the velocity kernel's
recorded rate (the same access pattern) and the HBM peak; the scan stage in rows per second.  The numpy contract (tests/possession_ref.py) is timed on
the same table for scale.  A record holds 300 detections (about 22 KB), so a table of 2^20 rows cannot be built from records on an ordinary host:
--op-rows runs eagle_op_possession on a constructed table of that many rows --reps times and prints only the wall time; its per-kernel times come from
a kernel trace of that run (rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eagle_amd import lib, weights  # noqa: E402
from control_rate import records, timed  # noqa: E402

HBM_TBS = 6.3
VELOCITY_TBS = 3.6          # docs/experiments.md, "Pitch control (K22)": post_velocity_kernel on a 203 MB table


def constructed(rows, persons, seed=0):
    """values [persons + 1][rows][2]: persons on a random walk, the ball hopping between them every few rows"""
    r = np.random.default_rng(seed)
    v = np.empty((persons + 1, rows, 2), np.float64)
    for c in range(persons):
        v[c] = np.array([r.uniform(5, 100), r.uniform(5, 63)]) + np.cumsum(r.normal(0, 0.05, (rows, 2)), 0)
    who = np.repeat(r.integers(0, persons, rows // 8 + 1), 8)[:rows]
    v[persons] = v[who, np.arange(rows)] + r.normal(0, 0.7, (rows, 2))
    cols = [(lib.POST_PLAYER, c + 1, 0) for c in range(persons)] + [(lib.POST_BALL, 0, 0)]
    return v, np.arange(rows, dtype=np.int32), cols, {c + 1: c % 2 for c in range(persons)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1 << 14, 1 << 17])
    ap.add_argument("--players", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--op-rows", type=int, default=0)
    a = ap.parse_args()
    if a.op_rows:
        v, f, cols, tm = constructed(a.op_rows, a.players + 2)
        p = lib.possession_params(25)
        wall = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            out = lib.op_possession(v, f, cols, tm, p)
            wall.append(time.perf_counter() - t0)
        print(json.dumps({"op_rows": a.op_rows, "person_columns": a.players + 2, "events": out[4], "owned_rows": int((out[1] >= 0).sum()),
                          "wall_s_median_incl_copies": round(float(np.median(wall[1:])), 4)}))
        return
    import possession_ref as PR
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    res = {"reps": a.reps, "hbm_TB_per_s": HBM_TBS, "velocity_kernel_TB_per_s": VELOCITY_TBS, "tables": []}
    try:
        for rows in a.rows:
            t = h.postprocess(records(rows, a.players, 2), 25, 1280, {i + 1: i % 2 for i in range(a.players)})
            try:
                p = lib.possession_params(25)
                call = lambda: h.L.eagle_post_possession(h._h, t._t, p)
                persons = sum(1 for k in t.columns if not k["video"] and int(k["kind"]) in (lib.POST_PLAYER, lib.POST_GOALKEEPER))
                n = len(t.rows)
                cand = timed(h, "possession_cand", a.reps, call)
                scan = timed(h, "possession_scan", a.reps, call)
                moved = n * (16.0 * (persons + 1) + 13.0)
                cand.update(MB=round(moved / 1e6, 2), GB_per_s=round(moved / (cand["ms_median"] * 1e-3) / 1e9, 1))
                cand["of_velocity_kernel"] = round(cand["GB_per_s"] / (VELOCITY_TBS * 1e3), 3)
                scan.update(rows_per_s=float("%.4g" % (n / (scan["ms_median"] * 1e-3))), us_per_chunk_of_1024=round(scan["ms_median"] * 1e3 / max(1, (n + 1023) // 1024), 3))
                _, owner, _, ev = h.possession(t, p)
                cols = [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in t.columns]
                values = np.array(t.values)
                t0 = time.perf_counter()
                exp = PR.possession(values, t.rows, cols, t.team_mapping, 25)
                numpy_s = time.perf_counter() - t0
                assert np.array_equal(owner, exp["owner"]) and ev.tobytes() == exp["events"].tobytes()
                res["tables"].append({"rows": n, "columns": len(t.columns), "person_columns": persons, "events": len(ev), "owned_rows": int((owner >= 0).sum()),
                                      "candidate": cand, "scan": scan, "numpy_contract_ms": round(numpy_s * 1e3, 2)})
            finally:
                t.close()
    finally:
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
