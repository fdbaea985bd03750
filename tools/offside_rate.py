#!/usr/bin/env python3
"""Cost of the offside kernels (include/eagle.h, eagle_post_offside; csrc/offside.hip): one JSON line.

    python tools/offside_rate.py [--rows 30000] [--reps 5] [--numpy-rows 2000]

A processed table of --rows rows is built by eagle_postprocess from constructed records: two teams of eleven outfield players round a 4-4-2 each, two
goalkeepers and the ball, everybody present on every row; the ball sits on a player for three frames and hops to another, so eagle_post_possession
gives a few thousand events.  The four launches of one eagle_post_offside call (vote, rows, totals, events) are timed over all rows: HIP events of the
profiling mode around the launches, --reps calls after a warm-up call, reported as the median with the minimum and the maximum.  Next to them stands the
time the numpy restatement (tests/offside_ref.py) takes on --numpy-rows of the same rows, scaled to the table.  A report, not a gate: nothing here is
compared with a threshold."""
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

FORM = [(20, 8), (18, 26), (18, 42), (20, 60), (45, 10), (43, 27), (43, 41), (45, 58), (70, 24), (70, 44), (57, 34)]
NAMES = ("offside_vote", "offside_rows", "offside_totals", "offside_events")


def records(n, seed=0):
    """n records of 22 players (ids 1 .. 22, slot s of team g is detection 11 g + s), two goalkeepers (ids 23, 24) and the ball"""
    r = np.random.default_rng(seed)
    k = 25
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = k, 1, 1
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    base = np.array([(x, y) for x, y in FORM] + [(105 - x, y) for x, y in FORM] + [(3, 34), (102, 34), (52, 34)], np.float64)
    pos = base[None] + r.normal(0, 2.0, (n, k, 2)) + np.cumsum(r.normal(0, 0.2, (n, 1, 2)), 0)
    holder = np.repeat(r.integers(0, 22, n // 3 + 1), 3)[:n]
    pos[:, k - 1] = pos[np.arange(n), holder]
    pos = np.clip(pos, 0, [105, 68])
    d, j = recs["det"], np.arange(k)
    d["reported"][:, :k], d["in_bounds"][:, :k], d["conf"][:, :k] = 1, 1, 0.9
    d["cls"][:, :k] = np.where(j == k - 1, 2, np.where(j >= 22, 1, 0))[None]
    d["id"][:, :k] = (j + 1)[None]
    d["bx1"][:, :k], d["bx2"][:, :k], d["by1"][:, :k], d["by2"][:, :k] = (4 * j)[None], (4 * j + 3)[None], 300, 340
    d["pitch_x"][:, :k], d["pitch_y"][:, :k] = pos[..., 0].astype(np.int32), pos[..., 1].astype(np.int32)
    return recs


def timed(h, reps, call):
    """ms of the launches accumulated under each of NAMES in one call: reps calls after one warm-up -> {name: {median, min, max}}"""
    call()
    ms = {k: [] for k in NAMES}
    for _ in range(reps):
        h.set_profiling(1)
        call()
        rows = h.kernel_times()
        h.set_profiling(0)
        for k in NAMES:
            ms[k].append(sum(x[1] for x in rows if x[0] == k))
    out = {k: {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(min(v)), 4), "ms_max": round(float(max(v)), 4)} for k, v in ms.items()}
    out["ms_median_sum"] = round(sum(o["ms_median"] for o in out.values()), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-rows", type=int, default=2000)
    a = ap.parse_args()
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    import offside_ref as OR
    t = h.postprocess(records(a.rows), 25, 1280, {i: 0 if i <= 11 else 1 for i in range(1, 23)})
    try:
        rows = len(t.rows)
        ev = h.possession(t, lib.possession_params(25))[3]
        p = lib.offside_params()
        res = timed(h, a.reps, lambda: h.offside(t, p))
        rec, mg, totals, clip = h.offside(t, p)
        oev = h.offside_events(t)
        res.update(reps=a.reps, rows=rows, members=int(len(totals)), keepers=int(clip[0]["n_keepers"]), events=int(len(ev)), passes=int((ev["kind"] == lib.EVENT_PASS).sum()),
                   direction=lib.OFFSIDE_DIR_NAMES[int(clip[0]["direction"])], ok_rows=[int((rec[:, g]["status"] == lib.OFFSIDE_OK).sum()) for g in (0, 1)],
                   verdicts={name: int((oev["verdict"] == v).sum()) for v, name in enumerate(lib.OFFSIDE_VERDICT_NAMES) if name})
        k = min(a.numpy_rows, rows)
        values = np.array(t.values)[:, :k]
        cols = [(int(c["kind"]), int(c["id"]), int(c["video"])) for c in t.columns]
        t0 = time.perf_counter()
        OR.offside(values, cols, t.team_mapping, OR.offside_params())
        dt = time.perf_counter() - t0
        res["numpy"] = {"rows": k, "seconds": round(dt, 3), "seconds_scaled_to_table": round(dt * rows / max(k, 1), 2)}
    finally:
        t.close()
    h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
