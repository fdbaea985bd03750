#!/usr/bin/env python3
"""Cost of the goal-view launches (include/eagle.h, eagle_op_goal_view; csrc/goalview.hip): one JSON line.

    python tools/goalview_rate.py [--rows 30000] [--reps 5] [--limit 240]

One workload: --rows rows of 22 players (11 a side) on a random walk, two keepers, the ball and an owner per row, the grid over every row for the owner's
group, at R = 1, 2 and 4 cells per metre and with either form of the grid kernel's weights: `direct` (a division per open slice of a cell) and `table`
(a prefix table int32 [2][68 R][105 R][65] built once per call, two reads per open run).  Per launch group (prepare, points, rows and totals, table, grid,
the whole call) device events, two warm-up calls, then --reps calls, reported as the median with the minimum and the maximum (milliseconds); table plus grid
decides the form; the grid also in nanoseconds per evaluated cell.  The grid stays on the device.  `check`: 40 rows of the same walk against
tests/goalview_ref.py, byte for byte, in both forms.

Every step runs in a process of its own under a time limit (--limit seconds); after a step that fails, is killed or runs out of time nothing more is
started and the line says where it stopped.  A report, not a gate: nothing here is compared with a threshold."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORMS = (("direct", 1), ("table", 2))


def walk(rows, seed=0):
    """-> (values [25][rows][2], columns, mapping, owner): 22 players, team 0 on the left, two keepers, the ball on its owner"""
    r = np.random.default_rng(seed)
    x0 = np.array([r.uniform(15, 95) for _ in range(22)] + [4.0, 101.0])
    y0 = np.concatenate([r.uniform(8, 60, 22), [34.0, 34.0]])
    pos = np.stack([x0, y0], 1)[:, None, :] + np.cumsum(r.normal(0, 0.25, (24, rows, 2)), 1)
    for k, hi in ((0, 105.0), (1, 68.0)):                             # folded back into the pitch
        pos[:, :, k] = hi - np.abs(np.mod(pos[:, :, k], 2 * hi) - hi)
    owner = np.repeat(r.integers(0, 22, rows // 25 + 1), 25)[:rows].astype(np.int32)
    ball = pos[owner, np.arange(rows)] + 0.3
    cols = [(0, 1 + i, 0) for i in range(22)] + [(1, 90, 0), (1, 91, 0), (2, 0, 0)]
    return np.concatenate([pos, ball[None]]), cols, {1 + i: i % 2 for i in range(22)}, owner


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def step(rows, R, form, reps):
    from eagle_amd import lib
    values, cols, mp, owner = walk(rows)
    p = lib.goal_view_params(lib.OFFSIDE_DIR_RIGHT, group=-1, cells_per_metre=R, form=form, grid_rows=rows)
    ms = []
    for k in range(2 + reps):
        out = lib.op_goal_view(values, cols, mp, p, owner, times=True, fetch_grid=False)
        if k >= 2:
            ms.append([out["times"][n] for n in lib.GOALVIEW_TIMES])
    ms = np.array(ms)
    res = {n: stats(ms[:, i]) for i, n in enumerate(lib.GOALVIEW_TIMES)}
    res["table_plus_grid"] = stats(ms[:, 3] + ms[:, 4])
    # the cells within max_range of a goal and beyond min_depth, of 68 R x 105 R
    i, j = np.meshgrid((np.arange(105 * R) + 0.5) / R, (np.arange(68 * R) + 0.5) / R)
    cells = int((((105.0 - i) ** 2 + (34.0 - j) ** 2 <= 1600.0) & (105.0 - i >= 1.0)).sum())
    res["cells_per_row"] = cells
    res["grid_ns_per_cell"] = round(1e6 * res["grid"]["median"] / (rows * cells), 4)
    res["members_evaluated"] = int((out["status"] == 0).sum())
    return res


def check(rows):
    import goalview_ref as GR
    from eagle_amd import lib
    values, cols, mp, owner = walk(rows)
    same = True
    for R in (1, 2):
        exp = GR.goal_view(values, cols, mp, GR.goal_view_params(1, group=-1, cells_per_metre=R, grid_rows=rows), owner)
        for form in (0, 1, 2):
            got = lib.op_goal_view(values, cols, mp, lib.goal_view_params(1, group=-1, cells_per_metre=R, form=form, grid_rows=rows), owner)
            same = same and all(got[k].tobytes() == exp[k].tobytes() for k in ("rows", "open", "mask", "status", "totals", "grid"))
    return {"rows": rows, "equal_to_reference": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # R,form or `check`: one step, in this process
    a = ap.parse_args()
    if a.step is not None:
        if a.step == "check":
            print(json.dumps(check(40)))
        else:
            R, form = (int(v) for v in a.step.split(","))
            print(json.dumps(step(a.rows, R, form, a.reps)))
        return 0
    res = {"rows": a.rows, "players": 22, "reps": a.reps, "workloads": []}
    steps = [("check", None)] + [(f"{R},{code}", (R, name)) for R in (1, 2, 4) for name, code in FORMS]
    for arg, what in steps:
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--reps", str(a.reps), "--step", arg], capture_output=True, text=True,
                                  timeout=a.limit)
            failed = None if done.returncode == 0 else f"exit status {done.returncode}: {done.stderr.strip()[-300:]}"
        except subprocess.TimeoutExpired:
            failed = f"no result within {a.limit} s"
        if failed:
            res["stopped_at"] = {"step": arg, "why": failed}              # nothing more is started
            break
        out = json.loads(done.stdout.strip().splitlines()[-1])
        if what is None:
            res["check"] = out
        else:
            res["workloads"].append({"cells_per_metre": what[0], "form": what[1], **out})
    print(json.dumps(res), flush=True)
    return 1 if "stopped_at" in res else 0


if __name__ == "__main__":
    sys.exit(main())
