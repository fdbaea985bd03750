#!/usr/bin/env python3
"""Cost of the ball-flight launches (include/eagle.h, eagle_op_ball_flights; csrc/flights.hip): one JSON line.

    python tools/flights_rate.py [--rows 30000] [--reps 7] [--limit 120]

Two workloads, a ball path of --rows rows (passes, carries and rests with 0.15 m jitter and 2 % displaced samples) as one run and the same rows cut into 64
runs by absent cells, each at L = 32, 64 and 128 and with either layout of the cost table: end-major c[end][k] (the walk's loads are contiguous, the
cost kernel's stores strided) and k-major c[k][end] (the reverse).  Per launch group (prepare, cost, walk, path, fit, events, the whole call) device
events, two warm-up calls, then --reps calls, reported as the median with the minimum and the maximum (milliseconds); cost plus walk decides the layout;
the walk also in microseconds per row: one wave walks a run, so it is bound by latency by construction and the time per row is what there is to report.
`check`: the first 600 rows as a table of their own against tests/flights_ref.py, bit for bit.

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

LAYOUTS = (("end_major", 1), ("k_major", 2))


def path(rows, runs, seed=0, fps=25.0):
    """-> (values [2][rows][2]: the ball and one player, frames, columns)"""
    r = np.random.default_rng(seed)
    vel = np.zeros((rows, 2))
    at, kind = 0, 0
    while at < rows:
        n = int(r.integers(12, 45)) if kind % 3 == 0 else int(r.integers(15, 50)) if kind % 3 == 1 else int(r.integers(10, 40))
        speed = r.uniform(8, 22) if kind % 3 == 0 else r.uniform(2, 6) if kind % 3 == 1 else 0.0
        ang = r.uniform(0, 2 * np.pi)
        vel[at:at + n] = speed * np.array([np.cos(ang), np.sin(ang)])
        at += n
        kind += 1
    pos = np.cumsum(vel / fps, 0) + (52.5, 34.0)
    for k, hi in ((0, 105.0), (1, 68.0)):                             # folded back into the pitch: a reflection at the edge
        pos[:, k] = hi - np.abs(np.mod(pos[:, k], 2 * hi) - hi)
    ball = pos + r.normal(0.0, 0.15, (rows, 2))
    hit = r.choice(np.arange(2, rows - 2, 4), rows // 50, replace=False)
    ang = r.uniform(0, 2 * np.pi, len(hit))
    ball[hit] += 3.0 * np.stack([np.cos(ang), np.sin(ang)], 1)
    for k in range(1, runs):
        ball[k * rows // runs] = np.nan
    values = np.stack([ball, pos + (0.6, 0.4)])
    return values, np.arange(rows, dtype=np.int32), [(2, 0, 0), (0, 7, 0)]


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def step(rows, runs, L, layout, reps):
    from eagle_amd import lib
    values, frames, cols = path(rows, runs)
    p = lib.flight_params(25.0, 25, max_rows=L, layout=layout)
    ms = []
    for k in range(2 + reps):
        out = lib.op_ball_flights(values, frames, cols, p, times=True)
        if k >= 2:
            ms.append([out["times"][n] for n in lib.FLIGHT_TIMES])
    ms = np.array(ms)
    res = {n: stats(ms[:, i]) for i, n in enumerate(lib.FLIGHT_TIMES)}
    res["cost_plus_walk"] = stats(ms[:, 1] + ms[:, 2])
    res["walk_us_per_row"] = round(1000.0 * res["walk"]["median"] / rows, 4)
    t = out["totals"][0]
    res.update(flights=int(t["flights"]), kicks=int(t["kicks"]), spikes=int(t["spikes"]), capped=int(t["capped"]))
    return res


def check(rows):
    import flights_ref as FR
    from eagle_amd import lib
    values, frames, cols = path(rows, 4)
    exp = FR.flights(values, frames, cols, FR.params(25.0, 25))
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    same = True
    for layout in (0, 1, 2):
        got = lib.op_ball_flights(values, frames, cols, lib.flight_params(25.0, 25, layout=layout))
        same = same and all(np.array_equal(bits(got[k]), bits(exp[k])) for k in ("fitted", "velocity")) and all(got[k].tobytes() == exp[k].tobytes() for k in
                                                                                                                 ("seg", "flags", "flights", "kicks", "totals"))
    return {"rows": rows, "flights": len(exp["flights"]), "kicks": len(exp["kicks"]), "equal_to_reference": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)      # runs,L,layout or `check`: one step, in this process
    a = ap.parse_args()
    if a.step is not None:
        if a.step == "check":
            print(json.dumps(check(600)))
        else:
            runs, L, layout = (int(v) for v in a.step.split(","))
            print(json.dumps(step(a.rows, runs, L, layout, a.reps)))
        return 0
    res = {"rows": a.rows, "reps": a.reps, "workloads": []}
    steps = [("check", None)] + [(f"{runs},{L},{code}", (runs, L, name)) for runs in (1, 64) for L in (32, 64, 128) for name, code in LAYOUTS]
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
            res["workloads"].append({"runs": what[0], "L": what[1], "layout": what[2], **out})
    print(json.dumps(res))
    return 1 if "stopped_at" in res else 0


if __name__ == "__main__":
    sys.exit(main())
