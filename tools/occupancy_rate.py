#!/usr/bin/env python3
"""Cost of the occupancy kernels (include/eagle.h, eagle_post_occupancy / eagle_occupancy_picture; csrc/occupancy.hip): one JSON line.

    python tools/occupancy_rate.py [--rows 30000] [--players 22] [--reps 10]
    python tools/occupancy_rate.py --op-rows 1048576 [--reps 5]            # under a kernel trace: the operator entry on a constructed table

A processed table of --rows rows is built by eagle_postprocess from constructed records (--players players, 2 goalkeepers and the ball on a random
walk: 23 people + ball by default is --players 21) and eagle_post_occupancy is called --reps times after a warm-up call with the default selections
(one map per person, one per team, the ball) for R = 1, 2, 4 and sigma 0 and 2 m.  Each launch is timed separately: HIP events of the profiling mode
around the launch of ONE call, reported as the median with the minimum and the maximum.  The histogram stage is given in member-rows per second and in
GB/s against the 20 bytes a member row reads (a 16-byte cell and a frame number), next to the velocity kernel's recorded rate (the same access
pattern); the two blur passes in GB/s against a plane read and a plane written and in cell-taps per second; the byte form in GB/s.  The library ships
ONE histogram form, global integer atomics behind a wave-level merge of equal cells, at every R; `atomics_per_member_row` says what the merge leaves of
the table at hand (computed on the host from the table: runs of equal cell within a wave's 64 rows).  The numpy contract (tests/occupancy_ref.py) is
timed on the same table for scale.  A record holds 300 detections (about 22 KB), so a table of 2^20 rows cannot be built from records on an ordinary
host: --op-rows runs eagle_op_occupancy on a constructed table of that many rows --reps times and prints only the wall time; its per-kernel times
come from a kernel trace of that run (rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eagle_amd import lib, occupancy as oc, weights  # noqa: E402
from control_rate import records, timed  # noqa: E402

HBM_TBS = 6.3
VELOCITY_TBS = 3.6          # docs/experiments.md, "Pitch control (K22)": post_velocity_kernel on a 203 MB table
STAGES = ("occupancy_hist", "occupancy_blur_x", "occupancy_blur_y", "occupancy_norm")


def constructed(rows, persons, seed=0):
    """values [persons + 1][rows][2]: persons and the ball on a random walk of a few centimetres per row"""
    r = np.random.default_rng(seed)
    v = np.empty((persons + 1, rows, 2), np.float64)
    for c in range(persons + 1):
        v[c] = np.array([r.uniform(5, 100), r.uniform(5, 63)]) + np.cumsum(r.normal(0, 0.05, (rows, 2)), 0)
    cols = [(lib.POST_PLAYER, c + 1, 0) for c in range(persons)] + [(lib.POST_BALL, 0, 0)]
    return v, np.arange(rows, dtype=np.int32), cols, {c + 1: c % 2 for c in range(persons)}


def merged_atomics(values, sel_cols, R):
    """global atomics the wave-level merge leaves per member row: runs of equal cell within each run of 64 rows"""
    n = tot = 0
    for c in sel_cols:
        x, y = values[c, :, 0], values[c, :, 1]
        ok = np.isfinite(x) & np.isfinite(y)
        with np.errstate(invalid="ignore"):
            ins = ok & (x >= 0) & (x < 105) & (y >= 0) & (y < 68)
        key = np.where(ins, np.floor(np.where(ins, y, 0) * R) * 105 * R + np.floor(np.where(ins, x, 0) * R), -1)
        brk = np.ones(len(key), bool)
        brk[1:] = (key[1:] != key[:-1]) | (np.arange(1, len(key)) % 64 == 0)
        n += int((brk & ins).sum())
        tot += len(key)
    return n / max(tot, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--players", type=int, default=21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--op-rows", type=int, default=0)
    a = ap.parse_args()
    if a.op_rows:
        v, f, cols, tm = constructed(a.op_rows, a.players + 2)
        off, sc, _ = oc.default_selections(np.array([(k, i, vid, 0) for k, i, vid in cols], lib.POSTCOL_DTYPE), tm)
        out = {"op_rows": a.op_rows, "columns": len(cols), "maps": len(off) - 1, "member_rows": len(sc) * a.op_rows}
        for R in (1, 2, 4):
            p = lib.occupancy_params(25, R, 2.0)
            wall = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                lib.op_occupancy(v, f, cols, p, off, sc)
                wall.append(time.perf_counter() - t0)
            out["R%d_wall_s_median_incl_copies" % R] = round(float(np.median(wall[1:])), 4)
        print(json.dumps(out))
        return
    import occupancy_ref as OR
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    res = {"reps": a.reps, "hbm_TB_per_s": HBM_TBS, "velocity_kernel_TB_per_s": VELOCITY_TBS, "runs": []}
    t = h.postprocess(records(a.rows, a.players, 2), 25, 1280, {i + 1: i % 2 for i in range(a.players)})
    try:
        off, sc, names = oc.default_selections(t.columns, t.team_mapping)
        off_a, sc_a = np.array(off, np.int32), np.array(sc, np.int32)
        n, n_sel, members = len(t.rows), len(off) - 1, len(sc)
        values = np.array(t.values)
        cols = [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in t.columns]
        res.update(rows=n, columns=len(t.columns), maps=n_sel, member_rows=members * n)
        for R in (1, 2, 4):
            for sigma in (0.0, 2.0):
                p = lib.occupancy_params(25, R, sigma)
                call = lambda: h.L.eagle_post_occupancy(h._h, t._t, p, off_a.ctypes.data, sc_a.ctypes.data, n_sel)
                rad = OR.taps(sigma, R)[0]
                plane = n_sel * 7140 * R * R
                run = {"R": R, "sigma": sigma, "rad": rad, "atomics_per_member_row": round(merged_atomics(values, sc, R), 4)}
                for st in STAGES:
                    run[st] = timed(h, st, a.reps, call)
                hist = run["occupancy_hist"]
                hist.update(member_rows_per_s=float("%.4g" % (members * n / (hist["ms_median"] * 1e-3))), GB_per_s=round(members * n * 20.0 / (hist["ms_median"] * 1e-3) / 1e9, 1))
                for st in ("occupancy_blur_x", "occupancy_blur_y"):
                    run[st].update(GB_per_s=round(plane * 8.0 / (run[st]["ms_median"] * 1e-3) / 1e9, 1),
                                   cell_taps_per_s=float("%.4g" % (plane * (2 * rad + 1) / (run[st]["ms_median"] * 1e-3))))
                run["occupancy_norm"].update(GB_per_s=round(plane * 5.0 / (run["occupancy_norm"]["ms_median"] * 1e-3) / 1e9, 1))
                run["sum_ms_median"] = round(sum(run[st]["ms_median"] for st in STAGES), 4)
                if R == 1:                                                               # the contract on the same table, for scale and as a check
                    got = h.occupancy(t, p, off, sc)
                    t0 = time.perf_counter()
                    exp = OR.occupancy(values, t.rows, cols, off, sc, R, sigma, p.max_gap)
                    run["numpy_contract_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                    assert np.array_equal(got[0], exp["grids"]) and np.array_equal(got[2], exp["counts"]) and np.array_equal(got[1], exp["bytes"])
                res["runs"].append(run)
        p = lib.occupancy_params(25, 4, 2.0)
        h.occupancy(t, p, off, sc)
        res["picture_872x576"] = timed(h, "occupancy_picture", a.reps, lambda: h.occupancy_picture(t, n_sel - 1, 8, 16))
    finally:
        t.close()
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
