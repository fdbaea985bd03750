#!/usr/bin/env python3
"""Cost of the space kernels (include/eagle.h, eagle_post_space; csrc/space.hip): one JSON line.

    python tools/space_rate.py [--rows 30000] [--reps 5] [--numpy-rows 20]

A processed table of --rows rows is built by eagle_postprocess from constructed records: two teams of ten outfield players round a 4-4-2 each, two
goalkeepers and the ball, everybody present on every row, so every row is ACTIVE with 22 sites.  For 1, 2 and 4 cells per metre the three stages of one
eagle_post_space call are timed over all rows: HIP events of the profiling mode around the launches, --reps calls after a warm-up call, reported as the
median with the minimum and the maximum.  Next to the cells kernel stand its (cell, site) distance evaluations per second, the VALU bound of its inner
loop estimated from the instruction mix in the gfx950 disassembly (see docs/experiments.md, "Space (K30)") and the share of it reached, and the time the
numpy restatement (tests/space_ref.py) takes on --numpy-rows of the same rows, scaled to the table."""
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

# VALU bound of space_cells_kernel's inner loop.  One pass handles one site for the 64 cells of a wave.  Counted in the gfx950 disassembly (the loop is
# unrolled by two) a pass issues 2 v_sub_u32, 2 v_mad_i64_i32, 1 v_cmp_lt_i64, 3 v_cndmask_b32 and 1.5 v_mov_b32 beside half a ds_read_b128: 9.5 vector
# instructions, 19 cycles at the 2 cycles a SIMD takes to issue a wave64 instruction.  The two 64-bit instructions may well issue slower than that; their
# price on gfx950 is not known here, so the bound is a floor and the share reached is a lower estimate of how close the loop is to what the VALU can do.
# 256 CUs x 4 SIMDs at 2.4 GHz: 2.458e12 SIMD-cycles/s
CYCLES_PER_PASS = 19
SIMD_CYCLES = 256 * 4 * 2.4e9
FORM = [(20, 8), (18, 26), (18, 42), (20, 60), (45, 10), (43, 27), (43, 41), (45, 58), (70, 24), (70, 44)]
NAMES = ("space_sites", "space_cells", "space_totals")


def records(n, seed=0):
    """n records of 20 players (ids 1 .. 20, slot s of team g is detection 10 g + s), two goalkeepers (ids 21, 22) and the ball"""
    r = np.random.default_rng(seed)
    k = 23
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = k, 1, 1
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    base = np.array([(x, y) for x, y in FORM] + [(105 - x, y) for x, y in FORM] + [(3, 34), (102, 34), (52, 34)], np.float64)
    pos = np.clip(base[None] + r.normal(0, 2.0, (n, k, 2)) + np.cumsum(r.normal(0, 0.2, (n, 1, 2)), 0), 0, [105, 68])
    d, j = recs["det"], np.arange(k)
    d["reported"][:, :k], d["in_bounds"][:, :k], d["conf"][:, :k] = 1, 1, 0.9
    d["cls"][:, :k] = np.where(j == k - 1, 2, np.where(j >= 20, 1, 0))[None]
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
    return {k: {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(min(v)), 4), "ms_max": round(float(max(v)), 4)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-rows", type=int, default=20)
    a = ap.parse_args()
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    res = {"reps": a.reps, "valu_cycles_per_pass": CYCLES_PER_PASS}
    import space_ref as SR
    t = h.postprocess(records(a.rows), 25, 1280, {i: 0 if i <= 10 else 1 for i in range(1, 21)})
    try:
        rows = len(t.rows)
        values = np.array(t.values)
        cols = [(int(c["kind"]), int(c["id"]), int(c["video"])) for c in t.columns]
        for R in (1, 2, 4):
            p = lib.space_params(R)
            out = timed(h, a.reps, lambda: h.space(t, p))
            rec, sites, totals = h.space(t, p)
            act = rec["status"] == lib.SPACE_ACTIVE
            # a wave takes 64 cells of a band of 420 R; a band is ceil(420 R / 64) wave steps, a row 17 R bands
            passes = float(rec["n_sites"][act].astype(np.int64).sum()) * 17 * R * -(-420 * R // 64)
            evals = float(rec["n_sites"][act].astype(np.int64).sum()) * 7140 * R * R
            g = out["space_cells"]
            sec = g["ms_median"] * 1e-3
            g.update(active_rows=int(act.sum()), sites_per_row=round(float(rec["n_sites"][act].mean()), 2), evaluations=float("%.4g" % evals),
                     evaluations_per_s=float("%.4g" % (evals / sec)), ms_at_valu_bound=round(passes * CYCLES_PER_PASS / SIMD_CYCLES * 1e3, 4),
                     of_valu_bound=round(passes * CYCLES_PER_PASS / SIMD_CYCLES / sec, 4))
            out.update(rows=rows, members=int(len(totals)))
            k = min(a.numpy_rows, rows)
            t0 = time.perf_counter()
            SR.space(values[:, :k], cols, t.team_mapping, SR.space_params(R))
            dt = time.perf_counter() - t0
            out["numpy"] = {"rows": k, "seconds": round(dt, 3), "seconds_scaled_to_table": round(dt * rows / max(k, 1), 1)}
            res["R%d" % R] = out
    finally:
        t.close()
    h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
