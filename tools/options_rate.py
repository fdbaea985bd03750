#!/usr/bin/env python3
"""Cost of the pass-option kernels (include/eagle.h, eagle_pass_options_device; csrc/options.hip): one JSON line.

    python tools/options_rate.py [--rows 30000] [--samples 16] [--reps 7] [--numpy-rows 50]

A processed table of --rows rows is built by eagle_postprocess from constructed records: 22 mapped players (11 a side, a site each on every row) and the
ball.  Possession runs with a radius that always finds an owner, so every row is active with 10 teammates and 11 defenders.  The sites, grid and
options (targets + best) launches are timed separately for R = 1, 2, 4 over ALL rows in one call of the device entry: HIP events of the profiling mode
around the launches, --reps calls after a warm-up call, reported as the median with the minimum and the maximum.  Next to the grid kernel stands its VALU
bound, estimated from the inner loop's instruction count in the gfx950 disassembly (see docs/experiments.md, "Pass options (K28)"), and the time the
numpy restatement (tests/options_ref.py) takes for --numpy-rows of the same rows at R = 1, scaled to the table."""
import argparse
import ctypes as C
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

# VALU bound of options_grid_kernel.  A SIMD issues a wave64 vector instruction over 2 cycles.  The defender loop is unrolled by four; per round a wave
# (256 cells: 4 per lane) issues, counted in the gfx950 disassembly, 16 x (2 v_sub + 2 v_mul + 1 v_add) + 8 v_min3 + 1 v_mov = 89 vector instructions
# against two 16-byte LDS broadcast reads: 22.25 per defender, 44.5 cycles.  256 CUs x 4 SIMDs at 2.4 GHz: 2.458e12 SIMD-cycles/s
VALU_PER_ITEM = 89 / 16.0
CYCLES_PER_WAVE_DEFENDER = 2 * 89 / 4.0
VALU_BOUND = 256 * 4 * 2.4e9 / CYCLES_PER_WAVE_DEFENDER * 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--numpy-rows", type=int, default=50)
    a = ap.parse_args()
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    res = {"reps": a.reps, "samples": a.samples, "valu_per_cell_sample_defender": VALU_PER_ITEM, "valu_bound_items_per_s": float("%.4g" % VALU_BOUND)}
    mapping = {i + 1: i % 2 for i in range(22)}
    t = h.postprocess(records(a.rows, 22, 0, 1), 25, 1280, mapping)
    rows = len(t.rows)
    vel = h.velocities(t, 25)
    cand, owner, _, _ = h.possession(t, lib.possession_params(25, 1024.0, 1, 1000))
    ns = len(h.pass_options_layout(t))
    d = C.c_void_p()
    need = rows * (7140 * 16 + 40 + 2 * ns) + 4096
    h._check(h.L.eagle_device_alloc(h._h, need, C.byref(d)), "device_alloc")
    try:
        recs = h.pass_options(t, lib.pass_option_params(1, a.samples), grids=False, options=False)[1]
        live = (recs["status"] == lib.PASS_ACTIVE) & (recs["n_mates"] > 0)
        items_per_cell = float(a.samples) * float(recs["n_defenders"][live].sum())        # (cell, sample, defender) evaluations per cell of the grid, over the table
        res.update(rows=rows, sites=ns, active_rows=int(live.sum()), mean_defenders=round(float(recs["n_defenders"][live].mean()) if live.any() else 0.0, 2))
        for R in (1, 2, 4):
            p = lib.pass_option_params(R, a.samples)
            cells = 7140 * R * R
            d_rows = C.c_void_p(d.value + ((rows * cells + 255) & ~255))
            d_opt = C.c_void_p(d_rows.value + ((rows * 40 + 255) & ~255))
            call = lambda: h.pass_options_device(t, p, d_rows, 0, rows, d, d_opt)
            out = {}
            for name in ("options_sites", "options_grid", "options_targets"):
                out[name] = timed(h, name, a.reps, call)
            work = items_per_cell * cells
            g = out["options_grid"]
            g.update(items=float("%.4g" % work), items_per_s=float("%.4g" % (work / (g["ms_median"] * 1e-3))), ms_at_bound=round(work / VALU_BOUND * 1e3, 3),
                     of_bound=round(work / (g["ms_median"] * 1e-3) / VALU_BOUND, 3), grids_per_s=round(rows / (g["ms_median"] * 1e-3)))
            res["R%d" % R] = out
        # the numpy restatement on the first rows of the same table, R = 1
        import options_ref as OR
        k = min(a.numpy_rows, rows)
        values = np.array(t.values)
        cols = [(int(c["kind"]), int(c["id"]), int(c["video"])) for c in t.columns]
        t0 = time.perf_counter()
        OR.rows(values, vel, cols, t.team_mapping, cand, owner, 0, k, OR.params(1, a.samples))
        dt = time.perf_counter() - t0
        res["numpy_R1"] = {"rows": k, "seconds": round(dt, 3), "seconds_scaled_to_table": round(dt * rows / max(k, 1), 1)}
    finally:
        h.free(d)
        t.close()
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
