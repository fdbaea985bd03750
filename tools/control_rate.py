#!/usr/bin/env python3
"""Cost of the kinematics and pitch-control kernels (include/eagle.h, eagle_post_velocities / eagle_control_device_grids / eagle_minimap_device_frames;
csrc/post.hip, csrc/control.hip, csrc/minimap.hip): one JSON line.

    python tools/control_rate.py [--rows 2000] [--batch 200] [--vel-rows 135000] [--vel-ids 44] [--reps 10]

Two processed tables are built by eagle_postprocess from constructed records.  The first has --vel-rows rows (match length) and 2 x --vel-ids + 6
columns: post_velocity_kernel, in GB/s against the table's bytes (16 read + 16 written per cell).  A match has about 1206 columns; a record holds at
most 300 detections, so the table here is narrower.  Columns are independent streams of the kernel (one grid row each), so the rate per byte does not
depend on their number once the table and the velocity table together (2 x 203 MB here) exceed the 256 MB of last-level cache.  The second has --rows rows with 22 mapped players (22 sites on every row), 2 goalkeepers and the ball: control_kernel for R = 1, 2, 4, --batch
rows per call, in cells x sites per second, and the minimap at 8 pixels per metre (872 x 576, BGR) without a tint, with the Voronoi tint and with the
control layer (whose time includes its grids).  Every figure: HIP events of the profiling mode around the launches of ONE call, --reps calls after a
warm-up call, reported as the median with the minimum and the maximum.  Next to each control figure stands the VALU bound estimated from the kernel's
instruction count per cell and site (see docs/experiments.md, "Pitch control (K22)")."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eagle_amd import lib, weights  # noqa: E402

HBM_TBS = 6.3
# VALU bound of control_kernel.  A SIMD issues a wave64 vector instruction over 2 cycles (4 for v_sqrt_f32 / v_rcp_f32).  Per site, a wave (256 cells: 4 per
# lane) issues, counted in the gfx950 disassembly, 22 instructions in pass 1's loop and 232 in pass 2's (d^2, the correctly rounded sqrtf and division
# with their scale / fix-up sequences, d_expf's clamp and polynomial, the two sums), 8 of them of the slow kind: 2 x 254 + 2 x 8 = 524 cycles.
# 256 CUs x 4 SIMDs at 2.4 GHz: 2.458e12 SIMD-cycles/s
VALU_PER_CELL_SITE = (22 + 232) / 4.0
CYCLES_PER_WAVE_SITE = 2 * (22 + 232) + 2 * 8
VALU_BOUND = 256 * 4 * 2.4e9 / CYCLES_PER_WAVE_SITE * 256


def records(n, players, keepers, seed=0):
    """n records: `players` players and `keepers` goalkeepers on a random walk over the pitch, one ball, the camera's bounds on every frame"""
    r = np.random.default_rng(seed)
    k = players + keepers + 1
    assert k <= 300
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = k, 1, 1
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    pos = np.stack([r.uniform(5, 100, k), r.uniform(5, 63, k)], 1)[None] + np.cumsum(r.normal(0, 0.3, (n, k, 2)), 0)
    pos = np.clip(pos, 0, [105, 68])
    d = recs["det"]
    j = np.arange(k)
    d["reported"][:, :k], d["in_bounds"][:, :k], d["conf"][:, :k] = 1, 1, 0.9
    d["cls"][:, :k] = np.where(j == k - 1, 2, np.where(j >= players, 1, 0))[None]
    d["id"][:, :k] = (j + 1)[None]
    d["bx1"][:, :k], d["bx2"][:, :k], d["by1"][:, :k], d["by2"][:, :k] = (4 * j)[None], (4 * j + 3)[None], 300, 340
    d["pitch_x"][:, :k], d["pitch_y"][:, :k] = pos[..., 0].astype(np.int32), pos[..., 1].astype(np.int32)
    return recs


def timed(h, name, reps, call):
    """ms of the launches accumulated under `name` in one call: reps calls after one warm-up -> {median, min, max}"""
    call()
    ms = []
    for _ in range(reps):
        h.set_profiling(1)
        call()
        row = [x for x in h.kernel_times() if x[0] == name]
        h.set_profiling(0)
        ms.append(sum(x[1] for x in row))
    ms = np.sort(ms)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms[0]), 4), "ms_max": round(float(ms[-1]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--vel-rows", type=int, default=135000)
    ap.add_argument("--vel-ids", type=int, default=44)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    res = {"reps": a.reps, "hbm_TB_per_s": HBM_TBS, "valu_per_cell_site": VALU_PER_CELL_SITE}
    # ---- the velocity kernel ----
    t = h.postprocess(records(a.vel_rows, a.vel_ids - 2, 2), 25, 1280, None)
    try:
        cells = len(t.rows) * len(t.columns)
        r = timed(h, "post_velocity", a.reps, lambda: h.L.eagle_post_velocities(h._h, t._t, lib.kinematics_params(25)))
        r.update(rows=len(t.rows), columns=len(t.columns), table_MB=round(cells * 16 / 1e6, 1), GB_per_s=round(cells * 32 / (r["ms_median"] * 1e-3) / 1e9, 1),
                 bound_GB_per_s=HBM_TBS * 1e3)
        r["of_bound"] = round(r["GB_per_s"] / r["bound_GB_per_s"], 3)
        res["velocity"] = r
    finally:
        t.close()
    # ---- control_kernel and the minimap ----
    t = h.postprocess(records(a.rows, 22, 2, 1), 25, 1280, {i + 1: i % 2 for i in range(22)})
    B = min(a.batch, len(t.rows))
    h.velocities(t, 25)
    w, hh = lib.minimap_size(lib.minimap_params(8))
    d_out = h.upload(np.zeros(max(B * hh * w * 3, B * 7140 * 16), np.uint8))
    try:
        res["control"] = {"rows_per_call": B, "sites": 22}
        for R in (1, 2, 4):
            p = lib.control_params(R)
            r = timed(h, "control", a.reps, lambda: h.control_device(t, d_out, p, 0, B))
            work = B * 7140 * R * R * 22
            r.update(cell_sites_per_s=float("%.4g" % (work / (r["ms_median"] * 1e-3))), valu_bound_cell_sites_per_s=float("%.4g" % VALU_BOUND),
                     of_bound=round(work / (r["ms_median"] * 1e-3) / VALU_BOUND, 3), grids_per_s=round(B / (r["ms_median"] * 1e-3)))
            res["control"]["R%d" % R] = r
        res["minimap_872x576_bgr"] = {"rows_per_call": B}
        h.minimap_set_control(t, lib.control_params(4))
        for key, par in (("plain", lib.minimap_params(8)), ("voronoi", lib.minimap_params(8, voronoi=True)), ("control_R4", lib.minimap_params(8, control=True))):
            r = timed(h, "minimap", a.reps, lambda: h.minimap_device(t, d_out, par, 0, B, "bgr"))
            if key == "control_R4":
                g = timed(h, "control", a.reps, lambda: h.minimap_device(t, d_out, par, 0, B, "bgr"))
                r["grids_ms_median"] = g["ms_median"]
                r["frames_per_s"] = round(B / ((r["ms_median"] + g["ms_median"]) * 1e-3))
            else:
                r["frames_per_s"] = round(B / (r["ms_median"] * 1e-3))
            res["minimap_872x576_bgr"][key] = r
    finally:
        h.free(d_out)
        t.close()
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
