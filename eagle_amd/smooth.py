"""Track smoothing of a processed clip table: the pitch positions of every Player and Goalkeeper column (and, on request, the ball) are replaced by windowed
least-squares fits, velocities and accelerations come from the fits' derivatives, jumps are trimmed and reported.

The fits run on the GPU where the post-processor left the table in HBM (include/eagle.h, eagle_post_smooth_tracks; csrc/smooth.hip; tests/smooth_ref.py
defines every bit).  This module holds the defaults, the call and the host arithmetic of smooth.json: a column's RMS and largest residual in metres are
its integer totals over 16 * 1024.  It is opt-in and comes first: every later stage (kinematics, physical report, pass options, control, possession ...)
then reads the smoothed table and the fits' velocities.  The half-width (0.4 s), the degree (2), the threshold (4 medians) and its floor (0.25 m) are
conventional choices, not fitted to data; gap-filled cells count as samples; a homography jump is detected (suspect rows) and trimmed per person
(correcting it as a common motion is eagle_amd.stabilise's part, which runs before this stage); a quadratic over 0.8 s blunts a cut that is faster
than that; the ball stays as it is by default, because a kick is not smooth."""
import math

import numpy as np

from . import lib

RES_UNIT = 16 * lib.SMOOTH_Q            # residual_q per metre
TYPE_NAMES = {lib.POST_PLAYER: "Player", lib.POST_GOALKEEPER: "Goalkeeper", lib.POST_BALL: "Ball"}


def default_window(fps):
    return max(2, int(round(0.4 * fps)))


def resolve(fps, window=None, degree=2, outlier_k=4.0, outlier_floor=0.25, ball_window=0, max_gap=None, speed_cap=12.0):
    """The call's EagleSmoothParams with the defaults filled in; ValueError for what the library would refuse."""
    fps = int(fps)
    if fps <= 0:
        raise ValueError(f"smooth: fps {fps} must be positive")
    p = lib.smooth_params(fps, default_window(fps) if window is None else window, degree, outlier_k, outlier_floor, ball_window, max_gap, speed_cap)
    if not 1 <= p.window <= 64 or not 0 <= p.ball_window <= 64:
        raise ValueError(f"smooth: window {p.window} must lie in 1 .. 64 and ball_window {p.ball_window} in 0 .. 64")
    if p.degree not in (1, 2):
        raise ValueError(f"smooth: degree {p.degree} is neither 1 nor 2")
    if not (math.isfinite(p.outlier_k) and p.outlier_k >= 0.0 and math.isfinite(p.outlier_floor) and p.outlier_floor >= 0.0):
        raise ValueError(f"smooth: outlier_k {p.outlier_k} and outlier_floor {p.outlier_floor} must be finite and not negative")
    if p.max_gap <= 0 or not (math.isfinite(p.speed_cap) and p.speed_cap > 0.0):
        raise ValueError(f"smooth: max_gap {p.max_gap} and speed_cap {p.speed_cap} must be positive")
    return p


def params_dict(p):
    return {"fps": int(p.fps), "window": int(p.window), "degree": int(p.degree), "outlier_k": float(p.outlier_k), "outlier_floor": float(p.outlier_floor),
            "ball_window": int(p.ball_window), "max_gap": int(p.max_gap), "speed_cap": float(p.speed_cap)}


def derive(res, columns, frames, params=None):
    """Handle.smooth_tracks' arrays, the table's columns (lib.POSTCOL_DTYPE) and frame numbers -> {"params", "columns": one entry per smoothed column
    (column, id, type, window, present, outliers, low_degree, rms_residual and max_residual in metres), "suspect": [{"row", "frame"}], and the arrays}."""
    cols = []
    for c, t in enumerate(res["totals"]):
        if int(t["window"]) == 0:
            continue
        k = columns[c]
        n = int(t["present"])
        cols.append({"column": c, "id": int(k["id"]), "type": TYPE_NAMES[int(k["kind"])], "window": int(t["window"]), "present": n, "outliers": int(t["outliers"]),
                     "low_degree": int(t["low_degree"]), "rms_residual": math.sqrt(int(t["sum_sq"]) / n) / RES_UNIT if n else 0.0,
                     "max_residual": int(t["max_residual_q"]) / RES_UNIT})
    suspect = [{"row": int(r), "frame": int(frames[r])} for r in np.flatnonzero(res["suspect"])]
    return {"params": params, "columns": cols, "suspect": suspect, **{k: res[k] for k in ("velocities", "acc", "flags", "count", "residual_q") if k in res}}


def smooth_tracks(handle, table, fps, **kw):
    """A lib.PostTable of ``handle`` that carries no derived result yet -> derive()'s dict; the table holds the smoothed positions and the fits' velocities
    afterwards (Handle.raw_values gives the old positions)."""
    p = resolve(fps, **kw)
    return derive(handle.smooth_tracks(table, p), table.columns, table.rows, params_dict(p))


def to_json(d, rows=False):
    """derive()'s dict in JSON's types only.  rows False: without the per-cell arrays; True: per smoothed column its cells' flags, count, residual (m),
    velocity and acceleration, None where the cell is absent."""
    out = {"params": d["params"], "columns": [dict(c) for c in d["columns"]], "suspect": list(d["suspect"])}
    if rows:
        fl = lambda a: [None if v[0] != v[0] else [float(v[0]), float(v[1])] for v in a]
        for c in out["columns"]:
            i = c["column"]
            present = d["flags"][i] != 0
            c["cells"] = {"flags": [int(v) if ok else None for v, ok in zip(d["flags"][i], present)], "count": [int(v) if ok else None for v, ok in zip(d["count"][i], present)],
                          "residual": [int(v) / RES_UNIT if ok else None for v, ok in zip(d["residual_q"][i], present)], "velocity": fl(d["velocities"][i]),
                          "acceleration": fl(d["acc"][i])}
    return out
