"""Stabilisation of a processed clip table: the motion that every player and the ball of one frame share, the small translation, stretch and shear of the
pitch plane that a slightly wrong homography gives them all at once, is estimated per kept frame and removed.

It runs on the GPU where the post-processor left the table in HBM (include/eagle.h, eagle_post_stabilise; csrc/stab.hip; tests/stab_ref.py defines
every bit).  This module holds the defaults, the call and the host arithmetic of stabilise.json: RMS residuals in metres are the integer totals over
1024.  It is opt-in and comes first, before eagle_amd.smooth and every derived result.

Limits.  What differs from the window's trend is removed: an error that lasts (a homography that stays wrong for a second, the drift between two
key-point frames of the cadence) is a path like any other and stays.  Gap-filled cells cannot be told from seen ones: they lie on a line, vote for "no
motion" and bias a row in which many cells are filled.  A real common jerk, the whole team stopping in one frame, is taken for camera error.  The affine
map is a first-order stand-in for a projective error, valid where the players stand, which is why boundaries are not moved.  The ball is moved by the map
although it may be in the air.  At most 64 voters per row.  The half-width (1 s), the degree (2), six voters, two rounds, 3 medians with a 0.1 m floor,
5 m of spread, 5 % of gain and the 1 m jump are conventional choices, not fitted to data; nothing was validated on real footage."""
import math

import numpy as np

from . import lib

MODEL_NAMES = ("none", "translation", "affine")
FLAG_NAMES = ((lib.STAB_OVER_CAP, "over_cap"), (lib.STAB_FEW, "few_inliers"), (lib.STAB_SPREAD, "low_spread"), (lib.STAB_CORR, "correlated"), (lib.STAB_GAIN, "high_gain"),
              (lib.STAB_JUMP, "jump"))


def default_window(fps):
    return min(64, max(2, int(round(1.0 * fps))))


def resolve(fps, window=None, degree=2, model=1, min_voters=6, iterations=2, trim_k=3.0, floor=0.1, min_spread=5.0, max_gain=0.05, jump=1.0):
    """The call's EagleStabParams with the defaults filled in; ValueError for what the library would refuse."""
    fps = int(fps)
    if fps <= 0:
        raise ValueError(f"stabilise: fps {fps} must be positive")
    if model not in (0, 1, "translation", "affine"):
        raise ValueError(f"stabilise: model {model!r} is neither translation (0) nor affine (1)")
    p = lib.stab_params(fps, default_window(fps) if window is None else window, degree, model, min_voters, iterations, trim_k, floor, min_spread, max_gain, jump)
    fin = math.isfinite
    if not 1 <= p.window <= 64:
        raise ValueError(f"stabilise: window {p.window} must lie in 1 .. 64")
    if p.degree not in (1, 2):
        raise ValueError(f"stabilise: degree {p.degree} is neither 1 nor 2")
    if not 3 <= p.min_voters <= 64:
        raise ValueError(f"stabilise: min_voters {p.min_voters} must lie in 3 .. 64")
    if not 1 <= p.iterations <= 4:
        raise ValueError(f"stabilise: iterations {p.iterations} must lie in 1 .. 4")
    if not (fin(p.trim_k) and (p.trim_k == 0.0 or 1.0 <= p.trim_k <= 1000.0)):
        raise ValueError(f"stabilise: trim_k {p.trim_k} must be 0 (no trimming) or lie in 1 .. 1000")
    if not (fin(p.floor) and 0.0 <= p.floor <= 1024.0):
        raise ValueError(f"stabilise: floor {p.floor} must lie in 0 .. 1024")
    if not (fin(p.min_spread) and 0.0 < p.min_spread <= 1024.0):
        raise ValueError(f"stabilise: min_spread {p.min_spread} must be positive and at most 1024")
    if not (fin(p.max_gain) and 0.0 < p.max_gain <= 1.0):
        raise ValueError(f"stabilise: max_gain {p.max_gain} must be positive and at most 1")
    if not (fin(p.jump) and p.jump > 0.0):
        raise ValueError(f"stabilise: jump {p.jump} must be positive and finite")
    return p


def params_dict(p):
    return {"fps": int(p.fps), "window": int(p.window), "degree": int(p.degree), "model": MODEL_NAMES[1 + int(p.model)], "min_voters": int(p.min_voters),
            "iterations": int(p.iterations), "trim_k": float(p.trim_k), "floor": float(p.floor), "min_spread": float(p.min_spread), "max_gain": float(p.max_gain),
            "jump": float(p.jump)}


def _rms(ss, n):
    return math.sqrt(int(ss) / int(n)) / lib.STAB_Q if int(n) else 0.0


def derive(res, frames, params=None):
    """Handle.stabilise's arrays and the table's frame numbers -> {"params", "totals" (the counts and the RMS residual of the inliers' votes before and after
    the map, in metres), "jumps": [{"row", "frame", "shift": [x, y] in metres}], and the arrays "rows", "votes"}."""
    t = res["totals"][0]
    totals = {k: int(t[k]) for k in ("rows", "none", "translation", "affine", "few_inliers", "low_spread", "correlated", "high_gain", "jumps", "over_cap", "inliers", "moved")}
    totals["rms_before"], totals["rms_after"] = _rms(t["ss_before"], t["inliers"]), _rms(t["ss_after"], t["inliers"])
    rows = res["rows"]
    jumps = [{"row": int(r), "frame": int(frames[r]), "shift": [int(rows[r]["shift_q"][0]) / lib.STAB_Q, int(rows[r]["shift_q"][1]) / lib.STAB_Q]}
             for r in np.flatnonzero(rows["flags"] & lib.STAB_JUMP)]
    return {"params": params, "totals": totals, "jumps": jumps, "rows": rows, "votes": res.get("votes"), "frames": [int(f) for f in frames]}


def stabilise(handle, table, fps, **kw):
    """A lib.PostTable of ``handle`` that carries no derived result yet -> derive()'s dict; the table holds the stabilised positions afterwards
    (Handle.original_values gives the old ones)."""
    p = resolve(fps, **kw)
    return derive(handle.stabilise(table, p), table.rows, params_dict(p))


def to_json(d, rows=False):
    """derive()'s dict in JSON's types only.  rows False: parameters, totals and the jump rows; True: also a record per row (frame, voters, inliers, model,
    flags by name, shift and centre in metres, the four gains, the inliers' RMS residual before and after in metres, cells moved)."""
    out = {"params": d["params"], "totals": dict(d["totals"]), "jumps": [dict(j) for j in d["jumps"]]}
    if rows:
        out["rows"] = [{"frame": f, "voters": int(e["voters"]), "inliers": int(e["inliers"]), "model": MODEL_NAMES[int(e["model"])],
                        "flags": [name for bit, name in FLAG_NAMES if int(e["flags"]) & bit], "shift": [int(v) / lib.STAB_Q for v in e["shift_q"]],
                        "centre": [int(v) / lib.STAB_Q for v in e["centre_q"]], "gain": [float(v) for v in e["gain"]],
                        "rms_before": _rms(e["ss_before"], e["inliers"]), "rms_after": _rms(e["ss_after"], e["inliers"]), "moved": int(e["moved"])}
                       for f, e in zip(d["frames"], d["rows"])]
    return out
