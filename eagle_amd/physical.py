"""Physical report of a processed clip table: how far each player ran at which intensity, how fast at most, and how many high-speed runs, sprints,
hard accelerations and hard decelerations they made.

Speeds, zones, integer totals and efforts are computed on the GPU from the table's velocities where the post-processor left them in HBM (include/eagle.h,
eagle_post_physical; csrc/physical.hip; tests/physical_ref.py defines every bit): a step's distance is quantised once to 2^-20 m, sums are integers after
that.  This module is pure host arithmetic on those integers: metres are q / 2^20 and seconds frames / fps, each one correctly rounded division of exact
integers, so a person's zone distances add up to the total distance exactly as integers do (``distance_q``).  The zone edges (2 / 4 / 5.5 / 7 m/s: standing
and walking, jogging, running, high-speed running, sprinting), the effort thresholds (5.5 and 7 m/s, 2 m/s^2) and the shortest effort (half a second) are
conventional choices, not fitted to data.  The figures follow a column of the table: they follow a person only when fragmented track ids have been merged
(process_data's merge_ids)."""
import numpy as np

from . import lib

Q = lib.LOAD_Q
KIND_NAMES = ("high_speed_run", "sprint", "acceleration", "deceleration")
ZONE_NAMES = ("walk", "jog", "run", "high_speed", "sprint")


def derive(speed, accel, zone, totals, efforts, columns, frames, fps, params=None):
    """Handle.physical's arrays, the table's columns (lib.POSTCOL_DTYPE) and frame numbers -> {"params", "players": [...], "efforts": [...], "speed",
    "accel", "zone"}.  A player entry: id, type, rows, distance_q and zone_distance_q (integers, 2^-20 m), distance and zone_distance (m), zone_seconds,
    top_speed (m/s) and the number of efforts per kind; an effort: id, kind, first / last row and frame, seconds, distance (m), peak_speed, peak_accel."""
    fps = int(fps)
    players = []
    for t in totals:
        k = columns[int(t["col"])]
        zq = [int(x) for x in t["zone_dist_q"]]
        players.append({"id": int(k["id"]), "type": "Player" if int(k["kind"]) == lib.POST_PLAYER else "Goalkeeper", "rows": int(t["rows_present"]),
                        "distance_q": sum(zq), "zone_distance_q": zq, "distance": sum(zq) / Q, "zone_distance": [x / Q for x in zq],
                        "zone_seconds": [int(x) / fps for x in t["zone_frames"]], "top_speed": float(t["top_speed"]),
                        **{KIND_NAMES[j] + "s": int(t["efforts"][j]) for j in range(4)}})
    out = []
    for e in efforts:
        first, last = int(e["first_row"]), int(e["last_row"])
        out.append({"id": int(columns[int(e["col"])]["id"]), "kind": KIND_NAMES[int(e["kind"])], "first_row": first, "last_row": last,
                    "first_frame": int(frames[first]), "last_frame": int(frames[last]), "seconds": int(e["frames"]) / fps, "distance_q": int(e["distance_q"]),
                    "distance": int(e["distance_q"]) / Q, "peak_speed": float(e["peak_speed"]), "peak_accel": float(e["peak_accel"])})
    return {"params": params, "players": players, "efforts": out, "speed": speed, "accel": accel, "zone": zone}


def params_dict(p):
    return {"fps": int(p.fps), "max_gap": int(p.max_gap), "zone_edges": [float(x) for x in p.zone_edges], "zone_names": list(ZONE_NAMES),
            "effort_speed": [float(x) for x in p.effort_speed], "accel": float(p.accel), "min_frames": [int(x) for x in p.min_frames]}


def physical(handle, table, fps, max_gap=None, zone_edges=(2.0, 4.0, 5.5, 7.0), effort_speed=(5.5, 7.0), accel=2.0, min_frames=None):
    """A lib.PostTable of ``handle`` with velocities (Handle.velocities, or eagle_amd.control.kinematics) -> derive()'s dict.  The per-row arrays are
    [persons, rows] in the order of "players"; speed and zone stay with the table in HBM (Handle.physical_device)."""
    p = lib.load_params(fps, max_gap, zone_edges, effort_speed, accel, min_frames)
    speed, acc, zone, totals, efforts = handle.physical(table, p)
    return derive(speed, acc, zone, totals, efforts, table.columns, table.rows, fps, params_dict(p))


def to_json(d, rows=False):
    """derive()'s dict in JSON's types only.  rows False: without the per-row arrays (persons x rows x 3 numbers); True: they become lists, with None
    where a row is absent"""
    def conv(a):
        a = np.asarray(a)
        if a.dtype == np.uint8:
            return [[None if v == lib.LOAD_ABSENT else int(v) for v in r] for r in a]
        return [[None if v != v else float(v) for v in r] for r in a]
    out = {k: v for k, v in d.items() if k not in ("speed", "accel", "zone")}
    if rows:
        for k in ("speed", "accel", "zone"):
            out[k] = conv(d[k])
    return out


def from_json(j):
    """The inverse of to_json: per-row arrays, where the file has them, are numpy arrays again (NaN / 255 where absent)"""
    out = dict(j)
    n = len(j["players"])
    for k, dt, miss in (("speed", np.float64, np.nan), ("accel", np.float64, np.nan), ("zone", np.uint8, lib.LOAD_ABSENT)):
        if k in j:
            out[k] = np.array([[miss if v is None else v for v in r] for r in j[k]], dt).reshape(n, -1)
    return out
