"""Ball flights of a processed clip table: the ball's path cut into straight lines of constant speed (flights), the rows where two lines meet (knots),
and the knots at which the velocity changes by a kick's worth (kicks); per flight its fitted ends, velocity, kind (still, carried, free) and whether it
would cross a goal line between the posts (a shot).

The rule is this project's own.  Between two touches a ball moves in a straight line at nearly constant speed on the pitch plane; a touch is where the
line breaks.  The breaks are found exactly: a segmented least-squares fit with a penalty per segment, solved by a dynamic program over the kept rows,
after isolated false positions (spikes) have been set aside by a three-sample test.  Everything runs on the GPU where the post-processor left the table
in HBM (include/eagle.h, eagle_post_ball_flights; csrc/flights.hip; tests/flights_ref.py defines every bit).  This module holds the defaults, the call,
the join with a possession result and the writer of ball_flights.json.

The constants (64 rows, 0.25 m noise, a penalty of 16 noise variances, 1 m spikes, 3 m/s kicks, 2 m radius, 0.5 m/s still, shots from 10 m/s within
40 m and 2 m beside the posts) are conventional choices, not fitted to data.  Limits: two displaced samples within two rows of each other are not
spikes, they become a short flight; a flight longer than max_rows is split at a `capped` knot whose dv is small; a rolling ball that slows and a lofted
ball seen through the homography are curves, cut into several flights whose knots mostly stay below kick_dv; gap-filled ball cells lie on a line and
make a perfect flight; the fitted positions are offered as arrays and do not replace the table's ball column; nothing is validated on real footage."""
import math

import numpy as np

from . import lib

PARAM_NAMES = ("max_rows", "noise", "penalty", "spike", "kick_dv", "radius", "still_speed", "shot_speed", "shot_range", "shot_margin")
SHOT_NAMES = (None, "near", "on_target")


def resolve(fps, max_gap=None, **kw):
    """The call's EagleFlightParams with the defaults filled in; ValueError for what the library would refuse."""
    unknown = set(kw) - set(PARAM_NAMES)
    if unknown:
        raise TypeError(f"ball_flights: unknown parameters {sorted(unknown)}")
    p = lib.flight_params(fps, max_gap, **kw)
    fin = math.isfinite
    if not (fin(p.fps) and p.fps > 0.0):
        raise ValueError(f"ball_flights: fps {p.fps} must be finite and positive")
    if not 1 <= p.max_gap <= 1024 or not 2 <= p.max_rows <= 128:
        raise ValueError(f"ball_flights: max_gap {p.max_gap} must lie in 1 .. 1024 and max_rows {p.max_rows} in 2 .. 128")
    if not (fin(p.noise) and 0.0 <= p.noise <= 1024.0 and fin(p.spike) and 0.0 <= p.spike <= 1024.0):
        raise ValueError(f"ball_flights: noise {p.noise} and spike {p.spike} must be finite and within 0 .. 1024 m")
    for k in ("penalty", "kick_dv", "still_speed", "shot_speed", "shot_range", "shot_margin"):
        if not (fin(getattr(p, k)) and getattr(p, k) >= 0.0):
            raise ValueError(f"ball_flights: {k} {getattr(p, k)} must be finite and not negative")
    if not 0.0 < p.radius <= 1024.0:
        raise ValueError(f"ball_flights: radius {p.radius} must be positive and at most 1024 m")
    if not p.penalty * ((p.noise * 1024.0) * (p.noise * 1024.0)) <= 2.0 ** 40:
        raise ValueError(f"ball_flights: penalty {p.penalty} times (noise {p.noise} * 1024)^2 exceeds 2^40")
    return p


def params_dict(p):
    return {"fps": float(p.fps), "max_gap": int(p.max_gap), "max_rows": int(p.max_rows), **{k: float(getattr(p, k)) for k in PARAM_NAMES[1:]}}


def ball_flights(handle, table, fps, cuts=None, **kw):
    """A lib.PostTable of ``handle`` -> {"params", "cuts", "frames", "columns" and Handle.ball_flights' arrays: "seg", "flags", "fitted", "velocity",
    "flights" (lib.FLIGHT_DTYPE), "kicks" (lib.KICK_DTYPE), "totals"}.  The result stays with the table; the table's positions are not changed."""
    p = resolve(fps, **kw)
    cuts = [] if cuts is None else [int(c) for c in cuts]
    res = handle.ball_flights(table, p, cuts)
    return {"params": params_dict(p), "cuts": cuts, "frames": np.asarray(table.rows).copy(), "columns": table.columns.copy(), **res}


def _num(v):
    v = float(v)
    return v if v == v else None


def flight_json(f, frames):
    r0, r1 = int(f["row0"]), int(f["row1"])
    fl = int(f["flags"])
    return {"row0": r0, "row1": r1, "frame0": int(frames[r0]), "frame1": int(frames[r1]), "used": int(f["used"]), "spikes": int(f["spikes"]), "near": int(f["near"]),
            "kind": lib.FLIGHT_KIND_NAMES[int(f["kind"])], "capped": bool(fl & lib.FLIGHT_CAPPED), "continues": bool(fl & lib.FLIGHT_CONTINUES),
            "x0": float(f["x0"]), "y0": float(f["y0"]), "x1": float(f["x1"]), "y1": float(f["y1"]), "vx": float(f["vx"]), "vy": float(f["vy"]),
            "speed": float(f["speed"]), "rms": float(f["rms"]), "shot": SHOT_NAMES[int(f["shot"])], "y_cross": _num(f["y_cross"])}


def join_passes(d, events):
    """Per possession event (lib.EVENT_DTYPE): the first kick with release_row <= row <= receive_row and its kicker, the fastest FREE flight between the
    two rows (the pass speed, m/s) and whether the kicker is the event's `from` id.  Host arithmetic over the small record arrays."""
    ids = lambda c: int(d["columns"][c]["id"]) if c >= 0 else None
    out = []
    for k, e in enumerate(events):
        a, b = int(e["release_row"]), int(e["receive_row"])
        kick = next((q for q in d["kicks"] if a <= int(q["row"]) <= b), None)
        free = [float(f["speed"]) for f in d["flights"] if int(f["kind"]) == lib.FLIGHT_FREE and int(f["row0"]) <= b and int(f["row1"]) >= a]
        kicker = ids(int(kick["col"])) if kick is not None else None
        out.append({"event": k, "frame": int(d["frames"][int(e["row"])]), "from_id": ids(int(e["from_col"])), "to_id": ids(int(e["to_col"])),
                    "kick_row": None if kick is None else int(kick["row"]), "kick_frame": None if kick is None else int(d["frames"][int(kick["row"])]),
                    "kicker_id": kicker, "pass_speed": max(free) if free else None, "kicker_is_from": kicker is not None and kicker == ids(int(e["from_col"]))})
    return out


def to_json(d, events=None, cells=False):
    """ball_flights()' dict in JSON's types only: ids in place of column indices.  events: the table's possession events (Handle.events) for the per-pass
    join; cells: also the per-row arrays."""
    frames = d["frames"]
    t = d["totals"][0]
    flights = [flight_json(f, frames) for f in d["flights"]]
    kicks = [{"row": int(k["row"]), "frame": int(frames[int(k["row"])]), "flight_in": int(k["seg_in"]), "flight_out": int(k["seg_out"]),
              "id": int(d["columns"][int(k["col"])]["id"]) if int(k["col"]) >= 0 else None, "speed_in": float(k["speed_in"]), "speed_out": float(k["speed_out"]),
              "dv": float(k["dv"]), "cos_turn": _num(k["cos_turn"])} for k in d["kicks"]]
    out = {"params": d["params"], "cuts": list(d["cuts"]),
           "totals": {"runs": int(t["runs"]), "flights": int(t["flights"]), "still": int(t["kinds"][0]), "carried": int(t["kinds"][1]), "free": int(t["kinds"][2]),
                      "spikes": int(t["spikes"]), "knots": int(t["knots"]), "kicks": int(t["kicks"]), "shots_evaluated": int(t["shots"].sum()),
                      "shots_near": int(t["shots"][1]), "shots_on_target": int(t["shots"][2]), "capped": int(t["capped"]), "sum_cost": int(t["sum_c"])},
           "flights": flights, "kicks": kicks, "shots": [dict(f, flight=i) for i, f in enumerate(flights) if f["shot"] is not None]}
    if events is not None:
        out["passes"] = join_passes(d, events)
    if cells:
        pair = lambda a: [None if v[0] != v[0] else [float(v[0]), float(v[1])] for v in a]
        out["cells"] = {"frame": [int(f) for f in frames], "flight": [int(s) if s >= 0 else None for s in d["seg"]], "flags": [int(v) for v in d["flags"]],
                        "fitted": pair(d["fitted"]), "velocity": pair(d["velocity"])}
    return out
