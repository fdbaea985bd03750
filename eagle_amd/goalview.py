"""Goal view of a processed clip table: how much of the goal mouth every attacker, the ball and, optionally, every cell of the pitch sees past the
other team's players and keeper.  The value of a position for a shot: the open angle in radians.

The rule is this project's own.  The mouth of the goal a group attacks (y = 30.34 .. 37.66 on the line x = 0 or x = 105) is cut into 64 slices; an
opponent between the point and the line is a disc (0.4 m, a keeper 1.0 m) whose two tangents from the point bound the slices it hides; a slice's angle
is the midpoint rule's DY |s| / (s^2 + dy^2), an integer in units of 2^-24 rad; the open angle is the sum over the slices nobody hides.  Everything
runs on the GPU where the post-processor left the table in HBM (include/eagle.h, eagle_post_goal_view; csrc/goalview.hip; tests/goalview_ref.py
defines every bit).  This module holds the defaults, the call, the joins with the ball flights and the pass events, and the writer of goal_view.json.

Limits: players are discs at their foot point; height, the ball's loft, the speed of a shot and a keeper's dive are not modelled.  The radii, the
1 m least depth, the 40 m range and the 0.3 rad of a "chance" are conventional choices, not fitted to data.  A defender outside the picture is not in
the table and hides nothing.  A row with more than 32 blockers is not evaluated.  Nothing is validated on real footage."""
import math

import numpy as np

from . import lib

PARAM_NAMES = ("direction", "group", "cells_per_metre", "form", "radius", "keeper_radius", "min_depth", "max_range", "chance")
UNIT = 2.0 ** -24                                                         # radians per unit of `open`
Y0, DY = 30.34, 7.32 / 64.0


def resolve(rows=0, grid=False, has_team=True, offside_direction=None, has_possession=False, **kw):
    """The call's EagleGoalViewParams with the defaults filled in; ValueError for what the library would refuse.  offside_direction: None when the
    table has no offside result, else the direction it settled (0: none); grid: a grid over all the rows."""
    unknown = set(kw) - set(PARAM_NAMES)
    if unknown:
        raise TypeError(f"goal_view: unknown parameters {sorted(unknown)}")
    p = lib.goal_view_params(grid_row0=0, grid_rows=int(rows) if grid else 0, **kw)
    for k in ("radius", "keeper_radius", "min_depth", "max_range", "chance"):
        if not math.isfinite(getattr(p, k)):
            raise ValueError(f"goal_view: {k} {getattr(p, k)} is not finite")
    for k in ("radius", "keeper_radius"):
        if not 0.0 <= getattr(p, k) <= 16.0:
            raise ValueError(f"goal_view: {k} {getattr(p, k)} is outside 0 .. 16 m")
    if p.min_depth < 1.0:
        raise ValueError(f"goal_view: min_depth {p.min_depth} is below 1 m")
    if not p.min_depth < p.max_range <= 1024.0:
        raise ValueError(f"goal_view: max_range {p.max_range} must lie above min_depth {p.min_depth} and within 1024 m")
    if not 0.0 <= p.chance <= 4.0:
        raise ValueError(f"goal_view: chance {p.chance} is outside 0 .. 4 rad")
    if p.cells_per_metre not in (1, 2, 4):
        raise ValueError(f"goal_view: cells_per_metre {p.cells_per_metre} is none of 1, 2, 4")
    if p.direction not in (lib.OFFSIDE_DIR_AUTO, lib.OFFSIDE_DIR_RIGHT, lib.OFFSIDE_DIR_LEFT):
        raise ValueError(f"goal_view: direction {p.direction} is none of 0 (the offside result's), 1 (right), 2 (left)")
    if p.group not in (-1, 0, 1) or p.form not in (lib.GOALVIEW_FORM_DEFAULT, lib.GOALVIEW_FORM_DIRECT, lib.GOALVIEW_FORM_TABLE):
        raise ValueError(f"goal_view: group {p.group} must be -1, 0 or 1 and form {p.form} a GOALVIEW_FORM_*")
    if p.direction == lib.OFFSIDE_DIR_AUTO and offside_direction not in (lib.OFFSIDE_DIR_RIGHT, lib.OFFSIDE_DIR_LEFT):
        raise ValueError("goal_view: direction 0 takes the direction of the table's offside result, and the table has " +
                         ("none" if offside_direction is None else "one that settled no direction"))
    if grid and p.group < 0 and not has_possession:
        raise ValueError("goal_view: group -1 (the group that owns the ball) needs a possession result")
    if not has_team:
        raise ValueError("goal_view: the table has no team mapping")
    return p


def params_dict(p):
    return {"direction": int(p.direction), "group": int(p.group), "cells_per_metre": int(p.cells_per_metre), "form": int(p.form),
            **{k: float(getattr(p, k)) for k in PARAM_NAMES[4:]}}


def goal_view(handle, table, grid=False, **kw):
    """A lib.PostTable of ``handle`` -> {"params", "direction" (resolved), "frames", "columns" and Handle.goal_view's arrays: "rows", "open", "mask",
    "status", "totals", "grid"}.  The result stays with the table; nothing in the table changes."""
    direction = _offside_direction(handle, table) if handle.offside_device(table)[0] is not None else None
    p = resolve(len(table.rows), grid, table.team_mapping is not None, direction, handle.possession_device(table) is not None, **kw)
    res = handle.goal_view(table, p)
    return {"params": params_dict(p), "direction": int(p.direction) or direction, "frames": np.asarray(table.rows).copy(), "columns": table.columns.copy(), **res}


def _offside_direction(handle, table):
    """the direction the table's offside result settled (its clip record)"""
    import ctypes as C
    rows = len(table.rows)
    clip = np.zeros(1, lib.OFFSIDE_CLIP_DTYPE)
    if rows:
        handle._check(handle.L.eagle_post_offside_values(table._t, None, None, None, clip.ctypes.data_as(C.c_void_p)), "post_offside_values")
    return int(clip[0]["direction"])


def radians(v):
    """an `open` or `full` value -> radians, None for -1 (not evaluated)"""
    return None if int(v) < 0 else int(v) * UNIT


def lane(y_cross):
    """the slice that contains y_cross, or None outside the mouth"""
    if y_cross is None or not (y_cross == y_cross) or not Y0 <= y_cross < Y0 + 7.32:
        return None
    return min(63, int(math.floor((y_cross - Y0) / DY)))


def attacking_group(direction, towards_right):
    """the group that attacks the goal at x = 105 (towards_right) or at x = 0"""
    return 0 if (direction == lib.OFFSIDE_DIR_RIGHT) == bool(towards_right) else 1


def join_shots(d, flights):
    """Per K40 shot flight (lib.FLIGHT_DTYPE with shot >= 1): the ball's view of the goal it flies at, at the flight's first row, and whether the
    slice its line crosses is open.  Host arithmetic over the small record arrays."""
    out = []
    for i, f in enumerate(flights):
        if int(f["shot"]) < 1:
            continue
        r = int(f["row0"])
        g = attacking_group(d["direction"], float(f["vx"]) > 0.0)
        rec = d["rows"][r, g]
        ok = int(rec["ball_status"]) == lib.GOALVIEW_PT_OK
        k = lane(float(f["y_cross"]))
        out.append({"flight": i, "row": r, "frame": int(d["frames"][r]), "group": g, "status": lib.GOALVIEW_PT_NAMES[int(rec["ball_status"])],
                    "mask": "%016x" % int(rec["ball_mask"]), "open": radians(rec["ball_open"]), "full": radians(rec["ball_full"]) if ok else None,
                    "lane": k, "lane_open": None if k is None or not ok else not (int(rec["ball_mask"]) >> k) & 1})
    return out


def join_passes(d, events):
    """Per PASS event (lib.EVENT_DTYPE): the passer's open angle at the release row, the receiver's at the receive row and their difference."""
    member = {int(t["col"]): k for k, t in enumerate(d["totals"])}
    ids = lambda c: int(d["columns"][c]["id"]) if c >= 0 else None
    at = lambda c, r: radians(d["open"][member[c], r]) if c in member else None
    out = []
    for k, e in enumerate(events):
        if int(e["kind"]) != lib.EVENT_PASS:
            continue
        a, b = at(int(e["from_col"]), int(e["release_row"])), at(int(e["to_col"]), int(e["receive_row"]))
        out.append({"event": k, "frame": int(d["frames"][int(e["row"])]), "from_id": ids(int(e["from_col"])), "to_id": ids(int(e["to_col"])),
                    "passer_open": a, "receiver_open": b, "threat_added": None if a is None or b is None else b - a})
    return out


def totals_json(d):
    return [{"id": int(d["columns"][int(t["col"])]["id"]), "group": int(t["group"]), "rows": int(t["rows"]), "mean_open": int(t["sum_open"]) * UNIT / int(t["rows"]) if t["rows"] else None,
             "max_open": radians(t["max_open"]), "max_frame": int(d["frames"][int(t["max_row"])]) if t["max_row"] >= 0 else None, "chance_rows": int(t["chance_rows"])}
            for t in d["totals"]]


def to_json(d, flights=None, events=None, cells=False):
    """goal_view()'s dict in JSON's types only: ids in place of column indices, radians in place of units.  flights: the table's ball flights
    (Handle.ball_flight_values()["flights"]) for the per-shot join; events: its possession events for the per-pass join; cells: also the per-row records."""
    rec = d["rows"]
    out = {"params": d["params"], "direction": d["direction"], "unit": "rad",
           "rows": {"evaluated": [int((rec[:, g]["status"] == lib.GOALVIEW_OK).sum()) for g in (0, 1)],
                    "too_many": [int((rec[:, g]["status"] == lib.GOALVIEW_TOO_MANY).sum()) for g in (0, 1)]},
           "totals": totals_json(d)}
    if flights is not None:
        out["shots"] = join_shots(d, flights)
    if events is not None:
        out["passes"] = join_passes(d, events)
    if cells:
        ids = lambda c: int(d["columns"][c]["id"]) if c >= 0 else None
        out["cells"] = [{"frame": int(f), "groups": [{"blockers": int(o["n_blockers"]), "too_many": bool(o["status"]), "ball": lib.GOALVIEW_PT_NAMES[int(o["ball_status"])],
                                                      "ball_open": radians(o["ball_open"]), "best_id": ids(int(o["best_col"])), "best_open": radians(o["best_open"]),
                                                      "owner_id": ids(int(o["owner_col"])), "owner_open": radians(o["owner_open"])} for o in rec[r]]}
                        for r, f in enumerate(d["frames"])]
    return out
