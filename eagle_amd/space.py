"""Space per player of a processed clip table: how much room each player has — the area of the pitch nearer to him than to anybody else, where that
area lies (the thirds of the pitch along x), how far the nearest opponent is, how often an opponent stands within reach and who usually marks him.

The integers are computed on the GPU from the table where the post-processor left it in HBM (include/eagle.h, eagle_post_space; csrc/space.hip;
tests/space_ref.py defines every bit): per row the exact nearest-site partition of the pitch grid among the present members, per site the nearest
opponent and the opponents within the radius, per member the totals.  This module is pure host arithmetic on those integers: an area is cells / R^2
square metres, a mean is one correctly rounded division of exact integers, a distance is the correctly rounded square root of an exact integer divided by
1024, and a mean distance is math.fsum of those over their number.  Groups: 0 = team value 0, 1 = every other team, 2 = the goalkeepers (they own
area; they mark nobody and nobody marks them).

Limits: the nearest-site rule ignores velocity (the control surface is the stage that does not); an area follows a person over the whole clip only when
the table was built with the id merge (--merge-ids), otherwise it follows a tracker id; rows with more than 32 present members are skipped; there is no
minimap layer.  Rows are counted, not weighted by the frame step.  The rule is this project's own; the 3 m radius is a conventional choice."""
import json
import math

import numpy as np

from . import lib

Q = lib.SHAPE_Q
PITCH_CELLS = 105 * 68


def _site_of(rec, sites, r, col):
    """the site record of table column `col` on row r, or None (absent, or the row is not active)"""
    if col < 0 or rec[r]["status"] != lib.SPACE_ACTIVE:
        return None
    k = np.nonzero(sites[r, :rec[r]["n_sites"]]["col"] == col)[0]
    return sites[r, k[0]] if len(k) else None


def _area(s, R):
    return None if s is None else int(s["cells"].sum()) / (R * R)


def derive(rec, sites, totals, columns, params, frames=None, owner=None, events=None, per_row=False):
    """lib.SPACE_ROW_DTYPE [rows], lib.SPACE_SITE_DTYPE [rows, 32], lib.SPACE_TOTALS_DTYPE [members], the table's columns (lib.POSTCOL_DTYPE); owner int32
    [rows] and events lib.EVENT_DTYPE of a possession result, or None -> the dict described in the module's docstring (JSON's types only, apart from
    None)"""
    R, rows = int(params.cells_per_metre), len(rec)
    ids = [int(k["id"]) for k in columns]
    active = rec["status"] == lib.SPACE_ACTIVE
    n_active = int(active.sum())
    cells = PITCH_CELLS * R * R
    out = {"params": {"cells_per_metre": R, "goalkeepers": int(bool(params.goalkeepers)), "radius": float(params.radius)}, "rows": rows, "active_rows": n_active,
           "skipped_rows": int((rec["status"] == lib.SPACE_TOO_MANY).sum()), "ids": [], "teams": []}
    used = sites["col"] >= 0
    marked = used & (sites["near_col"] >= 0)
    for t in totals:
        c, n = int(t["col"]), int(t["rows"])
        tot = [int(v) for v in t["cells"]]
        mine = marked & (sites["col"] == c)
        dist = [math.sqrt(int(v)) / Q for v in sites["near_d2"][mine]]
        marker = None
        if len(dist):
            cols, cnt = np.unique(sites["near_col"][mine], return_counts=True)       # (ascending: of equal counts the earlier column)
            marker = ids[int(cols[np.argmax(cnt)])]
        out["ids"].append({"id": ids[c], "goalkeeper": int(columns[c]["kind"]) == lib.POST_GOALKEEPER, "group": int(t["group"]), "rows": n,
                           "mean_area": sum(tot) / (n * R * R) if n else None, "min_area": int(t["min"]) / (R * R) if n else None,
                           "max_area": int(t["max"]) / (R * R) if n else None, "thirds": [v / sum(tot) for v in tot] if sum(tot) else None,
                           "opponent_rows": int(t["opp_rows"]), "mean_nearest": math.fsum(dist) / len(dist) if dist else None,
                           "pressed_share": int(t["within_rows"]) / n if n else None, "mean_within": int(t["within_sum"]) / n if n else None, "marker": marker})
    for g in range(3):
        tot = [int(rec["cells"][active, g, t].sum()) for t in range(3)]
        out["teams"].append({"group": g, "mean_share": sum(tot) / (n_active * cells) if n_active else None, "thirds": [v / sum(tot) for v in tot] if sum(tot) else None,
                             "mean_present": int(rec["n"][active, g].sum()) / n_active if n_active else None})
    if owner is not None:
        out["possession"] = []
        for r in np.nonzero(np.asarray(owner) >= 0)[0]:
            s = _site_of(rec, sites, r, int(owner[r]))
            if s is not None:
                out["possession"].append({"row": int(r), "frame": None if frames is None else int(frames[r]), "id": ids[int(owner[r])], "area": _area(s, R),
                                          "within": int(s["within"])})
    if events is not None:
        out["passes"] = []
        for e in events:
            if int(e["kind"]) != lib.EVENT_PASS:
                continue
            a, b = int(e["release_row"]), int(e["receive_row"])
            passer, at_release, at_receive = _site_of(rec, sites, a, int(e["from_col"])), _site_of(rec, sites, a, int(e["to_col"])), _site_of(rec, sites, b, int(e["to_col"]))
            out["passes"].append({"row": int(e["row"]), "release_row": a, "receive_row": b, "from": ids[int(e["from_col"])], "to": ids[int(e["to_col"])],
                                  "passer_within": None if passer is None else int(passer["within"]), "receiver_area_release": _area(at_release, R),
                                  "receiver_area_receive": _area(at_receive, R)})
    if per_row:
        out["per_row"] = [{"frame": None if frames is None else int(frames[r]), "status": lib.SPACE_STATUS_NAMES[int(rec[r]["status"])], "n": [int(v) for v in rec[r]["n"]],
                           "share": [int(v) / cells for v in rec[r]["cells"].sum(1)],
                           "sites": [{"id": ids[int(s["col"])], "group": int(s["group"]), "area": _area(s, R),
                                      "nearest": math.sqrt(int(s["near_d2"])) / Q if s["near_col"] >= 0 else None,
                                      "nearest_id": ids[int(s["near_col"])] if s["near_col"] >= 0 else None, "within": int(s["within"])}
                                     for s in sites[r] if s["col"] >= 0]} for r in range(rows)]
    return out


def space(handle, table, cells_per_metre=1, goalkeepers=True, radius=3.0, per_row=False):
    """A lib.PostTable of ``handle`` (with a team mapping) -> derive()'s dict.  The result stays with the table (Handle.space_device).  With a possession
    result on the table (Handle.possession) the owner's area per row and the passes' figures are added."""
    params = lib.space_params(cells_per_metre, int(bool(goalkeepers)), radius)
    rec, sites, totals = handle.space(table, params)
    owner = events = None
    if handle.possession_device(table):
        owner, events = handle.possession_values(table)[1], handle.events(table)
    return derive(rec, sites, totals, table.columns, params, table.rows, owner, events, per_row)


def to_json(d):
    """derive()'s dict as space.json holds it: derive() uses JSON's types only, so this is what json.load gives back of json.dump"""
    return json.loads(json.dumps(d))
