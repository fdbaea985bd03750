"""Team shape of a processed clip table: each team as a body in every kept frame — where its centre is, how long and wide it stands, how much ground
its convex hull covers, how stretched it is, where its two lines are — and what that adds up to over the clip.

The integer records and the exact hulls are computed on the GPU from the table where the post-processor left it in HBM (include/eagle.h,
eagle_post_team_shape; csrc/shape.hip; tests/shape_ref.py defines every bit): positions quantised to 1/1024 m, integer sums after that.  This module
is pure host arithmetic on those integers.  Every numerator and denominator is a Python integer, so a derived float is one correctly rounded division of
exact integers, or the correctly rounded square root of such a quotient; the clip means are math.fsum (a correctly rounded sum) divided by a count.
Groups: 0 = team value 0, 1 = every other team (the minimap's red and blue); goalkeepers are in neither.  The rule is this project's own (the
reference's users derive such figures by hand from processed_data.json); nothing here is fitted to data."""
import math
from fractions import Fraction

import numpy as np

from . import lib

Q = lib.SHAPE_Q
MEAN_KEYS = ("length", "width", "area", "stretch")


def group_values(rec, hull, ids):
    """One lib.SHAPE_DTYPE record, its int32 [SHAPE_HULL_CAP] vertex columns and the table's column ids -> the group's dict (None entries where n == 0)"""
    n = int(rec["n"])
    out = {"n": n, "centroid": None, "length": None, "width": None, "area": None, "stretch": None, "low_line": None, "high_line": None, "low_ids": [], "high_ids": [],
           "hull": [int(ids[c]) for c in hull if c >= 0], "hull_n": int(rec["hull_n"]), "hull_cut": bool(int(rec["flags"]) & lib.SHAPE_CUT)}
    if n == 0:
        return out
    sx, sy, sxx, syy = (int(rec[k]) for k in ("sum_x", "sum_y", "sum_xx", "sum_yy"))
    out["centroid"] = (sx / (n * Q), sy / (n * Q))
    out["length"] = (int(rec["max_x"]) - int(rec["min_x"])) / Q
    out["width"] = (int(rec["max_y"]) - int(rec["min_y"])) / Q
    out["area"] = int(rec["area2"]) / (2 * Q * Q)
    out["stretch"] = math.sqrt((n * (sxx + syy) - sx * sx - sy * sy) / (n * n * Q * Q))       # sqrt(var_x + var_y), the numerator n sum(q^2) - (sum q)^2 exact
    out["low_line"], out["high_line"] = int(rec["min_x"]) / Q, int(rec["max_x"]) / Q
    return out


def centroid_distance(a, b):
    """Two records with n > 0 -> the distance of their centroids in metres: sqrt of one exact quotient"""
    na, nb = int(a["n"]), int(b["n"])
    dx = int(a["sum_x"]) * nb - int(b["sum_x"]) * na
    dy = int(a["sum_y"]) * nb - int(b["sum_y"]) * na
    return math.sqrt((dx * dx + dy * dy) / (na * nb * Q) ** 2)


def derive(rec, hull, columns, frames=None, line_members=None):
    """lib.SHAPE_DTYPE [rows, 2], int32 [rows, 2, cap], the table's columns (lib.POSTCOL_DTYPE) -> {"rows": [{"frame", "groups": [g0, g1],
    "centroid_distance"}], "clip": {...}}.  line_members (optional): per row and group the ids standing on the low and on the high line, [(low, high)];
    without it the lines carry the earliest column's id only (col_min_x / col_max_x of the record)."""
    ids = [int(k["id"]) for k in columns]
    rows = []
    for r in range(len(rec)):
        groups = []
        for g in (0, 1):
            d = group_values(rec[r, g], hull[r, g], ids)
            if d["n"]:
                if line_members is not None:
                    d["low_ids"], d["high_ids"] = [list(map(int, v)) for v in line_members[r][g]]
                else:
                    d["low_ids"], d["high_ids"] = [ids[int(rec[r, g]["col_min_x"])]], [ids[int(rec[r, g]["col_max_x"])]]
            groups.append(d)
        both = groups[0]["n"] > 0 and groups[1]["n"] > 0
        rows.append({"frame": None if frames is None else int(frames[r]), "groups": groups,
                     "centroid_distance": centroid_distance(rec[r, 0], rec[r, 1]) if both else None})
    return {"rows": rows, "clip": clip_values(rec, rows)}


def clip_values(rec, rows):
    """the means over the rows with n >= 3 per group, the mean centroid distance over the rows where both groups are present, and who defends the left"""
    out = {"groups": [], "centroid_distance": None, "defends_left": None}
    for g in (0, 1):
        use = [r["groups"][g] for r in rows if r["groups"][g]["n"] >= 3]
        m = {"rows": len(use)}
        for k in MEAN_KEYS:
            m[k] = math.fsum(d[k] for d in use) / len(use) if use else None
        m["centroid"] = (math.fsum(d["centroid"][0] for d in use) / len(use), math.fsum(d["centroid"][1] for d in use) / len(use)) if use else None
        out["groups"].append(m)
    both = [r for r in range(len(rows)) if int(rec[r, 0]["n"]) > 0 and int(rec[r, 1]["n"]) > 0]
    if both:
        out["centroid_distance"] = math.fsum(rows[r]["centroid_distance"] for r in both) / len(both)
        # the same number of rows on both sides: the smaller sum of exact centroid x has the smaller mean
        s = [sum(Fraction(int(rec[r, g]["sum_x"]), int(rec[r, g]["n"])) for r in both) for g in (0, 1)]
        out["defends_left"] = [s[0] < s[1], s[1] < s[0]]
    return out


def shape(handle, table):
    """A lib.PostTable of ``handle`` (with a team mapping) -> derive()'s dict, the lines with every id standing on them.  The records stay with the table
    (Handle.team_shape_device; the minimap's hull layer draws them)."""
    rec, hull = handle.team_shape(table)
    columns = table.columns
    groups = member_columns(columns, table.team_mapping)
    values = np.asarray(table.values)
    lines = []
    for r in range(len(rec)):
        row = []
        for g in (0, 1):
            cols = groups[g]
            x = values[cols, r, 0] if cols else np.zeros(0)
            y = values[cols, r, 1] if cols else np.zeros(0)
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(x) & np.isfinite(y) & (np.abs(x) <= 1024.0) & (np.abs(y) <= 1024.0)
            q = np.floor(np.where(ok, x, 0.0) * float(Q) + 0.5).astype(np.int64)
            ids = [int(k["id"]) for k in columns]
            present = [(c, int(v)) for c, v, o in zip(cols, q, ok) if o]
            row.append(([ids[c] for c, v in present if v == int(rec[r, g]["min_x"])], [ids[c] for c, v in present if v == int(rec[r, g]["max_x"])]))
        lines.append(row)
    return derive(rec, hull, columns, table.rows, lines)


def member_columns(columns, team_mapping):
    """the member columns of the two groups in table order (the library's rule: Player pitch columns with a non-negative mapping entry)"""
    tm = {int(i): int(v) for i, v in (team_mapping or {}).items()}
    out = ([], [])
    for c, k in enumerate(columns):
        if not k["video"] and int(k["kind"]) == lib.POST_PLAYER and int(k["id"]) in tm and tm[int(k["id"])] >= 0:
            out[0 if tm[int(k["id"])] == 0 else 1].append(c)
    return out


def to_json(d):
    """derive()'s dict in JSON's types only (tuples become lists)"""
    def conv(v):
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        return v
    return conv(d)


def from_json(j):
    """The inverse of to_json: centroids are tuples again"""
    def conv(v, key=None):
        if isinstance(v, dict):
            return {k: conv(x, k) for k, x in v.items()}
        if isinstance(v, list):
            return tuple(v) if key == "centroid" else [conv(x) for x in v]
        return v
    return conv(j)
