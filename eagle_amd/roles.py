"""Player roles of a processed clip table: what a team's players DO, whatever ids the tracker gave them — the team's mean formation, its lines, a
label such as 4-4-2, how long each id played each role, every row at which an id changed its role, and who held each role when.

The assignment is computed on the GPU from the table where the post-processor left it in HBM (include/eagle.h, eagle_post_roles; csrc/roles.hip;
tests/roles_ref.py defines every bit): per row the exact least-cost assignment of the present members of a group to R role positions, re-estimated from
the assignment.  This module is pure host arithmetic on those integers: every derived float is one correctly rounded division of exact integers, or the
correctly rounded square root of one.  Role positions are relative to the row's centre (the rounded mean of the present members), in metres.
Groups: 0 = team value 0, 1 = every other team; goalkeepers are in neither.  The orientation comes from the team shape (shape.clip_values'
"defends_left"): the x of the group that defends the right is mirrored, so depth grows away from the own goal; with the orientation unknown the label is
None and the lines are those of the plain x.  The rule is this project's own; the defaults are conventional choices and nothing here is fitted to data."""
import ctypes as C
import math

import numpy as np

from . import lib, shape

Q = lib.SHAPE_Q


def split_lines(depths, lines=3):
    """depths: one exact number (an integer) per role, larger = farther from the own goal -> (order, groups): the roles sorted by (depth, role) and
    that order cut into `lines` lines at the lines - 1 largest gaps between consecutive depths; of equal gaps the one nearer the own goal is cut."""
    if not 2 <= lines <= 4:
        raise ValueError("lines %r outside 2 .. 4" % (lines,))
    if lines > len(depths):
        raise ValueError("%d lines of %d roles" % (lines, len(depths)))
    order = sorted(range(len(depths)), key=lambda j: (depths[j], j))
    gaps = sorted(range(len(order) - 1), key=lambda i: (-(depths[order[i + 1]] - depths[order[i]]), i))[:lines - 1]
    out, at = [], 0
    for i in sorted(gaps):
        out.append(order[at:i + 1])
        at = i + 1
    out.append(order[at:])
    return order, out


def label_of(groups):
    return "-".join(str(len(g)) for g in groups)


def group_values(mg, R, rows, mirror, lines):
    """One lib.ROLE_GROUP_DTYPE record -> the group's dict; mirror: None (orientation unknown), False or True (the group defends the right)"""
    ok = int(mg["status"]) == lib.ROLE_MODEL_OK
    out = {"status": "ok" if ok else "no_seeds", "active_rows": int(mg["active_rows"]), "active_share": int(mg["active_rows"]) / rows if rows else None,
           "oriented": mirror is not None, "roles": [], "order": [], "lines": [], "label": None}
    if not ok:
        return out
    sign = -1 if mirror else 1
    depths = [sign * int(mg["mean"][j][0]) for j in range(R)]
    out["order"], out["lines"] = split_lines(depths, lines)
    if mirror is not None:
        out["label"] = label_of(out["lines"])
    line_of = {j: k for k, g in enumerate(out["lines"]) for j in g}
    for j in range(R):
        n, sx, sy, sxx, syy = int(mg["count"][j]), int(mg["sum"][j][0]), int(mg["sum"][j][1]), int(mg["sum2"][j][0]), int(mg["sum2"][j][1])
        out["roles"].append({"role": j, "mean": [int(mg["mean"][j][0]) / Q, int(mg["mean"][j][1]) / Q], "depth": depths[j] / Q, "line": line_of[j], "count": n,
                             "played": [sx / (n * Q), sy / (n * Q)] if n else None,                   # the mean of the final assignment itself
                             "spread": math.sqrt((n * (sxx + syy) - sx * sx - sy * sy) / (n * n * Q * Q)) if n else None})
    return out


def derive(rec, mroles, model, columns, member_cols, params, frames=None, defends_left=None, lines=3, per_row=False):
    """lib.ROLE_ROW_DTYPE [rows, 2], int8 [members, rows], lib.ROLE_MODEL_DTYPE [1], the table's columns (lib.POSTCOL_DTYPE), the member columns of the
    two groups (shape.member_columns) -> the dict described in the module's docstring (JSON's types only, apart from None)"""
    R, rows = int(params.roles), len(rec)
    ids = [int(k["id"]) for k in columns]
    out = {"params": {"roles": R, "min_present": int(params.min_present), "iterations": int(params.iterations), "lines": int(lines)},
           "changed": [int(v) for v in model["changed"][0][:int(params.iterations)]], "groups": [], "ids": [], "swaps": [], "stints": []}
    for g in (0, 1):
        mirror = None if defends_left is None or not (defends_left[0] or defends_left[1]) else not defends_left[g]
        out["groups"].append(group_values(model["group"][0, g], R, rows, mirror, lines))
    m = 0
    for g in (0, 1):
        for c in member_cols[g]:
            row_roles = mroles[m]
            m += 1
            out["ids"].append({"id": ids[c], "group": g, "rows": [int((row_roles == j).sum()) for j in range(R)]})
            last = -1
            for r in np.nonzero(row_roles >= 0)[0]:
                j = int(row_roles[r])
                if last >= 0 and j != last:
                    out["swaps"].append({"row": int(r), "frame": None if frames is None else int(frames[r]), "id": ids[c], "from": last, "to": j})
                last = j
    out["swaps"].sort(key=lambda s: (s["row"], s["id"]))
    for g in (0, 1):
        per_role = []
        for j in range(R):
            held, st = rec[:, g]["col"][:, j], []
            for r in np.nonzero(held >= 0)[0]:
                i = ids[int(held[r])]
                if st and st[-1][2] == i:
                    st[-1][1] = int(r)
                else:
                    st.append([int(r), int(r), i])
            per_role.append(st)
        out["stints"].append(per_role)
    if per_row:
        out["rows"] = [{"frame": None if frames is None else int(frames[r]),
                        "groups": [{"status": lib.ROLE_STATUS_NAMES[int(rec[r, g]["status"])], "n": int(rec[r, g]["n"]), "cost": int(rec[r, g]["cost"]),
                                    "centre": [int(rec[r, g]["cx"]) / Q, int(rec[r, g]["cy"]) / Q],
                                    "ids": [ids[int(c)] if c >= 0 else None for c in rec[r, g]["col"][:R]]} for g in (0, 1)]} for r in range(rows)]
    return out


def roles(handle, table, roles=10, min_present=8, iterations=8, lines=3, per_row=False):
    """A lib.PostTable of ``handle`` (with a team mapping) -> derive()'s dict.  The result stays with the table (Handle.roles_device).  The team shape
    is computed if the table has none (its clip figures say who defends the left)."""
    params = lib.role_params(roles, min_present, iterations)
    split_lines([0] * int(roles), lines)                        # (refuses a bad `lines` before any work)
    rec, mroles, model = handle.roles(table, params)
    n = len(table.rows)
    if handle.team_shape_device(table)[0] is None:
        srec, hull = handle.team_shape(table)
    else:
        srec, hull = np.zeros((n, 2), lib.SHAPE_DTYPE), np.zeros((n, 2, lib.SHAPE_HULL_CAP), np.int32)
        if n:
            handle._check(handle.L.eagle_post_team_shape_values(table._t, srec.ctypes.data_as(C.c_void_p), hull.ctypes.data_as(C.c_void_p)), "post_team_shape_values")
    left = shape.derive(srec, hull, table.columns)["clip"]["defends_left"]
    return derive(rec, mroles, model, table.columns, shape.member_columns(table.columns, table.team_mapping), params, table.rows, left, lines, per_row)


def to_json(d):
    """derive()'s dict as JSON takes it (it holds JSON's types only: a deep copy)"""
    def conv(v):
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        return v
    return conv(d)


def from_json(j):
    """The inverse of to_json"""
    return to_json(j)
