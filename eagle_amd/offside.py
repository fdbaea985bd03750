"""Offside lines of a processed clip table and an offside verdict per pass: where the line stood for each team in every kept frame, who stood on it,
who was beyond it and by how much, how often each player was in an offside position, and for every pass whether the receiver was onside, close or
offside at the moment the ball was played.

The integers are computed on the GPU from the table where the post-processor left it in HBM (include/eagle.h, eagle_post_offside; csrc/offside.hip;
tests/offside_ref.py defines every bit): positions are quantised once to q = 1 / 1024 m; per row and attacking team the line is the deepest of the
second-last opponent, the halfway line and the ball; a margin is the attacker's depth minus the line, positive beyond it, level is onside.  This module
is pure host arithmetic on those integers: metres are q / 1024, a share is one correctly rounded division of exact integers.  Groups: 0 = team value 0,
1 = every other team.  "attacking": the group whose members the margins belong to.

Limits: only the foot point of a box is known, not the head or body; a defender outside the picture is not in the table, so the line can be too shallow
when the camera does not see the last defender; a keeper is given to the half he stands in; goal kicks, throw-ins and corners, which the Law exempts,
are not recognised; "interfering with play" is not judged, the verdict is about the receiver's position only; a margin follows a person over the whole
clip only when the table was built with the id merge (--merge-ids), otherwise it follows a tracker id.  The rule is this project's own; the 0.5 m
tolerance is a conventional choice."""
import json

import numpy as np

from . import lib

Q = lib.SHAPE_Q
FLAG_NAMES = ((lib.OFFSIDE_KEEPER_ASSUMED, "keeper_assumed"), (lib.OFFSIDE_BY_DEFENDER, "by_defender"), (lib.OFFSIDE_BY_BALL, "by_ball"), (lib.OFFSIDE_BY_HALF, "by_half"),
              (lib.OFFSIDE_NO_BALL, "no_ball"))


def metres(q):
    return int(q) / Q


def _margin(q):
    return None if int(q) == lib.OFFSIDE_NONE else metres(q)


def line_by(flags):
    """the term that set the line: "defender", "ball" or "half" """
    return "defender" if flags & lib.OFFSIDE_BY_DEFENDER else "ball" if flags & lib.OFFSIDE_BY_BALL else "half"


def derive(rec, margins, totals, clip, columns, params, frames=None, events=None, offside_events=None, per_row=False):
    """lib.OFFSIDE_ROW_DTYPE [rows, 2], margins int32 [members, rows], lib.OFFSIDE_TOTALS_DTYPE [members], lib.OFFSIDE_CLIP_DTYPE [1], the table's columns
    (lib.POSTCOL_DTYPE); events lib.EVENT_DTYPE of a possession result with their lib.OFFSIDE_EVENT_DTYPE records, or None -> the dict described in the
    module's docstring (JSON's types only, apart from None)"""
    rows = len(rec)
    ids = [int(k["id"]) for k in columns]
    c = clip[0]
    out = {"params": {"direction": lib.OFFSIDE_DIR_NAMES[int(params.direction)] if params.direction else "auto", "assume_keeper": int(bool(params.assume_keeper)),
                      "tolerance": float(params.tolerance)},
           "rows": rows,
           "clip": {"direction": lib.OFFSIDE_DIR_NAMES[int(c["direction"])], "votes": {"neg": int(c["neg"]), "pos": int(c["pos"]), "zero": int(c["zero"])},
                    "members": [int(v) for v in c["n_members"]], "keepers": int(c["n_keepers"])},
           "teams": [], "ids": []}
    for a in (0, 1):
        o = rec[:, a]
        ok = o["status"] == lib.OFFSIDE_OK
        n = int(ok.sum())
        out["teams"].append({"group": a, "ok_rows": n, "too_few_rows": int((o["status"] == lib.OFFSIDE_TOO_FEW).sum()),
                             "rows_with_offside": int((o["n_off"][ok] > 0).sum()), "offside_positions": int(o["n_off"][ok].astype(np.int64).sum()),
                             "mean_line": int(o["line_qx"][ok].astype(np.int64).sum()) / (n * Q) if n else None,
                             "keeper_assumed_rows": int(((o["flags"] & lib.OFFSIDE_KEEPER_ASSUMED) != 0).sum()),
                             "line_by": {name: int(((o["flags"] & bit) != 0).sum()) for bit, name in FLAG_NAMES[1:4]}})
    for t in totals:
        n = int(t["rows"])
        out["ids"].append({"id": ids[int(t["col"])], "group": int(t["group"]), "rows": n, "offside_rows": int(t["off_rows"]),
                           "offside_share": int(t["off_rows"]) / n if n else None, "max_margin": _margin(t["max_margin"])})
    if events is not None:
        out["passes"] = []
        for e, o in zip(events, offside_events):
            if int(e["kind"]) != lib.EVENT_PASS:
                continue
            st = int(o["status"])
            out["passes"].append({"row": int(e["row"]), "release_row": int(e["release_row"]), "receive_row": int(e["receive_row"]),
                                  "release_frame": None if frames is None else int(frames[int(e["release_row"])]), "from": ids[int(e["from_col"])],
                                  "to": ids[int(e["to_col"])], "status": lib.OFFSIDE_EV_STATUS_NAMES[st], "verdict": lib.OFFSIDE_VERDICT_NAMES[int(o["verdict"])],
                                  "margin": _margin(o["margin"]), "line": metres(o["line_qx"]) if st == lib.OFFSIDE_EV_OK else None,
                                  "teammates_offside": int(o["n_off"]) if st == lib.OFFSIDE_EV_OK else None,
                                  "bypassed": int(o["bypassed"]) if int(o["bypassed"]) >= 0 else None})
    if per_row:
        member_cols = [int(t["col"]) for t in totals]
        out["per_row"] = []
        for r in range(rows):
            teams = []
            for a in (0, 1):
                o = rec[r, a]
                ok = int(o["status"]) == lib.OFFSIDE_OK
                mine = [(m, int(margins[m, r])) for m, t in enumerate(totals) if int(t["group"]) == a and int(margins[m, r]) != lib.OFFSIDE_NONE]
                teams.append({"group": a, "status": lib.OFFSIDE_STATUS_NAMES[int(o["status"])], "line": metres(o["line_qx"]) if ok else None,
                              "line_by": line_by(int(o["flags"])) if ok else None, "keeper_assumed": bool(o["flags"] & lib.OFFSIDE_KEEPER_ASSUMED),
                              "no_ball": bool(o["flags"] & lib.OFFSIDE_NO_BALL), "second_last": ids[int(o["second_col"])] if ok else None,
                              "attackers": int(o["n_att"]), "defenders": int(o["n_def"]), "keepers_seen": int(o["keepers_seen"]),
                              "on_the_line": [ids[member_cols[m]] for m, v in mine if v == 0], "beyond": [{"id": ids[member_cols[m]], "margin": metres(v)} for m, v in mine if v > 0],
                              "max_margin": _margin(o["max_margin"]), "max_id": ids[int(o["max_col"])] if int(o["max_col"]) >= 0 else None})
            out["per_row"].append({"frame": None if frames is None else int(frames[r]), "teams": teams})
    return out


def offside(handle, table, direction="auto", tolerance=0.5, assume_keeper=True, per_row=False):
    """A lib.PostTable of ``handle`` (with a team mapping) -> derive()'s dict.  The result stays with the table (Handle.offside_device).  With a
    possession result on the table (Handle.possession) every pass gets its verdict."""
    params = lib.offside_params(direction_value(direction), int(bool(assume_keeper)), tolerance)
    rec, margins, totals, clip = handle.offside(table, params)
    events = off_ev = None
    if handle.possession_device(table):
        events, off_ev = handle.events(table), handle.offside_events(table)
    return derive(rec, margins, totals, clip, table.columns, params, table.rows, events, off_ev, per_row)


def direction_value(direction):
    """"auto", "right", "left" (or the lib.OFFSIDE_DIR_* value itself) -> lib.OFFSIDE_DIR_*"""
    if isinstance(direction, str):
        try:
            return {"auto": lib.OFFSIDE_DIR_AUTO, "right": lib.OFFSIDE_DIR_RIGHT, "left": lib.OFFSIDE_DIR_LEFT}[direction.lower()]
        except KeyError:
            raise lib.EagleError(f"unknown offside direction {direction!r} (auto, right or left)") from None
    return int(direction)


def to_json(d):
    """derive()'s dict as offside.json holds it: derive() uses JSON's types only, so this is what json.load gives back of json.dump"""
    return json.loads(json.dumps(d))


def from_json(text_or_dict):
    """offside.json's text (or what json.load made of it) -> derive()'s dict"""
    return json.loads(text_or_dict) if isinstance(text_or_dict, (str, bytes)) else to_json(text_or_dict)
