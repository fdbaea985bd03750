"""Ball possession and pass events of a processed clip table: who has the ball in each kept frame, when it changes feet, and whether the change was a
pass (same team), a turnover (other team) or of unknown kind (a team is not known), plus what that adds up to per id, per team and per pair of ids.

The rule is this project's own (the reference leaves the step to an analyst: its examples/pass.py draws a pass between two hand-chosen rows):
the person nearest to the ball and within ``radius`` metres is the candidate of a row; ``min_hold`` consecutive rows as candidate confirm an owner, who
keeps the ball while it flies or rolls until someone else is confirmed; a step of more than ``max_gap`` frames or a row without a ball forgets the
owner.  radius 2 m, min_hold 2 rows and max_gap = fps are conventional choices, not fitted to data.  Candidates, owners and events are computed on the
GPU from the table where the post-processor left it in HBM (include/eagle.h, eagle_post_possession; csrc/possession.hip); this module names the
columns and sums the aggregates on the host.  tests/possession_ref.py defines every output bit."""
import numpy as np

from . import lib

KIND_NAMES = ("pass", "turnover", "unknown")


def _team_of(columns, team_mapping):
    team = np.full(max(len(columns), 1), -1, np.int64)
    if team_mapping is not None:
        for c, k in enumerate(columns):
            if not k["video"] and int(k["kind"]) in (lib.POST_PLAYER, lib.POST_GOALKEEPER):
                for i, v in team_mapping.items():            # the first entry with the id counts, as in the library
                    if int(i) == int(k["id"]):
                        team[c] = int(v) if int(v) >= 0 else -1
                        break
    return team


def summarise(owner, events, frames, columns, team_mapping, fps, max_gap=None):
    """owner int32 [rows] and events (lib.EVENT_DTYPE) as the library gives them, the table's kept frame numbers and columns (lib.POSTCOL_DTYPE) -> the
    dict possession() returns.  Pure host arithmetic: sums in row order, so the figures are reproducible bit for bit."""
    gap = int(fps if max_gap is None else max_gap)
    frames = [int(f) for f in frames]
    team = _team_of(columns, team_mapping)
    kind_name = lambda c: "Player" if int(columns[c]["kind"]) == lib.POST_PLAYER else "Goalkeeper"
    by_col, players = {}, []
    for c, k in enumerate(columns):
        if k["video"] or int(k["kind"]) not in (lib.POST_PLAYER, lib.POST_GOALKEEPER):
            continue
        by_col[c] = {"id": int(k["id"]), "type": kind_name(c), "rows": 0, "seconds": 0.0, "passes_made": 0, "passes_received": 0, "turnovers_lost": 0,
                     "turnovers_won": 0}
        players.append(by_col[c])
    team_s = {int(t): 0.0 for t in sorted(set(int(team[c]) for c in by_col)) if t >= 0}
    rows_out = []
    for r, o in enumerate(owner):
        o = int(o)
        rows_out.append({"frame": frames[r], "id": by_col[o]["id"] if o >= 0 else None, "type": by_col[o]["type"] if o >= 0 else None})
        if o < 0:
            continue
        by_col[o]["rows"] += 1
        if r >= 1 and int(owner[r - 1]) == o and frames[r] - frames[r - 1] <= gap:      # (an owned row has a ball: only the frame step can start a segment)
            dt = float(frames[r] - frames[r - 1]) / float(int(fps))
            by_col[o]["seconds"] += dt
            if team[o] >= 0:
                team_s[int(team[o])] += dt
    ev_out, matrix = [], {}
    for e in events:
        a, b = by_col[int(e["from_col"])], by_col[int(e["to_col"])]
        kind = int(e["kind"])
        if kind == lib.EVENT_PASS:
            a["passes_made"] += 1
            b["passes_received"] += 1
            matrix[(a["id"], b["id"])] = matrix.get((a["id"], b["id"]), 0) + 1
        elif kind == lib.EVENT_TURNOVER:
            a["turnovers_lost"] += 1
            b["turnovers_won"] += 1
        ev_out.append({"frame": frames[int(e["row"])], "kind": KIND_NAMES[kind], "from_id": a["id"], "from_type": a["type"], "to_id": b["id"], "to_type": b["type"],
                       "release_frame": frames[int(e["release_row"])], "receive_frame": frames[int(e["receive_row"])], "x0": float(e["x0"]), "y0": float(e["y0"]),
                       "x1": float(e["x1"]), "y1": float(e["y1"]), "length": float(e["length"]), "duration": float(e["duration"])})
    total = 0.0
    for t in team_s:
        total += team_s[t]
    return {"owner": rows_out, "events": ev_out, "players": players, "teams": {t: (team_s[t] / total if total > 0.0 else 0.0) for t in team_s},
            "pass_matrix": matrix}


def possession(handle, table, fps, radius=2.0, min_hold=2, max_gap=None):
    """A lib.PostTable of ``handle`` -> {"owner": per kept frame {"frame", "id", "type"} (id and type None: nobody has the ball), "events": [{"frame",
    "kind": "pass" | "turnover" | "unknown", "from_id", "from_type", "to_id", "to_type", "release_frame", "receive_frame", "x0", "y0", "x1", "y1",
    "length" (m), "duration" (s)}], "players": per Player / Goalkeeper pitch column in table order {"id", "type", "rows", "seconds", "passes_made",
    "passes_received", "turnovers_lost", "turnovers_won"}, "teams": {team: share of the owned seconds}, "pass_matrix": {(from id, to id): passes}}."""
    p = lib.possession_params(fps, radius, min_hold, max_gap)
    _, owner, _, events = handle.possession(table, p)
    return summarise(owner, events, table.rows, table.columns, table.team_mapping, fps, p.max_gap)


def to_json(d):
    """The dict of possession() with JSON's key types: team keys as strings, the pass matrix as a list of {"from", "to", "count"}."""
    out = dict(d)
    out["teams"] = {str(t): s for t, s in d["teams"].items()}
    out["pass_matrix"] = [{"from": a, "to": b, "count": n} for (a, b), n in d["pass_matrix"].items()]
    return out


def from_json(j):
    """The inverse of to_json."""
    out = dict(j)
    out["teams"] = {int(t): s for t, s in j["teams"].items()}
    out["pass_matrix"] = {(e["from"], e["to"]): e["count"] for e in j["pass_matrix"]}
    return out
