"""The written definition of ball possession and pass events (include/eagle.h, eagle_post_possession / eagle_op_possession; csrc/possession.hip): an own
specification, the reference derives none of this.  Everything is float64, one operation at a time (numpy never contracts), sqrt and division correctly
rounded.  The contract is held TWICE: possession() is the scan formulation the kernels follow (every rule an inclusive max-scan of row indices),
state_machine() an independent plain loop over the rows carrying (current run, its length, last confirmed, owner); tests/test_possession_cpu.py holds
them against each other bit for bit.

Inputs: values [cols][rows][2], frames [rows] strictly ascending, columns (kind, id, video) in table order, mapping {id: team} or None, fps, radius,
min_hold, max_gap, no_ball (the table's EAGLE_POST_NO_BALL flag).  Outputs: a dict with cand, owner (int32 [rows], column indices or -1), dist (float64
[rows]), events (EVENT_DTYPE, ascending rows) and the intermediate rows of the scan formulation (ball, seg, head, headrow, run, conf, lastconf,
lastseg) for the tests that assert an edge was forced."""
import math

import numpy as np

PLAYER, GOALKEEPER, BALL, BOUNDARY = 0, 1, 2, 3
PASS, TURNOVER, UNKNOWN = 0, 1, 2
KIND_NAMES = ("pass", "turnover", "unknown")
RADIUS, MIN_HOLD = 2.0, 2             # conventional choices (max_gap: fps), not fitted to data
EVENT_DTYPE = np.dtype([("row", "<i4"), ("from_col", "<i4"), ("to_col", "<i4"), ("release_row", "<i4"), ("receive_row", "<i4"), ("kind", "<i4"),
                        ("reserved", "<i4", 2), ("x0", "<f8"), ("y0", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("length", "<f8"), ("duration", "<f8")])


def check(fps, radius, min_hold, max_gap):
    if not (int(fps) > 0 and int(min_hold) > 0 and int(max_gap) > 0 and 0.0 < float(radius) <= 1024.0):
        raise ValueError("possession: fps, min_hold, max_gap must be positive, radius within (0, 1024]")


def layout(columns, mapping, no_ball=False):
    """-> (ball column or -1, person columns in table order, team per column: -1 unknown).  The FIRST mapping entry with a column's id counts."""
    ball, persons, team = -1, [], np.full(max(len(columns), 1), -1, np.int32)
    for c, (kind, cid, video) in enumerate(columns):
        if kind not in (PLAYER, GOALKEEPER, BALL, BOUNDARY):
            raise ValueError("possession: unknown column kind")
        if video:
            continue
        if kind == BALL:
            if ball >= 0:
                raise ValueError("possession: more than one ball column")
            ball = c
        elif kind in (PLAYER, GOALKEEPER):
            persons.append(c)
            if mapping is not None:
                for k, v in mapping.items():
                    if int(k) == int(cid):
                        team[c] = int(v) if int(v) >= 0 else -1
                        break
    return (-1 if no_ball else ball), persons, team


def _present(cells):
    return np.isfinite(cells[..., 0]) & np.isfinite(cells[..., 1])


def candidates(values, columns, radius, no_ball=False):
    """§1 -> (ball bool [rows], cand int32 [rows], dist float64 [rows])"""
    values = np.asarray(values, np.float64)
    rows = values.shape[1]
    bcol, persons, _ = layout(columns, None, no_ball)
    r2 = float(radius) * float(radius)
    if bcol < 0:                              # no ball column (or NO_BALL): nothing is present
        return np.zeros(rows, bool), np.full(rows, -1, np.int32), np.full(rows, np.nan)
    ball = _present(values[bcol])
    best, bc = np.zeros(rows, np.float64), np.full(rows, -1, np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in persons:
            p = values[c]
            dx, dy = p[:, 0] - values[bcol][:, 0], p[:, 1] - values[bcol][:, 1]
            d2 = dx * dx + dy * dy
            take = ball & _present(p) & ((bc < 0) | (d2 < best))          # strictly nearer, or the first: a tie keeps the earlier column
            best[take], bc[take] = d2[take], c
        dist = np.where(bc >= 0, np.sqrt(best), np.nan)
    cand = np.where((bc >= 0) & (best <= r2), bc, -1).astype(np.int32)
    return ball, cand, dist


def _max_scan(flag):
    """per row the greatest index r' <= r with flag[r'], or -1"""
    idx = np.where(flag, np.arange(len(flag), dtype=np.int64), -1)
    return np.maximum.accumulate(idx) if len(idx) else idx


def _events(values, frames, bcol, team, fps, rows_ev, owner, lastconf, headrow):
    ev = np.zeros(len(rows_ev), EVENT_DTYPE)
    for i, r in enumerate(rows_ev):
        e = ev[i]
        e["row"], e["from_col"], e["to_col"] = r, owner[r - 1], owner[r]
        rel, rec = int(lastconf[r - 1]), int(headrow[r])
        e["release_row"], e["receive_row"] = rel, rec
        tf, tt = int(team[owner[r - 1]]), int(team[owner[r]])
        e["kind"] = UNKNOWN if tf < 0 or tt < 0 else (PASS if tf == tt else TURNOVER)
        x0, y0 = values[bcol, rel]
        x1, y1 = values[bcol, rec]
        e["x0"], e["y0"], e["x1"], e["y1"] = x0, y0, x1, y1
        with np.errstate(over="ignore"):
            dx, dy = np.float64(x1) - np.float64(x0), np.float64(y1) - np.float64(y0)
            e["length"] = np.sqrt(dx * dx + dy * dy)
        e["duration"] = np.float64(int(frames[rec]) - int(frames[rel])) / np.float64(int(fps))
    return ev


def possession(values, frames, columns, mapping, fps, radius=RADIUS, min_hold=MIN_HOLD, max_gap=None, no_ball=False):
    """the scan formulation (§1 - §4)"""
    max_gap = int(fps if max_gap is None else max_gap)
    check(fps, radius, min_hold, max_gap)
    values = np.asarray(values, np.float64)
    frames = np.asarray(frames, np.int64)
    rows = values.shape[1]
    assert len(frames) == rows and (np.diff(frames) > 0).all()
    bcol, persons, team = layout(columns, mapping, no_ball)
    ball, cand, dist = candidates(values, columns, radius, no_ball)
    r = np.arange(rows, dtype=np.int64)
    seg = ~ball
    head = np.ones(rows, bool)
    if rows:
        seg[0] = True
        seg[1:] |= np.diff(frames) > max_gap
        head[1:] = seg[1:] | (cand[1:] < 0) | (cand[1:] != cand[:-1])
    headrow = _max_scan(head)
    run = np.where(cand >= 0, r - headrow + 1, 0)
    conf = (cand >= 0) & (run >= int(min_hold))
    lastconf, lastseg = _max_scan(conf), _max_scan(seg)
    owned = ball & (lastconf >= 0) & (lastconf >= lastseg)
    owner = np.where(owned, cand[np.maximum(lastconf, 0)], -1).astype(np.int32) if rows else np.zeros(0, np.int32)
    flag = np.zeros(rows, bool)
    if rows:
        flag[1:] = ~seg[1:] & (owner[1:] >= 0) & (owner[:-1] >= 0) & (owner[1:] != owner[:-1])
    events = _events(values, frames, bcol, team, fps, np.flatnonzero(flag), owner, lastconf, headrow)
    return {"ball": ball, "cand": cand, "dist": dist, "seg": seg, "head": head, "headrow": headrow.astype(np.int32), "run": run.astype(np.int32), "conf": conf,
            "lastconf": lastconf.astype(np.int32), "lastseg": lastseg.astype(np.int32), "owner": owner, "events": events, "team": team, "persons": persons,
            "ball_col": bcol}


def state_machine(values, frames, columns, mapping, fps, radius=RADIUS, min_hold=MIN_HOLD, max_gap=None, no_ball=False):
    """The same outputs (cand, owner, dist, events) by a plain loop over the rows: python floats and ints, math.sqrt, no arrays of flags and no scans."""
    max_gap = int(fps if max_gap is None else max_gap)
    check(fps, radius, min_hold, max_gap)
    values = np.asarray(values, np.float64)
    rows = values.shape[1]
    bcol, persons, team = layout(columns, mapping, no_ball)
    r2 = float(radius) * float(radius)
    fin = math.isfinite
    cand, owner, dist, events = [], [], [], []
    cur, length, start = -1, 0, -1            # the current run: its candidate, its length in rows, its first row
    touch = -1                                # the last confirmed row of the present owner (or of the one before a loose spell)
    own = -1
    for r in range(rows):
        bx, by = (float(values[bcol, r, 0]), float(values[bcol, r, 1])) if bcol >= 0 else (math.nan, math.nan)
        has_ball = fin(bx) and fin(by)
        # the nearest person
        best, bc = 0.0, -1
        if has_ball:
            for c in persons:
                px, py = float(values[c, r, 0]), float(values[c, r, 1])
                if not (fin(px) and fin(py)):
                    continue
                dx, dy = px - bx, py - by
                d2 = dx * dx + dy * dy                 # (python floats are IEEE doubles: an overflow is inf, not an exception)
                if bc < 0 or d2 < best:
                    best, bc = d2, c
        dist.append(math.sqrt(best) if bc >= 0 else math.nan)
        c_now = bc if bc >= 0 and best <= r2 else -1
        cand.append(c_now)
        # a new segment forgets everything
        new_seg = r == 0 or not has_ball or int(frames[r]) - int(frames[r - 1]) > max_gap
        if new_seg:
            cur, length, start, touch, own = -1, 0, -1, -1, -1
        # the run
        if c_now < 0:
            cur, length, start = -1, 0, -1
        elif c_now == cur:
            length += 1
        else:
            cur, length, start = c_now, 1, r
        # confirmation makes (or keeps) an owner; its release row is kept for the event
        event = None
        if cur >= 0 and length >= int(min_hold):
            if own >= 0 and own != cur:
                event = (r, own, cur, touch, start)
            own, touch = cur, r
        if not has_ball:
            own = -1
        owner.append(own)
        if event is not None:
            events.append(event)
    ev = np.zeros(len(events), EVENT_DTYPE)
    for i, (r, a, b, rel, rec) in enumerate(events):
        x0, y0, x1, y1 = (float(values[bcol, rel, 0]), float(values[bcol, rel, 1]), float(values[bcol, rec, 0]), float(values[bcol, rec, 1]))
        dx, dy = x1 - x0, y1 - y0
        d2 = dx * dx + dy * dy
        tf, tt = int(team[a]), int(team[b])
        ev[i] = (r, a, b, rel, rec, UNKNOWN if tf < 0 or tt < 0 else (PASS if tf == tt else TURNOVER), (0, 0), x0, y0, x1, y1, math.sqrt(d2),
                 float(int(frames[rec]) - int(frames[rel])) / float(int(fps)))
    return {"cand": np.array(cand, np.int32).reshape(rows), "owner": np.array(owner, np.int32).reshape(rows), "dist": np.array(dist, np.float64).reshape(rows),
            "events": ev}


# ---- aggregates (summed on the host by eagle_amd/possession.py; defined here) -------------------------------------------------------------
def aggregates(res, frames, columns, fps):
    """-> (players, teams, pass_matrix): per person column in table order {"id", "type", "rows", "seconds", "passes_made", "passes_received",
    "turnovers_lost", "turnovers_won"}; per known team {team: share of the owned seconds} (0.0 each when nothing is owned); {(from id, to id): passes}.
    seconds: the sum of (frames[r] - frames[r - 1]) / fps over rows with owner[r] == owner[r - 1] >= 0 and not seg[r], added in row order."""
    owner, seg, team = res["owner"], res["seg"], res["team"]
    players, by_col = [], {}
    for c in res["persons"]:
        kind, cid, _ = columns[c]
        by_col[c] = {"id": int(cid), "type": "Player" if kind == PLAYER else "Goalkeeper", "rows": 0, "seconds": 0.0, "passes_made": 0, "passes_received": 0,
                     "turnovers_lost": 0, "turnovers_won": 0}
        players.append(by_col[c])
    team_s = {int(t): 0.0 for t in sorted(set(int(team[c]) for c in res["persons"])) if t >= 0}
    for r in range(len(owner)):
        o = int(owner[r])
        if o < 0:
            continue
        by_col[o]["rows"] += 1
        if r >= 1 and int(owner[r - 1]) == o and not seg[r]:
            dt = float(int(frames[r]) - int(frames[r - 1])) / float(int(fps))
            by_col[o]["seconds"] += dt
            if int(team[o]) >= 0:
                team_s[int(team[o])] += dt
    matrix = {}
    for e in res["events"]:
        a, b = by_col[int(e["from_col"])], by_col[int(e["to_col"])]
        if e["kind"] == PASS:
            a["passes_made"] += 1
            b["passes_received"] += 1
            matrix[(a["id"], b["id"])] = matrix.get((a["id"], b["id"]), 0) + 1
        elif e["kind"] == TURNOVER:
            a["turnovers_lost"] += 1
            b["turnovers_won"] += 1
    total = 0.0
    for t in team_s:
        total += team_s[t]
    teams = {t: (team_s[t] / total if total > 0.0 else 0.0) for t in team_s}
    return players, teams, matrix
