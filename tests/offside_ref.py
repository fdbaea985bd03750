"""numpy / Python-integer restatement of the offside stage (include/eagle.h, eagle_post_offside / eagle_op_offside; csrc/offside.hip): per row and
attacking team the offside line and every attacker's margin beyond it, per pass a verdict about the receiver.  It is the single written definition of
every output bit: the kernels equal it bit for bit.  OWN SPEC: the reference leaves the question to a reader with a ruler over pass.png.

GROUPS, MEMBERS, PRESENT, QUANTISE are shape_ref's (members, quantise): groups 0 (team value 0) and 1 (any other non-negative team value) hold the
Player pitch columns (video == 0) with a mapping entry; the FIRST entry for an id counts (here the mapping is a dict, or a list of (id, value) pairs
that may repeat an id); a mapping is required; a member is PRESENT on a row when x and y are finite and |x|, |y| <= 1024 m; q = floor(v * 1024 + 0.5) in
float64, |q| <= 2^20.  Integers only behind that step.

KEEPERS: the Goalkeeper pitch columns, mapped or not.  BALL: the one Ball pitch column; absent when there is none or the table is flagged NO_BALL
(no_ball=True), else present on a row by the members' rule.  More than one Ball pitch column, a column of unknown kind, more than
shape_ref.MAX_MEMBERS members and keepers are refused.

DIRECTION: RIGHT (1), group 0 attacks towards x = 105; LEFT (2), towards x = 0; AUTO (0), a vote over the rows on which both groups have a present
member: s_r = sign(sum_x0 n1 - sum_x1 n0), neg = #{s_r < 0}, pos = #{s_r > 0}, zero = #{s_r == 0}; neg > pos: group 0 stands on the left and attacks
RIGHT; pos > neg: LEFT; else unresolved (0): every row has status NO_DIRECTION and nothing else is computed.  The votes are counted for a forced
direction too.  CLIP record: the resolved direction, the requested one, neg, pos, zero, the members per group, the keepers.

DEPTH for the attacking group a, defenders d = 1 - a: u = qx when a attacks right, else u = U_MAX - qx, U_MAX = 107520 = 105 * 1024.  Greater u is
nearer the defenders' goal line; U_HALF = 53760.

DEFENDERS of a row: the present members of d and every present keeper with u > U_HALF (a keeper "seen"; one exactly on the halfway line is nobody's):
K = n_def of them.  SECOND: a keeper was seen or assume_keeper == 0: the second-largest of the K depths as a multiset (two level defenders: second ==
largest), K < 2 is status TOO_FEW.  No keeper seen and assume_keeper != 0: the keeper is taken to stand on the goal line behind everyone, second = the
largest depth, K < 1 is TOO_FEW, flag KEEPER_ASSUMED.  second_col = the earliest table column among the defenders at depth second.

LINE = max(second, U_HALF, u_ball), the ball's term only when the ball is present on the row (else flag NO_BALL).  One of BY_DEFENDER, BY_BALL, BY_HALF
names the term that set it, on a tie in that order.  line_qx = the line mapped back to qx.

MARGINS: every present member of a: m = u - line; in an offside position iff m > 0 (level is onside).  An absent member and every member on a row that
is not OK: NONE (INT32_MIN).  The row record [row][a]: status, flags, line_qx, second_col, n_att (the present members of a), n_def, keepers_seen, n_off =
#{m > 0}, max_margin and max_col = the earliest column attaining it (NONE, -1 without an attacker).  A TOO_FEW row still holds n_att, n_def and
keepers_seen; everything else of a row that is not OK is 0 / -1 / NONE.

TOTALS per member, in group order 0, 1 and by column inside a group, over the OK rows on which it is present: rows, off_rows = #{m > 0}, max_margin
(NONE when rows == 0).

EVENTS: one record per event handed in, in their order.  NOT_PASS: kind != PASS.  NO_RECEIVER: to_col is no member of group 0 or 1.  NO_LINE: the
record of the receiver's group at release_row is not OK, or the receiver is absent there.  Else OK: group = the receiver's, margin = its margin at
release_row, line_qx and n_off that record's, verdict with tq = floor(tolerance * 1024 + 0.5): OFFSIDE when m > tq, else CLOSE when m > -tq, else
ONSIDE; bypassed = the members of d present at release_row and at receive_row with u(release) > u_ball(release) and u(receive) <= u_ball(receive), -1
when the ball is absent at either row.  A record that is not OK: verdict 0, margin NONE, line_qx 0, n_off 0, bypassed -1, group = the receiver's for
NO_LINE and -1 otherwise.  A pass event whose rows or receiver column lie outside the table is refused.

TWO DEFINITIONS: offside() is vectorised over the rows in int64; offside_scalar() is a plain loop over rows and columns in Python integers."""
import math

import numpy as np

import minimap_ref as R_
from shape_ref import MAX_MEMBERS, members, quantise

DIR_AUTO, DIR_RIGHT, DIR_LEFT = 0, 1, 2
OK, NO_DIRECTION, TOO_FEW = 0, 1, 2
KEEPER_ASSUMED, BY_DEFENDER, BY_BALL, BY_HALF, NO_BALL = 1, 2, 4, 8, 16
EV_OK, EV_NOT_PASS, EV_NO_RECEIVER, EV_NO_LINE = 0, 1, 2, 3
ONSIDE, CLOSE, OFFSIDE = 1, 2, 3
NONE = -2 ** 31
U_MAX, U_HALF = 107520, 53760
EVENT_PASS = 0
ROW_DTYPE = np.dtype([("status", "<i4"), ("flags", "<i4"), ("line_qx", "<i4"), ("second_col", "<i4"), ("n_att", "<i4"), ("n_def", "<i4"), ("keepers_seen", "<i4"),
                      ("n_off", "<i4"), ("max_margin", "<i4"), ("max_col", "<i4"), ("reserved", "<i4", 2)])                                              # EagleOffsideRow, 48 bytes
TOTALS_DTYPE = np.dtype([("col", "<i4"), ("group", "<i4"), ("rows", "<i4"), ("off_rows", "<i4"), ("max_margin", "<i4"), ("reserved", "<i4", 3)])          # EagleOffsideTotals, 32 bytes
EVENT_DTYPE = np.dtype([("status", "<i4"), ("verdict", "<i4"), ("margin", "<i4"), ("line_qx", "<i4"), ("n_off", "<i4"), ("bypassed", "<i4"), ("group", "<i4"),
                        ("reserved", "<i4")])                                                                                                            # EagleOffsideEvent, 32 bytes
CLIP_DTYPE = np.dtype([("direction", "<i4"), ("requested", "<i4"), ("neg", "<i4"), ("pos", "<i4"), ("zero", "<i4"), ("n_members", "<i4", 2), ("n_keepers", "<i4")])   # EagleOffsideClip, 32 bytes
assert (ROW_DTYPE.itemsize, TOTALS_DTYPE.itemsize, EVENT_DTYPE.itemsize, CLIP_DTYPE.itemsize) == (48, 32, 32, 32)
_LOW = -2 ** 40                                                          # below every depth and margin


def offside_params(direction=DIR_AUTO, assume_keeper=1, tolerance=0.5):
    return {"direction": int(direction), "assume_keeper": int(assume_keeper), "tolerance": float(tolerance)}


def check_params(p):
    if p["direction"] not in (DIR_AUTO, DIR_RIGHT, DIR_LEFT):
        raise ValueError("direction %r is none of AUTO, RIGHT, LEFT" % (p["direction"],))
    if not (math.isfinite(p["tolerance"]) and 0.0 <= p["tolerance"] <= 1024.0):
        raise ValueError("tolerance %r outside [0, 1024]" % (p["tolerance"],))


def tolerance_q(p):
    return int(math.floor(p["tolerance"] * 1024.0 + 0.5))


def first_entries(mapping):
    """a dict, or (id, value) pairs of which the first for an id counts -> dict (None stays None)"""
    if mapping is None or isinstance(mapping, dict):
        return mapping
    out = {}
    for ident, v in mapping:
        out.setdefault(int(ident), int(v))
    return out


def columns_of(columns, mapping, no_ball=False):
    """-> ([columns of group 0], [of group 1], [keepers], the ball's column or -1), table order each"""
    g0, g1 = members(columns, first_entries(mapping))
    keepers = [c for c, (kind, _, video) in enumerate(columns) if kind == R_.GOALKEEPER and not video]
    balls = [c for c, (kind, _, video) in enumerate(columns) if kind == R_.BALL and not video]
    if len(balls) > 1:
        raise ValueError("columns %d and %d are both the ball" % (balls[0], balls[1]))
    if len(g0) + len(g1) + len(keepers) > MAX_MEMBERS:
        raise ValueError("more than %d members and keepers" % MAX_MEMBERS)
    return g0, g1, keepers, -1 if no_ball or not balls else balls[0]


def check_events(events, rows, ncols):
    for k, e in enumerate(() if events is None else events):
        if int(e["kind"]) == EVENT_PASS and not (0 <= int(e["release_row"]) < rows and 0 <= int(e["receive_row"]) < rows and 0 <= int(e["to_col"]) < ncols):
            raise ValueError("pass event %d lies outside the table" % k)


def attacks_right(direction, a):
    return (direction == DIR_RIGHT) == (a == 0)


def resolve(requested, neg, pos):
    if requested != DIR_AUTO:
        return requested
    return DIR_RIGHT if neg > pos else DIR_LEFT if pos > neg else 0


def verdict_of(m, tq):
    return OFFSIDE if m > tq else CLOSE if m > -tq else ONSIDE


def _outputs(rows, g0, g1, keepers, p, n_events):
    rec = np.zeros((rows, 2), ROW_DTYPE)
    rec["status"], rec["second_col"], rec["max_col"], rec["max_margin"] = NO_DIRECTION, -1, -1, NONE
    margins = np.full((len(g0) + len(g1), rows), NONE, np.int32)
    totals = np.zeros(len(g0) + len(g1), TOTALS_DTYPE)
    totals["col"], totals["group"], totals["max_margin"] = g0 + g1, [0] * len(g0) + [1] * len(g1), NONE
    clip = np.zeros(1, CLIP_DTYPE)
    clip["requested"], clip["n_members"], clip["n_keepers"] = p["direction"], [len(g0), len(g1)], len(keepers)
    ev = np.zeros(n_events, EVENT_DTYPE)
    ev["margin"], ev["bypassed"], ev["group"] = NONE, -1, -1
    return rec, margins, totals, clip, ev


def _totals(margins, totals):
    """the totals from the margins: Python integers, member by member"""
    for t, row in zip(totals, margins):
        ms = [int(v) for v in row if int(v) != NONE]
        if ms:
            t["rows"], t["off_rows"], t["max_margin"] = len(ms), sum(m > 0 for m in ms), max(ms)


# ---- definition one: vectorised over the rows, int64 --------------------------------------------------------------------------------------
def offside(values, columns, mapping, p, events=None, no_ball=False):
    """values float64 [cols][rows][2]; events: possession_ref.EVENT_DTYPE or None -> (ROW_DTYPE [rows, 2], margins int32 [members, rows], TOTALS_DTYPE
    [members], CLIP_DTYPE [1], EVENT_DTYPE [events])"""
    check_params(p)
    g0, g1, keepers, ball = columns_of(columns, mapping, no_ball)
    rows = values.shape[1]
    check_events(events, rows, len(columns))
    rec, margins, totals, clip, evo = _outputs(rows, g0, g1, keepers, p, 0 if events is None else len(events))
    listed = sorted(g0 + g1 + keepers)
    grp = np.array([0 if c in g0 else 1 if c in g1 else 2 for c in listed], np.int64)
    col = np.array(listed + [-1], np.int64)                              # (the last entry: the column of "nobody")
    member = {c: k for k, c in enumerate(g0 + g1)}
    qx, _, ok = quantise(values[listed, :, 0], values[listed, :, 1])     # [listed, rows]
    n = [ok[grp == g].sum(0) for g in (0, 1)]
    sx = [np.where(ok[grp == g], qx[grp == g], 0).sum(0) for g in (0, 1)]
    v = np.where((n[0] > 0) & (n[1] > 0), np.sign(sx[0] * n[1] - sx[1] * n[0]), 2)
    clip["neg"], clip["pos"], clip["zero"] = (v == -1).sum(), (v == 1).sum(), (v == 0).sum()
    direction = resolve(p["direction"], int(clip[0]["neg"]), int(clip[0]["pos"]))
    clip["direction"] = direction
    if ball >= 0:
        bq, _, bok = quantise(values[ball, :, 0], values[ball, :, 1])
    else:
        bq, bok = np.zeros(rows, np.int64), np.zeros(rows, bool)
    low = np.full((1, rows), _LOW, np.int64)
    for a in (0, 1) if direction else ():
        right = attacks_right(direction, a)
        u = qx if right else U_MAX - qx
        seen = ok & (grp == 2)[:, None] & (u > U_HALF)
        isdef = (ok & (grp == 1 - a)[:, None]) | seen
        isatt = ok & (grp == a)[:, None]
        K, ns = isdef.sum(0), seen.sum(0)
        top = -np.sort(-np.concatenate([np.where(isdef, u, _LOW), low, low]), axis=0)[:2]
        assumed = (ns == 0) & (p["assume_keeper"] != 0)
        second = np.where(assumed, top[0], top[1])
        good = K >= np.where(assumed, 1, 2)
        at = np.concatenate([isdef & (u == second[None]), np.ones((1, rows), bool)])
        second_col = col[np.argmax(at, 0)]                               # (the first of them in table order)
        ub = bq if right else U_MAX - bq
        line, by = second.copy(), np.full(rows, BY_DEFENDER)
        m = bok & (ub > line)
        line, by = np.where(m, ub, line), np.where(m, BY_BALL, by)
        m = U_HALF > line
        line, by = np.where(m, U_HALF, line), np.where(m, BY_HALF, by)
        o = rec[:, a]
        o["status"] = np.where(good, OK, TOO_FEW)
        o["n_att"], o["n_def"], o["keepers_seen"] = isatt.sum(0), K, ns
        o["flags"] = np.where(good, by | np.where(assumed, KEEPER_ASSUMED, 0) | np.where(bok, 0, NO_BALL), 0)
        o["line_qx"] = np.where(good, line if right else U_MAX - line, 0)
        o["second_col"] = np.where(good, second_col, -1)
        has = isatt & good[None]
        mg = np.concatenate([np.where(has, u - line[None], _LOW), low])
        best = mg.max(0)
        o["n_off"] = (has & (mg[:-1] > 0)).sum(0)
        o["max_margin"] = np.where(best > _LOW, best, NONE)
        o["max_col"] = np.where(best > _LOW, col[np.argmax(mg == best[None], 0)], -1)
        for k, c in enumerate(listed):
            if grp[k] == a:
                margins[member[c]] = np.where(has[k], mg[k], NONE)
    _totals(margins, totals)
    for k, e in enumerate(() if events is None else events):
        o = evo[k]
        c, r0, r1 = int(e["to_col"]), int(e["release_row"]), int(e["receive_row"])
        if int(e["kind"]) != EVENT_PASS:
            o["status"] = EV_NOT_PASS
        elif c not in member:
            o["status"] = EV_NO_RECEIVER
        else:
            a = int(totals[member[c]]["group"])
            o["group"] = a
            m = int(margins[member[c], r0])
            if rec[r0, a]["status"] != OK or m == NONE:
                o["status"] = EV_NO_LINE
                continue
            o["status"], o["margin"], o["line_qx"], o["n_off"], o["verdict"] = EV_OK, m, rec[r0, a]["line_qx"], rec[r0, a]["n_off"], verdict_of(m, tolerance_q(p))
            if bok[r0] and bok[r1]:
                right = attacks_right(direction, a)
                u = qx if right else U_MAX - qx
                ub = bq if right else U_MAX - bq
                opp = grp == 1 - a
                o["bypassed"] = (opp & ok[:, r0] & ok[:, r1] & (u[:, r0] > ub[r0]) & (u[:, r1] <= ub[r1])).sum()
    return rec, margins, totals, clip, evo


# ---- definition two: a plain loop over rows and columns, Python integers ------------------------------------------------------------------
def _qx(cell):
    """the contract's quantisation of one cell -> qx as a Python integer, or None when absent"""
    x, y = float(cell[0]), float(cell[1])
    if not (math.isfinite(x) and math.isfinite(y)) or abs(x) > 1024.0 or abs(y) > 1024.0:
        return None
    return math.floor(x * 1024.0 + 0.5)


def offside_scalar(values, columns, mapping, p, events=None, no_ball=False):
    check_params(p)
    g0, g1, keepers, ball = columns_of(columns, mapping, no_ball)
    rows = values.shape[1]
    check_events(events, rows, len(columns))
    rec, margins, totals, clip, evo = _outputs(rows, g0, g1, keepers, p, 0 if events is None else len(events))
    groups = (g0, g1)
    member = {c: k for k, c in enumerate(g0 + g1)}
    neg = pos = zero = 0
    for r in range(rows):
        xs = [[q for q in (_qx(values[c, r]) for c in g) if q is not None] for g in groups]
        if xs[0] and xs[1]:
            v = sum(xs[0]) * len(xs[1]) - sum(xs[1]) * len(xs[0])
            neg, pos, zero = neg + (v < 0), pos + (v > 0), zero + (v == 0)
    direction = resolve(p["direction"], neg, pos)
    clip[0]["neg"], clip[0]["pos"], clip[0]["zero"], clip[0]["direction"] = neg, pos, zero, direction
    depth = lambda q, right: q if right else U_MAX - q
    for r in range(rows) if direction else ():
        for a in (0, 1):
            right = attacks_right(direction, a)
            o = rec[r, a]
            defenders, seen = [], 0
            for c in groups[1 - a]:
                q = _qx(values[c, r])
                if q is not None:
                    defenders.append((depth(q, right), c))
            for c in keepers:
                q = _qx(values[c, r])
                if q is not None and depth(q, right) > U_HALF:
                    defenders.append((depth(q, right), c))
                    seen += 1
            attackers = [(depth(q, right), c) for q, c in ((_qx(values[c, r]), c) for c in groups[a]) if q is not None]
            o["n_att"], o["n_def"], o["keepers_seen"] = len(attackers), len(defenders), seen
            assumed = seen == 0 and p["assume_keeper"] != 0
            if len(defenders) < (1 if assumed else 2):
                o["status"] = TOO_FEW
                continue
            depths = sorted((u for u, _ in defenders), reverse=True)
            second = depths[0] if assumed else depths[1]
            q = _qx(values[ball, r]) if ball >= 0 else None
            line, by = second, BY_DEFENDER
            if q is not None and depth(q, right) > line:
                line, by = depth(q, right), BY_BALL
            if U_HALF > line:
                line, by = U_HALF, BY_HALF
            o["status"], o["flags"] = OK, by | (KEEPER_ASSUMED if assumed else 0) | (NO_BALL if q is None else 0)
            o["line_qx"] = line if right else U_MAX - line
            o["second_col"] = min(c for u, c in defenders if u == second)
            for u, c in attackers:
                margins[member[c], r] = u - line
            o["n_off"] = sum(u - line > 0 for u, _ in attackers)
            if attackers:
                best = max(u for u, _ in attackers)
                o["max_margin"], o["max_col"] = best - line, min(c for u, c in attackers if u == best)
    _totals(margins, totals)
    tq = tolerance_q(p)
    for k, e in enumerate(() if events is None else events):
        o = evo[k]
        c, r0, r1 = int(e["to_col"]), int(e["release_row"]), int(e["receive_row"])
        if int(e["kind"]) != EVENT_PASS:
            o["status"] = EV_NOT_PASS
            continue
        if c not in member:
            o["status"] = EV_NO_RECEIVER
            continue
        a = 0 if c in g0 else 1
        o["group"] = a
        if rec[r0, a]["status"] != OK or _qx(values[c, r0]) is None:
            o["status"] = EV_NO_LINE
            continue
        right = attacks_right(direction, a)
        line = depth(int(rec[r0, a]["line_qx"]), right)
        m = depth(_qx(values[c, r0]), right) - line
        o["status"], o["margin"], o["line_qx"], o["verdict"] = EV_OK, m, rec[r0, a]["line_qx"], verdict_of(m, tq)
        o["n_off"] = sum(1 for t in groups[a] if _qx(values[t, r0]) is not None and depth(_qx(values[t, r0]), right) > line)
        b0, b1 = (_qx(values[ball, r]) if ball >= 0 else None for r in (r0, r1))
        if b0 is not None and b1 is not None:
            n = 0
            for t in groups[1 - a]:
                q0, q1 = _qx(values[t, r0]), _qx(values[t, r1])
                if q0 is not None and q1 is not None and depth(q0, right) > depth(b0, right) and depth(q1, right) <= depth(b1, right):
                    n += 1
            o["bypassed"] = n
    return rec, margins, totals, clip, evo
