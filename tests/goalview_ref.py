"""numpy / Python-integer restatement of the goal-view stage (include/eagle.h, eagle_post_goal_view / eagle_op_goal_view; csrc/goalview.hip): per row,
attacking group and point (every member, the ball, optionally every cell of the pitch) the slices of the goal mouth that the other team hides and the
open angle.  It is the single written definition of every output bit: the kernels equal it bit for bit.  OWN SPEC.

ARITHMETIC: float64, one numpy operation at a time in the order written in the functions below (numpy contracts nothing), correctly rounded division
and sqrt; only + - * / sqrt, comparisons, floor and rint; copysign and where only move bits.  Sums are integers.

POSITIONS are offside_ref's: groups 0 and 1, the keepers, the ball (columns_of), present and quantised by shape_ref.quantise, q = floor(v * 1024 + 0.5);
metres are q / 1024, exact.

GOALS: x_g = 0 and x_g = 105, the mouth y = 30.34 .. 37.66 in 64 slices of DY = 7.32 / 64 with centres YC[k] = 30.34 + (k + 0.5) * DY.  direction
(offside_ref.DIR_RIGHT / DIR_LEFT, resolved by the caller) says which goal group 0 attacks: attacks_right.

BLOCKERS of the attacking group g on a row (row_blockers): the present members of 1 - g with rho = radius and every present keeper with depth
u > U_HALF (offside's "seen" keeper) with rho = keeper_radius, in table order.  More than BLOCKERS of them: the record has status TOO_MANY, every point
of g on the row has status PT_ROW.  n_blockers counts them all.

POINT (point_status): s = x_g - P.x; |s| < min_depth -> PT_NEAR_LINE; ex = x_g - P.x, ey = 34 - P.y, ex ex + ey ey > max_range max_range -> PT_FAR
(open 0); else PT_OK.  Absent: PT_ABSENT.  Every status but OK and FAR has open -1; every status but OK has mask 0 (and full 0).

SHADOW (shadow): see the function; slice k is blocked iff lo <= YC[k] <= hi.  ANGLE (weights): w_k = rint(2^24 ((DY |s|) / (s s + (YC[k] - P.y)^2))).

RECORDS [rows][2], MEMBERS (open, mask, status [members][rows]), TOTALS and GRID: include/eagle.h states them; goal_view() below is their definition."""
import math

import numpy as np

import offside_ref as O
from shape_ref import quantise

BLOCKERS, SLICES = 32, 64
Y0, DY, TWO24 = 30.34, 7.32 / 64.0, 16777216.0
OK, TOO_MANY = 0, 1
PT_OK, PT_ABSENT, PT_ROW, PT_NEAR_LINE, PT_FAR = 0, 1, 2, 3, 4
FORM_DEFAULT, FORM_DIRECT, FORM_TABLE = 0, 1, 2
YC = Y0 + (np.arange(SLICES, dtype=np.float64) + 0.5) * DY
ROW_DTYPE = np.dtype([("status", "<i4"), ("n_blockers", "<i4"), ("ball_status", "<i4"), ("ball_open", "<i4"), ("ball_full", "<i4"), ("best_col", "<i4"),
                      ("best_open", "<i4"), ("owner_col", "<i4"), ("owner_open", "<i4"), ("reserved", "<i4"), ("ball_mask", "<u8"), ("owner_mask", "<u8")])   # EagleGoalViewRow, 56 bytes
TOTALS_DTYPE = np.dtype([("col", "<i4"), ("group", "<i4"), ("rows", "<i4"), ("max_open", "<i4"), ("max_row", "<i4"), ("chance_rows", "<i4"), ("sum_open", "<i8")])   # EagleGoalViewTotals, 32 bytes
assert (ROW_DTYPE.itemsize, TOTALS_DTYPE.itemsize) == (56, 32)
_BIT = np.uint64(1) << np.arange(SLICES, dtype=np.uint64)


def goal_view_params(direction=O.DIR_RIGHT, group=0, cells_per_metre=1, form=FORM_DEFAULT, grid_row0=0, grid_rows=0, radius=0.4, keeper_radius=1.0, min_depth=1.0,
                     max_range=40.0, chance=0.3):
    return {"direction": int(direction), "group": int(group), "cells_per_metre": int(cells_per_metre), "form": int(form), "grid_row0": int(grid_row0),
            "grid_rows": int(grid_rows), "radius": float(radius), "keeper_radius": float(keeper_radius), "min_depth": float(min_depth), "max_range": float(max_range),
            "chance": float(chance)}


def check_params(p, rows, has_owner):
    for k in ("radius", "keeper_radius", "min_depth", "max_range", "chance"):
        if not math.isfinite(p[k]):
            raise ValueError("%s %r is not finite" % (k, p[k]))
    for k in ("radius", "keeper_radius"):
        if not 0.0 <= p[k] <= 16.0:
            raise ValueError("%s %r outside [0, 16]" % (k, p[k]))
    if p["min_depth"] < 1.0:
        raise ValueError("min_depth %r below 1" % (p["min_depth"],))
    if not p["min_depth"] < p["max_range"] <= 1024.0:
        raise ValueError("max_range %r must lie above min_depth and within 1024" % (p["max_range"],))
    if not 0.0 <= p["chance"] <= 4.0:
        raise ValueError("chance %r outside [0, 4]" % (p["chance"],))
    if p["cells_per_metre"] not in (1, 2, 4):
        raise ValueError("cells_per_metre %r is none of 1, 2, 4" % (p["cells_per_metre"],))
    if p["direction"] not in (O.DIR_RIGHT, O.DIR_LEFT):
        raise ValueError("direction %r is not resolved to RIGHT or LEFT" % (p["direction"],))
    if p["group"] not in (-1, 0, 1):
        raise ValueError("group %r is none of -1, 0, 1" % (p["group"],))
    if p["form"] not in (FORM_DEFAULT, FORM_DIRECT, FORM_TABLE):
        raise ValueError("form %r" % (p["form"],))
    if p["grid_rows"] < 0 or p["grid_row0"] < 0 or (p["grid_rows"] > 0 and p["grid_row0"] + p["grid_rows"] > rows):
        raise ValueError("the grid's rows lie outside the table")
    if p["grid_rows"] > 0 and p["group"] < 0 and not has_owner:
        raise ValueError("group -1 needs a possession result")


def point_status(px, py, xg, p):
    """float64 arrays of points -> (status int array, s)"""
    s = xg - px
    ey = 34.0 - py
    far = s * s + ey * ey > p["max_range"] * p["max_range"]
    return np.where(np.abs(s) < p["min_depth"], PT_NEAR_LINE, np.where(far, PT_FAR, PT_OK)), s


def _reach(py, s, tx, ty):
    good = np.where(s > 0.0, tx > 0.0, tx < 0.0)
    with np.errstate(all="ignore"):
        y = py + (ty * s) / np.where(good, tx, 1.0)
    return np.where(good, y, np.copysign(np.inf, ty))


def shadow(px, py, s, xg, bx, by, rho):
    """points (arrays) and one disc (scalars) -> bool [points][64]: the slices the disc hides"""
    wx, gx = bx - px, xg - bx
    counts = np.where(s > 0.0, (wx > 0.0) & (gx >= 0.0), (wx < 0.0) & (gx <= 0.0))
    wy = by - py
    d2 = wx * wx + wy * wy
    r2 = rho * rho
    inside = d2 <= r2
    l = np.sqrt(np.where(inside, 0.0, d2 - r2))
    lx, ly, rx, ry = l * wx, l * wy, rho * wx, rho * wy
    y1, y2 = _reach(py, s, lx - ry, ly + rx), _reach(py, s, lx + ry, ly - rx)
    lo, hi = np.where(y1 <= y2, y1, y2), np.where(y1 <= y2, y2, y1)
    blocked = (lo[:, None] <= YC[None]) & (YC[None] <= hi[:, None])
    return counts[:, None] & (inside[:, None] | blocked)


def weights(py, s):
    """-> int64 [points][64]"""
    e = YC[None] - py[:, None]
    return np.rint(TWO24 * ((DY * np.abs(s))[:, None] / ((s * s)[:, None] + e * e))).astype(np.int64)


def pack(bits):
    """bool [..., 64] -> uint64 [...]"""
    return np.bitwise_or.reduce(np.where(bits, _BIT, np.uint64(0)), axis=-1)


def evaluate(px, py, right, blockers, p):
    """points of an evaluated row -> (status, blocked bool [n][64], open, full int64); open is 0 for FAR and -1 for NEAR_LINE, full 0 unless OK"""
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    xg = 105.0 if right else 0.0
    st, s = point_status(px, py, xg, p)
    ok = st == PT_OK
    bits = np.zeros((len(px), SLICES), bool)
    opn, full = np.where(st == PT_FAR, 0, -1).astype(np.int64), np.zeros(len(px), np.int64)
    if ok.any():
        x, y, ss = px[ok], py[ok], s[ok]
        b = np.zeros((len(x), SLICES), bool)
        for bx, by, rho in blockers:
            b |= shadow(x, y, ss, xg, bx, by, rho)
        w = weights(y, ss)
        bits[ok], opn[ok], full[ok] = b, np.where(b, 0, w).sum(1), w.sum(1)
    return st, bits, opn, full


def row_blockers(values, r, g, right, g0, g1, keepers, p):
    """-> [(x, y, rho)] in table order, all of them"""
    out = []
    other = g1 if g == 0 else g0
    for c in sorted(other + keepers):
        qx, qy, ok = quantise(values[c, r, 0], values[c, r, 1])
        if not ok:
            continue
        if c in keepers and c not in other:
            if (int(qx) if right else O.U_MAX - int(qx)) <= O.U_HALF:
                continue
            out.append((int(qx) / 1024.0, int(qy) / 1024.0, p["keeper_radius"]))
        else:
            out.append((int(qx) / 1024.0, int(qy) / 1024.0, p["radius"]))
    return out


def cell_points(R):
    """-> px, py float64 [68 R * 105 R], row-major, row 0 at y = 0"""
    i, j = np.meshgrid(np.arange(105 * R, dtype=np.float64), np.arange(68 * R, dtype=np.float64))
    return ((i + 0.5) / float(R)).ravel(), ((j + 0.5) / float(R)).ravel()


def goal_view(values, columns, mapping, p, owner=None, no_ball=False):
    """values float64 [cols][rows][2]; owner int [rows] or None -> {"rows": ROW_DTYPE [rows, 2], "open": int32, "mask": uint64, "status": uint8
    [members, rows], "totals": TOTALS_DTYPE [members], "grid": uint8 [grid_rows, 68 R, 105 R]}"""
    rows = values.shape[1]
    check_params(p, rows, owner is not None)
    g0, g1, keepers, ball = O.columns_of(columns, mapping, no_ball)
    groups, mcols = (g0, g1), g0 + g1
    member = {c: k for k, c in enumerate(mcols)}
    nm = len(mcols)
    rec = np.zeros((rows, 2), ROW_DTYPE)
    opn, msk, sts = np.full((nm, rows), -1, np.int32), np.zeros((nm, rows), np.uint64), np.full((nm, rows), PT_ABSENT, np.uint8)
    R = p["cells_per_metre"]
    grid = np.zeros((p["grid_rows"], 68 * R, 105 * R), np.uint8)
    cx, cy = cell_points(R) if p["grid_rows"] else (None, None)
    for r in range(rows):
        for g in (0, 1):
            right = O.attacks_right(p["direction"], g)
            bl = row_blockers(values, r, g, right, g0, g1, keepers, p)
            many = len(bl) > BLOCKERS
            o = rec[r, g]
            o["status"], o["n_blockers"] = TOO_MANY if many else OK, len(bl)
            # the members of g and the ball
            pts = [(k, values[c, r]) for k, c in enumerate(mcols) if c in groups[g]] + ([(-1, values[ball, r])] if ball >= 0 else [])
            qx, qy, ok = quantise([v[0] for _, v in pts], [v[1] for _, v in pts]) if pts else (np.zeros(0),) * 3
            here = [n for n in range(len(pts)) if ok[n]]
            o["ball_status"], o["ball_open"], o["best_col"], o["best_open"], o["owner_col"], o["owner_open"] = PT_ABSENT, -1, -1, -1, -1, -1
            if here and many:
                for n in here:
                    if pts[n][0] >= 0:
                        sts[pts[n][0], r] = PT_ROW
                    else:
                        o["ball_status"] = PT_ROW
            elif here:
                st, bits, op, full = evaluate(qx[here] / 1024.0, qy[here] / 1024.0, right, bl, p)
                m64 = pack(bits)
                for n, s_, m_, o_, f_ in zip(here, st, m64, op, full):
                    k = pts[n][0]
                    if k >= 0:
                        sts[k, r], msk[k, r], opn[k, r] = s_, m_, o_
                        if s_ == PT_OK and int(o_) > int(o["best_open"]):        # members come in column order: a tie keeps the smaller column
                            o["best_open"], o["best_col"] = o_, mcols[k]
                    else:
                        o["ball_status"], o["ball_mask"], o["ball_open"], o["ball_full"] = s_, m_, o_, f_
            if owner is not None and int(owner[r]) in member and (0 if int(owner[r]) in g0 else 1) == g:
                k = member[int(owner[r])]
                o["owner_col"], o["owner_mask"], o["owner_open"] = int(owner[r]), msk[k, r], opn[k, r]
        if p["grid_row0"] <= r < p["grid_row0"] + p["grid_rows"]:
            g = p["group"]
            if g < 0:
                c = int(owner[r])
                g = -1 if c not in member else 0 if c in g0 else 1
            if g >= 0 and rec[r, g]["status"] == OK:
                right = O.attacks_right(p["direction"], g)
                st, _, op, _ = evaluate(cx, cy, right, row_blockers(values, r, g, right, g0, g1, keepers, p), p)
                grid[r - p["grid_row0"]] = np.where(st == PT_OK, np.minimum(255, op >> 16), 0).reshape(68 * R, 105 * R)
    totals = np.zeros(nm, TOTALS_DTYPE)
    totals["col"], totals["group"], totals["max_open"], totals["max_row"] = mcols, [0] * len(g0) + [1] * len(g1), -1, -1
    cq = int(np.rint(TWO24 * p["chance"]))
    for k in range(nm):
        vals = [(int(opn[k, r]), r) for r in range(rows) if sts[k, r] == PT_OK]
        if vals:
            best = max(v for v, _ in vals)
            t = totals[k]
            t["rows"], t["sum_open"], t["max_open"] = len(vals), sum(v for v, _ in vals), best
            t["max_row"], t["chance_rows"] = min(r for v, r in vals if v == best), sum(v >= cq for v, _ in vals)
    return {"rows": rec, "open": opn, "mask": msk, "status": sts, "totals": totals, "grid": grid}


# ---- the independent test of a shadow: the distance from the disc's centre to the ray from P through a slice centre -----------------------------
def brute_blocked(px, py, xg, bx, by, rho):
    """scalars -> (bool [64], distance - rho float64 [64]): slice k is hidden when the ray from P through (xg, YC[k]) passes within rho of the centre.
    A disc whose centre does not lie between the point and the line hides nothing."""
    s = xg - px
    sg = 1.0 if s > 0 else -1.0
    if not (sg * (bx - px) > 0 and sg * (xg - bx) >= 0):
        return np.zeros(SLICES, bool), np.full(SLICES, np.inf)
    ux, uy = np.full(SLICES, s), YC - py
    n = np.hypot(ux, uy)
    ux, uy = ux / n, uy / n
    wx, wy = bx - px, by - py
    t = wx * ux + wy * uy                                                 # along the ray; behind the point the nearest point of the ray is P itself
    dist = np.where(t > 0, np.abs(wx * uy - wy * ux), math.hypot(wx, wy))
    return dist <= rho, dist - rho
