"""The ball-flight contract (include/eagle.h, eagle_post_ball_flights / eagle_op_ball_flights; csrc/flights.hip), restated on the host.

Between two touches a ball moves in a straight line at nearly constant speed on the pitch plane; a touch is where the line breaks.  The ball's one
pitch column is cut into such lines (flights) by a segmented least-squares fit, solved exactly by a dynamic program over the kept rows.

  present     x and y finite and |x|, |y| <= 1024;  q = rint(x * 1024) (ties to even), an integer from here on
  run         row r starts one when r == 0, the ball is absent at r or r - 1, f[r] - f[r-1] > max_gap, or f[r] is a cut
  spike       interior row r of a run (p = r - 1 and n = r + 1 in the run): D = f[n] - f[p], A = max over the axes of
              |(q[r] - q[p]) D - (q[n] - q[p]) (f[r] - f[p])|; A = 0 and D = 1 at a run's first and last row.  Spike when A[r] > T D[r] (T =
              rint(spike * 1024)), A[r] D[r-1] > A[r-1] D[r] and A[r] D[r+1] >= A[r+1] D[r].  used = present and not spike.
  c(i, j)     used rows i < j of one run, j - i <= L: over the used rows r' of [i, j], t = f[r'] - f[i], d = q[r'] - q[i]; integer S0, S1, S2 and per
              axis B0, B1, Q; det = S0 S2 - S1 S1; a0 = (S2 B0 - S1 B1) / det, a1 = (S0 B1 - S1 B0) / det, sse = max(0, Q - (a0 B0 + a1 B1));
              c = rint(min(sse_x + sse_y, 2^40))
  lam         rint(penalty * ((noise * 1024) * (noise * 1024))), at most 2^40
  best        best[first] = 0, best[j] = min over used i < j, j - i <= L of best[i] + c(i, j) + lam, ties to the smaller i; the path from the run's
              last row gives the segments; a knot is a row two consecutive segments share

Everything that is an integer or a decision is written twice: `flights()` forms the sums of every start row incrementally, as the kernels do, and walks
the dynamic program forwards; `second()` quantises and finds runs and spikes with numpy, forms the sums of a pair from the listed samples, and solves
the dynamic program by memoised recursion from the end.  tests/test_flights_cpu.py holds the two against each other.  The float solve is written once
(`line_cost`), in float64, one operation at a time; `line_cost_exact` is the same system in fractions.Fraction."""
import math
from fractions import Fraction

import numpy as np

PLAYER, GOALKEEPER, BALL, BOUNDARY = 0, 1, 2, 3
LIMIT = 1024.0
Q = 1024.0
C_CAP = float(1 << 40)
MAX_ROWS = 1 << 20
NAN = float("nan")
STILL, CARRIED, FREE = 0, 1, 2
F_PRESENT, F_USED, F_SPIKE, F_KNOT, F_KICK = 1, 2, 4, 8, 16
FL_CAPPED, FL_CONTINUES = 1, 2
GOAL_X, GOAL_Y, GOAL_HALF = 105.0, 34.0, 3.66

FLIGHT_DTYPE = np.dtype([("row0", "<i4"), ("row1", "<i4"), ("used", "<i4"), ("spikes", "<i4"), ("near", "<i4"), ("kind", "<i4"), ("shot", "<i4"), ("flags", "<i4"),
                         ("x0", "<f8"), ("y0", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("vx", "<f8"), ("vy", "<f8"), ("speed", "<f8"), ("rms", "<f8"),
                         ("y_cross", "<f8"), ("c", "<i8")])                                                       # EagleBallFlight (112 bytes)
KICK_DTYPE = np.dtype([("row", "<i4"), ("seg_in", "<i4"), ("seg_out", "<i4"), ("col", "<i4"), ("speed_in", "<f8"), ("speed_out", "<f8"), ("dv", "<f8"),
                       ("cos_turn", "<f8")])                                                                      # EagleBallKick (48 bytes)
TOTALS_DTYPE = np.dtype([("runs", "<i4"), ("flights", "<i4"), ("kinds", "<i4", 3), ("spikes", "<i4"), ("knots", "<i4"), ("kicks", "<i4"), ("shots", "<i4", 3),
                         ("capped", "<i4"), ("sum_c", "<i8"), ("reserved", "<i8")])                                # EagleFlightTotals (64 bytes)
assert FLIGHT_DTYPE.itemsize == 112 and KICK_DTYPE.itemsize == 48 and TOTALS_DTYPE.itemsize == 64

DEFAULTS = dict(max_rows=64, noise=0.25, penalty=16.0, spike=1.0, kick_dv=3.0, radius=2.0, still_speed=0.5, shot_speed=10.0, shot_range=40.0, shot_margin=2.0)


def params(fps, max_gap, **kw):
    """the resolved parameters as a dict; ValueError for what the library refuses with EAGLE_E_INVALID"""
    p = dict(DEFAULTS, fps=float(fps), max_gap=int(max_gap))
    for k, v in kw.items():
        if k not in DEFAULTS:
            raise TypeError(f"unknown parameter {k}")
        p[k] = int(v) if k == "max_rows" else float(v)
    fin = lambda v: v == v and abs(v) != float("inf")
    if not (fin(p["fps"]) and p["fps"] > 0):
        raise ValueError(f"fps {p['fps']} must be finite and positive")
    if not 1 <= p["max_gap"] <= 1024:
        raise ValueError(f"max_gap {p['max_gap']} is outside 1 .. 1024")
    if not 2 <= p["max_rows"] <= 128:
        raise ValueError(f"max_rows {p['max_rows']} is outside 2 .. 128")
    for k in ("noise", "spike"):
        if not (fin(p[k]) and 0 <= p[k] <= 1024):
            raise ValueError(f"{k} {p[k]} must be finite and within [0, 1024] m")
    for k in ("penalty", "kick_dv", "still_speed", "shot_speed", "shot_range", "shot_margin"):
        if not (fin(p[k]) and p[k] >= 0):
            raise ValueError(f"{k} {p[k]} must be finite and not negative")
    if not (p["radius"] > 0 and p["radius"] <= 1024):
        raise ValueError(f"radius {p['radius']} must be positive and at most 1024 m")
    if lam_of(p) is None:
        raise ValueError("penalty * (noise * 1024)^2 exceeds 2^40")
    return p


def lam_of(p):
    nq = p["noise"] * Q
    lam = p["penalty"] * (nq * nq)
    return int(round(lam)) if lam <= C_CAP else None


def layout(columns, no_ball=False):
    """-> (ball column or -1, person columns in table order)"""
    ball, persons = -1, []
    for c, (kind, _, video) in enumerate(columns):
        if kind not in (PLAYER, GOALKEEPER, BALL, BOUNDARY):
            raise ValueError("flights: unknown column kind")
        if video:
            continue
        if kind == BALL:
            if ball >= 0:
                raise ValueError("flights: more than one ball column")
            ball = c
        elif kind in (PLAYER, GOALKEEPER):
            persons.append(c)
    return (-1 if no_ball else ball), persons


def check_rows(frames, cuts):
    frames = [int(v) for v in frames]
    if len(frames) > MAX_ROWS:
        raise ValueError("flights: too many rows")
    if any(b <= a for a, b in zip(frames, frames[1:])):
        raise ValueError("flights: frame numbers must ascend")
    cuts = [] if cuts is None else [int(v) for v in cuts]
    if any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError("flights: cuts must ascend")
    return frames, cuts


def _present(x, y):
    return abs(x) <= LIMIT and abs(y) <= LIMIT          # False for NaN and +-inf


def candidate(values, persons, bcol, r, r2):
    """possession's candidate at row r (the ball cell present): the nearest finite person cell, the earlier column on a tie, when within the radius"""
    bx, by = float(values[bcol][r][0]), float(values[bcol][r][1])
    best, bc = 0.0, -1
    for c in persons:
        px, py = float(values[c][r][0]), float(values[c][r][1])
        if not (math.isfinite(px) and math.isfinite(py)):
            continue
        dx, dy = px - bx, py - by
        d2 = dx * dx + dy * dy
        if bc < 0 or d2 < best:
            best, bc = d2, c
    return bc if bc >= 0 and best <= r2 else -1


def line_cost(S0, S1, S2, B0x, B1x, Qx, B0y, B1y, Qy):
    """-> (c, a0x, a1x, a0y, a1y): float64, every operation in the stated order"""
    det = float(S0 * S2 - S1 * S1)
    out = []
    cost = None
    for B0, B1, QQ in ((B0x, B1x, Qx), (B0y, B1y, Qy)):
        a0 = (float(S2) * float(B0) - float(S1) * float(B1)) / det
        a1 = (float(S0) * float(B1) - float(S1) * float(B0)) / det
        sse = max(0.0, float(QQ) - (a0 * float(B0) + a1 * float(B1)))
        out += [a0, a1]
        cost = sse if cost is None else cost + sse
    return int(round(min(cost, C_CAP))), out[0], out[1], out[2], out[3]


def line_cost_exact(S0, S1, S2, B0x, B1x, Qx, B0y, B1y, Qy):
    """the cost before rounding, exactly (a Fraction)"""
    det = Fraction(S0 * S2 - S1 * S1)
    cost = Fraction(0)
    for B0, B1, QQ in ((B0x, B1x, Qx), (B0y, B1y, Qy)):
        a0 = Fraction(S2 * B0 - S1 * B1) / det
        a1 = Fraction(S0 * B1 - S1 * B0) / det
        cost += max(Fraction(0), QQ - (a0 * B0 + a1 * B1))
    return min(cost, Fraction(1 << 40))


def pair_sums(q, f, used, i, j):
    """the nine sums of segment [i, j] from its listed samples"""
    rows = [r for r in range(i, j + 1) if used[r]]
    t = [f[r] - f[i] for r in rows]
    dx = [q[r][0] - q[i][0] for r in rows]
    dy = [q[r][1] - q[i][1] for r in rows]
    return (len(rows), sum(t), sum(v * v for v in t), sum(dx), sum(a * b for a, b in zip(t, dx)), sum(v * v for v in dx),
            sum(dy), sum(a * b for a, b in zip(t, dy)), sum(v * v for v in dy))


def prepare(values, frames, columns, p, cuts, no_ball):
    """-> dict: ball, persons, q, present, head, A, D, spike, used (lists)"""
    rows = len(frames)
    ball, persons = layout(columns, no_ball)
    cutset = set(cuts)
    q = [(0, 0)] * rows
    present = [False] * rows
    for r in range(rows if ball >= 0 else 0):
        x, y = float(values[ball][r][0]), float(values[ball][r][1])
        if _present(x, y):
            present[r] = True
            q[r] = (int(round(x * Q)), int(round(y * Q)))
    head = [r == 0 or not present[r] or not present[r - 1] or frames[r] - frames[r - 1] > p["max_gap"] or frames[r] in cutset for r in range(rows)]
    A, D = [0] * rows, [1] * rows
    for r in range(1, rows - 1):
        if present[r] and not head[r] and not head[r + 1]:
            D[r] = frames[r + 1] - frames[r - 1]
            tr = frames[r] - frames[r - 1]
            A[r] = max(abs((q[r][k] - q[r - 1][k]) * D[r] - (q[r + 1][k] - q[r - 1][k]) * tr) for k in (0, 1))
    T = int(round(p["spike"] * Q))
    spike = [False] * rows
    for r in range(1, rows - 1):
        if A[r] > T * D[r] and A[r] * D[r - 1] > A[r - 1] * D[r] and A[r] * D[r + 1] >= A[r + 1] * D[r]:
            spike[r] = True
    used = [present[r] and not spike[r] for r in range(rows)]
    return dict(ball=ball, persons=persons, q=q, present=present, head=head, A=A, D=D, spike=spike, used=used)


def run_list(present, head):
    """the runs with at least two present rows as (first, last); and the number of runs with a present row"""
    rows, runs, n = len(present), [], 0
    r = 0
    while r < rows:
        if not present[r]:
            r += 1
            continue
        e = r
        while e + 1 < rows and not head[e + 1]:
            e += 1
        n += 1
        if e > r:
            runs.append((r, e))
        r = e + 1
    return runs, n


def costs_from(q, f, used, i, last, L):
    """c(i, j) and the fit for every used j in (i, min(i + L, last)], the sums formed incrementally -> {j: (c, a0x, a1x, a0y, a1y)}"""
    S0, S1, S2, B0x, B1x, Qx, B0y, B1y, Qy = 1, 0, 0, 0, 0, 0, 0, 0, 0
    out = {}
    for j in range(i + 1, min(i + L, last) + 1):
        if not used[j]:
            continue
        t, dx, dy = f[j] - f[i], q[j][0] - q[i][0], q[j][1] - q[i][1]
        S0 += 1; S1 += t; S2 += t * t
        B0x += dx; B1x += t * dx; Qx += dx * dx
        B0y += dy; B1y += t * dy; Qy += dy * dy
        out[j] = line_cost(S0, S1, S2, B0x, B1x, Qx, B0y, B1y, Qy)
    return out


def dp_run(q, f, used, first, last, L, lam):
    """-> (best {row: value}, pred {row: row}, cost {(i, j): tuple}) of one run, forwards"""
    cost = {}
    for i in range(first, last):
        if used[i]:
            for j, v in costs_from(q, f, used, i, last, L).items():
                cost[(i, j)] = v
    best, pred = {first: 0}, {}
    for j in range(first + 1, last + 1):
        if not used[j]:
            continue
        for i in range(max(first, j - L), j):                   # ascending i and a strict comparison: a tie keeps the smaller i
            if used[i]:
                v = best[i] + cost[(i, j)][0] + lam
                if j not in best or v < best[j]:
                    best[j], pred[j] = v, i
    return best, pred, cost


def flights(values, frames, columns, p, cuts=None, no_ball=False):
    """The whole contract -> dict(seg int32 [rows], flags uint8 [rows], fitted, velocity float64 [rows][2], flights FLIGHT_DTYPE, kicks KICK_DTYPE,
    totals TOTALS_DTYPE [1]) and, for the tests, "best" (the value at each run's last row) and "prep"."""
    values = np.asarray(values, np.float64)
    frames, cuts = check_rows(frames, cuts)
    rows, f = len(frames), frames
    prep = prepare(values, frames, columns, p, cuts, no_ball)
    q, present, head, spike, used, ball, persons = (prep[k] for k in ("q", "present", "head", "spike", "used", "ball", "persons"))
    L, lam, fps = p["max_rows"], lam_of(p), p["fps"]
    r2 = p["radius"] * p["radius"]
    seg = np.full(rows, -1, np.int32)
    flags = np.zeros(rows, np.uint8)
    fitted, velocity = np.full((rows, 2), np.nan), np.full((rows, 2), np.nan)
    fl, kk = [], []
    tot = np.zeros(1, TOTALS_DTYPE)
    for r in range(rows):
        flags[r] = (F_PRESENT if present[r] else 0) | (F_USED if used[r] else 0) | (F_SPIKE if spike[r] else 0)
    runs, nruns = run_list(present, head)
    tot["runs"] = nruns
    tot["spikes"] = sum(spike)
    best_end = []
    for first, last in runs:
        best, pred, cost = dp_run(q, f, used, first, last, L, lam)
        best_end.append(best[last])
        path = [last]
        while path[-1] != first:
            path.append(pred[path[-1]])
        path.reverse()
        run_first_seg = len(fl)
        for i, j in zip(path, path[1:]):
            c, a0x, a1x, a0y, a1y = cost[(i, j)]
            k = len(fl)
            rec = np.zeros(1, FLIGHT_DTYPE)[0]
            urows = [r for r in range(i, j + 1) if used[r]]
            cands = {r: candidate(values, persons, ball, r, r2) for r in urows}
            t1 = float(f[j] - f[i])
            fit = lambda a0, a1, q0, t: ((float(q0) + a0) + a1 * t) / Q
            vx, vy = (a1x * fps) / Q, (a1y * fps) / Q
            speed = math.sqrt(vx * vx + vy * vy)
            near = sum(1 for r in urows if cands[r] >= 0)
            kind = STILL if speed < p["still_speed"] else CARRIED if 2 * near > len(urows) else FREE
            x0, y0 = fit(a0x, a1x, q[i][0], 0.0), fit(a0y, a1y, q[i][1], 0.0)
            shot, y_cross = 0, NAN
            if kind == FREE and speed >= p["shot_speed"] and vx != 0.0:
                X = GOAL_X if vx > 0.0 else 0.0
                s = (X - x0) / vx
                y_cross = y0 + vy * s
                reach = speed * s
                if 0.0 <= reach <= p["shot_range"]:
                    off = abs(y_cross - GOAL_Y)
                    shot = 2 if off <= GOAL_HALF else 1 if off <= GOAL_HALF + p["shot_margin"] else 0
                tot["shots"][0, shot] += 1
            rec["row0"], rec["row1"], rec["used"], rec["spikes"], rec["near"], rec["kind"], rec["shot"] = i, j, len(urows), (j - i + 1) - len(urows), near, kind, shot
            rec["flags"] = FL_CAPPED if j - i == L else 0
            rec["x0"], rec["y0"], rec["x1"], rec["y1"] = x0, y0, fit(a0x, a1x, q[i][0], t1), fit(a0y, a1y, q[i][1], t1)
            rec["vx"], rec["vy"], rec["speed"], rec["y_cross"], rec["c"] = vx, vy, speed, y_cross, c
            rec["rms"] = math.sqrt(float(c) / float(len(urows))) / Q
            fl.append(rec)
            tot["kinds"][0, kind] += 1
            tot["capped"] += 1 if j - i == L else 0
            tot["sum_c"] += c
            for r in range(i, j + 1):
                if r == j and j != last:
                    continue                                    # a knot row belongs to the segment that starts there
                seg[r] = k
                tr = float(f[r] - f[i])
                fitted[r] = (fit(a0x, a1x, q[i][0], tr), fit(a0y, a1y, q[i][1], tr))
                velocity[r] = (vx, vy)
        for k in range(run_first_seg + 1, len(fl)):             # the knots of the run
            a, b = fl[k - 1], fl[k]
            r = int(b["row0"])
            dvx, dvy = float(b["vx"]) - float(a["vx"]), float(b["vy"]) - float(a["vy"])
            dv = math.sqrt(dvx * dvx + dvy * dvy)
            flags[r] |= F_KNOT
            tot["knots"] += 1
            if dv >= p["kick_dv"]:
                flags[r] |= F_KICK
                e = np.zeros(1, KICK_DTYPE)[0]
                e["row"], e["seg_in"], e["seg_out"], e["col"] = r, k - 1, k, candidate(values, persons, ball, r, r2)
                si, so = float(a["speed"]), float(b["speed"])
                e["speed_in"], e["speed_out"], e["dv"] = si, so, dv
                e["cos_turn"] = NAN if si == 0.0 or so == 0.0 else (float(a["vx"]) * float(b["vx"]) + float(a["vy"]) * float(b["vy"])) / (si * so)
                kk.append(e)
            else:
                a["flags"] |= FL_CONTINUES
    tot["flights"], tot["kicks"] = len(fl), len(kk)
    return dict(seg=seg, flags=flags, fitted=fitted, velocity=velocity, flights=np.array(fl, FLIGHT_DTYPE), kicks=np.array(kk, KICK_DTYPE), totals=tot,
                best=best_end, prep=prep, runs=runs)


def second(values, frames, columns, p, cuts=None, no_ball=False):
    """The integers and decisions once more, another way -> dict(q int64 [rows][2], present, head, spike bool [rows], runs, best [per run], knots
    [per run: the path], cost {(i, j): c})."""
    values = np.asarray(values, np.float64)
    frames, cuts = check_rows(frames, cuts)
    rows = len(frames)
    ball, _ = layout(columns, no_ball)
    f = np.asarray(frames, np.int64)
    if ball >= 0 and rows:
        cell = values[ball]
        with np.errstate(invalid="ignore"):
            present = np.isfinite(cell).all(1) & (np.abs(cell) <= LIMIT).all(1)
        q = np.where(present[:, None], np.rint(np.where(present[:, None], cell, 0.0) * Q), 0.0).astype(np.int64)
    else:
        present, q = np.zeros(rows, bool), np.zeros((rows, 2), np.int64)
    head = np.ones(rows, bool)
    if rows > 1:
        head[1:] = ~present[1:] | ~present[:-1] | (np.diff(f) > p["max_gap"]) | np.isin(f[1:], np.asarray(cuts, np.int64))
    A, D = np.zeros(rows, np.int64), np.ones(rows, np.int64)
    if rows > 2:
        inner = present[1:-1] & ~head[1:-1] & ~head[2:]
        Dm = f[2:] - f[:-2]
        dev = np.abs((q[1:-1] - q[:-2]) * Dm[:, None] - (q[2:] - q[:-2]) * (f[1:-1] - f[:-2])[:, None]).max(1)
        A[1:-1] = np.where(inner, dev, 0)
        D[1:-1] = np.where(inner, Dm, 1)
    T = int(round(p["spike"] * Q))
    spike = np.zeros(rows, bool)
    if rows > 2:
        spike[1:-1] = (A[1:-1] > T * D[1:-1]) & (A[1:-1] * D[:-2] > A[:-2] * D[1:-1]) & (A[1:-1] * D[2:] >= A[2:] * D[1:-1])
    used = present & ~spike
    L, lam = p["max_rows"], lam_of(p)
    ql, fl, ul = [tuple(int(v) for v in row) for row in q], [int(v) for v in f], [bool(v) for v in used]
    starts = [r for r in range(rows) if present[r] and head[r] and r + 1 < rows and not head[r + 1]]
    runs, bests, paths, cost = [], [], [], {}
    for first in starts:
        last = first
        while last + 1 < rows and not head[last + 1]:
            last += 1
        runs.append((first, last))
        urows = [r for r in range(first, last + 1) if ul[r]]
        memo = {first: (0, None)}
        for j in urows[1:]:                                     # (ascending, so the recursion of a long run is never deep)
            opts = []
            for i in urows:
                if i < j and j - i <= L:
                    c = line_cost(*pair_sums(ql, fl, ul, i, j))[0]
                    cost[(i, j)] = c
                    opts.append((memo[i][0] + c + lam, i))
            memo[j] = min(opts)                                 # the least value, then the smaller i
        path = [last]
        while memo[path[-1]][1] is not None:
            path.append(memo[path[-1]][1])
        bests.append(memo[last][0])
        paths.append(path[::-1])
    return dict(q=q, present=present, head=head, spike=spike, runs=runs, best=bests, knots=paths, cost=cost)


def brute_force(q, f, used, first, last, L, lam):
    """every admissible segmentation of a short run -> (least total, the path the tie rule selects).  The dynamic program prefers, at every end row from
    the last backwards, the smaller start among equal totals: among all least paths, the one whose reversed knot list is lexicographically least."""
    urows = [r for r in range(first, last + 1) if used[r]]
    inner = urows[1:-1]
    best = None
    for mask in range(1 << len(inner)):
        path = [first] + [r for k, r in enumerate(inner) if mask >> k & 1] + [last]
        if any(b - a > L for a, b in zip(path, path[1:])):
            continue
        total = sum(line_cost(*pair_sums(q, f, used, a, b))[0] + lam for a, b in zip(path, path[1:]))
        key = (total, path[::-1])
        if best is None or key < best:
            best = key
    return best[0], best[1][::-1]
