"""The written definition of the physical report (include/eagle.h, eagle_post_physical / eagle_op_physical; csrc/physical.hip): speed zones, efforts
(high-speed runs, sprints, accelerations, decelerations) and totals per person.  An own specification, the reference derives none of this.  Everything is
float64, one operation at a time (numpy never contracts), sqrt and division correctly rounded; every total is a Python integer or a maximum, so no order
of accumulation can show.  The contract is held TWICE: physical() is the scan formulation the kernels follow (run starts as inclusive max-scans of row
indices), state_machine() an independent plain loop over the rows of each column carrying the open run of every kind; tests/test_physical_cpu.py holds
them against each other bit for bit.

Inputs: velocities [cols][rows][2] (eagle_post_velocities' layout: NaN where the cell is absent), frames [rows] strictly ascending, columns (kind, id,
video) in table order, fps, max_gap, zone_edges[4], effort_speed[2], accel, min_frames[2].  Outputs: a dict with persons (the Player and Goalkeeper pitch
columns in table order), speed, accel (float64 [persons][rows]), zone (uint8 [persons][rows]), totals (TOTALS_DTYPE [persons]), efforts (EFFORT_DTYPE, in
ascending (person, kind, first_row)) and the intermediate rows of the scan formulation (pres, link, q, zs, hot, head, tail, start) for the tests that
assert an edge was forced."""
import math

import numpy as np

PLAYER, GOALKEEPER, BALL, BOUNDARY = 0, 1, 2, 3
HSR, SPRINT, ACCEL, DECEL = 0, 1, 2, 3
KIND_NAMES = ("high_speed_run", "sprint", "acceleration", "deceleration")
ZONE_EDGES, EFFORT_SPEED, ACCEL_EDGE = (2.0, 4.0, 5.5, 7.0), (5.5, 7.0), 2.0      # conventional choices (max_gap: fps, min_frames: fps // 2), not fitted to data
Q = 1 << 20                            # distances are quantised to 1 / Q metres per step
D_CLAMP = 1048576.0                    # metres: a step's distance is clamped to this before it is quantised
ABSENT_ZONE = 255
TOTALS_DTYPE = np.dtype([("zone_frames", "<i8", 5), ("zone_dist_q", "<i8", 5), ("top_speed", "<f8"), ("col", "<i4"), ("rows_present", "<i4"),
                         ("efforts", "<i4", 4), ("reserved", "<i4", 4)])                                           # EagleLoadTotals (128 bytes)
EFFORT_DTYPE = np.dtype([("col", "<i4"), ("kind", "<i4"), ("first_row", "<i4"), ("last_row", "<i4"), ("frames", "<i4"), ("reserved0", "<i4"),
                         ("distance_q", "<i8"), ("peak_speed", "<f8"), ("peak_accel", "<f8")])                     # EagleLoadEffort (48 bytes)


def default_min_frames(fps):
    return max(1, int(fps) // 2)


def check(fps, max_gap, zone_edges, effort_speed, accel, min_frames):
    e = [float(x) for x in zone_edges]
    ok = int(fps) > 0 and int(max_gap) > 0 and len(e) == 4 and len(min_frames) == 2 and all(int(m) > 0 for m in min_frames)
    ok = ok and all(math.isfinite(x) and x > 0.0 for x in e) and all(e[k] < e[k + 1] for k in range(3))
    ok = ok and len(effort_speed) == 2 and all(math.isfinite(float(x)) and float(x) > 0.0 for x in tuple(effort_speed) + (accel,))
    if not ok:
        raise ValueError("physical: fps, max_gap, min_frames positive; edges finite, positive, strictly ascending; effort_speed and accel finite and positive")


def layout(columns):
    """-> the person columns in table order"""
    persons = []
    for c, (kind, cid, video) in enumerate(columns):
        if kind not in (PLAYER, GOALKEEPER, BALL, BOUNDARY):
            raise ValueError("physical: unknown column kind")
        if not video and kind in (PLAYER, GOALKEEPER):
            persons.append(c)
    return persons


def _max_scan(flag):
    """per row the greatest index r' <= r with flag[r'], or -1"""
    idx = np.where(flag, np.arange(len(flag), dtype=np.int64), -1)
    return np.maximum.accumulate(idx) if len(idx) else idx


def _args(velocities, frames, fps, max_gap, zone_edges, effort_speed, accel, min_frames):
    max_gap = int(fps if max_gap is None else max_gap)
    min_frames = (default_min_frames(fps),) * 2 if min_frames is None else tuple(int(m) for m in min_frames)
    check(fps, max_gap, zone_edges, effort_speed, accel, min_frames)
    velocities = np.asarray(velocities, np.float64)
    frames = np.asarray(frames, np.int64)
    assert velocities.ndim == 3 and velocities.shape[2] == 2 and len(frames) == velocities.shape[1] and (np.diff(frames) > 0).all()
    return velocities, frames, max_gap, min_frames


def column_rows(v, frames, fps, max_gap, zone_edges, effort_speed, accel):
    """the per-row and per-step quantities of one column: v [rows][2]"""
    rows = len(frames)
    fpsd = np.float64(int(fps))
    edges = [np.float64(x) for x in zone_edges]
    with np.errstate(over="ignore", invalid="ignore"):
        pres = np.isfinite(v[:, 0]) & np.isfinite(v[:, 1])
        s = np.where(pres, np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]), np.nan)
        link = np.zeros(rows, bool)
        if rows > 1:
            link[1:] = pres[1:] & pres[:-1] & (np.diff(frames) <= max_gap)
        # the speed differenced by the velocity kernel's neighbour rule
        lo_ok = link.copy()
        hi_ok = np.zeros(rows, bool)
        hi_ok[:-1] = link[1:]
        idx = np.arange(rows)
        lo, hi = np.where(lo_ok, idx - 1, idx), np.where(hi_ok, idx + 1, idx)
        a = np.zeros(rows, np.float64)
        if rows:
            span = frames[hi] - frames[lo]
            use = span != 0
            dt = span[use].astype(np.float64) / fpsd
            a[use] = (s[hi][use] - s[lo][use]) / dt
        a = np.where(pres, a, np.nan)
        zone = np.where(pres, sum((s >= e).astype(np.int64) for e in edges), ABSENT_ZONE).astype(np.uint8)
        # steps
        q, zs = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
        if rows > 1:
            st = np.flatnonzero(link)
            df = (frames[st] - frames[st - 1]).astype(np.float64)
            m = np.float64(0.5) * (s[st - 1] + s[st])
            d = m * (df / fpsd)
            d = np.where(d > D_CLAMP, D_CLAMP, d)
            q[st] = np.floor(d * np.float64(Q) + np.float64(0.5)).astype(np.int64)
            zs[st] = sum((m >= e).astype(np.int64) for e in edges)
        hot = np.stack([pres & (s >= np.float64(effort_speed[0])), pres & (s >= np.float64(effort_speed[1])), pres & (a >= np.float64(accel)),
                        pres & (a <= -np.float64(accel))])
    return pres, s, link, a, zone, q, zs, hot


def physical(velocities, frames, columns, fps, max_gap=None, zone_edges=ZONE_EDGES, effort_speed=EFFORT_SPEED, accel=ACCEL_EDGE, min_frames=None):
    """the scan formulation"""
    velocities, frames, max_gap, min_frames = _args(velocities, frames, fps, max_gap, zone_edges, effort_speed, accel, min_frames)
    persons = layout(columns)
    rows, P = len(frames), len(persons)
    out = {"persons": persons, "speed": np.full((P, rows), np.nan), "accel": np.full((P, rows), np.nan), "zone": np.full((P, rows), ABSENT_ZONE, np.uint8),
           "totals": np.zeros(P, TOTALS_DTYPE), "pres": np.zeros((P, rows), bool), "link": np.zeros((P, rows), bool), "q": np.zeros((P, rows), np.int64),
           "zs": np.zeros((P, rows), np.int64), "hot": np.zeros((P, 4, rows), bool), "head": np.zeros((P, 4, rows), bool), "tail": np.zeros((P, 4, rows), bool),
           "start": np.full((P, 4, rows), -1, np.int64)}
    efforts = []
    for i, c in enumerate(persons):
        pres, s, link, a, zone, q, zs, hot = column_rows(velocities[c], frames, fps, max_gap, zone_edges, effort_speed, accel)
        out["speed"][i], out["accel"][i], out["zone"][i], out["pres"][i], out["link"][i], out["q"][i], out["zs"][i], out["hot"][i] = s, a, zone, pres, link, q, zs, hot
        t = out["totals"][i]
        t["col"], t["rows_present"] = c, int(pres.sum())
        t["top_speed"] = s[pres].max() if pres.any() else 0.0
        df = np.zeros(rows, np.int64)
        if rows > 1:
            df[1:] = np.diff(frames)
        for z in range(5):
            sel = link & (zs == z)
            t["zone_frames"][z] = sum(int(x) for x in df[sel])
            t["zone_dist_q"][z] = sum(int(x) for x in q[sel])
        for k in range(4):
            h = hot[k]
            head, tail = h.copy(), h.copy()
            if rows > 1:
                head[1:] = h[1:] & (~link[1:] | ~h[:-1])
                tail[:-1] = h[:-1] & (~link[1:] | ~h[1:])
            start = _max_scan(head)
            out["head"][i, k], out["tail"][i, k], out["start"][i, k] = head, tail, start
            n = 0
            for r in np.flatnonzero(tail):
                r, f0 = int(r), int(start[r])
                if int(frames[r]) - int(frames[f0]) < min_frames[0 if k < 2 else 1]:
                    continue
                peak_s, peak_a = 0.0, 0.0
                for j in range(f0, r + 1):                          # "greater than the peak so far": a NaN (inf - inf) never is
                    if s[j] > peak_s:
                        peak_s = s[j]
                    if abs(a[j]) > peak_a:
                        peak_a = abs(a[j])
                efforts.append((c, k, f0, r, int(frames[r]) - int(frames[f0]), 0, sum(int(x) for x in q[f0 + 1:r + 1]), peak_s, peak_a))
                n += 1
            t["efforts"][k] = n
    out["efforts"] = np.array(efforts, EFFORT_DTYPE) if efforts else np.zeros(0, EFFORT_DTYPE)
    return out


def state_machine(velocities, frames, columns, fps, max_gap=None, zone_edges=ZONE_EDGES, effort_speed=EFFORT_SPEED, accel=ACCEL_EDGE, min_frames=None):
    """The same outputs (speed, accel, zone, totals, efforts) by a plain loop over the rows of each column: python floats and ints, math.sqrt, no arrays of
    flags and no scans.  Per kind it carries the open run (its first row, distance, peaks) and closes it where the next row does not continue it."""
    velocities, frames, max_gap, min_frames = _args(velocities, frames, fps, max_gap, zone_edges, effort_speed, accel, min_frames)
    persons = layout(columns)
    rows, P = len(frames), len(persons)
    fin = math.isfinite
    edges = [float(x) for x in zone_edges]
    f = [int(x) for x in frames]
    fpsd = float(int(fps))

    def speed_of(c, r):
        vx, vy = float(velocities[c, r, 0]), float(velocities[c, r, 1])
        if not (fin(vx) and fin(vy)):
            return None
        try:
            return math.sqrt(vx * vx + vy * vy)
        except OverflowError:
            return math.inf

    def sub(x, y):
        return math.nan if (x == math.inf and y == math.inf) else x - y

    speed, acc, zone = np.full((P, rows), np.nan), np.full((P, rows), np.nan), np.full((P, rows), ABSENT_ZONE, np.uint8)
    totals = np.zeros(P, TOTALS_DTYPE)
    efforts = []
    for i, c in enumerate(persons):
        sp = [speed_of(c, r) for r in range(rows)]
        zf, zd, n_pres, top = [0] * 5, [0] * 5, 0, 0.0
        found = [[] for _ in range(4)]
        run = [None] * 4                                            # per kind: [first_row, distance_q, peak_speed, peak_accel]
        for r in range(rows):
            if sp[r] is None:
                for k in range(4):
                    run[k] = None                                   # (closed at the row before, below)
                continue
            n_pres += 1
            top = max(top, sp[r])
            back = r >= 1 and sp[r - 1] is not None and f[r] - f[r - 1] <= max_gap
            fwd = r + 1 < rows and sp[r + 1] is not None and f[r + 1] - f[r] <= max_gap
            lo, hi = (r - 1 if back else r), (r + 1 if fwd else r)
            a = 0.0 if lo == hi else sub(sp[hi], sp[lo]) / (float(f[hi] - f[lo]) / fpsd)
            speed[i, r], acc[i, r], zone[i, r] = sp[r], a, sum(sp[r] >= e for e in edges)
            q = 0
            if back:
                m = 0.5 * (sp[r - 1] + sp[r])
                d = m * (float(f[r] - f[r - 1]) / fpsd)
                q = int(math.floor(min(d, D_CLAMP) * float(Q) + 0.5))
                z = sum(m >= e for e in edges)
                zf[z] += f[r] - f[r - 1]
                zd[z] += q
            hot = (sp[r] >= float(effort_speed[0]), sp[r] >= float(effort_speed[1]), a >= float(accel), a <= -float(accel))
            for k in range(4):
                if not hot[k]:
                    run[k] = None
                    continue
                if run[k] is None or not back:
                    run[k] = [r, 0, 0.0, 0.0]
                else:
                    run[k][1] += q
                if sp[r] > run[k][2]:
                    run[k][2] = sp[r]
                if abs(a) > run[k][3]:
                    run[k][3] = abs(a)
                # does the next row continue the run?  It does when it is linked to this one and hot itself; its heat needs its own acceleration, so look
                # ahead by the same rule instead of carrying the run open
                if fwd and _hot_next(sp, f, r + 1, rows, max_gap, fpsd, k, effort_speed, accel, sub):
                    continue
                if f[r] - f[run[k][0]] >= min_frames[0 if k < 2 else 1]:
                    found[k].append((c, k, run[k][0], r, f[r] - f[run[k][0]], 0, run[k][1], run[k][2], run[k][3]))
                run[k] = None
        t = totals[i]
        t["col"], t["rows_present"], t["top_speed"] = c, n_pres, top
        t["zone_frames"], t["zone_dist_q"] = zf, zd
        for k in range(4):
            t["efforts"][k] = len(found[k])
            efforts += found[k]
    return {"persons": persons, "speed": speed, "accel": acc, "zone": zone, "totals": totals,
            "efforts": np.array(efforts, EFFORT_DTYPE) if efforts else np.zeros(0, EFFORT_DTYPE)}


def _hot_next(sp, f, r, rows, max_gap, fpsd, k, effort_speed, accel, sub):
    """hot_k of row r (present, and linked to r - 1) for the state machine's look-ahead"""
    if k < 2:
        return sp[r] >= float(effort_speed[k])
    fwd = r + 1 < rows and sp[r + 1] is not None and f[r + 1] - f[r] <= max_gap
    lo, hi = r - 1, (r + 1 if fwd else r)
    a = sub(sp[hi], sp[lo]) / (float(f[hi] - f[lo]) / fpsd)
    return a >= float(accel) if k == 2 else a <= -float(accel)


def aggregates(res, columns, fps):
    """what eagle_amd/physical.py derives from totals and efforts: per person {"id", "type", "distance", "zone_distance", "zone_seconds", "top_speed",
    "rows", efforts per kind}; metres are q / 2^20 and seconds frames / fps, each one correctly rounded division of integers"""
    out = []
    for t in res["totals"]:
        kind, cid, _ = columns[int(t["col"])]
        zq = [int(x) for x in t["zone_dist_q"]]
        out.append({"id": int(cid), "type": "Player" if kind == PLAYER else "Goalkeeper", "distance": sum(zq) / Q, "zone_distance": [x / Q for x in zq],
                    "zone_seconds": [int(x) / int(fps) for x in t["zone_frames"]], "top_speed": float(t["top_speed"]), "rows": int(t["rows_present"]),
                    **{KIND_NAMES[k] + "s": int(t["efforts"][k]) for k in range(4)}})
    return out
