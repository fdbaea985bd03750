"""The track-smoothing contract (include/eagle.h, eagle_post_smooth_tracks / eagle_op_smooth_tracks; csrc/smooth.hip), restated on the host.

Everything that is an integer or a decision is written twice: `smooth(..., form="window")` walks, for every row, the rows within W rows of it, as the
kernels do (frame numbers ascend strictly, so a frame distance of at most W is a row distance of at most W); `smooth(..., form="plain")` asks every row
of the column, collects the window's samples in lists and forms the sums from those, takes the median by sorting (value, row) pairs, and counts the
totals and suspect rows with loops of its own.  tests/test_smooth_cpu.py holds the two against each other bit for bit.  The float solve is written once
(`solve`), in float64, one operation at a time in the order include/eagle.h states; `solve_exact` is the same system in fractions.Fraction.

The rule, per smoothed column (Player and Goalkeeper pitch columns with half-width `window`, the Ball pitch column with `ball_window` when that is > 0):
  present     x and y finite and |x|, |y| <= 1024;  q = rint(x * 1024) (ties to even), an integer from here on
  window of r the used rows r' of the column with |f[r'] - f[r]| <= W,  t = f[r'] - f[r]
  sums        S_k = sum t^k (k = 0 .. 4), per axis B_k = sum t^k q (k = 0 .. 2): integers
  degree      n >= 4: `degree`; n == 3: min(degree, 1); n == 2: 1; n == 1: 0; n == 0: the cell keeps its raw value
  pass 1      used = present; e[r] = max(|q_x - a0_x|, |q_y - a0_y|)
  pass 2      med[r] = the element of rank (n - 1) // 2 of the window's e; outlier: outlier_k > 0 and e[r] > max(outlier_floor * 1024, outlier_k * med[r])
  pass 3      used = present and not outlier; position a0 / 1024, velocity (a1 * fps) / 1024 scaled back to speed_cap, acceleration ((2 a2) * fps) * fps / 1024
Every other column keeps its bytes, gets post_velocity_kernel's velocity (tests/control_ref.py) and NaN acceleration."""
from fractions import Fraction

import numpy as np

import control_ref as CR

PLAYER, GOALKEEPER, BALL, BOUNDARY = 0, 1, 2, 3
LIMIT = 1024.0
Q = 1024.0
RES_CAP = 16777216.0            # 2^24: the largest residual_q
TOTALS_DTYPE = np.dtype([("sum_sq", "<i8"), ("present", "<i4"), ("outliers", "<i4"), ("low_degree", "<i4"), ("max_residual_q", "<i4"), ("window", "<i4"),
                         ("reserved", "<i4")])
F_FITTED, F_OUTLIER, F_DEG_SHIFT, F_RAW = 1, 2, 2, 16
NAN = float("nan")


def default_window(fps):
    return max(2, int(round(0.4 * fps)))


def check(fps, window, degree, outlier_k, outlier_floor, ball_window, max_gap, speed_cap):
    """ValueError for what the library refuses with EAGLE_E_INVALID"""
    fin = lambda v: v == v and abs(v) != float("inf")
    if fps <= 0 or max_gap <= 0 or not (fin(speed_cap) and speed_cap > 0):
        raise ValueError(f"fps {fps}, max_gap {max_gap} and speed_cap {speed_cap} must be positive (and finite)")
    if not 1 <= window <= 64:
        raise ValueError(f"window {window} is outside 1 .. 64")
    if degree not in (1, 2):
        raise ValueError(f"degree {degree} is neither 1 nor 2")
    if not 0 <= ball_window <= 64:
        raise ValueError(f"ball_window {ball_window} is outside 0 .. 64")
    if not (fin(outlier_k) and outlier_k >= 0):
        raise ValueError(f"outlier_k {outlier_k} must be 0 or finite and positive")
    if not (fin(outlier_floor) and outlier_floor >= 0):
        raise ValueError(f"outlier_floor {outlier_floor} must be finite and not negative")


def column_windows(columns, window, ball_window):
    """half-width per column; 0: the column is not smoothed"""
    out = []
    for kind, _, video in columns:
        w = 0
        if not video and kind in (PLAYER, GOALKEEPER):
            w = window
        elif not video and kind == BALL:
            w = ball_window
        out.append(int(w))
    return out


def quantise(col):
    """[rows][2] float64 -> (present [rows] bools, q [rows] pairs of Python ints)"""
    present, q = [], []
    for x, y in col:
        ok = bool(np.isfinite(x) and np.isfinite(y) and abs(x) <= LIMIT and abs(y) <= LIMIT)
        present.append(ok)
        q.append((int(round(float(x) * Q)), int(round(float(y) * Q))) if ok else (0, 0))
    return present, q


def degree_used(n, degree):
    if n >= 4:
        return degree
    if n == 3:
        return min(degree, 1)
    return (0, 0, 1)[n]


def solve(S, B, deg):
    """(a0, a1, a2) of one axis: Cramer's rule in float64 on the integer sums converted to double, every product and sum single and in this order"""
    S0, S1, S2, S3, S4 = (float(v) for v in S)
    B0, B1, B2 = (float(v) for v in B)
    if deg == 2:
        C00 = S2 * S4 - S3 * S3
        C01 = S2 * S3 - S1 * S4
        C02 = S1 * S3 - S2 * S2
        C11 = S0 * S4 - S2 * S2
        C12 = S1 * S2 - S0 * S3
        C22 = S0 * S2 - S1 * S1
        det = (S0 * C00 + S1 * C01) + S2 * C02
        return (((C00 * B0 + C01 * B1) + C02 * B2) / det, ((C01 * B0 + C11 * B1) + C12 * B2) / det, ((C02 * B0 + C12 * B1) + C22 * B2) / det)
    if deg == 1:
        det = S0 * S2 - S1 * S1
        return ((S2 * B0 - S1 * B1) / det, (S0 * B1 - S1 * B0) / det, 0.0)
    return (B0 / S0, 0.0, 0.0)


def solve_exact(S, B, deg):
    """the least-squares coefficients as exact fractions (Gaussian elimination on the normal equations)"""
    m = deg + 1
    A = [[Fraction(S[i + j]) for j in range(m)] + [Fraction(B[i])] for i in range(m)]
    for i in range(m):
        p = next(r for r in range(i, m) if A[r][i] != 0)
        A[i], A[p] = A[p], A[i]
        A[i] = [v / A[i][i] for v in A[i]]
        for r in range(m):
            if r != i:
                A[r] = [a - A[r][i] * b for a, b in zip(A[r], A[i])]
    return [A[i][m] for i in range(m)] + [Fraction(0)] * (3 - m)


def _window_rows(f, used, r, W, form):
    rows = len(f)
    rng = range(max(0, r - W), min(rows, r + W + 1)) if form == "window" else range(rows)
    return [j for j in rng if used[j] and abs(f[j] - f[r]) <= W]


def _sums(f, q, r, win, form):
    if form == "window":
        S, Bx, By = [0] * 5, [0] * 3, [0] * 3
        for j in win:
            t = f[j] - f[r]
            p = 1
            for k in range(5):
                S[k] += p
                if k < 3:
                    Bx[k] += p * q[j][0]
                    By[k] += p * q[j][1]
                p *= t
        return S, Bx, By
    ts = [f[j] - f[r] for j in win]
    return ([sum(t ** k for t in ts) for k in range(5)], [sum(t ** k * q[j][0] for t, j in zip(ts, win)) for k in range(3)],
            [sum(t ** k * q[j][1] for t, j in zip(ts, win)) for k in range(3)])


def _median(e, win, form):
    rank = (len(win) - 1) // 2
    if form == "plain":
        return sorted((e[j], j) for j in win)[rank][0]
    for i in win:                                                                   # the kernel's selection: the value v with #{< v} <= rank < #{<= v}
        less, leq = sum(1 for j in win if e[j] < e[i]), sum(1 for j in win if e[j] <= e[i])
        if less <= rank < leq:
            return e[i]
    raise AssertionError("no element of the rank")


def _fit(f, q, used, r, W, degree, form):
    win = _window_rows(f, used, r, W, form)
    n = len(win)
    if n == 0:
        return None
    S, Bx, By = _sums(f, q, r, win, form)
    assert S[0] == n
    deg = degree_used(n, degree)
    return {"n": n, "deg": deg, "S": S, "Bx": Bx, "By": By, "ax": solve(S, Bx, deg), "ay": solve(S, By, deg), "win": win}


def _resid(q, fit):
    return max(abs(float(q[0]) - fit["ax"][0]), abs(float(q[1]) - fit["ay"][0]))


def cap_speed(vx, vy, cap):
    s = float(np.sqrt(np.float64(vx * vx + vy * vy)))
    if s > cap:
        k = cap / s
        vx, vy = vx * k, vy * k
    return vx, vy


def smooth(values, frames, columns, fps, window=None, degree=2, outlier_k=4.0, outlier_floor=0.25, ball_window=0, max_gap=None, speed_cap=CR.SPEED_CAP, form="window"):
    """values float64 [cols][rows][2], frames [rows] strictly ascending, columns (kind, id, video) -> dict: values, vel, acc float64 [cols][rows][2]; flags,
    count uint8 and residual_q int32 [cols][rows]; suspect uint8 [rows]; totals TOTALS_DTYPE [cols]; and the intermediates (q, present, e, med, outlier, fit1,
    fit3, colw) by column index."""
    values = np.ascontiguousarray(values, np.float64)
    cols, rows = values.shape[:2]
    f = [int(v) for v in frames]
    W = default_window(fps) if window is None else int(window)
    max_gap = fps if max_gap is None else max_gap
    check(fps, W, degree, outlier_k, outlier_floor, ball_window, max_gap, speed_cap)
    assert all(b > a for a, b in zip(f, f[1:])), "frame numbers must ascend"
    colw = column_windows(columns, W, int(ball_window))
    fpsd, thr_floor = float(fps), float(outlier_floor) * Q
    out_v = values.copy()
    vel = np.full((cols, rows, 2), np.nan)
    rest = [c for c in range(cols) if colw[c] == 0]
    if rest and rows:
        vel[rest] = CR.velocities(values[rest], np.asarray(f, np.int64), fps, max_gap, speed_cap)
    acc = np.full((cols, rows, 2), np.nan)
    flags, count, resid = np.zeros((cols, rows), np.uint8), np.zeros((cols, rows), np.uint8), np.zeros((cols, rows), np.int32)
    totals = np.zeros(cols, TOTALS_DTYPE)
    inter = {"q": {}, "present": {}, "e": {}, "med": {}, "outlier": {}, "fit1": {}, "fit3": {}, "colw": colw}
    for c in range(cols):
        Wc = colw[c]
        if Wc == 0:
            continue
        present, q = quantise(values[c])
        fit1 = [(_fit(f, q, present, r, Wc, degree, form) if present[r] else None) for r in range(rows)]
        e = [(_resid(q[r], fit1[r]) if present[r] else -1.0) for r in range(rows)]
        med, outl = [None] * rows, [False] * rows
        for r in range(rows):
            if present[r]:
                med[r] = _median(e, fit1[r]["win"], form)
                outl[r] = bool(outlier_k > 0 and e[r] > max(thr_floor, float(outlier_k) * med[r]))
        used = [present[r] and not outl[r] for r in range(rows)]
        fit3 = [None] * rows
        for r in range(rows):
            out_v[c, r] = vel[c, r] = acc[c, r] = (NAN, NAN)
            if not present[r]:
                continue
            ft = fit3[r] = _fit(f, q, used, r, Wc, degree, form)
            if ft is None:                                                          # every sample of the window was rejected: the raw value stays
                out_v[c, r] = values[c, r]
                vel[c, r] = acc[c, r] = (0.0, 0.0)
                flags[c, r] = F_RAW | (F_OUTLIER if outl[r] else 0)
                continue
            out_v[c, r] = (ft["ax"][0] / Q, ft["ay"][0] / Q)
            vel[c, r] = cap_speed((ft["ax"][1] * fpsd) / Q, (ft["ay"][1] * fpsd) / Q, float(speed_cap))
            acc[c, r] = ((((2.0 * ft["ax"][2]) * fpsd) * fpsd) / Q, (((2.0 * ft["ay"][2]) * fpsd) * fpsd) / Q)
            flags[c, r] = F_FITTED | (F_OUTLIER if outl[r] else 0) | (ft["deg"] << F_DEG_SHIFT)
            count[c, r] = ft["n"]
            resid[c, r] = int(round(min(16.0 * _resid(q[r], ft), RES_CAP)))
        inter["q"][c], inter["present"][c], inter["e"][c], inter["med"][c], inter["outlier"][c], inter["fit1"][c], inter["fit3"][c] = q, present, e, med, outl, fit1, fit3
        # per column
        if form == "window":
            pres = np.array(present, bool)
            dg = (flags[c] >> F_DEG_SHIFT) & 3
            rq = resid[c].astype(np.int64)
            totals[c] = (int((rq * rq).sum()), int(pres.sum()), int(np.array(outl, bool).sum()), int((pres & (dg < degree)).sum()), int(rq.max()) if rows else 0, Wc, 0)
        else:
            ssq = npres = nout = nlow = mx = 0
            for r in range(rows):
                if present[r]:
                    npres += 1
                    nout += outl[r]
                    nlow += (0 if fit3[r] is None else fit3[r]["deg"]) < degree
                    ssq += int(resid[c, r]) ** 2
                    mx = max(mx, int(resid[c, r]))
            totals[c] = (ssq, npres, nout, nlow, mx, Wc, 0)
    # per row: the smoothed person cells
    suspect = np.zeros(rows, np.uint8)
    persons = [c for c, (kind, _, video) in enumerate(columns) if colw[c] and kind in (PLAYER, GOALKEEPER)]
    if form == "window" and persons and rows:
        pres = np.array([inter["present"][c] for c in persons], bool).sum(0)
        outs = np.array([inter["outlier"][c] for c in persons], bool).sum(0)
        suspect = ((pres >= 4) & (2 * outs >= pres)).astype(np.uint8)
    else:
        for r in range(rows):
            pres = sum(1 for c in persons if inter["present"][c][r])
            outs = sum(1 for c in persons if inter["outlier"][c][r])
            suspect[r] = 1 if pres >= 4 and outs * 2 >= pres else 0
    return {"values": out_v, "vel": vel, "acc": acc, "flags": flags, "count": count, "residual_q": resid, "suspect": suspect, "totals": totals, **inter}
