"""The stabilisation contract (include/eagle.h, eagle_post_stabilise / eagle_op_stabilise; csrc/stab.hip), restated on the host.

Everything that is an integer or a decision is written twice: `stabilise(..., form="window")` works as the kernels do (a row's window is walked over the
rows within W rows of it with running sums, a row's voters are compacted in column order, a median is found by rank counting, the sums run over the
voters one by one); `stabilise(..., form="plain")` asks every row of the column, forms the sums from lists, takes a median by sorting and counts the
totals with loops of its own.  tests/test_stab_cpu.py holds the two against each other bit for bit.  The float solves are written once (`SR.solve` for the
prediction, `affine_solve` for the map), in float64, one operation at a time in the order include/eagle.h states; `affine_exact` is the same system in
fractions.Fraction.

The rule.  Voter columns: Player and Goalkeeper pitch columns (video == 0); moved columns: the voters and the Ball pitch column; every other column
keeps its bytes.  A cell of a moved column is present when x and y are finite and |x|, |y| <= 1024; q = rint(x * 1024) once; C starts as q.
Per round (`iterations` of them), from C of the round before for the neighbours and from q for the row itself:
  predict   per present voter cell (c, r): the window is the present rows r' != r of the column with |f[r'] - f[r]| <= W; it needs a row before r, a row
            after r and n >= 2.  K37's sums S_k, B_k over C[r'] with t = f[r'] - f[r], K37's degree rule and solve; the cell votes when both |a0| <= 2^40
            and, with p = llrint(a0), d = q - p has |d| <= 2^24 on both axes (a detail the issue leaves open: a vote has to fit its int32).
  estimate  per row: the first 64 voters in column order (more: flag OVER_CAP); fewer than min_voters: no estimate.  b = per-axis lower median of d,
            dev_i = max(|d_x - b_x|, |d_y - b_y|), m = lower median of dev; inlier: trim_k == 0 or (double)dev_i <= max(floor * 1024, trim_k * (double)m).
            s = floor((2 sum d + n_in) / (2 n_in)) per axis; centre c = floor(sum q / n_in); u = q_x - c_x, v = q_y - c_y.
            Affine (model 1) when n_in >= 6 (else FEW), Cuu and Cvv >= (n n) (smin smin) as doubles (else SPREAD), Cuv Cuv <= 0.75 (Cuu Cvv) as doubles
            (else CORR), and after the solve every |gain| <= max_gain (else GAIN); otherwise the translation s.  T(q) = llrint((b0 + g_u u) + g_v v)
            per axis (translation: s); shift = T(c) = llrint(b0); JUMP when |shift| > jump * 1024 on either axis.
  apply     C = q - T(q) for every present cell of a moved column in a row with an estimate, C = q in a row without.
After the last round the value of such a cell is (double)C / 1024.0; rows without an estimate and absent cells keep their bytes."""
from fractions import Fraction

import numpy as np

import smooth_ref as SR

PLAYER, GOALKEEPER, BALL, BOUNDARY = 0, 1, 2, 3
LIMIT, Q = 1024.0, 1024.0
MAX_VOTERS = 64
A0_CAP = 2.0 ** 40
VOTE_CAP = 2 ** 24
F_OVER_CAP, F_FEW, F_SPREAD, F_CORR, F_GAIN, F_JUMP = 1, 2, 4, 8, 16, 32
M_NONE, M_TRANSLATION, M_AFFINE = 0, 1, 2
ROW_DTYPE = np.dtype([("voters", "<i4"), ("inliers", "<i4"), ("model", "<i4"), ("flags", "<i4"), ("shift_q", "<i4", (2,)), ("centre_q", "<i4", (2,)),
                      ("offset", "<f8", (2,)), ("gain", "<f8", (4,)), ("ss_before", "<i8"), ("ss_after", "<i8"), ("moved", "<i4"), ("reserved", "<i4")])
TOTALS_DTYPE = np.dtype([("ss_before", "<i8"), ("ss_after", "<i8"), ("inliers", "<i8"), ("moved", "<i8"), ("rows", "<i4"), ("none", "<i4"), ("translation", "<i4"),
                         ("affine", "<i4"), ("few_inliers", "<i4"), ("low_spread", "<i4"), ("correlated", "<i4"), ("high_gain", "<i4"), ("jumps", "<i4"),
                         ("over_cap", "<i4"), ("iterations", "<i4"), ("window", "<i4")])
assert ROW_DTYPE.itemsize == 104 and TOTALS_DTYPE.itemsize == 80
DEFAULTS = dict(degree=2, model=1, min_voters=6, iterations=2, trim_k=3.0, floor=0.1, min_spread=5.0, max_gain=0.05, jump=1.0)


def default_window(fps):
    return min(64, max(2, int(round(1.0 * fps))))


def check(fps, window, degree, model, min_voters, iterations, trim_k, floor, min_spread, max_gain, jump):
    """ValueError for what the library refuses with EAGLE_E_INVALID"""
    fin = lambda v: v == v and abs(v) != float("inf")
    if fps <= 0:
        raise ValueError(f"fps {fps} must be positive")
    if not 1 <= window <= 64:
        raise ValueError(f"window {window} is outside 1 .. 64")
    if degree not in (1, 2):
        raise ValueError(f"degree {degree} is neither 1 nor 2")
    if model not in (0, 1):
        raise ValueError(f"model {model} is neither 0 (translation) nor 1 (affine)")
    if not 3 <= min_voters <= 64:
        raise ValueError(f"min_voters {min_voters} is outside 3 .. 64")
    if not 1 <= iterations <= 4:
        raise ValueError(f"iterations {iterations} is outside 1 .. 4")
    if not (fin(trim_k) and (trim_k == 0 or 1.0 <= trim_k <= 1000.0)):
        raise ValueError(f"trim_k {trim_k} must be 0 (no trimming) or lie in 1 .. 1000")
    if not (fin(floor) and 0.0 <= floor <= 1024.0):
        raise ValueError(f"floor {floor} must lie in 0 .. 1024")
    if not (fin(min_spread) and 0.0 < min_spread <= 1024.0):
        raise ValueError(f"min_spread {min_spread} must be positive and at most 1024")
    if not (fin(max_gain) and 0.0 < max_gain <= 1.0):
        raise ValueError(f"max_gain {max_gain} must be positive and at most 1")
    if not (fin(jump) and jump > 0.0):
        raise ValueError(f"jump {jump} must be positive and finite")


def column_kinds(columns):
    """per column: 0 untouched, 1 moved only (the ball), 3 voter and moved"""
    out = []
    for kind, _, video in columns:
        if kind not in (PLAYER, GOALKEEPER, BALL, BOUNDARY):
            raise ValueError(f"column of unknown kind {kind}")
        out.append(0 if video else 3 if kind in (PLAYER, GOALKEEPER) else 1 if kind == BALL else 0)
    return out


def affine_solve(n, Su, Sv, Suu, Suv, Svv, D0, Du, Dv):
    """(b0, g_u, g_v) of one axis: Cramer's rule in float64 on the integer sums converted to double, every product and sum single and in this order"""
    n, Su, Sv, Suu, Suv, Svv, D0, Du, Dv = (float(v) for v in (n, Su, Sv, Suu, Suv, Svv, D0, Du, Dv))
    C00 = Suu * Svv - Suv * Suv
    C01 = Suv * Sv - Su * Svv
    C02 = Su * Suv - Suu * Sv
    C11 = n * Svv - Sv * Sv
    C12 = Su * Sv - n * Suv
    C22 = n * Suu - Su * Su
    det = (n * C00 + Su * C01) + Sv * C02
    return (((C00 * D0 + C01 * Du) + C02 * Dv) / det, ((C01 * D0 + C11 * Du) + C12 * Dv) / det, ((C02 * D0 + C12 * Du) + C22 * Dv) / det)


def affine_exact(n, Su, Sv, Suu, Suv, Svv, D0, Du, Dv):
    """the least-squares plane d ~ b0 + g_u u + g_v v as exact fractions"""
    A = [[Fraction(n), Fraction(Su), Fraction(Sv), Fraction(D0)], [Fraction(Su), Fraction(Suu), Fraction(Suv), Fraction(Du)], [Fraction(Sv), Fraction(Suv), Fraction(Svv), Fraction(Dv)]]
    for i in range(3):
        p = next(r for r in range(i, 3) if A[r][i] != 0)
        A[i], A[p] = A[p], A[i]
        A[i] = [v / A[i][i] for v in A[i]]
        for r in range(3):
            if r != i:
                A[r] = [a - A[r][i] * b for a, b in zip(A[r], A[i])]
    return [A[i][3] for i in range(3)]


def _predict(f, present, Cc, q, r, W, degree, form):
    """the vote of row r of one column, or None; and the fit's record"""
    rows = len(f)
    rng = range(max(0, r - W), min(rows, r + W + 1)) if form == "window" else range(rows)
    win = [j for j in rng if j != r and present[j] and abs(f[j] - f[r]) <= W]
    n = len(win)
    if n < 2 or not any(j < r for j in win) or not any(j > r for j in win):
        return None, None
    if form == "window":
        S, Bx, By = [0] * 5, [0] * 3, [0] * 3
        for j in win:
            t, p = f[j] - f[r], 1
            for k in range(5):
                S[k] += p
                if k < 3:
                    Bx[k] += p * Cc[j][0]
                    By[k] += p * Cc[j][1]
                p *= t
    else:
        ts = [f[j] - f[r] for j in win]
        S = [sum(t ** k for t in ts) for k in range(5)]
        Bx = [sum(t ** k * Cc[j][0] for t, j in zip(ts, win)) for k in range(3)]
        By = [sum(t ** k * Cc[j][1] for t, j in zip(ts, win)) for k in range(3)]
    deg = SR.degree_used(n, degree)
    ax, ay = SR.solve(S, Bx, deg), SR.solve(S, By, deg)
    fit = {"n": n, "deg": deg, "S": S, "Bx": Bx, "By": By, "ax": ax, "ay": ay, "win": win}
    if not (abs(ax[0]) <= A0_CAP and abs(ay[0]) <= A0_CAP):
        return None, fit
    d = (q[r][0] - int(round(ax[0])), q[r][1] - int(round(ay[0])))
    if abs(d[0]) > VOTE_CAP or abs(d[1]) > VOTE_CAP:
        return None, fit
    return d, fit


def _lower_median(v, form):
    rank = (len(v) - 1) // 2
    if form == "plain":
        return sorted(v)[rank]
    for a in v:                                                                     # the kernel's selection: the value with #{< a} <= rank < #{<= a}
        less, leq = sum(1 for b in v if b < a), sum(1 for b in v if b <= a)
        if less <= rank < leq:
            return a
    raise AssertionError("no element of the rank")


def _estimate(d, qv, over, moved, P, form):
    """d, qv: the row's voters in column order (at most 64) -> the row record as a dict, with the map"""
    n = len(d)
    rec = {"voters": n, "inliers": 0, "model": M_NONE, "flags": F_OVER_CAP if over else 0, "shift_q": (0, 0), "centre_q": (0, 0), "offset": (0.0, 0.0),
           "gain": (0.0, 0.0, 0.0, 0.0), "ss_before": 0, "ss_after": 0, "moved": 0}
    if n < P["min_voters"]:
        return rec
    bx, by = _lower_median([v[0] for v in d], form), _lower_median([v[1] for v in d], form)
    dev = [max(abs(v[0] - bx), abs(v[1] - by)) for v in d]
    m = _lower_median(dev, form)
    thr = max(P["floor"] * Q, P["trim_k"] * float(m))
    inl = [i for i in range(n) if P["trim_k"] == 0 or float(dev[i]) <= thr]
    ni = len(inl)
    assert ni >= 1
    if form == "window":
        sdx = sdy = sqx = sqy = ssb = 0
        for i in inl:
            sdx += d[i][0]; sdy += d[i][1]; sqx += qv[i][0]; sqy += qv[i][1]; ssb += d[i][0] * d[i][0] + d[i][1] * d[i][1]
    else:
        sdx, sdy = sum(d[i][0] for i in inl), sum(d[i][1] for i in inl)
        sqx, sqy = sum(qv[i][0] for i in inl), sum(qv[i][1] for i in inl)
        ssb = sum(d[i][0] ** 2 + d[i][1] ** 2 for i in inl)
    s = ((2 * sdx + ni) // (2 * ni), (2 * sdy + ni) // (2 * ni))
    c = (sqx // ni, sqy // ni)
    uv = [(qv[i][0] - c[0], qv[i][1] - c[1]) for i in inl]
    model, flags, off, gain = M_TRANSLATION, rec["flags"], (float(s[0]), float(s[1])), (0.0, 0.0, 0.0, 0.0)
    sums = None
    if P["model"] == 1:
        if form == "window":
            Su = Sv = Suu = Suv = Svv = Dux = Dvx = Duy = Dvy = 0
            for (u, v), i in zip(uv, inl):
                Su += u; Sv += v; Suu += u * u; Suv += u * v; Svv += v * v
                Dux += u * d[i][0]; Dvx += v * d[i][0]; Duy += u * d[i][1]; Dvy += v * d[i][1]
        else:
            Su, Sv = sum(u for u, _ in uv), sum(v for _, v in uv)
            Suu, Suv, Svv = sum(u * u for u, _ in uv), sum(u * v for u, v in uv), sum(v * v for _, v in uv)
            Dux, Dvx = sum(u * d[i][0] for (u, _), i in zip(uv, inl)), sum(v * d[i][0] for (_, v), i in zip(uv, inl))
            Duy, Dvy = sum(u * d[i][1] for (u, _), i in zip(uv, inl)), sum(v * d[i][1] for (_, v), i in zip(uv, inl))
        sums = (ni, Su, Sv, Suu, Suv, Svv, (sdx, Dux, Dvx), (sdy, Duy, Dvy))
        Cuu, Cvv, Cuv = ni * Suu - Su * Su, ni * Svv - Sv * Sv, ni * Suv - Su * Sv
        smin = P["min_spread"] * Q
        lim = float(ni * ni) * (smin * smin)
        if ni < 6:
            flags |= F_FEW
        elif not (float(Cuu) >= lim and float(Cvv) >= lim):
            flags |= F_SPREAD
        elif not (float(Cuv) * float(Cuv) <= 0.75 * (float(Cuu) * float(Cvv))):
            flags |= F_CORR
        else:
            gx = affine_solve(ni, Su, Sv, Suu, Suv, Svv, sdx, Dux, Dvx)
            gy = affine_solve(ni, Su, Sv, Suu, Suv, Svv, sdy, Duy, Dvy)
            if all(abs(g) <= P["max_gain"] for g in (gx[1], gx[2], gy[1], gy[2])) and abs(gx[0]) <= A0_CAP and abs(gy[0]) <= A0_CAP:
                model, off, gain = M_AFFINE, (gx[0], gy[0]), (gx[1], gx[2], gy[1], gy[2])
            else:
                flags |= F_GAIN

    def T(p):
        if model == M_TRANSLATION:
            return s
        u, v = float(p[0] - c[0]), float(p[1] - c[1])
        return (int(round((off[0] + gain[0] * u) + gain[1] * v)), int(round((off[1] + gain[2] * u) + gain[3] * v)))

    shift = T(c)
    if float(abs(shift[0])) > P["jump"] * Q or float(abs(shift[1])) > P["jump"] * Q:
        flags |= F_JUMP
    ssa = 0
    for i in inl:
        t = T(qv[i])
        ssa += (d[i][0] - t[0]) ** 2 + (d[i][1] - t[1]) ** 2
    rec.update(inliers=ni, model=model, flags=flags, shift_q=shift, centre_q=c, offset=off, gain=gain, ss_before=ssb, ss_after=ssa, moved=moved, T=T, inl=inl, b=(bx, by),
               dev=dev, m=m, s=s, sums=sums)
    return rec


def _wrap64(v):
    return ((int(v) + 2 ** 63) % 2 ** 64) - 2 ** 63


def stabilise(values, frames, columns, fps, window=None, form="window", **kw):
    """values float64 [cols][rows][2], frames [rows] strictly ascending, columns (kind, id, video) -> dict: values float64 [cols][rows][2]; rows ROW_DTYPE
    [rows]; votes int32 [cols][rows][2] (the last round's, (0, 0) where a cell did not vote); totals TOTALS_DTYPE [1]; and the intermediates of the last
    round (kinds, present, q, C, voted, fits, recs) plus `rounds`, the records of every round."""
    P = {**DEFAULTS, **kw}
    values = np.ascontiguousarray(values, np.float64)
    cols, rows = values.shape[:2]
    f = [int(v) for v in frames]
    W = default_window(fps) if window is None else int(window)
    check(fps, W, P["degree"], P["model"], P["min_voters"], P["iterations"], P["trim_k"], P["floor"], P["min_spread"], P["max_gain"], P["jump"])
    assert all(b > a for a, b in zip(f, f[1:])), "frame numbers must ascend"
    kinds = column_kinds(columns)
    present, q = {}, {}
    for c in range(cols):
        if kinds[c]:
            present[c], q[c] = SR.quantise(values[c])
    Cq = {c: list(q[c]) for c in q}
    voters = [c for c in range(cols) if kinds[c] == 3]
    rounds = []
    for _ in range(P["iterations"]):
        votes, fits = {}, {}
        for c in voters:
            votes[c], fits[c] = [None] * rows, [None] * rows
            for r in range(rows):
                if present[c][r]:
                    votes[c][r], fits[c][r] = _predict(f, present[c], Cq[c], q[c], r, W, P["degree"], form)
        recs = []
        for r in range(rows):
            if form == "window":
                vc = []
                for c in voters:
                    if votes[c][r] is not None:
                        vc.append(c)
            else:
                vc = [c for c in range(cols) if kinds[c] == 3 and votes[c][r] is not None]
            over = len(vc) > MAX_VOTERS
            vc = vc[:MAX_VOTERS]
            moved = sum(1 for c in q if present[c][r])
            recs.append(_estimate([votes[c][r] for c in vc], [q[c][r] for c in vc], over, moved, P, form))
        newC = {}
        for c in q:
            newC[c] = list(q[c])
            for r in range(rows):
                if present[c][r] and recs[r]["model"] != M_NONE:
                    t = recs[r]["T"](q[c][r])
                    newC[c][r] = (q[c][r][0] - t[0], q[c][r][1] - t[1])
        Cq = newC
        rounds.append(recs)
    out = values.copy()
    for c in q:
        for r in range(rows):
            if present[c][r] and recs[r]["model"] != M_NONE:
                out[c, r] = (float(Cq[c][r][0]) / Q, float(Cq[c][r][1]) / Q)
    rec_arr = np.zeros(rows, ROW_DTYPE)
    for r, e in enumerate(recs):
        rec_arr[r] = (e["voters"], e["inliers"], e["model"], e["flags"], e["shift_q"], e["centre_q"], e["offset"], e["gain"], e["ss_before"], e["ss_after"], e["moved"] if e["model"] else 0, 0)
    vote_arr = np.zeros((cols, rows, 2), np.int32)
    for c in voters:
        for r in range(rows):
            if votes[c][r] is not None:
                vote_arr[c, r] = votes[c][r]
    totals = np.zeros(1, TOTALS_DTYPE)
    if form == "window":
        fl, md = rec_arr["flags"], rec_arr["model"]
        totals[0] = (_wrap64(sum(int(v) for v in rec_arr["ss_before"])), _wrap64(sum(int(v) for v in rec_arr["ss_after"])), int(rec_arr["inliers"].sum()), int(rec_arr["moved"].sum()),
                     rows, int((md == 0).sum()), int((md == 1).sum()), int((md == 2).sum()), int(((fl & F_FEW) != 0).sum()), int(((fl & F_SPREAD) != 0).sum()),
                     int(((fl & F_CORR) != 0).sum()), int(((fl & F_GAIN) != 0).sum()), int(((fl & F_JUMP) != 0).sum()), int(((fl & F_OVER_CAP) != 0).sum()), P["iterations"], W)
    else:
        t = [0] * 14
        for e in recs:
            t[0] += e["ss_before"]; t[1] += e["ss_after"]; t[2] += e["inliers"]; t[3] += e["moved"] if e["model"] else 0
            t[5 + e["model"]] += 1
            for k, bit in enumerate((F_FEW, F_SPREAD, F_CORR, F_GAIN, F_JUMP, F_OVER_CAP)):
                t[8 + k] += 1 if e["flags"] & bit else 0
        t[4] = rows
        totals[0] = (_wrap64(t[0]), _wrap64(t[1]), *t[2:14], P["iterations"], W)
    return {"values": out, "rows": rec_arr, "votes": vote_arr, "totals": totals, "kinds": kinds, "present": present, "q": q, "C": Cq, "voted": votes, "fits": fits,
            "recs": recs, "rounds": rounds, "window": W}


def rms_m(ss, n):
    """RMS residual in metres of a sum of squared residuals (in quantisation units squared) over n inliers"""
    return float(np.sqrt(ss / n)) / Q if n else 0.0
