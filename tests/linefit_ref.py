"""The written definition of line registration (K39; include/eagle.h eagle_linefit_* / eagle_op_linefit, csrc/linefit.hip): every bit of the line-pixel
masks, the refined homographies and the per-frame records.  The per-pixel part is stated twice: vectorised over a frame's pixels (numpy, float64 and
int64) and as plain loops over pixels and primitives (Python floats, which are IEEE doubles, and Python ints for every sum).  The per-frame part behind the
integer sums (solve, compose, decide) is a handful of float64 operations in a stated order and is written once, with Python floats.  The kernels equal
all of it with no tolerance.  Units: Q = 1 / 1024 m (K26's quantisation) wherever an integer stands for a length.

LINE PIXELS (integers)  Y = b + 2 g + r.  GRASS: g >= 48 and g - max(r, b) >= 16 (the shots stage's key).  A pixel p = (x, y) with k <= x <= w - 1 - k
         and k <= y <= h - 1 - k is a LINE PIXEL iff for d = (1, 0) or d = (0, 1): p - k d and p + k d are grass and Y(p) - max(Y(p - k d), Y(p + k d))
         >= tau; and, with boxes, iff it lies in no box: x1 - box_pad <= x <= x2 + box_pad and y1 - box_pad <= y <= y2 + box_pad in float64, the
         float32 boxes widened exactly (the top view's inclusive comparison).  MASK: uint32 [h][(w + 31) / 32], pixel x is bit x & 31 of word x >> 5.
TARGETS  PRIMS below, from minimap_ref's constants, q(v) = floor(v 1024 + 0.5): 17 segments (orient 0: the line x = c for a0 <= y <= a1; orient 1: y = c
         for a0 <= x <= a1), then the centre circle and the two penalty arcs (cx, cy, R, side, lim; side +1: only where qx > lim, -1: qx < lim).
MAP      sb = (h6 ((w - 1) / 2) + h7 (h - 1)) + h8, every operation single.  NO MAP when valid == 0, any h_i or sb is not finite, or sb == 0.  G = H when
         sb > 0, else -H; the rounds refine G and the sign returns at the end.
POINT    a line pixel (x, y) under a matrix M: u' = ((m0 x) + (m1 y)) + m2, v', w' from rows 1 and 2; it FAILS unless w' > 0 and X = u' / w', Y = v' / w'
         have |X| <= 1024 and |Y| <= 1024 (NaN fails); qx = floor(X 1024 + 0.5), qy likewise.
MATCH    segment orient 0: e = qx - c, candidate iff a0 <= qy <= a1; orient 1: e = qy - c, iff a0 <= qx <= a1.  Arc: d2 = (qx - cx)^2 + (qy - cy)^2,
         e = floor((d2 - R^2 + R) / (2 R)), the algebraic distance rounded to a Q; candidate on its side.  The target is the candidate of least e^2, ties
         to the earlier primitive; INLIER iff e^2 <= rq^2.
ROW      g in 1 / 128: a segment's (128, 0) or (0, 128); an arc's gx = floor((256 (qx - cx) + R) / (2 R)), gy likewise.  xs = (qx - 53760) >> 7 and
         ys = (qy - 34816) >> 7 (1 / 8 m about the centre spot; x = xs / 512 is the normalised coordinate, unit 64 m), t = gx xs + gy ys,
         J = (512 gx, gx xs, gx ys, 512 gy, gy xs, gy ys, -((t xs) >> 9), -((t ys) >> 9)): the gradient times d(dx, dy)/da of
         dx = a0 + a1 x + a2 y - (a6 x + a7 y) x, dy = a3 + a4 x + a5 y - (a6 x + a7 y) y, in units of 2^-16.
SUMS     per frame and evaluation, exact integers: N[i][j] = sum J_i J_j (i <= j), b[i] = sum J_i e, cnt, se2 = sum e^2, and the inliers per primitive.
         |J_i| < 2^17 and |e| <= 2^13 (radius <= 8 m), a frame has at most 2^28 pixels: every sum stays below 2^62 (check_size).
ROUND    radii: r_0 = radius, r_(i + 1) = max(radius_min, r_i factor) in float64, rq_i = floor(r_i 1024 + 0.5).  From the sums at rq_i under the current
         matrix: nV, nH, nA = the orient-0 segments, orient-1 segments and arcs with at least min_per_line inliers.  LADDER from rung = model downwards:
         3 (projective, a0 .. a7) needs nV + nH + nA >= 4, nV + nA >= 2 and nH + nA >= 2; 2 (affine, a0 .. a5) needs nV + nH + nA >= 3, nV + nA >= 1
         and nH + nA >= 1; 1 (translation) needs nV + nH + nA >= 1 and solves a0 when nV + nA >= 1 and a3 when nH + nA >= 1; a rung that lacks its
         lines falls (cause LINES).  SOLVE N a = -b over the rung's unknowns in float64: Gaussian elimination, in column c the pivot is the row r >= c
         of largest |A[r][c]| (the first of equals); it fails (cause PIVOT) unless |pivot| >= 1e-9 times the largest diagonal entry of the rung's N;
         elimination and back substitution as solve() writes them.  CAP: the rung falls unless every |64 a_i| <= max_step (NaN fails) and the new
         matrix is finite.  NEW MATRIX = T (D (T^-1 M)), D = [[1 + a1, a2, a0], [a4, 1 + a5, a3], [a6, a7, 1]], T = [[64, 0, 52.5], [0, 64, 34],
         [0, 0, 1]], every entry of a product ((r0 c0) + (r1 c1)) + (r2 c2).  Rung 0 leaves the matrix as it is.
DECIDE   cnt and se2 at rq = floor(radius_min 1024 + 0.5) under G (before) and under the last matrix (after).  SHIFT: over the nine image points
         x in {0, (w - 1) / 2, w - 1}, y in {0, (h - 1) / 2, h - 1} whose POINT under G has -10240 <= qx <= 117760 and -10240 <= qy <= 79872 (the part of
         the view within 10 m of the pitch), shift2 = the largest squared distance between the POINT under G and under the last matrix; a point that
         fails under the last matrix gives shift2 = -1.  Status, the first that applies: NO_MAP; UNCHANGED (no round left rung 0, or rounds == 0);
         FEW_POINTS (cnt after < min_points); NO_GAIN (unless cnt before == 0 or se2 after / cnt after < se2 before / cnt before, float64 quotients);
         SHIFT (shift2 == -1 or shift2 > floor(max_shift 1024 + 0.5)^2); else ACCEPTED: Hs_out = the last matrix, negated when G = -H.  Every other
         status keeps the frame's nine doubles bit for bit.  Frames are independent.
RECORD   status, model (the last round's rung), rounds, n_line, n_before, n_after, fall (bit 3 (rung - 1) + cause for every rung that fell in any round,
         cause 0 LINES, 1 PIVOT, 2 CAP), e2_before, e2_after, shift2.  A frame without a map has n_line and zeros."""
import numpy as np

import minimap_ref as MR

F = np.float64
NO_MAP, ACCEPTED, UNCHANGED, FEW_POINTS, NO_GAIN, SHIFT = range(6)
LINES, PIVOT, CAP = range(3)
MAX_DIM, MAX_DET = 16384, 300
ROW_MAX, E_MAX, MAX_PIXELS = 1 << 17, 1 << 13, 1 << 28
PIVOT_REL = 1e-9
NSUM = 66                                                       # 36 N, 8 b, cnt, se2, 20 per primitive
FRAME_DTYPE = np.dtype([("status", "<i4"), ("model", "<i4"), ("rounds", "<i4"), ("n_line", "<i4"), ("n_before", "<i4"), ("n_after", "<i4"), ("fall", "<i4"),
                        ("reserved", "<i4"), ("e2_before", "<i8"), ("e2_after", "<i8"), ("shift2", "<i8")])
DEFAULTS = dict(k=4, tau=200, rounds=5, model=3, min_points=200, min_per_line=20, box_pad=3.0, radius=2.5, radius_min=0.5, radius_factor=0.6, max_shift=3.0,
                max_step=4.0)


def q(v):
    return int(np.floor(F(v) * F(1024) + F(0.5)))


CX, CY = q(MR.MID_X), q(MR.MID_Y)
_X = dict(w=q(MR.PW), h=q(MR.PH), pa=q(MR.PA_X), par=q(MR.PW - MR.PA_X), pa0=q(MR.PA_Y0), pa1=q(MR.PA_Y1), ga=q(MR.GA_X), gar=q(MR.PW - MR.GA_X), ga0=q(MR.GA_Y0),
          ga1=q(MR.GA_Y1), pm=q(MR.PM_X), pmr=q(MR.PW - MR.PM_X), R=q(MR.CIRCLE_R))
SEGMENTS = (
    (1, 0, 0, _X["w"]), (1, _X["h"], 0, _X["w"]), (0, 0, 0, _X["h"]), (0, _X["w"], 0, _X["h"]), (0, CX, 0, _X["h"]),
    (0, _X["pa"], _X["pa0"], _X["pa1"]), (1, _X["pa0"], 0, _X["pa"]), (1, _X["pa1"], 0, _X["pa"]),
    (0, _X["par"], _X["pa0"], _X["pa1"]), (1, _X["pa0"], _X["par"], _X["w"]), (1, _X["pa1"], _X["par"], _X["w"]),
    (0, _X["ga"], _X["ga0"], _X["ga1"]), (1, _X["ga0"], 0, _X["ga"]), (1, _X["ga1"], 0, _X["ga"]),
    (0, _X["gar"], _X["ga0"], _X["ga1"]), (1, _X["ga0"], _X["gar"], _X["w"]), (1, _X["ga1"], _X["gar"], _X["w"]),
)
ARCS = ((CX, CY, _X["R"], 0, 0), (_X["pm"], CY, _X["R"], 1, _X["pa"]), (_X["pmr"], CY, _X["R"], -1, _X["par"]))
NSEG, NPRIM = len(SEGMENTS), len(SEGMENTS) + len(ARCS)
# the table csrc/linefit.hip holds as literals
assert SEGMENTS == ((1, 0, 0, 107520), (1, 69632, 0, 107520), (0, 0, 0, 69632), (0, 107520, 0, 69632), (0, 53760, 0, 69632), (0, 16896, 14172, 55460),
                    (1, 14172, 0, 16896), (1, 55460, 0, 16896), (0, 90624, 14172, 55460), (1, 14172, 90624, 107520), (1, 55460, 90624, 107520),
                    (0, 5632, 25436, 44196), (1, 25436, 0, 5632), (1, 44196, 0, 5632), (0, 101888, 25436, 44196), (1, 25436, 101888, 107520),
                    (1, 44196, 101888, 107520))
assert ARCS == ((53760, 34816, 9370, 0, 0), (11264, 34816, 9370, 1, 16896), (96256, 34816, 9370, -1, 90624)) and (CX, CY) == (53760, 34816)
NEAR = (-10240, 107520 + 10240, -10240, 69632 + 10240)
T = (64.0, 0.0, 52.5, 0.0, 64.0, 34.0, 0.0, 0.0, 1.0)
TINV = (0.015625, 0.0, -0.8203125, 0.0, 0.015625, -0.53125, 0.0, 0.0, 1.0)
BIG = 1 << 62


def params(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    p = dict(DEFAULTS, **kw)
    check_params(p)
    return p


def check_params(p):
    assert 1 <= p["k"] <= 64 and 1 <= p["tau"] <= 1020 and 0 <= p["rounds"] <= 16 and 1 <= p["model"] <= 3 and p["min_points"] >= 1 and p["min_per_line"] >= 1, p
    assert 0 <= p["box_pad"] < np.inf and 0 < p["radius_min"] <= p["radius"] <= 8 and 0 < p["radius_factor"] <= 1, p
    assert 0 <= p["max_shift"] <= 1024 and 0 < p["max_step"] <= 64 and q(p["radius_min"]) >= 1, p


def overflow_bound(pixels):
    """the largest value any sum of a frame with this many pixels can reach stays below 2^63"""
    assert pixels * max(ROW_MAX * ROW_MAX, ROW_MAX * E_MAX, E_MAX * E_MAX) < (1 << 63), pixels
    return True


def check_size(h, w):
    assert 1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM, (h, w)
    assert h * w <= MAX_PIXELS and overflow_bound(h * w)


def radii(p):
    """-> rq per round (Q), and the deciding rq"""
    out, r = [], F(p["radius"])
    for _ in range(p["rounds"]):
        out.append(q(r))
        r = r * F(p["radius_factor"])
        if r < F(p["radius_min"]):
            r = F(p["radius_min"])
    return out, q(p["radius_min"])


def frame_map(H, valid, h, w):
    """-> (G as 9 Python floats, flipped) or None"""
    if not valid:
        return None
    Hm = [float(t) for t in np.asarray(H, F).reshape(9)]
    with np.errstate(all="ignore"):
        sb = float((F(Hm[6]) * (F(w - 1) / F(2)) + F(Hm[7]) * F(h - 1)) + F(Hm[8]))
    if not (np.isfinite(Hm).all() and np.isfinite(sb)) or sb == 0:
        return None
    return (Hm, False) if sb > 0 else ([-t for t in Hm], True)


def words(w):
    return (w + 31) // 32


def pack_mask(m):
    """bool [h, w] -> uint32 [h, words(w)]"""
    h, w = m.shape
    pad = np.zeros((h, words(w) * 32), np.uint32)
    pad[:, :w] = m
    return (pad.reshape(h, -1, 32) << np.arange(32, dtype=np.uint32)).sum(2, dtype=np.uint64).astype(np.uint32)


def unpack_mask(bits, w):
    b = (bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return b.reshape(len(bits), -1)[:, :w].astype(bool)


def _boxes(boxes):
    return np.zeros((0, 4), F) if boxes is None else np.asarray(boxes, np.float32).reshape(-1, 4).astype(F)


# ---- vectorised -----------------------------------------------------------------------------------------------------------------
def line_mask(frame, boxes, p):
    """uint8 [h, w, 3] BGR -> bool [h, w]"""
    f = np.asarray(frame, np.uint8).astype(np.int64)
    h, w, _ = f.shape
    k, tau = p["k"], p["tau"]
    out = np.zeros((h, w), bool)
    if h < 2 * k + 1 or w < 2 * k + 1:
        return out
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    Y = b + 2 * g + r
    grass = (g >= 48) & (g - np.maximum(r, b) >= 16)
    c = (slice(k, h - k), slice(k, w - k))
    hit = np.zeros((h - 2 * k, w - 2 * k), bool)
    for lo, hi in (((slice(k, h - k), slice(0, w - 2 * k)), (slice(k, h - k), slice(2 * k, w))), ((slice(0, h - 2 * k), slice(k, w - k)), (slice(2 * k, h), slice(k, w - k)))):
        hit |= grass[lo] & grass[hi] & (Y[c] - np.maximum(Y[lo], Y[hi]) >= tau)
    out[c] = hit
    pad = F(p["box_pad"])
    xs, ys = np.arange(w, dtype=F)[None, :], np.arange(h, dtype=F)[:, None]
    for x1, y1, x2, y2 in _boxes(boxes):
        out &= ~((x1 - pad <= xs) & (xs <= x2 + pad) & (y1 - pad <= ys) & (ys <= y2 + pad))
    return out


def points(M, px, py):
    """POINT for float64 arrays of pixel coordinates -> (ok bool, qx, qy int64; 0 where not ok)"""
    px, py = np.asarray(px, F), np.asarray(py, F)
    with np.errstate(all="ignore"):
        up, vp, wp = (((F(M[3 * r]) * px) + (F(M[3 * r + 1]) * py)) + F(M[3 * r + 2]) for r in range(3))
        X, Y = up / wp, vp / wp
        ok = (wp > 0) & (np.abs(X) <= 1024) & (np.abs(Y) <= 1024)
        qx = np.floor(np.where(ok, X, 0) * F(1024) + F(0.5)).astype(np.int64)
        qy = np.floor(np.where(ok, Y, 0) * F(1024) + F(0.5)).astype(np.int64)
    return ok, qx, qy


def match(qx, qy):
    """-> (best primitive int64, -1: none; e int64)"""
    n = len(qx)
    e2s, es = np.full((NPRIM, n), BIG, np.int64), np.zeros((NPRIM, n), np.int64)
    for i, (o, c, a0, a1) in enumerate(SEGMENTS):
        along, across = (qy, qx) if o == 0 else (qx, qy)
        e = across - c
        es[i] = e
        e2s[i] = np.where((a0 <= along) & (along <= a1), e * e, BIG)
    for j, (cx, cy, R, side, lim) in enumerate(ARCS):
        d2 = (qx - cx) ** 2 + (qy - cy) ** 2
        e = (d2 - R * R + R) // (2 * R)
        cand = np.ones(n, bool) if side == 0 else (qx > lim if side > 0 else qx < lim)
        es[NSEG + j] = e
        e2s[NSEG + j] = np.where(cand, e * e, BIG)
    best = np.argmin(e2s, 0) if n else np.zeros(0, np.int64)
    idx = np.arange(n)
    return np.where(e2s[best, idx] < BIG, best, -1), es[best, idx]


def rows(qx, qy, prim):
    """J int64 [n, 8] of inliers matched to `prim`"""
    gx, gy = np.zeros(len(qx), np.int64), np.zeros(len(qx), np.int64)
    for i, (o, _, _, _) in enumerate(SEGMENTS):
        gx[prim == i], gy[prim == i] = (128, 0) if o == 0 else (0, 128)
    for j, (cx, cy, R, _, _) in enumerate(ARCS):
        m = prim == NSEG + j
        gx[m], gy[m] = (256 * (qx[m] - cx) + R) // (2 * R), (256 * (qy[m] - cy) + R) // (2 * R)
    xs, ys = (qx - CX) >> 7, (qy - CY) >> 7
    t = gx * xs + gy * ys
    return np.stack([512 * gx, gx * xs, gx * ys, 512 * gy, gy * xs, gy * ys, -((t * xs) >> 9), -((t * ys) >> 9)], 1)


def sums(M, px, py, rq):
    """the integer sums of one evaluation -> list of NSUM Python ints"""
    ok, qx, qy = points(M, px, py)
    qx, qy = qx[ok], qy[ok]
    prim, e = match(qx, qy)
    inl = (prim >= 0) & (e * e <= rq * rq)
    qx, qy, prim, e = qx[inl], qy[inl], prim[inl], e[inl]
    J = rows(qx, qy, prim)
    assert (np.abs(J) < ROW_MAX).all() and (np.abs(e) <= E_MAX).all()
    out = [int((J[:, i] * J[:, j]).sum()) for i in range(8) for j in range(i, 8)]
    out += [int((J[:, i] * e).sum()) for i in range(8)]
    out += [len(e), int((e * e).sum())]
    return out + [int((prim == i).sum()) for i in range(NPRIM)]


# ---- scalar: loops over pixels and primitives, Python ints for the sums -----------------------------------------------------------
def line_mask_scalar(frame, boxes, p):
    f = np.asarray(frame, np.uint8).tolist()
    h, w = len(f), len(f[0])
    k, tau, pad = p["k"], p["tau"], float(p["box_pad"])
    bx = [tuple(float(t) for t in b) for b in _boxes(boxes)]
    Y = lambda x, y: f[y][x][0] + 2 * f[y][x][1] + f[y][x][2]
    grass = lambda x, y: f[y][x][1] >= 48 and f[y][x][1] - max(f[y][x][2], f[y][x][0]) >= 16
    out = np.zeros((h, w), bool)
    for y in range(k, h - k):
        for x in range(k, w - k):
            hit = False
            for dx, dy in ((k, 0), (0, k)):
                if grass(x - dx, y - dy) and grass(x + dx, y + dy) and Y(x, y) - max(Y(x - dx, y - dy), Y(x + dx, y + dy)) >= tau:
                    hit = True
            if hit and not any(x1 - pad <= float(x) and float(x) <= x2 + pad and y1 - pad <= float(y) and float(y) <= y2 + pad for x1, y1, x2, y2 in bx):
                out[y, x] = True
    return out


def point_scalar(M, x, y):
    """-> (qx, qy) or None; M Python floats"""
    x, y = float(x), float(y)
    up = ((M[0] * x) + (M[1] * y)) + M[2]
    vp = ((M[3] * x) + (M[4] * y)) + M[5]
    wp = ((M[6] * x) + (M[7] * y)) + M[8]
    if not wp > 0:
        return None
    X, Y = up / wp, vp / wp
    if not (abs(X) <= 1024 and abs(Y) <= 1024):
        return None
    return int((X * 1024.0 + 0.5) // 1), int((Y * 1024.0 + 0.5) // 1)


def match_scalar(qx, qy):
    """-> (primitive or -1, e)"""
    best, be, be2 = -1, 0, None
    for i, (o, c, a0, a1) in enumerate(SEGMENTS):
        along, across = (qy, qx) if o == 0 else (qx, qy)
        if a0 <= along <= a1:
            e = across - c
            if be2 is None or e * e < be2:
                best, be, be2 = i, e, e * e
    for j, (cx, cy, R, side, lim) in enumerate(ARCS):
        if side == 0 or (side > 0 and qx > lim) or (side < 0 and qx < lim):
            e = ((qx - cx) ** 2 + (qy - cy) ** 2 - R * R + R) // (2 * R)
            if be2 is None or e * e < be2:
                best, be, be2 = NSEG + j, e, e * e
    return best, be


def row_scalar(qx, qy, prim):
    if prim < NSEG:
        gx, gy = (128, 0) if SEGMENTS[prim][0] == 0 else (0, 128)
    else:
        cx, cy, R, _, _ = ARCS[prim - NSEG]
        gx, gy = (256 * (qx - cx) + R) // (2 * R), (256 * (qy - cy) + R) // (2 * R)
    xs, ys = (qx - CX) >> 7, (qy - CY) >> 7
    t = gx * xs + gy * ys
    return [512 * gx, gx * xs, gx * ys, 512 * gy, gy * xs, gy * ys, -((t * xs) >> 9), -((t * ys) >> 9)]


def sums_scalar(M, px, py, rq):
    out = [0] * NSUM
    for x, y in zip(px, py):
        pt = point_scalar(M, x, y)
        if pt is None:
            continue
        prim, e = match_scalar(*pt)
        if prim < 0 or e * e > rq * rq:
            continue
        J = row_scalar(pt[0], pt[1], prim)
        assert all(abs(t) < ROW_MAX for t in J) and abs(e) <= E_MAX
        s = 0
        for i in range(8):
            for j in range(i, 8):
                out[s] += J[i] * J[j]
                s += 1
        for i in range(8):
            out[36 + i] += J[i] * e
        out[44] += 1
        out[45] += e * e
        out[46 + prim] += 1
    return out


# ---- per frame: solve, compose, decide (Python floats; every operator a single IEEE operation) -----------------------------------------
def solve(S, idx):
    """N a = -b over the unknowns idx -> [a] (Python floats) or None (PIVOT)"""
    m = len(idx)
    pos = {}
    s = 0
    for i in range(8):
        for j in range(i, 8):
            pos[(i, j)] = pos[(j, i)] = s
            s += 1
    A = [[float(S[pos[(i, j)]]) for j in idx] for i in idx]
    rhs = [-float(S[36 + i]) for i in idx]
    dmax = max(A[i][i] for i in range(m))
    for c in range(m):
        piv = c
        for r in range(c + 1, m):
            if abs(A[r][c]) > abs(A[piv][c]):
                piv = r
        if not abs(A[piv][c]) >= PIVOT_REL * dmax or A[piv][c] == 0.0:
            return None
        A[c], A[piv] = A[piv], A[c]
        rhs[c], rhs[piv] = rhs[piv], rhs[c]
        for r in range(c + 1, m):
            f = A[r][c] / A[c][c]
            for j in range(c + 1, m):
                A[r][j] = A[r][j] - f * A[c][j]
            rhs[r] = rhs[r] - f * rhs[c]
    x = [0.0] * m
    for c in range(m - 1, -1, -1):
        s = rhs[c]
        for j in range(c + 1, m):
            s = s - A[c][j] * x[j]
        x[c] = s / A[c][c]
    return x


def matmul3(A, B):
    return [((A[3 * r] * B[c]) + (A[3 * r + 1] * B[3 + c])) + (A[3 * r + 2] * B[6 + c]) for r in range(3) for c in range(3)]


def compose(M, a):
    D = [1.0 + a[1], a[2], a[0], a[4], 1.0 + a[5], a[3], a[6], a[7], 1.0]
    with np.errstate(all="ignore"):
        return [float(t) for t in matmul3([F(t) for t in T], matmul3([F(t) for t in D], matmul3([F(t) for t in TINV], [F(t) for t in M])))]


def step(S, M, p):
    """one round's ladder on the sums S -> (new matrix, rung, fall bits)"""
    cnt = S[46:46 + NPRIM]
    nV = sum(1 for i, sg in enumerate(SEGMENTS) if sg[0] == 0 and cnt[i] >= p["min_per_line"])
    nH = sum(1 for i, sg in enumerate(SEGMENTS) if sg[0] == 1 and cnt[i] >= p["min_per_line"])
    nA = sum(1 for j in range(len(ARCS)) if cnt[NSEG + j] >= p["min_per_line"])
    nT, cX, cY = nV + nH + nA, nV + nA, nH + nA
    fall, rung = 0, p["model"]
    while rung > 0:
        bit = 3 * (rung - 1)
        if rung == 3:
            ok, idx = nT >= 4 and cX >= 2 and cY >= 2, list(range(8))
        elif rung == 2:
            ok, idx = nT >= 3 and cX >= 1 and cY >= 1, list(range(6))
        else:
            ok, idx = nT >= 1, ([0] if cX >= 1 else []) + ([3] if cY >= 1 else [])
        if not ok:
            fall |= 1 << (bit + LINES)
            rung -= 1
            continue
        x = solve(S, idx)
        if x is None:
            fall |= 1 << (bit + PIVOT)
            rung -= 1
            continue
        a = [0.0] * 8
        for i, v in zip(idx, x):
            a[i] = v
        new = compose(M, a)
        if not all(abs(v * 64.0) <= p["max_step"] for v in a) or not np.isfinite(new).all():
            fall |= 1 << (bit + CAP)
            rung -= 1
            continue
        return new, rung, fall
    return list(M), 0, fall


def grid_points(h, w):
    xs = (0.0, float(F(w - 1) / F(2)), float(w - 1))
    ys = (0.0, float(F(h - 1) / F(2)), float(h - 1))
    return [(x, y) for y in ys for x in xs]


def shift2(G, M, h, w):
    out = 0
    for x, y in grid_points(h, w):
        a = point_scalar(G, x, y)
        if a is None or not (NEAR[0] <= a[0] <= NEAR[1] and NEAR[2] <= a[1] <= NEAR[3]):
            continue
        b = point_scalar(M, x, y)
        if b is None:
            return -1
        out = max(out, (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2)
    return out


def refine_frame(mask, H, valid, p, sums_fn=sums):
    """one frame from its line mask -> (H_out float64 [9], record)"""
    h, w = mask.shape
    check_size(h, w)
    rec = np.zeros((), FRAME_DTYPE)
    rec["n_line"] = int(mask.sum())
    H = np.array(H, F).reshape(9)
    fm = frame_map(H, valid, h, w)
    if fm is None:
        return H.copy(), rec
    G, flipped = fm
    py, px = np.nonzero(mask)
    px, py = px.astype(F), py.astype(F)
    rqs, rq_end = radii(p)
    M, changed, fall, rung = list(G), False, 0, 0
    for rq in rqs:
        M, rung, fb = step(sums_fn(M, px, py, rq), M, p)
        fall |= fb
        changed = changed or rung > 0
    before, after = sums_fn(G, px, py, rq_end), sums_fn(M, px, py, rq_end)
    sh = shift2(G, M, h, w)
    rec["model"], rec["rounds"], rec["fall"] = rung, len(rqs), fall
    rec["n_before"], rec["e2_before"], rec["n_after"], rec["e2_after"], rec["shift2"] = before[44], before[45], after[44], after[45], sh
    ms = q(p["max_shift"])
    if not changed:
        st = UNCHANGED
    elif after[44] < p["min_points"]:
        st = FEW_POINTS
    elif not (before[44] == 0 or float(after[45]) / float(after[44]) < float(before[45]) / float(before[44])):
        st = NO_GAIN
    elif sh < 0 or sh > ms * ms:
        st = SHIFT
    else:
        st = ACCEPTED
    rec["status"] = st
    if st != ACCEPTED:
        return H.copy(), rec
    return np.array([-t for t in M] if flipped else M, F), rec


def linefit(frames, Hs, valid, boxes, p, scalar=False):
    """a clip -> (Hs_out float64 [n, 9], records FRAME_DTYPE [n], masks uint32 [n, h, words(w)])"""
    frames = np.asarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    check_params(p)
    check_size(h, w)
    Hs, valid = np.asarray(Hs, F).reshape(-1, 9), np.asarray(valid).reshape(-1)
    out, recs, masks = np.zeros((n, 9), F), np.zeros(n, FRAME_DTYPE), np.zeros((n, h, words(w)), np.uint32)
    for i in range(n):
        m = (line_mask_scalar if scalar else line_mask)(frames[i], None if boxes is None else boxes[i], p)
        masks[i] = pack_mask(m)
        out[i], recs[i] = refine_frame(m, Hs[i], valid[i], p, sums_scalar if scalar else sums)
    return out, recs, masks


def metres(e2, n):
    """RMS residual in metres of an integer e^2 sum over n inliers"""
    return float(np.sqrt(e2 / max(n, 1))) / 1024.0
