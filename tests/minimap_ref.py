"""numpy restatement of the library's minimap contract (include/eagle.h, eagle_minimap_* / eagle_op_minimap; csrc/minimap.hip): a processed
table's row -> a top-down picture of the pitch with the camera's footprint, the players in team colours, the ball and, on request, the Voronoi
areas of the players.  It is the single written definition of every output byte; the kernel equals it byte for byte, so everything after the
one quantisation step is integer arithmetic.

PARITY UNPINNED, OWN SPEC.  The picture follows the reference's examples/minimap.py and examples/voronoi.py in intent; the rasterisation is this
project's own (no matplotlib / mplsoccer pixels).

Geometry.  scale S = pixels per metre (even, 2 .. 32), margin M pixels (even, 0 .. 64): canvas w = 105 S + 2 M, h = 68 S + 2 M.  Pixel (X, Y)
has its centre at (16 X, 16 Y) in units of 1/16 pixel; pitch y points up, the canvas flips it.  With K = 16 S a pitch point (x, y) becomes
    qx = 16 M + floor(x K + 0.5)            qy = 16 M + 16 * 68 * S - floor(y K + 0.5)
(float64, one multiply and one add, no contraction).  A point is ABSENT when x or y is NaN or +-inf or |x| or |y| exceeds 1024 m; points off
the pitch but inside that domain are kept and clipped to the canvas.  The PITCH RECTANGLE is M <= X < M + 105 S, M <= Y < M + 68 S.

The draw list of a row: the table's pitch columns (video == 0) in table order, as eagle_overlay_from_table walks the video columns: boundary
columns are not entities, an absent cell is skipped, goalkeepers are green, a player is red (team 0) or blue (any other team), a player
without a mapping entry is skipped, white when the table has no mapping at all.  Voronoi sites are the drawn PLAYER entries.

Layers, a later one wins:
  1. black
  2. Voronoi tint (voronoi != 0; pitch rectangle only; no site, no tint): the pixel belongs to the site with the smallest
     (16 X - qx)^2 + (16 Y - qy)^2 (exact), ties to the earlier column; every channel becomes (c * 51 + bg * 205 + 128) >> 8.
  3. camera footprint (footprint != 0): the union of the triangles (BL, TL, TR) and (BL, TR, BR) of the FIRST boundary column of each corner,
     annot_ref's inclusive TRI rule on the 1/16 px vertices at the pixel centres; blended with white: (255 * 77 + bg * 179 + 128) >> 8.  Any
     corner absent (or its column missing): no footprint.
  4. pitch markings, white (markings()).
  5. a disc per Player / Goalkeeper entry in list order: d^2 <= (16 r)^2, r = player_radius or max(2, S).
  6. a white ring per Ball entry in list order: (16 (rb - t))^2 < d^2 <= (16 rb)^2, rb = ball_radius or max(3, S / 2 + 1), t = max(1, rb / 3).

Markings.  hw = max(1, S / 4) pixels (integer division).  A length d in metres is u(d) = floor(d K + 0.5) sixteenths; a line position is the
pixel P(u) = (u + 8) >> 4 of its quantised coordinate (q as above).  A straight line from a to b along an axis is the integer rectangle
[P(a) - hw, P(b) + hw] x [P(c) - hw, P(c) + hw] (c its constant coordinate), clipped to the canvas.  A circle of radius R metres about a
quantised centre is (u(R) - 16 hw)^2 <= d^2 <= (u(R) + 16 hw)^2; a mark is the disc d^2 <= (32 hw)^2.  Drawn: the outline, the halfway
line, the centre circle (R = 9.15) and centre mark, both penalty areas and goal areas, both penalty marks, and of the 9.15 m circle about each
penalty mark the part beyond the penalty area's front line (16 X > q of x = 16.5, 16 X < q of x = 88.5).

BGR -> 4:2:0 and every output layout are annot_ref's (bgr_to_yuv / annotate)."""
import numpy as np

import annot_ref as A
from eagle_amd import pitch

PLAYER, GOALKEEPER, BALL, BOUNDARY = 0, 1, 2, 3                  # include/eagle.h EAGLE_POST_*
S_MIN, S_MAX, M_MAX, DOMAIN = 2, 32, 64, 1024.0
TINT_A, FOOT_A = 51, 77
CIRCLE_R = 9.15                                                 # pitch.py: CENTER_CIRCLE_R.x - CENTER_MARK.x
_W = {lab: (x, y) for _, lab, x, y, _ in pitch.LANDMARKS}
PA_X, PA_Y0, PA_Y1 = _W["L_PENALTY_AREA_BR_CORNER"][0], _W["L_PENALTY_AREA_BR_CORNER"][1], _W["L_PENALTY_AREA_TR_CORNER"][1]      # 16.5, 13.84, 54.16
GA_X, GA_Y0, GA_Y1 = _W["L_GOAL_AREA_BR_CORNER"][0], _W["L_GOAL_AREA_BR_CORNER"][1], _W["L_GOAL_AREA_TR_CORNER"][1]               # 5.5, 24.84, 43.16
PM_X, MID_X, MID_Y = _W["L_PENALTY_MARK"][0], _W["CENTER_MARK"][0], _W["CENTER_MARK"][1]                                           # 11, 52.5, 34
PW, PH = float(pitch.PITCH_WIDTH), float(pitch.PITCH_HEIGHT)


def check_params(S, M):
    assert S % 2 == 0 and S_MIN <= S <= S_MAX and M % 2 == 0 and 0 <= M <= M_MAX, (S, M)


def size(S, M):
    check_params(S, M)
    return 105 * S + 2 * M, 68 * S + 2 * M


def radii(S, player_radius=0, ball_radius=0):
    r = player_radius or max(2, S)
    rb = ball_radius or max(3, S // 2 + 1)
    return r, rb, max(1, rb // 3)


def u(d, S):
    return int(np.floor(np.float64(d) * np.float64(16 * S) + np.float64(0.5)))


def quantise(x, y, S, M):
    """float64 arrays -> (qx, qy int64, present bool); absent entries are 0"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ok = np.isfinite(x) & np.isfinite(y)
    ok &= (np.abs(np.where(ok, x, 0)) <= DOMAIN) & (np.abs(np.where(ok, y, 0)) <= DOMAIN)
    K = np.float64(16 * S)
    xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    qx = 16 * M + np.floor(xs * K + 0.5).astype(np.int64)
    qy = 16 * M + 16 * 68 * S - np.floor(ys * K + 0.5).astype(np.int64)
    return np.where(ok, qx, 0), np.where(ok, qy, 0), ok


def draw_list(values, columns, team_mapping, row, S, M):
    """-> [(qx, qy, kind, (b, g, r), is_site)]: the discs in column order, then the balls in column order"""
    persons, balls = [], []
    for c, (kind, ident, video) in enumerate(columns):
        if video or kind == BOUNDARY:
            continue
        qx, qy, ok = quantise(values[c, row, 0], values[c, row, 1], S, M)
        if not ok:
            continue
        if kind == BALL:
            balls.append((int(qx), int(qy), BALL, A.WHITE, False))
            continue
        color = A.GREEN
        if kind == PLAYER:
            if team_mapping is None:
                color = A.WHITE
            elif ident in team_mapping:
                color = A.RED if int(team_mapping[ident]) == 0 else A.BLUE
            else:
                continue
        persons.append((int(qx), int(qy), kind, color, kind == PLAYER))
    return persons + balls


def corners(values, columns, row, S, M):
    """the four quantised footprint corners BL, TL, TR, BR as [(qx, qy)], or None when one is absent"""
    out = []
    for k in range(4):
        c = next((i for i, (kind, ident, video) in enumerate(columns) if kind == BOUNDARY and ident == k and not video), None)
        if c is None:
            return None
        qx, qy, ok = quantise(values[c, row, 0], values[c, row, 1], S, M)
        if not ok:
            return None
        out.append((int(qx), int(qy)))
    return out


_MARK_CACHE = {}


def markings(S, M):
    """bool [h, w]: the white pitch markings"""
    if (S, M) in _MARK_CACHE:
        return _MARK_CACHE[(S, M)]
    w, h = size(S, M)
    hw = max(1, S // 4)
    m = np.zeros((h, w), bool)
    qx = lambda x: 16 * M + u(x, S)
    qy = lambda y: 16 * M + 16 * 68 * S - u(y, S)
    P = lambda q: (q + 8) >> 4

    def rect(xa, xb, ya, yb):                       # inclusive pixel rectangle, clipped
        x0, x1, y0, y1 = max(min(xa, xb) - hw, 0), min(max(xa, xb) + hw, w - 1), max(min(ya, yb) - hw, 0), min(max(ya, yb) + hw, h - 1)
        if x0 <= x1 and y0 <= y1:
            m[y0:y1 + 1, x0:x1 + 1] = True

    def vline(x, ya, yb):
        rect(P(qx(x)), P(qx(x)), P(qy(ya)), P(qy(yb)))

    def hline(y, xa, xb):
        rect(P(qx(xa)), P(qx(xb)), P(qy(y)), P(qy(y)))

    for x in (0.0, MID_X, PW):
        vline(x, 0.0, PH)
    for y in (0.0, PH):
        hline(y, 0.0, PW)
    for bx, y0, y1 in ((PA_X, PA_Y0, PA_Y1), (GA_X, GA_Y0, GA_Y1)):
        vline(bx, y0, y1); vline(PW - bx, y0, y1)
        for y in (y0, y1):
            hline(y, 0.0, bx); hline(y, PW - bx, PW)
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    R, t = u(CIRCLE_R, S), 16 * hw

    def d2(cx, cy):
        return (16 * X - qx(cx)) ** 2 + (16 * Y - qy(cy)) ** 2

    def ring(cx, cy):
        d = d2(cx, cy)
        return ((R - t) ** 2 <= d) & (d <= (R + t) ** 2)

    m |= ring(MID_X, MID_Y)
    m |= ring(PM_X, MID_Y) & (16 * X > qx(PA_X))
    m |= ring(PW - PM_X, MID_Y) & (16 * X < qx(PW - PA_X))
    for cx in (MID_X, PM_X, PW - PM_X):
        m |= d2(cx, MID_Y) <= (2 * t) ** 2
    _MARK_CACHE[(S, M)] = m
    return m


def _blend(bg, color, a):
    return ((np.asarray(color, np.int64) * a + bg.astype(np.int64) * (256 - a) + 128) >> 8).astype(np.uint8)


def voronoi_labels(sites, S, M):
    """sites [(qx, qy, ...)] -> int [h, w]: index of the nearest site per pixel (exact integer distance, first minimum), -1 without sites"""
    w, h = size(S, M)
    lab = np.full((h, w), -1, np.int64)
    if not sites:
        return lab
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    best = None
    for i, s in enumerate(sites):
        d = (16 * X - s[0]) ** 2 + (16 * Y - s[1]) ** 2
        if best is None:
            best, lab[:] = d, 0
        else:
            win = d < best
            best = np.where(win, d, best)
            lab[win] = i
    return lab


def footprint_mask(cs, S, M):
    w, h = size(S, M)
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    bl, tl, tr, br = cs
    t1 = (A.TRI, bl[0], bl[1], tl[0], tl[1], tr[0], tr[1], A.WHITE)
    t2 = (A.TRI, bl[0], bl[1], tr[0], tr[1], br[0], br[1], A.WHITE)
    return A.covers(t1, 16 * X, 16 * Y) | A.covers(t2, 16 * X, 16 * Y)


def draw_row(values, columns, team_mapping, row, S, M, voronoi=0, footprint=1, player_radius=0, ball_radius=0):
    """one table row -> BGR uint8 [h, w, 3]"""
    w, h = size(S, M)
    r, rb, t = radii(S, player_radius, ball_radius)
    img = np.zeros((h, w, 3), np.uint8)
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    lst = draw_list(values, columns, team_mapping, row, S, M)
    if voronoi:
        assert team_mapping is not None
        sites = [e for e in lst if e[4]]
        lab = voronoi_labels(sites, S, M)
        inside = (X >= M) & (X < M + 105 * S) & (Y >= M) & (Y < M + 68 * S)
        for i, s in enumerate(sites):
            sel = inside & (lab == i)
            img[sel] = _blend(img[sel], s[3], TINT_A)
    if footprint:
        cs = corners(values, columns, row, S, M)
        if cs is not None:
            sel = footprint_mask(cs, S, M)
            img[sel] = _blend(img[sel], A.WHITE, FOOT_A)
    img[markings(S, M)] = A.WHITE
    for qx, qy, kind, color, _ in lst:
        d = (16 * X - qx) ** 2 + (16 * Y - qy) ** 2
        if kind == BALL:
            img[((16 * (rb - t)) ** 2 < d) & (d <= (16 * rb) ** 2)] = A.WHITE
        else:
            img[d <= (16 * r) ** 2] = color
    return img


def frames_bgr(values, columns, team_mapping, row0, n, S, M, **kw):
    w, h = size(S, M)
    return np.stack([draw_row(values, columns, team_mapping, row0 + i, S, M, **kw) for i in range(n)]) if n else np.zeros((0, h, w, 3), np.uint8)


def minimap(values, columns, team_mapping, row0, n, S, M, fmt=A.BGR, layout=None, fill=0, **kw):
    """values float64 [cols][rows][2], columns [(kind, id, video)], team_mapping {id: team} or None -> a flat uint8 buffer holding rows
    row0 .. row0 + n - 1 as frames in the given output format and layout; bytes the layout does not cover = fill."""
    fr = frames_bgr(values, columns, team_mapping, row0, n, S, M, **kw)
    return A.annotate(fr, [[] for _ in range(n)], fmt, layout, fill)
