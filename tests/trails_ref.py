"""numpy restatement of the minimap's trail, pass-arrow and owner-ring layers and of the two still pictures drawn with them (include/eagle.h,
eagle_minimap_set_trails / eagle_op_minimap_trails / eagle_trajectory_picture / eagle_pass_picture; csrc/minimap.hip, csrc/trails.hip).  It is the
single written definition of every output byte of those entries; the kernels equal it byte for byte.  OWN SPEC: the pictures follow the reference's
examples/trajectory.py and examples/pass.py in intent, the rasterisation is this project's own.

The pieces below layer 4 and the discs are minimap_ref's (quantise, draw_list, markings, voronoi_labels, footprint_mask, _blend, radii); this file
composes the layers itself.  Everything after minimap_ref.quantise is integer arithmetic, except the three vertices of an arrow head.

Layers, a later one wins (numbers are minimap_ref's):
  1 black, 2 tint (Voronoi, or the control colours handed in), 3 footprint, 4 markings,
  4a trails, 4b pass arrows, 5 discs with 5a the owner ring directly after the owner's disc, 6 the ball ring.

CAPSULE.  Quantised end points A, B in 1/16 px, hw16 = 16 half_width.  The pixel centre P = (16 X, 16 Y) is covered when its squared distance to
the segment is <= hw16^2, decided exactly: d = B - A, L2 = d.d, t = (P - A).d;
    t <= 0:   |P - A|^2 <= hw16^2            (L2 == 0 lands here: a zero-length segment is a disc)
    t >= L2:  |P - B|^2 <= hw16^2
    else:     cross = (P - A) x d,  cross^2 <= hw16^2 L2.
Bounds: |q| < 2^20 (1024 m at 32 px per metre is 2^19 sixteenths, plus the margin), so |d| < 2^21, |t| and |cross| < 2^42; cross^2 needs up to 84
bits and is compared as a full 128-bit product (the kernel: the high and the low 64-bit halves); hw16 <= 128 and L2 < 2^43 give hw16^2 L2 < 2^57,
which fits 64 bits.  Here the comparison is made on Python integers: cross^2 <= N is |cross| <= isqrt(N), isqrt of the Python integer N being exact
(capsule_mask(product="object") forms cross^2 itself on an object array and is the same set; product="wrap64" is the WRONG 64-bit product a kernel
must not compute, kept for the test that shows a case where it differs).

TRAILS.  selection: table columns, pitch columns (video == 0) of kind Player, Goalkeeper or Ball, none twice; window W >= 1, max_gap > 0,
half_width 1 .. 8 px, dim_floor 0 .. 256.  A column's colour is its disc's colour in draw_list (a player without a mapping entry has no trail, white
without a mapping, the ball white).  On the picture of row r column c contributes the segments (j - 1, j), max(1, r - W + 1) <= j <= r, whose two
cells pass quantise and for which frames[j] - frames[j - 1] <= max_gap; selection order across columns, the oldest segment first within a column; a
segment of age a = r - j is drawn OPAQUE in (c * f) >> 8 per channel, f = 256 - (a (256 - dim_floor)) // W (blending would show every joint).

PASS ARROWS.  Event e shows on the rows release_row <= r < receive_row + pass_hold.  Colour by kind: pass white, turnover (0, 255, 255), unknown
(160, 160, 160) (BGR).  The shaft is the capsule of the trails' half_width from A = q(x0, y0) to B = q(x1, y1); the head is the triangle (annot_ref's
inclusive TRI rule) B, H1, H2 with, in float64 without contraction from the exact integer d,
    s = sqrt((double) L2), ux = dx / s, uy = dy / s, cx = bx - hl ux, cy = by - hl uy,      hl = 64 half_width, hh = 32 half_width
    H1 = (floor((cx - hh uy) + 0.5), floor((cy + hh ux) + 0.5)),  H2 = (floor((cx + hh uy) + 0.5), floor((cy - hh ux) + 0.5)).
L2 == 0: no head.  Either cell absent: no arrow.  Events in event order, an event's shaft before its head.

OWNER RING.  owner[r] a column draw_list draws on row r as a person: white, (16 R)^2 < d^2 <= (16 (R + t))^2 right after that disc, R the disc
radius, t = max(1, R // 3).

STILLS, BGR [h][w][3] on the minimap's canvas.
  trajectory (cols, row0, n): layers 1 and 4; the selection's segments with row0 < j < row0 + n under the same presence and gap rule at f = 256;
      then per drawn column in selection order a ring (the ball ring's radii) at its first present cell of the window and a disc (the player
      disc's radius) at its last present cell, in the column's colour.  A column without a present cell in the window draws nothing.
  pass (event): the picture of release_row with layers 1, 4, 4b (this event only, whatever pass_hold is), 5 and 6, the person discs of columns other
      than from_col and to_col blended at a = 64 over what lies under them.

BGR -> 4:2:0 and every output layout are annot_ref's."""
import math

import numpy as np

import annot_ref as A
import minimap_ref as R

TRAILS, PASSES, OWNER = 1, 2, 4                                 # include/eagle.h EAGLE_MM_*
EV_PASS, EV_TURNOVER, EV_UNKNOWN = 0, 1, 2                      # include/eagle.h EAGLE_EVENT_*
EVENT_COLOR = {EV_PASS: (255, 255, 255), EV_TURNOVER: (0, 255, 255), EV_UNKNOWN: (160, 160, 160)}
DIM_A = 64
DEFAULTS = dict(window=25, max_gap=25, half_width=1, pass_hold=5, dim_floor=64)


def trail_params(**kw):
    p = dict(DEFAULTS, **kw)
    check_trail_params(p)
    return p


def check_trail_params(p):
    if p["window"] < 1 or p["max_gap"] < 1 or p["pass_hold"] < 1 or not 1 <= p["half_width"] <= 8 or not 0 <= p["dim_floor"] <= 256:
        raise ValueError("trail parameters out of range: %r" % (p,))


def check_selection(sel, columns):
    seen = set()
    for c in sel:
        if not 0 <= c < len(columns) or columns[c][2] or columns[c][0] not in (R.PLAYER, R.GOALKEEPER, R.BALL) or c in seen:
            raise ValueError("selection member %r is out of range, not a person or ball pitch column, or repeated" % (c,))
        seen.add(c)


def check_layers(layers, p, sel, owner, events):
    if layers & ~7:
        raise ValueError("unknown layer bits")
    if layers and p is None:
        raise ValueError("a layer without trail parameters")
    if layers & TRAILS and not sel:
        raise ValueError("trails with an empty selection")
    if (layers & PASSES and events is None) or (layers & OWNER and owner is None):
        raise ValueError("passes / owner without a possession result")


def column_color(columns, mapping, c):
    """the colour column c's disc has in draw_list, None for a player without a mapping entry"""
    kind, ident, _ = columns[c]
    if kind == R.BALL:
        return A.WHITE
    if kind == R.GOALKEEPER:
        return A.GREEN
    if mapping is None:
        return A.WHITE
    if ident not in mapping:
        return None
    return A.RED if int(mapping[ident]) == 0 else A.BLUE


def capsule_mask(ax, ay, bx, by, hw16, w, h, product="exact"):
    """bool [h, w]: the pixels the capsule rule covers"""
    m = np.zeros((h, w), bool)
    if product == "wrap64":
        x0, x1, y0, y1 = 0, w - 1, 0, h - 1
    else:                                                       # a covered pixel lies within hw16 of the segment: inside its grown box
        x0, x1 = max(-((hw16 - min(ax, bx)) // 16), 0), min((max(ax, bx) + hw16) // 16, w - 1)
        y0, y1 = max(-((hw16 - min(ay, by)) // 16), 0), min((max(ay, by) + hw16) // 16, h - 1)
    if x0 > x1 or y0 > y1:
        return m
    Y, X = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    px, py, qx, qy = 16 * X - ax, 16 * Y - ay, 16 * X - bx, 16 * Y - by
    dx, dy = bx - ax, by - ay
    L2, hw2 = dx * dx + dy * dy, hw16 * hw16
    t, cross = px * dx + py * dy, px * dy - py * dx
    if product == "exact":
        mid = np.abs(cross) <= math.isqrt(hw2 * L2)
    elif product == "object":
        co = cross.astype(object)
        mid = (co * co <= hw2 * L2).astype(bool)
    else:
        cu = np.abs(cross).astype(np.uint64)
        with np.errstate(over="ignore"):
            mid = cu * cu <= np.uint64(hw2 * L2)
    m[y0:y1 + 1, x0:x1 + 1] = np.where(t <= 0, px * px + py * py <= hw2, np.where(t >= L2, qx * qx + qy * qy <= hw2, mid))
    return m


def points(values, c, S, M):
    """column c over all rows -> (qx, qy int64 [rows], present bool [rows])"""
    return R.quantise(values[c, :, 0], values[c, :, 1], S, M)


def trail_segments(values, frames, columns, mapping, sel, row, S, M, p, jlo=None, dim=True):
    """-> [(ax, ay, bx, by, (b, g, r))] in drawing order for the picture of `row`"""
    W = p["window"]
    lo = max(1, row - W + 1) if jlo is None else jlo
    out = []
    for c in sel:
        color = column_color(columns, mapping, c)
        if color is None:
            continue
        qx, qy, ok = points(values, c, S, M)
        for j in range(lo, row + 1):
            if not (ok[j - 1] and ok[j]) or int(frames[j]) - int(frames[j - 1]) > p["max_gap"]:
                continue
            f = 256 - ((row - j) * (256 - p["dim_floor"])) // W if dim else 256
            out.append((int(qx[j - 1]), int(qy[j - 1]), int(qx[j]), int(qy[j]), tuple((ch * f) >> 8 for ch in color)))
    return out


def arrow(ev, S, M, half_width):
    """an event -> None (a cell absent) or (ax, ay, bx, by, head or None, colour); head = (h1x, h1y, h2x, h2y)"""
    ax, ay, oka = R.quantise(ev["x0"], ev["y0"], S, M)
    bx, by, okb = R.quantise(ev["x1"], ev["y1"], S, M)
    if not (oka and okb):
        return None
    ax, ay, bx, by = int(ax), int(ay), int(bx), int(by)
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    head = None
    if L2:
        f = np.float64
        s = np.sqrt(f(L2))
        ux, uy = f(dx) / s, f(dy) / s
        hl, hh = f(64 * half_width), f(32 * half_width)
        cx, cy = f(bx) - hl * ux, f(by) - hl * uy
        fl = lambda v: int(np.floor(v + f(0.5)))
        head = (fl(cx - hh * uy), fl(cy + hh * ux), fl(cx + hh * uy), fl(cy - hh * ux))
    return ax, ay, bx, by, head, EVENT_COLOR[int(ev["kind"])]


def visible_events(events, row, H):
    return [k for k, e in enumerate(events) if int(e["release_row"]) <= row < int(e["receive_row"]) + H]


def _grid(S, M):
    w, h = R.size(S, M)
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    return w, h, X, Y


def _draw_segments(img, segs, hw16):
    h, w = img.shape[:2]
    for ax, ay, bx, by, color in segs:
        img[capsule_mask(ax, ay, bx, by, hw16, w, h)] = color


def _draw_arrow(img, arw, hw16, X, Y):
    ax, ay, bx, by, head, color = arw
    h, w = img.shape[:2]
    img[capsule_mask(ax, ay, bx, by, hw16, w, h)] = color
    if head is not None:
        img[A.covers((A.TRI, bx, by, head[0], head[1], head[2], head[3], color), 16 * X, 16 * Y)] = color


def draw_row(values, frames, columns, mapping, row, S, M, layers=0, p=None, sel=(), owner=None, events=None, voronoi=0, footprint=1, player_radius=0,
             ball_radius=0, tint=None, only_event=None, dim_except=None):
    """one table row -> BGR uint8 [h, w, 3].  tint: BGR [68 S, 105 S, 3] colours of the control layer (in Voronoi's slot); only_event / dim_except:
    the pass still (layer 4b is that event alone; person discs of other columns than dim_except are blended)"""
    w, h, X, Y = _grid(S, M)
    r, rb, t = R.radii(S, player_radius, ball_radius)
    img = np.zeros((h, w, 3), np.uint8)
    lst = R.draw_list(values, columns, mapping, row, S, M)
    if voronoi:
        sites = [e for e in lst if e[4]]
        lab = R.voronoi_labels(sites, S, M)
        inside = (X >= M) & (X < M + 105 * S) & (Y >= M) & (Y < M + 68 * S)
        for i, s in enumerate(sites):
            pick = inside & (lab == i)
            img[pick] = R._blend(img[pick], s[3], R.TINT_A)
    if tint is not None:
        rect = img[M:M + 68 * S, M:M + 105 * S]
        rect[:] = R._blend(rect, tint, R.TINT_A)
    if footprint:
        cs = R.corners(values, columns, row, S, M)
        if cs is not None:
            pick = R.footprint_mask(cs, S, M)
            img[pick] = R._blend(img[pick], A.WHITE, R.FOOT_A)
    img[R.markings(S, M)] = A.WHITE
    hw16 = 16 * p["half_width"] if p is not None else 0
    if layers & TRAILS:
        _draw_segments(img, trail_segments(values, frames, columns, mapping, sel, row, S, M, p), hw16)
    if only_event is not None:
        arw = arrow(events[only_event], S, M, p["half_width"])
        if arw is not None:
            _draw_arrow(img, arw, hw16, X, Y)
    elif layers & PASSES:
        for k in visible_events(events, row, p["pass_hold"]):
            arw = arrow(events[k], S, M, p["half_width"])
            if arw is not None:
                _draw_arrow(img, arw, hw16, X, Y)
    # the draw list with the table column of every entry: draw_list's walk, kept beside it
    entry_cols = _entry_columns(values, columns, mapping, row, S, M)
    assert len(entry_cols) == len(lst)
    own = int(owner[row]) if (layers & OWNER and owner is not None) else -1
    to = max(1, r // 3)
    for (qx, qy, kind, color, _), c in zip(lst, entry_cols):
        d = (16 * X - qx) ** 2 + (16 * Y - qy) ** 2
        if kind == R.BALL:
            img[((16 * (rb - t)) ** 2 < d) & (d <= (16 * rb) ** 2)] = A.WHITE
            continue
        pick = d <= (16 * r) ** 2
        if dim_except is not None and c not in dim_except:
            img[pick] = R._blend(img[pick], color, DIM_A)
        else:
            img[pick] = color
        if c == own:
            img[((16 * r) ** 2 < d) & (d <= (16 * (r + to)) ** 2)] = A.WHITE
    return img


def _entry_columns(values, columns, mapping, row, S, M):
    persons, balls = [], []
    for c, (kind, ident, video) in enumerate(columns):
        if video or kind == R.BOUNDARY:
            continue
        _, _, ok = R.quantise(values[c, row, 0], values[c, row, 1], S, M)
        if not ok:
            continue
        if kind == R.BALL:
            balls.append(c)
        elif kind == R.GOALKEEPER or mapping is None or ident in mapping:
            persons.append(c)
    return persons + balls


def frames_bgr(values, frames, columns, mapping, row0, n, S, M, layers=0, p=None, sel=(), owner=None, events=None, **kw):
    check_layers(layers, p, sel, owner, events)
    if p is not None:
        check_trail_params(p)
    check_selection(sel, columns)
    w, h = R.size(S, M)
    if not n:
        return np.zeros((0, h, w, 3), np.uint8)
    return np.stack([draw_row(values, frames, columns, mapping, row0 + i, S, M, layers, p, sel, owner, events, **kw) for i in range(n)])


def minimap(values, frames, columns, mapping, row0, n, S, M, fmt=A.BGR, layout=None, fill=0, **kw):
    fr = frames_bgr(values, frames, columns, mapping, row0, n, S, M, **kw)
    return A.annotate(fr, [[] for _ in range(n)], fmt, layout, fill)


def trajectory_picture(values, frames, columns, mapping, sel, row0, n, S, M, half_width=1, max_gap=25):
    check_selection(sel, columns)
    rows = values.shape[1]
    if n < 1 or row0 < 0 or row0 + n > rows:
        raise ValueError("the row window lies outside the table")
    p = trail_params(window=max(1, n - 1), max_gap=max_gap, half_width=half_width)
    w, h, X, Y = _grid(S, M)
    r, rb, t = R.radii(S)
    img = np.zeros((h, w, 3), np.uint8)
    img[R.markings(S, M)] = A.WHITE
    _draw_segments(img, trail_segments(values, frames, columns, mapping, sel, row0 + n - 1, S, M, p, jlo=row0 + 1, dim=False), 16 * half_width)
    for c in sel:
        color = column_color(columns, mapping, c)
        qx, qy, ok = points(values, c, S, M)
        there = np.flatnonzero(ok[row0:row0 + n]) + row0
        if color is None or not len(there):
            continue
        d = (16 * X - int(qx[there[0]])) ** 2 + (16 * Y - int(qy[there[0]])) ** 2
        img[((16 * (rb - t)) ** 2 < d) & (d <= (16 * rb) ** 2)] = color
        d = (16 * X - int(qx[there[-1]])) ** 2 + (16 * Y - int(qy[there[-1]])) ** 2
        img[d <= (16 * r) ** 2] = color
    return img


def pass_picture(values, frames, columns, mapping, events, event, S, M, half_width=1):
    if not 0 <= event < len(events):
        raise ValueError("event outside the event count")
    e = events[event]
    p = trail_params(half_width=half_width)
    return draw_row(values, frames, columns, mapping, int(e["release_row"]), S, M, 0, p, (), None, events, footprint=0, only_event=event,
                    dim_except=(int(e["from_col"]), int(e["to_col"])))
