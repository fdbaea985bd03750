"""numpy / Python-integer restatement of the team-shape stage (include/eagle.h, eagle_post_team_shape / eagle_op_team_shape / eagle_op_minimap_hulls;
csrc/shape.hip) and of the minimap's hull layer.  It is the single written definition of every output bit and byte: the kernels equal it bit for bit.
OWN SPEC: nothing of the reference computes this; its users derive such figures by hand from processed_data.json.

MEMBERS.  Two groups: 0 = team value 0, 1 = any other non-negative team value (the minimap's red / blue).  The members of a group are the table's
Player pitch columns (video == 0) whose id has a mapping entry of that group; a column's team is the first mapping entry with its id (here the mapping
is a dict, so there is one).  Goalkeepers, balls, boundary columns, video columns and players without an entry (or with a negative one) are no members.
A mapping is required; more than MAX_MEMBERS members over both groups are refused.  A member is PRESENT on a row when x and y are finite and |x|, |y|
<= 1024 m (the minimap's rule).

QUANTISATION.  qx = (int) floor(x * 1024.0 + 0.5), qy likewise (float64; the multiply by a power of two is exact).  |q| <= 2^20, differences are at
most 2^21, every cross product and squared distance below is at most 2^43 and exact in int64.  Everything after this step is integer arithmetic, so no
sum depends on its order.

RECORD (SHAPE_DTYPE, one per row and group): n present members; sum_x, sum_y, sum_xx, sum_yy of q and q^2 over them; min_x, max_x, min_y, max_y and
the EARLIEST table column that attains each (col_*; 0 and -1 when n == 0); hull_n, the true number of hull vertices; area2, twice the hull's area in
q^2 (>= 0, over all vertices also when more than HULL_CAP exist); flags bit 0: hull_n > HULL_CAP, the stored vertex list is cut.

HULL (table columns, counter-clockwise with pitch y up, -1 padded to HULL_CAP).  The start is the present member with the smallest (qy, qx, column).
From the current vertex c the candidates are the present members whose q differs from q_c; candidate p BEATS the best so far b when
    o = (bx - cx)(py - cy) - (by - cy)(px - cx) < 0,   or   o == 0 and |p - c|^2 > |b - c|^2,   or   both equal and p's column is smaller.
The march ends when the winner is the start, when there is no candidate, and after at most n steps.  area2 = the sum over the appended vertices of
cross(q_prev - q_start, q_next - q_start) (a fan from the start; the first term is 0).

WHY ANY ORDER GIVES THE SAME WINNER.  c is always an extreme point of the present members (the start is the lowest-then-leftmost point; every later c
won against everyone from an extreme point, farthest on its ray).  So the directions of the candidates as seen from c lie in a cone of less than 180
degrees, or all on one ray.  Inside such a cone "o < 0" (p is clockwise of b) is a strict weak order of the directions; equal directions are ordered by
distance, equal distance on an equal direction means equal q, and those are ordered by column.  BEATS is therefore a strict total order of the
candidates and the winner is its maximum: a left fold, a tree, a wave's butterfly reduction all return it.  (hull() below folds from the left.)

Consequences: a point strictly inside an edge is no vertex; coincident points are one vertex, the earliest column; n == 0 gives hull_n 0; all present
members coincident give hull_n 1; all collinear give hull_n 2 and area2 0.

PICTURE: the hull layer of the minimap (EAGLE_MM_HULLS = 8, layer "4.0": after the markings, before the trails), group 0 first.  Edge i of a group
joins stored vertex i and i + 1 (mod k), k = min(hull_n, HULL_CAP): k edges when hull_n >= 3 and the list is not cut, k - 1 (no closing edge) when it
is cut, one when hull_n == 2, none below.  Both end points are the minimap's quantisation (minimap_ref.quantise) of the vertex's cell; an edge is
trails_ref's CAPSULE of the hull layer's own half_width (1 .. 8 px), opaque, in the group's disc colour scaled (c * 160) >> 8 per channel."""
import numpy as np

import annot_ref as A
import minimap_ref as R
import trails_ref as T

Q, DOMAIN, HULL_CAP, MAX_MEMBERS, HULLS, FLAG_CUT, HULL_SHADE = 1024, 1024.0, 32, 4096, 8, 1, 160
SHAPE_DTYPE = np.dtype([("sum_x", "<i8"), ("sum_y", "<i8"), ("sum_xx", "<i8"), ("sum_yy", "<i8"), ("area2", "<i8"), ("n", "<i4"), ("hull_n", "<i4"),
                        ("flags", "<i4"), ("reserved0", "<i4"), ("min_x", "<i4"), ("max_x", "<i4"), ("min_y", "<i4"), ("max_y", "<i4"),
                        ("col_min_x", "<i4"), ("col_max_x", "<i4"), ("col_min_y", "<i4"), ("col_max_y", "<i4"), ("reserved", "<i4", 2)])      # EagleTeamShape, 96 bytes


def members(columns, mapping):
    """-> ([columns of group 0], [columns of group 1]) in table order"""
    if mapping is None:
        raise ValueError("team shape needs a team mapping")
    out = ([], [])
    for c, (kind, ident, video) in enumerate(columns):
        if kind not in (R.PLAYER, R.GOALKEEPER, R.BALL, R.BOUNDARY):
            raise ValueError("column %d is of unknown kind %r" % (c, kind))
        if video or kind != R.PLAYER or ident not in mapping or int(mapping[ident]) < 0:
            continue
        out[0 if int(mapping[ident]) == 0 else 1].append(c)
    if len(out[0]) + len(out[1]) > MAX_MEMBERS:
        raise ValueError("more than %d members" % MAX_MEMBERS)
    return out


def quantise(x, y):
    """float64 arrays -> (qx, qy int64, present bool); absent entries are 0"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ok = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    ok &= (np.abs(xs) <= DOMAIN) & (np.abs(ys) <= DOMAIN)
    xs, ys = np.where(ok, xs, 0.0), np.where(ok, ys, 0.0)
    return np.floor(xs * np.float64(Q) + 0.5).astype(np.int64), np.floor(ys * np.float64(Q) + 0.5).astype(np.int64), ok


def beats(c, p, b):
    """p, b, c = (qx, qy, column) of Python integers: p beats b as the next vertex after c"""
    o = (b[0] - c[0]) * (p[1] - c[1]) - (b[1] - c[1]) * (p[0] - c[0])
    if o:
        return o < 0
    dp, db = (p[0] - c[0]) ** 2 + (p[1] - c[1]) ** 2, (b[0] - c[0]) ** 2 + (b[1] - c[1]) ** 2
    if dp != db:
        return dp > db
    return p[2] < b[2]


def hull(pts):
    """pts [(qx, qy, column)] of the present members -> ([the vertices' columns, all of them], area2)"""
    if not pts:
        return [], 0
    start = min(pts, key=lambda p: (p[1], p[0], p[2]))
    out, area2, c = [start[2]], 0, start
    for _ in range(len(pts)):
        best = None
        for p in pts:
            if (p[0], p[1]) != (c[0], c[1]) and (best is None or beats(c, p, best)):
                best = p
        if best is None or best[2] == start[2]:
            break
        area2 += (c[0] - start[0]) * (best[1] - start[1]) - (c[1] - start[1]) * (best[0] - start[0])
        out.append(best[2])
        c = best
    return out, area2


def row_points(values, cols, row):
    qx, qy, ok = quantise(values[cols, row, 0], values[cols, row, 1]) if len(cols) else (np.zeros(0, np.int64),) * 2 + (np.zeros(0, bool),)
    return [(int(qx[k]), int(qy[k]), int(c)) for k, c in enumerate(cols) if ok[k]]


def shape(values, columns, mapping):
    """values float64 [cols][rows][2] -> (SHAPE_DTYPE [rows, 2], int32 [rows, 2, HULL_CAP])"""
    groups = members(columns, mapping)
    rows = values.shape[1]
    rec, hl = np.zeros((rows, 2), SHAPE_DTYPE), np.full((rows, 2, HULL_CAP), -1, np.int32)
    for r in range(rows):
        for g in (0, 1):
            pts = row_points(values, groups[g], r)
            o = rec[r, g]
            o["n"] = len(pts)
            for k in ("col_min_x", "col_max_x", "col_min_y", "col_max_y"):
                o[k] = -1
            if not pts:
                continue
            o["sum_x"], o["sum_y"] = sum(p[0] for p in pts), sum(p[1] for p in pts)
            o["sum_xx"], o["sum_yy"] = sum(p[0] * p[0] for p in pts), sum(p[1] * p[1] for p in pts)
            for name, axis, pick in (("min_x", 0, min), ("max_x", 0, max), ("min_y", 1, min), ("max_y", 1, max)):
                v = pick(p[axis] for p in pts)
                o[name], o["col_" + name] = v, min(p[2] for p in pts if p[axis] == v)
            vs, area2 = hull(pts)
            o["hull_n"], o["area2"], o["flags"] = len(vs), area2, FLAG_CUT if len(vs) > HULL_CAP else 0
            hl[r, g, :min(len(vs), HULL_CAP)] = vs[:HULL_CAP]
    return rec, hl


# ---- the picture --------------------------------------------------------------------------------------------------------------------
def check_hull_params(half_width):
    if not 1 <= half_width <= 8:
        raise ValueError("hull half_width %r outside 1 .. 8" % (half_width,))


def hull_color(g):
    return tuple((ch * HULL_SHADE) >> 8 for ch in (A.RED if g == 0 else A.BLUE))


def edge_indices(hull_n, flags):
    """[(i, j)]: positions in the stored vertex list each edge joins"""
    k = min(hull_n, HULL_CAP)
    if hull_n < 2:
        return []
    if hull_n == 2:
        return [(0, 1)]
    return [(i, i + 1) for i in range(k - 1)] if flags & FLAG_CUT else [(i, (i + 1) % k) for i in range(k)]


def hull_edges(values, rec, hl, row, S, M):
    """-> [(ax, ay, bx, by, (b, g, r))] in drawing order for the picture of `row`"""
    out = []
    for g in (0, 1):
        for i, j in edge_indices(int(rec[row, g]["hull_n"]), int(rec[row, g]["flags"])):
            a, b = int(hl[row, g, i]), int(hl[row, g, j])
            ax, ay, oka = R.quantise(values[a, row, 0], values[a, row, 1], S, M)
            bx, by, okb = R.quantise(values[b, row, 0], values[b, row, 1], S, M)
            assert oka and okb                                  # (a vertex is present, and presence is the minimap's rule)
            out.append((int(ax), int(ay), int(bx), int(by), hull_color(g)))
    return out


def draw_row(values, frames, columns, mapping, row, S, M, layers=0, p=None, sel=(), owner=None, events=None, hull_hw=None, shape_result=None, voronoi=0, footprint=1,
             player_radius=0, ball_radius=0):
    """one table row -> BGR uint8 [h, w, 3]: trails_ref.draw_row's layers with 4.0, the hulls, between the markings and the trails"""
    w, h = R.size(S, M)
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
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
    if footprint:
        cs = R.corners(values, columns, row, S, M)
        if cs is not None:
            pick = R.footprint_mask(cs, S, M)
            img[pick] = R._blend(img[pick], A.WHITE, R.FOOT_A)
    img[R.markings(S, M)] = A.WHITE
    if layers & HULLS:
        rec, hl = shape_result
        T._draw_segments(img, hull_edges(values, rec, hl, row, S, M), 16 * hull_hw)
    hw16 = 16 * p["half_width"] if p is not None else 0
    if layers & T.TRAILS:
        T._draw_segments(img, T.trail_segments(values, frames, columns, mapping, sel, row, S, M, p), hw16)
    if layers & T.PASSES:
        for k in T.visible_events(events, row, p["pass_hold"]):
            arw = T.arrow(events[k], S, M, p["half_width"])
            if arw is not None:
                T._draw_arrow(img, arw, hw16, X, Y)
    entry_cols = T._entry_columns(values, columns, mapping, row, S, M)
    assert len(entry_cols) == len(lst)
    own = int(owner[row]) if (layers & T.OWNER and owner is not None) else -1
    to = max(1, r // 3)
    for (qx, qy, kind, color, _), c in zip(lst, entry_cols):
        d = (16 * X - qx) ** 2 + (16 * Y - qy) ** 2
        if kind == R.BALL:
            img[((16 * (rb - t)) ** 2 < d) & (d <= (16 * rb) ** 2)] = A.WHITE
            continue
        img[d <= (16 * r) ** 2] = color
        if c == own:
            img[((16 * r) ** 2 < d) & (d <= (16 * (r + to)) ** 2)] = A.WHITE
    return img


def frames_bgr(values, frames, columns, mapping, row0, n, S, M, layers=0, p=None, sel=(), owner=None, events=None, hull_hw=None, **kw):
    if layers & ~15:
        raise ValueError("unknown layer bits")
    if layers & 7:                                              # (trails_ref.check_layers knows three bits; its rules, restated for four)
        if p is None or (layers & T.TRAILS and not sel) or (layers & T.PASSES and events is None) or (layers & T.OWNER and owner is None):
            raise ValueError("a layer without its parameters, selection or possession result")
        T.check_trail_params(p)
    T.check_selection(sel, columns)
    res = None
    if layers & HULLS:
        check_hull_params(hull_hw)
        res = shape(values, columns, mapping)
    w, h = R.size(S, M)
    if not n:
        return np.zeros((0, h, w, 3), np.uint8)
    return np.stack([draw_row(values, frames, columns, mapping, row0 + i, S, M, layers, p, sel, owner, events, hull_hw, res, **kw) for i in range(n)])
