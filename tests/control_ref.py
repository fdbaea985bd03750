"""numpy restatement of the library's kinematics and pitch-control contract (include/eagle.h, eagle_post_velocities / eagle_control_* /
eagle_op_velocities / eagle_op_control / eagle_op_minimap_control; csrc/post.hip, csrc/control.hip): a processed table -> per-cell velocities, and
per row a grid of the share of each pitch cell that team 0 reaches first.  It is the single written definition of every output bit; the kernels
equal it bit for bit.

PARITY UNPINNED, OWN SPEC.  The reference derives neither.  The model is the common exponential "time to intercept" softmin; its constants
(t_react, v_max, beta, the speed cap) are conventional choices, not fitted to data.

Velocities, float64, no contraction, for every column (video columns come out in px/s).  values[c][r] = (x, y), frames f[r] strictly ascending,
fps > 0, max_gap >= 1 (frames), speed_cap > 0.  A cell is PRESENT when x and y are both finite.  For a present cell a = r - 1 is usable when it
is present and f[r] - f[a] <= max_gap; b = r + 1 by the same rule.  Both usable: v = (p[b] - p[a]) / ((f[b] - f[a]) / fps); one usable: the
one-sided difference against p[r]; none: (0, 0); an absent cell: (NaN, NaN).  Then s = sqrt(vx vx + vy vy); s > speed_cap multiplies both
components by speed_cap / s.  Every operation is one IEEE float64 operation in the order written.

Control grid, float32, no contraction, one grid per row.  R in {1, 2, 4} cells per metre, gw = 105 R, gh = 68 R; cell (i, j) has its centre
at ((i + 0.5) / R, (j + 0.5) / R) (exact); grid row 0 is pitch y = 0.  SITES: the row's drawn PLAYER entries exactly as minimap_ref.draw_list
selects Voronoi sites (pitch columns in table order, present, |x|, |y| <= 1024, with a team-mapping entry; goalkeepers are not sites; a
mapping is required); team 0 against every other team.  Per site: position and velocity rounded to fp32 once, a velocity component that is
then not finite (NaN, or beyond fp32) counts as 0; the reaction point q = p + v * t_react, each component clamped to +-2^20 (so every later
value is finite for the parameter ranges the library accepts); arrival time at a cell t_i = t_react + sqrtf(dx dx + dy dy) / v_max with
dx = cx - qx, dy = cy - qy.  Per cell: t_min = min_i t_i, w_i = d_expf(-beta * (t_i - t_min)) (csrc/dmath.h; here oracle.prims.expf), num =
the sum of w_i over team-0 sites and den = the sum over all sites, both from 0 in table order (den >= 1), and the cell's byte is
(int) floorf(num / den * 255 + 0.5).  A row without sites: 128 everywhere.  Team-0 area share of a row: the sum of its bytes (exact int64),
divided on the host by 255 gw gh.

(sqrtf, the division and the addition are monotone, so t_min is the t of the smallest dx dx + dy dy: the kernel's first pass keeps that.)

Minimap layer `control`: in Voronoi's slot (layer 2), refused together with voronoi.  A pixel (X, Y) of the pitch rectangle reads cell
i = ((X - M) R) / S, j = gh - 1 - ((Y - M) R) / S (integer divisions); with a = c + (c >> 7) its colour per channel is
(RED a + BLUE (256 - a) + 128) >> 8, tinted over the background with Voronoi's formula and TINT_A.  Everything else is minimap_ref.draw_row."""
import numpy as np

import annot_ref as A
import minimap_ref as MR
from oracle import prims

F = np.float32
T_REACT, V_MAX, BETA, SPEED_CAP = 0.7, 5.0, 4.0, 12.0
Q_LIM = F(1048576.0)
RS = (1, 2, 4)


def size(R):
    assert R in RS, R
    return 105 * R, 68 * R


# ---- velocities -----------------------------------------------------------------------------------------------------------------------
def velocities(values, frames, fps, max_gap=None, speed_cap=SPEED_CAP):
    """values float64 [cols][rows][2], frames int [rows] -> float64 [cols][rows][2]"""
    values = np.asarray(values, np.float64)
    f = np.asarray(frames, np.int64)
    cols, rows = values.shape[:2]
    max_gap = int(fps) if max_gap is None else int(max_gap)
    assert fps > 0 and max_gap >= 1 and speed_cap > 0 and len(f) == rows and (np.diff(f) > 0).all()
    out = np.full((cols, rows, 2), np.nan, np.float64)
    if rows == 0 or cols == 0:
        return out
    present = np.isfinite(values).all(2)                                        # [cols][rows]
    ua = np.zeros((cols, rows), bool)
    ub = np.zeros((cols, rows), bool)
    near = (np.diff(f) <= max_gap)[None, :]
    ua[:, 1:] = present[:, 1:] & present[:, :-1] & near
    ub[:, :-1] = present[:, :-1] & present[:, 1:] & near
    fps64 = np.float64(fps)
    with np.errstate(all="ignore"):
        for c in range(cols):
            for r in range(rows):
                if not present[c, r]:
                    continue
                lo = r - 1 if ua[c, r] else r
                hi = r + 1 if ub[c, r] else r
                if lo == hi:
                    v = np.zeros(2, np.float64)
                else:
                    dt = np.float64(f[hi] - f[lo]) / fps64
                    v = (values[c, hi] - values[c, lo]) / dt
                s = np.sqrt(v[0] * v[0] + v[1] * v[1])
                if s > speed_cap:
                    k = np.float64(speed_cap) / s
                    v = v * k
                out[c, r] = v
    return out


def kinematics(values, vel, frames, columns, fps, max_gap=None):
    """the host summary of eagle_amd/control.py: per pitch Player / Goalkeeper column {"id", "type", "distance", "top_speed"}"""
    f = np.asarray(frames, np.int64)
    max_gap = int(fps) if max_gap is None else int(max_gap)
    out = []
    for c, (kind, ident, video) in enumerate(columns):
        if video or kind not in (MR.PLAYER, MR.GOALKEEPER):
            continue
        sp = np.sqrt(vel[c, :, 0] ** 2 + vel[c, :, 1] ** 2)
        ok = np.isfinite(sp)
        step = ok[1:] & ok[:-1] & (np.diff(f) <= max_gap)
        dist = float(np.sum(0.5 * (sp[1:] + sp[:-1])[step] * (np.diff(f)[step] / float(fps)))) if len(f) > 1 else 0.0
        out.append({"id": int(ident), "type": "Player" if kind == MR.PLAYER else "Goalkeeper", "distance": dist, "top_speed": float(sp[ok].max()) if ok.any() else 0.0})
    return out


# ---- the control grid -------------------------------------------------------------------------------------------------------------------
def sites(values, vel, columns, team_mapping, row, t_react=T_REACT):
    """-> (q float32 [n, 2], team0 bool [n]) of the row's sites in table order"""
    assert team_mapping is not None
    q, team = [], []
    tr = F(t_react)
    for c, (kind, ident, video) in enumerate(columns):
        if video or kind != MR.PLAYER or ident not in team_mapping:
            continue
        x, y = values[c, row]
        if not (np.isfinite(x) and np.isfinite(y) and abs(x) <= MR.DOMAIN and abs(y) <= MR.DOMAIN):
            continue
        with np.errstate(all="ignore"):
            p = np.array([x, y], np.float64).astype(F)
            v = np.asarray(vel[c, row], np.float64).astype(F)
            v = np.where(np.isfinite(v), v, F(0))
            qq = np.minimum(np.maximum(p + v * tr, -Q_LIM), Q_LIM)
        q.append(qq)
        team.append(int(team_mapping[ident]) == 0)
    return np.array(q, F).reshape(-1, 2), np.array(team, bool)


def centres(R):
    gw, gh = size(R)
    cx = (np.arange(gw, dtype=F) + F(0.5)) / F(R)
    cy = (np.arange(gh, dtype=F) + F(0.5)) / F(R)
    return np.broadcast_to(cx[None, :], (gh, gw)), np.broadcast_to(cy[:, None], (gh, gw))


def grid_of_sites(q, team0, R, t_react=T_REACT, v_max=V_MAX, beta=BETA):
    """sites -> uint8 [gh, gw]"""
    gw, gh = size(R)
    if len(q) == 0:
        return np.full((gh, gw), 128, np.uint8)
    cx, cy = centres(R)
    tr, vm, nb = F(t_react), F(v_max), -F(beta)
    ts = []
    for qx, qy in q:
        dx, dy = cx - qx, cy - qy
        ts.append(tr + np.sqrt(dx * dx + dy * dy) / vm)
    t_min = ts[0]
    for t in ts[1:]:
        t_min = np.minimum(t_min, t)
    num, den = np.zeros((gh, gw), F), np.zeros((gh, gw), F)
    for t, is0 in zip(ts, team0):
        w = prims.expf(nb * (t - t_min)).reshape(gh, gw)
        den = den + w
        if is0:
            num = num + w
    c = np.floor(num / den * F(255.0) + F(0.5))
    assert c.dtype == F and c.min() >= 0 and c.max() <= 255
    return c.astype(np.int32).astype(np.uint8)


def grid(values, vel, columns, team_mapping, row, R, t_react=T_REACT, v_max=V_MAX, beta=BETA):
    q, team0 = sites(values, vel, columns, team_mapping, row, t_react)
    return grid_of_sites(q, team0, R, t_react, v_max, beta)


def grids(values, vel, columns, team_mapping, row0, n, R, **kw):
    """-> (uint8 [n, gh, gw], int64 [n]: the sums of the bytes)"""
    gw, gh = size(R)
    g = np.stack([grid(values, vel, columns, team_mapping, row0 + i, R, **kw) for i in range(n)]) if n else np.zeros((0, gh, gw), np.uint8)
    return g, g.reshape(n, -1).astype(np.int64).sum(1)


def share(sums, R):
    gw, gh = size(R)
    return np.asarray(sums, np.float64) / float(255 * gw * gh)


# ---- the minimap layer --------------------------------------------------------------------------------------------------------------------
def layer_colors(g, R, S, M):
    """a row's grid -> (BGR uint8 [68 S, 105 S, 3]: the untinted colour of every pixel of the pitch rectangle)"""
    gw, gh = size(R)
    Y, X = np.mgrid[0:68 * S, 0:105 * S].astype(np.int64)                     # (X - M, Y - M) of the canvas
    c = g[gh - 1 - (Y * R) // S, (X * R) // S].astype(np.int64)
    a = c + (c >> 7)
    red, blue = np.asarray(A.RED, np.int64), np.asarray(A.BLUE, np.int64)
    return ((red[None, None] * a[..., None] + blue[None, None] * (256 - a[..., None]) + 128) >> 8).astype(np.uint8)


def draw_row(values, vel, columns, team_mapping, row, S, M, R, control_kw=None, **kw):
    """minimap_ref.draw_row with the control layer in Voronoi's slot.  The layers above it never read what is below them except the footprint's
    blend, so the row is drawn as the contract's plain row and every pixel the later layers left as "background or footprint over black" is redone."""
    assert not kw.get("voronoi", 0)
    w, h = MR.size(S, M)
    g = grid(values, vel, columns, team_mapping, row, R, **(control_kw or {}))
    base = np.zeros((h, w, 3), np.uint8)
    rect = base[M:M + 68 * S, M:M + 105 * S]
    rect[:] = MR._blend(rect, layer_colors(g, R, S, M), MR.TINT_A)
    img = base.copy()
    under = np.zeros((h, w, 3), np.uint8)                                       # layers 1 + 3 of the plain row
    cs = MR.corners(values, columns, row, S, M) if kw.get("footprint", 1) else None
    if cs is not None:
        sel = MR.footprint_mask(cs, S, M)
        img[sel] = MR._blend(img[sel], A.WHITE, MR.FOOT_A)
        under[sel] = MR._blend(under[sel], A.WHITE, MR.FOOT_A)
    # layers 4 .. 6 overwrite what is below them: they are taken from the plain row
    plain = MR.draw_row(values, columns, team_mapping, row, S, M, **kw)
    over = _overwritten(values, columns, team_mapping, row, S, M, kw)
    img[over] = plain[over]
    assert np.array_equal(plain[~over], under[~over])
    return img


def _overwritten(values, columns, team_mapping, row, S, M, kw):
    """bool [h, w]: the pixels layers 4 .. 6 (markings, discs, rings) write"""
    w, h = MR.size(S, M)
    r, rb, t = MR.radii(S, kw.get("player_radius", 0), kw.get("ball_radius", 0))
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    m = MR.markings(S, M).copy()
    for qx, qy, kind, color, _ in MR.draw_list(values, columns, team_mapping, row, S, M):
        d = (16 * X - qx) ** 2 + (16 * Y - qy) ** 2
        m |= (((16 * (rb - t)) ** 2 < d) & (d <= (16 * rb) ** 2)) if kind == MR.BALL else (d <= (16 * r) ** 2)
    return m


def frames_bgr(values, vel, columns, team_mapping, row0, n, S, M, R, **kw):
    w, h = MR.size(S, M)
    return np.stack([draw_row(values, vel, columns, team_mapping, row0 + i, S, M, R, **kw) for i in range(n)]) if n else np.zeros((0, h, w, 3), np.uint8)


def minimap(values, vel, columns, team_mapping, row0, n, S, M, R, fmt=A.BGR, layout=None, fill=0, **kw):
    fr = frames_bgr(values, vel, columns, team_mapping, row0, n, S, M, R, **kw)
    return A.annotate(fr, [[] for _ in range(n)], fmt, layout, fill)
