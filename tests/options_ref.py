"""numpy restatement of the library's pass-option contract (include/eagle.h, eagle_pass_options_* / eagle_op_pass_options; csrc/options.hip): a
processed table, its velocities and the possession arrays cand / owner -> per row a grid of how well a pass from the ball to each pitch cell would do,
the same figure for every teammate's own reaction point, and a row record.  It is the single written definition of every output bit; the kernels equal
it bit for bit.  It is held twice: bytes_at() is vectorised over any set of targets, byte_scalar() is an independent loop over one target with
np.float32 scalars.

PARITY UNPINNED, OWN SPEC.  The reference leaves the question to the analyst (examples/pass.py draws one pass between two hand-chosen rows).  The model
is a sampled pass lane over the time-to-intercept model of tests/control_ref.py; its constants (16 samples, t_react 0.7 s, v_max 5 m/s, beta 4 / s, a
15 m/s ball) are conventional choices, not fitted to data.

REUSED FROM control_ref, not restated: the cell centres (CR.centres), and per site the fp32 rounding of position and velocity, the non-finite-velocity
rule, the reaction point q = p + v t_react with its clamp to +-2^20 and the presence rule |x|, |y| <= 1024 (CR.sites, called on one column at a time).

Everything below is fp32, one operation at a time, no contraction, correctly rounded sqrt and division, d_expf of csrc/dmath.h (oracle.prims.expf).

SITE COLUMNS.  The Player pitch columns (video == 0) with a mapping entry >= 0, in table order; a negative entry is "unknown" and gives no site column;
goalkeepers are never sites.  group = 0 for team value 0, else 1.  n_sites counts them.  A column's site of a row is its cell when present within 1024 m.
The ball is the one Ball pitch column.

ROW STATUS, the first that applies: NO_OWNER owner[r] < 0; IN_FLIGHT cand[r] != owner[r]; NO_TEAM the owner's column is not a site column; OFF_DOMAIN the
ball cell is not within |x|, |y| <= 1024 (absent, or no ball column); ACTIVE.  A row that is not active: a grid of zeros, options all -1, best_col =
best_byte = -1, zero counts.  group is the owner's group whenever its column is a site column, else -1.

ACTIVE ROW.  b = the ball cell in fp32.  Attackers: the sites of the owner's group except the owner's own column; defenders: the sites of the other group.
For a target c: dx = cx - bx, dy = cy - by, L = sqrtf(dx dx + dy dy).  For k = 1 .. K: f_k = (float)k / (float)K, s_k = (bx + dx f_k, by + dy f_k),
T_k = (L f_k) / v_ball.  t_D(s) = t_react + sqrtf(min over defenders of ex ex + ey ey) / v_max with ex = sx - qx, ey = sy - qy; t_A(s) the same over
attackers; every min starts from FLT_MAX.  m = min over k = 1 .. K - 1 of (t_D(s_k) - T_k); safety = 1 / (1 + expf(-(beta m))), 1.0 when K = 1.
reach = 1 / (1 + expf(-(beta (t_D(s_K) - t_A(s_K))))), at s_K as computed (not at c).  Without defenders safety = reach = 1.0.
byte = (int)floorf(safety reach 255 + 0.5); 0 without attackers.

OUTPUTS per row: GRID u8 [gh][gw], the byte at every cell centre (grid row 0 is pitch y = 0); OPTIONS int16 [n_sites], for a present attacker the byte
at target c = q_i, everything else -1; the record ROW_DTYPE: best_col / best_byte the largest option (a tie: the earlier column), sum the sum of the
row's grid bytes (0 when no grid was asked for)."""
import numpy as np

import control_ref as CR
import minimap_ref as MR
from oracle import prims

F = np.float32
FLT_MAX = np.finfo(F).max
ACTIVE, NO_OWNER, IN_FLIGHT, NO_TEAM, OFF_DOMAIN = 0, 1, 2, 3, 4
MAX_SITES = 1024
SAMPLES, T_REACT, V_MAX, BETA, V_BALL = 16, CR.T_REACT, CR.V_MAX, CR.BETA, 15.0        # conventional choices, not fitted to data
ROW_DTYPE = np.dtype([("status", "<i4"), ("owner_col", "<i4"), ("group", "<i4"), ("n_mates", "<i4"), ("n_defenders", "<i4"), ("best_col", "<i4"),
                      ("best_byte", "<i4"), ("reserved", "<i4"), ("sum", "<i8")])       # EaglePassOptionRow (40 bytes)


def params(R=1, K=SAMPLES, t_react=T_REACT, v_max=V_MAX, beta=BETA, v_ball=V_BALL):
    assert R in CR.RS and 1 <= K <= 64
    return {"R": R, "K": K, "t_react": t_react, "v_max": v_max, "beta": beta, "v_ball": v_ball}


def site_columns(columns, mapping):
    """-> [(table column, group)] in table order"""
    assert mapping is not None
    return [(c, 0 if int(mapping[ident]) == 0 else 1) for c, (kind, ident, video) in enumerate(columns)
            if not video and kind == MR.PLAYER and ident in mapping and int(mapping[ident]) >= 0]


def ball_column(columns):
    b = [c for c, (kind, ident, video) in enumerate(columns) if kind == MR.BALL and not video]
    assert len(b) <= 1
    return b[0] if b else -1


def _q(values, vel, columns, c, row, t_react):
    """the reaction point of column c on the row, or None when it has no site there: control_ref's rules on the one column"""
    q, _ = CR.sites(values[c:c + 1], vel[c:c + 1], [(MR.PLAYER, columns[c][1], 0)], {columns[c][1]: 0}, row, t_react)
    return q[0] if len(q) else None


def row_state(values, vel, columns, mapping, cand, owner, row, t_react=T_REACT):
    """-> {"status", "owner_col", "group", "b" float32 [2], "A" float32 [nA, 2], "A_site" [nA] site indices, "D" float32 [nD, 2]}"""
    sc = site_columns(columns, mapping)
    o, cd = int(owner[row]), int(cand[row])
    group = dict(sc).get(o, -1)
    bc = ball_column(columns)
    x, y = values[bc, row] if bc >= 0 else (np.nan, np.nan)
    ball = bool(abs(x) <= MR.DOMAIN and abs(y) <= MR.DOMAIN)                  # (False for NaN)
    status = NO_OWNER if o < 0 else IN_FLIGHT if cd != o else NO_TEAM if group < 0 else OFF_DOMAIN if not ball else ACTIVE
    st = {"status": status, "owner_col": o, "group": group, "b": np.zeros(2, F), "A": np.zeros((0, 2), F), "A_site": [], "D": np.zeros((0, 2), F)}
    if status != ACTIVE:
        return st
    st["b"] = np.array([x, y], np.float64).astype(F)
    A, D = [], []
    for s, (c, g) in enumerate(sc):
        if c == o:
            continue
        q = _q(values, vel, columns, c, row, t_react)
        if q is None:
            continue
        if g == group:
            A.append(q); st["A_site"].append(s)
        else:
            D.append(q)
    st["A"], st["D"] = np.array(A, F).reshape(-1, 2), np.array(D, F).reshape(-1, 2)
    return st


# ---- formulation 1: vectorised over the targets --------------------------------------------------------------------------------------------------
def _min_d2(sx, sy, Q):
    best = np.full(sx.shape, FLT_MAX, F)
    for qx, qy in Q:
        ex, ey = sx - qx, sy - qy
        best = np.minimum(best, ex * ex + ey * ey)
    return best


def _sigmoid_of(x):
    return F(1.0) / (F(1.0) + prims.expf(-x).reshape(x.shape))


def bytes_at(b, A, D, cx, cy, K=SAMPLES, t_react=T_REACT, v_max=V_MAX, beta=BETA, v_ball=V_BALL, **_):
    """the bytes of the targets (cx, cy) (float32 arrays of one shape) of an active row -> int32 array of that shape"""
    cx, cy = np.asarray(cx, F), np.asarray(cy, F)
    if len(A) == 0:
        return np.zeros(cx.shape, np.int32)
    if len(D) == 0:
        return np.full(cx.shape, 255, np.int32)
    tr, vm, be, vb, bx, by = F(t_react), F(v_max), F(beta), F(v_ball), F(b[0]), F(b[1])
    with np.errstate(all="ignore"):
        dx, dy = cx - bx, cy - by
        L = np.sqrt(dx * dx + dy * dy)
        lane = np.full(cx.shape, FLT_MAX, F)
        for k in range(1, K + 1):
            f = F(k) / F(K)
            sx, sy = bx + dx * f, by + dy * f
            tD = tr + np.sqrt(_min_d2(sx, sy, D)) / vm
            if k < K:
                lane = np.minimum(lane, tD - (L * f) / vb)
        tA = tr + np.sqrt(_min_d2(sx, sy, A)) / vm                        # (sx, sy, tD: those of k = K)
        reach = _sigmoid_of(be * (tD - tA))
        safety = np.ones(cx.shape, F) if K == 1 else _sigmoid_of(be * lane)
        v = np.floor(safety * reach * F(255.0) + F(0.5))
    assert v.dtype == F and v.min() >= 0 and v.max() <= 255
    return v.astype(np.int32)


# ---- formulation 2: one target, scalar by scalar ---------------------------------------------------------------------------------------------------
def _expf1(x):
    return F(prims.expf(np.array([x], F)).reshape(-1)[0])


def byte_scalar(b, A, D, cx, cy, K=SAMPLES, t_react=T_REACT, v_max=V_MAX, beta=BETA, v_ball=V_BALL, **_):
    if len(A) == 0:
        return 0
    tr, vm, be, vb, bx, by, cx, cy = F(t_react), F(v_max), F(beta), F(v_ball), F(b[0]), F(b[1]), F(cx), F(cy)
    one = F(1.0)

    def t_of(sx, sy, Q):
        best = F(FLT_MAX)
        for q in Q:
            ex = F(sx - F(q[0])); ey = F(sy - F(q[1]))
            d2 = F(F(ex * ex) + F(ey * ey))
            if d2 < best:
                best = d2
        return F(tr + F(F(np.sqrt(best)) / vm))

    with np.errstate(all="ignore"):
        if len(D) == 0:
            safety = reach = one
        else:
            dx = F(cx - bx); dy = F(cy - by)
            L = F(np.sqrt(F(F(dx * dx) + F(dy * dy))))
            m = F(FLT_MAX)
            for k in range(1, K):
                f = F(F(k) / F(K))
                sx = F(bx + F(dx * f)); sy = F(by + F(dy * f))
                v = F(t_of(sx, sy, D) - F(F(L * f) / vb))
                if v < m:
                    m = v
            safety = one if K == 1 else F(one / F(one + _expf1(F(-F(be * m)))))
            f = F(F(K) / F(K))
            sx = F(bx + F(dx * f)); sy = F(by + F(dy * f))
            reach = F(one / F(one + _expf1(F(-F(be * F(t_of(sx, sy, D) - t_of(sx, sy, A)))))))
        return int(np.floor(F(F(F(safety * reach) * F(255.0)) + F(0.5))))


def centre(i, j, R):
    return F(F(F(i) + F(0.5)) / F(R)), F(F(F(j) + F(0.5)) / F(R))


# ---- rows -------------------------------------------------------------------------------------------------------------------------------------------
def row(values, vel, columns, mapping, cand, owner, r, p, grid=True):
    """-> (uint8 [gh, gw], int16 [n_sites], ROW_DTYPE record) of table row r"""
    gw, gh = CR.size(p["R"])
    sc = site_columns(columns, mapping)
    st = row_state(values, vel, columns, mapping, cand, owner, r, p["t_react"])
    g = np.zeros((gh, gw), np.uint8)
    opt = np.full(len(sc), -1, np.int16)
    rec = np.zeros((), ROW_DTYPE)
    rec["status"], rec["owner_col"], rec["group"], rec["best_col"], rec["best_byte"] = st["status"], st["owner_col"], st["group"], -1, -1
    if st["status"] == ACTIVE:
        rec["n_mates"], rec["n_defenders"] = len(st["A"]), len(st["D"])
        if grid:
            cx, cy = CR.centres(p["R"])
            g = bytes_at(st["b"], st["A"], st["D"], cx, cy, **p).astype(np.uint8)
        if len(st["A"]):
            opt[st["A_site"]] = bytes_at(st["b"], st["A"], st["D"], st["A"][:, 0], st["A"][:, 1], **p)
            s = int(np.argmax(opt))                                        # (the first of the largest: the earlier column)
            rec["best_col"], rec["best_byte"] = sc[s][0], opt[s]
    rec["sum"] = int(g.astype(np.int64).sum()) if grid else 0
    return g, opt, rec


def rows(values, vel, columns, mapping, cand, owner, row0, n, p, grid=True):
    """-> (uint8 [n, gh, gw], ROW_DTYPE [n], int16 [n, n_sites])"""
    gw, gh = CR.size(p["R"])
    ns = len(site_columns(columns, mapping))
    out = [row(values, vel, columns, mapping, cand, owner, row0 + i, p, grid) for i in range(n)]
    g = np.stack([o[0] for o in out]) if n else np.zeros((0, gh, gw), np.uint8)
    opt = np.stack([o[1] for o in out]).reshape(n, ns) if n else np.zeros((0, ns), np.int16)
    rec = np.array([o[2] for o in out], ROW_DTYPE) if n else np.zeros(0, ROW_DTYPE)
    return g, rec, opt


# ---- what eagle_amd/options.py derives per PASS event ---------------------------------------------------------------------------------------------------
def event_figures(ev, site_cols, recs, options, row0=0):
    """ev: a possession event (mapping with from_col, to_col, release_row); recs / options: the rows row0 .. of the table -> (chosen, best_byte, best_col,
    rank), (-1, -1, -1, -1) when the release row is not ACTIVE, its owner is not from_col, or to_col has no option there"""
    r = int(ev["release_row"]) - row0
    none = (-1, -1, -1, -1)
    if not 0 <= r < len(recs) or recs[r]["status"] != ACTIVE or recs[r]["owner_col"] != int(ev["from_col"]) or int(ev["to_col"]) not in list(site_cols):
        return none
    chosen = int(options[r][list(site_cols).index(int(ev["to_col"]))])
    if chosen < 0:
        return none
    return chosen, int(recs[r]["best_byte"]), int(recs[r]["best_col"]), 1 + int((options[r] > chosen).sum())
