"""Constructed tables for the pass-option entries (include/eagle.h eagle_op_pass_options; contract: tests/options_ref.py): values float64
[cols][rows][2], velocities (the contract's own, tests/control_ref.py, or handed in), the column descriptors (kind, id, video), the team mapping and the
possession arrays cand / owner, chosen for the seams of the kernels and of the contract, not for the workload.  A grid is 105 R x 68 R cells = 7140 R^2
bytes: 7 workgroups of 1024 cells at R = 1 (the last one partly idle), 28 at R = 2, 112 at R = 4.  The lists of a row are staged in LDS in rounds of 256
entries: 257 sites in one group cross one round, 1024 sites in total fill the staging; 1025 site columns are refused.  The row counts 65 and 257 cross a
wave and a 256-row block of the per-row kernels.  The large site counts stay at R = 1, one row and K = 2 so that the reference stays cheap.  Every case
lists the parameter sets it is run with ("variants"); reference(name, i) is computed once and shared."""
import functools

import numpy as np

import control_ref as CR
import minimap_ref as MR
import options_ref as OR

P, G, BALL, BND = MR.PLAYER, MR.GOALKEEPER, MR.BALL, MR.BOUNDARY
NAN, INF = float("nan"), float("inf")
BOUNDS = [(BND, k, 0) for k in range(4)]


def table(columns, rows):
    return np.full((len(columns), rows, 2), NAN, np.float64)


def _case(name, values, columns, mapping, cand, owner, variants, vel=None, frames=None, fps=5, row0=0, n=None):
    rows = values.shape[1]
    frames = np.arange(rows, dtype=np.int32) if frames is None else np.asarray(frames, np.int32)
    if vel is None:
        vel = CR.velocities(values, frames, fps)
    cand, owner = np.asarray(cand, np.int32), np.asarray(owner, np.int32)
    assert cand.shape == owner.shape == (rows,) and vel.shape == values.shape
    return {"name": name, "values": values, "vel": vel, "columns": columns, "mapping": mapping, "cand": cand, "owner": owner, "variants": variants,
            "row0": row0, "n": rows - row0 if n is None else n}


def col_of(columns, ident, kind=P):
    return columns.index((kind, ident, 0))


def walkers(name, count, rows, seed, variants, teams=2, step=0.4, **kw):
    """`count` mapped players on a random walk (present on every row), a video column after each, a goalkeeper and a ball that sits near one player per
    row; the owner of a row is that player on most rows, nobody or somebody else (the ball in flight) on the others"""
    r = np.random.default_rng(seed)
    cols = BOUNDS + [c for i in range(count) for c in ((P, i + 1, 0), (P, i + 1, 1))] + [(G, 900, 0), (BALL, 0, 0), (BALL, 0, 1)]
    v = table(cols, rows)
    pos = np.stack([r.uniform(0, 105, count), r.uniform(0, 68, count)], 1)
    cand, owner = np.full(rows, -1, np.int32), np.full(rows, -1, np.int32)
    for row in range(rows):
        pos = pos + r.normal(0, step, pos.shape)
        v[4:4 + 2 * count:2, row] = pos
        v[5:5 + 2 * count:2, row] = pos * 12.0 + r.normal(0, 3.0, pos.shape)                 # a video point: never a site
        k = int(r.integers(count))
        v[-3, row], v[-2, row], v[-1, row] = (3.0, 34.0 + 0.1 * row), pos[k] + r.normal(0, 0.5, 2), (640.0, 360.0)
        kind = row % 7
        cand[row] = 4 + 2 * k
        owner[row] = -1 if kind == 3 else 4 + 2 * int(r.integers(count)) if kind == 5 else cand[row]
        if kind == 6:
            cand[row] = -1
    return _case(name, v, cols, {i + 1: i % teams for i in range(count)}, cand, owner, variants, **kw)


def crowd(name, n0, n1, seed, variants):
    """one row: n0 players of team 0 (the first owns the ball) and n1 of team 3, alternating in table order while both last"""
    r = np.random.default_rng(seed)
    ids = []
    a, b = list(range(1, n0 + 1)), list(range(5001, 5001 + n1))
    while a or b:
        if a:
            ids.append(a.pop(0))
        if b:
            ids.append(b.pop(0))
    cols = [(BALL, 0, 0)] + [(P, i, 0) for i in ids]
    v = table(cols, 1)
    v[1:, 0] = np.stack([r.uniform(0, 105, len(ids)), r.uniform(0, 68, len(ids))], 1)
    o = col_of(cols, 1)
    v[0, 0] = v[o, 0] + (0.5, -0.25)
    vel = np.zeros_like(v)
    vel[1:, 0] = r.normal(0, 2.0, (len(ids), 2))
    return _case(name, v, cols, {i: (0 if i <= 5000 else 3) for i in ids}, [o], [o], variants, vel=vel)


V1 = [OR.params(1)]


def _cases():
    out = []
    # 0, 1 and 2 sites on consecutive rows: the owner's column is a site column, so the rows are active; an owner alone has no attackers (bytes 0)
    cols = BOUNDS + [(P, 1, 0), (P, 1, 1), (P, 2, 0), (G, 3, 0), (BALL, 0, 0)]
    v = table(cols, 3)
    v[4, 1], v[4, 2], v[6, 2], v[7, :], v[8, :] = (30.0, 20.0), (31.5, 21.0), (70.0, 50.0), (5.0, 34.0), (31.0, 20.5)
    v[5, :] = (400.0, 300.0)
    out.append(_case("sites_0_1_2", v, cols, {1: 0, 2: 1}, [4, 4, 4], [4, 4, 4], V1, frames=[3, 4, 6]))
    # no defenders: 255 wherever there is a teammate, options 255 (also with team values other than 0: group 1 owns the ball)
    cols = BOUNDS + [(P, 1, 0), (P, 2, 0), (P, 3, 0), (BALL, 0, 0)]
    v = table(cols, 2)
    v[4, :], v[5, :], v[6, :], v[7, :] = (10.0, 10.0), (60.0, 40.0), (100.0, 60.0), (10.5, 10.0)
    v[5, 1] = (61.0, 40.5)
    out.append(_case("no_defenders", v, cols, {1: 0, 2: 0, 3: 0}, [4, 5], [4, 5], V1))
    out.append(_case("no_defenders_group1", v, cols, {1: 1, 2: 7, 3: 1}, [4, 5], [4, 5], V1))
    # the workload's shape; every K and every R
    out.append(walkers("sites22", 22, 3, 0, [OR.params(1, K) for K in (16, 1, 2, 3, 64)] + [OR.params(2), OR.params(4, 3)]
                       + [OR.params(1, 5, t_react=0.25, v_max=7.5, beta=2.5, v_ball=22.0)]))
    out.append(crowd("sites257_one_group", 3, 257, 13, [OR.params(1, 2)]))
    out.append(crowd("sites1024", 512, 512, 14, [OR.params(1, 2)]))
    out.append(crowd("sites1025", 512, 513, 15, []))                                   # refused: no variant
    out.append(walkers("row1", 5, 1, 4, V1))
    out.append(walkers("rows65", 5, 65, 5, [OR.params(1, 3)], step=0.25))
    out.append(walkers("rows65_window", 5, 65, 5, [OR.params(1, 3)], step=0.25, row0=3, n=59))
    out.append(walkers("rows257", 4, 257, 6, [OR.params(1, 2)], step=0.1))

    # every row status, interleaved on consecutive rows
    cols = BOUNDS + [(P, 1, 0), (P, 2, 0), (P, 3, 0), (P, 4, 0), (P, 5, 0), (G, 6, 0), (P, 7, 0), (BALL, 0, 0), (BALL, 0, 1)]
    mapping = {1: 0, 2: 0, 3: 1, 5: -1, 6: 0, 7: 1}                                      # player 4: no entry; player 5: unknown; the goalkeeper is mapped
    c1, c3, c4, c5, c6, cb = [col_of(cols, i) for i in (1, 3, 4, 5)] + [col_of(cols, 6, G), col_of(cols, 0, BALL)]
    st = [(c1, c1, (30.5, 20.0), OR.ACTIVE), (-1, -1, (30.5, 20.0), OR.NO_OWNER), (-1, c1, (35.0, 22.0), OR.IN_FLIGHT), (c3, c1, (40.0, 24.0), OR.IN_FLIGHT),
          (c6, c6, (6.0, 34.0), OR.NO_TEAM), (c3, c3, (50.0, 30.0), OR.ACTIVE), (c4, c4, (60.0, 20.0), OR.NO_TEAM), (c5, c5, (20.0, 50.0), OR.NO_TEAM),
          (c1, c1, (1024.0, -1024.0), OR.ACTIVE), (c1, c1, (np.nextafter(1024.0, 2000.0), 0.0), OR.OFF_DOMAIN), (c1, c1, (0.0, -1025.0), OR.OFF_DOMAIN),
          (c1, c1, (NAN, 20.0), OR.OFF_DOMAIN), (c1, -1, (30.0, 20.0), OR.NO_OWNER), (c1, c1, (-1024.0, 1024.0), OR.ACTIVE)]
    v = table(cols, len(st))
    for r, (cd, ow, ball, _) in enumerate(st):
        v[4:4 + 7, r] = [(30.0 + 0.3 * r, 20.0), (55.0, 40.0 - 0.2 * r), (50.0, 30.0 + 0.1 * r), (60.0, 20.0), (20.0, 50.0), (5.0, 34.0), (70.0 - 0.25 * r, 45.0)]
        v[cb, r], v[cb + 1, r] = ball, (640.0, 360.0)
    case = _case("statuses", v, cols, mapping, [s[0] for s in st], [s[1] for s in st], V1)
    case["status"] = [s[3] for s in st]
    out.append(case)

    # lane and target geometry (velocities all zero: q = p).  b = (20.5, 34.5) is the centre of cell (20, 34): that target has L = 0
    cols = [(BALL, 0, 0), (P, 1, 0), (P, 2, 0), (P, 3, 0), (P, 11, 0), (P, 12, 0)]
    mapping = {1: 0, 2: 0, 3: 0, 11: 1, 12: 1}
    v = table(cols, 4)
    v[0, :], v[1, :] = (20.5, 34.5), (20.0, 34.0)
    # row 0: a defender exactly on sample 8 of 16 of the lane to teammate 2 (dx = 32: every f_k dx is exact); teammate 3 is as far away, off that lane
    v[2, 0], v[3, 0], v[4, 0] = (52.5, 34.5), (20.5, 66.5), (36.5, 34.5)
    # row 1: a defender at b
    v[2, 1], v[3, 1], v[4, 1], v[5, 1] = (52.5, 34.5), (40.0, 60.0), (20.5, 34.5), (80.0, 10.0)
    # row 2: two teammates mirrored about the lane axis, the one defender on it: equal bytes, best_col is the earlier column
    v[2, 2], v[3, 2], v[4, 2] = (40.5, 44.5), (40.5, 24.5), (30.5, 34.5)
    # row 3: a teammate 1 km away and a defender on the pitch: near the defender -(beta (t_D - t_A)) passes 88, at the teammate it passes -87
    v[2, 3], v[4, 3] = (1020.5, 34.5), (50.5, 34.5)
    o = col_of(cols, 1)
    out.append(_case("geometry", v, cols, mapping, [o] * 4, [o] * 4, V1, vel=np.zeros_like(v)))

    # velocities handed in: finite in fp32 but enormous (q is clamped to +-2^20), beyond fp32 and NaN (count as 0), and an ordinary one; with
    # t_react = 1000 s the ordinary one lands 12 km away, inside the clamp (control_cases.given_velocities' idea)
    cols = [(P, i + 1, 0) for i in range(6)] + [(BALL, 0, 0)]
    v = table(cols, 1)
    v[:, 0] = [(20.0, 30.0), (80.0, 30.0), (50.0, 10.0), (50.0, 60.0), (30.0, 50.0), (70.0, 40.0), (20.5, 30.0)]
    vel = np.zeros_like(v)
    vel[:6, 0] = [(0.5, 0.5), (1e39, -1e300), (NAN, INF), (12.0, 0.0), (-3.0e38, 2.0), (1e30, -1e30)]
    out.append(_case("given_velocities", v, cols, {1: 0, 2: 1, 3: 0, 4: 1, 5: 0, 6: 1}, [0], [0],
                     [OR.params(2), OR.params(1, 4, t_react=1000.0), OR.params(1, 4, t_react=0.0, v_max=0.001, beta=1e6, v_ball=1e6), OR.params(1, 4, v_ball=1e-3)], vel=vel))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
RUNS = [(c["name"], i) for c in CASES for i in range(len(c["variants"]))]


def run_id(run):
    p = BY_NAME[run[0]]["variants"][run[1]]
    return "%s-R%d-K%d%s" % (run[0], p["R"], p["K"], "" if (p["t_react"], p["v_max"], p["beta"], p["v_ball"]) == (OR.T_REACT, OR.V_MAX, OR.BETA, OR.V_BALL) else "-v%d" % run[1])


@functools.lru_cache(maxsize=None)
def reference(name, i):
    """the contract's (grids, records, options) of the case's window under its i-th parameter set (read only: shared by the tests)"""
    c = BY_NAME[name]
    out = OR.rows(c["values"], c["vel"], c["columns"], c["mapping"], c["cand"], c["owner"], c["row0"], c["n"], c["variants"][i])
    for a in out:
        a.setflags(write=False)
    return out
