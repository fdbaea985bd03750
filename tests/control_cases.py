"""Constructed tables for the kinematics and pitch-control entries (include/eagle.h eagle_op_velocities / eagle_op_control / eagle_op_minimap_control;
contract: tests/control_ref.py): values float64 [cols][rows][2], the kept frame numbers, the column descriptors (kind, id, video) and the team
mapping, chosen for the seams of the kernels and of the contract, not for the workload.  A grid is 105 R x 68 R cells = 7140 R^2 bytes: 7 workgroups of
1024 cells at R = 1 (the last one partly idle), 28 at R = 2, 112 at R = 4.  The site count 257 crosses the 256-entry LDS chunk; the row counts 65 and
257 cross a wave and a 256-row block of the velocity and site kernels.  given_velocities() is the one table whose velocities are not the contract's
own: they force the rules no differenced table reaches (a component beyond fp32, NaN, the clamp of the reaction point).  velocities(name) and grids(name, R) are computed once and shared."""
import functools

import numpy as np

import control_ref as CR
import minimap_ref as MR

P, G, BALL, BND = MR.PLAYER, MR.GOALKEEPER, MR.BALL, MR.BOUNDARY
NAN, INF = float("nan"), float("inf")
BOUNDS = [(BND, k, 0) for k in range(4)]


def table(columns, rows):
    return np.full((len(columns), rows, 2), NAN, np.float64)


def _case(name, values, frames, columns, mapping, fps=5, max_gap=None, speed_cap=CR.SPEED_CAP, row0=0, n=None):
    frames = np.asarray(frames, np.int32)
    assert len(frames) == values.shape[1]
    return {"name": name, "values": values, "frames": frames, "columns": columns, "mapping": mapping, "fps": fps, "max_gap": fps if max_gap is None else max_gap,
            "speed_cap": speed_cap, "row0": row0, "n": values.shape[1] - row0 if n is None else n}


def walkers(name, count, rows, seed, frames=None, fps=5, step=0.4, teams=2, **kw):
    """`count` mapped players on a random walk over the pitch (present on every row), a video column after each, a goalkeeper and a ball"""
    r = np.random.default_rng(seed)
    cols = BOUNDS + [c for i in range(count) for c in ((P, i + 1, 0), (P, i + 1, 1))] + [(G, 900, 0), (BALL, 0, 0), (BALL, 0, 1)]
    v = table(cols, rows)
    pos = np.stack([r.uniform(0, 105, count), r.uniform(0, 68, count)], 1)
    for row in range(rows):
        pos = pos + r.normal(0, step, pos.shape)
        v[4:4 + 2 * count:2, row] = pos
        v[5:5 + 2 * count:2, row] = pos * 12.0 + r.normal(0, 3.0, pos.shape)                 # a video point: never a site
        v[-3, row], v[-2, row], v[-1, row] = (3.0, 34.0 + 0.1 * row), (50.0 + row, 30.0), (640.0, 360.0)
    return _case(name, v, np.arange(rows) if frames is None else frames, cols, {i + 1: i % teams for i in range(count)}, fps, **kw)


def _cases():
    out = []
    # 0, 1 and 2 sites on consecutive rows; a single-row table (every velocity is (0, 0) or NaN)
    cols = BOUNDS + [(P, 1, 0), (P, 1, 1), (P, 2, 0), (G, 3, 0), (BALL, 0, 0)]
    v = table(cols, 3)
    v[4, 1], v[4, 2], v[6, 2], v[7, :], v[8, :] = (30.0, 20.0), (31.5, 21.0), (70.0, 50.0), (5.0, 34.0), (52.5, 34.0)
    v[5, :] = (400.0, 300.0)
    out.append(_case("sites_0_1_2", v, [3, 4, 6], cols, {1: 0, 2: 1}))
    out.append(_case("single_row", v[:, 2:3].copy(), [9], cols, {1: 0, 2: 1}))
    # one team only: every byte 255 (team 0) or 0 (any other team)
    cols = BOUNDS + [(P, 1, 0), (P, 2, 0), (P, 3, 0)]
    v = table(cols, 2)
    v[4, :], v[5, :], v[6, :] = (10.0, 10.0), (60.0, 40.0), (100.0, 60.0)
    v[5, 1] = (61.0, 40.5)
    out.append(_case("only_team0", v, [0, 1], cols, {1: 0, 2: 0, 3: 0}))
    out.append(_case("only_others", v, [0, 1], cols, {1: 1, 2: 7, 3: 1}))
    out.append(walkers("sites22", 22, 3, 0))
    out.append(walkers("sites257", 257, 2, 13, row0=1, n=1))
    out.append(walkers("rows65", 3, 65, 5, frames=2 * np.arange(65), fps=10, step=0.25))
    out.append(walkers("rows257", 2, 257, 6, fps=25, step=0.1))                   # every row is drawn: two blocks of the site kernel, grid rows beyond 255

    # what is a site and what is not; the exp clamp; two sites on one point
    pts = [(20.0, 30.0), (20.0, 30.0),                      # the same point, opposite teams: their weights are equal everywhere
           (1024.5, 10.0), (10.0, -1025.0), (1e30, 1e30),   # beyond 1024 m: not sites
           (-900.0, 34.0), (1024.0, -1024.0),               # far away but sites: -beta (t - t_min) passes -87
           (NAN, 30.0), (30.0, NAN), (INF, 30.0), (30.0, -INF),
           (80.0, 50.0), (52.5, 34.0)]
    cols = BOUNDS + [(P, i + 1, 0) for i in range(len(pts))] + [(G, 50, 0), (P, 99, 0), (BALL, 0, 0)]
    v = table(cols, 2)
    for i, pt in enumerate(pts):
        v[4 + i, :] = pt
    v[4 + 11, 1] = (82.0, 49.0)                              # one of them moves: 2 m/s
    v[4 + 5, 1] = (-1500.0, 34.0)                            # leaves the domain on row 1 (its row-0 velocity is capped at 12 m/s)
    v[-3, :], v[-2, :], v[-1, :] = (5.0, 34.0), (70.0, 20.0), (60.0, 30.0)        # goalkeeper: no site; player 99: no team entry
    out.append(_case("edges", v, [0, 5], cols, {i + 1: (0, 1, 7)[i % 3] for i in range(len(pts))}))

    # velocity seams: fps 1, max_gap 5, cap 5: frame gaps of exactly 5 and of 6, a speed exactly at the cap and above it, isolated cells, half cells
    cols = [(P, 1, 0), (P, 2, 0), (P, 2, 1), (P, 3, 0)]
    fr = [0, 1, 2, 7, 8, 14, 15, 16]
    v = table(cols, len(fr))
    v[0, :, 0] = [0.0, 3.0, 6.0, 6.0, 20.0, 20.0, 23.0, 27.0]                    # row 1: central (6, 8) / 2 = (3, 4): exactly 5; row 4: 14 m over 1 s, capped
    v[0, :, 1] = [0.0, 4.0, 8.0, 8.0, 8.0, 8.0, 12.0, 12.0]
    v[1, 1], v[1, 3], v[1, 6] = (10.0, 10.0), (11.0, 10.0), (40.0, 40.0)          # isolated cells: (0, 0)
    v[1, 4] = (NAN, 5.0)                                                          # half a cell is absent
    v[2, :, 0], v[2, :, 1] = 100.0 * np.arange(len(fr)), 50.0                    # a video column: px/s, capped like the others
    v[3, 0], v[3, 1], v[3, 7] = (50.0, 30.0), (INF, 30.0), (50.0, 31.0)           # an infinite neighbour is absent
    out.append(_case("seams", v, fr, cols, {1: 0, 2: 1, 3: 1}, fps=1, max_gap=5, speed_cap=5.0))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def velocities(name):
    c = BY_NAME[name]
    v = CR.velocities(c["values"], c["frames"], c["fps"], c["max_gap"], c["speed_cap"])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def grids(name, R):
    """the contract's grids and byte sums of the case's window (read only: shared by the tests)"""
    c = BY_NAME[name]
    g, s = CR.grids(c["values"], velocities(name), c["columns"], c["mapping"], c["row0"], c["n"], R)
    g.setflags(write=False); s.setflags(write=False)
    return g, s


def given_velocities():
    """five sites on one row with velocities handed in: finite in fp32 but enormous (q is clamped to +-2^20), beyond fp32 and NaN (count as 0), and an
    ordinary one; with t_react = 1000 s the ordinary one lands 12 km away, inside the clamp -> (values, velocities, columns, mapping)"""
    cols = [(P, i + 1, 0) for i in range(5)]
    v = table(cols, 1)
    v[:, 0] = [(20.0, 30.0), (80.0, 30.0), (50.0, 10.0), (50.0, 60.0), (30.0, 50.0)]
    vel = np.zeros_like(v)
    vel[:, 0] = [(1e30, -1e30), (1e39, -1e300), (NAN, INF), (12.0, 0.0), (-3.0e38, 2.0)]
    return v, vel, cols, {1: 0, 2: 1, 3: 0, 4: 1, 5: 0}
