"""Constructed tables for the occupancy entries (include/eagle.h eagle_op_occupancy / eagle_post_occupancy; contract: tests/occupancy_ref.py), each named
after the edge it forces (tests/test_occupancy_cpu.py asserts through the contract that it does).  The blur kernel's tile is 64 cells along the
filter's axis and 16 across, the histogram kernel's workgroup 256 rows and its wave 64: the radii and row counts lie on both sides of those.
reference(name) is computed once and shared.

One edge of the issue cannot be forced through the library: a radius beyond the grid's height.  The accepted sigma ends at 10 m, so rad <= 30 R, and the
grid is 68 R high.  The contract's functions take any sigma; tests/test_occupancy_cpu.py checks their clipping of such a radius directly."""
import functools

import numpy as np

import occupancy_ref as OR

P, G, BALL, BND = OR.PLAYER, OR.GOALKEEPER, OR.BALL, OR.BOUNDARY
NAN, INF = float("nan"), float("inf")
BOUNDS = [(BND, k, 0) for k in range(4)]
BLUR_TILE = 64
ROWS = (1, 255, 256, 257, 1025)
BELOW_105, BELOW_68 = float(np.nextafter(105.0, 0.0)), float(np.nextafter(68.0, 0.0))
# (sigma, R) -> rad: 0, 1, below the tile, the tile, beyond the tile, the maximum; 1e-30: rad 1 with an infinite 1 / (2 s s)
RADII = {"rad0": (0.0, 1, 0), "rad1": (0.3, 1, 1), "rad1_inv_inf": (1e-30, 2, 1), "rad_below_tile": (2.0, 4, 24), "rad_is_tile": (5.3, 4, 64),
         "rad_beyond_tile": (7.0, 4, 84), "rad_max": (10.0, 4, 120), "rad30_R1": (10.0, 1, 30), "rad60_R2": (10.0, 2, 60)}


def _case(name, values, frames, columns, sels, R=1, sigma=OR.SIGMA, max_gap=None, fps=5):
    values = np.asarray(values, np.float64)
    frames = np.asarray(frames, np.int32)
    assert values.shape == (len(columns), len(frames), 2), (name, values.shape)
    off, cols = [0], []
    for s in sels:
        cols += list(s)
        off.append(len(cols))
    return {"name": name, "values": values, "frames": frames, "columns": columns, "sel_off": off, "sel_cols": cols, "R": R, "sigma": sigma,
            "max_gap": fps if max_gap is None else max_gap, "fps": fps}


def single(name, points, frames=None, **kw):
    """one player column (column 4, behind the bounds) with its video column, one row per point"""
    cols = BOUNDS + [(P, 1, 0), (P, 1, 1)]
    v = np.full((len(cols), len(points), 2), NAN)
    v[4] = np.asarray(points, np.float64).reshape(-1, 2)
    v[5] = 300.0
    return _case(name, v, np.arange(len(points)) if frames is None else frames, cols, [[4]], **kw)


EDGE_POINTS = [(0.0, 0.0), (0.0, 5.5), (5.5, 0.0), (105.0, 5.5), (5.5, 68.0), (105.0, 68.0), (BELOW_105, BELOW_68), (BELOW_105, 5.5), (5.5, BELOW_68),
               (-0.0, -0.0), (-0.0, 7.25), (NAN, 5.5), (5.5, NAN), (INF, 5.5), (-INF, 5.5), (5.5, INF), (5.5, -INF), (1e300, -1e300), (-1e-300, 5.5),
               (5.5, -1e-300), (500.0, 5.5), (-3.0, 70.0), (52.5, 34.0)]


def corner_points(R):
    e = 1.0 / R
    return [(e / 2, e / 2), (105.0 - e / 2, e / 2), (e / 2, 68.0 - e / 2), (105.0 - e / 2, 68.0 - e / 2), (52.5 + e / 4, 34.0 + e / 4)]


def walkers(name, persons, rows, seed, R=1, sigma=OR.SIGMA, sels="default", gaps=True, ball=True, **kw):
    """`persons` players (the last one a goalkeeper when there are at least 3) and the ball on a random walk that leaves the pitch now and then, a few
    cells NaN, frame steps of 1 .. 4 when gaps; the default selections of tests/occupancy_ref.py"""
    r = np.random.default_rng(seed)
    cols = list(BOUNDS)
    for i in range(persons):
        kind = G if persons >= 3 and i == persons - 1 else P
        cols += [(kind, i + 1, 0), (kind, i + 1, 1)]
    if ball:
        cols += [(BALL, 0, 0), (BALL, 0, 1)]
    v = np.full((len(cols), rows, 2), NAN)
    for c, (kind, ident, video) in enumerate(cols):
        if kind == BND:
            v[c] = (50.0, 30.0)
        elif video:
            v[c] = 400.0
        else:
            v[c] = np.array([r.uniform(-2, 107), r.uniform(-2, 70)]) + np.cumsum(r.normal(0, 0.15, (rows, 2)), 0)
            v[c][r.random(rows) < 0.05] = NAN
    frames = np.cumsum(r.integers(1, 5, rows)) if gaps else np.arange(rows)
    mapping = {i + 1: i % 2 for i in range(persons) if i % 5 != 4}
    if sels == "default":
        off, sc, _ = OR.default_selections(cols, mapping)
        sels = [sc[off[s]:off[s + 1]] for s in range(len(off) - 1)]
    c = _case(name, v, frames, cols, sels, R=R, sigma=sigma, **kw)
    c["mapping"] = mapping
    return c


def _build():
    cases = []
    for R in OR.RS:
        cases.append(single("edges_R%d" % R, EDGE_POINTS, R=R, sigma=0.3))
        cases.append(single("corners_centre_R%d" % R, corner_points(R), R=R, sigma=2.0))
    for key, (sigma, R, rad) in RADII.items():
        cases.append(single(key, corner_points(R) + [(10.25, 60.25), (70.75, 20.75), (104.9, 33.0), (30.0, 0.1)], R=R, sigma=sigma))
    # contention: every row of a column in one cell, and the same with two member columns
    still = np.tile([[40.3, 20.6]], (4096, 1))
    cases.append(single("one_cell_4096", still, R=2, sigma=0.0))
    c = single("one_cell_two_columns_4096", still, R=4, sigma=0.5)
    c["columns"] = c["columns"] + [(G, 2, 0)]
    c["values"] = np.concatenate([c["values"], (still + [[0.05, 0.05]])[None]])
    c["sel_off"], c["sel_cols"] = [0, 2], [4, 6]
    cases.append(c)
    # frame steps 1, k, exactly max_gap, max_gap + 1 and the last row: one row per cell along x
    cases.append(single("frame_steps", [(2.5 + 3 * k, 10.5) for k in range(7)], frames=[0, 1, 2, 5, 12, 20, 21], max_gap=7, sigma=0.0))
    # selections
    w = walkers("selections", 4, 300, 11, R=2, sigma=1.0, sels=[[], [4, 6], [4], [4, 6, 8, 10], [12], []])
    cases.append(w)
    cases.append(walkers("ball_only_table", 0, 200, 12, sels="default"))
    cases.append(walkers("no_person_no_ball", 0, 50, 13, ball=False, sels="default"))
    cases.append(walkers("everyone_R2", 23, 600, 14, R=2, sigma=2.0))
    cases.append(walkers("everyone_R4_raw", 23, 300, 15, R=4, sigma=0.0))
    # a one-cell count beyond 2^24: the conversion to float32 rounds
    n = 131074
    big = single("count_above_2p24", np.tile([[60.5, 30.5]], (n, 1)), frames=128 * np.arange(n), max_gap=128, sigma=0.3)
    cases.append(big)
    for n in ROWS:
        cases.append(walkers("rows_%d" % n, 3, n, 100 + n, R=1, sigma=1.0))
    return cases


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def args(c):
    return c["values"], c["frames"], c["columns"], c["sel_off"], c["sel_cols"], c["R"], c["sigma"], c["max_gap"]


@functools.lru_cache(maxsize=None)
def reference(name):
    res = OR.occupancy(*args(BY_NAME[name]))
    for v in res.values():
        v.setflags(write=False)
    return res
