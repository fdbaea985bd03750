"""Constructed tables for the minimap (include/eagle.h eagle_op_minimap; contract: tests/minimap_ref.py): values float64 [cols][rows][2], the column
descriptors (kind, id, video) and the team mapping, chosen for the seams of the kernel and of the contract, not for the workload:
S = 2, M = 0 -> 210 x 136 (one tile column, a 2-pixel tail strip); S = 2, M = 2 -> 214 x 140 (a 6-pixel tail, a partial last tile row);
S = 4, M = 2 -> 424 x 276 (crosses the 256-pixel tile seam and seventeen 16-row seams).  The site counts 65, 257 and 300 cross a wave, the
256-entry LDS chunk of the draw pass and EAGLE_MAX_DET.  reference(name) is computed once per case and shared by the tests."""
import functools

import numpy as np

import minimap_ref as R

P, G, BALL, BND = R.PLAYER, R.GOALKEEPER, R.BALL, R.BOUNDARY
NAN, INF = float("nan"), float("inf")
BOUNDS = [(BND, k, 0) for k in range(4)]


def table(columns, rows):
    return np.full((len(columns), rows, 2), NAN, np.float64)


def put_bounds(v, row, bl, tl, tr, br):
    """the four boundary cells of a row as the post-processor writes them: x on the touch lines y = 0, 68, 68, 0"""
    for k, (x, y) in enumerate(((bl, 0.0), (tl, 68.0), (tr, 68.0), (br, 0.0))):
        v[k, row] = (x, y)


def _case(name, values, columns, mapping, S, M, row0=0, n=None, **kw):
    return {"name": name, "values": values, "columns": columns, "mapping": mapping, "S": S, "M": M, "row0": row0,
            "n": values.shape[1] - row0 if n is None else n, "kw": kw}


def sites_case(name, count, S, M, seed, rows=1, **kw):
    """`count` mapped players at uniformly random pitch points (every one present on every row), a video column in between, a ball"""
    r = np.random.default_rng(seed)
    cols = BOUNDS + [c for i in range(count) for c in ((P, i + 1, 0), (P, i + 1, 1))] + [(BALL, 0, 0), (BALL, 0, 1)]
    v = table(cols, rows)
    for row in range(rows):
        put_bounds(v, row, 20.0 + row, 10.0, 80.0, 70.0 - row)
        for i in range(count):
            v[4 + 2 * i, row] = (r.uniform(0, 105), r.uniform(0, 68))
            v[5 + 2 * i, row] = (r.uniform(0, 1280), r.uniform(0, 720))          # a video point: never drawn
        v[-2, row] = (r.uniform(0, 105), r.uniform(0, 68))
    return _case(name, v, cols, {i + 1: i % 2 for i in range(count)}, S, M, voronoi=1, **kw)


def tie_case(swapped):
    """two sites of different teams at x = 40 and x = 60 on the halfway height: at S = 2, M = 2 the pixel column X = 102 (16 X = 1632) is equidistant"""
    cols = BOUNDS + ([(P, 2, 0), (P, 1, 0)] if swapped else [(P, 1, 0), (P, 2, 0)])
    v = table(cols, 1)
    v[4 + (1 if swapped else 0), 0] = (40.0, 34.0)
    v[4 + (0 if swapped else 1), 0] = (60.0, 34.0)
    return _case("tie_swapped" if swapped else "tie", v, cols, {1: 0, 2: 1}, 2, 2, voronoi=1, player_radius=1)


def _cases():
    out = []
    cols = BOUNDS + [(P, 1, 0), (P, 1, 1), (P, 2, 0), (G, 3, 0), (BALL, 0, 0)]
    out.append(_case("all_nan", table(cols, 1), cols, {1: 0, 2: 1}, 2, 0, voronoi=1))
    out += [tie_case(False), tie_case(True)]
    out.append(sites_case("sites1", 1, 4, 2, 11))
    out.append(sites_case("sites22", 22, 4, 2, 0, rows=2))
    out.append(sites_case("sites65", 65, 2, 0, 12))
    out.append(sites_case("sites257", 257, 2, 2, 13))
    out.append(sites_case("sites300", 300, 2, 2, 14, rows=3, row0=1, n=2))

    # off the pitch, off the canvas, and everything that makes a cell absent; a goalkeeper (green, no site); a player without a team (nothing)
    pts = [(-3.0, 10.0), (107.5, 70.25), (50.0, -1.0), (-40.0, -40.0), (300.0, 34.0), (1024.0, -1024.0), (1024.5, 10.0), (10.0, -1025.0),
           (NAN, 30.0), (30.0, NAN), (INF, 30.0), (30.0, -INF), (1e30, 1e30), (52.5, 34.0)]
    cols = BOUNDS + [(P, i + 1, 0) for i in range(len(pts))] + [(G, 50, 0), (P, 99, 0), (G, 51, 0), (BALL, 0, 0)]
    v = table(cols, 1)
    for i, pt in enumerate(pts):
        v[4 + i, 0] = pt
    v[4 + len(pts), 0], v[5 + len(pts), 0], v[6 + len(pts), 0], v[7 + len(pts), 0] = (5.0, 34.0), (70.0, 20.0), (NAN, NAN), (106.0, 69.0)
    put_bounds(v, 0, 10.0, 25.0, 85.0, 95.0)
    mapping = {i + 1: (0, 1, 7)[i % 3] for i in range(len(pts))}                  # (99 has no entry; team 7 is "any other team": blue)
    out.append(_case("edges_voronoi", v, cols, mapping, 2, 2, voronoi=1))
    out.append(_case("edges_plain", v, cols, mapping, 4, 2, voronoi=0, footprint=0))
    out.append(_case("no_mapping", v, cols, None, 2, 0))

    # footprints: normal, crossed, off the canvas, a corner missing, a corner beyond the domain; drawn as windows of one to three rows
    cols = BOUNDS + [(P, 1, 0), (BALL, 0, 0), (BND, 0, 0)]                        # (a second Bottom_Left column: the first one counts)
    v = table(cols, 5)
    put_bounds(v, 0, 20.0, 5.0, 90.0, 75.0)
    put_bounds(v, 1, 75.0, 5.0, 90.0, 20.0)
    put_bounds(v, 2, -400.0, -300.0, -200.0, -250.0)
    put_bounds(v, 3, 20.0, 5.0, 90.0, 75.0); v[2, 3] = (NAN, 68.0)
    put_bounds(v, 4, 20.0, 5.0, 90.0, 2000.0)
    v[6, :] = (0.0, 0.0)
    for row in range(5):
        v[4, row], v[5, row] = (30.0 + 10 * row, 40.0), (31.0 + 10 * row, 41.0)
    out.append(_case("footprints_a", v, cols, {1: 1}, 2, 2, row0=0, n=3))
    out.append(_case("footprints_b", v, cols, {1: 1}, 4, 2, row0=3, n=2, voronoi=1))
    out.append(_case("footprint_uncrossed", v, cols, {1: 1}, 2, 2, row0=0, n=1))
    out.append(_case("footprint_crossed", v, cols, {1: 1}, 2, 2, row0=1, n=1))

    # nothing drawable: boundary and video columns only (markings + footprint), and a table whose only player has no team
    cols = BOUNDS + [(P, 1, 1), (BALL, 0, 1)]
    v = table(cols, 2)
    put_bounds(v, 1, 20.0, 5.0, 90.0, 75.0)
    v[4, :], v[5, :] = (640.0, 360.0), (600.0, 300.0)
    out.append(_case("no_drawable_columns", v, cols, {1: 0}, 2, 0, voronoi=1))
    cols = [(P, 9, 0)]
    v = table(cols, 1)
    v[0, 0] = (50.0, 30.0)
    out.append(_case("only_unmapped_player", v, cols, {1: 0}, 2, 2, voronoi=1))

    # the ball's ring on a disc on the centre mark and the halfway line; default and explicit radii
    cols = BOUNDS + [(P, 1, 0), (G, 2, 0), (BALL, 0, 0)]
    v = table(cols, 1)
    v[4, 0], v[5, 0], v[6, 0] = (52.5, 34.0), (11.0, 34.0), (52.5, 34.0)
    out.append(_case("stack_default", v, cols, {1: 0}, 4, 2))
    out.append(_case("stack_explicit", v, cols, {1: 0}, 4, 2, player_radius=7, ball_radius=16))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the contract's BGR pictures of a case, uint8 [n, h, w, 3] (read only: shared by the tests)"""
    c = BY_NAME[name]
    fr = R.frames_bgr(c["values"], c["columns"], c["mapping"], c["row0"], c["n"], c["S"], c["M"], **c["kw"])
    fr.setflags(write=False)
    return fr
