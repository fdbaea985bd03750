"""Constructed tables for the team-shape stage (include/eagle.h eagle_op_team_shape / eagle_op_minimap_hulls; contract: tests/shape_ref.py), each named
after what it forces; "check" says, on the contract's result (records [rows, 2], hulls [rows, 2, 32]), that it does.  reference(name) is computed once
per case and shared by the tests.  The hull kernel stages tile rows per workgroup, tile = the largest power of two <= 16 with members x (tile + 1) x 8
bytes <= 32 KB (csrc/shape.hip): up to 240 members give 16, 500 give 4, above 2048 give 1."""
import functools

import numpy as np

import minimap_ref as R
import shape_ref as SR
import trails_cases as TC
import trails_ref as T

P, G, BALL, BND = R.PLAYER, R.GOALKEEPER, R.BALL, R.BOUNDARY
NAN, INF = float("nan"), float("inf")
Q = SR.Q


def team(n, value=0, id0=1):
    """n mapped players of one team value -> (columns, mapping)"""
    return [(P, id0 + i, 0) for i in range(n)], {id0 + i: value for i in range(n)}


def one_row(pts):
    """[(x, y)] -> values [len(pts)][1][2]"""
    return np.array(pts, np.float64).reshape(len(pts), 1, 2)


def _case(name, values, columns, mapping, check=None):
    return {"name": name, "values": np.asarray(values, np.float64), "columns": columns, "mapping": mapping, "check": check or (lambda rec, hl: True)}


def _simple(name, pts, check):
    cols, mp = team(len(pts))
    return _case(name, one_row(pts), cols, mp, check)


def hull_of(hl, r=0, g=0):
    return [int(c) for c in hl[r, g] if c >= 0]


def cloud(seed, n, rows, spread=30.0, centre=(52.5, 34.0)):
    r = np.random.default_rng(seed)
    return np.asarray(centre) + r.uniform(-spread, spread, (n, rows, 2))


def two_teams(name, seed, n_each, rows, holes=0.1, check=None):
    """two groups of n_each players plus a goalkeeper, the ball and an unmapped player; a share of the cells absent"""
    cols = [(P, 1 + i, 0) for i in range(2 * n_each)] + [(G, 900, 0), (BALL, 0, 0), (P, 999, 0)]
    mp = {1 + i: i % 2 for i in range(2 * n_each)}
    v = cloud(seed, len(cols), rows)
    r = np.random.default_rng(seed + 1)
    v[r.uniform(size=v.shape[:2]) < holes] = NAN
    return _case(name, v, cols, mp, check)


def _cases():
    out = []
    tri = [(10.0, 10.0), (30.0, 12.0), (20.0, 40.0)]
    # ---- member counts ----
    out.append(_simple("n_0", [(NAN, 1.0), (2.0, NAN)], lambda rec, hl: rec[0, 0]["n"] == 0 and rec[0, 0]["hull_n"] == 0 and rec[0, 0]["col_min_x"] == -1 and (hl == -1).all()))
    out.append(_simple("n_1", [(NAN, 1.0), (2.0, 3.0)], lambda rec, hl: rec[0, 0]["n"] == 1 and rec[0, 0]["hull_n"] == 1 and hull_of(hl) == [1] and rec[0, 0]["area2"] == 0))
    out.append(_simple("n_2", [(5.0, 5.0), (NAN, NAN), (2.0, 3.0)], lambda rec, hl: rec[0, 0]["n"] == 2 and hull_of(hl) == [2, 0] and rec[0, 0]["area2"] == 0))
    out.append(_simple("all_coincident", [(7.0, 7.0)] * 4, lambda rec, hl: rec[0, 0]["n"] == 4 and rec[0, 0]["hull_n"] == 1 and hull_of(hl) == [0]))
    # ---- collinear sets: hull_n 2, the two far ends, area 0 (columns shuffled so that the ends are neither first nor last) ----
    out.append(_simple("collinear_horizontal", [(3.0, 5.0), (1.0, 5.0), (9.0, 5.0), (4.0, 5.0), (2.0, 5.0)], lambda rec, hl: hull_of(hl) == [1, 2] and rec[0, 0]["area2"] == 0))
    out.append(_simple("collinear_vertical", [(5.0, 3.0), (5.0, 9.0), (5.0, 1.0), (5.0, 4.0)], lambda rec, hl: hull_of(hl) == [2, 1] and rec[0, 0]["area2"] == 0))
    out.append(_simple("collinear_diagonal", [(3.0, 6.0), (1.0, 2.0), (2.0, 4.0), (5.0, 10.0), (4.0, 8.0)], lambda rec, hl: hull_of(hl) == [1, 3] and rec[0, 0]["area2"] == 0))
    # ---- duplicates of the start point: the earliest column is the vertex ----
    out.append(_simple("start_duplicate_later", tri + [tri[0]], lambda rec, hl: hull_of(hl) == [0, 1, 2] and rec[0, 0]["n"] == 4))
    out.append(_simple("start_duplicate_earlier", [tri[1], tri[0], tri[2], tri[0], tri[0]], lambda rec, hl: hull_of(hl) == [1, 0, 2]))
    # ---- points strictly inside an edge, a square and its centre ----
    sq = [(10.0, 10.0), (30.0, 10.0), (30.0, 30.0), (10.0, 30.0)]
    mids = [(20.0, 10.0), (30.0, 20.0), (20.0, 30.0), (10.0, 20.0), (15.0, 10.0)]
    out.append(_simple("inside_edges", mids + sq, lambda rec, hl: hull_of(hl) == [5, 6, 7, 8] and rec[0, 0]["area2"] == 2 * (20 * Q) ** 2))
    out.append(_simple("square_and_centre", [(20.0, 20.0)] + sq, lambda rec, hl: hull_of(hl) == [1, 2, 3, 4] and rec[0, 0]["n"] == 5))
    out.append(_simple("extremum_ties", [(20.0, 20.0), sq[3], sq[2], sq[1], sq[0]],
                       lambda rec, hl: [int(rec[0, 0][k]) for k in ("col_min_x", "col_max_x", "col_min_y", "col_max_y")] == [1, 2, 3, 1]))
    # ---- quantisation ties: x * 1024 + 0.5 is an exact integer: 1.5 / 1024 -> 2, -1.5 / 1024 -> -1, 0.5 / 1024 -> 1, -0.5 / 1024 -> 0 ----
    out.append(_simple("quantisation_ties", [(1.5 / Q, -1.5 / Q), (-1.5 / Q, 1.5 / Q), (0.5 / Q, -0.5 / Q)],
                       lambda rec, hl: [int(rec[0, 0][k]) for k in ("min_x", "max_x", "min_y", "max_y", "sum_x", "sum_y")] == [-1, 2, -1, 2, 2, 1]))
    # ---- the domain's corners: differences of 2^21, products of 2^42 (an int32 product would wrap) ----
    out.append(_simple("domain_corners", [(0.0, 0.0), (1024.0, 1024.0), (-1024.0, -1024.0), (1024.0, -1024.0), (-1024.0, 1024.0)],
                       lambda rec, hl: hull_of(hl) == [2, 3, 1, 4] and rec[0, 0]["area2"] == 2 ** 43 and rec[0, 0]["sum_xx"] == 4 * 2 ** 40))
    out.append(_simple("absent_cells", tri + [(NAN, 1.0), (1.0, INF), (-INF, 1.0), (1024.001, 1.0), (1.0, -1024.001), (NAN, NAN)],
                       lambda rec, hl: rec[0, 0]["n"] == 3 and hull_of(hl) == [0, 1, 2]))
    # ---- who is a member ----
    cols = [(G, 50, 0), (P, 99, 0), (P, 1, 0), (P, 2, 0), (P, 3, 0), (BALL, 0, 0), (BND, 0, 0), (P, 1, 1)]
    pts = [(-100.0, -100.0), (200.0, 200.0)] + tri + [(300.0, -50.0), (-300.0, 50.0), (500.0, 500.0)]
    out.append(_case("outsiders_are_no_members", one_row(pts), cols, {1: 0, 2: 0, 3: 0, 50: 0},
                     lambda rec, hl: rec[0, 0]["n"] == 3 and hull_of(hl) == [2, 3, 4] and rec[0, 1]["n"] == 0))
    cols = [(P, k, 0) for k in range(1, 9)]
    pts = [(10.0, 10.0), (20.0, 10.0), (15.0, 20.0), (40.0, 40.0), (50.0, 40.0), (45.0, 50.0), (60.0, 60.0), (45.0, 30.0)]
    out.append(_case("team_values", one_row(pts), cols, {1: 0, 2: 0, 3: 0, 4: 1, 5: 2, 6: 1, 7: -1, 8: 2},
                     lambda rec, hl: hull_of(hl, 0, 0) == [0, 1, 2] and hull_of(hl, 0, 1) == [7, 4, 5, 3] and rec[0, 1]["n"] == 4))
    # ---- more members than lanes ----
    for n in (65, 129):
        c, mp = team(n, 1)
        out.append(_case("present_%d" % n, cloud(n, n, 2), c, mp, lambda rec, hl, n=n: (rec[:, 1]["n"] == n).all() and (rec[:, 0]["n"] == 0).all()))
    ang = 2 * np.pi * np.arange(40) / 40
    ring = [(52.5 + 30.0 * np.cos(a), 34.0 + 30.0 * np.sin(a)) for a in ang]
    out.append(_simple("circle_40_cut", ring, lambda rec, hl: rec[0, 0]["hull_n"] == 40 and rec[0, 0]["flags"] == SR.FLAG_CUT and (hl[0, 0] >= 0).all()))
    # ---- rows ----
    c, mp = team(4)
    v = cloud(3, 4, 5)
    v[:, 1] = NAN; v[:3, 3] = NAN
    out.append(_case("present_in_some_rows", v, c, mp, lambda rec, hl: [int(x) for x in rec[:, 0]["n"]] == [4, 0, 4, 1, 4]))
    for rows in (1, 63, 64, 65):
        out.append(two_teams("rows_%d" % rows, rows, 5, rows))
    out.append(two_teams("rows_257", 257, 20, 257))
    # ---- rows per workgroup ----
    c, mp = team(2100)
    mp.update({k: 1 for k in range(1500, 2101)})
    out.append(_case("members_2100_tile_1", cloud(21, 2100, 3), c, mp, lambda rec, hl: int(rec[0, 0]["n"]) + int(rec[0, 1]["n"]) == 2100))
    c, mp = team(500)
    mp.update({k: 2 for k in range(1, 501, 3)})
    out.append(_case("members_500_tile_4", cloud(5, 500, 9), c, mp))
    out.append(two_teams("members_240_tile_16", 24, 120, 33, holes=0.3))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the contract's (records, hulls) of a case (read only: shared by the tests)"""
    c = BY_NAME[name]
    rec, hl = SR.shape(c["values"], c["columns"], c["mapping"])
    rec.setflags(write=False); hl.setflags(write=False)
    return rec, hl


# ---- the picture: two teams of five round their goalkeepers, the corners, the ball; six rows, a possession result ----
def picture_case(SM=TC.SMALL):
    cols = [(BND, k, 0) for k in range(4)] + [(P, 1 + i, 0) for i in range(10)] + [(G, 50, 0), (BALL, 0, 0), (P, 99, 0)]
    mp = {1 + i: i % 2 for i in range(10)}
    v = np.concatenate([np.zeros((4, 6, 2)), TC.walk(11, 6, 13, SM, step=3.0)])
    for k, (x, y) in enumerate(((20.0, 0.0), (5.0, 68.0), (90.0, 68.0), (75.0, 0.0))):
        v[k, :] = (x, y)
    v[5, 2] = NAN                                               # a member absent on one row
    ev = TC.events([(1, 2, 0, tuple(v[15, 1]), tuple(v[15, 2]), 4, 6), (3, 4, 1, tuple(v[15, 3]), tuple(v[15, 4]), 6, 5)])
    return {"values": v, "frames": np.arange(6, dtype=np.int32), "columns": cols, "mapping": mp, "S": SM[0], "M": SM[1], "row0": 2, "n": 3,
            "p": T.trail_params(window=3, half_width=1, pass_hold=2), "sel": [4, 5, 15], "owner": np.array([4, 4, 6, 6, 5, 5], np.int32), "events": ev, "hull_hw": 2}


@functools.lru_cache(maxsize=None)
def picture_reference(layers, large=False):
    c = picture_case((4, 2) if large else TC.SMALL)
    fr = SR.frames_bgr(c["values"], c["frames"], c["columns"], c["mapping"], c["row0"], c["n"], c["S"], c["M"], layers=layers, p=c["p"], sel=c["sel"], owner=c["owner"],
                       events=c["events"], hull_hw=c["hull_hw"])
    fr.setflags(write=False)
    return fr
