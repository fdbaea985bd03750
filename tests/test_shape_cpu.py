"""The contract of the team-shape stage (tests/shape_ref.py), its cases (tests/shape_cases.py) and the host module eagle_amd/shape.py, without a GPU:
every case forces what it is named after; the contract's gift-wrapping hull equals an independently written monotone-chain hull on Python integers;
every member lies inside or on its hull; area2 is the shoelace sum; BEATS gives the same winner under any order of comparisons (a shuffled fold and a
butterfly as a wave makes it); shape.py's floats against fractions.Fraction; the hull layer of the picture contract; JSON; the command line's
refusals; the ABI."""
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import minimap_ref as R
import shape_cases as SC
import shape_ref as SR
import trails_ref as T
from eagle_amd import lib, shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dtype_and_constants_are_the_library_s():
    assert SR.SHAPE_DTYPE == lib.SHAPE_DTYPE and lib.SHAPE_DTYPE.itemsize == 96
    assert (SR.HULLS, SR.HULL_CAP, SR.MAX_MEMBERS, SR.FLAG_CUT, SR.Q) == (lib.MM_HULLS, lib.SHAPE_HULL_CAP, lib.SHAPE_MAX_MEMBERS, lib.SHAPE_CUT, lib.SHAPE_Q)
    head = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name, v in (("EAGLE_MM_HULLS", 8), ("EAGLE_SHAPE_HULL_CAP", 32), ("EAGLE_SHAPE_MAX_MEMBERS", 4096), ("EAGLE_SHAPE_CUT", 1)):
        assert re.search(r"#define %s %d\b" % (name, v), head), name
    for name in ("eagle_post_team_shape", "eagle_post_team_shape_values", "eagle_post_device_team_shape", "eagle_minimap_set_hulls", "eagle_op_team_shape",
                 "eagle_op_minimap_hulls"):
        assert re.search(r"\bint %s\(" % name, head) and name in lib.EXPORTS
    import ctypes as C
    assert C.sizeof(lib.EagleHullParams) == 16 and C.sizeof(lib.EagleMinimapParams) == 32


@pytest.mark.parametrize("name", [c["name"] for c in SC.CASES])
def test_case_forces_what_it_is_named_after(name):
    rec, hl = SC.reference(name)
    assert SC.BY_NAME[name]["check"](rec, hl), name


def test_tile_cases_cross_the_thresholds():
    """csrc/shape.hip: tile = the largest power of two <= 16 with members x (tile + 1) x 8 <= 32768 (tile 1: members x 8)"""
    def tile(m):
        t = 16
        while t > 1 and m * (t + 1) * 8 > 32768:
            t >>= 1
        return t
    count = lambda n: sum(len(g) for g in SR.members(SC.BY_NAME[n]["columns"], SC.BY_NAME[n]["mapping"]))
    assert tile(count("members_2100_tile_1")) == 1 and tile(count("members_500_tile_4")) == 4 and tile(count("members_240_tile_16")) == 16
    assert tile(240) == 16 and tile(241) == 8 and tile(4096) == 1 and 4096 * 8 == 32768


def monotone_chain(pts):
    """[(qx, qy, column)] -> the hull's columns counter-clockwise from the smallest (qy, qx), collinear points dropped (Andrew's algorithm, written
    independently of shape_ref.hull); coincident points count once, as their earliest column"""
    first = {}
    for x, y, c in pts:
        first[(x, y)] = min(c, first.get((x, y), c))
    P = sorted(first)
    if len(P) <= 1:
        return [first[p] for p in P]
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for p in P:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(P):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    ring = lower[:-1] + upper[:-1]
    k = min(range(len(ring)), key=lambda i: (ring[i][1], ring[i][0]))
    return [first[p] for p in ring[k:] + ring[:k]]


def _check_row(pts):
    vs, area2 = SR.hull(pts)
    assert vs == monotone_chain(pts)
    at = {c: (x, y) for x, y, c in pts}
    poly = [at[c] for c in vs]
    if len(poly) >= 3:
        for i in range(len(poly)):                              # every member inside or on the hull
            a, b = poly[i], poly[(i + 1) % len(poly)]
            assert all((b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0]) >= 0 for x, y, _ in pts)
    shoelace = sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1] for i in range(len(poly))) if len(poly) >= 3 else 0
    assert area2 == shoelace and area2 >= 0


def test_hull_equals_monotone_chain_on_the_cases():
    for c in SC.CASES:
        groups = SR.members(c["columns"], c["mapping"])
        for r in range(min(c["values"].shape[1], 4)):
            for g in (0, 1):
                _check_row(SR.row_points(c["values"], groups[g], r))


def test_hull_equals_monotone_chain_on_random_rows():
    rng = np.random.default_rng(26)
    for k in range(300):
        n = int(rng.integers(1, 40))
        span = int(rng.choice([3, 50, 2 ** 20]))                # tiny grids force collinear and coincident points
        q = rng.integers(-span, span + 1, (n, 2))
        _check_row([(int(q[i, 0]), int(q[i, 1]), i) for i in range(n)])


def test_any_order_of_comparisons_gives_the_same_winner():
    """BEATS is a strict total order of the candidates seen from an extreme point: a shuffled fold and a 64-lane butterfly return the left fold's winner"""
    rng = np.random.default_rng(7)
    for k in range(200):
        n = int(rng.integers(2, 150))
        span = int(rng.choice([2, 6, 1000]))
        q = rng.integers(-span, span + 1, (n, 2))
        pts = [(int(q[i, 0]), int(q[i, 1]), i) for i in range(n)]
        vs, _ = SR.hull(pts)
        for c in [pts[v] for v in vs]:                          # every vertex the march stands on
            cand = [p for p in pts if (p[0], p[1]) != (c[0], c[1])]
            if not cand:
                continue
            def fold(seq):
                b = seq[0]
                for p in seq[1:]:
                    b = p if SR.beats(c, p, b) else b
                return b
            want = fold(cand)
            shuffled = [cand[i] for i in rng.permutation(len(cand))]
            assert fold(shuffled) == want
            lanes = [None] * 64                                 # the kernel: lane l folds members l, l + 64, ...; then xor-butterfly
            for p in pts:
                if (p[0], p[1]) != (c[0], c[1]):
                    l = p[2] % 64
                    lanes[l] = p if lanes[l] is None or SR.beats(c, p, lanes[l]) else lanes[l]
            d = 32
            while d:
                nxt = list(lanes)
                for l in range(64):
                    o = lanes[l ^ d]
                    if o is not None and (lanes[l] is None or SR.beats(c, o, lanes[l])):
                        nxt[l] = o
                lanes, d = nxt, d // 2
            assert all(v == want for v in lanes)


def _columns(case):
    return np.array([(k, i, v, 0) for k, i, v in case["columns"]], lib.POSTCOL_DTYPE)


def test_derived_values_against_fractions():
    for name in ("rows_65", "team_values", "domain_corners", "quantisation_ties", "present_in_some_rows", "n_0"):
        c = SC.BY_NAME[name]
        rec, hl = SC.reference(name)
        d = shape.derive(rec, hl, _columns(c))
        Q = Fraction(SR.Q)
        for r, row in enumerate(d["rows"]):
            for g in (0, 1):
                o, v = rec[r, g], row["groups"][g]
                n = int(o["n"])
                assert v["n"] == n and v["hull"] == [c["columns"][k][1] for k in hl[r, g] if k >= 0]
                if n == 0:
                    assert v["centroid"] is None and v["area"] is None
                    continue
                sx, sy, sxx, syy = (Fraction(int(o[k])) for k in ("sum_x", "sum_y", "sum_xx", "sum_yy"))
                assert v["centroid"] == (float(sx / (n * Q)), float(sy / (n * Q)))
                assert v["length"] == float((int(o["max_x"]) - int(o["min_x"])) / Q) and v["width"] == float((int(o["max_y"]) - int(o["min_y"])) / Q)
                assert v["area"] == float(Fraction(int(o["area2"])) / (2 * Q * Q))
                assert v["low_line"] == float(int(o["min_x"]) / Q) and v["high_line"] == float(int(o["max_x"]) / Q)
                var = (n * (sxx + syy) - sx * sx - sy * sy) / (n * n * Q * Q)          # var_x + var_y, exact
                assert var >= 0 and v["stretch"] == math.sqrt(float(var))
                # one rounded division and one rounded sqrt: the square is within 3 half ulps of the exact variance
                assert abs(Fraction(v["stretch"]) ** 2 - var) <= var * Fraction(1, 2 ** 51)
            if rec[r, 0]["n"] and rec[r, 1]["n"]:
                a, b = rec[r, 0], rec[r, 1]
                dx = Fraction(int(a["sum_x"]), int(a["n"])) - Fraction(int(b["sum_x"]), int(b["n"]))
                dy = Fraction(int(a["sum_y"]), int(a["n"])) - Fraction(int(b["sum_y"]), int(b["n"]))
                exact = (dx * dx + dy * dy) / (Q * Q)
                assert row["centroid_distance"] == math.sqrt(float(exact))
            else:
                assert row["centroid_distance"] is None
        for g in (0, 1):
            use = [row["groups"][g] for row in d["rows"] if row["groups"][g]["n"] >= 3]
            m = d["clip"]["groups"][g]
            assert m["rows"] == len(use)
            for k in shape.MEAN_KEYS:
                assert m[k] == (float(sum(Fraction(u[k]) for u in use)) / len(use) if use else None)
        both = [r for r in range(len(rec)) if rec[r, 0]["n"] and rec[r, 1]["n"]]
        if both:
            s = [sum(Fraction(int(rec[r, g]["sum_x"]), int(rec[r, g]["n"])) for r in both) for g in (0, 1)]
            assert d["clip"]["defends_left"] == [s[0] < s[1], s[1] < s[0]]
        else:
            assert d["clip"]["defends_left"] is None and d["clip"]["centroid_distance"] is None


def test_defends_left_and_lines():
    cols, mp = SC.team(4)
    mp.update({3: 1, 4: 1})
    v = SC.one_row([(10.0, 5.0), (10.0, 5.0), (80.0, 5.0), (90.0, 5.0)])
    rec, hl = SR.shape(v, cols, mp)
    d = shape.derive(rec, hl, np.array([(k, i, x, 0) for k, i, x in cols], lib.POSTCOL_DTYPE), line_members=[[([1, 2], [1, 2]), ([3], [4])]])
    assert d["clip"]["defends_left"] == [True, False] and d["rows"][0]["groups"][0]["low_ids"] == [1, 2] and d["rows"][0]["groups"][1]["high_ids"] == [4]
    assert d["rows"][0]["centroid_distance"] == 75.0 and d["clip"]["groups"][0]["rows"] == 0 and d["clip"]["groups"][0]["area"] is None
    assert shape.member_columns(np.array([(k, i, x, 0) for k, i, x in cols], lib.POSTCOL_DTYPE), mp) == tuple(SR.members(cols, mp))


def test_json_round_trip():
    c = SC.BY_NAME["rows_63"]
    rec, hl = SC.reference("rows_63")
    d = shape.derive(rec, hl, _columns(c), frames=np.arange(63))
    j = json.loads(json.dumps(shape.to_json(d)))
    assert shape.from_json(j) == d


def test_hull_layer_covers_only_pixels_within_half_width_of_an_edge():
    c = SC.picture_case()
    S, M, hw = c["S"], c["M"], c["hull_hw"]
    res = SR.shape(c["values"], c["columns"], c["mapping"])
    w, h = R.size(S, M)
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    for row in range(c["row0"], c["row0"] + c["n"]):
        with_l = SR.draw_row(c["values"], c["frames"], c["columns"], c["mapping"], row, S, M, layers=SR.HULLS, hull_hw=hw, shape_result=res)
        without = SR.draw_row(c["values"], c["frames"], c["columns"], c["mapping"], row, S, M)
        assert np.array_equal(without, T.draw_row(c["values"], c["frames"], c["columns"], c["mapping"], row, S, M))      # no layer: trails_ref's picture
        changed = (with_l != without).any(-1)
        edges = SR.hull_edges(c["values"], res[0], res[1], row, S, M)
        assert changed.any() and len(edges) >= 6
        near = np.zeros((h, w), bool)
        for ax, ay, bx, by, _ in edges:                        # exact: squared distance to the segment <= (16 hw)^2, on rationals cleared of denominators
            px, py, dx, dy = 16 * X - ax, 16 * Y - ay, bx - ax, by - ay
            L2 = dx * dx + dy * dy
            t = np.clip(px * dx + py * dy, 0, L2)
            near |= (px * L2 - t * dx) ** 2 + (py * L2 - t * dy) ** 2 <= (16 * hw) ** 2 * L2 * L2
        assert not (changed & ~near).any()
        colors = {tuple(int(v) for v in p) for p in with_l[changed]}
        assert colors <= {SR.hull_color(0), SR.hull_color(1), (0, 0, 255), (255, 0, 0), (0, 255, 0), (255, 255, 255)} and SR.hull_color(0) == (0, 0, 159)


def test_contract_refusals():
    c = SC.BY_NAME["team_values"]
    with pytest.raises(ValueError):
        SR.shape(c["values"], c["columns"], None)
    with pytest.raises(ValueError):
        SR.shape(c["values"], [(7, 1, 0)] + c["columns"][1:], c["mapping"])
    cols, mp = SC.team(4097)
    with pytest.raises(ValueError):
        SR.members(cols, mp)
    for hw in (0, 9):
        with pytest.raises(ValueError):
            SR.check_hull_params(hw)
    assert SR.edge_indices(1, 0) == [] and SR.edge_indices(2, 0) == [(0, 1)] and SR.edge_indices(3, 0) == [(0, 1), (1, 2), (2, 0)]
    assert len(SR.edge_indices(40, 1)) == 31 and SR.edge_indices(40, 1)[-1] == (30, 31) and SR.edge_indices(32, 0)[-1] == (31, 0)


@pytest.mark.parametrize("argv", [["--shape"], ["--processed", "--minimap-hulls"], ["--processed", "--minimap", "--minimap-hulls", "0"],
                                  ["--processed", "--minimap", "--minimap-hulls", "9"], ["--processed", "--minimap", "--minimap-hulls", "x"]])
def test_cli_refuses(argv, capsys):
    from eagle_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--synthetic-weights"] + argv)
    assert e.value.code == 2
