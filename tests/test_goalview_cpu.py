"""The goal-view contract on the host (tests/goalview_ref.py): its shadows agree with an independent test by the distance from the disc's centre to
the ray through each slice centre, its angle stays within the midpoint rule's bound of the arctangent, the constructed cases are what their names say,
eagle_amd.goalview.resolve refuses what the library refuses, and the joins with the ball flights and the pass events work on constructed results.
No GPU."""
import math
import os
import re

import numpy as np
import pytest

import goalview_cases as GC
import goalview_ref as GR
import offside_ref as OR
from eagle_amd import goalview as GV, lib

NAMES = [c["name"] for c in GC.CASES]
SEED = 20261021


def _configurations(n, seed):
    """n random (P, D, rho, goal) on the grid of q; half of the points within 25 m of their goal; most discs near the way to the mouth"""
    r = np.random.default_rng(seed)
    right = r.integers(0, 2, n).astype(bool)
    xg = np.where(right, 105.0, 0.0)
    near = np.arange(n) % 2 == 0
    dist = np.where(near, r.uniform(1.0, 25.0, n), r.uniform(25.0, 60.0, n))
    ang = r.uniform(-1.3, 1.3, n)
    px = xg - np.where(right, 1.0, -1.0) * np.maximum(dist * np.cos(ang), 1.0)
    py = 34.0 + dist * np.sin(ang)
    t = r.uniform(0.02, 1.05, n)
    ty = r.uniform(28.0, 40.0, n)
    bx = px + t * (xg - px) + r.normal(0, 0.3, n)
    by = py + t * (ty - py) + r.normal(0, 1.0, n)
    rho = np.where(r.uniform(size=n) < 0.4, 0.4, np.where(r.uniform(size=n) < 0.5, 1.0, r.uniform(0.05, 2.0, n)))
    q = lambda v: np.rint(v * 1024.0) / 1024.0
    return q(px), q(py), xg, q(bx), q(by), rho


def test_shadows_against_the_ray_distance_test():
    n = 12000
    px, py, xg, bx, by, rho = _configurations(n, SEED)
    got = np.zeros((n, 64), bool)
    for goal in (0.0, 105.0):
        m = xg == goal
        got[m] = GR.shadow(px[m], py[m], goal - px[m], goal, bx[m], by[m], rho[m])
    want, margin = np.zeros((n, 64), bool), np.zeros((n, 64))
    for k in range(n):
        want[k], margin[k] = GR.brute_blocked(px[k], py[k], xg[k], bx[k], by[k], rho[k])
    diff = got != want
    print("bits %d, blocked %d, differing %d, of them within 1e-9 m of the disc's edge %d" % (diff.size, want.sum(), diff.sum(), (diff & (np.abs(margin) < 1e-9)).sum()))
    assert want.sum() > 20000 and (~want).sum() > 20000                    # both answers are exercised
    assert (np.abs(margin[diff]) < 1e-9).all()
    assert diff.sum() <= 1e-4 * diff.size
    assert diff.sum() == 0                                                # (this seed: no bit lies that near an edge)


def test_full_angle_within_the_midpoint_rule_bound():
    r = np.random.default_rng(SEED + 1)
    n = 20000
    depth = np.concatenate([r.uniform(1.0, 3.0, n // 2), r.uniform(3.0, 60.0, n // 2), [1.0, 1.0, 1.0]])
    py = np.concatenate([r.uniform(-20.0, 90.0, n), [34.0, 30.34, 0.0]])
    depth, py = np.rint(depth * 1024.0) / 1024.0, np.rint(py * 1024.0) / 1024.0
    depth = np.maximum(depth, 1.0)
    for sign in (1.0, -1.0):
        full = GR.weights(py, sign * depth).sum(1)
        theta = np.arctan2(37.66 - py, depth) - np.arctan2(30.34 - py, depth)
        err = np.abs(full / 2.0 ** 24 - theta)
        bound = 0.008 / depth ** 3 + 64 * 2.0 ** -25
        print("largest error / bound: %.3f" % (err / bound).max())
        assert (err <= bound).all()
        assert (full < 2 ** 27).all() and (full > 0).all()


def test_slice_centres_ascend_and_are_symmetric_to_rounding():
    assert (np.diff(GR.YC) > 0.1).all() and len(GR.YC) == 64
    assert np.abs(GR.YC + GR.YC[::-1] - 68.0).max() < 1e-13 and GR.YC[0] > 30.34 and GR.YC[-1] < 37.66


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_its_name_says(name):
    o = GC.reference(name)
    c = GC.BY_NAME[name]
    rows, nm = c["values"].shape[1], len(o["totals"])
    R = c["p"]["cells_per_metre"]
    assert o["rows"].shape == (rows, 2) and o["open"].shape == o["mask"].shape == o["status"].shape == (nm, rows)
    assert o["grid"].shape == (c["p"]["grid_rows"], 68 * R, 105 * R) and 1 <= rows <= 70
    assert c["check"](o)


def test_cases_cover_the_shapes_the_kernels_need():
    blockers = set()
    for name in NAMES:
        blockers |= set(GC.reference(name)["rows"]["n_blockers"].ravel().tolist())
    assert {0, 1, 32, 33} <= blockers
    assert sorted(c["p"]["cells_per_metre"] for c in GC.CASES if c["p"]["cells_per_metre"] != 1) == [2, 4]
    assert all(c["p"]["grid_rows"] > 0 for c in GC.CASES) and max(c["values"].shape[1] for c in GC.CASES) == 70
    assert any(c["p"]["group"] == -1 for c in GC.CASES) and any(c["p"]["direction"] == OR.DIR_LEFT for c in GC.CASES)


def test_records_match_the_header_and_the_bindings():
    head = open(os.path.join(os.path.dirname(__file__), "..", "include", "eagle.h")).read()
    for name in ("eagle_goal_view_params_default", "eagle_post_goal_view", "eagle_post_goal_view_values", "eagle_post_device_goal_view", "eagle_op_goal_view"):
        assert re.search(r"^int %s\(" % name, head, re.M) and name in lib.EXPORTS, name
    assert lib.GOALVIEW_ROW_DTYPE == GR.ROW_DTYPE and lib.GOALVIEW_TOTALS_DTYPE == GR.TOTALS_DTYPE
    for k, v in (("BLOCKERS", GR.BLOCKERS), ("SLICES", GR.SLICES), ("OK", GR.OK), ("TOO_MANY", GR.TOO_MANY), ("PT_OK", GR.PT_OK), ("PT_ABSENT", GR.PT_ABSENT), ("PT_ROW", GR.PT_ROW),
                 ("PT_NEAR_LINE", GR.PT_NEAR_LINE), ("PT_FAR", GR.PT_FAR), ("FORM_DEFAULT", 0), ("FORM_DIRECT", GR.FORM_DIRECT), ("FORM_TABLE", GR.FORM_TABLE),
                 ("TIMES", len(lib.GOALVIEW_TIMES))):
        assert re.search(r"^#define EAGLE_GOALVIEW_%s %d\b" % (k, v), head, re.M) and getattr(lib, "GOALVIEW_" + k) in (v, lib.GOALVIEW_TIMES), k
    p = lib.goal_view_params()
    d = GR.goal_view_params(direction=0)
    assert all(getattr(p, k) == d[k] for k in d)
    assert "72 bytes" in head and "EagleGoalViewRow;                /* 56 bytes */" in head


BAD = [dict(radius=float("nan")), dict(keeper_radius=float("inf")), dict(min_depth=float("nan")), dict(max_range=float("inf")), dict(chance=float("nan")),
       dict(radius=-0.1), dict(radius=16.5), dict(keeper_radius=-1.0), dict(keeper_radius=17.0), dict(min_depth=0.99), dict(max_range=1.0), dict(max_range=0.5),
       dict(min_depth=5.0, max_range=5.0), dict(cells_per_metre=0), dict(cells_per_metre=3), dict(cells_per_metre=8), dict(direction=3), dict(group=2), dict(form=3)]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_resolve_refuses_what_the_library_refuses(kw):
    with pytest.raises(ValueError):
        GV.resolve(4, True, True, lib.OFFSIDE_DIR_RIGHT, True, **dict(dict(direction=lib.OFFSIDE_DIR_RIGHT), **kw))
    p = GR.goal_view_params(**dict(dict(direction=OR.DIR_RIGHT), **kw))
    with pytest.raises(ValueError):
        GR.check_params(p, 4, True)


def test_resolve_refuses_missing_results():
    R = lib.OFFSIDE_DIR_RIGHT
    with pytest.raises(ValueError, match="offside"):
        GV.resolve(4, False, True, None, True)                             # direction 0 without an offside result
    with pytest.raises(ValueError, match="no direction"):
        GV.resolve(4, False, True, 0, True)                                # ... with one that settled none
    with pytest.raises(ValueError, match="possession"):
        GV.resolve(4, True, True, R, False, direction=R, group=-1)         # the owner's group without a possession result
    with pytest.raises(ValueError, match="team mapping"):
        GV.resolve(4, False, False, R, True, direction=R)
    with pytest.raises(TypeError):
        GV.resolve(4, nothing=1)
    p = GV.resolve(4, False, True, lib.OFFSIDE_DIR_LEFT, False, group=-1)  # no grid: the group is not used
    assert (p.direction, p.grid_rows, p.radius, p.keeper_radius, p.min_depth, p.max_range, p.chance) == (0, 0, 0.4, 1.0, 1.0, 40.0, 0.3)
    p = GV.resolve(7, True, True, None, True, direction=R, cells_per_metre=4)
    assert (p.grid_row0, p.grid_rows, p.cells_per_metre) == (0, 7, 4)
    with pytest.raises(ValueError):
        GR.check_params(GR.goal_view_params(group=-1, grid_rows=2), 4, False)
    with pytest.raises(ValueError):
        GR.check_params(GR.goal_view_params(grid_row0=3, grid_rows=2), 4, True)
    with pytest.raises(ValueError):
        GR.goal_view(np.zeros((1, 1, 2)), [(GC.P, 1, 0)], None, GR.goal_view_params())     # no mapping


def _result(name):
    c, o = GC.BY_NAME[name], GC.reference(name)
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    return dict(o, params={}, direction=c["p"]["direction"], frames=np.arange(c["values"].shape[1]) * 2 + 100, columns=cols)


def test_join_shots_on_a_constructed_flights_result():
    d = _result("a_scene_towards_the_right_goal")
    rec = d["rows"][0]
    fl = np.zeros(4, lib.FLIGHT_DTYPE)
    blocked, free = GC.bits(rec[0]["ball_mask"])[0], [k for k in range(64) if k not in GC.bits(rec[0]["ball_mask"])][0]
    fl["shot"], fl["row0"], fl["vx"] = [2, 0, 1, 2], 0, [20.0, 20.0, 20.0, -20.0]
    fl["y_cross"] = [GR.Y0 + (blocked + 0.5) * GR.DY, 34.0, 29.0, GR.Y0 + (free + 0.25) * GR.DY]
    out = GV.join_shots(d, fl)
    assert [s["flight"] for s in out] == [0, 2, 3] and [s["group"] for s in out] == [0, 0, 1] and out[0]["frame"] == 100
    assert out[0]["lane"] == blocked and out[0]["lane_open"] is False and out[0]["mask"] == "%016x" % int(rec[0]["ball_mask"])
    assert out[0]["open"] == int(rec[0]["ball_open"]) * 2.0 ** -24 and out[0]["full"] == int(rec[0]["ball_full"]) * 2.0 ** -24 and 0 < out[0]["open"] < out[0]["full"] < 1.0
    assert out[1]["lane"] is None and out[1]["lane_open"] is None                               # beside the post
    assert out[2]["status"] == "far" and out[2]["lane"] == free and out[2]["lane_open"] is None and out[2]["full"] is None and out[2]["open"] == 0.0
    assert GV.lane(30.34) == 0 and GV.lane(37.66) is None and GV.lane(37.6599) == 63 and GV.lane(float("nan")) is None and GV.lane(30.3399) is None
    d2 = dict(d, direction=OR.DIR_LEFT)
    assert [s["group"] for s in GV.join_shots(d2, fl)] == [1, 1, 0]


def test_join_passes_and_totals_on_a_constructed_events_result():
    d = _result("ties_of_the_best_member_the_owner_and_the_totals")
    ev = np.zeros(4, lib.EVENT_DTYPE)
    ev["kind"] = [lib.EVENT_PASS, lib.EVENT_TURNOVER, lib.EVENT_PASS, lib.EVENT_PASS]
    ev["from_col"], ev["to_col"], ev["release_row"], ev["receive_row"], ev["row"] = [0, 0, 1, 3], [1, 4, 2, 5], [0, 0, 2, 0], [4, 1, 3, 1], [4, 1, 3, 1]
    out = GV.join_passes(d, ev)
    u = 2.0 ** -24
    assert [p["event"] for p in out] == [0, 2, 3] and out[0]["from_id"] == 1 and out[0]["to_id"] == 2 and out[0]["frame"] == 108
    assert out[0]["passer_open"] == int(d["open"][0, 0]) * u and out[0]["receiver_open"] == int(d["open"][1, 4]) * u
    assert out[0]["threat_added"] == out[0]["receiver_open"] - out[0]["passer_open"] > 0
    assert out[1]["receiver_open"] is None and out[1]["threat_added"] is None                   # the receiver is absent on that row
    assert out[2]["receiver_open"] is None and out[2]["to_id"] == 6                              # a keeper is no member
    t = GV.totals_json(d)
    assert [x["id"] for x in t] == [1, 2, 3, 4, 5] and t[1]["rows"] == 5 and t[1]["max_frame"] == 108 and t[1]["chance_rows"] == 4
    assert t[1]["mean_open"] == int(d["totals"][1]["sum_open"]) * u / 5 and t[4]["mean_open"] is None and t[4]["max_open"] is None and t[4]["max_frame"] is None
    j = GV.to_json(d, events=ev, cells=True)
    import json
    back = json.loads(json.dumps(j))
    assert back["rows"]["evaluated"] == [5, 5] and len(back["passes"]) == 3 and "shots" not in back and len(back["cells"]) == 5
    assert back["cells"][0]["groups"][0]["owner_id"] == 2 and back["cells"][3]["groups"][0]["owner_id"] is None and back["cells"][0]["groups"][0]["best_id"] == 2
