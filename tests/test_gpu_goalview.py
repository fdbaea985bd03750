"""Goal view on the GPU (include/eagle.h, eagle_op_goal_view / eagle_post_goal_view and its accessors; csrc/goalview.hip): every output bit equals the
contract of tests/goalview_ref.py — no tolerances, records compared as bytes — on the constructed tables of tests/goalview_cases.py, in both forms of the
grid kernel's weights; NULL outputs; every refusal leaves poisoned outputs alone; through a handle on tables eagle_postprocess built: equal to the
operator entry and the contract, the accessors before the call, a second call, the owner's group with and without a possession result, the offside
result's direction with and without one, the table's positions, events and flights afterwards; the CLI's goal_view.json and goal_view.npy on a small
synthetic-weights clip."""
import ctypes as C

import numpy as np
import pytest

import goalview_cases as GC
import goalview_ref as GR
import offside_ref as OR
import post_cases
from eagle_amd import goalview as GV, lib, postprocess, weights

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in GC.CASES]
FORMS = (lib.GOALVIEW_FORM_DEFAULT, lib.GOALVIEW_FORM_DIRECT, lib.GOALVIEW_FORM_TABLE)


def _params(p, **more):
    return lib.goal_view_params(**dict(p, **more))


def _equal(got, exp, what):
    for k in GC.PARTS:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
        if got[k].tobytes() != exp[k].tobytes():
            where = np.argwhere(got[k] != exp[k])[:5]
            raise AssertionError((what, k, where.tolist(), [(got[k][tuple(w)], exp[k][tuple(w)]) for w in where]))


def _op(c, **kw):
    v = c["values"]
    if c["no_ball"]:                                                      # the operator entry takes no table flags: a table flagged NO_BALL is one whose ball is absent
        v = v.copy()
        v[[k for k, col in enumerate(c["columns"]) if col[0] == GC.BALL and not col[2]]] = np.nan
    return lib.op_goal_view(v, c["columns"], c["mapping"], _params(c["p"], **kw), c["owner"])


@pytest.mark.parametrize("name", NAMES)
def test_op_goal_view_equals_contract(name):
    c, exp = GC.BY_NAME[name], GC.reference(name)
    for form in FORMS:
        _equal(_op(c, form=form), exp, (name, form))


def test_op_times():
    c = GC.BY_NAME["seventy_rows_with_holes_and_an_owner"]
    for form in (lib.GOALVIEW_FORM_DIRECT, lib.GOALVIEW_FORM_TABLE):
        got = lib.op_goal_view(c["values"], c["columns"], c["mapping"], _params(c["p"], form=form), c["owner"], times=True)
        _equal(got, GC.reference(c["name"]), "times")
        t = got["times"]
        assert set(t) == set(lib.GOALVIEW_TIMES) and all(v >= 0.0 for v in t.values()) and t["total"] > 0.0 and t["grid"] > 0.0
        assert (t["table"] > 0.0) == (form == lib.GOALVIEW_FORM_TABLE)


KEYS = ("rows", "open", "mask", "status", "totals", "grid")


def _poisoned(c, nm):
    rows, R = c["values"].shape[1], c["p"]["cells_per_metre"]
    rec, tot = np.zeros((rows, 2), lib.GOALVIEW_ROW_DTYPE), np.zeros(nm, lib.GOALVIEW_TOTALS_DTYPE)
    rec["status"], tot["col"] = -7, -7
    return [rec, np.full((nm, rows), -7, np.int32), np.full((nm, rows), 7, np.uint64), np.full((nm, rows), 77, np.uint8), tot,
            np.full((c["p"]["grid_rows"], 68 * R, 105 * R), 77, np.uint8)]


def _raw_call(L, c, p, outs, rows=None, values=True, columns=True, cols_arr=None, mapping="case", owner="case", n_team=None, count=True):
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    v = np.ascontiguousarray(c["values"])
    cols = np.array([(k, i, vd, 0) for k, i, vd in c["columns"]], lib.POSTCOL_DTYPE) if cols_arr is None else cols_arr
    mapping = c["mapping"] if isinstance(mapping, str) else mapping
    pairs = None if mapping is None else list(mapping.items() if isinstance(mapping, dict) else mapping)
    ids = None if pairs is None else np.ascontiguousarray([k for k, _ in pairs], np.int32)
    vals = None if pairs is None else np.ascontiguousarray([t for _, t in pairs], np.int32)
    own = c["owner"] if isinstance(owner, str) else owner
    own = None if own is None else np.ascontiguousarray(own, np.int32)
    nm = C.c_int(-7)
    rc = L.eagle_op_goal_view(0, vp(v) if values else None, vp(cols) if columns else None, v.shape[1] if rows is None else rows, len(cols), vp(ids), vp(vals),
                              (0 if pairs is None else len(pairs)) if n_team is None else n_team, vp(own), None if p is None else C.byref(p), *[vp(o) for o in outs],
                              C.byref(nm) if count else None, None)
    return rc, L.eagle_last_error(None).decode(), nm.value


def test_op_null_outputs():
    L = lib.load()
    name = "ties_of_the_best_member_the_owner_and_the_totals"
    c, exp = GC.BY_NAME[name], GC.reference(name)
    p = _params(c["p"])
    assert _raw_call(L, c, p, [None] * 6, count=False)[0] == 0           # every output may be NULL
    rc, _, nm = _raw_call(L, c, p, [None] * 6)
    assert rc == 0 and nm == len(exp["totals"]) == 5
    for i, k in enumerate(KEYS):                                          # each alone
        outs = [None] * 6
        outs[i] = _poisoned(c, nm)[i]
        assert _raw_call(L, c, p, outs)[0] == 0, k
        assert outs[i].tobytes() == exp[k].tobytes(), k
    q = _params(c["p"], grid_rows=0, group=0)                             # no grid: the grid buffer is not touched
    outs = _poisoned(c, nm)
    assert _raw_call(L, c, q, outs, owner=None)[0] == 0 and (outs[5] == 77).all() and outs[1].tobytes() == exp["open"].tobytes()
    assert (outs[0]["owner_col"] == -1).all() and (outs[0]["best_col"] == exp["rows"]["best_col"]).all()


def test_op_refusals_leave_the_outputs_alone():
    L = lib.load()
    c = GC.BY_NAME["ties_of_the_best_member_the_owner_and_the_totals"]
    P = lambda **kw: _params(c["p"], **kw)
    outs = _poisoned(c, 5)
    before = [o.copy() for o in outs]
    nan, inf = float("nan"), float("inf")
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    unknown, two_balls = cols.copy(), cols.copy()
    unknown[2]["kind"] = 9
    two_balls[2]["kind"] = lib.POST_BALL
    reserved = P()
    reserved.reserved[1] = 1
    bad = [(dict(p=None), "NULL"), (dict(p=P(radius=nan)), "radius"), (dict(p=P(keeper_radius=inf)), "keeper_radius"), (dict(p=P(min_depth=nan)), "min_depth"),
           (dict(p=P(max_range=inf)), "max_range"), (dict(p=P(chance=nan)), "chance"), (dict(p=P(radius=-0.5)), "radius"), (dict(p=P(radius=16.25)), "radius"),
           (dict(p=P(keeper_radius=-1.0)), "keeper_radius"), (dict(p=P(keeper_radius=20.0)), "keeper_radius"), (dict(p=P(min_depth=0.5)), "min_depth"),
           (dict(p=P(max_range=1.0)), "max_range"), (dict(p=P(min_depth=3.0, max_range=2.0)), "max_range"), (dict(p=P(max_range=2000.0)), "max_range"),
           (dict(p=P(chance=-0.1)), "chance"), (dict(p=P(cells_per_metre=0)), "cells_per_metre"), (dict(p=P(cells_per_metre=3)), "cells_per_metre"),
           (dict(p=P(cells_per_metre=8)), "cells_per_metre"), (dict(p=P(direction=0)), "offside"), (dict(p=P(direction=3)), "direction"), (dict(p=P(group=2)), "group"),
           (dict(p=P(group=-2)), "group"), (dict(p=P(form=3)), "form"), (dict(p=reserved), "reserved"), (dict(p=P(grid_rows=-1)), "grid"), (dict(p=P(grid_row0=-1)), "grid"),
           (dict(p=P(grid_row0=1)), "grid"), (dict(p=P(grid_rows=6)), "grid"), (dict(p=P(), owner=None), "possession"), (dict(p=P(), mapping=None), "mapping"),
           (dict(p=P(), values=False), "bad argument"), (dict(p=P(), columns=False), "bad argument"), (dict(p=P(), rows=-1), "bad argument"),
           (dict(p=P(), n_team=-1), "bad argument"), (dict(p=P(), cols_arr=unknown), "unknown kind"), (dict(p=P(), cols_arr=two_balls), "both the ball")]
    for kw, word in bad:
        rc, msg, nm = _raw_call(L, c, kw.pop("p"), outs, **kw)
        assert rc == lib.E_INVALID and word in msg, (kw, word, msg)
        assert nm == -7 and all(a.tobytes() == b.tobytes() for a, b in zip(outs, before)), word         # nothing launched, nothing written
    assert _raw_call(L, c, P(), outs)[0] == 0 and all(a.tobytes() != b.tobytes() for a, b in zip(outs, before))     # the same buffers are written by a good call


# ---- through a handle ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


def _records(n, players=8, keepers=2, seed=11):
    """n records of `players` players and `keepers` goalkeepers on a slow random walk in the right half, team 0 (even detections) attacking x = 105; the
    ball sits on a player for three frames and hops to another (ids are detection index + 1)"""
    r = np.random.default_rng(seed)
    k = players + keepers + 1
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = k, 1, 1
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    x0 = np.array([r.uniform(60, 95) if j % 2 == 0 else r.uniform(75, 102) for j in range(players)] + [4.0, 103.0][:keepers] + [0.0])
    pos = np.stack([x0, r.uniform(20, 48, k)], 1)[None] + np.cumsum(r.normal(0, 0.7, (n, k, 2)), 0)
    holder = np.repeat(r.integers(0, players, n // 3 + 1), 3)[:n]
    pos[:, k - 1] = pos[np.arange(n), holder]
    pos = np.clip(pos, 0, [105, 68])
    d, j = recs["det"], np.arange(k)
    d["reported"][:, :k], d["in_bounds"][:, :k], d["conf"][:, :k] = 1, 1, 0.9
    d["cls"][:, :k] = np.where(j == k - 1, 2, np.where(j >= players, 1, 0))[None]
    d["id"][:, :k] = (j + 1)[None]
    d["bx1"][:, :k], d["bx2"][:, :k], d["by1"][:, :k], d["by2"][:, :k] = (4 * j)[None], (4 * j + 3)[None], 300, 340
    d["pitch_x"][:, :k], d["pitch_y"][:, :k] = pos[:, :, 0].astype(np.int32), pos[:, :, 1].astype(np.int32)
    return recs


MAPPING = {i + 1: i % 2 for i in range(8)}


def _contract(t, p, owner=None):
    return GR.goal_view(np.array(t.values), _columns(t), t.team_mapping, p, owner, bool(t.flags & lib.POST_NO_BALL))


def test_handle_goal_view_equals_operator_entry_and_contract(handle):
    L = handle.L
    t = postprocess.process_data(handle, _records(24), 25, 1280, MAPPING)
    try:
        rows, cols, raw = len(t.rows), _columns(t), t.values.copy()
        assert rows == 24
        # before the call: NULLs, zeros and EAGLE_E_INVALID
        assert handle.goal_view_device(t) == (None,) * 6 + (0,) * 4
        assert L.eagle_post_goal_view_values(t._t, None, None, None, None, None, None) == lib.E_INVALID and b"no goal view" in L.eagle_last_error(handle._h)
        with pytest.raises(lib.EagleError):
            handle.goal_view_values(t)
        R, LEFT = OR.DIR_RIGHT, OR.DIR_LEFT
        # the owner's group and the offside result's direction are refused while the table has neither, and leave no result
        for p, word in ((lib.goal_view_params(R, group=-1, grid_rows=rows), b"possession"), (lib.goal_view_params(0), b"offside")):
            assert L.eagle_post_goal_view(handle._h, t._t, C.byref(p)) == lib.E_INVALID and word in L.eagle_last_error(handle._h), word
        with pytest.raises(ValueError, match="offside"):
            GV.goal_view(handle, t)
        with pytest.raises(ValueError, match="possession"):
            GV.goal_view(handle, t, grid=True, direction=R, group=-1)
        assert handle.goal_view_device(t)[0] is None
        # a fixed group, a forced direction, no possession: no owner anywhere
        p = GR.goal_view_params(R, group=0, grid_row0=2, grid_rows=5)
        got = handle.goal_view(t, lib.goal_view_params(**p))
        exp = _contract(t, p)
        _equal(got, exp, "group 0")
        _equal(lib.op_goal_view(raw, cols, t.team_mapping, lib.goal_view_params(**p)), got, "operator entry")
        assert got["grid_row0"] == 2 and (got["rows"]["owner_col"] == -1).all() and (got["status"] == GR.PT_OK).any() and (got["mask"] != 0).any() and got["grid"].any()
        dev = handle.goal_view_device(t)
        assert all(dev[:6]) and len(set(dev[:6])) == 6 and dev[6:] == (8, 2, 5, 1)
        assert L.eagle_post_goal_view_values(t._t, None, None, None, None, None, None) == 0               # any pointer may be NULL
        # possession and offside, then the owner's group and the settled direction
        cand, owner, dist, ev = handle.possession(t, lib.possession_params(25, 1024.0, 1, 1000))
        rec, mg, tot, clip = handle.offside(t, lib.offside_params())
        flights = handle.ball_flights(t, lib.flight_params(25))
        settled = int(clip[0]["direction"])
        assert settled == R and (owner >= 0).any()
        p2 = GR.goal_view_params(settled, group=-1, grid_rows=rows, cells_per_metre=2, chance=0.1)
        got2 = handle.goal_view(t, lib.goal_view_params(**dict(p2, direction=0)))
        _equal(got2, _contract(t, p2, owner), "the owner's group, the offside result's direction")
        _equal(lib.op_goal_view(raw, cols, t.team_mapping, lib.goal_view_params(**p2), owner), got2, "operator entry with an owner")
        _equal(handle.goal_view_values(t), got2, "kept")                                                  # the second call replaced the first
        assert (got2["rows"]["owner_col"] >= 0).any() and got2["grid"].shape == (rows, 136, 210) and handle.goal_view_device(t)[6:] == (8, 0, rows, 2)
        d = GV.goal_view(handle, t, grid=False, chance=0.1)                                               # the module's call: direction 0 resolved, the joins
        assert d["direction"] == settled and d["grid"].shape[0] == 0 and d["open"].tobytes() == got2["open"].tobytes()
        j = GV.to_json(d, flights=flights["flights"], events=ev, cells=True)
        assert len(j["passes"]) == int((ev["kind"] == lib.EVENT_PASS).sum()) and len(j["totals"]) == 8 and len(j["cells"]) == rows
        assert len(j["shots"]) == int((flights["flights"]["shot"] >= 1).sum())
        # a refused call leaves the result in place
        bad = lib.goal_view_params(R, radius=float("nan"))
        assert L.eagle_post_goal_view(handle._h, t._t, C.byref(bad)) == lib.E_INVALID and b"radius" in L.eagle_last_error(handle._h)
        _equal(handle.goal_view_values(t), dict(d, grid=d["grid"]), "after a refusal")
        # towards the other goal: another result
        got3 = handle.goal_view(t, lib.goal_view_params(LEFT))
        _equal(got3, _contract(t, GR.goal_view_params(LEFT), owner), "left")
        assert got3["open"].tobytes() != got2["open"].tobytes()
        # nothing else of the table has changed
        t._values = None
        assert t.values.tobytes() == raw.tobytes()
        assert handle.events(t).tobytes() == ev.tobytes() and handle.possession_values(t)[1].tobytes() == owner.tobytes()
        again = handle.ball_flight_values(t)
        assert all(again[k].tobytes() == flights[k].tobytes() for k in ("seg", "flags", "fitted", "velocity", "flights", "kicks", "totals"))
        assert handle.offside(t, lib.offside_params())[0].tobytes() == rec.tobytes()
    finally:
        t.close()


def test_handle_refusals_tables_without_rows_or_mapping(handle):
    L = handle.L
    good = lib.goal_view_params(OR.DIR_RIGHT)
    other = lib.Handle(batch=1, frame_h=140, frame_w=204)
    case = post_cases.BY_NAME["goalkeeper_fold"]
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], case["team_mapping"])
    u = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], None)
    e = postprocess.process_data(handle, post_cases.records_of(post_cases.BY_NAME["empty"]), 25, 1280, {1: 0})
    try:
        assert L.eagle_post_goal_view(handle._h, None, C.byref(good)) == lib.E_INVALID and L.eagle_post_goal_view(None, t._t, C.byref(good)) == lib.E_INVALID
        assert L.eagle_post_goal_view(other._h, t._t, C.byref(good)) == lib.E_INVALID and b"another handle" in L.eagle_last_error(other._h)
        assert L.eagle_post_goal_view(handle._h, t._t, None) == lib.E_INVALID and b"NULL" in L.eagle_last_error(handle._h)
        assert L.eagle_post_goal_view(handle._h, u._t, C.byref(good)) == lib.E_INVALID and b"mapping" in L.eagle_last_error(handle._h)
        over = lib.goal_view_params(OR.DIR_RIGHT, grid_rows=len(t.rows) + 1)
        assert L.eagle_post_goal_view(handle._h, t._t, C.byref(over)) == lib.E_INVALID and b"grid" in L.eagle_last_error(handle._h)
        assert handle.goal_view_device(t)[0] is None and handle.goal_view_device(u)[0] is None
        assert L.eagle_post_goal_view_values(None, None, None, None, None, None, None) == lib.E_INVALID
        assert L.eagle_post_device_goal_view(t._t, None, None, None, None, None, None, None, None, None, None) == lib.E_INVALID
        p = GR.goal_view_params(OR.DIR_RIGHT, grid_rows=len(t.rows))
        got = handle.goal_view(t, lib.goal_view_params(**p))
        _equal(got, _contract(t, p), "goalkeeper_fold")
        print("goalkeeper_fold: statuses", np.unique(got["status"]).tolist(), "blockers", got["rows"]["n_blockers"].tolist())
        nb = postprocess.process_data(handle, post_cases.records_of(post_cases.BY_NAME["ball_none"]), 25, 1280, {i: i % 2 for i in range(64)})
        try:                                                                                              # a table flagged NO_BALL: the ball is absent on every row
            assert nb.flags & lib.POST_NO_BALL and len(nb.rows)
            q = GR.goal_view_params(OR.DIR_LEFT, group=1, grid_rows=1)
            got = handle.goal_view(nb, lib.goal_view_params(**q))
            _equal(got, _contract(nb, q), "ball_none")
            assert (got["rows"]["ball_status"] == GR.PT_ABSENT).all()
        finally:
            nb.close()
        assert len(e.rows) == 0
        empty = handle.goal_view(e, good)                                                                 # a table without rows: success, nothing to read
        assert empty["rows"].shape == (0, 2) and empty["open"].shape[1] == 0 and empty["grid"].shape[0] == 0
        # a table that carries the result is derived: the stages that move positions refuse it
        sp, st = lib.smooth_params(int(case["fps"]), window=2), lib.stab_params(int(case["fps"]), window=2)
        assert L.eagle_post_smooth_tracks(handle._h, t._t, C.byref(sp)) == lib.E_INVALID and b"goal view" in L.eagle_last_error(handle._h)
        assert L.eagle_post_stabilise(handle._h, t._t, C.byref(st)) == lib.E_INVALID and b"goal view" in L.eagle_last_error(handle._h)
    finally:
        t.close()
        u.close()
        e.close()
        other.close()


def test_cli_goal_view(tmp_path):
    import json
    import os
    from eagle_amd import cli
    base = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--processed", "--merge-ids", "--possession", "--ball-flights", "--offside"]
    plain, out, bare = str(tmp_path / "plain"), str(tmp_path / "out"), str(tmp_path / "bare")
    assert cli.main(base + ["--out", plain]) == 0
    assert cli.main(base + ["--out", out, "--goal-view", "--goal-view-direction", "right", "--goal-view-cells", "--goal-view-map", "--goal-view-grid", "2"]) == 0
    assert cli.main([a for a in base if a not in ("--possession", "--ball-flights", "--offside")] + ["--out", bare, "--goal-view", "--goal-view-direction", "left", "--goal-view-map"]) == 0
    load = lambda d, n: json.load(open(os.path.join(d, n)))
    assert not os.path.exists(os.path.join(plain, "goal_view.json")) and "goal_view" not in load(plain, "metadata.json")               # only with the flag
    for name in ("processed_data.json", "raw_data.json", "possession.json", "ball_flights.json", "offside.json"):                   # everything else is what it was
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(plain, name), "rb").read(), name
    meta, j, b = load(out, "metadata.json"), load(out, "goal_view.json"), load(bare, "goal_view.json")
    assert meta["goal_view"] is True and {k: v for k, v in meta.items() if k not in ("goal_view", "seconds")} == {k: v for k, v in load(plain, "metadata.json").items() if k != "seconds"}
    assert set(j) == {"params", "direction", "unit", "rows", "totals", "shots", "passes", "cells"} and set(b) == {"params", "direction", "unit", "rows", "totals"}
    assert j["params"] == {"direction": 1, "group": -1, "cells_per_metre": 2, "form": 0, "radius": 0.4, "keeper_radius": 1.0, "min_depth": 1.0, "max_range": 40.0, "chance": 0.3}
    assert (j["direction"], b["direction"], b["params"]["group"], b["params"]["cells_per_metre"]) == (1, 2, 0, 1)
    rows = load(out, "processed_data.json")
    grid, bgrid = np.load(os.path.join(out, "goal_view.npy")), np.load(os.path.join(bare, "goal_view.npy"))
    assert grid.shape == (len(rows), 136, 210) and grid.dtype == np.uint8 and bgrid.shape == (len(rows), 68, 105)
    assert len(j["cells"]) == len(rows) and sum(j["rows"]["evaluated"]) + sum(j["rows"]["too_many"]) == 2 * len(rows)
    assert len(j["passes"]) == sum(1 for e in load(out, "possession.json")["events"] if e["kind"] == "pass") and len(j["shots"]) == len(load(out, "ball_flights.json")["shots"])
    for t in j["totals"]:
        assert set(t) == {"id", "group", "rows", "mean_open", "max_open", "max_frame", "chance_rows"} and (t["rows"] == 0) == (t["max_open"] is None)
        assert t["max_open"] is None or 0.0 <= t["mean_open"] <= t["max_open"] < 3.2
    for c in j["cells"]:
        assert set(c) == {"frame", "groups"} and len(c["groups"]) == 2 and set(c["groups"][0]) == {"blockers", "too_many", "ball", "ball_open", "best_id", "best_open", "owner_id", "owner_open"}
