"""Ball possession and pass events on the GPU (include/eagle.h, eagle_op_possession / eagle_post_possession / eagle_post_possession_values /
eagle_post_device_possession / eagle_post_events; csrc/possession.hip): every output bit equals the numpy contract of tests/possession_ref.py — no
tolerances — for the constructed tables of tests/possession_cases.py; through a handle on tables eagle_postprocess built (host and device entries, a
second call replacing the first, merge_ids on and off); every refusal; rows == 0; the CLI's possession.json."""
import ctypes as C

import numpy as np
import pytest

import possession_cases as PC
import possession_ref as PR
import post_cases
import stitch_cases
from eagle_amd import lib, postprocess, weights

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in PC.CASES]


def _params(c):
    return lib.possession_params(c["fps"], c["radius"], c["min_hold"], c["max_gap"])


def _check(got, exp, what):
    cand, owner, dist, ev = got
    assert cand.dtype == np.int32 and np.array_equal(cand, exp["cand"]), (what, "cand", np.flatnonzero(cand != exp["cand"])[:5])
    assert owner.dtype == np.int32 and np.array_equal(owner, exp["owner"]), (what, "owner", np.flatnonzero(owner != exp["owner"])[:5])
    assert np.array_equal(np.isnan(dist), np.isnan(exp["dist"])) and np.array_equal(dist, exp["dist"], equal_nan=True), (what, "dist")
    assert len(ev) == len(exp["events"]), (what, len(ev), len(exp["events"]))
    for k in PR.EVENT_DTYPE.names:
        assert np.array_equal(ev[k], exp["events"][k]), (what, k)


@pytest.mark.parametrize("name", NAMES)
def test_op_possession_equals_contract(name):
    c = PC.BY_NAME[name]
    exp = PC.reference(name)
    cand, owner, dist, ev, n = lib.op_possession(c["values"], c["frames"], c["columns"], c["mapping"], _params(c))
    assert n == len(exp["events"])
    _check((cand, owner, dist, ev), exp, name)


def test_op_possession_cap_smaller_than_the_event_count_and_null_outputs():
    c = PC.BY_NAME["alternating_1025"]
    exp = PC.reference("alternating_1025")
    for cap in (0, 1, 700):
        cand, owner, dist, ev, n = lib.op_possession(c["values"], c["frames"], c["columns"], c["mapping"], _params(c), cap=cap)
        assert n == 1024 and len(ev) == cap and ev.tobytes() == exp["events"][:cap].tobytes()
    L = lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    values, frames = np.ascontiguousarray(c["values"]), np.ascontiguousarray(c["frames"])
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    ev = np.zeros(8, lib.EVENT_DTYPE)
    ev["row"] = -7
    n = C.c_int(-1)
    owner = np.zeros(1025, np.int32)
    assert L.eagle_op_possession(0, vp(values), vp(frames), vp(cols), 1025, len(cols), None, None, 0, C.byref(_params(c)), None, vp(owner), None, vp(ev), 5, C.byref(n)) == 0
    assert n.value == 1024 and np.array_equal(owner, exp["owner"]) and np.array_equal(ev["row"][:5], exp["events"]["row"][:5]) and (ev["row"][5:] == -7).all()
    assert (ev["kind"][:5] == lib.EVENT_UNKNOWN).all()                                   # no mapping: every event is of unknown kind


def test_op_possession_rows_0():
    cand, owner, dist, ev, n = lib.op_possession(np.zeros((3, 0, 2)), np.zeros(0, np.int32), [(PC.P, 1, 0), (PC.BALL, 0, 0), (PC.BALL, 0, 1)], {1: 0},
                                                 lib.possession_params(5))
    assert n == 0 and len(cand) == 0 and len(ev) == 0
    cand, owner, dist, ev, n = lib.op_possession(np.zeros((0, 0, 2)), np.zeros(0, np.int32), [], None, lib.possession_params(5))
    assert n == 0
    cand, owner, dist, ev, n = lib.op_possession(np.zeros((0, 3, 2)), np.arange(3), [], None, lib.possession_params(5))          # rows without a column
    assert n == 0 and (owner == -1).all() and (cand == -1).all() and np.isnan(dist).all()


# ---- through a handle ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


HANDLE_CASES = [("goalkeeper_fold", False), ("appear_vanish_return", False), ("ball_one_sighting", False), ("ball_none", False), ("empty", False),
                ("teams_head_inherits", True), ("teams_head_inherits", False), ("hand_over", True)]


@pytest.mark.parametrize("name,merge", HANDLE_CASES, ids=lambda v: str(v))
def test_handle_possession_equals_contract(handle, name, merge):
    case = post_cases.BY_NAME[name] if name in post_cases.BY_NAME else stitch_cases.BY_NAME[name]
    tm = case["team_mapping"] or None
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], tm, merge_ids=merge)
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        no_ball = bool(t.flags & lib.POST_NO_BALL)
        assert (no_ball or name not in ("ball_one_sighting", "ball_none")) and (rows == 0) == (name == "empty")
        d = C.c_void_p(1)
        assert handle.L.eagle_post_device_possession(t._t, C.byref(d)) == 0 and not d.value               # none before the first call
        assert handle.L.eagle_post_device_possession(t._t, None) == lib.E_INVALID
        n = C.c_int(-1)
        assert handle.L.eagle_post_events(t._t, None, 0, C.byref(n)) == 0 and n.value == 0
        assert handle.L.eagle_post_possession_values(t._t, None, None, None) == lib.E_INVALID           # no result yet
        owned = 0
        for fps, radius, min_hold, max_gap in ((case["fps"], 2.0, 2, None), (case["fps"], 1024.0, 1, 3), (5, 40.0, 2, 1000)):      # each call replaces the one before
            p = lib.possession_params(fps, radius, min_hold, max_gap)
            exp = PR.possession(values, t.rows, cols, t.team_mapping, fps, radius, min_hold, max_gap, no_ball=no_ball)
            got = handle.possession(t, p)
            _check(got, exp, (name, radius))
            owned += int((exp["owner"] >= 0).sum())
            assert handle.L.eagle_post_possession_values(t._t, None, None, None) == 0                     # any pointer may be NULL
            dev = handle.possession_device(t)
            assert dev and dev != t.device_values
            if rows:                                                                                     # the device entry: owner[rows] where it says
                back = np.zeros(rows, np.int32)
                assert handle.L.eagle_post_possession_values(t._t, None, back.ctypes.data_as(C.c_void_p), None) == 0 and np.array_equal(back, exp["owner"])
            if len(exp["events"]) > 1:                                                                   # eagle_post_events with a small cap
                ev = np.zeros(1, lib.EVENT_DTYPE)
                assert handle.L.eagle_post_events(t._t, ev.ctypes.data_as(C.c_void_p), 1, C.byref(n)) == 0 and n.value == len(exp["events"])
                assert ev.tobytes() == exp["events"][:1].tobytes()
            from eagle_amd import possession as po
            d_mod = po.possession(handle, t, fps, radius, min_hold, max_gap)
            players, teams, matrix = PR.aggregates(exp, t.rows, cols, fps)
            assert d_mod["players"] == players and d_mod["teams"] == teams and d_mod["pass_matrix"] == matrix
            assert [o["id"] for o in d_mod["owner"]] == [None if o < 0 else cols[o][1] for o in exp["owner"]]
        if name in ("ball_one_sighting", "ball_none", "empty"):
            assert owned == 0
    finally:
        t.close()


def test_refusals(handle):
    L = handle.L
    c = PC.BY_NAME["change_across_teams"]
    values, frames = np.ascontiguousarray(c["values"]), np.ascontiguousarray(c["frames"])
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    rows = len(frames)
    ids, vals = np.array([1, 2, 3], np.int32), np.array([0, 1, 0], np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    cand, owner, dist = np.full(rows, 77, np.int32), np.full(rows, 77, np.int32), np.full(rows, 7.0)
    ev = np.zeros(rows, lib.EVENT_DTYPE)
    ev["row"] = -7
    n = C.c_int(-9)
    good = lib.possession_params(5)

    def op(params=good, values_p=vp(values), frames_p=vp(frames), cols_p=vp(cols), n_p=C.byref(n), ev_p=vp(ev), cap=rows, nrows=rows, vals_p=vp(vals)):
        rc = L.eagle_op_possession(0, values_p, frames_p, cols_p, nrows, len(cols), vp(ids), vals_p, 3, None if params is None else C.byref(params),
                                   vp(cand), vp(owner), vp(dist), ev_p, cap, n_p)
        assert (cand == 77).all() and (owner == 77).all() and (dist == 7.0).all() and (ev["row"] == -7).all()
        return rc, L.eagle_last_error(None).decode()

    two_balls = cols.copy()
    two_balls[4]["kind"] = lib.POST_BALL
    unknown = cols.copy()
    unknown[5]["kind"] = 9
    negative = cols.copy()
    negative[0]["kind"] = -1
    same, back = frames.copy(), frames.copy()
    same[3] = same[2]
    back[4] = back[3] - 1
    P = lib.possession_params
    bad = [dict(params=None), dict(params=P(0)), dict(params=P(-5)), dict(params=P(5, max_gap=0)), dict(params=P(5, max_gap=-1)), dict(params=P(5, min_hold=0)),
           dict(params=P(5, min_hold=-2)), dict(params=P(5, radius=0.0)), dict(params=P(5, radius=-1.0)), dict(params=P(5, radius=float("nan"))),
           dict(params=P(5, radius=float("inf"))), dict(params=P(5, radius=np.nextafter(1024.0, 2000.0))), dict(values_p=None), dict(frames_p=None), dict(cols_p=None),
           dict(n_p=None), dict(ev_p=None), dict(cap=-1), dict(nrows=-1), dict(vals_p=None), dict(cols_p=vp(two_balls)), dict(cols_p=vp(unknown)),
           dict(cols_p=vp(negative)), dict(frames_p=vp(same)), dict(frames_p=vp(back))]
    for kw in bad:
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and msg, kw
    assert n.value == -9
    assert op(params=P(5, radius=1024.0), nrows=0)[0] == 0 and n.value == 0                # rows == 0: success, nothing written
    assert op(ev_p=None, cap=0, nrows=0)[0] == 0

    # the handle entry
    case = post_cases.BY_NAME["goalkeeper_fold"]
    t = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, case["team_mapping"])
    other = lib.Handle(batch=1, frame_h=140, frame_w=204)
    try:
        for p in (None, P(0), P(25, max_gap=0), P(25, min_hold=0), P(25, radius=0.0), P(25, radius=float("nan")), P(25, radius=1025.0)):
            assert L.eagle_post_possession(handle._h, t._t, None if p is None else C.byref(p)) == lib.E_INVALID and L.eagle_last_error(handle._h)
        assert L.eagle_post_possession(handle._h, None, C.byref(good)) == lib.E_INVALID
        assert L.eagle_post_possession(None, t._t, C.byref(good)) == lib.E_INVALID
        assert L.eagle_post_possession(other._h, t._t, C.byref(good)) == lib.E_INVALID and b"another handle" in L.eagle_last_error(other._h)
        d = C.c_void_p(1)
        assert L.eagle_post_device_possession(t._t, C.byref(d)) == 0 and not d.value            # a refused call leaves no result
        assert L.eagle_post_possession_values(None, None, None, None) == lib.E_INVALID
        assert L.eagle_post_events(t._t, None, 1, C.byref(n)) == lib.E_INVALID and L.eagle_post_events(t._t, None, 0, None) == lib.E_INVALID
        assert L.eagle_post_events(t._t, None, -1, C.byref(n)) == lib.E_INVALID and L.eagle_post_events(None, None, 0, C.byref(n)) == lib.E_INVALID
        assert len(handle.possession(t, good)[1]) == len(t.rows)                               # the handle still works
    finally:
        t.close()
        other.close()


def test_cli_possession(tmp_path):
    import json
    import os
    from eagle_amd import cli, possession as po
    out = str(tmp_path / "out")
    assert cli.main(["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed", "--merge-ids", "--possession"]) == 0
    rows = json.load(open(os.path.join(out, "processed_data.json")))
    j = json.load(open(os.path.join(out, "possession.json")))
    d = po.from_json(j)
    assert set(d) == {"owner", "events", "players", "teams", "pass_matrix"} and len(d["owner"]) == len(rows)
    assert po.from_json(json.loads(json.dumps(po.to_json(d)))) == d
    assert all(set(p) == {"id", "type", "rows", "seconds", "passes_made", "passes_received", "turnovers_lost", "turnovers_won"} for p in d["players"])
    assert sum(p["rows"] for p in d["players"]) == sum(o["id"] is not None for o in d["owner"])
    assert sum(p["passes_made"] for p in d["players"]) == sum(e["kind"] == "pass" for e in d["events"]) == sum(d["pass_matrix"].values())
