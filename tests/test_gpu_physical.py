"""The physical report on the GPU (include/eagle.h, eagle_op_physical / eagle_post_physical / eagle_post_physical_values / eagle_post_physical_totals /
eagle_post_physical_efforts / eagle_post_device_physical; csrc/physical.hip): every output bit equals the numpy contract of tests/physical_ref.py — no
tolerances, the per-row arrays compared as bit patterns — for the constructed tables of tests/physical_cases.py; through a handle on tables
eagle_postprocess built, against the operator entry fed the same velocities (a second call replacing the first, merge_ids on and off); every refusal;
rows == 0 and no person; the consistency with eagle_amd.control.kinematics; the CLI's physical.json."""
import ctypes as C

import numpy as np
import pytest

import physical_cases as PC
import physical_ref as PR
import post_cases
import stitch_cases
from eagle_amd import lib, postprocess, weights

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in PC.CASES]
BITS = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _params(c):
    return lib.load_params(c["fps"], c["max_gap"], c["zone_edges"], c["effort_speed"], c["accel"], c["min_frames"])


def _check(got, exp, what):
    speed, accel, zone, totals, ev = got
    assert speed.shape == exp["speed"].shape and accel.shape == exp["accel"].shape and zone.shape == exp["zone"].shape, (what, speed.shape)
    assert np.array_equal(BITS(speed), BITS(exp["speed"])), (what, "speed", np.argwhere(BITS(speed) != BITS(exp["speed"]))[:5])
    assert np.array_equal(BITS(accel), BITS(exp["accel"])), (what, "accel", np.argwhere(BITS(accel) != BITS(exp["accel"]))[:5])
    assert zone.dtype == np.uint8 and np.array_equal(zone, exp["zone"]), (what, "zone", np.argwhere(zone != exp["zone"])[:5])
    assert len(totals) == len(exp["totals"]) and len(ev) == len(exp["efforts"]), (what, len(totals), len(ev), len(exp["efforts"]))
    for k in PR.TOTALS_DTYPE.names:
        assert np.array_equal(totals[k], exp["totals"][k]), (what, k, totals[k], exp["totals"][k])
    for k in PR.EFFORT_DTYPE.names:                                                                       # field for field, order included
        assert np.array_equal(ev[k], exp["efforts"][k]), (what, k)
    assert np.array_equal(BITS(totals["top_speed"]), BITS(exp["totals"]["top_speed"])) and ev.tobytes() == exp["efforts"].tobytes()


def _empty(exp):
    """what the library reports where the contract has rows or persons but not both: nothing"""
    out = dict(exp)
    out["totals"] = exp["totals"][:0]
    out["speed"], out["accel"], out["zone"] = (exp[k].reshape(0, exp[k].shape[1]) for k in ("speed", "accel", "zone"))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_op_physical_equals_contract(name):
    c = PC.BY_NAME[name]
    exp = PC.reference(name)
    speed, accel, zone, totals, ev, n = lib.op_physical(c["velocities"], c["frames"], c["columns"], _params(c))
    assert n == len(exp["efforts"])
    _check((speed, accel, zone, totals, ev), exp, name)


def test_op_physical_cap_smaller_than_the_counts_and_null_outputs():
    name = "accelerations_alternate"
    c, exp = PC.BY_NAME[name], PC.reference(name)
    n_all = len(exp["efforts"])
    assert n_all > 400
    for cap in (0, 1, 300):
        got = lib.op_physical(c["velocities"], c["frames"], c["columns"], _params(c), cap=cap)
        assert got[5] == n_all and len(got[4]) == cap and got[4].tobytes() == exp["efforts"][:cap].tobytes()
    L = lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    vel, frames = np.ascontiguousarray(c["velocities"]), np.ascontiguousarray(c["frames"])
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    tot = np.zeros(2, lib.LOAD_TOTALS_DTYPE)
    tot["col"] = -7
    zone = np.zeros((2, len(frames)), np.uint8)
    npers, nev = C.c_int(-1), C.c_int(-1)
    assert L.eagle_op_physical(0, vp(vel), vp(frames), vp(cols), len(frames), len(cols), C.byref(_params(c)), None, None, vp(zone), vp(tot), 1, C.byref(npers),
                               None, 0, C.byref(nev)) == 0
    assert npers.value == 2 and nev.value == n_all and np.array_equal(zone, exp["zone"]) and tot[0].tobytes() == exp["totals"][0].tobytes() and tot[1]["col"] == -7


def test_op_physical_rows_0_and_no_person():
    cols3 = [(PC.P, 1, 0), (PC.BALL, 0, 0), (PC.G, 2, 0)]
    speed, accel, zone, totals, ev, n = lib.op_physical(np.zeros((3, 0, 2)), np.zeros(0, np.int32), cols3, lib.load_params(5))
    assert n == 0 and len(totals) == 0 and len(ev) == 0 and speed.size == 0
    assert lib.op_physical(np.zeros((0, 0, 2)), np.zeros(0, np.int32), [], lib.load_params(5))[5] == 0
    speed, accel, zone, totals, ev, n = lib.op_physical(np.ones((2, 3, 2)), np.arange(3), [(PC.BALL, 0, 0), (PC.P, 4, 1)], lib.load_params(5))     # rows without a person
    assert n == 0 and len(totals) == 0 and speed.shape == (0, 3)


# ---- through a handle ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


HANDLE_CASES = [("goalkeeper_fold", False), ("appear_vanish_return", False), ("ball_none", False), ("empty", False), ("teams_head_inherits", True), ("hand_over", True),
                ("hand_over", False)]
CALLS = ((None, None, PR.ZONE_EDGES, PR.EFFORT_SPEED, 2.0, None), (3, 3, (0.25, 0.5, 1.0, 2.0), (0.5, 1.0), 0.25, (1, 1)), (5, 1000, (1.0, 3.0, 6.0, 9.0), (3.0, 1.0), 1.0, (2, 1)))


@pytest.mark.parametrize("name,merge", HANDLE_CASES, ids=lambda v: str(v))
def test_handle_physical_equals_operator_entry_and_contract(handle, name, merge):
    case = post_cases.BY_NAME[name] if name in post_cases.BY_NAME else stitch_cases.BY_NAME[name]
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], case["team_mapping"] or None, merge_ids=merge)
    try:
        cols, rows = _columns(t), len(t.rows)
        a, b = C.c_void_p(1), C.c_void_p(1)
        assert handle.L.eagle_post_device_physical(t._t, C.byref(a), C.byref(b)) == 0 and not a.value and not b.value      # none before the first call
        assert handle.L.eagle_post_device_physical(t._t, None, C.byref(b)) == lib.E_INVALID
        n = C.c_int(-1)
        assert handle.L.eagle_post_physical_totals(t._t, None, 0, C.byref(n)) == 0 and n.value == 0
        assert handle.L.eagle_post_physical_efforts(t._t, None, 0, C.byref(n)) == 0 and n.value == 0
        assert handle.L.eagle_post_physical_values(t._t, None, None, None) == lib.E_INVALID                # no result yet
        good = lib.load_params(case["fps"])
        assert handle.L.eagle_post_physical(handle._h, t._t, C.byref(good)) == lib.E_INVALID and b"no velocities" in handle.L.eagle_last_error(handle._h)
        vel = handle.velocities(t, case["fps"])
        assert (rows == 0) == (name == "empty")
        persons = len(PR.layout(cols))
        for fps, max_gap, edges, espeed, accel, minf in CALLS:                                               # each call replaces the one before
            fps = case["fps"] if fps is None else fps
            p = lib.load_params(fps, max_gap, edges, espeed, accel, minf)
            exp = PR.physical(vel, t.rows, cols, fps, max_gap, edges, espeed, accel, minf)
            if rows == 0 or persons == 0:
                exp = _empty(exp)
            got = handle.physical(t, p)
            _check(got, exp, (name, fps))
            op = lib.op_physical(vel, t.rows, cols, p)                                                       # the operator entry fed the same velocities
            _check(op[:5], exp, (name, fps, "op"))
            assert handle.L.eagle_post_physical_values(t._t, None, None, None) == 0                         # any pointer may be NULL
            d_speed, d_zone = handle.physical_device(t)
            assert d_speed and d_zone and d_speed != t.device_values and d_zone == d_speed + 16 * persons * rows
            if len(exp["efforts"]) > 1:                                                                      # a small cap
                ev = np.zeros(1, lib.LOAD_EFFORT_DTYPE)
                assert handle.L.eagle_post_physical_efforts(t._t, ev.ctypes.data_as(C.c_void_p), 1, C.byref(n)) == 0 and n.value == len(exp["efforts"])
                assert ev.tobytes() == exp["efforts"][:1].tobytes()
            from eagle_amd import physical as ph
            d = ph.physical(handle, t, fps, max_gap, edges, espeed, accel, minf)
            assert [{k: pl[k] for k in w} for pl, w in zip(d["players"], PR.aggregates(exp, cols, fps))] == PR.aggregates(exp, cols, fps)
            assert all(sum(pl["zone_distance_q"]) == pl["distance_q"] for pl in d["players"]) and len(d["efforts"]) == len(exp["efforts"])
    finally:
        t.close()                                                                                           # eagle_post_free after a replaced result


def _kin_distance(sp, f, fps, gap):
    """eagle_amd.control.kinematics' sum for one column, restated"""
    ok = np.isfinite(sp)
    step = ok[1:] & ok[:-1] & (np.diff(f) <= gap)
    return float(np.sum(0.5 * (sp[1:] + sp[:-1])[step] * (np.diff(f)[step] / float(fps)))), int(step.sum())


def test_consistent_with_kinematics(handle):
    from eagle_amd import control as ct, physical as ph
    case = post_cases.BY_NAME["goalkeeper_fold"]
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], case["team_mapping"] or None)
    try:
        kin = ct.kinematics(handle, t, case["fps"])
        d = ph.physical(handle, t, case["fps"])
        assert len(kin["players"]) == len(d["players"]) > 0
        f = np.asarray(t.rows, np.int64)
        moved = 0
        for c, (k, pl) in zip(PR.layout(_columns(t)), zip(kin["players"], d["players"])):
            assert k["id"] == pl["id"] and k["type"] == pl["type"]
            assert np.float64(k["top_speed"]).view(np.uint64) == np.float64(pl["top_speed"]).view(np.uint64)         # the same operations: the same bits
            sp = np.sqrt(kin["velocities"][c, :, 0] ** 2 + kin["velocities"][c, :, 1] ** 2)
            dist, steps = _kin_distance(sp, f, case["fps"], case["fps"])
            assert dist == k["distance"]
            bound = steps * 2.0 ** -21 + 1e-9 * k["distance"]
            print("id", k["id"], "steps", steps, "kinematics", k["distance"], "physical", pl["distance"], "difference", abs(pl["distance"] - k["distance"]), "bound", bound)
            assert abs(pl["distance"] - k["distance"]) <= bound
            moved += k["distance"] > 0
        assert moved > 0
    finally:
        t.close()
    # the same on a long constructed table: 2049 rows, three persons
    c, exp = PC.BY_NAME["walk_2049_rows_3_persons"], PC.reference("walk_2049_rows_3_persons")
    speed, _, _, totals, _, _ = lib.op_physical(c["velocities"], c["frames"], c["columns"], _params(c))
    for i, col in enumerate(exp["persons"]):
        v = c["velocities"][col]
        sp = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2)
        dist, steps = _kin_distance(sp, c["frames"].astype(np.int64), c["fps"], c["max_gap"])
        got = int(totals[i]["zone_dist_q"].sum()) / 2 ** 20
        bound = steps * 2.0 ** -21 + 1e-9 * dist
        print("column", col, "steps", steps, "numpy", dist, "physical", got, "difference", abs(got - dist), "bound", bound)
        assert steps > 1500 and abs(got - dist) <= bound
        assert np.float64(sp[np.isfinite(sp)].max()).view(np.uint64) == totals[i]["top_speed"].view(np.uint64)


def test_refusals(handle):
    L = handle.L
    c = PC.BY_NAME["run_across_rows_1023_1024"]
    vel, frames = np.ascontiguousarray(c["velocities"]), np.ascontiguousarray(c["frames"])
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    rows = len(frames)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    speed, accel, zone = np.full((3, rows), 7.0), np.full((3, rows), 7.0), np.full((3, rows), 77, np.uint8)
    tot = np.zeros(3, lib.LOAD_TOTALS_DTYPE)
    tot["col"] = -7
    ev = np.zeros(16, lib.LOAD_EFFORT_DTYPE)
    ev["col"] = -7
    npers, nev = C.c_int(-9), C.c_int(-9)
    P = lib.load_params
    good = P(10)

    def op(params=good, vel_p=vp(vel), frames_p=vp(frames), cols_p=vp(cols), np_p=C.byref(npers), ne_p=C.byref(nev), tot_p=vp(tot), tcap=3, ev_p=vp(ev), ecap=16, nrows=rows):
        rc = L.eagle_op_physical(0, vel_p, frames_p, cols_p, nrows, len(cols), None if params is None else C.byref(params), vp(speed), vp(accel), vp(zone), tot_p, tcap, np_p,
                                 ev_p, ecap, ne_p)
        assert (speed == 7.0).all() and (accel == 7.0).all() and (zone == 77).all() and (tot["col"] == -7).all() and (ev["col"] == -7).all()      # nothing launched, nothing written
        return rc, L.eagle_last_error(None).decode()

    unknown, negative = cols.copy(), cols.copy()
    unknown[5]["kind"] = 9
    negative[0]["kind"] = -1
    same, back = frames.copy(), frames.copy()
    same[3] = same[2]
    back[4] = back[3] - 1
    nan, inf = float("nan"), float("inf")
    bad = [(dict(params=None), "NULL"), (dict(params=P(0)), "positive"), (dict(params=P(-5)), "positive"), (dict(params=P(10, max_gap=0)), "positive"),
           (dict(params=P(10, max_gap=-1)), "positive"), (dict(params=P(10, min_frames=(0, 1))), "positive"), (dict(params=P(10, min_frames=(1, -2))), "positive"),
           (dict(params=P(10, zone_edges=(2.0, 4.0, 4.0, 7.0))), "ascending"), (dict(params=P(10, zone_edges=(4.0, 2.0, 5.5, 7.0))), "ascending"),
           (dict(params=P(10, zone_edges=(0.0, 4.0, 5.5, 7.0))), "ascending"), (dict(params=P(10, zone_edges=(-1.0, 4.0, 5.5, 7.0))), "ascending"),
           (dict(params=P(10, zone_edges=(2.0, nan, 5.5, 7.0))), "ascending"), (dict(params=P(10, zone_edges=(2.0, 4.0, 5.5, inf))), "ascending"),
           (dict(params=P(10, effort_speed=(0.0, 7.0))), "effort_speed"), (dict(params=P(10, effort_speed=(5.5, -7.0))), "effort_speed"),
           (dict(params=P(10, effort_speed=(nan, 7.0))), "effort_speed"), (dict(params=P(10, effort_speed=(5.5, inf))), "effort_speed"),
           (dict(params=P(10, accel=0.0)), "accel"), (dict(params=P(10, accel=-2.0)), "accel"), (dict(params=P(10, accel=nan)), "accel"), (dict(params=P(10, accel=inf)), "accel"),
           (dict(vel_p=None), "bad argument"), (dict(frames_p=None), "bad argument"), (dict(cols_p=None), "bad argument"), (dict(np_p=None), "bad argument"),
           (dict(ne_p=None), "bad argument"), (dict(tot_p=None), "bad argument"), (dict(ev_p=None), "bad argument"), (dict(tcap=-1), "bad argument"),
           (dict(ecap=-1), "bad argument"), (dict(nrows=-1), "bad argument"), (dict(cols_p=vp(unknown)), "unknown kind"), (dict(cols_p=vp(negative)), "unknown kind"),
           (dict(frames_p=vp(same)), "ascend"), (dict(frames_p=vp(back)), "ascend")]
    for kw, word in bad:
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and word in msg, (kw, msg)
    assert npers.value == -9 and nev.value == -9
    assert op(nrows=0)[0] == 0 and npers.value == 0 and nev.value == 0                   # rows == 0: success, nothing written
    assert op(tot_p=None, tcap=0, ev_p=None, ecap=0, nrows=0)[0] == 0

    # the handle entry
    case = post_cases.BY_NAME["goalkeeper_fold"]
    t = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, case["team_mapping"])
    other = lib.Handle(batch=1, frame_h=140, frame_w=204)
    try:
        good = P(25)
        assert L.eagle_post_physical(handle._h, t._t, C.byref(good)) == lib.E_INVALID and b"no velocities" in L.eagle_last_error(handle._h)
        handle.velocities(t, 25)
        for p, word in ((None, b"NULL"), (P(0), b"positive"), (P(25, max_gap=0), b"positive"), (P(25, min_frames=(0, 3)), b"positive"),
                        (P(25, zone_edges=(2.0, 2.0, 5.5, 7.0)), b"ascending"), (P(25, zone_edges=(2.0, 4.0, 5.5, nan)), b"ascending"), (P(25, effort_speed=(0.0, 7.0)), b"effort_speed"),
                        (P(25, accel=nan), b"accel"), (P(25, accel=0.0), b"accel")):
            assert L.eagle_post_physical(handle._h, t._t, None if p is None else C.byref(p)) == lib.E_INVALID and word in L.eagle_last_error(handle._h), word
        assert L.eagle_post_physical(handle._h, None, C.byref(good)) == lib.E_INVALID
        assert L.eagle_post_physical(None, t._t, C.byref(good)) == lib.E_INVALID
        assert L.eagle_post_physical(other._h, t._t, C.byref(good)) == lib.E_INVALID and b"another handle" in L.eagle_last_error(other._h)
        a, b = C.c_void_p(1), C.c_void_p(1)
        assert L.eagle_post_device_physical(t._t, C.byref(a), C.byref(b)) == 0 and not a.value and not b.value       # a refused call leaves no result
        n = C.c_int(0)
        assert L.eagle_post_physical_values(None, None, None, None) == lib.E_INVALID
        assert L.eagle_post_physical_totals(t._t, None, 1, C.byref(n)) == lib.E_INVALID and L.eagle_post_physical_totals(t._t, None, 0, None) == lib.E_INVALID
        assert L.eagle_post_physical_efforts(t._t, None, -1, C.byref(n)) == lib.E_INVALID and L.eagle_post_physical_efforts(None, None, 0, C.byref(n)) == lib.E_INVALID
        assert handle.physical(t, good)[0].shape[1] == len(t.rows)                               # the handle still works
    finally:
        t.close()
        other.close()


def test_cli_physical(tmp_path):
    import json
    import os
    from eagle_amd import cli
    out = str(tmp_path / "out")
    assert cli.main(["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed", "--merge-ids", "--physical",
                     "--physical-edges", "0.5,1,2,4", "--physical-rows"]) == 0
    rows = json.load(open(os.path.join(out, "processed_data.json")))
    j = json.load(open(os.path.join(out, "physical.json")))
    assert set(j) == {"params", "players", "efforts", "speed", "accel", "zone"} and j["params"]["zone_edges"] == [0.5, 1.0, 2.0, 4.0] and j["params"]["fps"] == 5
    assert len(j["speed"]) == len(j["zone"]) == len(j["players"]) and all(len(r) == len(rows) for r in j["zone"])
    for pl in j["players"]:
        assert sum(pl["zone_distance_q"]) == pl["distance_q"] and pl["distance"] == pl["distance_q"] / 2 ** 20      # the zones add up to the total exactly
        assert sum(pl["zone_distance"]) == pl["distance"] and len(pl["zone_seconds"]) == 5              # multiples of 2^-20 m far below 2^53 of them: the float sum is exact
    assert not os.path.exists(os.path.join(out, "kinematics.json"))
