"""Ball flights on the GPU (include/eagle.h, eagle_op_ball_flights / eagle_post_ball_flights and its accessors; csrc/flights.hip): every output bit
equals the contract of tests/flights_ref.py — no tolerances, float arrays compared as bit patterns — on the constructed tables of tests/flights_cases.py,
in both layouts of the cost table; NULL outputs; every refusal leaves poisoned outputs alone; through a handle on tables eagle_postprocess built: equal to
the operator entry and the contract, the accessors before the call, a second call, the refused eagle_post_smooth_tracks / eagle_post_stabilise, a twin
table never asked; the CLI's ball_flights.json on a small synthetic-weights clip."""
import ctypes as C

import numpy as np
import pytest

import flights_cases as FC
import flights_ref as FR
import post_cases
import stitch_cases
from eagle_amd import lib, postprocess, weights

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in FC.CASES]
FLOATS = ("fitted", "velocity")
BITS = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _params(kw, **more):
    kw = dict(kw, **more)
    return lib.flight_params(kw.pop("fps"), kw.pop("max_gap"), **kw)


def _equal(got, exp, what):
    for k in FLOATS:
        assert got[k].shape == exp[k].shape and np.array_equal(BITS(got[k]), BITS(exp[k])), (what, k, np.argwhere(BITS(got[k]) != BITS(exp[k]))[:5])
    for k in ("seg", "flags"):
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:5])
    for k in ("flights", "kicks", "totals"):                         # records byte for byte: the floats as bit patterns, NaN included
        assert got[k].dtype == exp[k].dtype and got[k].tobytes() == exp[k].tobytes(), (what, k, got[k], exp[k])


@pytest.mark.parametrize("name", NAMES)
def test_op_flights_equal_contract(name):
    c, exp = FC.BY_NAME[name], FC.reference(name)
    for layout in (lib.FLIGHT_LAYOUT_DEFAULT, lib.FLIGHT_LAYOUT_END_MAJOR, lib.FLIGHT_LAYOUT_K_MAJOR):
        got = lib.op_ball_flights(c["values"], c["frames"], c["columns"], _params(c["params"], layout=layout), c["cuts"])
        _equal(got, exp, (name, layout))


def test_demo_clip_and_times():
    d = FC.demo(FC.DEMO_SEED)
    exp = FR.flights(d["values"], d["frames"], d["columns"], FR.params(d["fps"], 25))
    got = lib.op_ball_flights(d["values"], d["frames"], d["columns"], lib.flight_params(d["fps"], 25), times=True)
    _equal(got, exp, "demo")
    assert set(got["times"]) == set(lib.FLIGHT_TIMES) and all(v >= 0.0 for v in got["times"].values()) and got["times"]["total"] > 0.0


KEYS = ("seg", "flags", "fitted", "velocity", "flights", "kicks", "totals")


def _poisoned(c):
    rows = c["values"].shape[1]
    tot = np.zeros(1, lib.FLIGHT_TOTALS_DTYPE)
    tot["runs"] = -7
    fl, kk = np.zeros(max(rows, 1), lib.FLIGHT_DTYPE), np.zeros(max(rows, 1), lib.KICK_DTYPE)
    fl["row0"], kk["row"] = -7, -7
    return [np.full(rows, -7, np.int32), np.full(rows, 77, np.uint8), np.full((rows, 2), 7.0), np.full((rows, 2), 7.0), fl, kk, tot]


def _raw_call(L, c, p, outs, rows=None, values=True, frames=True, columns=True, frames_arr=None, cols_arr=None, cuts="case", n_cuts=None, counts=True, caps=None):
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    v, f = np.ascontiguousarray(c["values"]), np.ascontiguousarray(c["frames"] if frames_arr is None else frames_arr)
    cols = np.array([(k, i, vd, 0) for k, i, vd in c["columns"]], lib.POSTCOL_DTYPE) if cols_arr is None else cols_arr
    cuts = c["cuts"] if isinstance(cuts, str) else cuts
    cuts = None if cuts is None else np.ascontiguousarray(cuts, np.int32)
    nf, nk = C.c_int(-7), C.c_int(-7)
    seg, flags, fitted, velocity, fl, kk, tot = outs
    cf, ck = (0 if fl is None else len(fl), 0 if kk is None else len(kk)) if caps is None else caps
    rc = L.eagle_op_ball_flights(0, vp(v) if values else None, vp(f) if frames else None, vp(cols) if columns else None, len(f) if rows is None else rows, len(cols), vp(cuts),
                                 (0 if cuts is None else len(cuts)) if n_cuts is None else n_cuts, None if p is None else C.byref(p), vp(seg), vp(flags), vp(fitted), vp(velocity),
                                 vp(fl), cf, C.byref(nf) if counts else None, vp(kk), ck, C.byref(nk) if counts else None, vp(tot), None)
    return rc, L.eagle_last_error(None).decode(), nf.value, nk.value


def test_op_null_outputs():
    L = lib.load()
    name = "general"
    c, exp = FC.BY_NAME[name], FC.reference(name)
    p = _params(c["params"])
    assert _raw_call(L, c, p, [None] * 7, counts=False)[0] == 0       # every output may be NULL
    rc, _, nf, nk = _raw_call(L, c, p, [None] * 7)
    assert rc == 0 and nf == len(exp["flights"]) and nk == len(exp["kicks"])
    for i, k in enumerate(KEYS):                                      # each alone
        outs = [None] * 7
        outs[i] = _poisoned(c)[i]
        rc, _, nf, nk = _raw_call(L, c, p, outs)
        assert rc == 0, k
        got = outs[i][:nf] if k == "flights" else outs[i][:nk] if k == "kicks" else outs[i]
        if k in FLOATS:
            assert np.array_equal(BITS(got), BITS(exp[k])), k
        else:
            assert got.tobytes() == exp[k].tobytes(), k
    # a cap below the number found: the count is the number found, the rest of the buffer stays
    outs = [None] * 7
    outs[4] = _poisoned(c)[4]
    rc, _, nf, nk = _raw_call(L, c, p, outs, caps=(2, 0))
    assert rc == 0 and nf == len(exp["flights"]) > 2 and outs[4][:2].tobytes() == exp["flights"][:2].tobytes() and (outs[4]["row0"][2:] == -7).all()


def test_op_refusals_leave_the_outputs_alone():
    L = lib.load()
    c = FC.BY_NAME["general"]
    P = lambda **kw: _params(c["params"], **kw)
    outs = _poisoned(c)
    before = [o.copy() for o in outs]
    nan, inf = float("nan"), float("inf")
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    unknown, two_balls = cols.copy(), cols.copy()
    unknown[2]["kind"] = 9
    two_balls[2]["kind"] = FR.BALL
    same, back = c["frames"].copy(), c["frames"].copy()
    same[3] = same[2]
    back[4] = back[3] - 1
    reserved = P()
    reserved.reserved = 1
    bad = [(dict(p=None), "NULL"), (dict(p=P(fps=0.0)), "fps"), (dict(p=P(fps=-3.0)), "fps"), (dict(p=P(fps=nan)), "fps"), (dict(p=P(fps=inf)), "fps"),
           (dict(p=P(max_gap=0)), "max_gap"), (dict(p=P(max_gap=1025)), "max_gap"), (dict(p=P(max_rows=1)), "max_rows"), (dict(p=P(max_rows=129)), "max_rows"),
           (dict(p=P(noise=-0.1)), "noise"), (dict(p=P(noise=nan)), "noise"), (dict(p=P(noise=1025.0)), "noise"), (dict(p=P(penalty=-1.0)), "penalty"),
           (dict(p=P(penalty=inf)), "penalty"), (dict(p=P(noise=1.0, penalty=2.0 ** 20 + 1.0)), "2^40"), (dict(p=P(spike=-1.0)), "spike"), (dict(p=P(spike=nan)), "spike"),
           (dict(p=P(spike=1025.0)), "spike"), (dict(p=P(kick_dv=-1.0)), "kick_dv"), (dict(p=P(kick_dv=nan)), "kick_dv"), (dict(p=P(radius=0.0)), "radius"),
           (dict(p=P(radius=nan)), "radius"), (dict(p=P(radius=1025.0)), "radius"), (dict(p=P(still_speed=-1.0)), "still_speed"), (dict(p=P(shot_speed=inf)), "shot_speed"),
           (dict(p=P(shot_range=nan)), "shot_range"), (dict(p=P(shot_margin=-2.0)), "shot_margin"), (dict(p=P(layout=3)), "layout"), (dict(p=reserved), "reserved"),
           (dict(p=P(), values=False), "bad argument"), (dict(p=P(), frames=False), "bad argument"), (dict(p=P(), columns=False), "bad argument"),
           (dict(p=P(), rows=-1), "bad argument"), (dict(p=P(), caps=(-1, 0)), "bad argument"), (dict(p=P(), cols_arr=unknown), "unknown kind"),
           (dict(p=P(), cols_arr=two_balls), "both the ball"), (dict(p=P(), frames_arr=same), "ascend"), (dict(p=P(), frames_arr=back), "ascend"),
           (dict(p=P(), cuts=[9, 4]), "cut"), (dict(p=P(), cuts=[4, 4]), "cut"), (dict(p=P(), cuts=None, n_cuts=2), "cuts"), (dict(p=P(), n_cuts=-1), "cuts")]
    for kw, word in bad:
        rc, msg, nf, nk = _raw_call(L, c, kw.pop("p"), outs, **kw)
        assert rc == lib.E_INVALID and word in msg, (kw, word, msg)
        assert (nf, nk) == (-7, -7) and all(a.tobytes() == b.tobytes() for a, b in zip(outs, before)), word        # nothing launched, nothing written
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


def _table(handle, name, merge):
    case = post_cases.BY_NAME[name] if name in post_cases.BY_NAME else stitch_cases.BY_NAME[name]
    return case, postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], case["team_mapping"] or None, merge_ids=merge)


HANDLE_CASES = [("goalkeeper_fold", False, dict()), ("appear_vanish_return", False, dict(max_rows=3, penalty=1.0)), ("ball_none", False, dict()), ("empty", False, dict()),
                ("ball_candidates_tie", False, dict(noise=0.05, radius=30.0)), ("ball_two_sightings", False, dict(spike=0.1)), ("hand_over", True, dict(max_rows=2, kick_dv=0.5))]


@pytest.mark.parametrize("name,merge,kw", HANDLE_CASES, ids=lambda v: str(v))
def test_handle_flights_equal_operator_entry_and_contract(handle, name, merge, kw):
    case, t = _table(handle, name, merge)
    try:
        cols, rows = _columns(t), len(t.rows)
        raw = t.values.copy()
        L = handle.L
        n = C.c_int(-7)
        assert handle.ball_flights_device(t) == (None, None, None, None)                              # before the call: NULLs and EAGLE_E_INVALID
        assert L.eagle_post_ball_flight_values(t._t, None, None, None, None, None) == lib.E_INVALID
        assert L.eagle_post_ball_flight_records(t._t, None, 0, C.byref(n)) == lib.E_INVALID and L.eagle_post_ball_kicks(t._t, None, 0, C.byref(n)) == lib.E_INVALID and n.value == -7
        no_ball = bool(t.flags & lib.POST_NO_BALL)
        assert no_ball or name != "ball_none"                                                         # (tables without rows or sightings carry the flag too)
        cuts = [int(t.rows[len(t.rows) // 2])] if rows else None
        p = lib.flight_params(case["fps"], **kw)
        got = handle.ball_flights(t, p, cuts)
        exp = FR.flights(raw, t.rows, cols, FR.params(case["fps"], p.max_gap, **kw), cuts, no_ball=no_ball)
        _equal(got, exp, (name, "contract"))
        if not no_ball:
            _equal(got, lib.op_ball_flights(raw, t.rows, cols, p, cuts), (name, "op"))
        else:
            assert len(got["flights"]) == 0 and (got["seg"] == -1).all() and not got["flags"].any() and np.isnan(got["fitted"]).all() and np.isnan(got["velocity"]).all()
        dev = handle.ball_flights_device(t)
        assert all(dev) == (rows > 0) and len(set(dev)) == (4 if rows else 1)
        assert L.eagle_post_ball_flight_values(t._t, None, None, None, None, None) == 0                # any pointer may be NULL
        # a second call replaces the result
        p2 = lib.flight_params(case["fps"], max_rows=2, penalty=0.0, kick_dv=0.0)
        got2 = handle.ball_flights(t, p2)
        _equal(got2, FR.flights(raw, t.rows, cols, FR.params(case["fps"], p2.max_gap, max_rows=2, penalty=0.0, kick_dv=0.0), None, no_ball=no_ball), (name, "second call"))
        _equal(handle.ball_flight_values(t), got2, (name, "kept"))
        t._values = None
        assert t.values.tobytes() == raw.tobytes()                                                    # the table's positions are not touched
        # later stages that move the positions are refused and leave the table alone
        sp, st = lib.smooth_params(int(case["fps"]), window=2), lib.stab_params(int(case["fps"]), window=2)
        assert L.eagle_post_smooth_tracks(handle._h, t._t, C.byref(sp)) == lib.E_INVALID and b"flights" in L.eagle_last_error(handle._h)
        assert L.eagle_post_stabilise(handle._h, t._t, C.byref(st)) == lib.E_INVALID and b"flights" in L.eagle_last_error(handle._h)
        t._values = None
        assert t.values.tobytes() == raw.tobytes()
    finally:
        t.close()


def test_handle_refusals_and_a_twin_never_asked(handle):
    L = handle.L
    good = lib.flight_params(25)
    other = lib.Handle(batch=1, frame_h=140, frame_w=204)
    case, t = _table(handle, "goalkeeper_fold", False)
    case, u = _table(handle, "goalkeeper_fold", False)
    try:
        raw = t.values.copy()
        cuts = np.array([5, 3], np.int32)
        assert L.eagle_post_ball_flights(handle._h, None, C.byref(good), None, 0) == lib.E_INVALID
        assert L.eagle_post_ball_flights(None, t._t, C.byref(good), None, 0) == lib.E_INVALID
        assert L.eagle_post_ball_flights(other._h, t._t, C.byref(good), None, 0) == lib.E_INVALID and b"another handle" in L.eagle_last_error(other._h)
        assert L.eagle_post_ball_flights(handle._h, t._t, C.byref(good), cuts.ctypes.data_as(C.c_void_p), 2) == lib.E_INVALID and b"cut" in L.eagle_last_error(handle._h)
        assert L.eagle_post_ball_flights(handle._h, t._t, C.byref(good), None, 3) == lib.E_INVALID and b"cuts" in L.eagle_last_error(handle._h)
        for p, word in ((None, b"NULL"), (lib.flight_params(0.0), b"fps"), (lib.flight_params(25, max_gap=0), b"max_gap"), (lib.flight_params(25, max_rows=200), b"max_rows"),
                        (lib.flight_params(25, noise=float("nan")), b"noise"), (lib.flight_params(25, radius=0.0), b"radius"), (lib.flight_params(25, noise=4.0, penalty=1e6), b"2^40")):
            assert L.eagle_post_ball_flights(handle._h, t._t, None if p is None else C.byref(p), None, 0) == lib.E_INVALID and word in L.eagle_last_error(handle._h), word
        assert handle.ball_flights_device(t) == (None, None, None, None)                              # a refused call leaves no result
        assert L.eagle_post_ball_flight_values(None, None, None, None, None, None) == lib.E_INVALID and L.eagle_post_device_ball_flights(t._t, None, None, None, None) == lib.E_INVALID
        # a twin table that is asked does not change this one: its bytes, and every stage it could run before, stay
        handle.ball_flights(u, good)
        t._values = None
        assert t.values.tobytes() == raw.tobytes() and u.values.tobytes() == raw.tobytes() and handle.ball_flights_device(t) == (None, None, None, None)
        got = handle.smooth_tracks(t, lib.smooth_params(25, window=2))                                 # the twin never asked can still be smoothed
        assert got["flags"].any()
    finally:
        t.close()
        u.close()
        other.close()


def test_cli_ball_flights(tmp_path):
    import json
    import os
    from eagle_amd import cli
    base = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--processed", "--merge-ids", "--possession"]
    plain, out, bare = str(tmp_path / "plain"), str(tmp_path / "out"), str(tmp_path / "bare")
    assert cli.main(base + ["--out", plain]) == 0
    assert cli.main(base + ["--out", out, "--ball-flights", "--ball-flights-rows", "3", "--ball-flights-noise", "0.5", "--ball-flights-penalty", "4", "--ball-flights-spike", "2",
                            "--ball-flights-kick", "1.5", "--ball-flights-shot", "8", "--ball-flights-cells"]) == 0
    assert cli.main([a for a in base if a != "--possession"] + ["--out", bare, "--ball-flights"]) == 0
    load = lambda d, n: json.load(open(os.path.join(d, n)))
    assert not os.path.exists(os.path.join(plain, "ball_flights.json")) and "ball_flights" not in load(plain, "metadata.json")      # only with the flag
    for name in ("processed_data.json", "raw_data.json", "possession.json"):                                                       # everything else is what it was
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(plain, name), "rb").read(), name
    meta, j, b = load(out, "metadata.json"), load(out, "ball_flights.json"), load(bare, "ball_flights.json")
    assert meta["ball_flights"] is True and {k: v for k, v in meta.items() if k not in ("ball_flights", "seconds")} == {k: v for k, v in load(plain, "metadata.json").items() if k != "seconds"}
    assert set(j) == {"params", "cuts", "totals", "flights", "kicks", "shots", "passes", "cells"} and set(b) == {"params", "cuts", "totals", "flights", "kicks", "shots"}
    assert j["params"] == {"fps": 5.0, "max_gap": 5, "max_rows": 3, "noise": 0.5, "penalty": 4.0, "spike": 2.0, "kick_dv": 1.5, "radius": 2.0, "still_speed": 0.5, "shot_speed": 8.0,
                           "shot_range": 40.0, "shot_margin": 2.0}
    assert b["params"]["max_rows"] == 64 and b["params"]["noise"] == 0.25 and b["params"]["kick_dv"] == 3.0
    rows = load(out, "processed_data.json")
    assert set(j["cells"]) == {"frame", "flight", "flags", "fitted", "velocity"} and all(len(v) == len(rows) for v in j["cells"].values())
    t = j["totals"]
    assert t["flights"] == len(j["flights"]) == t["still"] + t["carried"] + t["free"] and t["kicks"] == len(j["kicks"]) and len(j["shots"]) == t["shots_near"] + t["shots_on_target"]
    assert len(j["passes"]) == len(load(out, "possession.json")["events"])
    for f in j["flights"]:
        assert set(f) == {"row0", "row1", "frame0", "frame1", "used", "spikes", "near", "kind", "capped", "continues", "x0", "y0", "x1", "y1", "vx", "vy", "speed", "rms", "shot",
                          "y_cross"} and f["kind"] in ("still", "carried", "free") and 1 <= f["row1"] - f["row0"] <= 3
    for k in j["kicks"]:
        assert set(k) == {"row", "frame", "flight_in", "flight_out", "id", "speed_in", "speed_out", "dv", "cos_turn"} and k["dv"] >= 1.5 and k["flight_out"] == k["flight_in"] + 1
    for e in j["passes"]:
        assert set(e) == {"event", "frame", "from_id", "to_id", "kick_row", "kick_frame", "kicker_id", "pass_speed", "kicker_is_from"}
    used = [c for c, fl in zip(j["cells"]["flight"], j["cells"]["flags"]) if fl & 1]
    assert all((c is None) == (v is None) for c, v in zip(j["cells"]["flight"], j["cells"]["fitted"])) and len(used) == sum(1 for fl in j["cells"]["flags"] if fl & 1)
