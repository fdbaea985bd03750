"""Track smoothing on the GPU (include/eagle.h, eagle_op_smooth_tracks / eagle_post_smooth_tracks / eagle_post_smooth_values / eagle_post_device_smooth /
eagle_post_raw_values; csrc/smooth.hip): every output bit equals the contract of tests/smooth_ref.py — no tolerances, float arrays compared as bit
patterns — on the constructed tables of tests/smooth_cases.py; the columns that are not smoothed keep their bytes and get eagle_op_velocities' result;
NULL outputs; every refusal leaves poisoned outputs alone; through a handle on tables eagle_postprocess built: equal to the operator entry fed the same
table, eagle_post_physical afterwards without eagle_post_velocities, the refused orders, the raw values, and a table never smoothed; the CLI's smooth.json and metadata.json on a small synthetic-weights clip."""
import ctypes as C

import numpy as np
import pytest

import physical_ref as PR
import post_cases
import smooth_cases as SC
import smooth_ref as SR
import stitch_cases
from eagle_amd import lib, postprocess, weights

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in SC.CASES]
FLOATS = ("values", "vel", "acc")
INTS = ("flags", "count", "residual_q", "suspect")
BITS = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _params(kw):
    kw = dict(kw)
    return lib.smooth_params(kw.pop("fps"), **kw)


def _equal(got, exp, what):
    for k in FLOATS:
        assert got[k].shape == exp[k].shape and np.array_equal(BITS(got[k]), BITS(exp[k])), (what, k, np.argwhere(BITS(got[k]) != BITS(exp[k]))[:5])
    for k in INTS:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:5])
    assert got["totals"].tobytes() == exp["totals"].tobytes(), (what, got["totals"], exp["totals"])


@pytest.mark.parametrize("name", NAMES)
def test_op_smooth_equals_contract(name):
    c, exp = SC.BY_NAME[name], SC.reference(name)
    p = _params(c["params"])
    got = lib.op_smooth_tracks(c["values"], c["frames"], c["columns"], p)
    _equal(got, exp, name)
    rest = [i for i, w in enumerate(exp["colw"]) if w == 0]
    if rest and len(c["frames"]):                                     # the columns that are not smoothed: the input bytes, eagle_op_velocities' velocities
        assert got["values"][rest].tobytes() == c["values"][rest].tobytes()
        vel = lib.op_velocities(c["values"], c["frames"], lib.kinematics_params(p.fps, p.max_gap, p.speed_cap))
        assert np.array_equal(BITS(got["vel"][rest]), BITS(vel[rest]))
        assert np.isnan(got["acc"][rest]).all() and not got["flags"][rest].any() and not got["totals"][rest]["present"].any()


def _raw_call(L, c, p, outs, rows=None, values=True, frames=True, columns=True, frames_arr=None, cols_arr=None):
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    v, f = np.ascontiguousarray(c["values"]), np.ascontiguousarray(c["frames"] if frames_arr is None else frames_arr)
    cols = np.array([(k, i, vd, 0) for k, i, vd in c["columns"]], lib.POSTCOL_DTYPE) if cols_arr is None else cols_arr
    rc = L.eagle_op_smooth_tracks(0, vp(v) if values else None, vp(f) if frames else None, vp(cols) if columns else None, len(f) if rows is None else rows, len(cols),
                                  None if p is None else C.byref(p), *(vp(o) for o in outs))
    return rc, L.eagle_last_error(None).decode()


def _poisoned(c):
    cols, rows = c["values"].shape[:2]
    tot = np.zeros(cols, lib.SMOOTH_TOTALS_DTYPE)
    tot["present"] = -7
    return [np.full((cols, rows, 2), 7.0), np.full((cols, rows, 2), 7.0), np.full((cols, rows, 2), 7.0), np.full((cols, rows), 77, np.uint8), np.full((cols, rows), 77, np.uint8),
            np.full((cols, rows), -7, np.int32), np.full(rows, 77, np.uint8), tot]


def test_op_null_outputs():
    L = lib.load()
    name = "suspect_rows"
    c, exp = SC.BY_NAME[name], SC.reference(name)
    p = _params(c["params"])
    assert _raw_call(L, c, p, [None] * 8)[0] == 0                       # every output may be NULL
    keys = ("values", "vel", "acc", "flags", "count", "residual_q", "suspect", "totals")
    for i, k in enumerate(keys):                                         # each alone
        outs = [None] * 8
        outs[i] = _poisoned(c)[i]
        assert _raw_call(L, c, p, outs)[0] == 0
        if k in FLOATS:
            assert np.array_equal(BITS(outs[i]), BITS(exp[k])), k
        else:
            assert outs[i].tobytes() == exp[k].tobytes(), k


def test_op_refusals_leave_the_outputs_alone():
    L = lib.load()
    c = SC.BY_NAME["ball_window_3"]
    P = lambda **kw: _params({**c["params"], **kw})
    outs = _poisoned(c)
    before = [o.copy() for o in outs]
    nan, inf = float("nan"), float("inf")
    unknown = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    unknown[2]["kind"] = 9
    same, back = c["frames"].copy(), c["frames"].copy()
    same[3] = same[2]
    back[4] = back[3] - 1
    bad = [(dict(p=None), "NULL"), (dict(p=P(fps=0)), "positive"), (dict(p=P(fps=-3)), "positive"), (dict(p=P(max_gap=0)), "positive"), (dict(p=P(speed_cap=0.0)), "positive"),
           (dict(p=P(speed_cap=nan)), "positive"), (dict(p=P(speed_cap=inf)), "positive"), (dict(p=P(window=0)), "window"), (dict(p=P(window=65)), "window"),
           (dict(p=P(window=-1)), "window"), (dict(p=P(degree=0)), "degree"), (dict(p=P(degree=3)), "degree"), (dict(p=P(ball_window=-1)), "ball_window"),
           (dict(p=P(ball_window=65)), "ball_window"), (dict(p=P(outlier_k=-1.0)), "outlier_k"), (dict(p=P(outlier_k=nan)), "outlier_k"), (dict(p=P(outlier_k=inf)), "outlier_k"),
           (dict(p=P(outlier_floor=-0.5)), "outlier_floor"), (dict(p=P(outlier_floor=nan)), "outlier_floor"), (dict(p=P(outlier_floor=inf)), "outlier_floor"),
           (dict(p=P(), values=False), "bad argument"), (dict(p=P(), frames=False), "bad argument"), (dict(p=P(), columns=False), "bad argument"),
           (dict(p=P(), rows=-1), "bad argument"), (dict(p=P(), cols_arr=unknown), "unknown kind"), (dict(p=P(), frames_arr=same), "ascend"), (dict(p=P(), frames_arr=back), "ascend")]
    for kw, word in bad:
        rc, msg = _raw_call(L, c, kw.pop("p"), outs, **kw)
        assert rc == lib.E_INVALID and word in msg, (kw, word, msg)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, before)), word                            # nothing launched, nothing written
    assert _raw_call(L, c, P(), outs)[0] == 0 and outs[0].tobytes() != before[0].tobytes()                  # the same buffers are written by a good call


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


HANDLE_CASES = [("goalkeeper_fold", False, dict(window=2)), ("appear_vanish_return", False, dict(window=3, ball_window=2, degree=1)), ("ball_none", False, dict(window=1)),
                ("empty", False, dict()), ("hand_over", True, dict(window=4, outlier_floor=0.0, outlier_k=1.0))]


@pytest.mark.parametrize("name,merge,kw", HANDLE_CASES, ids=lambda v: str(v))
def test_handle_smooth_equals_operator_entry_and_contract(handle, name, merge, kw):
    case, t = _table(handle, name, merge)
    try:
        cols, rows = _columns(t), len(t.rows)
        raw = t.values.copy()
        assert handle.smooth_device(t) == (None, None, None)
        assert handle.L.eagle_post_smooth_values(t._t, None, None, None, None, None, None) == lib.E_INVALID            # no result yet
        assert handle.raw_values(t).tobytes() == raw.tobytes()                                                      # without a call: the table's own
        p = lib.smooth_params(case["fps"], **kw)
        got = handle.smooth_tracks(t, p)
        got["values"], got["vel"] = t.values, got["velocities"]
        op = lib.op_smooth_tracks(raw, t.rows, cols, p)
        _equal(got, op, (name, "op"))
        exp = SR.smooth(raw, t.rows, cols, case["fps"], **kw)
        _equal(got, exp, (name, "contract"))
        assert handle.raw_values(t).tobytes() == raw.tobytes()
        d_acc, d_flags, d_suspect = handle.smooth_device(t)
        assert d_acc and d_flags and d_suspect and d_acc != t.device_values
        assert handle.L.eagle_post_smooth_values(t._t, None, None, None, None, None, None) == 0                        # any pointer may be NULL
        # the physical report runs on the fit's velocities without eagle_post_velocities
        lp = lib.load_params(case["fps"])
        speed, accel, zone, totals, ev = handle.physical(t, lp)
        ref = PR.physical(got["vel"], t.rows, cols, case["fps"], None, PR.ZONE_EDGES, PR.EFFORT_SPEED, 2.0, None)
        if rows and len(PR.layout(cols)):
            assert np.array_equal(BITS(speed), BITS(ref["speed"])) and np.array_equal(zone, ref["zone"]) and totals.tobytes() == ref["totals"].tobytes()
            assert ev.tobytes() == ref["efforts"].tobytes()
        # a second call is refused and leaves the table alone; a later eagle_post_velocities replaces the velocities, as it always did
        after = t.values.copy()
        assert handle.L.eagle_post_smooth_tracks(handle._h, t._t, C.byref(p)) == lib.E_INVALID and b"second call" in handle.L.eagle_last_error(handle._h)
        t._values = None
        assert t.values.tobytes() == after.tobytes()
        vel = handle.velocities(t, case["fps"])
        assert np.array_equal(BITS(vel), BITS(lib.op_velocities(after, t.rows, lib.kinematics_params(case["fps"])))) or rows == 0
    finally:
        t.close()


def test_handle_order_and_refusals(handle):
    L = handle.L
    good = lib.smooth_params(25, window=2)
    other = lib.Handle(batch=1, frame_h=140, frame_w=204)
    case, t = _table(handle, "goalkeeper_fold", False)
    case, u = _table(handle, "goalkeeper_fold", False)
    try:
        raw = t.values.copy()
        assert L.eagle_post_smooth_tracks(handle._h, None, C.byref(good)) == lib.E_INVALID
        assert L.eagle_post_smooth_tracks(None, t._t, C.byref(good)) == lib.E_INVALID
        assert L.eagle_post_smooth_tracks(other._h, t._t, C.byref(good)) == lib.E_INVALID and b"another handle" in L.eagle_last_error(other._h)
        for p, word in ((None, b"NULL"), (lib.smooth_params(0, window=2), b"positive"), (lib.smooth_params(25, window=0), b"window"), (lib.smooth_params(25, window=65), b"window"),
                        (lib.smooth_params(25, degree=3), b"degree"), (lib.smooth_params(25, outlier_k=-1.0), b"outlier_k"), (lib.smooth_params(25, outlier_floor=float("nan")), b"outlier_floor"),
                        (lib.smooth_params(25, ball_window=99), b"ball_window")):
            assert L.eagle_post_smooth_tracks(handle._h, t._t, None if p is None else C.byref(p)) == lib.E_INVALID and word in L.eagle_last_error(handle._h), word
        assert handle.smooth_device(t) == (None, None, None)
        # after eagle_post_velocities: refused, the table's bytes stay
        handle.velocities(t, 25)
        assert L.eagle_post_smooth_tracks(handle._h, t._t, C.byref(good)) == lib.E_INVALID and b"velocities" in L.eagle_last_error(handle._h)
        t._values = None
        assert t.values.tobytes() == raw.tobytes() and handle.smooth_device(t) == (None, None, None)
        assert L.eagle_post_smooth_values(None, None, None, None, None, None, None) == lib.E_INVALID
        assert L.eagle_post_raw_values(t._t, None) == lib.E_INVALID and L.eagle_post_device_smooth(t._t, None, None, None) == lib.E_INVALID
        # a table never smoothed is what it is today: a twin table that is smoothed does not change this one, and its own later stages see the new positions
        handle.smooth_tracks(u, good)
        assert t.values.tobytes() == raw.tobytes() and handle.raw_values(u).tobytes() == raw.tobytes()
        persons = [i for i, k in enumerate(_columns(u)) if not k[2] and k[0] in (SR.PLAYER, SR.GOALKEEPER)]
        rest = [i for i in range(len(u.columns)) if i not in persons]
        assert u.values[rest].tobytes() == raw[rest].tobytes() and u.values[persons].tobytes() != raw[persons].tobytes()
    finally:
        t.close()
        u.close()
        other.close()


def test_cli_smooth(tmp_path):
    import json
    import os
    from eagle_amd import cli
    base = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--processed", "--merge-ids", "--kinematics"]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    assert cli.main(base + ["--out", plain]) == 0
    assert cli.main(base + ["--out", out, "--smooth-tracks", "--smooth-window", "2", "--smooth-degree", "1", "--smooth-outlier", "3", "--smooth-floor", "0.5", "--smooth-rows",
                            "--physical"]) == 0
    load = lambda d, n: json.load(open(os.path.join(d, n)))
    assert not os.path.exists(os.path.join(plain, "smooth.json")) and "positions" not in load(plain, "metadata.json")
    meta, j = load(out, "metadata.json"), load(out, "smooth.json")
    assert meta["positions"] == "smoothed" and set(j) == {"params", "columns", "suspect"}
    assert j["params"] == {"fps": 5, "window": 2, "degree": 1, "outlier_k": 3.0, "outlier_floor": 0.5, "ball_window": 0, "max_gap": 5, "speed_cap": 12.0}
    rows, rows_plain = load(out, "processed_data.json"), load(plain, "processed_data.json")
    assert len(rows) == len(rows_plain) > 0 and len(j["columns"]) > 0
    pos = lambda rr: {(i, e["ID"]): e["Coordinates"] for i, r in enumerate(rr) for e in r["Coordinates"] if e["ID"] != "Ball"}
    a, b = pos(rows), pos(rows_plain)
    assert a.keys() == b.keys() and a != b                                                                 # the same cells, smoothed positions
    assert [r["Coordinates_video"] for r in rows] == [r["Coordinates_video"] for r in rows_plain]         # the video columns and the ball are untouched
    assert [r["Coordinates"][-1] for r in rows] == [r["Coordinates"][-1] for r in rows_plain] and [r["Boundaries"] for r in rows] == [r["Boundaries"] for r in rows_plain]
    kin = load(out, "kinematics.json")["players"]
    assert len(kin) == len(j["columns"]) == len(load(out, "physical.json")["players"])
    for k, c in zip(kin, j["columns"]):                                                                    # kinematics.json sums the fits' velocities
        cells = c["cells"]
        assert k["id"] == c["id"] and c["type"] in ("Player", "Goalkeeper") and c["window"] == 2 and len(cells["flags"]) == len(rows)
        sp = [np.sqrt(np.float64(v[0]) ** 2 + np.float64(v[1]) ** 2) for v in cells["velocity"] if v is not None]
        assert c["present"] == len(sp) and k["top_speed"] == (float(max(sp)) if sp else 0.0)
        assert c["max_residual"] >= c["rms_residual"] >= 0.0 and all((f & 12) <= 4 for f in cells["flags"] if f is not None)      # degree 1 at most
