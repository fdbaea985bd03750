"""Stabilisation on the GPU (include/eagle.h, eagle_op_stabilise / eagle_post_stabilise / eagle_post_stabilise_values / eagle_post_original_values /
eagle_post_device_stabilise; csrc/stab.hip): every output bit equals the contract of tests/stab_ref.py — no tolerances, float arrays compared as bit
patterns, records as bytes — on the constructed tables of tests/stab_cases.py; the untouched columns keep their
bytes; NULL outputs; every refusal leaves poisoned outputs alone; two runs give the same bytes; through a handle on tables eagle_postprocess built: equal
to the operator entry and the contract, the original values, a twin table, eagle_post_smooth_tracks afterwards, the refused orders; the CLI's
stabilise.json and metadata.json on a small synthetic-weights clip."""
import ctypes as C

import numpy as np
import pytest

import post_cases
import smooth_ref as SR
import stab_cases as SC
import stab_ref as SB
import stitch_cases
from eagle_amd import lib, postprocess, weights

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in SC.CASES]
KEYS = ("values", "rows", "votes", "totals")
BITS = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _params(kw, **more):
    kw = {**kw, **more}
    return lib.stab_params(kw.pop("fps"), **kw)


def _equal(got, exp, what):
    assert got["values"].shape == exp["values"].shape and np.array_equal(BITS(got["values"]), BITS(exp["values"])), (what, np.argwhere(BITS(got["values"]) != BITS(exp["values"]))[:5])
    assert got["votes"].dtype == exp["votes"].dtype and np.array_equal(got["votes"], exp["votes"]), (what, np.argwhere(got["votes"] != exp["votes"])[:5])
    bad = [r for r in range(len(exp["rows"])) if got["rows"][r].tobytes() != exp["rows"][r].tobytes()]
    assert got["rows"].dtype == exp["rows"].dtype and not bad, (what, bad[:3], got["rows"][bad[:3]], exp["rows"][bad[:3]])
    assert got["totals"].tobytes() == exp["totals"].tobytes(), (what, got["totals"], exp["totals"])


@pytest.mark.parametrize("name", NAMES)
def test_op_stabilise_equals_contract(name):
    c, exp = SC.BY_NAME[name], SC.reference(name)
    got = lib.op_stabilise(c["values"], c["frames"], c["columns"], _params(c["params"]))
    _equal(got, exp, name)
    rest = [i for i, k in enumerate(exp["kinds"]) if k == 0]
    if rest:                                                          # video columns, boundaries: the input bytes
        assert got["values"][rest].tobytes() == c["values"][rest].tobytes()
    again = lib.op_stabilise(c["values"], c["frames"], c["columns"], _params(c["params"]))     # a second run gives the same bytes
    assert all(again[k].tobytes() == got[k].tobytes() for k in KEYS)


def _raw_call(L, c, p, outs, rows=None, values=True, frames=True, columns=True, frames_arr=None, cols_arr=None):
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    v, f = np.ascontiguousarray(c["values"]), np.ascontiguousarray(c["frames"] if frames_arr is None else frames_arr)
    cols = np.array([(k, i, vd, 0) for k, i, vd in c["columns"]], lib.POSTCOL_DTYPE) if cols_arr is None else cols_arr
    rc = L.eagle_op_stabilise(0, vp(v) if values else None, vp(f) if frames else None, vp(cols) if columns else None, len(f) if rows is None else rows, len(cols),
                              None if p is None else C.byref(p), *(vp(o) for o in outs))
    return rc, L.eagle_last_error(None).decode()


def _poisoned(c):
    cols, rows = c["values"].shape[:2]
    rec, tot = np.zeros(rows, lib.STAB_ROW_DTYPE), np.zeros(1, lib.STAB_TOTALS_DTYPE)
    rec["voters"], tot["rows"] = -7, -7
    return [np.full((cols, rows, 2), 7.0), rec, np.full((cols, rows, 2), -7, np.int32), tot]


def test_op_null_outputs():
    L = lib.load()
    name = "nan_inf_limit"
    c, exp = SC.BY_NAME[name], SC.reference(name)
    p = _params(c["params"])
    assert _raw_call(L, c, p, [None] * 4)[0] == 0                       # every output may be NULL
    for i, k in enumerate(KEYS):                                         # each alone
        outs = [None] * 4
        outs[i] = _poisoned(c)[i]
        assert _raw_call(L, c, p, outs)[0] == 0
        assert outs[i].tobytes() == exp[k].tobytes(), k


def test_op_refusals_leave_the_outputs_alone():
    L = lib.load()
    c = SC.BY_NAME["iterations_2"]
    P = lambda **kw: _params({**c["params"], **kw})
    outs = _poisoned(c)
    before = [o.copy() for o in outs]
    nan, inf = float("nan"), float("inf")
    unknown = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    unknown[2]["kind"] = 9
    same, back = c["frames"].copy(), c["frames"].copy()
    same[3] = same[2]
    back[4] = back[3] - 1
    bad = [(dict(p=None), "NULL"), (dict(p=P(fps=0)), "fps"), (dict(p=P(fps=-3)), "fps"), (dict(p=P(window=0)), "window"), (dict(p=P(window=65)), "window"),
           (dict(p=P(degree=0)), "degree"), (dict(p=P(degree=3)), "degree"), (dict(p=P(model=2)), "model"), (dict(p=P(model=-1)), "model"),
           (dict(p=P(min_voters=2)), "min_voters"), (dict(p=P(min_voters=65)), "min_voters"), (dict(p=P(iterations=0)), "iterations"), (dict(p=P(iterations=5)), "iterations"),
           (dict(p=P(trim_k=-1.0)), "trim_k"), (dict(p=P(trim_k=0.5)), "trim_k"), (dict(p=P(trim_k=nan)), "trim_k"),
           (dict(p=P(trim_k=inf)), "trim_k"), (dict(p=P(floor=-0.5)), "floor"), (dict(p=P(floor=nan)), "floor"), (dict(p=P(floor=inf)), "floor"),
           (dict(p=P(min_spread=0.0)), "min_spread"), (dict(p=P(min_spread=nan)), "min_spread"), (dict(p=P(min_spread=2000.0)), "min_spread"),
           (dict(p=P(max_gain=0.0)), "max_gain"), (dict(p=P(max_gain=1.5)), "max_gain"), (dict(p=P(max_gain=nan)), "max_gain"), (dict(p=P(jump=0.0)), "jump"),
           (dict(p=P(jump=inf)), "jump"), (dict(p=P(jump=nan)), "jump"),
           (dict(p=P(), values=False), "bad argument"), (dict(p=P(), frames=False), "bad argument"), (dict(p=P(), columns=False), "bad argument"),
           (dict(p=P(), rows=-1), "bad argument"), (dict(p=P(), cols_arr=unknown), "unknown kind"), (dict(p=P(), frames_arr=same), "ascend"), (dict(p=P(), frames_arr=back), "ascend")]
    for kw, word in bad:
        rc, msg = _raw_call(L, c, kw.pop("p"), outs, **kw)
        assert rc == lib.E_INVALID and word in msg, (kw, word, msg)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, before)), word                            # nothing launched, nothing written
    assert _raw_call(L, c, P(), outs)[0] == 0 and all(a.tobytes() != b.tobytes() for a, b in zip(outs, before))   # the same buffers are written by a good call


# ---- through a handle ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


SEVEN = (3, 5, 7, 9, 11, 13, 15)


def _table(handle, name, merge):
    if name == "seven_ids":                                           # post_cases' builder with enough persons for a row to have an estimate at the defaults
        case = post_cases._case(name, post_cases._base(30, ids=SEVEN), team_mapping={i: k & 1 for k, i in enumerate(SEVEN)})
    else:
        case = post_cases.BY_NAME[name] if name in post_cases.BY_NAME else stitch_cases.BY_NAME[name]
    return case, postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], case["team_mapping"] or None, merge_ids=merge)


HANDLE_CASES = [("goalkeeper_fold", False, dict(window=2, min_voters=3)), ("appear_vanish_return", False, dict(window=3, min_voters=3, degree=1, model=0, iterations=1)),
                ("ball_none", False, dict(window=1, min_voters=3)), ("seven_ids", False, dict(window=3)), ("seven_ids", False, dict(window=5, degree=1, iterations=3)), ("empty", False, dict()), ("hand_over", True, dict(window=4, min_voters=3, floor=0.0, trim_k=1.0, iterations=4))]


@pytest.mark.parametrize("name,merge,kw", HANDLE_CASES, ids=lambda v: str(v))
def test_handle_stabilise_equals_operator_entry_and_contract(handle, name, merge, kw):
    case, t = _table(handle, name, merge)
    try:
        cols = _columns(t)
        raw = t.values.copy()
        assert handle.stabilise_device(t) is None
        assert handle.L.eagle_post_stabilise_values(t._t, None, None, None) == lib.E_INVALID                           # no result yet
        assert handle.original_values(t).tobytes() == raw.tobytes()                                                 # without a call: the table's own
        p = lib.stab_params(case["fps"], **kw)
        got = handle.stabilise(t, p)
        got["values"] = t.values
        _equal(got, lib.op_stabilise(raw, t.rows, cols, p), (name, "op"))
        exp = SB.stabilise(raw, t.rows, cols, case["fps"], **kw)
        _equal(got, exp, (name, "contract"))
        assert name != "seven_ids" or (exp["totals"][0]["affine"] + exp["totals"][0]["translation"] > 20 and not np.array_equal(BITS(exp["values"]), BITS(raw)))
        assert handle.original_values(t).tobytes() == raw.tobytes()
        assert (handle.stabilise_device(t) is not None) == (raw.size > 0)
        assert handle.L.eagle_post_stabilise_values(t._t, None, None, None) == 0                                       # any pointer may be NULL
        # a second call is refused and leaves the table alone
        after = t.values.copy()
        assert handle.L.eagle_post_stabilise(handle._h, t._t, C.byref(p)) == lib.E_INVALID and b"second call" in handle.L.eagle_last_error(handle._h)
        t._values = None
        assert t.values.tobytes() == after.tobytes()
        # eagle_post_smooth_tracks accepts the stabilised table: it equals the smoothing contract on the stabilised values, which are its raw values
        sp = lib.smooth_params(case["fps"], window=2)
        sm = handle.smooth_tracks(t, sp)
        exp = SR.smooth(after, t.rows, cols, case["fps"], window=2)
        assert np.array_equal(BITS(t.values), BITS(exp["values"])) and np.array_equal(BITS(sm["velocities"]), BITS(exp["vel"])) and np.array_equal(sm["flags"], exp["flags"])
        assert handle.raw_values(t).tobytes() == after.tobytes() and handle.original_values(t).tobytes() == raw.tobytes()
    finally:
        t.close()


def test_handle_order_and_refusals(handle):
    L = handle.L
    good = lib.stab_params(25, window=2)
    other = lib.Handle(batch=1, frame_h=140, frame_w=204)
    tables = [_table(handle, "seven_ids", False)[1] for _ in range(4)]
    t, u, s, w = tables
    try:
        raw = t.values.copy()
        assert L.eagle_post_stabilise(handle._h, None, C.byref(good)) == lib.E_INVALID
        assert L.eagle_post_stabilise(None, t._t, C.byref(good)) == lib.E_INVALID
        assert L.eagle_post_stabilise(other._h, t._t, C.byref(good)) == lib.E_INVALID and b"another handle" in L.eagle_last_error(other._h)
        for p, word in ((None, b"NULL"), (lib.stab_params(0, window=2), b"fps"), (lib.stab_params(25, window=0), b"window"), (lib.stab_params(25, window=65), b"window"),
                        (lib.stab_params(25, degree=3), b"degree"), (lib.stab_params(25, model=3), b"model"), (lib.stab_params(25, min_voters=2), b"min_voters"),
                        (lib.stab_params(25, iterations=5), b"iterations"), (lib.stab_params(25, trim_k=-1.0), b"trim_k"), (lib.stab_params(25, floor=float("nan")), b"floor"),
                        (lib.stab_params(25, min_spread=0.0), b"min_spread"), (lib.stab_params(25, max_gain=2.0), b"max_gain"), (lib.stab_params(25, jump=0.0), b"jump")):
            assert L.eagle_post_stabilise(handle._h, t._t, None if p is None else C.byref(p)) == lib.E_INVALID and word in L.eagle_last_error(handle._h), word
        assert handle.stabilise_device(t) is None
        # after eagle_post_velocities: refused, the table's bytes stay
        handle.velocities(t, 25)
        assert L.eagle_post_stabilise(handle._h, t._t, C.byref(good)) == lib.E_INVALID and b"velocities" in L.eagle_last_error(handle._h)
        assert b"stabilising comes first" in L.eagle_last_error(handle._h)
        t._values = None
        assert t.values.tobytes() == raw.tobytes() and handle.stabilise_device(t) is None
        # after eagle_post_smooth_tracks: refused, the smoothed table's bytes stay
        handle.smooth_tracks(s, lib.smooth_params(25, window=2))
        smoothed = s.values.copy()
        assert L.eagle_post_stabilise(handle._h, s._t, C.byref(good)) == lib.E_INVALID and b"stabilising comes first" in L.eagle_last_error(handle._h)
        s._values = None
        assert s.values.tobytes() == smoothed.tobytes() and handle.stabilise_device(s) is None
        assert L.eagle_post_stabilise_values(None, None, None, None) == lib.E_INVALID
        assert L.eagle_post_original_values(t._t, None) == lib.E_INVALID and L.eagle_post_device_stabilise(t._t, None) == lib.E_INVALID
        # a twin table that is stabilised does not change this one; the columns that are not moved keep their bytes
        handle.stabilise(u, good)
        assert w.values.tobytes() == raw.tobytes() and handle.original_values(u).tobytes() == raw.tobytes() and handle.original_values(w).tobytes() == raw.tobytes()
        moved = [i for i, k in enumerate(_columns(u)) if not k[2] and k[0] in (SB.PLAYER, SB.GOALKEEPER, SB.BALL)]
        rest = [i for i in range(len(u.columns)) if i not in moved]
        assert u.values[rest].tobytes() == raw[rest].tobytes() and u.values[moved].tobytes() != raw[moved].tobytes()
    finally:
        for x in tables:
            x.close()
        other.close()


def test_cli_stabilise(tmp_path):
    import json
    import os
    from eagle_amd import cli
    base = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--processed", "--merge-ids"]
    plain, out = str(tmp_path / "plain"), str(tmp_path / "out")
    assert cli.main(base + ["--out", plain]) == 0
    assert cli.main(base + ["--out", out, "--stabilise", "--stabilise-window", "2", "--stabilise-degree", "1", "--stabilise-model", "translation", "--stabilise-min-voters", "3",
                            "--stabilise-iterations", "1", "--stabilise-trim", "2", "--stabilise-floor", "0.5", "--stabilise-rows"]) == 0
    load = lambda d, n: json.load(open(os.path.join(d, n)))
    assert not os.path.exists(os.path.join(plain, "stabilise.json")) and "stabilised" not in load(plain, "metadata.json")
    meta, j = load(out, "metadata.json"), load(out, "stabilise.json")
    assert meta["stabilised"] is True and set(j) == {"params", "totals", "jumps", "rows"}
    assert j["params"] == {"fps": 5, "window": 2, "degree": 1, "model": "translation", "min_voters": 3, "iterations": 1, "trim_k": 2.0, "floor": 0.5, "min_spread": 5.0,
                           "max_gain": 0.05, "jump": 1.0}
    rows, rows_plain = load(out, "processed_data.json"), load(plain, "processed_data.json")
    assert len(rows) == len(rows_plain) == len(j["rows"]) == j["totals"]["rows"] > 0
    assert j["totals"]["none"] + j["totals"]["translation"] + j["totals"]["affine"] == len(rows) and j["totals"]["affine"] == 0
    assert j["totals"]["rms_after"] <= j["totals"]["rms_before"] and [e["row"] for e in j["jumps"]] == [i for i, e in enumerate(j["rows"]) if "jump" in e["flags"]]
    pos = lambda rr: {(i, e["ID"]): e["Coordinates"] for i, r in enumerate(rr) for e in r["Coordinates"]}
    a, b = pos(rows), pos(rows_plain)
    assert a.keys() == b.keys()                                                                            # the same cells
    moved_rows = {i for i, e in enumerate(j["rows"]) if e["model"] != "none"}
    assert all((a[k] != b[k]) <= (k[0] in moved_rows) for k in a)                                          # only rows with an estimate change
    assert [r["Coordinates_video"] for r in rows] == [r["Coordinates_video"] for r in rows_plain]         # the video columns and boundaries are untouched
    assert [r["Boundaries"] for r in rows] == [r["Boundaries"] for r in rows_plain]
