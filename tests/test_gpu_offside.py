"""The offside stage on the GPU (include/eagle.h, eagle_op_offside / eagle_post_offside; csrc/offside.hip): every field of every output equals the
contract of tests/offside_ref.py — tobytes(), no tolerance — for the constructed tables of tests/offside_cases.py; two runs give identical bytes; NULL
outputs in every combination and rows == 0; every refusal leaves poisoned outputs alone; through a handle on tables eagle_postprocess built from the
golden clips' records and from a constructed clip whose ball hops between team mates (the result is kept, a second call replaces it, a refused call
leaves it, a need beyond the table's memory budget is refused, the event records equal the contract computed from that table and its possession result);
Processor.offside; the command line's offside.json equals offside.py applied to the contract on the table the run built."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import offside_cases as OC
import offside_ref as OR
import possession_ref as PR
import post_cases
import stitch_cases
from eagle_amd import lib, offside, postprocess, weights

pytestmark = pytest.mark.gpu

vp = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def _equal(got, exp, what):
    for a, b, part in zip(got, exp, OC.PARTS):
        if a.dtype.names:
            for k in a.dtype.names:
                assert np.array_equal(a[k], b[k]), (what, part, k)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, part)


def _op(c):
    return lib.op_offside(c["values"], c["columns"], c["mapping"], lib.offside_params(**c["p"]), c["events"])


@pytest.mark.parametrize("name", [c["name"] for c in OC.CASES])
def test_op_offside_equals_contract(name):
    _equal(_op(OC.BY_NAME[name]), OC.reference(name), name)


def test_two_runs_give_identical_bytes():
    for name in ("members_130", "rows_300", "passes_at_tolerance_0.5"):
        _equal(_op(OC.BY_NAME[name]), _op(OC.BY_NAME[name]), "second run of " + name)


def _raw(c):
    values = np.ascontiguousarray(c["values"], np.float64)
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    pairs = list(c["mapping"].items() if isinstance(c["mapping"], dict) else c["mapping"])
    return values, cols, np.array([k for k, _ in pairs], np.int32), np.array([v for _, v in pairs], np.int32)


def _poisoned(rows, nm, ne):
    rec, mg, tot, clip, ev = (np.zeros((rows, 2), lib.OFFSIDE_ROW_DTYPE), np.full((nm, rows), 0x5A5A5A5A, np.int32), np.zeros(nm, lib.OFFSIDE_TOTALS_DTYPE),
                              np.zeros(1, lib.OFFSIDE_CLIP_DTYPE), np.zeros(ne, lib.OFFSIDE_EVENT_DTYPE))
    rec["n_att"] = 77; tot["rows"] = 66; clip["neg"] = 55; ev["n_off"] = 44
    return rec, mg, tot, clip, ev


UNTOUCHED = (lambda rec: (rec["n_att"] == 77).all() and not rec["status"].any() and not rec["line_qx"].any(), lambda mg: (mg == 0x5A5A5A5A).all(),
             lambda tot: (tot["rows"] == 66).all() and not tot["col"].any(), lambda clip: (clip["neg"] == 55).all() and not clip["pos"].any(),
             lambda ev: (ev["n_off"] == 44).all() and not ev["status"].any())


def _untouched(*out):
    return all(f(a) for f, a in zip(UNTOUCHED, out))


def test_null_outputs_in_every_combination_and_no_rows():
    L = lib.load()
    c = OC.BY_NAME["passes_at_tolerance_0.5"]
    values, cols, ids, vals = _raw(c)
    rows, exp = values.shape[1], OC.reference(c["name"])
    p = lib.offside_params(**c["p"])
    ev = np.ascontiguousarray(c["events"], lib.EVENT_DTYPE)
    head = (0, vp(values), None, vp(cols), rows, len(cols), vp(ids), vp(vals), len(ids), C.byref(p), vp(ev), len(ev))
    for want in itertools.product((False, True), repeat=5):
        out = _poisoned(rows, len(exp[2]), len(ev))
        assert L.eagle_op_offside(*head, *[vp(a) if w else None for a, w in zip(out, want)]) == 0, want
        for a, b, w, alone in zip(out, exp, want, UNTOUCHED):
            assert a.tobytes() == b.tobytes() if w else alone(a), want
    out = _poisoned(rows, len(exp[2]), len(ev))
    assert L.eagle_op_offside(0, vp(values), None, vp(cols), 0, len(cols), vp(ids), vp(vals), len(ids), C.byref(p), vp(ev), len(ev), *map(vp, out)) == 0      # rows == 0
    assert _untouched(*out)
    out = _poisoned(rows, len(exp[2]), len(ev))
    assert L.eagle_op_offside(*head[:10], None, 0, *map(vp, out)) == 0 and UNTOUCHED[4](out[4]) and out[0].tobytes() == exp[0].tobytes()                      # no events
    frames = np.arange(rows, dtype=np.int32)
    assert L.eagle_op_offside(0, vp(values), vp(frames), *head[3:], *map(vp, out)) == 0 and out[4].tobytes() == exp[4].tobytes()                               # frames are carried, not read
    rec, mg, tot, clip, e = lib.op_offside(values[:, :0], c["columns"], c["mapping"], p)
    assert rec.shape == (0, 2) and mg.shape == (6, 0) and tot.shape == (6,) and e.shape == (0,)


def test_refusals_leave_the_outputs_alone():
    L = lib.load()
    c = OC.BY_NAME["passes_at_tolerance_0.5"]
    values, cols, ids, vals = _raw(c)
    rows = values.shape[1]
    events = np.ascontiguousarray(c["events"], lib.EVENT_DTYPE)
    out = _poisoned(rows, 6, len(events))

    def op(p=lib.offside_params(), values_a=values, cols_a=cols, ids_a=ids, ncols=None, par=True, ev=events, nev=None):
        rc = L.eagle_op_offside(0, vp(values_a), None, vp(cols_a), rows, len(cols) if ncols is None else ncols, vp(ids_a), vp(vals), len(ids), C.byref(p) if par else None,
                                vp(ev), len(events) if nev is None else nev, *map(vp, out))
        return rc, L.eagle_last_error(None).decode()

    unknown = cols.copy(); unknown[2]["kind"] = 9
    two_balls = cols.copy(); two_balls[6]["kind"] = lib.POST_BALL
    reserved = lib.offside_params(); reserved.reserved[3] = 1
    bad_events = []
    for field, v in (("release_row", -1), ("release_row", rows), ("receive_row", rows), ("receive_row", -5), ("to_col", len(cols)), ("to_col", -1)):
        e = events.copy()
        e[1][field] = v
        bad_events.append(dict(ev=e))
    for kw in [dict(par=False), dict(ids_a=None), dict(values_a=None), dict(cols_a=None), dict(cols_a=unknown), dict(cols_a=two_balls), dict(p=reserved),
               dict(p=lib.offside_params(3)), dict(p=lib.offside_params(-1)), dict(p=lib.offside_params(0, 1, -0.5)), dict(p=lib.offside_params(0, 1, float("nan"))),
               dict(p=lib.offside_params(0, 1, float("inf"))), dict(p=lib.offside_params(0, 1, 1024.5)), dict(ncols=-1), dict(nev=-1), dict(ev=None)] + bad_events:
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and msg and _untouched(*out), kw
    # 4095 players, a goalkeeper and another are 4097 listed columns; without the last 4096 pass
    bc = np.array([(lib.POST_PLAYER, 1 + i, 0, 0) for i in range(4095)] + [(lib.POST_GOALKEEPER, 5000, 0, 0), (lib.POST_GOALKEEPER, 5001, 0, 0)], lib.POSTCOL_DTYPE)
    bi, bv, bvals = np.arange(1, 4096, dtype=np.int32), (np.arange(4095) % 2).astype(np.int32), np.zeros((4097, 1, 2))
    bvals[:, 0, 0] = 40.0 + np.arange(4097) % 50
    big = _poisoned(1, 4095, 0)
    p = lib.offside_params(lib.OFFSIDE_DIR_RIGHT)
    assert L.eagle_op_offside(0, vp(bvals), None, vp(bc), 1, 4097, vp(bi), vp(bv), 4095, C.byref(p), None, 0, *map(vp, big)) == lib.E_INVALID and _untouched(*big)
    assert L.eagle_op_offside(0, vp(bvals), None, vp(bc), 1, 4096, vp(bi), vp(bv), 4095, C.byref(p), None, 0, *map(vp, big)) == 0
    exp = OR.offside(bvals[:4096], [(int(k["kind"]), int(k["id"]), 0) for k in bc[:4096]], dict(zip(bi.tolist(), bv.tolist())), OR.offside_params(OR.DIR_RIGHT))
    _equal(big, exp, "4096 listed columns")
    assert big[0][0, 0]["n_def"] == 2048 and big[0][0, 1]["n_att"] == 2047
    ok = dict(c["p"])
    assert op(p=lib.offside_params(**ok))[0] == 0
    _equal(out, OC.reference(c["name"]), "after the refusals")


# ---- through a handle -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


def _hop_records(n, players=8, keepers=2, seed=5):
    """n records of `players` players and `keepers` goalkeepers on a slow random walk, team 0 (even detections) on the left; the ball sits on a player for
    three frames and hops to another (ids are detection index + 1)"""
    r = np.random.default_rng(seed)
    k = players + keepers + 1
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = k, 1, 1
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    x0 = np.array([r.uniform(10, 70) if j % 2 == 0 else r.uniform(35, 95) for j in range(players)] + [3.0, 102.0][:keepers] + [0.0])
    pos = np.stack([x0, r.uniform(5, 63, k)], 1)[None] + np.cumsum(r.normal(0, 0.7, (n, k, 2)), 0)
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


HOP_MAPPING = {i + 1: i % 2 for i in range(8)}


def _contract(t, p, events=None):
    return OR.offside(np.array(t.values), _columns(t), t.team_mapping, p, events, bool(t.flags & lib.POST_NO_BALL))


HANDLE_CASES = [("goalkeeper_fold", False), ("appear_vanish_return", False), ("rare_id_dropped", False), ("smooth_odd_rows", False), ("ball_none", False), ("empty", False),
                ("teams_head_inherits", True), ("hand_over", True)]


@pytest.mark.parametrize("name,merge", HANDLE_CASES, ids=lambda v: str(v))
def test_handle_offside_on_golden_clips_equals_contract(handle, name, merge):
    case = post_cases.BY_NAME[name] if name in post_cases.BY_NAME else stitch_cases.BY_NAME[name]
    recs = post_cases.records_of(case)
    tm = case["team_mapping"] or {i: i % 2 for i in range(64)}                                          # (a clip without a mapping gets one: the stage needs it)
    t = postprocess.process_data(handle, recs, case["fps"], case["frame_w"], tm, merge_ids=merge)
    try:
        rows = len(t.rows)
        assert (rows == 0) == (name == "empty") and (name != "ball_none" or t.flags & lib.POST_NO_BALL)
        assert handle.offside_device(t) == (None,) * 5 + (0, 0) and len(handle.offside_events(t)) == 0
        assert handle.L.eagle_post_offside_values(t._t, None, None, None, None) == lib.E_INVALID              # no result yet
        for direction, assume, tol in ((OR.DIR_AUTO, 1, 0.5), (OR.DIR_RIGHT, 0, 0.0), (OR.DIR_LEFT, 1, 2.0)):
            p = OR.offside_params(direction, assume, tol)
            got = handle.offside(t, lib.offside_params(**p))
            if rows:
                _equal(got, _contract(t, p)[:4], (name, direction))
            assert len(handle.offside_events(t)) == 0                                                         # no possession result: no events
        cand, owner, dist, ev = handle.possession(t, lib.possession_params(case["fps"], 1024.0, 1, 1000))
        p = OR.offside_params(OR.DIR_RIGHT, 1, 0.5)
        got = handle.offside(t, lib.offside_params(**p)) + (handle.offside_events(t),)
        exp = _contract(t, p, ev)
        print(name, "rows", rows, "members", len(got[2]), "events", len(ev), "event statuses", got[4]["status"].tolist(), "row statuses", np.unique(got[0]["status"]).tolist())
        if rows:
            _equal(got, exp, (name, "with events"))
        assert len(got[4]) == len(ev) and handle.offside_device(t)[5:] == (len(got[2]), len(ev) if rows else 0)
        assert handle.L.eagle_post_offside_values(t._t, None, None, None, None) == 0                          # any pointer may be NULL
    finally:
        t.close()


def test_handle_keeps_replaces_and_leaves_the_result(handle):
    t = handle.postprocess(_hop_records(40), 25, 1280, HOP_MAPPING)
    bare = handle.postprocess(_hop_records(9), 25, 1280, None)
    try:
        rows = len(t.rows)
        cand, owner, dist, ev = handle.possession(t, lib.possession_params(25, 1024.0, 1, 1000))
        p1 = OR.offside_params(OR.DIR_AUTO, 1, 0.5)
        got = handle.offside(t, lib.offside_params(**p1)) + (handle.offside_events(t),)
        exp = _contract(t, p1, ev)
        n_pass = int((ev["kind"] == lib.EVENT_PASS).sum())
        print("rows", rows, "events", len(ev), "passes", n_pass, "statuses", got[4]["status"].tolist(), "verdicts", got[4]["verdict"].tolist(), "clip", got[3][0])
        assert rows >= 30 and n_pass >= 2 and (exp[4]["status"] == OR.EV_OK).sum() >= 2 and exp[3][0]["direction"] == OR.DIR_RIGHT and len(exp[2]) == 8
        _equal(got, exp, "handle")
        _equal(got, lib.op_offside(np.array(t.values), _columns(t), t.team_mapping, lib.offside_params(**p1), ev), "handle against the operator entry")
        dev = handle.offside_device(t)
        assert all(dev[:5]) and dev[5:] == (8, len(ev))
        one = np.zeros(1, lib.OFFSIDE_EVENT_DTYPE)
        n = C.c_int(-1)
        assert handle.L.eagle_post_offside_events(t._t, vp(one), 1, C.byref(n)) == 0 and n.value == len(ev) and one.tobytes() == exp[4][:1].tobytes()      # a small cap
        p2 = OR.offside_params(OR.DIR_LEFT, 0, 0.0)
        second = handle.offside(t, lib.offside_params(**p2)) + (handle.offside_events(t),)                     # the other way round: another result
        _equal(second, _contract(t, p2, ev), "second call")
        assert second[0].tobytes() != got[0].tobytes()
        for bad, word in ((lib.offside_params(5), "direction"), (lib.offside_params(0, 1, -1.0), "tolerance"), (lib.offside_params(0, 1, float("nan")), "tolerance")):
            assert handle.L.eagle_post_offside(handle._h, t._t, C.byref(bad)) == lib.E_INVALID and word in handle.L.eagle_last_error(handle._h).decode()
        bad = lib.offside_params(); bad.reserved[0] = 7
        assert handle.L.eagle_post_offside(handle._h, t._t, C.byref(bad)) == lib.E_INVALID and "reserved" in handle.L.eagle_last_error(handle._h).decode()
        assert handle.L.eagle_post_offside(handle._h, t._t, None) == lib.E_INVALID
        kept = _poisoned(rows, 8, len(ev))
        assert handle.L.eagle_post_offside_values(t._t, *map(vp, kept[:4])) == 0                               # the refused calls left the good result in place
        kept[4][:] = handle.offside_events(t)
        _equal(kept, second, "kept")
        pr = lib.offside_params()
        assert handle.L.eagle_post_offside(handle._h, bare._t, C.byref(pr)) == lib.E_INVALID and "mapping" in handle.L.eagle_last_error(handle._h).decode()
        assert handle.offside_device(bare) == (None,) * 5 + (0, 0)
        assert handle.L.eagle_post_offside(handle._h, None, C.byref(pr)) == lib.E_INVALID and handle.L.eagle_post_offside(None, t._t, C.byref(pr)) == lib.E_INVALID
    finally:
        t.close(); bare.close()


def test_a_need_beyond_the_table_s_budget_is_refused(handle):
    """what the call allocates is held against the table's max_bytes, and it allocates every part of a result and of its lists from a 256-byte boundary: nine
    parts, 2304 bytes at least.  A clip of two frames of one player builds a table inside 1500 bytes ((raw + kept columns) x 2 rows x 16 bytes and the
    lists: at most 1080 with eight columns of each); its offside result does not fit them and is refused with the budget named, no result appears; under
    5000 bytes the same clip gets its result"""
    recs = _hop_records(2, players=1, keepers=0)
    recs["n_det"] = 1                                                                                         # (the player alone: no ball)
    for max_bytes, fits in ((1500, False), (5000, True)):
        t = handle.postprocess(recs, 25, 1280, {1: 0}, max_bytes=max_bytes)
        try:
            assert len(t.rows) == 2
            p = OR.offside_params(OR.DIR_RIGHT)
            pr = lib.offside_params(**p)
            rc = handle.L.eagle_post_offside(handle._h, t._t, C.byref(pr))
            if fits:
                assert rc == 0
                got = handle.offside(t, pr)
                _equal(got, _contract(t, p)[:4], "inside the budget")
                assert [list(r) for r in got[0]["status"]] == [[OR.TOO_FEW, OR.OK]] * 2 and list(got[0]["n_att"][:, 0]) == [1, 1]      # (nobody defends against group 0; the assumed keeper and its one player against group 1)
            else:
                assert rc == lib.E_INVALID and b"budget" in handle.L.eagle_last_error(handle._h)
                assert handle.offside_device(t) == (None,) * 5 + (0, 0) and handle.L.eagle_post_offside_values(t._t, None, None, None, None) == lib.E_INVALID
        finally:
            t.close()


def test_processor_offside_with_and_without_possession(handle):
    import types

    from eagle_amd.processor import Processor
    pr = Processor(types.SimpleNamespace(handle=handle))
    t = handle.postprocess(_hop_records(40), 25, 1280, HOP_MAPPING)
    try:
        p = OR.offside_params(OR.DIR_AUTO, 1, 1.0)
        rec, mg, tot, clip, _ = _contract(t, p)
        d = pr.offside(t, tolerance=1.0, per_row=True)
        assert d == offside.derive(rec, mg, tot, clip, t.columns, lib.offside_params(**p), t.rows, per_row=True) and "passes" not in d and len(d["ids"]) == 8
        cand, owner, dist, ev = handle.possession(t, lib.possession_params(25, 1024.0, 1, 1000))
        d = pr.offside(t, "right", 0.0, False)
        p = OR.offside_params(OR.DIR_RIGHT, 0, 0.0)
        rec, mg, tot, clip, oev = _contract(t, p, ev)
        assert d == offside.derive(rec, mg, tot, clip, t.columns, lib.offside_params(**p), t.rows, ev, oev) and len(d["passes"]) >= 2 and "per_row" not in d
    finally:
        t.close()


def test_cli_offside(tmp_path, monkeypatch):
    """the detections of the constructed clip whose ball hops stand in for the random networks' (the model's records and the team mapping are substituted,
    as in test_gpu_space); the table each run builds is taken where Processor.process_data hands it to the command line; everything behind it is the
    command line's own path.  offside.json must be the contract's result on that table put through offside.derive"""
    from eagle_amd import cli, records
    from eagle_amd.coordinate_model import CoordinateModel
    from eagle_amd.processor import Processor
    recs = _hop_records(30)

    def get_coordinates(self, frames, fps, **kw):
        coords = {i: records.to_reference_dict(r, i, fps) for i, r in enumerate(recs)}
        self._last = (coords, recs, np.ones(len(recs), bool))
        return coords

    monkeypatch.setattr(CoordinateModel, "get_coordinates", get_coordinates)
    monkeypatch.setattr(Processor, "get_team_mapping", lambda self, frames, coords, pixel_format="bgr": dict(HOP_MAPPING))
    seen = []
    build = Processor.process_data

    def spy(self, *a, **kw):
        t, tm = build(self, *a, **kw)
        seen.append({"values": np.array(t.values), "cols": _columns(t), "columns": t.columns.copy(), "frames": t.rows.copy(), "mapping": t.team_mapping,
                     "no_ball": bool(t.flags & lib.POST_NO_BALL)})
        return t, tm

    monkeypatch.setattr(Processor, "process_data", spy)
    out = str(tmp_path / "out")
    common = ["--frames", "30", "--fps", "25", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed"]
    assert cli.main(common + ["--offside", "--offside-direction", "right", "--offside-tolerance", "0.25", "--offside-no-assumed-keeper", "--offside-rows"]) == 0
    T = seen[-1]
    p = OR.offside_params(OR.DIR_RIGHT, 0, 0.25)
    rec, mg, tot, clip, _ = OR.offside(T["values"], T["cols"], T["mapping"], p, None, T["no_ball"])
    j = json.load(open(os.path.join(out, "offside.json")))
    print("rows", len(rec), "statuses", np.unique(rec["status"]).tolist(), "members", len(tot))
    assert len(rec) == len(T["frames"]) >= 20 and (rec["status"] == OR.OK).sum() >= 20 and len(tot) == 8
    assert j == offside.to_json(offside.derive(rec, mg, tot, clip, T["columns"], lib.offside_params(**p), T["frames"], per_row=True)) and "passes" not in j
    assert cli.main(common + ["--offside", "--possession"]) == 0
    T = seen[-1]
    p = OR.offside_params()
    poss = PR.possession(T["values"], T["frames"], T["cols"], T["mapping"], 25, no_ball=T["no_ball"])
    rec, mg, tot, clip, oev = OR.offside(T["values"], T["cols"], T["mapping"], p, poss["events"], T["no_ball"])
    j = json.load(open(os.path.join(out, "offside.json")))
    assert j == offside.to_json(offside.derive(rec, mg, tot, clip, T["columns"], lib.offside_params(**p), T["frames"], poss["events"], oev))
    assert "per_row" not in j and "passes" in j and j["clip"]["direction"] == "right"
