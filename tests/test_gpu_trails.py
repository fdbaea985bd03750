"""The minimap's trail, pass-arrow and owner layers and the two stills on the GPU (include/eagle.h, eagle_op_minimap_trails / eagle_op_trajectory_picture /
eagle_op_pass_picture / eagle_minimap_set_trails / eagle_trajectory_picture / eagle_pass_picture; csrc/minimap.hip, csrc/trails.hip): every output byte
equals the numpy contract of tests/trails_ref.py — no tolerances — for the constructed tables of tests/trails_cases.py; with no layer the new entry is
eagle_op_minimap; padded layouts; through a handle on a table eagle_postprocess and eagle_post_possession built, merge_ids on and off, without side
effects; every refusal; the command line."""
import ctypes as C
import os

import numpy as np
import pytest

import annot_ref as A
import control_ref as CR
import minimap_cases as MC
import minimap_ref as R
import post_cases
import stitch_cases
import trails_cases as TC
import trails_ref as T
from eagle_amd import lib, postprocess, synth, weights

pytestmark = pytest.mark.gpu


def _params(c, layers=None):
    kw = c["kw"]
    return lib.minimap_params(c["S"], c["M"], kw.get("voronoi", 0), kw.get("footprint", 1), kw.get("player_radius", 0), kw.get("ball_radius", 0),
                              layers=c["layers"] if layers is None else layers)


def _trail(p):
    return lib.trail_params(p["window"], p["max_gap"], p["half_width"], p["pass_hold"], p["dim_floor"])


def _run(c, fmt="bgr", layout=None, out=None):
    return lib.op_minimap_trails(c["values"], c["frames"], c["columns"], c["mapping"], _params(c), _trail(c["p"]), c["sel"], c["owner"], c["events"], c["row0"], c["n"],
                                 fmt, layout, out)


@pytest.mark.parametrize("name", [c["name"] for c in TC.CASES])
def test_op_minimap_trails_equals_contract(name):
    got = _run(TC.BY_NAME[name])
    exp = TC.reference(name)
    assert got.shape == exp.shape and np.array_equal(got, exp)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
@pytest.mark.parametrize("name", TC.YUV_CASES)
def test_op_minimap_trails_yuv(name, fmt):
    fr = TC.reference(name)
    assert np.array_equal(_run(TC.BY_NAME[name], fmt).reshape(-1), A.annotate(fr, [[] for _ in fr], fmt))


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_padded_layout_leaves_uncovered_bytes(fmt):
    c = TC.BY_NAME[TC.PADDED_CASE]
    w, h = R.size(c["S"], c["M"])
    lay = {"y_pitch": 3 * w + 40, "frame_stride": (3 * w + 40) * (h + 3)} if fmt == "bgr" else {"y_pitch": w + 64, "c_offset": (w + 64) * (h + 16), "c_pitch": w + 64,
                                                                                              "frame_stride": (w + 64) * (2 * h + 40)}
    fr = TC.reference(c["name"])
    exp = A.annotate(fr, [[] for _ in fr], fmt, lay, 0xA5)
    got = _run(c, fmt, lay, np.full(exp.size, 0xA5, np.uint8))
    assert np.array_equal(got, exp)
    slack = exp.size - c["n"] * (h * w * 3 if fmt == "bgr" else h * w * 3 // 2)
    assert slack > 0 and (got == 0xA5).sum() >= slack


def test_layers_0_is_eagle_op_minimap():
    for name in ("sites22", "edges_voronoi", "footprints_a", "sites257"):
        c = MC.BY_NAME[name]
        kw = c["kw"]
        p = lib.minimap_params(c["S"], c["M"], kw.get("voronoi", 0), kw.get("footprint", 1), kw.get("player_radius", 0), kw.get("ball_radius", 0))
        frames = np.arange(c["values"].shape[1], dtype=np.int32)
        plain = lib.op_minimap(c["values"], c["columns"], c["mapping"], p, c["row0"], c["n"])
        assert np.array_equal(plain, MC.reference(name))
        assert np.array_equal(lib.op_minimap_trails(c["values"], frames, c["columns"], c["mapping"], p, None, row0=c["row0"], n=c["n"]), plain)
        assert np.array_equal(lib.op_minimap_trails(c["values"], None, c["columns"], c["mapping"], p, lib.trail_params(), row0=c["row0"], n=c["n"]), plain)


@pytest.mark.parametrize("name", [n for n, _ in TC.TRAJ])
def test_op_trajectory_picture_equals_contract(name):
    c = TC.trajectory_case(name)
    got = lib.op_trajectory_picture(c["values"], c["frames"], c["columns"], c["mapping"], c["sel"], c["row0"], c["n"], c["S"], c["M"], c["half_width"], c["max_gap"])
    assert np.array_equal(got, TC.trajectory_reference(name))


def test_op_pass_picture_equals_contract():
    c = TC.pass_case()
    got = lib.op_pass_picture(c["values"], c["columns"], c["mapping"], c["events"], c["event"], c["S"], c["M"], c["half_width"])
    assert np.array_equal(got, TC.pass_reference())


# ---- through a handle -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


# (case, merge_ids, whether the possession step must find events and owners on it: the pass and owner layers and eagle_pass_picture really run)
@pytest.mark.parametrize("name,merge,busy", [("goalkeeper_fold", False, True), ("appear_vanish_return", False, True), ("hand_over", True, False),
                                             ("hand_over", False, False)], ids=lambda v: str(v))
def test_handle_layers_and_stills_equal_contract_without_side_effects(handle, name, merge, busy):
    frames = synth.clip(0, 2)
    before = handle.process(frames).copy()
    case = post_cases.BY_NAME[name] if name in post_cases.BY_NAME else stitch_cases.BY_NAME[name]
    tm = case["team_mapping"] or None
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], tm, merge_ids=merge)
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        fr = np.asarray(t.rows, np.int32)
        _, owner, _, ev = handle.possession(t, lib.possession_params(case["fps"], 1024.0, 1, 1000))
        print(name, merge, "rows", rows, "events", len(ev), "owned rows", int((owner >= 0).sum()))
        if busy:
            assert len(ev) > 0 and (owner >= 0).any()
        sel = [c for c, (k, _, v) in enumerate(cols) if not v and k in (R.PLAYER, R.GOALKEEPER, R.BALL)]
        S, M = 2, 2
        p = T.trail_params(window=5, max_gap=case["fps"], half_width=2, pass_hold=3, dim_floor=64)
        plain_par = lib.minimap_params(S, M)
        plain = handle.minimap(t, plain_par)
        assert np.array_equal(plain, R.frames_bgr(values, cols, t.team_mapping, 0, rows, S, M))
        handle.minimap_set_trails(t, _trail(p), sel)
        par = lib.minimap_params(S, M, layers=7)
        ref = T.frames_bgr(values, fr, cols, t.team_mapping, 0, rows, S, M, layers=7, p=p, sel=sel, owner=owner, events=ev)
        assert not np.array_equal(ref, plain)
        assert np.array_equal(handle.minimap(t, par), ref)
        assert np.array_equal(handle.minimap(t, par, 3, 4, "i420").reshape(-1), A.annotate(ref[3:7], [[]] * 4, "i420"))      # a window, 4:2:0
        from eagle_amd import minimap as mm
        assert np.array_equal(mm.minimap(handle, t, S, M, trails=sel, passes=True, owner=True, trail_params=_trail(p), rows=(2, 3)), ref[2:5])
        half = rows // 2
        got = mm.trajectory_picture(handle, t, sel[:3], (1, half), S, M, 2, case["fps"])
        assert np.array_equal(got, T.trajectory_picture(values, fr, cols, t.team_mapping, sel[:3], 1, half, S, M, 2, case["fps"]))
        for k in range(len(ev)):
            assert np.array_equal(mm.pass_picture(handle, t, k, S, M, 2), T.pass_picture(values, fr, cols, t.team_mapping, ev, k, S, M, 2)), k
        # nothing moved: the table, the events, the owner, a later plain minimap
        assert np.array_equal(np.array(t.values), values, equal_nan=True) and handle.events(t).tobytes() == ev.tobytes()
        back = np.zeros(rows, np.int32)
        assert handle.L.eagle_post_possession_values(t._t, None, back.ctypes.data_as(C.c_void_p), None) == 0 and np.array_equal(back, owner)
        assert np.array_equal(handle.minimap(t, plain_par), plain)
        handle.minimap_set_trails(t, None)
        assert np.array_equal(handle.minimap(t, plain_par), plain)
    finally:
        t.close()
    after = handle.process(frames)
    assert all(np.array_equal(before[k], after[k]) for k in lib.RESULT_DTYPE.names)


def _control_ref(values, vel, fr, cols, tm, row0, n, S, M, Rc, **layers):
    """the contract's pictures with the control layer in Voronoi's slot: its colours from control_ref, composed by trails_ref"""
    out = []
    for r in range(row0, row0 + n):
        tint = CR.layer_colors(CR.grid(values, vel, cols, tm, r, Rc), Rc, S, M)
        out.append(T.draw_row(values, fr, cols, tm, r, S, M, tint=tint, **layers))
    return np.stack(out)


def test_handle_layers_together_with_control(handle):
    """the layers over the pitch-control tint, through a handle (the operator entry takes no velocities): one pass, a window in 4:2:0, and pictures large
    enough that the host entry's 32 MB staging takes them in two passes (10 and 1 of 1264 x 820), so the per-pass row offsets of the layers are used"""
    case = post_cases.BY_NAME["goalkeeper_fold"]
    tm = case["team_mapping"]
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], tm)
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        fr = np.asarray(t.rows, np.int32)
        vel = handle.velocities(t, case["fps"])
        _, owner, _, ev = handle.possession(t, lib.possession_params(case["fps"], 1024.0, 1, 1000))
        assert len(ev) > 0 and (owner >= 0).any()
        sel = [c for c, (k, _, v) in enumerate(cols) if not v and k in (R.PLAYER, R.GOALKEEPER, R.BALL)]
        p = T.trail_params(window=4, max_gap=case["fps"], half_width=1, pass_hold=2, dim_floor=32)
        layers = dict(layers=7, p=p, sel=sel, owner=owner, events=ev)
        handle.minimap_set_trails(t, _trail(p), sel)
        handle.minimap_set_control(t, lib.control_params(2))
        S, M = 2, 2
        par = lib.minimap_params(S, M, control=True, layers=7)
        ref = _control_ref(values, vel, fr, cols, tm, 0, rows, S, M, 2, **layers)
        assert not np.array_equal(ref, CR.frames_bgr(values, vel, cols, tm, 0, rows, S, M, 2))           # the layers show
        assert np.array_equal(handle.minimap(t, par), ref)
        assert np.array_equal(handle.minimap(t, par, 6, 3, "nv12").reshape(-1), A.annotate(ref[6:9], [[]] * 3, "nv12"))
        handle.minimap_set_control(t, lib.control_params(1))
        big = lib.minimap_params(12, 2, control=True, layers=7)
        wb, hb = lib.minimap_size(big)
        assert 10 * wb * hb * 3 <= 32 << 20 < 11 * wb * hb * 3
        assert np.array_equal(handle.minimap(t, big, 3, 11), _control_ref(values, vel, fr, cols, tm, 3, 11, 12, 2, 1, **layers))
        # without the layers the control picture is what it was
        assert np.array_equal(handle.minimap(t, lib.minimap_params(S, M, control=True)), CR.frames_bgr(values, vel, cols, tm, 0, rows, S, M, 1))
    finally:
        t.close()


def test_refusals(handle):
    c = TC.BY_NAME["pictures_3"]
    L = handle.L
    values = np.ascontiguousarray(c["values"])
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    frames, owner = np.arange(8, dtype=np.int32), np.full(8, -1, np.int32)
    ids, vals = np.array([1, 2], np.int32), np.array([0, 1], np.int32)
    ev = TC.events([(1, 2, 0, (10.0, 10.0), (20.0, 20.0), 0, 5)])
    w, h = R.size(2, 0)
    out = np.full(w * h * 3, 0x5A, np.uint8)
    vp = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    good = dict(window=2, max_gap=2, half_width=1, pass_hold=1, dim_floor=0)

    def op(layers=1, tp=good, sel=(0,), owner_a=owner, ev_a=ev, frames_a=frames, row0=0, n=1, control=False):
        par = lib.minimap_params(2, 0, control=control, layers=layers)
        trail = None if tp is None else lib.trail_params(**tp)
        s = np.array(sel, np.int32)
        rc = L.eagle_op_minimap_trails(0, vp(values), vp(frames_a), vp(cols), 8, len(cols), vp(ids), vp(vals), 2, C.byref(par), None if trail is None else C.byref(trail),
                                       vp(s) if len(s) else None, len(s), vp(owner_a), vp(ev_a), 0 if ev_a is None else len(ev_a), row0, n, 0, None, vp(out))
        msg = L.eagle_last_error(None).decode()
        assert (out == 0x5A).all() or rc == 0
        return rc, msg

    bad = [dict(tp=None), dict(layers=2, ev_a=None), dict(layers=4, owner_a=None), dict(sel=()), dict(tp=dict(good, window=0)), dict(tp=dict(good, half_width=0)),
           dict(tp=dict(good, half_width=9)), dict(tp=dict(good, dim_floor=-1)), dict(tp=dict(good, dim_floor=257)), dict(tp=dict(good, pass_hold=0)),
           dict(tp=dict(good, max_gap=0)), dict(sel=(6,)), dict(sel=(-1,)), dict(sel=(1,)), dict(sel=(0, 0)), dict(layers=8), dict(layers=9), dict(row0=8),
           dict(n=9), dict(frames_a=None), dict(control=True)]
    for kw in bad:
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and msg, kw
    bnd = np.array([(R.BOUNDARY, 0, 0, 0)], lib.POSTCOL_DTYPE)
    par, trail, s0 = lib.minimap_params(2, 0, layers=1), lib.trail_params(**good), np.zeros(1, np.int32)
    assert L.eagle_op_minimap_trails(0, vp(values), vp(frames), vp(bnd), 8, 1, None, None, 0, C.byref(par), C.byref(trail), vp(s0), 1, None, None, 0, 0, 1, 0, None,
                                     vp(out)) == lib.E_INVALID                                        # a boundary column
    assert L.eagle_op_minimap(0, vp(values), vp(cols), 8, len(cols), vp(ids), vp(vals), 2, C.byref(par), 0, 1, 0, None, vp(out)) == lib.E_INVALID      # layers without parameters
    assert op(n=0)[0] == 0 and (out == 0x5A).all()
    # the stills
    pic = np.full(w * h * 3, 0x5A, np.uint8)

    def traj(sel=(0,), row0=0, n=2, hw=1, gap=2, S=2):
        s = np.array(sel, np.int32)
        rc = L.eagle_op_trajectory_picture(0, vp(values), vp(frames), vp(cols), 8, len(cols), vp(ids), vp(vals), 2, vp(s), len(s), row0, n, S, 0, hw, gap, vp(pic))
        assert (pic == 0x5A).all() or rc == 0
        return rc

    for kw in (dict(sel=(1,)), dict(sel=(0, 0)), dict(sel=(7,)), dict(row0=7), dict(n=0), dict(row0=-1), dict(hw=0), dict(hw=9), dict(gap=0), dict(S=3)):
        assert traj(**kw) == lib.E_INVALID, kw

    def pas(event=0, hw=1, ev_a=ev):
        rc = L.eagle_op_pass_picture(0, vp(values), vp(cols), 8, len(cols), vp(ids), vp(vals), 2, vp(ev_a), 0 if ev_a is None else len(ev_a), event, 2, 0, hw, vp(pic))
        assert (pic == 0x5A).all() or rc == 0
        return rc

    for kw in (dict(event=1), dict(event=-1), dict(hw=0), dict(ev_a=None), dict(ev_a=TC.events([(1, 9, 0, (1.0, 1.0), (2.0, 2.0), 0, 1)]))):
        assert pas(**kw) == lib.E_INVALID, kw
    # the handle entries
    case = post_cases.BY_NAME["goalkeeper_fold"]
    t = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, case["team_mapping"])
    try:
        rows, ncols = len(t.rows), len(t.columns)
        big = np.full(w * h * 3, 0x5A, np.uint8)
        person = next(c for c, k in enumerate(t.columns) if not k["video"] and int(k["kind"]) == R.PLAYER)
        video = next(c for c, k in enumerate(t.columns) if k["video"])
        bound = next(c for c, k in enumerate(t.columns) if not k["video"] and int(k["kind"]) == R.BOUNDARY)

        def draw(layers):
            par = lib.minimap_params(2, 0, layers=layers)
            rc = L.eagle_minimap_frames(handle._h, t._t, 0, 1, C.byref(par), 0, None, vp(big))
            assert (big == 0x5A).all() or rc == 0
            return rc, L.eagle_last_error(handle._h).decode()

        assert draw(1)[0] == lib.E_INVALID and "eagle_minimap_set_trails" in draw(1)[1]               # a layer without its parameters
        trail = lib.trail_params(**good)
        one = np.array([person], np.int32)
        for sel_a in ([video], [bound], [ncols], [-1], [person, person]):
            s = np.array(sel_a, np.int32)
            assert L.eagle_minimap_set_trails(t._t, C.byref(trail), vp(s), len(s)) == lib.E_INVALID, sel_a
        for tp in (dict(good, window=0), dict(good, half_width=9), dict(good, dim_floor=300), dict(good, pass_hold=0), dict(good, max_gap=0)):
            assert L.eagle_minimap_set_trails(t._t, C.byref(lib.trail_params(**tp)), vp(one), 1) == lib.E_INVALID, tp
        assert draw(1)[0] == lib.E_INVALID                                                              # (a refused set_trails set nothing)
        assert L.eagle_minimap_set_trails(t._t, C.byref(trail), None, 0) == 0                           # passes and owner only
        assert draw(1)[0] == lib.E_INVALID                                                              # trails with an empty selection
        for layers in (2, 4, 6):
            rc, msg = draw(layers)
            assert rc == lib.E_INVALID and "possession" in msg                                          # no possession result yet
        assert draw(8)[0] == lib.E_INVALID
        assert L.eagle_pass_picture(handle._h, t._t, 0, 2, 0, 1, vp(big)) == lib.E_INVALID and (big == 0x5A).all()
        handle.possession(t, lib.possession_params(25))
        n_ev = len(handle.events(t))
        assert L.eagle_pass_picture(handle._h, t._t, n_ev, 2, 0, 1, vp(big)) == lib.E_INVALID and L.eagle_pass_picture(handle._h, t._t, -1, 2, 0, 1, vp(big)) == lib.E_INVALID
        for args in ((one, 1, rows, 1), (one, 1, 0, 0), (one, 1, -1, 1), (np.array([video], np.int32), 1, 0, 1)):
            assert L.eagle_trajectory_picture(handle._h, t._t, vp(args[0]), args[1], args[2], args[3], 2, 0, 1, 25, vp(big)) == lib.E_INVALID, args[1:]
        assert L.eagle_trajectory_picture(handle._h, t._t, vp(one), 1, 0, 1, 2, 0, 0, 25, vp(big)) == lib.E_INVALID
        assert (big == 0x5A).all()
        assert draw(6)[0] == 0                                                                          # the handle still works
    finally:
        t.close()


def test_cli_trails(tmp_path):
    from eagle_amd import cli
    out = str(tmp_path / "out")
    common = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed", "--minimap-scale", "2"]
    assert cli.main(common + ["--minimap", "--minimap-trails", "--minimap-passes", "--trajectory", "ball,1,2,3", "--pass-pictures"]) == 0
    import json
    rows = len(json.load(open(os.path.join(out, "processed_data.json"))))
    w, h = R.size(2, 4)
    blob = open(os.path.join(out, "minimap.y4m"), "rb").read()
    assert len(blob.split(b"\n", 1)[1]) == rows * (6 + w * h * 3 // 2)
    ppm = open(os.path.join(out, "trajectory.ppm"), "rb").read()
    assert ppm.startswith(b"P6\n%d %d\n255\n" % (w, h)) and len(ppm) == len(b"P6\n%d %d\n255\n" % (w, h)) + w * h * 3
    assert all(f.endswith(".ppm") for f in os.listdir(out) if f.startswith("pass_"))
