"""Occupancy heat maps on the GPU (include/eagle.h, eagle_op_occupancy / eagle_op_occupancy_picture / eagle_post_occupancy / eagle_post_occupancy_values /
eagle_post_device_occupancy / eagle_occupancy_picture; csrc/occupancy.hip): every output bit equals the numpy contract of tests/occupancy_ref.py — no
tolerances — for the constructed tables of tests/occupancy_cases.py; the picture byte for byte; through a handle on tables eagle_postprocess built (host
and device entries, a second call replacing the first, merge_ids on and off, the minimap of the same table unchanged); every refusal; rows == 0 and
n_sel == 0; the CLI's files."""
import ctypes as C

import numpy as np
import pytest

import minimap_ref as MR
import occupancy_cases as OC
import occupancy_ref as OR
import post_cases
import stitch_cases
from eagle_amd import lib, postprocess, weights

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in OC.CASES]
vp = lambda a: a.ctypes.data_as(C.c_void_p)


def _params(c):
    return lib.occupancy_params(c["fps"], c["R"], c["sigma"], c["max_gap"])


def _check(got, exp, what):
    grids, by, counts, total, outside = got
    assert counts.dtype == np.int32 and np.array_equal(counts, exp["counts"]), (what, "counts", np.argwhere(counts != exp["counts"])[:5])
    assert total.dtype == np.int64 and np.array_equal(total, exp["total"]), (what, "total", total, exp["total"])
    assert np.array_equal(outside, exp["outside"]), (what, "outside", outside, exp["outside"])
    assert grids.dtype == np.float32 and np.array_equal(grids, exp["grids"]), (what, "grids", np.argwhere(grids != exp["grids"])[:5])
    assert by.dtype == np.uint8 and np.array_equal(by, exp["bytes"]), (what, "bytes", np.argwhere(by != exp["bytes"])[:5])


@pytest.mark.parametrize("name", NAMES)
def test_op_occupancy_equals_contract(name):
    c = OC.BY_NAME[name]
    _check(lib.op_occupancy(c["values"], c["frames"], c["columns"], _params(c), c["sel_off"], c["sel_cols"]), OC.reference(name), name)


@pytest.mark.parametrize("R", OR.RS)
def test_op_picture_equals_contract(R):
    by = OC.reference("corners_centre_R%d" % R)["bytes"][0]
    for S, M, colour in ((2, 0, (0, 0, 255)), (2, 8, (255, 0, 0)), (8, 0, (255, 255, 255)), (8, 8, (37, 201, 118))):
        got = lib.op_occupancy_picture(by, R, S, M, colour)
        assert np.array_equal(got, OR.picture(by, R, S, M, colour)), (R, S, M)
    ramp = (np.arange(68 * R * 105 * R) % 256).astype(np.uint8).reshape(68 * R, 105 * R)                # every byte value, every cell distinct from its neighbour
    assert np.array_equal(lib.op_occupancy_picture(ramp, R, 4, 2, (255, 128, 1)), OR.picture(ramp, R, 4, 2, (255, 128, 1)))


def test_op_rows_0_and_n_sel_0():
    cols = [(OC.P, 1, 0), (OC.BALL, 0, 0), (OC.BALL, 0, 1)]
    grids, by, counts, total, outside = lib.op_occupancy(np.zeros((3, 0, 2)), np.zeros(0, np.int32), cols, lib.occupancy_params(5, 2, 1.0), [0, 1, 2], [0, 1])
    assert grids.shape == (2, 136, 210) and not grids.any() and not by.any() and not counts.any() and not total.any() and not outside.any()
    c = OC.BY_NAME["frame_steps"]
    got = lib.op_occupancy(c["values"], c["frames"], c["columns"], _params(c), [0], [])                 # n_sel == 0: success, nothing to write
    assert all(a.shape[0] == 0 for a in got)
    got = lib.op_occupancy(np.zeros((0, 3, 2)), np.arange(3), [], lib.occupancy_params(5), [0, 0], [])  # rows without a column: an empty selection
    assert got[0].shape == (1, 68, 105) and not got[0].any() and got[3][0] == 0


def test_op_null_outputs():
    c = OC.BY_NAME["selections"]
    exp = OC.reference("selections")
    L = lib.load()
    values, frames = np.ascontiguousarray(c["values"]), np.ascontiguousarray(c["frames"])
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    off, sc = np.array(c["sel_off"], np.int32), np.array(c["sel_cols"], np.int32)
    total = np.zeros(6, np.int64)
    assert L.eagle_op_occupancy(0, vp(values), vp(frames), vp(cols), len(frames), len(cols), C.byref(_params(c)), vp(off), vp(sc), 6, None, None, vp(total), None, None) == 0
    assert np.array_equal(total, exp["total"])
    assert L.eagle_op_occupancy(0, vp(values), vp(frames), vp(cols), len(frames), len(cols), C.byref(_params(c)), vp(off), vp(sc), 6, None, None, None, None, None) == 0


# ---- through a handle ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


HANDLE_CASES = [("goalkeeper_fold", False), ("appear_vanish_return", False), ("ball_none", False), ("empty", False), ("teams_head_inherits", True),
                ("teams_head_inherits", False), ("hand_over", True)]


@pytest.mark.parametrize("name,merge", HANDLE_CASES, ids=lambda v: str(v))
def test_handle_occupancy_equals_contract(handle, name, merge):
    from eagle_amd import occupancy as oc
    case = post_cases.BY_NAME[name] if name in post_cases.BY_NAME else stitch_cases.BY_NAME[name]
    tm = case["team_mapping"] or None
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], tm, merge_ids=merge)
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        assert (rows == 0) == (name == "empty")
        assert handle.occupancy_device(t) == (None, None)                                                # none before the first call
        assert handle.L.eagle_post_device_occupancy(t._t, None, None) == lib.E_INVALID
        assert handle.L.eagle_post_occupancy_values(t._t, None, None, None, None, None) == lib.E_INVALID   # no result yet
        mm = lib.minimap_params(4, voronoi=bool(t.team_mapping))
        before = handle.minimap(t, mm, 0, min(rows, 2))
        off, sc, names = OR.default_selections(cols, t.team_mapping)
        assert (off, sc, names) == oc.default_selections(t.columns, t.team_mapping)
        for fps, R, sigma, max_gap in ((case["fps"], 1, 2.0, None), (case["fps"], 4, 0.0, 3), (5, 2, 0.7, 1000)):       # each call replaces the one before
            p = lib.occupancy_params(fps, R, sigma, max_gap)
            exp = OR.occupancy(values, t.rows, cols, off, sc, R, sigma, p.max_gap)
            _check(handle.occupancy(t, p, off, sc), exp, (name, R))
            assert handle.L.eagle_post_occupancy_values(t._t, None, None, None, None, None) == 0        # any pointer may be NULL
            d_g, d_b = handle.occupancy_device(t)
            cells = 7140 * R * R * (len(off) - 1)
            assert d_g and d_b and d_g != t.device_values and d_b - d_g >= 8 * cells                     # grids, then counts, then the bytes
            s = len(off) - 1 - 1                                                                         # the ball's map as a picture
            assert np.array_equal(handle.occupancy_picture(t, s, 2, 8, (255, 255, 255)), OR.picture(exp["bytes"][s], R, 2, 8, (255, 255, 255)))
            d = oc.occupancy(handle, t, fps, R, sigma, max_gap)
            assert np.array_equal(d["grids"], exp["grids"].astype(np.float64) / fps) and [dict(n) for n in names] == [{k: v for k, v in e.items() if k in ("kind", "id", "team")} for e in d["selections"]]
            assert [e["seconds"] for e in d["selections"]] == [int(n) / fps for n in exp["total"]]
            for e, cnt in zip(d["selections"], exp["counts"]):
                assert (e["thirds"], e["channels"]) == OR.shares(cnt, R)
        # the minimap of the same table: byte for byte what it was (the picture above changed the handle's marking mask in between)
        assert np.array_equal(handle.minimap(t, mm, 0, min(rows, 2)), before)
        if rows:
            assert np.array_equal(before, MR.frames_bgr(values, cols, t.team_mapping, 0, min(rows, 2), 4, 8, voronoi=int(bool(t.team_mapping))))
    finally:
        t.close()


def test_refusals(handle):
    L = handle.L
    c = OC.single("eight", [(5.5 + k, 7.5) for k in range(8)])
    values, frames = np.ascontiguousarray(c["values"]), np.ascontiguousarray(c["frames"])
    base = np.array([(k, i, v, 0) for k, i, v in c["columns"]] + [(lib.POST_BALL, 0, 0, 0)], lib.POSTCOL_DTYPE)      # 0-3 bounds, 4 player, 5 its video column, 6 ball
    values = np.ascontiguousarray(np.concatenate([values, values[4:5]]))
    rows = len(frames)
    grids, by, counts = np.full((2, 68, 105), 7.0, np.float32), np.full((2, 68, 105), 7, np.uint8), np.full((2, 68, 105), 7, np.int32)
    total, outside = np.full(2, 7, np.int64), np.full(2, 7, np.int64)
    P = lib.occupancy_params
    good = P(5)
    I = lambda *v: np.array(v, np.int32)

    def op(params=good, values_p=vp(values), frames_p=vp(frames), cols_p=vp(base), off=I(0, 1, 2), sel=I(4, 6), n_sel=2, nrows=rows, ncols=len(base)):
        rc = L.eagle_op_occupancy(0, values_p, frames_p, cols_p, nrows, ncols, None if params is None else C.byref(params), None if off is None else vp(off),
                                  None if sel is None else vp(sel), n_sel, vp(grids), vp(by), vp(total), vp(outside), vp(counts))
        msg = L.eagle_last_error(None).decode()
        if rc:
            assert (grids == 7.0).all() and (by == 7).all() and (counts == 7).all() and (total == 7).all() and (outside == 7).all()
        return rc, msg

    same, back = frames.copy(), frames.copy()
    same[3] = same[2]
    back[4] = back[3] - 1
    bad = [dict(params=None), dict(params=P(0)), dict(params=P(-5)), dict(params=P(5, max_gap=0)), dict(params=P(5, max_gap=-1)), dict(params=P(5, 0)), dict(params=P(5, 3)),
           dict(params=P(5, 8)), dict(params=P(5, -1)), dict(params=P(5, sigma=float("nan"))), dict(params=P(5, sigma=float("inf"))), dict(params=P(5, sigma=-0.1)),
           dict(params=P(5, sigma=np.nextafter(10.0, 20.0))), dict(values_p=None), dict(frames_p=None), dict(cols_p=None), dict(nrows=-1), dict(ncols=-1), dict(n_sel=-1),
           dict(off=None), dict(sel=None), dict(off=I(1, 1, 2)), dict(off=I(0, 2, 1)), dict(off=I(0, -1, 2)), dict(sel=I(4, 7)), dict(sel=I(-1, 6)), dict(sel=I(5, 6)),
           dict(sel=I(0, 6)), dict(sel=I(4, 3)), dict(off=I(0, 2, 2), sel=I(4, 4)), dict(off=I(0, 0, 3), sel=I(6, 4, 6)), dict(frames_p=vp(same)), dict(frames_p=vp(back)),
           dict(params=P(5, max_gap=2 ** 28)), dict(params=P(5, max_gap=2 ** 31 - 1)), dict(params=P(5, max_gap=2 ** 27), off=I(0, 2, 2))]
    for kw in bad:
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and msg, kw
    assert op(params=P(5, max_gap=2 ** 28 - 1))[0] == 0 and counts.sum() == 16 and total.tolist() == [8, 8]      # just below the 2^31 bound; the two maps are equal
    assert op(params=P(5, sigma=10.0), off=I(0, 2, 2))[0] == 0 and total.tolist() == [16, 0]              # a column with another in one selection, sigma at its end
    gw, gh = C.c_int(0), C.c_int(0)
    assert L.eagle_occupancy_size(C.byref(P(5, 4)), C.byref(gw), C.byref(gh)) == 0 and (gw.value, gh.value) == (420, 272) == lib.control_size(lib.control_params(4))
    assert L.eagle_occupancy_size(C.byref(P(5, 3)), C.byref(gw), C.byref(gh)) == lib.E_INVALID and L.eagle_occupancy_size(C.byref(good), None, C.byref(gh)) == lib.E_INVALID
    assert L.eagle_occupancy_size(None, C.byref(gw), C.byref(gh)) == lib.E_INVALID

    # the picture's operator entry
    pic = np.full((68 * 2 + 16, 105 * 2 + 16, 3), 9, np.uint8)
    cell = np.zeros((68, 105), np.uint8)
    for R, S, M, g_p, o_p in ((3, 2, 8, vp(cell), vp(pic)), (1, 3, 8, vp(cell), vp(pic)), (1, 0, 8, vp(cell), vp(pic)), (1, 34, 8, vp(cell), vp(pic)), (1, 2, 1, vp(cell), vp(pic)),
                              (1, 2, -2, vp(cell), vp(pic)), (1, 2, 66, vp(cell), vp(pic)), (1, 2, 8, None, vp(pic)), (1, 2, 8, vp(cell), None)):
        assert L.eagle_op_occupancy_picture(0, g_p, R, S, M, 0xffffff, o_p) == lib.E_INVALID and L.eagle_last_error(None) and (pic == 9).all(), (R, S, M)

    # the handle entries
    case = post_cases.BY_NAME["goalkeeper_fold"]
    t = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, case["team_mapping"])
    small = handle.postprocess(post_cases.records_of(case), 25, 1280, case["team_mapping"], max_bytes=1 << 20)
    other = lib.Handle(batch=1, frame_h=140, frame_w=204)
    try:
        cols = _columns(t)
        off, sc, _ = OR.default_selections(cols, t.team_mapping)
        off, sc = np.array(off, np.int32), np.array(sc, np.int32)
        n_sel = len(off) - 1
        call = lambda hh, tt, p, o=off, s=sc, n=n_sel: L.eagle_post_occupancy(hh, tt, None if p is None else C.byref(p), None if o is None else vp(o), None if s is None else vp(s), n)
        video = next(i for i, k in enumerate(cols) if k[2])
        bound = next(i for i, k in enumerate(cols) if k[0] == lib.POST_BOUNDARY and not k[2])
        for p in (None, P(0), P(25, max_gap=0), P(25, 5), P(25, sigma=float("nan")), P(25, sigma=10.5)):
            assert call(handle._h, t._t, p) == lib.E_INVALID and L.eagle_last_error(handle._h)
        for kw in (dict(o=None), dict(s=None), dict(n=-1), dict(o=I(0, 1), s=I(video), n=1), dict(o=I(0, 1), s=I(bound), n=1), dict(o=I(0, 1), s=I(len(cols)), n=1),
                   dict(o=I(0, 2), s=I(sc[0], sc[0]), n=1), dict(o=I(1, 2), s=sc[:2], n=1)):
            assert call(handle._h, t._t, good, **kw) == lib.E_INVALID and L.eagle_last_error(handle._h), kw
        assert call(handle._h, None, good) == lib.E_INVALID and call(None, t._t, good) == lib.E_INVALID
        assert call(other._h, t._t, good) == lib.E_INVALID and b"another handle" in L.eagle_last_error(other._h)
        assert handle.occupancy_device(t) == (None, None)                                                # a refused call leaves no result
        out = np.full((68 * 2, 105 * 2, 3), 9, np.uint8)
        assert L.eagle_occupancy_picture(handle._h, t._t, 0, 2, 0, 0xffffff, vp(out)) == lib.E_INVALID and b"no occupancy" in L.eagle_last_error(handle._h)
        assert L.eagle_post_occupancy_values(None, None, None, None, None, None) == lib.E_INVALID
        # the table's memory budget: one map at 1 cell per metre fits a 1 MiB table, the default selections at 4 cells per metre do not
        assert call(handle._h, small._t, P(25, 4)) == lib.E_INVALID and b"budget" in L.eagle_last_error(handle._h)
        assert call(handle._h, small._t, P(25, 1), o=I(0, 1), s=sc[:1], n=1) == 0
        # n_sel == 0 is a result without maps; then a real one
        assert call(handle._h, t._t, good, o=I(0), s=None, n=0) == 0 and handle.occupancy_device(t) == (None, None)
        assert L.eagle_post_occupancy_values(t._t, None, None, None, None, None) == 0
        assert L.eagle_occupancy_picture(handle._h, t._t, 0, 2, 0, 0xffffff, vp(out)) == lib.E_INVALID
        assert call(handle._h, t._t, good) == 0
        for sel, S, M, o_p, hh in ((-1, 2, 0, vp(out), handle._h), (n_sel, 2, 0, vp(out), handle._h), (0, 3, 0, vp(out), handle._h), (0, 34, 0, vp(out), handle._h),
                                   (0, 2, 1, vp(out), handle._h), (0, 2, 66, vp(out), handle._h), (0, 2, 0, None, handle._h), (0, 2, 0, vp(out), other._h)):
            assert L.eagle_occupancy_picture(hh, t._t, sel, S, M, 0xffffff, o_p) == lib.E_INVALID and (out == 9).all(), (sel, S, M)
        assert L.eagle_occupancy_picture(None, t._t, 0, 2, 0, 0xffffff, vp(out)) == lib.E_INVALID
        assert L.eagle_occupancy_picture(handle._h, t._t, n_sel - 1, 2, 0, 0xffffff, vp(out)) == 0 and (out != 9).any()      # the handle still works
    finally:
        t.close()
        small.close()
        other.close()


def test_cli_occupancy(tmp_path):
    import glob
    import json
    import os
    from eagle_amd import cli, occupancy as oc
    out = str(tmp_path / "out")
    assert cli.main(["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed", "--merge-ids", "--occupancy",
                     "--occupancy-grid", "2", "--occupancy-sigma", "1.5", "--occupancy-pictures", "--minimap-scale", "4"]) == 0
    grids = np.load(os.path.join(out, "occupancy.npy"))
    d = oc.from_json(json.load(open(os.path.join(out, "occupancy.json"))), grids)
    sel = d["selections"]
    assert grids.dtype == np.float64 and grids.shape == (len(sel), 136, 210) and (d["fps"], d["cells_per_metre"], d["sigma"]) == (5, 2, 1.5)
    assert sel[-1]["kind"] == "ball" and all(set(e) >= {"kind", "seconds", "outside_seconds", "thirds", "channels"} for e in sel)
    assert all(abs(sum(e["thirds"]) - 1.0) < 1e-12 and abs(sum(e["channels"]) - 1.0) < 1e-12 for e in sel if e["seconds"] > 0)
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(out, "occupancy_*.ppm")))
    assert names == sorted(["occupancy_ball.ppm"] + ["occupancy_team%d.ppm" % e["team"] for e in sel if e["kind"] == "team"])
    w, h = MR.size(4, 8)
    for n in names:
        raw = open(os.path.join(out, n), "rb").read()
        head = b"P6\n%d %d\n255\n" % (w, h)
        assert raw.startswith(head) and len(raw) == len(head) + w * h * 3
        rgb = np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)
        assert (rgb[MR.markings(4, 8)] == 255).all()
