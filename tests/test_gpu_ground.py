"""The ground layer on the GPU (include/eagle.h, eagle_op_ground / eagle_ground_*; csrc/ground.hip): the pictures and the covered counts equal
tests/ground_ref.py — np.array_equal, no tolerance — for the constructed cases of tests/ground_cases.py in every format their size admits, with and
without the kernel's per-tile cull; padded layouts keep the bytes they do not cover; the handle entries, from a device pointer and from host memory with
the staging forced to one frame per pass, equal the operator entry; every refusal names the value and leaves the output alone; offside_view with
empty shape lists is annotate(table=...), and on a constructed clip with pass events it is the rule followed by the library's annotate_prims."""
import ctypes as C

import numpy as np
import pytest

import ground_cases as GC
import ground_ref as R
from eagle_amd import lib

pytestmark = pytest.mark.gpu

vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype and np.array_equal(got, exp), what


def _run(c, fmt="bgr", **kw):
    shapes, off = GC.library_shapes(c)
    return lib.op_ground(c["frames"], c["Hs"], c["valid"], shapes, off, lib.ground_params(**c["key"], **kw), fmt)


@pytest.mark.parametrize("name", [c["name"] for c in GC.CASES])
def test_op_ground_equals_the_rule(name):
    c = GC.BY_NAME[name]
    pics, cov = GC.reference(name)
    for fmt in c["formats"]:
        got, got_cov = _run(c, fmt)
        _same(got, GC.dense(name, fmt), (name, fmt))
        _same(got_cov, cov, (name, fmt, "covered"))
    got, got_cov = _run(c, no_cull=True)                      # the cull changes no byte
    _same(got, pics, (name, "no cull"))
    _same(got_cov, cov, (name, "no cull", "covered"))


def test_minus_3_h_gives_the_same_bytes_and_the_orders_differ():
    _same(_run(GC.BY_NAME["horizon_times_minus_3"])[0], _run(GC.BY_NAME["horizon_264x34"])[0], "-3 H")
    both = _run(GC.BY_NAME["overlap_both_orders"])[0]
    assert not np.array_equal(both[0], both[1])


@pytest.mark.parametrize("name, fmt, layout", GC.PADDED)
def test_padded_layouts_keep_the_fill(name, fmt, layout):
    c = GC.BY_NAME[name]
    exp, cov = R.ground(c["frames"], c["Hs"], c["valid"], c["shapes"], c["key"], GC.FMT[fmt], layout, fill=0xA5)
    assert (exp == 0xA5).sum() > len(c["frames"]) * 50
    out = np.full(exp.nbytes + 64, 0xA5, np.uint8)
    shapes, off = GC.library_shapes(c)
    got, got_cov = lib.op_ground(c["frames"], c["Hs"], c["valid"], shapes, off, None, fmt, layout, out)
    assert np.array_equal(got[: exp.nbytes], exp) and (got[exp.nbytes:] == 0xA5).all() and np.array_equal(got_cov, cov)


def test_two_runs_give_the_same_bytes():
    a, b = _run(GC.BY_NAME["shapes_16_then_0"]), _run(GC.BY_NAME["shapes_16_then_0"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- through a handle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shift_264x34", "shapes_16_then_0", "no_map"])
def test_handle_entries_equal_the_operator_entry(name):
    c = GC.BY_NAME[name]
    n, h, w, _ = c["frames"].shape
    shapes, off = GC.library_shapes(c)
    p = lib.ground_params(**c["key"])
    hd = lib.Handle(batch=1, frame_h=h, frame_w=w)
    try:
        for fmt in c["formats"]:
            exp, exp_cov = lib.op_ground(c["frames"], c["Hs"], c["valid"], shapes, off, p, fmt)
            for bound in (0, 1, h * w * 3, 2 * h * w * 3 + 5):                    # one pass; one frame per pass (twice); two frames per pass
                got, cov = hd.ground(c["frames"], c["Hs"], c["valid"], shapes, off, p, fmt, max_staging_bytes=bound)
                _same(got, exp, (name, fmt, bound))
                _same(cov, exp_cov, (name, fmt, bound, "covered"))
            d = hd.upload(c["frames"])
            d_out = hd.upload(np.full(exp.nbytes, 0xA5, np.uint8))
            try:
                cov = hd.ground_device(d, n, c["Hs"], c["valid"], shapes, off, d_out, p, fmt)
                _same(cov, exp_cov, (name, fmt, "device covered"))
                if fmt == "bgr":                                                  # read back through the annotation stage with nothing to draw
                    _same(hd.annotate(d_out, n, np.zeros(n, lib.RESULT_DTYPE), None, "bgr"), exp, (name, "device"))
            finally:
                hd.free(d)
                hd.free(d_out)
        d = hd.upload(c["frames"])
        try:
            with pytest.raises(lib.EagleError, match="the clip itself"):
                hd.ground_device(d, n, c["Hs"], c["valid"], shapes, off, d, p)
        finally:
            hd.free(d)
        with pytest.raises(lib.EagleError, match="max_staging_bytes"):
            hd.ground(c["frames"], c["Hs"], c["valid"], shapes, off, p, max_staging_bytes=-1)
        assert hd.ground(c["frames"][:0], c["Hs"][:0], c["valid"][:0], shapes[:0], off[:1], p)[0].shape == (0, h, w, 3)
    finally:
        hd.close()


def test_refusals_name_the_value_and_leave_the_output_alone():
    L = lib.load()
    c = GC.BY_NAME["tails_38x18"]
    frames, Hs, valid = c["frames"], np.ascontiguousarray(c["Hs"]), np.ascontiguousarray(c["valid"])
    n, h, w, _ = frames.shape
    shapes, off = GC.library_shapes(c)
    out, cov = np.full((n, h, w, 3), 0x5A, np.uint8), np.full(n, 77, np.uint32)
    untouched = lambda: (out == 0x5A).all() and (cov == 77).all()

    def op(sh=shapes, of=off, par=None, n_=n, h_=h, w_=w, fmt=0, layout=None, null=()):
        q = lib.ground_params() if par is None else par
        a = dict(frames=frames, Hs=Hs, valid=valid, shapes=sh, off=of, out=out, p=q)
        a.update({k: None for k in null})
        lay = None if layout is None else C.byref(lib._yuv_layout(layout))
        code = L.eagle_op_ground(0, vp(a["frames"]), n_, h_, w_, vp(a["Hs"]), vp(a["valid"]), vp(a["shapes"]), vp(a["off"]), None if a["p"] is None else C.byref(a["p"]), fmt, lay,
                                 vp(a["out"]), vp(cov))
        return code, L.eagle_last_error(None).decode()

    for change, text in GC.SHAPE_REFUSALS:
        bad = shapes.copy()
        for k, v in change.items():
            bad[1][k] = v
        code, msg = op(sh=bad)
        assert code == lib.E_INVALID and text in msg and untouched(), (change, msg)
    for change, text in GC.PARAM_REFUSALS:
        q = lib.ground_params()
        for k, v in change.items():
            setattr(q, k, v)
        code, msg = op(par=q)
        assert code == lib.E_INVALID and text in msg and untouched(), (change, msg)
    seventeen = np.concatenate([shapes[:1]] * 17)
    for kw, text in ((dict(null=("frames",)), "frames are NULL"), (dict(null=("Hs",)), "homographies are NULL"), (dict(null=("valid",)), "valid flags are NULL"),
                     (dict(null=("shapes",)), "shapes are NULL"), (dict(null=("off",)), "off is NULL"), (dict(null=("out",)), "output is NULL"), (dict(null=("p",)), "parameters are NULL"),
                     (dict(of=np.array([1, 2, 3, 3], np.int32)), "off[0] is 1"), (dict(of=np.array([0, 2, 1, 3], np.int32)), "frame 1 has -1 shapes"),
                     (dict(sh=seventeen, of=np.array([0, 17, 17, 17], np.int32)), "17 shapes"), (dict(n_=-1), "n -1"), (dict(h_=0), "0 x 38"), (dict(w_=16385), "18 x 16385"),
                     (dict(fmt=7), ""), (dict(layout={"y_pitch": 3 * w - 1}), "pitch"), (dict(fmt=1, layout={"c_offset": 5}), ""), (dict(fmt=1, h_=17), "even"), (dict(fmt=2, w_=37), "even")):
        code, msg = op(**kw)
        assert code == lib.E_INVALID and text in msg and untouched(), (kw, msg)
    code, _ = op(n_=0)                                        # n == 0 succeeds and writes nothing
    assert code == 0 and untouched()
    code, _ = op()
    assert code == 0 and np.array_equal(out, GC.reference("tails_38x18")[0]) and np.array_equal(cov, GC.reference("tails_38x18")[1])


# ---- the offside view: the table's offside result as shapes, the ground stage, the table's annotation on top -------------------------------------
VH, VW = 128, 256
VIEW_H = [0.5, 0, -10, 0, 0.5, 2, 0, 0, 1]                     # image -> pitch: x = u / 2 - 10, y = v / 2 + 2
HOP_MAPPING = {i + 1: i % 2 for i in range(8)}


def _hop_records(n, players=8, keepers=2, seed=5, H=None, px=2, ox=10, oy=-2):
    """n records of `players` players and `keepers` goalkeepers on a slow random walk, team 0 (even detections) on the left; the ball sits on a player for
    three frames and hops to another (ids are detection index + 1); every record carries H (VIEW_H), and a box whose foot point is the pixel
    (px (x + ox), px (y + oy)) of its pitch point"""
    r = np.random.default_rng(seed)
    k = players + keepers + 1
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = k, 1, 1
    recs["H"] = np.array(VIEW_H if H is None else H, np.float64).reshape(recs["H"].shape[1:])
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    x0 = np.array([r.uniform(10, 70) if j % 2 == 0 else r.uniform(35, 95) for j in range(players)] + [3.0, 102.0][:keepers] + [0.0])
    pos = np.stack([x0, r.uniform(5, 63, k)], 1)[None] + np.cumsum(r.normal(0, 0.7, (n, k, 2)), 0)
    holder = np.repeat(r.integers(0, players, n // 3 + 1), 3)[:n]
    pos[:, k - 1] = pos[np.arange(n), holder]
    pos = np.clip(pos, 0, [105, 68]).astype(np.int32)
    d, j = recs["det"], np.arange(k)
    d["reported"][:, :k], d["in_bounds"][:, :k], d["conf"][:, :k] = 1, 1, 0.9
    d["cls"][:, :k] = np.where(j == k - 1, 2, np.where(j >= players, 1, 0))[None]
    d["id"][:, :k] = (j + 1)[None]
    fx, fy = px * (pos[:, :, 0] + ox), px * (pos[:, :, 1] + oy)
    d["bx1"][:, :k], d["bx2"][:, :k], d["by1"][:, :k], d["by2"][:, :k] = fx - 3, fx + 3, fy - 20, fy
    d["foot_x"][:, :k], d["foot_y"][:, :k] = fx, fy
    d["pitch_x"][:, :k], d["pitch_y"][:, :k] = pos[:, :, 0], pos[:, :, 1]
    return recs


def _ref_lists(shapes, off):
    """the library's shape records -> ground_ref's lists"""
    mk = lambda s: dict(kind=int(s["kind"]), a=tuple(int(t) for t in s["a"]), colour=int(s["colour"]), alpha=int(s["alpha"]), flags=int(s["flags"]))
    return [[mk(s) for s in shapes[off[i]: off[i + 1]]] for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def view():
    """a handle of 128 x 256, a model around it that runs no network, a clip of grass, the records of the hopping ball and their table with a
    possession and an offside result"""
    from eagle_amd.coordinate_model import CoordinateModel
    hd = lib.Handle(batch=1, frame_h=VH, frame_w=VW)
    model = CoordinateModel.__new__(CoordinateModel)
    model.handle = hd
    recs = _hop_records(40)
    frames = GC.green(40, VH, VW, 21)
    t = hd.postprocess(recs, 25, VW, HOP_MAPPING)
    owner = hd.possession(t, lib.possession_params(25, 1024.0, 1, 1000))[1]
    res = hd.offside(t, lib.offside_params(lib.OFFSIDE_DIR_RIGHT, 0, 0.5))
    yield model, frames, recs, t, owner, res
    t.close()
    hd.close()


def test_offside_view_without_shapes_is_the_annotated_table(view):
    from eagle_amd import ground
    model, frames, recs, t, owner, res = view
    n = len(t.rows)
    empty = (np.zeros(0, lib.GROUND_SHAPE_DTYPE), np.zeros(n + 1, np.int32))
    for fmt in ("bgr", "i420"):
        pics, info = ground.offside_view(model, frames, recs, t, out_format=fmt, shape_lists=empty)
        _same(pics, model.annotate(frames, recs, out_format=fmt, table=t), fmt)
        assert [r["covered"] for r in info["rows"]] == [0] * n and [r["shapes"] for r in info["rows"]] == [0] * n


@pytest.mark.parametrize("team", ["possession", "both", 1])
def test_offside_view_is_the_rule_under_the_annotation(view, team):
    from eagle_amd import ground, topview
    from eagle_amd.processor import Processor
    model, frames, recs, t, owner, res = view
    hd = model.handle
    rows = np.asarray(t.rows, np.int64)
    n = len(rows)
    shapes, off = ground.offside_shapes(t, res, team, owner=owner)
    assert off[-1] > 2 * n if team == "both" else off[-1] > n // 2
    Hs, valid, kind = topview.homographies(recs, carry=True)
    mid, cov = R.frames_bgr(frames[rows], Hs[rows], valid[rows], _ref_lists(shapes, off))
    assert cov.sum() > 0
    lists = [t.overlay(r, recs[int(f)]) for r, f in enumerate(rows)]
    d = hd.upload(mid)
    try:
        exp = hd.annotate_prims(d, n, np.concatenate(lists), np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int32))
    finally:
        hd.free(d)
    pics, info = Processor(model).offside_view(frames, recs, t, team)
    _same(pics, exp, team)
    assert [r["covered"] for r in info["rows"]] == [int(c) for c in cov] and [r["shapes"] for r in info["rows"]] == list(np.diff(off)) and info["rows"][0]["homography"] == 1


def test_offside_stills_one_picture_per_pass_with_a_verdict(view):
    from eagle_amd import ground
    from eagle_amd.processor import Processor
    model, frames, recs, t, owner, res = view
    hd = model.handle
    ev, oev = hd.events(t), hd.offside_events(t)
    ok = [k for k in range(len(ev)) if int(ev[k]["kind"]) == lib.EVENT_PASS and int(oev[k]["status"]) == lib.OFFSIDE_EV_OK]
    assert len(ok) >= 2
    stills = Processor(model).offside_stills(frames, recs, t)
    assert [k for k, _, _ in stills] == ok and all(p.shape == (VH, VW, 3) and p.dtype == np.uint8 for _, p, _ in stills)
    k, pic, info = stills[0]
    r = int(ev[k]["release_row"])
    f = int(t.rows[r])
    g = int(oev[k]["group"])
    ring = ground._ring(t.values, ev[k]["to_col"], r, ground.VERDICT_COLOURS[int(oev[k]["verdict"])], True)
    sh, off = lib.ground_shape_lists([ground.line_shapes(int(oev[k]["line_qx"]), g, g == 0, 0.25, True, True) + [ring]])
    mid, cov = R.frames_bgr(frames[f: f + 1], [VIEW_H], [1], _ref_lists(sh, off))
    prims = t.overlay(r, recs[f])
    d = hd.upload(mid)
    try:
        exp = hd.annotate_prims(d, 1, prims, np.array([0, len(prims)], np.int32))
    finally:
        hd.free(d)
    _same(pic, exp[0], "still 0")
    assert info["covered"] == int(cov[0]) > 0 and info["verdict"] in ("onside", "close", "offside") and info["frame"] == f


def test_cli_offside_view_and_stills(tmp_path, monkeypatch):
    """the detections of the constructed clip whose ball hops stand in for the random networks' (the model's records and the team mapping are substituted,
    as in test_gpu_offside); everything behind them is the command line's own path"""
    import json
    import os

    from eagle_amd import cli, records
    from eagle_amd.coordinate_model import CoordinateModel
    from eagle_amd.processor import Processor
    recs = _hop_records(30, H=[0.1, 0, -10, 0, 0.1, -2, 0, 0, 1], px=10, ox=10, oy=2)          # 720 x 1280: x = u / 10 - 10, y = v / 10 - 2

    def get_coordinates(self, frames, fps, **kw):
        coords = {i: records.to_reference_dict(r, i, fps) for i, r in enumerate(recs)}
        self._last = (coords, recs, np.ones(len(recs), bool))
        return coords

    monkeypatch.setattr(CoordinateModel, "get_coordinates", get_coordinates)
    monkeypatch.setattr(Processor, "get_team_mapping", lambda self, frames, coords, pixel_format="bgr": dict(HOP_MAPPING))
    out = str(tmp_path / "out")
    assert cli.main(["--frames", "30", "--fps", "25", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed", "--offside", "--possession", "--offside-view",
                     "--offside-view-team", "both", "--offside-view-width", "0.5", "--offside-view-no-key", "--offside-stills"]) == 0
    info = json.load(open(os.path.join(out, "offside_view.json")))
    n = len(info["rows"])
    y4m = open(os.path.join(out, "offside_view.y4m"), "rb").read()
    assert y4m.startswith(b"YUV4MPEG2 W1280 H720") and y4m.count(b"FRAME\n") >= n >= 20 and len(y4m) > n * 1280 * 720 * 3 // 2
    assert info["params"] == {"team": "both", "width": 0.5, "zone": True, "rings": True, "keyed": False, "key_min": 48, "key_lead": 16}
    assert sum(r["shapes"] >= 4 for r in info["rows"]) >= 20 and sum(r["covered"] > 1000 for r in info["rows"]) >= 20 and all(r["homography"] == 1 for r in info["rows"])
    passes = [p for p in json.load(open(os.path.join(out, "offside.json")))["passes"] if p["status"] == "ok"]
    stills = sorted(f for f in os.listdir(out) if f.startswith("offside_") and f.endswith(".ppm"))
    assert len(stills) == len(passes) >= 1
    ppm = open(os.path.join(out, stills[0]), "rb").read()
    assert ppm.startswith(b"P6\n1280 720\n255\n") and len(ppm) == len(b"P6\n1280 720\n255\n") + 1280 * 720 * 3
