"""Line registration on the GPU (include/eagle.h, eagle_op_linefit / eagle_linefit_*; csrc/linefit.hip): the refined matrices as raw bytes, every field of
the frame records and the line-pixel masks equal tests/linefit_ref.py — np.array_equal, no tolerance — for the constructed cases of tests/linefit_cases.py;
two runs give the same bytes; the handle entries at 720 x 1280, from a device pointer and from host memory with the staging forced to one frame per pass,
equal the rule and leave the handle's records alone; CoordinateModel.refine_lines re-projects with the library's own arithmetic and returns rejected
frames byte for byte; every refusal names the value; the CLI writes lines.json and, without --refine-lines, what it wrote before."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import linefit_cases as LC
import linefit_ref as R
from eagle_amd import lib, linefit, synth

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in LC.all_cases()}
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def _params(p):
    return lib.linefit_params(**p)


def _same(got, exp, what):
    out, rec, masks = got
    eo, er, em = exp
    assert out.tobytes() == eo.tobytes(), (what, "Hs_out")
    for f in R.FRAME_DTYPE.names:
        assert np.array_equal(rec[f], er[f]), (what, f, rec[f], er[f])
    assert masks.shape == em.shape and np.array_equal(masks, em), (what, "masks")


@pytest.mark.parametrize("name", list(CASES))
def test_op_linefit_equals_the_rule(name):
    c = CASES[name]
    exp = R.linefit(c["frames"], c["Hs"], c["valid"], c["boxes"], c["p"])
    c["expect"](*exp)
    _same(lib.op_linefit(c["frames"], c["Hs"], c["valid"], _params(c["p"]), c["boxes"]), exp, name)


def test_two_runs_give_the_same_bytes_and_masks_are_optional():
    c = CASES["sixty_five_frames"]
    a = lib.op_linefit(c["frames"], c["Hs"], c["valid"], _params(c["p"]))
    b = lib.op_linefit(c["frames"], c["Hs"], c["valid"], _params(c["p"]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    o, r, m = lib.op_linefit(c["frames"], c["Hs"], c["valid"], _params(c["p"]), masks=False)
    assert m is None and o.tobytes() == a[0].tobytes() and r.tobytes() == a[1].tobytes()


def test_no_frames_succeed_and_write_nothing():
    o, r, m = lib.op_linefit(np.zeros((0, 12, 20, 3), np.uint8), np.zeros((0, 9)), np.zeros(0, np.uint8))
    assert o.shape == (0, 9) and r.shape == (0,) and m.shape == (0, 12, 1)


# ---- through a handle, at 720 x 1280 ------------------------------------------------------------------------------------------------
DISTURB = np.array([[1.012, .006, .9], [-.004, .99, -.6], [1e-4, -2e-4, 1]])


@functools.lru_cache(None)
def _clip():
    """three synthetic frames, the disturbed true matrices (the second frame without a map), the records with the players' boxes, and the rule's result"""
    views = ((3, 0), (3, 200), (11, 400))
    frames = np.stack([synth.frame(s, t) for s, t in views])
    Hs = np.stack([(DISTURB @ np.linalg.inv(synth.camera(s, t))).reshape(9) for s, t in views])
    valid = np.array([1, 0, 1], np.uint8)
    recs = np.zeros(3, lib.RESULT_DTYPE)
    boxes = []
    for i, (s, t) in enumerate(views):
        bx = np.array([b[1:] for b in synth.player_boxes(s, t)], np.float32)
        boxes.append(bx)
        recs[i]["n_det"] = len(bx)
        for k, name in enumerate(("x1", "y1", "x2", "y2")):
            recs[i]["det"][name][:len(bx)] = bx[:, k]
    return frames, Hs, valid, recs, R.linefit(frames, Hs, valid, boxes, R.params())


def test_handle_entries_equal_the_rule():
    frames, Hs, valid, recs, exp = _clip()
    assert [int(t) for t in exp[1]["status"]] == [R.ACCEPTED, R.NO_MAP, R.ACCEPTED]
    hd = lib.Handle(batch=1, frame_h=720, frame_w=1280)
    try:
        _same(hd.linefit(frames, Hs, valid, recs, masks=True, max_staging_bytes=1), exp, "one frame per pass")
        _same(hd.linefit(frames, Hs, valid, recs, masks=True), exp, "one pass")
        d = hd.upload(frames)
        try:
            _same(hd.linefit_device(d, 3, Hs, valid, recs, masks=True), exp, "device")
        finally:
            hd.free(d)
        with pytest.raises(lib.EagleError, match="max_staging_bytes -1"):
            hd.linefit(frames, Hs, valid, recs, max_staging_bytes=-1)
        o, r, m = hd.linefit(frames[:0], Hs[:0], valid[:0])
        assert o.shape == (0, 9) and len(r) == 0 and m is None
    finally:
        hd.close()


def test_refusals_name_the_value():
    L = lib.load()
    c = CASES["rung_affine"]
    frames, Hs, valid = c["frames"], np.ascontiguousarray(c["Hs"]), c["valid"]
    n, h, w, _ = frames.shape
    out, rec = np.full((n, 9), 7.0), np.zeros(n, lib.LINEFIT_FRAME_DTYPE)
    good = dict(frames=frames, Hs=Hs, valid=valid, boxes=None, off=None, out=out, rec=rec, n=n, h=h, w=w)

    def refused(match, p=None, **kw):
        a = dict(good, **kw)
        q = lib.linefit_params() if p is None else p
        code = L.eagle_op_linefit(0, vp(a["frames"]), a["n"], a["h"], a["w"], vp(a["Hs"]), vp(a["valid"]), vp(a["boxes"]), vp(a["off"]), None if q is False else C.byref(q),
                                  vp(a["out"]), vp(a["rec"]), None)
        msg = L.eagle_last_error(None).decode()
        assert code == lib.E_INVALID and match in msg, (code, msg)
        assert (out == 7.0).all()

    for field, bad, match in (("k", 0, "k 0"), ("k", 65, "k 65"), ("tau", 0, "tau 0"), ("tau", 1021, "tau 1021"), ("rounds", -1, "rounds -1"), ("rounds", 17, "rounds 17"),
                              ("model", 0, "model 0"), ("model", 4, "model 4"), ("min_points", 0, "min_points 0"), ("min_per_line", 0, "min_per_line 0"),
                              ("box_pad", -1.0, "box_pad -1"), ("box_pad", float("nan"), "box_pad nan"), ("radius", 9.0, "radius 9"), ("radius_min", 3.0, "radius_min 3"),
                              ("radius_min", 0.0, "radius_min 0"), ("radius_factor", 0.0, "radius_factor 0"), ("radius_factor", 1.5, "radius_factor 1.5"),
                              ("max_shift", -1.0, "max_shift -1"), ("max_step", 0.0, "max_step 0"), ("max_step", 65.0, "max_step 65")):
        refused(match, lib.linefit_params(**{field: bad}))
    p = lib.linefit_params()
    p.reserved[2] = 5
    refused("reserved[2] is 5", p)
    refused("parameters are NULL", False)
    refused("n is -2", n=-2)
    refused("frames are NULL", frames=None)
    refused("homographies are NULL", Hs=None)
    refused("valid flags are NULL", valid=None)
    refused("Hs_out or frames_out is NULL", rec=None)
    refused("0 x 20", h=0, w=20)
    refused("16385", h=16385, w=4)
    bx = np.zeros((2, 4), np.float32)
    refused("come together", boxes=bx)
    refused("box_off[0] is 1", boxes=bx, off=np.array([1, 2], np.int32))
    refused("-1 boxes", boxes=bx, off=np.array([0, -1], np.int32))
    refused("301 boxes", boxes=np.zeros((301, 4), np.float32), off=np.array([0, 301], np.int32))


# ---- CoordinateModel.refine_lines -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(state_dicts):
    from eagle_amd.coordinate_model import CoordinateModel
    hs, ys = state_dicts
    cm = CoordinateModel(frame_hw=(720, 1280), batch=3, hrnet_state_dict=hs, detector_state_dict=ys)
    yield cm
    cm.handle.close()


def _fields_equal(a, b):
    """every named field, as bytes (the 4 bytes of tail padding of a record are not the library's to define)"""
    if a.dtype.names is None:
        return a.tobytes() == b.tobytes()
    return all(_fields_equal(np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])) for k in a.dtype.names)


def _constructed_records(model):
    """the records of the three frames with the handle-test's matrices put in place of what the seeded random networks found, and the players' boxes as
    their detections"""
    frames, Hs, valid, boxed, _ = _clip()
    recs = np.ascontiguousarray(model.process_records(frames)).copy()
    for i in range(3):
        recs[i]["H"] = Hs[i]
        recs[i]["H_valid"] = valid[i]
        n = int(boxed[i]["n_det"])
        recs[i]["n_det"] = n
        for name in ("x1", "y1", "x2", "y2"):
            recs[i]["det"][name][:n] = boxed[i]["det"][name][:n]
        det = recs[i]["det"]
        det["cls"][:n], det["reported"][:n], det["id"][:n] = 0, 1, np.arange(n)
        for a, b in (("bx1", "x1"), ("by1", "y1"), ("bx2", "x2"), ("by2", "y2")):
            det[a][:n] = det[b][:n].astype(np.int32)
        det["foot_x"][:n], det["foot_y"][:n] = (det["bx1"][:n] + det["bx2"][:n]) // 2, det["by2"][:n]
    return frames, Hs, recs


def test_refine_lines_reprojects_with_the_librarys_arithmetic(model):
    frames, Hs, recs = _constructed_records(model)
    exp = _clip()[4]
    before = recs.copy()
    process_a = model.process_records(frames).copy()
    coords, report = model.refine_lines(frames, recs, fps=5)
    assert _fields_equal(model.process_records(frames), process_a)                           # a call between two process calls leaves the handle's records as they were
    assert report.Hs[[0, 2]].tobytes() == exp[0][[0, 2]].tobytes() and report.frames.tobytes() == exp[1].tobytes()      # (frame 1 has no matrix in effect)
    flags = (report.frames["status"] == lib.LINEFIT_ACCEPTED).astype(np.uint8)
    assert list(flags) == [1, 0, 1]
    want = model.handle.reproject(before.copy(), report.Hs, flags)
    _, got, own = model._last
    assert _fields_equal(got, want) and _fields_equal(before[1:2], got[1:2])
    for i in (0, 2):
        assert np.array_equal(got[i]["H"], report.Hs[i]) and got[i]["H_valid"] and not np.array_equal(got[i]["H"], before[i]["H"])
        n = int(got[i]["n_det"])
        assert not np.array_equal(got[i]["det"]["pitch_x"][:n], before[i]["det"]["pitch_x"][:n])
        for oid, d in coords[i]["Coordinates"].get("Player", {}).items():
            if d["Transformed_Coordinates"] is not None:
                assert d["Transformed_Coordinates"] == [int(got[i]["det"]["pitch_x"][oid]), int(got[i]["det"]["pitch_y"][oid])]
    assert model.annotate(frames, coords).shape == frames.shape                              # the new dict is the remembered one
    js = linefit.to_json(report, rows=True)
    assert js["totals"]["status"]["accepted"] == 2 and js["totals"]["status"]["no_map"] == 1 and len(js["rows"]) == 3
    assert js["totals"]["rms_after"] < js["totals"]["rms_before"] and js["params"]["model"] == "projective"
    json.dumps(js)


def test_refine_lines_with_every_frame_rejected_returns_the_records_byte_for_byte(model):
    frames, Hs, recs = _constructed_records(model)
    coords, report = model.refine_lines(frames, recs, fps=5, max_shift=0.01)
    assert [int(s) for s in report.frames["status"]] == [lib.LINEFIT_SHIFT, lib.LINEFIT_NO_MAP, lib.LINEFIT_SHIFT]
    assert _fields_equal(model._last[1], recs) and report.Hs[[0, 2]].tobytes() == Hs[[0, 2]].tobytes()
    first = model.get_coordinates(frames, 5, num_homography=5, num_keypoint_detection=5, verbose=False)
    again, rep = model.refine_lines(frames, first, min_points=10 ** 9)
    assert json.dumps(again, default=float) == json.dumps(first, default=float) and not (rep.frames["status"] == lib.LINEFIT_ACCEPTED).any()


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_refine_lines(tmp_path):
    from eagle_amd import cli
    np.save(tmp_path / "clip.npy", synth.clip(0, 3))
    common = ["--fps", "5", "--synthetic-weights", "--batch", "2", "--every-frame", "--clip", str(tmp_path / "clip.npy")]
    out, plain, plain2 = (str(tmp_path / d) for d in ("out", "plain", "plain2"))
    assert cli.main(common + ["--out", out, "--refine-lines", "--refine-lines-rounds", "3", "--refine-lines-radius", "2", "--refine-lines-min-radius", "0.4",
                              "--refine-lines-max-shift", "2.5", "--refine-lines-contrast", "180", "--refine-lines-model", "affine", "--refine-lines-rows"]) == 0
    assert cli.main(common + ["--out", plain]) == 0 and cli.main(common + ["--out", plain2]) == 0
    d = json.load(open(os.path.join(out, "lines.json")))
    assert set(d) == {"params", "totals", "far_frames", "rows"} and len(d["rows"]) == 3 and d["totals"]["frames"] == 3
    assert d["params"] == dict(d["params"], rounds=3, radius=2.0, radius_min=0.4, max_shift=2.5, tau=180, model="affine", k=4)
    assert sum(d["totals"]["status"].values()) == 3 and all(0 <= r["line_pixels"] <= 720 * 1280 and r["frame"] == i for i, r in enumerate(d["rows"]))
    assert json.load(open(os.path.join(out, "metadata.json")))["homography"] == "refined"
    # without --refine-lines the files are what they were: no lines.json, no metadata key, the same coordinates in two runs
    assert sorted(os.listdir(plain)) == sorted(os.listdir(plain2)) and "lines.json" not in os.listdir(plain) and "lines.json" in os.listdir(out)
    assert "homography" not in json.load(open(os.path.join(plain, "metadata.json")))
    assert open(os.path.join(plain, "raw_coordinates.json"), "rb").read() == open(os.path.join(plain2, "raw_coordinates.json"), "rb").read()
    for bad in (["--refine-lines-rows"], ["--refine-lines-model", "affine"], ["--refine-lines-rounds", "2"]):
        with pytest.raises(SystemExit):
            cli.main(common + ["--out", out] + bad)
    with pytest.raises(SystemExit):
        cli.main(common + ["--out", out, "--refine-lines", "--refine-lines-radius", "9"])
