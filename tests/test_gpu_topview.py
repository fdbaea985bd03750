"""The top view on the GPU (include/eagle.h, eagle_op_topview / eagle_topview_*; csrc/topview.hip): warped frames, mosaic, cnt and the residual triples
equal tests/topview_ref.py — np.array_equal, no tolerance — for the constructed cases of tests/topview_cases.py in BGR, NV12 and I420; padded layouts
keep the bytes they do not cover; through a handle at 720 x 1280 from a device pointer and from host memory, with the staging forced to one frame per
pass; a call between two process calls leaves the records as they were; every refusal names the value; the command line writes its files."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import annot_ref as A
import topview_cases as TC
import topview_ref as R
from eagle_amd import lib, synth, topview, weights

pytestmark = pytest.mark.gpu

vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
FMT = {"bgr": A.BGR, "nv12": A.NV12, "i420": A.I420}
ALL = lib.TOPVIEW_VIDEO | lib.TOPVIEW_MOSAIC | lib.TOPVIEW_RESIDUAL


def _cp(p):
    return lib.topview_params(**p)


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype and np.array_equal(got, exp), what


@pytest.mark.parametrize("name", [c["name"] for c in TC.CASES])
def test_op_topview_equals_the_rule(name):
    c = TC.BY_NAME[name]
    vid, pic, cnt, rs, rc, cv = TC.reference(name)
    got = lib.op_topview(c["frames"], c["Hs"], c["valid"], _cp(c["p"]), c["boxes"], ALL)
    _same(got["video"], vid, (name, "video"))
    _same(got["mosaic"], pic, (name, "mosaic"))
    _same(got["cnt"], cnt, (name, "cnt"))
    for k, e in (("res_sum", rs), ("res_cnt", rc), ("covered", cv)):
        assert got[k].dtype == e.dtype and [int(t) for t in got[k]] == [int(t) for t in e], (name, k)
    n, (Hc, W) = len(vid), vid.shape[1:3]
    for fmt in ("nv12", "i420") if n else ():
        exp = A.annotate(vid, [[]] * n, FMT[fmt]).reshape(n, Hc * 3 // 2, W)
        _same(lib.op_topview(c["frames"], c["Hs"], c["valid"], _cp(dict(c["p"], mask_boxes=0)), None, lib.TOPVIEW_VIDEO, fmt)["video"], exp, (name, fmt))


@pytest.mark.parametrize("name, fmt, layout", [
    ("frame_5x7_odd_pitch", "bgr", {"y_pitch": 3 * 210 + 5, "frame_stride": (3 * 210 + 5) * 136 + 11}),
    ("pinhole_trapezoid", "nv12", {"y_pitch": 214 + 10, "c_offset": 224 * 140 + 32, "c_pitch": 214 + 6, "frame_stride": 224 * 140 + 32 + 220 * 70 + 9}),
    ("pinhole_trapezoid", "i420", {"y_pitch": 214 + 3, "c_offset": 217 * 140 + 1, "c_pitch": 107 + 2, "v_offset": 217 * 140 + 1 + 109 * 70 + 5,
                                   "frame_stride": 217 * 140 + 1 + 2 * 109 * 70 + 5 + 7})])
def test_padded_layouts_keep_the_fill(name, fmt, layout):
    c = TC.BY_NAME[name]
    exp = R.video(c["frames"], c["Hs"], c["valid"], c["p"], FMT[fmt], layout, fill=0xA5)
    assert (exp == 0xA5).sum() > len(c["frames"]) * 100
    out = np.full(exp.nbytes + 64, 0xA5, np.uint8)
    got = lib.op_topview(c["frames"], c["Hs"], c["valid"], _cp(c["p"]), None, lib.TOPVIEW_VIDEO, fmt, layout, out)["video"]
    assert np.array_equal(got[: exp.nbytes], exp) and (got[exp.nbytes:] == 0xA5).all()


def test_two_runs_give_the_same_bytes():
    c = TC.BY_NAME["mosaic_65_frames"]
    a = lib.op_topview(c["frames"], c["Hs"], c["valid"], _cp(c["p"]), None, ALL)
    b = lib.op_topview(c["frames"], c["Hs"], c["valid"], _cp(c["p"]), None, ALL)
    assert all(np.array_equal(a[k], b[k]) for k in a)


# ---- through a handle -----------------------------------------------------------------------------------------------------------
H, W = 720, 1280
P720 = R.params(4, 6, markings=1, mask_boxes=1, box_pad=3.0, background=0x203040)


@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=H, frame_w=W)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


@pytest.fixture(scope="module")
def clip720():
    """three synthetic frames, three constructed maps (a scale, a pinhole camera, a scale handed over as -3 H) and records with two boxes each"""
    frames = np.stack([synth.frame(0, 3 * t) for t in range(3)])
    Hs = np.stack([TC.adj(TC.scale_map(12.0, 10.0, -50.0)), TC.adj(TC.pinhole((52.5, -45.0, 28.0), (52.5, 28.0, 0.0), 1500.0, 639.5, 359.5)),
                   -3 * TC.adj(TC.scale_map(11.0, 40.0, -20.0))])
    valid = np.ones(3, np.uint8)
    recs = np.zeros(3, lib.RESULT_DTYPE)
    boxes = []
    for i in range(3):
        b = np.array([[100 + 50 * i, 200, 400 + 50 * i, 420.5], [700, 100 + 30 * i, 1000.25, 300]], np.float32)
        recs[i]["n_det"] = 2
        for k, key in enumerate(("x1", "y1", "x2", "y2")):
            recs[i]["det"][key][:2] = b[:, k]
        recs[i]["det"]["x1"][2:5] = 0, 0, 0                                   # beyond n_det: not a box
        recs[i]["det"]["x2"][2], recs[i]["det"]["y2"][2] = 1280, 720
        boxes.append(b)
    exp = R.topview(frames, Hs, valid, boxes, P720)
    assert exp[2].max() == 3 and (exp[4] > 0).all() and exp[3].any()
    return frames, Hs, valid, recs, exp


def test_handle_device_and_host_entries(handle, clip720):
    frames, Hs, valid, recs, (vid, pic, cnt, rs, rc, cv) = clip720
    p = _cp(P720)
    Wc, Hc = lib.topview_size(p)
    _same(handle.topview(frames, Hs, valid, p), vid, "host video")
    for fmt in ("nv12", "i420"):
        _same(handle.topview(frames, Hs, valid, p, fmt), A.annotate(vid, [[]] * 3, FMT[fmt]).reshape(3, Hc * 3 // 2, Wc), ("host video", fmt))
    d = handle.upload(frames)
    d_out = handle.upload(np.full(vid.nbytes, 0xA5, np.uint8))
    d_acc = handle.topview_accumulator(p)
    reader = lib.Handle(batch=3, frame_h=Hc, frame_w=Wc)
    try:
        handle.topview_device(d, 3, Hs, valid, p, d_out)
        _same(reader.annotate(d_out, 3, np.zeros(3, lib.RESULT_DTYPE), None, "bgr"), vid, "device video")
        handle.topview_mosaic_add(d, Hs, valid, p, d_acc, recs, n=3)
        got_pic, got_cnt = handle.topview_mosaic_finish(d_acc, p)
        _same(got_pic, pic, "device mosaic")
        _same(got_cnt, cnt, "device cnt")
        for g, e in zip(handle.topview_residuals(d, Hs, valid, p, d_acc, recs, n=3), (rs, rc, cv)):
            _same(g, e, "device residual")
        # two halves into one accumulator equal the whole: the second call does not reset
        handle.topview_mosaic_add(d, Hs[:2], valid[:2], p, d_acc, recs[:2], n=2)
        d2 = C.c_void_p(d.value + 2 * H * W * 3)
        handle.topview_mosaic_add(d2, Hs[2:], valid[2:], p, d_acc, recs[2:], reset=False, n=1)
        _same(handle.topview_mosaic_finish(d_acc, p)[1], cnt, "two calls")
    finally:
        reader.close()
        for x in (d, d_out, d_acc):
            handle.free(x)


def test_host_fed_mosaic_one_frame_per_pass_equals_one_pass(handle, clip720):
    frames, Hs, valid, recs, (vid, pic, cnt, rs, rc, cv) = clip720
    p = _cp(P720)
    d_acc = handle.topview_accumulator(p)
    try:
        for bound in (0, 1, H * W * 3, 2 * H * W * 3 + 5):                       # one pass; one frame per pass (twice); two frames per pass
            handle.topview_mosaic_add(frames, Hs, valid, p, d_acc, recs, max_staging_bytes=bound)
            got_pic, got_cnt = handle.topview_mosaic_finish(d_acc, p)
            _same(got_pic, pic, ("mosaic", bound))
            _same(got_cnt, cnt, ("cnt", bound))
            for g, e in zip(handle.topview_residuals(frames, Hs, valid, p, d_acc, recs, max_staging_bytes=bound), (rs, rc, cv)):
                _same(g, e, ("residual", bound))
    finally:
        handle.free(d_acc)
    res = topview.mosaic(handle, frames, _records(recs, Hs), params=p)
    _same(res.mosaic, pic, "topview.mosaic")
    assert list(res.kind) == [1, 1, 1] and topview.to_json(res)["frames"][0]["covered"] == int(cv[0])


def _records(recs, Hs):
    out = recs.copy()
    out["H_valid"], out["H"] = 1, Hs
    return out


def test_a_call_between_two_process_calls_leaves_the_records_unchanged(handle, clip720):
    frames, Hs, valid, recs, exp = clip720
    two = np.stack([synth.frame(0, 3), synth.noise_frame(2)])
    before = handle.process(two)
    p = _cp(P720)
    _same(handle.topview(frames, Hs, valid, p), exp[0], "between")
    res = topview.mosaic(handle, frames, _records(recs, Hs), params=p)
    _same(res.cnt, exp[2], "between, cnt")
    after = handle.process(two)
    assert before.tobytes() == after.tobytes()


def test_refusals_name_the_value():
    L = lib.load()
    c = TC.BY_NAME["frame_4x4"]
    frames, Hs, valid = c["frames"], np.ascontiguousarray(c["Hs"]), np.ascontiguousarray(c["valid"])
    n, h, w, _ = frames.shape
    Wc, Hc = R.size(2, 2)
    out, pic, cnt = np.full((n, Hc, Wc, 3), 0x5A, np.uint8), np.full((Hc, Wc, 3), 0x5A, np.uint8), np.full((Hc, Wc), 0x5A5A5A5A, np.uint32)
    rs, rc, cv = np.full(n, 77, np.uint64), np.full(n, 77, np.uint32), np.full(n, 77, np.uint32)
    untouched = lambda: (out == 0x5A).all() and (pic == 0x5A).all() and (cnt == 0x5A5A5A5A).all() and (rs == 77).all() and (rc == 77).all() and (cv == 77).all()

    def op(change=None, n_=n, h_=h, w_=w, mode=ALL, fmt=0, layout=None, par=True, **null):
        q = _cp(dict(c["p"], **(change or {})))
        a = dict(frames=frames, Hs=Hs, valid=valid, out=out, pic=pic, cnt=cnt, rs=rs, rc=rc, cv=cv)
        a.update({k: None for k in null})
        lay = None if layout is None else C.byref(lib._yuv_layout(layout))
        code = L.eagle_op_topview(0, vp(a["frames"]), n_, h_, w_, vp(a["Hs"]), vp(a["valid"]), None, None, C.byref(q) if par else None, mode, fmt, lay, vp(a["out"]),
                                  vp(a["pic"]), vp(a["cnt"]), vp(a["rs"]), vp(a["rc"]), vp(a["cv"]))
        return code, L.eagle_last_error(None).decode()

    for change, text in TC.REFUSALS:
        code, msg = op(change)
        assert code == lib.E_INVALID and text in msg and untouched(), (change, msg)
    for kw, text in ((dict(n_=-1), "n -1"), (dict(n_=lib.TOPVIEW_MAX_FRAMES + 1), "above"), (dict(par=False), "NULL"), (dict(frames=1), "frames are NULL"),
                     (dict(Hs=1), "homographies are NULL"), (dict(valid=1), "valid flags are NULL"), (dict(out=1), "out is NULL"), (dict(pic=1), "mosaic_out"),
                     (dict(cnt=1), "cnt_out"), (dict(rs=1), "res_sum"), (dict(cv=1), "covered"), (dict(h_=0), "0 x 4"), (dict(w_=16385), "4 x 16385"),
                     (dict(mode=0), "mode"), (dict(mode=8), "mode"), (dict(fmt=7), ""), (dict(layout={"y_pitch": 3 * Wc - 1}), "pitch"),
                     (dict(fmt=1, layout={"c_offset": 5}), "")):
        code, msg = op(**kw)
        assert code == lib.E_INVALID and text in msg and untouched(), (kw, msg)
    q = _cp(c["p"])
    q.reserved[2] = 1
    assert L.eagle_op_topview(0, vp(frames), n, h, w, vp(Hs), vp(valid), None, None, C.byref(q), ALL, 0, None, vp(out), vp(pic), vp(cnt), vp(rs), vp(rc), vp(cv)) == lib.E_INVALID
    assert "reserved" in L.eagle_last_error(None).decode() and untouched()
    off = np.array([0, 301, 301], np.int32)                                      # 301 boxes in a frame
    bx = np.zeros((301, 4), np.float32)
    q = _cp(dict(c["p"], mask_boxes=1))
    assert L.eagle_op_topview(0, vp(frames), n, h, w, vp(Hs), vp(valid), vp(bx), vp(off), C.byref(q), ALL, 0, None, vp(out), vp(pic), vp(cnt), vp(rs), vp(rc), vp(cv)) == lib.E_INVALID
    assert "301 boxes" in L.eagle_last_error(None).decode() and untouched()
    w_, h_ = C.c_int(-1), C.c_int(-1)
    assert L.eagle_topview_size(None, C.byref(w_), C.byref(h_)) == lib.E_INVALID and L.eagle_topview_size(C.byref(_cp(c["p"])), None, C.byref(h_)) == lib.E_INVALID and w_.value == -1
    code, _ = op(n_=0, mode=lib.TOPVIEW_VIDEO | lib.TOPVIEW_RESIDUAL)            # n == 0 succeeds and writes nothing
    assert code == 0 and untouched()
    code, _ = op()
    assert code == 0 and np.array_equal(out, TC.reference("frame_4x4")[0]) and np.array_equal(cnt, TC.reference("frame_4x4")[2])


def test_handle_refusals(handle, clip720):
    frames, Hs, valid, recs, _ = clip720
    L, hd = handle.L, handle._h
    p = _cp(P720)
    small = np.zeros((1, 4, 4, 3), np.uint8)
    with pytest.raises(lib.EagleError, match="720"):                              # a frame size other than the handle's
        handle.topview(small, Hs[:1], valid[:1], p)
    d_acc = handle.topview_accumulator(p)
    try:
        q = _cp(dict(P720, mask_boxes=1))
        assert L.eagle_topview_mosaic_frames(hd, vp(frames), 3, 0, vp(Hs), vp(valid), None, C.byref(q), d_acc, 1) == lib.E_INVALID
        assert "mask_boxes needs the records" in L.eagle_last_error(hd).decode()
        assert L.eagle_topview_mosaic_frames(hd, vp(frames), 3, -1, vp(Hs), vp(valid), vp(recs), C.byref(q), d_acc, 1) == lib.E_INVALID
        assert "max_staging_bytes" in L.eagle_last_error(hd).decode()
        assert L.eagle_topview_mosaic_device(hd, None, lib.TOPVIEW_MAX_FRAMES + 1, vp(Hs), vp(valid), None, C.byref(p), d_acc, 1) == lib.E_INVALID
        assert L.eagle_topview_mosaic_frames(hd, vp(frames), 3, 0, vp(Hs), vp(valid), vp(recs), C.byref(q), None, 1) == lib.E_INVALID
        assert "d_acc is NULL" in L.eagle_last_error(hd).decode()
        bad = recs.copy()
        bad[1]["n_det"] = 301
        assert L.eagle_topview_residual_frames(hd, vp(frames), 3, 0, vp(Hs), vp(valid), vp(bad), C.byref(q), d_acc, vp(np.zeros(3, np.uint64)), vp(np.zeros(3, np.uint32)),
                                               vp(np.zeros(3, np.uint32))) == lib.E_INVALID
        assert "n_det 301" in L.eagle_last_error(hd).decode()
        out = np.zeros(16, np.uint8)
        assert L.eagle_topview_frames(hd, vp(frames), 3, vp(Hs), vp(valid), C.byref(_cp(dict(P720, scale=5))), 0, None, vp(out)) == lib.E_INVALID
        assert "scale 5" in L.eagle_last_error(hd).decode()
        assert L.eagle_topview_frames(hd, vp(frames), 3, vp(Hs), vp(valid), C.byref(p), 0, C.byref(lib._yuv_layout({"y_pitch": 7})), vp(out)) == lib.E_INVALID
        assert L.eagle_topview_mosaic_finish(hd, d_acc, C.byref(p), None, None) == lib.E_INVALID
        assert handle.topview(frames[:0], Hs[:0], valid[:0], p).shape == (0, 284, 432, 3)          # n == 0
    finally:
        handle.free(d_acc)


def test_cli_topview(tmp_path):
    from eagle_amd import cli
    np.save(tmp_path / "clip.npy", synth.clip(0, 3))
    out, plain = str(tmp_path / "out"), str(tmp_path / "plain")
    common = ["--fps", "5", "--synthetic-weights", "--batch", "2", "--every-frame", "--clip", str(tmp_path / "clip.npy")]
    assert cli.main(common + ["--out", out, "--topview", "--topview-scale", "2", "--topview-margin", "4", "--topview-markings", "--topview-carry", "--topview-mosaic",
                              "--topview-mask-boxes", "2", "--topview-step", "2", "--topview-min-count", "1", "--topview-suspect", "1.5"]) == 0
    assert cli.main(common + ["--out", plain]) == 0
    Wc, Hc = R.size(2, 4)
    y4m = open(os.path.join(out, "topview.y4m"), "rb").read()
    assert y4m.startswith(b"YUV4MPEG2 W%d H%d" % (Wc, Hc)) and y4m.count(b"FRAME\n") >= 3 and len(y4m) > 3 * Wc * Hc * 3 // 2
    ppm = open(os.path.join(out, "topview_mosaic.ppm"), "rb").read()
    assert ppm.startswith(b"P6\n%d %d\n255\n" % (Wc, Hc)) and len(ppm) == len(b"P6\n%d %d\n255\n" % (Wc, Hc)) + Wc * Hc * 3
    cnt = np.load(os.path.join(out, "topview_count.npy"))
    assert cnt.shape == (Hc, Wc) and cnt.dtype == np.uint32 and cnt.max() <= 2
    d = json.load(open(os.path.join(out, "topview.json")))
    assert len(d["frames"]) == 3 and d["params"]["scale"] == 2 and d["params"]["margin"] == 4 and d["params"]["step"] == 2 and d["params"]["suspect"] == 1.5
    assert d["params"]["mask_boxes"] == 1 and d["params"]["box_pad"] == 2.0 and d["params"]["carry"] is True and set(d) == {"params", "frames", "median_residual", "suspect_frames"}
    # a run without --topview writes what it wrote before: the same files, the same coordinates
    assert not any(f.startswith("topview") for f in os.listdir(plain))
    assert open(os.path.join(out, "raw_coordinates.json"), "rb").read() == open(os.path.join(plain, "raw_coordinates.json"), "rb").read()
