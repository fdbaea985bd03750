"""The minimap on the GPU (include/eagle.h, eagle_minimap_* / eagle_op_minimap; csrc/minimap.hip): every output byte equals the numpy contract of
tests/minimap_ref.py — no tolerances — for the constructed tables of tests/minimap_cases.py in BGR, NV12 and I420, dense and padded; through a
handle on a table eagle_postprocess built (host and device entries, a row window, no side effect on the handle); every refusal; the command line."""
import ctypes as C
import os

import numpy as np
import pytest

import annot_ref as A
import minimap_cases as MC
import minimap_ref as R
import post_cases
from eagle_amd import lib, postprocess, synth, weights

pytestmark = pytest.mark.gpu
FMTS = ["bgr", "nv12", "i420"]


def _params(c, **over):
    kw = dict(c["kw"], **over)
    return lib.minimap_params(c["S"], c["M"], kw.get("voronoi", 0), kw.get("footprint", 1), kw.get("player_radius", 0), kw.get("ball_radius", 0))


def _expected(name, fmt, layout=None, fill=0):
    fr = MC.reference(name)
    return A.annotate(fr, [[] for _ in fr], fmt, layout, fill)


def _padded_layout(fmt, h, w):
    if fmt == "bgr":
        return {"y_pitch": 3 * w + 40, "frame_stride": (3 * w + 40) * (h + 3)}
    yp = w + 64
    return {"y_pitch": yp, "c_offset": yp * (h + 16), "c_pitch": yp if fmt == "nv12" else w // 2 + 32, "frame_stride": yp * (2 * h + 40)}


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", [c["name"] for c in MC.CASES])
def test_op_minimap_equals_contract(name, fmt):
    c = MC.BY_NAME[name]
    got = lib.op_minimap(c["values"], c["columns"], c["mapping"], _params(c), c["row0"], c["n"], fmt)
    exp = _expected(name, fmt)
    assert got.size == exp.size and np.array_equal(got.reshape(-1), exp)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["sites22", "footprints_a"])
def test_padded_layout_leaves_uncovered_bytes(name, fmt):
    c = MC.BY_NAME[name]
    w, h = R.size(c["S"], c["M"])
    lay = _padded_layout(fmt, h, w)
    exp = _expected(name, fmt, lay, fill=0xA5)
    out = np.full(exp.size, 0xA5, np.uint8)
    got = lib.op_minimap(c["values"], c["columns"], c["mapping"], _params(c), c["row0"], c["n"], fmt, lay, out=out)
    assert np.array_equal(got, exp)
    slack = exp.size - c["n"] * (h * w * 3 if fmt == "bgr" else h * w * 3 // 2)
    assert slack > 0 and (got == 0xA5).sum() >= slack                # every byte the layout does not cover is still 0xA5


# ---- through a handle -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


def test_handle_minimap_equals_contract_and_has_no_side_effect(handle):
    frames = synth.clip(0, 2)
    before = handle.process(frames).copy()
    captures = handle.timings().graph_captures
    case = post_cases.BY_NAME["goalkeeper_fold"]
    tm = case["team_mapping"]
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], tm)
    reader = None
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        assert rows == 16 and any(k == R.GOALKEEPER and not v for k, _, v in cols)
        S, M = 2, 2
        w, h = R.size(S, M)
        par = lib.minimap_params(S, M, voronoi=True)
        ref = R.frames_bgr(values, cols, tm, 0, rows, S, M, voronoi=1)
        assert len({fr.tobytes() for fr in ref}) > 1
        reader = lib.Handle(batch=rows, frame_h=h, frame_w=w)
        for fmt in FMTS:
            exp = A.annotate(ref, [[] for _ in ref], fmt).reshape((rows, h, w, 3) if fmt == "bgr" else (rows, h * 3 // 2, w))
            got = handle.minimap(t, par, fmt=fmt)
            assert got.shape == exp.shape and np.array_equal(got, exp), fmt
            assert np.array_equal(handle.minimap(t, par, 5, 3, fmt), exp[5:8]), fmt      # a window
            pinned = handle.host_buffer(exp.nbytes)
            try:
                pinned[:] = 0
                assert np.array_equal(handle.minimap(t, par, fmt=fmt, out=pinned)[: exp.nbytes], exp.reshape(-1)), fmt
            finally:
                handle.host_free(pinned)
            # the device entry into an eagle_device_alloc buffer, fetched byte for byte: a second handle whose frames are h x w BGR reads the buffer
            # as a clip and copies it out with an empty overlay (16 dense 4:2:0 pictures are the bytes of 8 such frames; device pointers are process-wide)
            d_out = handle.upload(np.full(exp.nbytes, 0xA5, np.uint8))
            try:
                handle.minimap_device(t, d_out, par, 0, rows, fmt)
                nb = exp.nbytes // (h * w * 3)
                assert nb * h * w * 3 == exp.nbytes
                assert np.array_equal(reader.annotate(d_out, nb, np.zeros(nb, lib.RESULT_DTYPE), None, "bgr").reshape(-1), exp.reshape(-1)), fmt
            finally:
                handle.free(d_out)
        assert handle.minimap(t, par, 3, 0).shape == (0, h, w, 3)                  # n == 0: success, nothing written
        # more pictures than one pass of the host entry's 32 MB staging holds: 12 rows of 1264 x 820 BGR (3.1 MB each) go in passes of 10 and 2
        big = lib.minimap_params(12, 2)
        wb, hb = lib.minimap_size(big)
        assert 10 * wb * hb * 3 <= 32 << 20 < 11 * wb * hb * 3
        assert np.array_equal(handle.minimap(t, big, 2, 12), R.frames_bgr(values, cols, tm, 2, 12, 12, 2))
        from eagle_amd.minimap import minimap, size
        assert size(2, 2) == (w, h) and np.array_equal(minimap(handle, t, 2, 2, voronoi=True, rows=(5, 3)), ref[5:8])
    finally:
        t.close()
        if reader is not None:
            reader.close()
    after = handle.process(frames)
    assert all(np.array_equal(before[k], after[k]) for k in lib.RESULT_DTYPE.names)
    assert handle.timings().graph_captures == captures


def test_refusals(handle):
    c = MC.BY_NAME["sites1"]
    L = handle.L
    values = np.ascontiguousarray(c["values"])
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    ids, vals = np.array([1], np.int32), np.array([0], np.int32)
    w, h = R.size(2, 0)
    out = np.full(w * h * 3, 0x5A, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def op(params=lib.minimap_params(2, 0), values_p=vp(values), cols_p=vp(cols), rows=1, ids_p=vp(ids), row0=0, n=1, fmt=0, lay=None, out_p=vp(out)):
        rc = L.eagle_op_minimap(0, values_p, cols_p, rows, len(cols), ids_p, vp(vals), 1, None if params is None else C.byref(params), row0, n, fmt,
                                None if lay is None else C.byref(lay), out_p)
        msg = L.eagle_last_error(None).decode()
        assert (out == 0x5A).all()
        return rc, msg

    bad = [dict(params=None), dict(values_p=None), dict(cols_p=None), dict(out_p=None),
           dict(params=lib.minimap_params(3, 0)), dict(params=lib.minimap_params(0, 0)), dict(params=lib.minimap_params(34, 0)),
           dict(params=lib.minimap_params(2, 1)), dict(params=lib.minimap_params(2, 66)), dict(params=lib.minimap_params(2, -2)),
           dict(params=lib.minimap_params(2, 0, player_radius=-1)), dict(params=lib.minimap_params(2, 0, player_radius=9)),
           dict(params=lib.minimap_params(2, 0, ball_radius=-1)), dict(params=lib.minimap_params(2, 0, ball_radius=9)),
           dict(params=lib.minimap_params(2, 0, voronoi=True), ids_p=None),
           dict(row0=1), dict(row0=-1), dict(n=2), dict(n=-1), dict(rows=0), dict(fmt=3),
           dict(fmt=1, lay=lib.EagleYuvLayout(y_pitch=w - 2)), dict(fmt=0, lay=lib.EagleYuvLayout(y_pitch=3 * w - 1)), dict(fmt=2, lay=lib.EagleYuvLayout(c_pitch=-8)),
           dict(fmt=1, lay=lib.EagleYuvLayout(c_offset=w * (h - 1))), dict(fmt=2, lay=lib.EagleYuvLayout(frame_stride=w * h))]
    for kw in bad:
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and msg, kw
    assert op(n=0)[0] == 0                                            # n == 0 is success and writes nothing
    assert op(params=lib.minimap_params(2, 0, player_radius=8, ball_radius=8), n=0)[0] == 0
    # the handle entries: the same checks, plus the table's own
    case = post_cases.BY_NAME["goalkeeper_fold"]
    t = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, None)         # no mapping
    empty = postprocess.process_data(handle, post_cases.records_of(post_cases.BY_NAME["empty"]), 25, 1280, {})
    try:
        big = np.full(16 * w * h * 3, 0x5A, np.uint8)

        def hd(entry, table, params, row0, n, fmt=0, lay=None, dst=vp(big)):
            rc = entry(handle._h, table, row0, n, None if params is None else C.byref(params), fmt, None if lay is None else C.byref(lay), dst)
            msg = L.eagle_last_error(handle._h).decode()
            assert (big == 0x5A).all()
            return rc, msg

        good = lib.minimap_params(2, 0)
        for entry in (L.eagle_minimap_frames, L.eagle_minimap_device_frames):
            for args in ((t._t, lib.minimap_params(2, 0, voronoi=True), 0, 1), (t._t, good, 0, 17), (t._t, good, 16, 1), (t._t, good, -1, 1), (t._t, good, 0, -1),
                         (None, good, 0, 1), (t._t, None, 0, 1), (t._t, lib.minimap_params(5, 0), 0, 1), (empty._t, good, 0, 1)):
                rc, msg = hd(entry, *args)
                assert rc == lib.E_INVALID and msg, args
            assert hd(entry, t._t, good, 0, 1, dst=None)[0] == lib.E_INVALID
            assert hd(entry, t._t, good, 0, 1, 1, lib.EagleYuvLayout(y_pitch=w - 2))[0] == lib.E_INVALID
            assert hd(entry, t._t, good, 16, 0)[0] == 0 and hd(entry, empty._t, good, 0, 0)[0] == 0
        assert handle.minimap(t, good, 0, 1).shape == (1, h, w, 3)      # the handle still works
    finally:
        t.close(); empty.close()


def test_cli_minimap(tmp_path):
    from eagle_amd import cli
    out = str(tmp_path / "out")
    common = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out]
    assert cli.main(common + ["--processed", "--minimap", "--minimap-voronoi", "--minimap-scale", "4"]) == 0
    blob = open(os.path.join(out, "minimap.y4m"), "rb").read()
    header, rest = blob.split(b"\n", 1)
    tok = header.decode().split()
    w, h = R.size(4, 8)
    assert tok[0] == "YUV4MPEG2" and f"W{w}" in tok and f"H{h}" in tok and "F5:1" in tok
    import json
    rows = len(json.load(open(os.path.join(out, "processed_data.json"))))
    assert len(rest) == rows * (6 + w * h * 3 // 2)                   # per row "FRAME\n" + w h 3 / 2 bytes of payload
    with pytest.raises(SystemExit) as e:
        cli.main(common + ["--minimap"])
    assert e.value.code == 2
