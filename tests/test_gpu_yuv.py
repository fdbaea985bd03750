"""Decoder-native input on the GPU (include/eagle.h, eagle_*_yuv; csrc/yuv.hip): the conversion equals the numpy restatement of cv2's
COLOR_YUV2BGR_NV12 / _I420 (tests/yuv_ref.py) byte for byte, and every record of an NV12 / I420 call equals the record of the BGR call on the
converted frames — host-fed (pageable, pinned and padded), device-fed, under graph replay, with plain launches, at 1080p, through the Processor
and the flow cadence.  Bad layouts come back as EagleError and leave the handle usable."""
import numpy as np
import pytest

import yuv_ref as Y
from eagle_amd import lib, synth, weights

pytestmark = pytest.mark.gpu
FMTS = ["nv12", "i420"]


def _encode(fmt, bgr):
    return synth.bgr_to_nv12(bgr) if fmt == "nv12" else synth.bgr_to_i420(bgr)


def _padded_layout(fmt, h, w):
    """a decoder surface: pitch padded by 64 bytes, chroma after h + 16 rows, chroma pitch padded too"""
    yp = w + 64
    return {"y_pitch": yp, "c_offset": yp * (h + 16), "c_pitch": yp if fmt == "nv12" else w // 2 + 32}


def _handle(state_dicts, batch, h=720, w=1280):
    hd = lib.Handle(batch=batch, frame_h=h, frame_w=w)
    weights.load_into(hd, list(state_dicts))
    return hd


# ---- 1. the conversion alone ------------------------------------------------------------------------------------------------
def _op_case(fmt, case):
    r = np.random.default_rng(11)
    if case == "random720":
        n, h, w = 2, 720, 1280
        planes = (r.integers(0, 256, (n, h, w)), r.integers(0, 256, (n, h // 2, w // 2)), r.integers(0, 256, (n, h // 2, w // 2)))
        return planes, None
    if case == "extremes":
        ys, cs = [0, 15, 16, 235, 255], [0, 1, 127, 128, 255]
        combos = [(a, b, c) for a in ys for b in cs for c in cs]                 # 125 blocks of 2 x 2 pixels
        h, w = 2 * 5, 2 * 25
        Yp = np.zeros((1, h, w), np.int64); U = np.zeros((1, h // 2, w // 2), np.int64); V = np.zeros_like(U)
        for k, (a, b, c) in enumerate(combos):
            by, bx = divmod(k, w // 2)
            Yp[0, 2 * by: 2 * by + 2, 2 * bx: 2 * bx + 2] = a
            U[0, by, bx], V[0, by, bx] = b, c
        return (Yp, U, V), None
    if case == "tail":
        n, h, w = 3, 18, 34                                                     # 34 = 4 strips of 8 + a 2-pixel tail; odd rows not 4-byte aligned
        return (r.integers(0, 256, (n, h, w)), r.integers(0, 256, (n, h // 2, w // 2)), r.integers(0, 256, (n, h // 2, w // 2))), None
    n, h, w = 2, 64, 200                                                        # padded decoder layout, 200 = 25 strips
    return (r.integers(0, 256, (n, h, w)), r.integers(0, 256, (n, h // 2, w // 2)), r.integers(0, 256, (n, h // 2, w // 2))), _padded_layout(fmt, h, w)


@pytest.mark.parametrize("case", ["random720", "extremes", "tail", "padded"])
@pytest.mark.parametrize("fmt", FMTS)
def test_op_yuv_to_bgr_equals_oracle(fmt, case):
    (Yp, U, V), lay = _op_case(fmt, case)
    n, h, w = Yp.shape
    buf = Y.pack(fmt, Yp, U, V, lay, fill=201)
    got = lib.op_yuv_to_bgr(buf, fmt, lay, h=h, w=w, n=n)
    exp = Y.planes_to_bgr(Yp, U, V)
    assert got.shape == exp.shape and np.array_equal(got, exp)
    assert np.array_equal(exp, Y.to_bgr(fmt, buf, lay, h, w, n))


# ---- 2. - 4. records of the handle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_handle_records_equal_bgr_under_graph_replay(state_dicts, fmt):
    """batch 8 (graph replay), 11 frames (a partial last step): pageable, pinned padded and device-fed NV12 / I420 give the BGR call's records, and
    the YUV calls replay the graphs the BGR call captured."""
    n = 11
    yuv = _encode(fmt, synth.clip(4, n))
    bgr = Y.to_bgr(fmt, yuv)
    hd = _handle(state_dicts, 8)
    try:
        exp = hd.process(bgr)
        caps = hd.timings().graph_captures
        assert caps > 0
        assert hd.process_yuv(yuv, fmt).tobytes() == exp.tobytes()
        lay = _padded_layout(fmt, 720, 1280)
        packed = Y.pack(fmt, *Y.split(fmt, yuv), lay, fill=255)
        pinned = hd.host_buffer(packed.nbytes)
        try:
            pinned[:] = packed
            assert hd.process_yuv(pinned, fmt, layout=lay, n=n).tobytes() == exp.tobytes()
        finally:
            hd.host_free(pinned)
        for src, l in ((yuv, None), (packed, lay)):
            d = hd.upload(src)
            try:
                assert hd.process_device_yuv(d, n, fmt, layout=l).tobytes() == exp.tobytes()
            finally:
                hd.free(d)
        assert hd.timings().graph_captures == caps
    finally:
        hd.close()


def test_handle_records_equal_bgr_plain_launches(state_dicts):
    n = 60
    yuv = _encode("nv12", synth.clip(6, n, distinct=12))
    bgr = Y.to_bgr("nv12", yuv)
    hd = _handle(state_dicts, 50)
    try:
        assert hd.process_yuv(yuv, "nv12").tobytes() == hd.process(bgr).tobytes()
    finally:
        hd.close()


def test_handle_records_equal_bgr_1080p(state_dicts):
    """1920 x 1080: HRNet's input takes the 2 x 2 area-decimation path of the resize"""
    yuv = _encode("nv12", np.stack([synth.frame(1, 5 * t, 1080, 1920) for t in range(3)]))
    bgr = Y.to_bgr("nv12", yuv)
    hd = _handle(state_dicts, 4, 1080, 1920)
    try:
        assert hd.process_yuv(yuv, "nv12").tobytes() == hd.process(bgr).tobytes()
    finally:
        hd.close()


# ---- 5. the Python API above the handle ---------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("fmt", FMTS)
def test_processor_and_flow_cadence_equal_bgr(state_dicts, fmt):
    from eagle_amd.processor import Processor
    hs, ys = state_dicts
    yuv = _encode(fmt, np.stack([synth.frame(2, 3 * t) for t in range(6)]))
    bgr = Y.to_bgr(fmt, yuv)
    p = Processor(batch=2, hrnet_state_dict=hs, detector_state_dict=ys)
    try:
        assert _same(p.process(yuv[0], pixel_format=fmt), p.process(bgr[0]))
        cad = dict(fps=25, num_homography=1, num_keypoint_detection=5, verbose=False)
        exp = p.model.get_coordinates(bgr, **cad)
        got = p.model.get_coordinates(yuv, pixel_format=fmt, **cad)
        assert sorted(got) == list(range(6)) and _same(got, exp)
    finally:
        p.model.handle.close()


# ---- 6. bad arguments ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_bad_layouts_raise_and_leave_the_handle_usable(state_dicts, fmt):
    n, h, w = 2, 720, 1280
    yuv = _encode(fmt, synth.clip(8, n))
    bgr = Y.to_bgr(fmt, yuv)
    hd = _handle(state_dicts, 2)
    try:
        exp = hd.process(bgr)
        flat = np.zeros(4 << 20, np.uint8)
        with pytest.raises(lib.EagleError, match="even"):
            lib.op_yuv_to_bgr(flat, fmt, None, h=h, w=w - 1, n=1)
        with pytest.raises(lib.EagleError, match="unknown pixel format"):
            hd.process_yuv(yuv, 3)
        with pytest.raises(lib.EagleError, match="y_pitch"):
            hd.process_yuv(flat, fmt, layout={"y_pitch": w - 2}, n=1)
        with pytest.raises(lib.EagleError, match="overlaps"):
            hd.process_yuv(flat, fmt, layout={"c_offset": w * (h - 1)}, n=1)
        with pytest.raises(lib.EagleError, match="frame_stride"):
            hd.process_yuv(flat, fmt, layout={"frame_stride": w * h}, n=2)
        d = hd.upload(yuv)
        try:
            with pytest.raises(lib.EagleError, match="frame_stride"):
                hd.process_device_yuv(d, n, fmt, layout={"frame_stride": w * h})
            with pytest.raises(lib.EagleError, match="unknown pixel format"):
                hd.yuv_to_bgr_device(d, n, 0)
            assert hd.process_device_yuv(d, n, fmt).tobytes() == exp.tobytes()
        finally:
            hd.free(d)
        assert hd.process_yuv(yuv, fmt).tobytes() == exp.tobytes()
    finally:
        hd.close()
