"""CPU checks of the 4:2:0 input contract (include/eagle.h, eagle_*_yuv): the oracle's formula (tests/yuv_ref.py), the dense-default layout
arithmetic and the synthetic decoder output of eagle_amd/synth.py.  The GPU side is tests/test_gpu_yuv.py."""
import numpy as np
import pytest

import yuv_ref as Y
from eagle_amd import synth


def _px(fmt, y, u, v):
    """one 2x2 block of luma y with chroma (u, v) -> its BGR pixel (0, 0)"""
    Yp = np.full((1, 2, 2), y, np.int32)
    return Y.planes_to_bgr(Yp, np.full((1, 1, 1), u), np.full((1, 1, 1), v))[0, 0, 0]


def test_anchors_black_and_white():
    assert list(_px(Y.NV12, 16, 128, 128)) == [0, 0, 0]
    assert list(_px(Y.NV12, 235, 128, 128)) == [255, 255, 255]


def test_luma_below_16_clamps_to_black():
    for y in (0, 1, 15, 16):
        assert list(_px(Y.NV12, y, 128, 128)) == [0, 0, 0]
    assert list(_px(Y.NV12, 17, 128, 128)) == [1, 1, 1]       # (1220542 + 2^19) >> 20


def test_chroma_extremes_saturate():
    b, g, r = _px(Y.NV12, 128, 255, 128)         # U = 255: B clips high
    assert b == 255 and r == 130
    b, g, r = _px(Y.NV12, 128, 0, 128)           # U = 0: B clips low
    assert b == 0
    b, g, r = _px(Y.NV12, 128, 128, 255)         # V = 255: R clips high
    assert r == 255 and b == 130
    b, g, r = _px(Y.NV12, 128, 128, 0)
    assert r == 0
    b, g, r = _px(Y.NV12, 235, 255, 255)         # every channel computed in int32 range and saturated, not wrapped
    assert (b, r) == (255, 255) and 0 <= g <= 255
    b, g, r = _px(Y.NV12, 16, 0, 0)
    assert (b, r) == (0, 0) and g == (524288 + 128 * (852492 + 409993)) >> 20 == 154


def test_formula_matches_integer_restatement():
    rng = np.random.default_rng(3)
    yy, uu, vv = rng.integers(0, 256, 500), rng.integers(0, 256, 500), rng.integers(0, 256, 500)
    for y, u, v in zip(yy, uu, vv):
        yt = max(0, int(y) - 16) * 1220542
        exp = [min(255, max(0, (yt + (1 << 19) + c) >> 20)) for c in (2116026 * (int(u) - 128), -852492 * (int(v) - 128) - 409993 * (int(u) - 128),
                                                                     1673527 * (int(v) - 128))]
        assert list(_px(Y.I420, y, u, v)) == exp


def _random_planes(n, h, w, seed=0):
    r = np.random.default_rng(seed)
    return (r.integers(0, 256, (n, h, w)), r.integers(0, 256, (n, h // 2, w // 2)), r.integers(0, 256, (n, h // 2, w // 2)))


def test_nv12_and_i420_of_the_same_planes_decode_identically():
    Yp, U, V = _random_planes(2, 6, 10)
    nv = Y.pack(Y.NV12, Yp, U, V).reshape(2, 9, 10)
    i4 = Y.pack(Y.I420, Yp, U, V).reshape(2, 9, 10)
    assert not np.array_equal(nv, i4)
    a, b = Y.nv12_to_bgr(nv), Y.i420_to_bgr(i4)
    assert a.shape == (2, 6, 10, 3) and np.array_equal(a, b)
    assert np.array_equal(a, Y.planes_to_bgr(Yp, U, V))


def test_one_chroma_sample_per_2x2_block():
    Yp = np.full((1, 4, 4), 120, np.int32)
    U = np.array([[[40, 200], [90, 160]]]); V = np.array([[[220, 30], [128, 70]]])
    bgr = Y.planes_to_bgr(Yp, U, V)[0]
    for by in range(2):
        for bx in range(2):
            blk = bgr[2 * by: 2 * by + 2, 2 * bx: 2 * bx + 2].reshape(4, 3)
            assert (blk == blk[0]).all()                                   # the four pixels share one chroma sample, no interpolation
    assert len({tuple(bgr[2 * by, 2 * bx]) for by in range(2) for bx in range(2)}) == 4


def test_dense_default_layout_arithmetic():
    assert Y.dense_layout(Y.NV12, 720, 1280) == {"frame_stride": 1382400, "y_pitch": 1280, "c_offset": 921600, "c_pitch": 1280, "v_offset": 0}
    assert Y.dense_layout(Y.I420, 720, 1280) == {"frame_stride": 1382400, "y_pitch": 1280, "c_offset": 921600, "c_pitch": 640, "v_offset": 1152000}
    for fmt in (Y.NV12, Y.I420):
        for h, w in ((720, 1280), (1080, 1920), (18, 34), (2, 2)):
            d = Y.dense_layout(fmt, h, w)
            assert d["frame_stride"] == h * w * 3 // 2
            assert Y.resolve(fmt, h, w) == d == Y.resolve(fmt, h, w, {k: 0 for k in d})
    # a padded decoder surface: chroma after h + 16 rows of the padded pitch, frame_stride defaults to the end of the last plane
    p = Y.resolve(Y.I420, 720, 1280, {"y_pitch": 1344, "c_offset": 1344 * 736, "c_pitch": 704})
    assert p["v_offset"] == 1344 * 736 + 704 * 360 and p["frame_stride"] == p["v_offset"] + 704 * 360


def test_library_span_of_a_layout():
    from eagle_amd import lib
    for fmt in ("nv12", "i420"):
        assert lib.yuv_span(fmt, 720, 1280, None, 3) == 3 * 1382400
        assert lib.yuv_span(fmt, 720, 1280, None, 0) == 0
    lay = {"y_pitch": 1344, "c_offset": 1344 * 736, "c_pitch": 1344}
    assert lib.yuv_span("nv12", 720, 1280, lay, 2) == (1344 * 736 + 1344 * 360) + 1344 * 736 + 1344 * 359 + 1280


def test_layout_packing_roundtrip():
    Yp, U, V = _random_planes(3, 8, 12, seed=5)
    for fmt, lay in ((Y.NV12, {"y_pitch": 16, "c_offset": 16 * 12, "c_pitch": 20, "frame_stride": 400}),
                     (Y.I420, {"y_pitch": 14, "c_offset": 14 * 9, "c_pitch": 8, "v_offset": 14 * 9 + 40, "frame_stride": 300})):
        buf = Y.pack(fmt, Yp, U, V, lay, fill=77)
        got = Y.planes(fmt, buf, 3, 8, 12, lay)
        assert all(np.array_equal(a, b) for a, b in zip(got, (Yp, U, V)))
        assert np.array_equal(Y.to_bgr(fmt, buf, lay, 8, 12, 3), Y.planes_to_bgr(Yp, U, V))


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_synth_decoder_output_shapes(fmt):
    f = np.stack([synth.frame(0, 0, 72, 128), synth.noise_frame(1, 72, 128)])
    enc = synth.bgr_to_nv12 if fmt == "nv12" else synth.bgr_to_i420
    out = enc(f)
    assert out.shape == (2, 108, 128) and out.dtype == np.uint8
    assert enc(f[0]).shape == (1, 108, 128)
    dec = Y.to_bgr(fmt, out)
    assert dec.shape == f.shape
    # a BT.601 round trip: chroma is shared per 2x2 block, so only a loose closeness holds (the contract is checked against the decoded frames)
    assert np.abs(dec[0].astype(int) - f[0].astype(int)).mean() < 12
    Yp, U, V = Y.split(fmt, out)
    assert Yp.min() >= 16 and Yp.max() <= 235 and U.min() >= 16 and U.max() <= 240
    other = synth.bgr_to_i420 if fmt == "nv12" else synth.bgr_to_nv12
    assert all(np.array_equal(a, b) for a, b in zip(Y.split("i420" if fmt == "nv12" else "nv12", other(f)), (Yp, U, V)))


def test_synth_rejects_odd_sizes():
    with pytest.raises(ValueError):
        synth.bgr_to_nv12(np.zeros((1, 5, 8, 3), np.uint8))


@pytest.mark.parametrize("fmt,h,w,lay,msg", [
    ("nv12", 18, 33, None, "even"),
    ("nv12", 17, 34, None, "even"),
    (7, 18, 34, None, "unknown pixel format"),
    ("i420", 18, 34, {"c_pitch": -4}, "negative"),
    ("nv12", 18, 34, {"y_pitch": 32}, "y_pitch"),
    ("i420", 18, 34, {"c_pitch": 16}, "c_pitch"),
    ("nv12", 18, 34, {"c_offset": 34 * 17}, "overlaps"),
    ("i420", 18, 34, {"v_offset": 34 * 18 + 17 * 8}, "overlaps"),
    ("nv12", 18, 34, {"frame_stride": 34 * 27 - 1}, "frame_stride"),
])
def test_library_rejects_bad_layouts_before_touching_the_gpu(fmt, h, w, lay, msg):
    """The one argument check of the four eagle_*yuv* entries runs before any HIP call (here through the operator entry, no GPU needed)."""
    from eagle_amd import lib
    with pytest.raises(lib.EagleError, match=msg):
        lib.op_yuv_to_bgr(np.zeros(1 << 16, np.uint8), fmt, lay, h=h, w=w, n=2)
