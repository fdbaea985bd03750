"""-m gpu: every OSNet (ReID) kernel of csrc/reid.hip alone (eagle_op_reid_*), at the shapes of tests/reid_cases.py, against
 - a float32 restatement bit for bit (np.array_equal) where the arithmetic has no fmaf and a fixed order: crop, maxpool3s2, avgpool2, the all-ones
   integer cases of conv7 and dw3, the gated sum given the kernel's own gates;
 - the float64 reference with the DERIVED forward-error bound gamma_k * S of its fmaf chain (reid_cases' docstring: k = 148 conv7, 10 dw3, two-stage
   bounds for the gate and the head; no tuned tolerance), and
 - additionally, since oracle.prims.fmaf restates the chains exactly (C fmaf in the kernel's order), the kernel-order float32 restatement bit for bit:
   conv7, dw3, the gates g (through oracle.prims.sigmoid) and the head.  Bit equality is the stronger statement; the bound stays asserted next to it,
   against the independent float64 reference, and its observed slack is printed per operator.
Dense outputs come back without a sentinel; in the slice cases (cs = c + 16, off = 8 on inputs, cs = c + 4, off = 4 on outputs) everything outside a slice is
a NaN sentinel: a read outside an input slice shows as NaN, a write outside an output slice as an overwritten sentinel (reid_cases.unslice).
The grid-stride tails (more than 65535 * 256 items per launch) are not reachable at the network's 64 crops per pass and are deliberately not tested."""
import itertools

import numpy as np
import pytest

import reid_cases as R
from eagle_amd import lib

pytestmark = pytest.mark.gpu


def _ratio(got, ref, bound):
    d = np.abs(got.astype(np.float64) - ref)
    ok = bound > 0
    assert (d[~ok] == 0).all()
    return float((d[ok] / bound[ok]).max()) if ok.any() else 0.0


def _report(op, worst):
    print(f"{op}: largest |got - ref| / bound = {worst:.4f}")
    assert worst <= 1.0, (op, worst)


def _slice_kw(c_in, c_out):
    kw = {}
    if c_in is not None:
        kw.update(x_cs=c_in + R.SLICE_IN[0], x_off=R.SLICE_IN[1])
    if c_out is not None:
        kw.update(y_cs=c_out + R.SLICE_OUT[0], y_off=R.SLICE_OUT[1])
    return kw


def test_crop_is_bit_exact_and_rejected_rectangles_give_zeros():
    from oracle import reid
    for (fh, fw), (oh, ow) in itertools.product(((720, 1280), (97, 61)), ((256, 128), (8, 4))):
        frames = R.frames(fh, fw)
        ok, bad = R.crop_cases(fh, fw, oh, ow)
        rects = [r for _, r in ok + bad]
        step = 3 if oh == 256 else len(rects)               # the production output size three crops at a time
        got = np.concatenate([lib.op_reid_crop(frames, rects[i:i + step], (oh, ow)) for i in range(0, len(rects), step)])
        assert got.shape == (len(rects), oh, ow, 4) and (got[..., 3] == 0).all()
        for k, (name, (f, *rect)) in enumerate(ok):
            ref = reid.prepare_crop(frames[f], rect) if (oh, ow) == (256, 128) else R.crop_f32(frames[f], rect, oh, ow)
            assert np.array_equal(got[k, :, :, :3], ref), (fh, fw, oh, ow, name)
        assert (got[len(ok):] == 0).all(), "a rejected rectangle must give an all-zero crop"
    frames = R.frames(97, 61)
    ok, bad = R.crop_cases(97, 61, 8, 4)
    whole = lib.op_reid_crop(frames, [r for _, r in ok + bad], (8, 4), **_slice_kw(None, 4))
    assert np.array_equal(R.unslice(whole, 4, R.SLICE_OUT[1]), lib.op_reid_crop(frames, [r for _, r in ok + bad], (8, 4)))


def test_conv7_within_its_bound_and_bit_exact():
    worst = 0.0
    for (h, w), n in itertools.product(R.CONV7_SIZES, R.NS):
        x, wt, b = R.conv7_case(n, h, w)
        got = lib.op_reid_conv7(x, wt, b)
        ref, bound = R.conv7_ref(x, wt, b)
        assert got.shape == ref.shape
        worst = max(worst, _ratio(got, ref, bound))
        assert (np.abs(got - ref) <= bound).all(), (h, w, n)
        assert np.array_equal(got, R.conv7_f32(x, wt, b)), (h, w, n)
        x, wt, b = R.conv7_case(n, h, w, ones=True)
        assert np.array_equal(lib.op_reid_conv7(x, wt, b), np.broadcast_to(3.0 * R.tap_counts(h, w, 7, 2, 3)[None, :, :, None], got.shape)), (h, w, n)
    x, wt, b = R.conv7_case(3, 9, 6)
    y = R.unslice(lib.op_reid_conv7(x, wt, b, **_slice_kw(4, 16)), 16, R.SLICE_OUT[1])
    assert np.array_equal(y, lib.op_reid_conv7(x, wt, b)) and np.array_equal(y, R.conv7_f32(x, wt, b))
    _report("conv7", worst)


def test_maxpool3s2_is_bit_exact():
    for (h, w), c, n in itertools.product(R.MAPS, R.CHANNELS, R.NS):
        x = R.pool_case(n, h, w, c)
        got = lib.op_reid_maxpool3s2(x)
        assert np.array_equal(got, R.maxpool3s2_ref(x)), (h, w, c, n)
        assert (got[..., 1] < 0).all()                      # the strictly negative channel: no padding value took part
    x = R.pool_case(3, 5, 7, 32)
    assert np.array_equal(R.unslice(lib.op_reid_maxpool3s2(x, **_slice_kw(32, 32)), 32, R.SLICE_OUT[1]), R.maxpool3s2_ref(x))


def test_avgpool2_is_bit_exact():
    """maps without a 2 x 2 window ((1, 1), (1, 7), (7, 1)) have no output pixel: AvgPool2d refuses them and so does the entry (no launch)"""
    for (h, w), c, n in itertools.product(R.MAPS, R.CHANNELS, R.NS):
        x = R.pool_case(n, h, w, c)
        if h < 2 or w < 2:
            with pytest.raises(lib.EagleError):
                lib.op_reid_avgpool2(x)
            continue
        got = lib.op_reid_avgpool2(x)
        assert got.shape == (n, h // 2, w // 2, c) and np.array_equal(got, R.avgpool2_ref(x)), (h, w, c, n)
    x = R.pool_case(3, 5, 7, 32)                            # odd map, input in a slice: the last row and column (and the NaN around the slice) are not read
    assert np.array_equal(R.unslice(lib.op_reid_avgpool2(x, **_slice_kw(32, 32)), 32, R.SLICE_OUT[1]), R.avgpool2_ref(x))


def test_dw3_within_its_bound_and_bit_exact():
    worst = 0.0
    for (h, w), c, n in itertools.product(R.MAPS, R.CHANNELS, R.NS):
        x, wt, b = R.dw3_case(n, h, w, c)
        got = lib.op_reid_dw3(x, wt, b)
        ref, bound = R.dw3_ref(x, wt, b)
        worst = max(worst, _ratio(got, ref, bound))
        assert (np.abs(got - ref) <= bound).all(), (h, w, c, n)
        assert np.array_equal(got, R.dw3_f32(x, wt, b)), (h, w, c, n)
        assert (got[..., R.CHANNELS[c]:] == 0).all()        # padding channels (zero weights and bias) are written as zeros
        x, wt, b = R.dw3_case(n, h, w, c, ones=True)
        assert np.array_equal(lib.op_reid_dw3(x, wt, b), np.broadcast_to(R.tap_counts(h, w, 3, 1, 1)[None, :, :, None].astype(np.float32), x.shape)), (h, w, c, n)
    x, wt, b = R.dw3_case(3, 5, 7, 32)
    assert np.array_equal(R.unslice(lib.op_reid_dw3(x, wt, b, **_slice_kw(32, 32)), 32, R.SLICE_OUT[1]), R.dw3_f32(x, wt, b))
    _report("dw3", worst)


def _check_gate(streams, w1, b1, w2, b2, what, **kw):
    c, c_real = streams[0].shape[-1], w1.shape[1]
    g, whole = lib.op_reid_gate(streams, w1, b1, w2, b2, **kw)
    y = R.unslice(whole, c, kw.get("y_off", 0))
    _, et, g64 = R.gate_ref(streams, w1, b1, w2, b2)
    bound = R.gate_g_bound(et, g64)
    assert (np.abs(g - g64) <= bound).all(), what
    assert np.array_equal(g, R.gate_g_f32(streams, w1, b1, w2, b2)), what
    assert (g[..., c_real:] == 0).all() and (y[..., c_real:] == 0).all(), what          # padding gates and padding channels of the sum are exactly 0
    assert np.array_equal(y, R.gated_sum_f32(streams, g)), what
    return g, _ratio(g, g64, bound)


def test_gate_within_its_bound_and_bit_exact():
    worst = 0.0
    for (c, c_real, r), (h, w), n in itertools.product(R.GATE_CFGS, R.GATE_MAPS, R.NS):
        g, ratio = _check_gate(*R.gate_case(n, h, w, c, c_real, r), (c, c_real, r, h, w, n))
        worst = max(worst, ratio)
        if n == 3:
            assert not np.array_equal(g[0], g[1]) and not np.array_equal(g[:, 0], g[:, 3])      # crops and streams are told apart
    # padding channels of the inputs at 1e6 (dense layout): no real-channel gate moves, the padding gates stay exactly 0
    clean = R.gate_case(3, 16, 8, 32, 24, 1)
    dirty = R.gate_case(3, 16, 8, 32, 24, 1, pad_value=1e6)
    g0, _ = lib.op_reid_gate(*clean)
    g1, y1 = lib.op_reid_gate(*dirty)
    assert np.array_equal(g0, g1) and (g1[..., 24:] == 0).all() and (y1[..., 24:] == 0).all()
    _check_gate(*R.gate_case(3, 16, 8, 32, 24, 1), "slices", **_slice_kw(32, 32))
    _report("gate g", worst)


def test_head_within_its_bound_and_bit_exact():
    worst = 0.0
    for c, (h, w), dim, n in itertools.product(R.HEAD_CS, R.HEAD_MAPS, R.HEAD_DIMS, R.NS):
        x, wt, b = R.head_case(n, h, w, c, dim)
        got = lib.op_reid_head(x, wt, b)
        ref, bound = R.head_ref(x, wt, b)
        assert got.shape == (n, dim) and not np.isnan(got).any()
        worst = max(worst, _ratio(got, ref, bound))
        assert (np.abs(got - ref) <= bound).all(), (c, h, w, dim, n)
        assert np.array_equal(got, R.head_f32(x, wt, b)), (c, h, w, dim, n)
    x, wt, b = R.head_case(3, 3, 5, 16, 300)
    assert np.array_equal(lib.op_reid_head(x, wt, b, **_slice_kw(16, None)), R.head_f32(x, wt, b))
    _report("head", worst)
