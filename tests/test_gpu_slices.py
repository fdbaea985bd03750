"""-m gpu: the detector's concat-by-slice path one launch at a time (csrc/nets.hip build_yolo / YoloBuilder::c2f; lib.op_conv2d_sliced, op_maxpool5,
op_upsample2, op_split_to_f32) at the geometries of tests/slice_cases.py.  The test owns whole buffers: everything outside the slices of a launch is a NaN
sentinel, so a read outside an input or residual slice shows as a NaN in the output slice and a write outside the output slice as a changed value.

Convolutions on slice views assert
 (a) slice_cases.unslice: nothing outside the output slice changed, no NaN inside it;
 (b) BIT equality with lib.op_conv2d on the same dense values under the same force switches.  Derived, not measured: a view changes addresses only; the
     kernel instance conv_choose picks (it sees the slice's channel counts, as for the dense tensor) and the summation order are the same;
 (c) the bounds of tests/test_gpu_ops.py against oracle.prims.conv2d, unchanged: bit-exact (f32), F16_TOL (f16), F32S_TOL (f32s).
maxpool5, upsample2 and split_to_f32 are exact: bit equality with the NumPy references on the values the buffer stores.

No r_in_x case exists for stride 2 (the residual has the output's size, the input buffer the input's)."""
import functools

import numpy as np
import pytest

import conv_form_cases as F
import slice_cases as S
from eagle_amd import lib
from test_gpu_ops import F16_TOL, F32S_TOL

pytestmark = pytest.mark.gpu

PREC = {"f32": lib.PREC_F32, "f16": lib.PREC_F16, "f32s": lib.PREC_F32S}
SILU = 2


@functools.lru_cache(maxsize=None)
def _dense(fmt, ks, st, cin, cout, shape, res, pre, post, force, stack):
    """(dense operands, lib.op_conv2d's result, the oracle's) of one convolution, shared by the slice modes and geometries that compute it; force / stack: the
    switches in the environment while this runs (part of the key only)"""
    from oracle import prims as P
    x, wt, b, rs = S.conv_data(ks, st, cin, cout, shape, res)
    r1 = rs[0] if rs else None
    got = lib.op_conv2d(x, wt, b, st, pre, r1, None, post, PREC[fmt])
    q = P.round_f16 if fmt == "f16" else (lambda a: a)
    ref = P.conv2d(q(x), q(wt), b, stride=st, pre=pre, r1=None if r1 is None else q(r1), r2=None, post=post, f16_out=fmt == "f16")
    for a in (x, wt, b, got, ref, *rs):
        a.setflags(write=False)
    return (x, wt, b, rs), got, ref


def _check_oracle(fmt, got, ref):
    if fmt == "f32":
        assert np.array_equal(ref, got), f"fp32 conv not bit-exact: max|d|={np.abs(ref - got).max()}"
    else:
        err = np.abs(ref - got).max() / max(np.abs(ref).max(), 1e-6)
        assert err < (F16_TOL if fmt == "f16" else F32S_TOL), f"{fmt} conv error {err}"


def _forced(monkeypatch, fmt, force, ks, st, cin, cout, shape, pre, post, stack=None):
    """the force switches for the dense and the sliced call of one case (both see the same channel counts, one residual), and the proof that the form they
    name is what conv_choose gives: a string that does not apply is ignored without a word"""
    F.set_force(monkeypatch, fmt, force, stack)
    F.assert_form(monkeypatch, fmt, force, ks, st, cin, cout, F.out_size(shape[1], shape[2], ks, st)[1], pre == 0 and post <= 1, False)


def _sliced_conv(fmt, ks, st, mode, G, shape, cin, cout, pre, post, force=None, stack=None):
    n, h, w = shape
    ho, wo = (h + 2 * (ks // 2) - ks) // st + 1, (w + 2 * (ks // 2) - ks) // st + 1
    res = 1 if mode == "c2f_x" else S.n_res(mode)
    (x, wt, b, rs), dense, ref = _dense(fmt, ks, st, cin, cout, shape, res, pre, post, force, stack)
    op = S.conv_operands(mode, G, x, rs, ho, wo, cout)
    whole = lib.op_conv2d_sliced(op["x"], op["x_off"], wt, b, op["y"], op["y_off"], st, pre, op["r1"], None, post, PREC[fmt])
    got = S.unslice(whole, cout, op["y_off"], fmt, before=op["y"])                                  # (a)
    assert np.array_equal(got.view(np.uint32), dense.view(np.uint32)), \
        f"the sliced result differs from the dense one: max|d|={np.abs(got - dense).max()} in {(got != dense).sum()} values"      # (b)
    _check_oracle(fmt, got, ref)                                                                   # (c)
    return got


@pytest.mark.parametrize("ks,st,mode,g,shape", S.conv_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("fmt", S.FMTS)
def test_conv_on_slices(fmt, ks, st, mode, g, shape, monkeypatch):
    for k in ("EAGLE_CONV_FORCE", "EAGLE_F32_FORCE", "EAGLE_F32_STACK"):
        monkeypatch.delenv(k, raising=False)
    G = S.GEOMS[g]
    _sliced_conv(fmt, ks, st, mode, G, shape, G["c"], G["c"], SILU, 0)


@pytest.mark.parametrize("shape", S.FORCE_MAPS, ids=str)
@pytest.mark.parametrize("stack", ["1", "0"])
@pytest.mark.parametrize("force", S.FORCE_F32)
def test_conv_f32_every_tiling_on_slices(force, stack, shape, monkeypatch):
    _forced(monkeypatch, "f32", force, 3, 1, 48, 48, shape, SILU, 0, stack)
    _sliced_conv("f32", 3, 1, "r_in_x", S.GEOMS["c48"], shape, 48, 48, SILU, 0, force, stack)


@pytest.mark.parametrize("shape", S.FORCE_MAPS, ids=str)
@pytest.mark.parametrize("fmt,force", [("f16", f) for f in S.FORCE_F16] + [("f32s", f) for f in S.FORCE_SPLIT])
def test_conv_f16_and_split_every_tiling_on_slices(fmt, force, shape, monkeypatch):
    _forced(monkeypatch, fmt, force, 3, 1, 48, 48, shape, SILU, 0)
    _sliced_conv(fmt, 3, 1, "r_in_x", S.GEOMS["c48"], shape, 48, 48, SILU, 0, force)


@pytest.mark.parametrize("fmt,force,st,cin,cout", S.AD_FORMS)
def test_conv_a_direct_and_weight_stationary_forms_on_slices(fmt, force, st, cin, cout, monkeypatch):
    """The plain-epilogue forms (HRNet's, which runs them dense): sliced input, output and residual, the residual in the output buffer.  ConvLaunch takes any
    TView, so these forms honour slices like the generic ones: (a) - (c) as above."""
    _forced(monkeypatch, fmt, force, 3, st, cin, cout, S.AD_MAP, 0, 1)
    _sliced_conv(fmt, 3, st, "c2f_x", S.ad_geom(cin, cout), S.AD_MAP, cin, cout, 0, 1, force)


def test_conv_entry_refuses_bad_slices():
    x, wt, b, rs = S.conv_data(3, 1, 16, 16, (1, 4, 5), 1)
    xb, yb = S.place(S.buffer((1, 4, 5, 48)), 16, x), S.place(S.buffer((1, 4, 5, 48)), 16, rs[0])
    ok = lib.op_conv2d_sliced(xb, 16, wt, b, yb, 32, 1, SILU, (lib.RES_IN_Y, None, 16), None, 0, lib.PREC_F32)
    S.unslice(ok, 16, 32, before=yb)
    bad = [dict(x_off=40), dict(x_off=18), dict(y_off=40), dict(y_off=-16), dict(r1=(lib.RES_IN_Y, None, 24)), dict(r1=(lib.RES_IN_Y, None, 40)), dict(r1=(7, None, 0)),
           dict(r1=(lib.RES_IN_X, None, 16), stride=2), dict(x=S.buffer((1, 4, 5, 42)))]
    for kw in bad:
        a = dict(x=xb, x_off=16, y=yb, y_off=32, stride=1, r1=(lib.RES_IN_Y, None, 16)); a.update(kw)
        y = a["y"] if a["stride"] == 1 else S.buffer((1, 2, 3, 48))
        with pytest.raises(lib.EagleError, match=r"\(-?\d+\)"):
            lib.op_conv2d_sliced(a["x"], a["x_off"], wt, b, y, a["y_off"], a["stride"], SILU, a["r1"], None, 0, lib.PREC_F32)
    with pytest.raises(lib.EagleError):                       # 8-channel granularity of the 2-byte families: offset 20 is fine for fp32 only
        lib.op_conv2d_sliced(S.place(S.buffer((1, 4, 5, 48)), 20, x), 20, wt, b, yb, 32, 1, SILU, None, None, 0, lib.PREC_F16)


# ---- maxpool5 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.POOL_CS)
@pytest.mark.parametrize("n", S.POOL_NS)
@pytest.mark.parametrize("h,w", S.POOL_MAPS)
@pytest.mark.parametrize("fmt", S.FMTS)
def test_maxpool5_on_slices_is_exact(fmt, h, w, n, c):
    x = S.pool_input(n, h, w, c, fmt)
    ref = S.maxpool5_ref(S.stored(x, fmt))
    assert (ref[..., 1] < 0).all() and np.isfinite(ref).all()
    g = S.POOL_SLICES[c]
    yb = S.buffer((n, h, w, g["y_cs"]))
    whole = lib.op_maxpool5(S.place(S.buffer((n, h, w, g["x_cs"])), g["x_off"], x), c, g["x_off"], yb, g["y_off"], PREC[fmt])
    assert np.array_equal(S.unslice(whole, c, g["y_off"], fmt).view(np.uint32), ref.view(np.uint32))
    dense = lib.op_maxpool5(x, c, 0, S.buffer((n, h, w, c)), 0, PREC[fmt])
    assert np.array_equal(dense.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("c", S.POOL_CS)
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (3, 7, 11), (1, 12, 20)])
@pytest.mark.parametrize("fmt", S.FMTS)
def test_sppf_chain_in_one_buffer(fmt, n, h, w, c):
    """s0 -> s1 -> s2 -> s3 inside one 4-slice buffer, three launches: the slices are the 5 / 9 / 13 windows of s0, s0 stays, nothing else exists to be touched"""
    x = S.pool_input(n, h, w, c, fmt)
    buf = S.place(S.buffer((n, h, w, 4 * c)), 0, x)
    for k in range(3):
        before = buf
        buf = lib.op_maxpool5(buf, c, k * c, None, (k + 1) * c, PREC[fmt])
        S.unslice(buf, c, (k + 1) * c, fmt, before=before)
    xs = S.stored(x, fmt)
    for k, win in enumerate((1, 5, 9, 13)):
        assert np.array_equal(buf[..., k * c:(k + 1) * c].view(np.uint32), S.maxpool_ref(xs, win).view(np.uint32)), f"slice {k}: window {win}"


def test_maxpool5_entry_refuses_bad_slices():
    x = S.buffer((1, 3, 3, 48))
    for kw in (dict(c=12, precision=lib.PREC_F16), dict(x_off=36), dict(y=None, y_off=24), dict(y_off=4, precision=lib.PREC_F32S), dict(c=0)):
        a = dict(c=16, x_off=16, y=S.buffer((1, 3, 3, 48)), y_off=32, precision=lib.PREC_F32); a.update(kw)
        with pytest.raises(lib.EagleError):
            lib.op_maxpool5(x, a["c"], a["x_off"], a["y"], a["y_off"], a["precision"])


# ---- upsample2 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.POOL_CS)
@pytest.mark.parametrize("h,w", S.UP_MAPS)
@pytest.mark.parametrize("fmt", S.FMTS)
def test_upsample2_into_a_slice_is_exact(fmt, h, w, c):
    n = 2
    x = S.tensor([8, h, w, c], (n, h, w, c))
    g = S.UP_SLICES[c]
    xb = S.place(S.buffer((n, h, w, g["x_cs"])), g["x_off"], x)
    for yh, yw in S.up_sizes(h, w):
        ref = S.upsample2_ref(S.stored(x, fmt), yh, yw)
        whole = lib.op_upsample2(xb, c, g["x_off"], S.buffer((n, yh, yw, g["y_cs"])), g["y_off"], (yh, yw), PREC[fmt])
        assert np.array_equal(S.unslice(whole, c, g["y_off"], fmt).view(np.uint32), ref.view(np.uint32)), (yh, yw)
    for bad in ((2 * h + 1, 2 * w), (2 * h, 2 * w - 2), (h, w) if h > 1 else (3, 1)):
        with pytest.raises(lib.EagleError):
            lib.op_upsample2(xb, c, g["x_off"], S.buffer((n,) + bad + (g["y_cs"],)), g["y_off"], bad, PREC[fmt])


@pytest.mark.parametrize("fmt", S.FMTS)
def test_upsample2_one_pixel_inside_one_buffer(fmt):
    x = S.tensor([9], (3, 1, 1, 16))
    buf = S.place(S.buffer((3, 1, 1, 48)), 32, x)
    out = lib.op_upsample2(buf, 16, 32, None, 0, (1, 1), PREC[fmt])
    assert np.array_equal(S.unslice(out, 16, 0, fmt, before=buf), S.stored(x, fmt))


# ---- split_to_f32 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (2, 9, 13), (1, 17, 30)])
@pytest.mark.parametrize("c,x_cs,x_off,y_cs,y_off", [(16, 16, 0, 16, 0), (16, 48, 32, 80, 16), (80, 208, 128, 144, 0), (48, 144, 16, 208, 80), (8, 24, 8, 20, 12)])
def test_split_to_f32_is_split_value_bit_for_bit(n, h, w, c, x_cs, x_off, y_cs, y_off):
    x = S.split_input(n, h, w, c)
    ref = S.split_value(x)
    whole = lib.op_split_to_f32(S.place(S.buffer((n, h, w, x_cs)), x_off, x), c, x_off, S.buffer((n, h, w, y_cs)), y_off)
    got = S.unslice(whole, c, y_off)                          # the output buffer is fp32: the sentinel's bits come back
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{(got.view(np.uint32) != ref.view(np.uint32)).sum()} values differ"
    if n * h * w * c >= 4 * len(S.SPLIT_EDGES):
        assert np.isin(S.split_value(S.SPLIT_EDGES), got).all(), "every edge value is among the inputs"
    with pytest.raises(lib.EagleError):
        lib.op_split_to_f32(S.buffer((n, h, w, x_cs + 8)), c, x_cs + 8 - c + 4, S.buffer((n, h, w, y_cs)), y_off)       # x_off no multiple of 8
