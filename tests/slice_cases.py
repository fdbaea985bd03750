"""Cases and references for the detector's concat-by-slice path (csrc/nets.hip build_yolo / YoloBuilder::c2f): convolutions on TView::slice views, SPPF's
maxpool5 chain, the neck's upsample2 and the mixed detector's split_to_f32 seam (no GPU; tests/test_gpu_slices.py runs them on the GPU through
lib.op_conv2d_sliced / op_maxpool5 / op_upsample2 / op_split_to_f32, tests/test_slice_cases_cpu.py checks the references themselves).

The caller owns whole buffers [n, h, w, cs]; everything outside the slices of a launch holds the quiet NaN SENTINEL (reid_cases.SENTINEL).  A read outside an
input or residual slice then shows as a NaN inside the output slice, a write outside the output slice as a changed value outside it.  fp32 buffers come back
with the sentinel's bits; binary16 and split storage keep a NaN a NaN but not its payload, so there the check is "NaN wherever a NaN was, the stored value
wherever a value was" (unslice with fmt)."""
import numpy as np

from reid_cases import SENTINEL, tensor, weights

FMTS = ("f32", "f16", "f32s")


def sentinel():
    return np.array([SENTINEL], np.uint32).view(np.float32)[0]


def split_value(a):
    """What split storage keeps of a float32 array: hi = rn16(16 v), lo = rn16(16 v - hi) -> (hi + lo) / 16 (the _split_round of test_gpu_ops.py)."""
    s = np.asarray(a, np.float32) * np.float32(16)
    with np.errstate(invalid="ignore"):
        hi = s.astype(np.float16).astype(np.float32)
        lo = (s - hi).astype(np.float16).astype(np.float32)
        return (hi + lo) * np.float32(0.0625)


def stored(a, fmt):
    """the float32 values a buffer holds after the library stored it in format fmt"""
    a = np.asarray(a, np.float32)
    if fmt == "f16":
        with np.errstate(invalid="ignore"):
            return a.astype(np.float16).astype(np.float32)
    return split_value(a) if fmt == "f32s" else a


def buffer(shape):
    """a whole buffer [n, h, w, cs] of sentinels"""
    return np.full(shape, sentinel(), np.float32)


def place(buf, off, dense):
    """dense [n, h, w, c] into channels off .. off + c of buf (in place) -> buf"""
    buf[..., off:off + dense.shape[-1]] = dense
    return buf


def unslice(whole, c, off, fmt="f32", before=None):
    """the slice [.., off:off + c] of a buffer returned whole.  Asserts that nothing outside it changed and that there is no NaN inside.  before: the buffer as it
    was handed in (None: sentinels everywhere outside).  fp32: bit for bit; f16 / f32s: NaN where a NaN was, stored(before) elsewhere."""
    whole = np.ascontiguousarray(whole, np.float32)
    outside = np.ones(whole.shape[-1], bool)
    outside[off:off + c] = False
    was = buffer(whole.shape) if before is None else np.ascontiguousarray(before, np.float32)
    assert was.shape == whole.shape
    if fmt == "f32":
        same = whole.view(np.uint32)[..., outside] == was.view(np.uint32)[..., outside]
    else:
        a, b = whole[..., outside], stored(was, fmt)[..., outside]
        same = (np.isnan(a) & np.isnan(b)) | (a.view(np.uint32) == b.view(np.uint32))
    assert same.all(), f"{(~same).sum()} values outside the output slice were overwritten"
    y = whole[..., off:off + c]
    assert not np.isnan(y).any(), "NaN inside the output slice: the kernel read outside an input slice, or left an element unwritten"
    return y


# ---- float64 / NumPy references ---------------------------------------------------------------------------------------------------------------
def maxpool_ref(x, k):
    """MaxPool2d(k, 1, k // 2) on [n, h, w, c]: padding never wins (-inf).  A maximum is exact in any precision: float64 inside, float32 out."""
    n, h, w, c = x.shape
    p = k // 2
    xp = np.full((n, h + 2 * p, w + 2 * p, c), -np.inf)
    xp[:, p:p + h, p:p + w] = x.astype(np.float64)
    m = np.full(x.shape, -np.inf)
    for dy in range(k):
        for dx in range(k):
            m = np.maximum(m, xp[:, dy:dy + h, dx:dx + w])
    return m.astype(np.float32)


def maxpool5_ref(x):
    return maxpool_ref(x, 5)


def upsample2_ref(x, yh, yw):
    """nearest x2, cropped to yh x yw: y[i, j] = x[i // 2, j // 2]"""
    n, h, w, c = x.shape
    assert yh in (2 * h - 1, 2 * h) and yw in (2 * w - 1, 2 * w)
    return x[:, np.arange(yh) // 2][:, :, np.arange(yw) // 2]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def pool_input(n, h, w, c, fmt):
    """normal values with exact zeros; channel 1 strictly negative everywhere (a pool that pads with 0 is wrong at the border); channel 2 holds the most
    negative finite binary16 number (fp16: -65504; split: the same pair, the value -65504 / 16) on the border ring: the window maximum there is that number"""
    x = tensor([55, n, h, w, c], (n, h, w, c), neg_channel=1)
    low = np.float32(-65504.0) if fmt != "f32s" else np.float32(-65504.0 / 16.0)
    x[..., 2] = low
    if h > 6 and w > 6:
        x[:, 3:-3, 3:-3, 2] = np.float32(-1.5)
    return x


SPLIT_EDGES = np.array([4094.0, -4094.0,                   # |16 v| = 65504: the largest pair (hi = +-65504, lo = 0)
                        4093.75, -4093.75,                 # one binary16 ulp (32 / 16) + lo below it
                        1.0, -0.5, 0.0625, 3.0,            # lo = 0
                        0.0, -0.0,                         # +-0: hi = +-0, lo = +0 -> hi + lo = +0
                        (1.0 + 2.0 ** -20) / 16.0, -(2.0 + 2.0 ** -22) / 16.0, (0.25 + 2.0 ** -24) / 16.0,     # subnormal lo (2^-20, 2^-22, 2^-24: the smallest)
                        2.0 ** -24 / 16.0, 2.0 ** -20 / 16.0,                                                  # subnormal hi, lo = 0
                        0.1, -1.0 / 3.0, 1234.567], np.float32)


def split_input(n, h, w, c):
    """normal values with the edge values scattered over every channel group and pixel position"""
    x = tensor([66, n, h, w, c], (n, h, w, c)) * np.float32(3.0)
    flat = x.reshape(-1)
    idx = np.random.default_rng([67, n, h, w, c]).permutation(flat.size)[:4 * len(SPLIT_EDGES)] if flat.size >= 4 * len(SPLIT_EDGES) else np.arange(flat.size)
    flat[idx] = np.resize(SPLIT_EDGES, len(idx))
    return x


# ---- slice geometries: those the five detector variants produce (yolo_dims: c = 16, 32, 48, 64, 80 in the C2f blocks of n, s, m, l, x) --------------
# c: channels of the input, output and residual slices; x_cs / x_off: the input slice; rx: where a residual inside the INPUT buffer lies; y_cs / y_off: the
# output slice; ry: where a residual inside the OUTPUT buffer lies (C2f: y = cat[(2 + k) c], r1 = cat[(1 + k) c]).  Strides 48, 80, 144, 208 (no power of
# two), offsets 0 (first slice), 16, 48, 80, 128; "last": the slice ends where the pixel ends, so whatever is read past it on the last pixel lies past the
# allocation, and on every earlier pixel it is the next pixel's sentinel.
GEOMS = {
    "c16": dict(c=16, x_cs=48, x_off=16, rx=32, y_cs=48, y_off=32, ry=16),       # C2f of yolov8n with n = 1: y last, r1 its left neighbour; rx last
    "c16first": dict(c=16, x_cs=48, x_off=0, rx=16, y_cs=80, y_off=16, ry=48),   # x first slice
    "c32": dict(c=32, x_cs=80, x_off=48, rx=16, y_cs=80, y_off=48, ry=16),       # x last, y last
    "c48": dict(c=48, x_cs=144, x_off=80, rx=16, y_cs=144, y_off=0, ry=48),      # y first
    "c64": dict(c=64, x_cs=144, x_off=80, rx=16, y_cs=144, y_off=80, ry=16),     # x last, y last
    "c80": dict(c=80, x_cs=208, x_off=48, rx=128, y_cs=208, y_off=48, ry=128),   # rx last, ry last
}
MAPS = [(2, 9, 13), (1, 17, 30), (3, 1, 1), (1, 5, 70)]      # (n, h, w): ragged, one wider than 32 columns (wx = 2, wo > 32), a 1 x 1 map with a batch
KS_STRIDE = [(1, 1), (3, 1), (3, 2)]
MODES = ("in", "out", "both", "c2f", "r_in_x")
# in: sliced input, dense output;  out: dense input, sliced output;  both: both sliced and r1 a slice of a third buffer;
# c2f: input from a dense buffer, r1 and y slices of one buffer (model.N.m.k.cv2);  r_in_x: x and r1 slices of one buffer, y sliced (stride 1: same map size)


def conv_cases():
    """(ks, stride, mode, geometry name, map): every (ks, stride) x mode x geometry, the maps dealt round-robin so that every mode meets every map"""
    out, k = [], 0
    for ks, st in KS_STRIDE:
        for mode in MODES:
            if mode == "r_in_x" and st != 1:
                continue                               # a stride-2 output has another size than its input: no such pair of slices exists
            for g in GEOMS:
                out.append((ks, st, mode, g, MAPS[k % len(MAPS)]))
                k += 1
    return out


def conv_data(ks, st, c_in, c_out, shape, res, seed=0):
    """dense operands of one convolution: x, w, b and `res` residuals; pre = SiLU as every detector layer"""
    n, h, w = shape
    ho, wo = (h + 2 * (ks // 2) - ks) // st + 1, (w + 2 * (ks // 2) - ks) // st + 1
    key = [77, seed, ks, st, c_in, c_out, n, h, w]
    x = tensor(key + [0], (n, h, w, c_in), zeros=0.0)
    wt = weights(key + [1], (ks, ks, c_in, c_out), (2.0 / (c_in * ks * ks)) ** 0.5)
    b = weights(key + [2], (c_out,), 0.1)
    rs = [tensor(key + [3 + i], (n, ho, wo, c_out), zeros=0.0) for i in range(res)]
    return x, wt, b, rs


def conv_operands(mode, G, x, rs, ho, wo, cout):
    """the buffers of one sliced convolution in geometry G (a GEOMS entry) -> dict(x, x_off, y, y_off, r1) for lib.op_conv2d_sliced (r1 as its
    (where, buffer, off) triple; lib.RES_OWN / RES_IN_Y / RES_IN_X = 0 / 1 / 2).  mode "c2f_x": "c2f" with a sliced input as well"""
    n, h, w, cin = x.shape
    sl_x = mode in ("in", "both", "r_in_x", "c2f_x")
    sl_y = mode != "in"
    xb = place(buffer((n, h, w, G["x_cs"])), G["x_off"], x) if sl_x else x.copy()
    yb = buffer((n, ho, wo, G["y_cs"] if sl_y else cout))
    r1 = None
    if mode == "both":
        r1 = (0, place(buffer((n, ho, wo, G["x_cs"])), G["rx"], rs[0]), G["rx"])
    elif mode in ("c2f", "c2f_x"):
        place(yb, G["ry"], rs[0]); r1 = (1, None, G["ry"])
    elif mode == "r_in_x":
        place(xb, G["rx"], rs[0]); r1 = (2, None, G["rx"])
    return dict(x=xb, x_off=G["x_off"] if sl_x else 0, y=yb, y_off=G["y_off"] if sl_y else 0, r1=r1)


def n_res(mode):
    return 0 if mode in ("in", "out") else 1


# Every tiling through the force switches at one geometry: 48 -> 48 channels, 3 x 3 stride 1, x and r1 slices of one buffer, y a slice ("r_in_x" of "c48"),
# two frames of 9 x 13 (row stacking of the exact family needs a batch) and one of 5 x 70 where the tile is 32 wide.
FORCE_F32 = ["3,2,0", "3,1,0", "3,2,3", "3,1,3", "3,2,4", "1,1,4"]                 # EAGLE_F32_FORCE "nt,wx,variant": full / half / quarter tiles, each x EAGLE_F32_STACK 0 / 1
FORCE_F16 = ["48,3,0", "16,3,0", "16,3,2", "48,3,3", "16,3,3", "48,3,4", "16,1,4"]   # EAGLE_CONV_FORCE "kc,nt,variant": variants 0 / 2 / 3 / 4
FORCE_SPLIT = ["16,3,0", "16,1,0", "16,3,3", "16,3,18"]                            # variants 0 / 3 / 18
FORCE_MAPS = [(2, 9, 13), (1, 5, 70)]

# The A-direct and weight-stationary forms (plain epilogue: no pre-activation, ReLU; what HRNet runs, dense): (family, force, stride, cin, cout).
# One case each: x = channels 48 .. 48 + cin of a buffer of 48 + cin (last slice), y = channels 16 .. 16 + cout of a buffer of 16 + 2 cout, r1 the slice
# right of it (last slice of the output buffer), two frames of 9 x 37 (partial tiles in both directions, two tile columns).  Variant 6 runs at 48 and 64
# channels: its 96-channel instance ("96,3,6", listed here until conv_form_cases.assert_form looked) needs more LDS than a workgroup can have and never ran.
AD_FORMS = [("f16", "48,3,6", 1, 48, 48), ("f16", "48,3,7", 1, 48, 48), ("f16", "64,4,6", 1, 64, 64), ("f16", "96,2,7", 1, 96, 32),
            ("f16", "32,12,8", 1, 96, 192), ("f16", "32,6,9", 1, 96, 96), ("f16", "32,12,10", 2, 96, 192), ("f16", "32,6,11", 2, 96, 96),
            ("f32s", "16,12,8", 1, 96, 192), ("f32s", "16,6,9", 1, 96, 96), ("f32s", "16,12,10", 2, 96, 192), ("f32s", "16,6,11", 2, 96, 96),
            ("f32s", "16,3,12", 1, 48, 48), ("f32s", "16,3,13", 1, 48, 48), ("f32s", "16,12,14", 2, 96, 192), ("f32s", "16,6,15", 2, 96, 96),
            ("f32s", "16,3,19", 1, 48, 48), ("f32s", "16,12,21", 1, 96, 192), ("f32s", "16,6,22", 1, 96, 96), ("f32s", "16,12,23", 1, 96, 192),
            ("f32s", "16,6,24", 1, 96, 96)]
AD_MAP = (2, 9, 37)


def ad_geom(cin, cout):
    return dict(c=cout, x_cs=48 + cin, x_off=48, rx=0, y_cs=16 + 2 * cout, y_off=16, ry=16 + cout)


# ---- maxpool5 / upsample2 / split_to_f32 ---------------------------------------------------------------------------------------------------------
POOL_MAPS = [(1, 1), (2, 3), (5, 5), (7, 11), (12, 20)]
POOL_NS = (1, 3)
POOL_CS = (16, 80)
POOL_SLICES = {16: dict(x_cs=48, x_off=16, y_cs=80, y_off=48), 80: dict(x_cs=208, x_off=128, y_cs=144, y_off=16)}     # x last slice (80: 128 + 80 = 208), y inside
UP_MAPS = [(1, 1), (2, 3), (5, 7), (9, 20)]
UP_SLICES = {16: dict(x_cs=48, x_off=32, y_cs=48, y_off=0), 80: dict(x_cs=144, x_off=16, y_cs=208, y_off=0)}          # cat12 / cat15: slice 0 of a wider buffer, from a later slice


def up_sizes(h, w):
    return [(yh, yw) for yh in sorted({2 * h - 1, 2 * h}) for yw in sorted({2 * w - 1, 2 * w})]
