"""Constructed inputs for the ground layer (K34): each a few frames with their homographies and shape lists, and what each is there to force.  A case
is a dict: name, frames uint8 [n, h, w, 3], Hs [n, 9], valid [n], shapes (n lists of ground_ref shapes), key, formats.  The maps have small integer
or dyadic entries, so that a band's edge can be put exactly on a sub-sample's q.  test_ground_cpu.py checks that each case forces what it is named
after; the references are computed once (reference below) and shared.

SHIFT    px = u / 8 + 10, py = v / 8 + 5: qx = 128 X + 128 dx + 10240, qy = 128 Y + 128 dy + 5120 exactly, the sub-samples of a pixel lie at
         128 dx = -48, 16, 48, -16 and 128 dy = -16, -48, 16, 48.
HORIZON  x' = 8 (u - 132), y' = 200, w' = v - 10: the horizon crosses the picture between rows 9 and 10 (no sub-sample lies on it), the rows just
         below it map beyond 1024 m."""
import functools

import numpy as np

import annot_ref as A
import ground_ref as R

F = np.float64
ALL, BGR = ("bgr", "nv12", "i420"), ("bgr",)
FMT = {"bgr": A.BGR, "nv12": A.NV12, "i420": A.I420}
SHIFT = [1 / 8, 0, 10, 0, 1 / 8, 5, 0, 0, 1]
HORIZON = [8, 0, -8 * 132, 0, 0, 200, 0, 1, -10]
RED, BLUE, WHITE, YELLOW = 0xFF0000, 0x0000FF, 0xFFFFFF, 0xFFFF00   # B | G << 8 | R << 16
TILE_W, TILE_H = 256, 16                                             # csrc/pix_out.h AN_TW, AN_TH


def qx(X, dx=0.0):
    return int(128 * X + 128 * dx + 10240)


def qy(Y, dy=0.0):
    return int(128 * Y + 128 * dy + 5120)


def rnd(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), np.uint8)


def green(n, h, w, seed):
    """random frames whose pixels are mostly grass under the default key"""
    f = np.random.default_rng(seed).integers(0, 64, (n, h, w, 3), np.uint8)
    f[..., 1] += 100
    f[:, ::3, ::5] = 200                                         # white lines: not grass
    return f


def case(name, frames, Hs, shapes, valid=None, key=None, formats=ALL):
    frames = np.ascontiguousarray(frames, np.uint8)
    n = len(frames)
    assert len(shapes) == n and len(Hs) == n
    return dict(name=name, frames=frames, Hs=np.array([np.asarray(H, F).reshape(9) for H in Hs], F).reshape(n, 9),
                valid=np.ones(n, np.uint8) if valid is None else np.asarray(valid, np.uint8), shapes=shapes, key=dict(key or R.DEFAULT_KEY), formats=formats)


def pinhole_h(C, T, f, cx, cy):
    """H (image -> pitch) of a camera at C looking at T, focal length f pixels, principal point (cx, cy)"""
    C, T = np.asarray(C, F), np.asarray(T, F)
    fw = (T - C) / np.linalg.norm(T - C)
    r = np.cross(fw, [0, 0, 1.0])
    r /= np.linalg.norm(r)
    Rm = np.stack([r, np.cross(fw, r), fw])
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    P = K @ np.stack([Rm[:, 0], Rm[:, 1], -Rm @ C], 1)
    return np.linalg.inv(P).reshape(9)


def _build():
    C = []
    line = R.band(qx(100), qx(102), -R.ARG_MAX, R.ARG_MAX, RED, 208)
    zone = R.band(qx(102), qx(240), qy(2), qy(30), BLUE, 48, keyed=True)
    disc = R.ring(qx(40), qy(17), 0, 700, YELLOW, 256)
    hoop = R.ring(qx(200), qy(9), 400, 900, WHITE, 128)
    # ---- 264 x 34: two tiles across, three down ----
    C.append(case("shift_264x34", green(2, 34, 264, 1), [SHIFT, SHIFT], [[zone, line, disc, hoop], [hoop]]))
    hz = [R.band(-20 * 1024, 20 * 1024, 10 * 1024, 40 * 1024, RED, 160), R.ring(0, 20 * 1024, 5 * 1024, 8 * 1024, WHITE, 256),
          R.band(-R.ARG_MAX, R.ARG_MAX, 500 * 1024, R.ARG_MAX, BLUE, 256)]              # the last one: the rows near the horizon, up to 1024 m
    f = green(1, 34, 264, 2)
    C.append(case("horizon_264x34", f, [HORIZON], [hz]))
    C.append(case("horizon_times_minus_3", f, [[-3 * t for t in HORIZON]], [hz]))
    g = rnd(5, 34, 264, 3)
    nan_h, inf_h = list(SHIFT), list(SHIFT)
    nan_h[1], inf_h[5] = np.nan, np.inf
    C.append(case("no_map", g, [SHIFT, nan_h, [1, 0, 0, 0, 1, 0, 0, 1, -33], inf_h, SHIFT], [[line, disc]] * 5, valid=[0, 1, 1, 1, 1]))
    # edges on a sub-sample's q, half-open on both sides: rows 0 .. 7 give c = 3 at X = 5 (x0 on the second sub-sample from the left) and c = 2 at X = 9
    # (x1 on the third); rows 8 .. 15 give c = 1 at X = 20 (x1 on the second); the same in y further right
    e = [R.band(qx(5, -0.125), qx(9, 0.125), qy(0, -0.5), qy(8, -0.5), RED, 256), R.band(qx(12), qx(20, -0.125), qy(8, -0.5), qy(16, -0.5), BLUE, 256),
         R.band(qx(30, -0.5), qx(40, -0.5), qy(20, -0.125), qy(25, 0.125), WHITE, 64), R.band(qx(50, -0.5), qx(60, -0.5), qy(3), qy(12, -0.125), YELLOW, 100)]
    C.append(case("band_edges_on_q", rnd(1, 34, 264, 4), [SHIFT], [e]))
    C.append(case("alpha_0_and_256", rnd(2, 34, 264, 5), [SHIFT] * 2, [[R.band(qx(3), qx(200), qy(1), qy(30), RED, 0), R.ring(qx(100), qy(16), 0, 1500, WHITE, 0)],
                                                                    [R.band(qx(3), qx(200), qy(1), qy(30), RED, 256), R.ring(qx(100), qy(16), 0, 1500, WHITE, 256)]]))
    o1, o2 = R.band(qx(10), qx(150), qy(4), qy(20), RED, 160), R.ring(qx(140), qy(16), 0, 2000, BLUE, 200)
    two = rnd(1, 34, 264, 6)
    C.append(case("overlap_both_orders", np.concatenate([two, two]), [SHIFT] * 2, [[o1, o2], [o2, o1]]))
    many = [R.band(qx(8 * k), qx(8 * k + 12), qy(k), qy(k + 14), (k * 0x0F1E2D) & 0xFFFFFF, 16 * k + 16, keyed=k % 3 == 0) if k % 2 else
            R.ring(qx(16 * k + 5), qy(2 * k), 100 * k, 100 * k + 300, (k * 0x123457) & 0xFFFFFF, 256 - 10 * k) for k in range(16)]
    C.append(case("shapes_16_then_0", green(2, 34, 264, 7), [SHIFT] * 2, [many, []]))
    # a band that reaches tile (0, 0) of the picture in one sub-sample only: the third of pixel (255, 15), whose q is the band's x0 and y0
    C.append(case("one_corner_sub_sample", rnd(1, 34, 264, 8), [SHIFT], [[R.band(qx(255, 0.375), R.ARG_MAX, qy(15, 0.125), R.ARG_MAX, RED, 256)]]))
    # ---- the grass key: g = 47 | 48 with a lead far above the threshold, and g = 48 with a lead of 15 | 16; every other pixel is grass ----
    k = np.zeros((1, 18, 38, 3), np.uint8)
    k[..., 1] = 120
    k[0, :, 0::4], k[0, :, 1::4], k[0, :, 2::4], k[0, :, 3::4] = (0, 47, 0), (0, 48, 0), (33, 48, 10), (10, 48, 32)
    k[0, 9:] = k[0, 9:, ::-1]
    kz = [R.band(qx(1), qx(30), qy(1), qy(16), RED, 256, keyed=True), R.ring(qx(20), qy(9), 0, 1200, WHITE, 128, keyed=True), R.band(qx(33), qx(36), qy(0), qy(18), BLUE, 256)]
    C.append(case("keyed_thresholds_38x18", k, [SHIFT], [kz]))
    C.append(case("keyed_other_key_38x18", rnd(2, 18, 38, 9), [SHIFT] * 2, [kz, kz[:2]], key=dict(key_min=100, key_lead=0)))
    # ---- tail strips and odd sizes ----
    C.append(case("tails_38x18", green(3, 18, 38, 10), [SHIFT, HORIZON, SHIFT], [[zone, R.band(qx(30), qx(37, 0.125), qy(-1), qy(17, 0.375), RED, 208)], hz, []]))
    C.append(case("odd_37x19", rnd(2, 19, 37, 11), [SHIFT, [1 / 4, 0, 0, 0, 1 / 4, 0, 0, 0, 1]], [[R.band(qx(30), qx(40), qy(10), qy(40), RED, 200), R.ring(qx(36), qy(18), 0, 300, WHITE, 256)],
                                                                                         [R.ring(4 * 1024, 2 * 1024, 1024, 3 * 1024, BLUE, 256)]], formats=BGR))
    C.append(case("frame_1x1", rnd(2, 1, 1, 12), [SHIFT] * 2, [[R.band(qx(0, -0.125), qx(0, 0.375), qy(0, -0.5), qy(0, 0.5), RED, 256)], []], formats=BGR))
    C.append(case("frame_8x2", rnd(1, 2, 8, 13), [SHIFT], [[R.band(qx(2), qx(6, 0.125), qy(0), qy(1, 0.375), BLUE, 128), R.ring(qx(7), qy(1), 0, 100, WHITE, 256)]]))
    # ---- one frame of the size the stage is made for: a camera in the stand, the offside picture's shapes ----
    Hp = pinhole_h((52.5, -45.0, 28.0), (52.5, 28.0, 0.0), 1500.0, 639.5, 359.5)
    big = [R.band(60 * 1024, 107520, 0, 69632, BLUE, 48, keyed=True), R.band(60 * 1024 - 128, 60 * 1024 + 128, 0, 69632, RED, 208),
           R.ring(60 * 1024, 30 * 1024, 614, 922, WHITE, 256, keyed=True), R.ring(64 * 1024, 20 * 1024, 614, 922, YELLOW, 256, keyed=True)]
    C.append(case("pinhole_1280x720", green(1, 720, 1280, 14), [Hp], [big]))
    return C


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the window of the large case that the scalar formulation walks (rows, columns): the line, the zone and a ring cross it
SCALAR_WINDOW = {"pinhole_1280x720": (slice(352, 368), slice(500, 900))}
PADDED = [("tails_38x18", "bgr", {"y_pitch": 3 * 38 + 5, "frame_stride": (3 * 38 + 5) * 18 + 11}),
          ("tails_38x18", "nv12", {"y_pitch": 38 + 10, "c_offset": 48 * 18 + 32, "c_pitch": 38 + 6, "frame_stride": 48 * 18 + 32 + 44 * 9 + 9}),
          ("shift_264x34", "i420", {"y_pitch": 264 + 3, "c_offset": 267 * 34 + 1, "c_pitch": 132 + 2, "v_offset": 267 * 34 + 1 + 134 * 17 + 5,
                                    "frame_stride": 267 * 34 + 1 + 2 * 134 * 17 + 5 + 7})]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(pictures uint8 [n, h, w, 3], covered uint32 [n]) of a case; computed once, shared, not to be written to"""
    c = BY_NAME[name]
    out = R.frames_bgr(c["frames"], c["Hs"], c["valid"], c["shapes"], c["key"])
    for a in out:
        a.setflags(write=False)
    return out


def dense(name, fmt):
    """the reference pictures of a case in an output format, in the numpy convention"""
    pics, _ = reference(name)
    n, h, w, _ = pics.shape
    buf = A.annotate(pics, [[]] * n, FMT[fmt])
    return buf.reshape(n, h, w, 3) if fmt == "bgr" else buf.reshape(n, h * 3 // 2, w)


def library_shapes(c):
    """the shape lists of a case as the library takes them: (lib.GROUND_SHAPE_DTYPE [off[n]], off int32 [n + 1])"""
    from eagle_amd import lib
    mk = lambda s: (lib.ground_band if s["kind"] == R.BAND else lib.ground_ring)(*s["a"][:4], s["colour"], s["alpha"], bool(s["flags"] & R.KEYED))
    return lib.ground_shape_lists([[mk(s) for s in x] for x in c["shapes"]])


# (a change of one shape's record, what the refusal's message must name)
SHAPE_REFUSALS = [(dict(kind=2), "kind 2"), (dict(flags=2), "flags 0x2"), (dict(alpha=-1), "alpha -1"), (dict(alpha=257), "alpha 257"), (dict(colour=0x1000000), "colour 0x1000000"),
                  (dict(a=(5, 5, 0, 9, 0, 0)), "empty"), (dict(a=(0, 9, 7, 7, 0, 0)), "empty"), (dict(a=(0, (1 << 21) + 1, 0, 9, 0, 0)), "beyond"),
                  (dict(a=(0, 9, -(1 << 21) - 1, 9, 0, 0)), "beyond"), (dict(kind=1, a=(0, 0, 5, 5, 0, 0)), "radii 5, 5"), (dict(kind=1, a=(0, 0, -1, 5, 0, 0)), "radii -1, 5"),
                  (dict(kind=1, a=(0, 0, 0, (1 << 20) + 1, 0, 0)), "radii"), (dict(kind=1, a=((1 << 21) + 1, 0, 0, 5, 0, 0)), "centre"), (dict(a=(0, 9, 0, 9, 1, 0)), "reserved"),
                  (dict(reserved=(0, 1)), "reserved")]
PARAM_REFUSALS = [(dict(key_min=-1), "key_min -1"), (dict(key_min=256), "key_min 256"), (dict(key_lead=-1), "key_lead -1"), (dict(key_lead=256), "key_lead 256"),
                  (dict(no_cull=2), "no_cull 2"), (dict(reserved=1), "reserved")]
