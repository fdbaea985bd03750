"""Constructed clips for the top view (K32): each a few frames with their homographies, and what each is there to force.  A case is a dict: name, frames
uint8 [n, h, w, 3], Hs [n, 9], valid [n], boxes (None or a list of n float32 [k, 4] arrays) and p (topview_ref.params).  Most maps are written as P,
the pitch -> image matrix, with small integer or dyadic entries; H = adj(P) is then exact, and so is G = adj(H) = det(P) P, which lets a case place a
sample exactly on a boundary of the rule.  test_topview_cpu.py checks that each case forces what it is named after; the references are computed once
(reference below) and shared."""
import functools

import numpy as np

import topview_ref as R

F = np.float64


def adj(P):
    P = np.asarray(P, F).reshape(9)
    return np.array([P[a] * P[b] - P[c] * P[d] for a, b, c, d in R.COFACTORS], F)


def rnd(n, h, w, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, (n, h, w, 3), np.uint8)


def scale_map(a, bx=0.0, by=0.0):
    """P: u = a x + bx, v = a (68 - y) + by"""
    return [[a, 0, bx], [0, -a, 68 * a + by], [0, 0, 1]]


def case(name, frames, Ps, p, valid=None, boxes=None, Hs=None):
    frames = np.ascontiguousarray(frames, np.uint8)
    n = len(frames)
    if Hs is None:
        Hs = [adj(P) for P in Ps]
    Hs = np.array([np.asarray(H, F).reshape(9) for H in Hs], F).reshape(n, 9)
    return dict(name=name, frames=frames, Hs=Hs, valid=np.ones(n, np.uint8) if valid is None else np.asarray(valid, np.uint8),
                boxes=boxes, p=p)


# a camera standing on the pitch at (52, 20), 4 m up, looking towards y = 0: u' = 16 (52 - x) + 32 w', v' = 64 + 8 w', w' = 20 - y; integers, det P = -1024
STANDING = [[-16, -32, 1472], [0, -8, 224], [0, -1, 20]]


def pinhole(C, T, f, cx, cy):
    """P of a camera at C looking at T (pitch plane z = 0), focal length f pixels, principal point (cx, cy)"""
    C, T = np.asarray(C, F), np.asarray(T, F)
    fw = (T - C) / np.linalg.norm(T - C)
    r = np.cross(fw, [0, 0, 1.0])
    r /= np.linalg.norm(r)
    d = np.cross(fw, r)
    Rm = np.stack([r, d, fw])
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    return K @ np.stack([Rm[:, 0], Rm[:, 1], -Rm @ C], 1)


def _build():
    C = []
    p20 = R.params(2, 0)
    # the canvas is an exact copy of the frame (the frame has one row and one column more): u = X, v = Y
    for S in (2, 4):
        fr = rnd(1, 68 * S + 1, 105 * S + 1, 10 + S)
        C.append(case(f"exact_copy_S{S}", fr, [scale_map(S)], R.params(S, 0)))
    # a mirrored map (v = S y: the frame upside down), handed over with det H < 0 (adj(P) itself always has det = det(P)^2 > 0)
    C.append(case("mirrored_det_negative", rnd(1, 137, 211, 3), None, p20, Hs=[-adj([[2, 0, 0], [0, 2, 0], [0, 0, 1]])]))
    # half-pixel shifts: one pixel per metre at S = 2 puts every other canvas column and row at fx = 128 / fy = 128
    tie = np.zeros((2, 5, 7, 3), np.uint8)
    tie[0, :, 0::2], tie[0, :, 1::2] = 7, 10                     # 7 | 10: (17 + 1) >> 1 ties along x, both orders
    tie[0, 1::2, 0::2], tie[0, 1::2, 1::2] = 8, 13               # 7 | 8 and 10 | 13 tie along y, 7 + 10 + 8 + 13 = 38 ties at fx = fy = 128
    tie[1] = rnd(1, 5, 7, 4)[0]
    C.append(case("half_pixel_ties", tie, [scale_map(1), scale_map(1)], p20))
    # samples exactly on the last column and row, 1 / 256 before and beyond: u = X / 256 + 3 - 10 / 256, v = Y / 256 + 3 - 7 / 256 on a 4 x 4 frame;
    # and tu exactly 0 and just below: u = X / 512 - 6 / 512, v = Y / 512 - 4 / 512
    e = rnd(2, 4, 4, 5)
    C.append(case("edges", e, [[[1 / 128, 0, 3 - 10 / 256], [0, -1 / 128, 68 / 128 + 3 - 7 / 256], [0, 0, 1]],
                               [[1 / 256, 0, -6 / 512], [0, -1 / 256, 68 / 256 - 4 / 512], [0, 0, 1]]], p20))
    # a 1 x 1 frame: only U = V = 0 is a valid sample (two columns and two rows of the canvas)
    C.append(case("frame_1x1", rnd(1, 1, 1, 6), [[[1 / 256, 0, -10 / 512], [0, -1 / 256, 68 / 256 - 5 / 512], [0, 0, 1]]], p20))
    # odd sizes under a general scale, canvases with and without a margin
    C.append(case("frame_2x2", rnd(2, 2, 2, 7), [scale_map(0.013, 0.2, 0.1), scale_map(0.02, -0.1, 0.0)], R.params(2, 2)))
    C.append(case("frame_4x4", rnd(2, 4, 4, 8), [scale_map(0.031, 0.0, 0.3), scale_map(0.05, -1.0, -0.5)], R.params(2, 2, background=0x123456)))
    C.append(case("frame_5x7_odd_pitch", rnd(3, 5, 7, 9), [scale_map(0.0611), scale_map(0.09, -1.3, 0.2), scale_map(0.2, -7.0, -3.0)], p20))
    C.append(case("frame_17x33", rnd(2, 17, 33, 11), [scale_map(0.3, 0.5, -2.0), scale_map(0.41, -3.0, 0.25)], R.params(4, 6)))
    C.append(case("frame_137x211_S8_M64", rnd(1, 137, 211, 12), [scale_map(2.003, -0.7, 0.4)], R.params(8, 64, markings=1)))
    # a pinhole camera whose footprint is a trapezoid inside the canvas
    C.append(case("pinhole_trapezoid", rnd(2, 48, 64, 13), [pinhole((52.5, -40.0, 30.0), (52.5, 30.0, 0.0), 200.0, 31.5, 23.5),
                                                           pinhole((40.0, -35.0, 25.0), (55.0, 34.0, 0.0), 180.0, 31.5, 23.5)], R.params(2, 2, markings=1)))
    # the camera on the pitch: the canvas rows y > 20 are behind it, w' == 0 exactly on the row y = 20; and H, -H, 3 H give the same bytes
    st = rnd(1, 48, 64, 14)
    H = adj(STANDING)
    C.append(case("behind_camera_and_scaled_H", np.concatenate([st, st, st]), None, R.params(2, 0, first=0, step=1), Hs=[H, -H, 3 * H]))
    # frames without a map, and u' so large that tu is inf
    g = rnd(9, 4, 4, 15)
    good = adj(scale_map(0.04))
    nan_h, inf_h, big_h = good.copy(), good.copy(), good.copy()
    nan_h[4], inf_h[2], big_h[:] = np.nan, np.inf, 1e200
    Hs = [good, [1, 2, 3, 2, 4, 6, 0, 0, 1], nan_h, inf_h, big_h, [1, 0, 0, 0, 1, 0, 0, -1, 3], good, adj([[1e300, 0, 0], [0, 1, 0], [0, 0, 1e-300]]), good]
    C.append(case("no_map", g, None, R.params(2, 0, background=0x0a0b0c), valid=[1, 1, 1, 1, 1, 1, 0, 1, 1], Hs=Hs))
    # markings on, in a colour the picture has too
    red = np.zeros((1, 4, 4, 3), np.uint8)
    red[..., 2] = 255
    C.append(case("markings_in_a_picture_colour", red, [scale_map(0.03)], R.params(2, 2, markings=1, marking_colour=R.RED, background=0x00ff00)))
    # ---- the mosaic ----
    C.append(case("mosaic_0_frames", np.zeros((0, 4, 4, 3), np.uint8), [], R.params(2, 0, background=0x010203, markings=1)))
    C.append(case("mosaic_1_frame_residual_0", rnd(1, 5, 7, 16), [scale_map(0.07)], p20))
    two = np.zeros((2, 4, 4, 3), np.uint8)
    two[0], two[1] = 10, 11                                      # mean 10.5: a tie
    C.append(case("mosaic_2_frames_mean_tie", two, [scale_map(0.04)] * 2, p20))
    # three frames side by side with overlaps, min_count 2: pixels with exactly 2 and with 1 contribution
    C.append(case("mosaic_3_frames_min_count", rnd(3, 4, 4, 17), [scale_map(0.1), scale_map(0.1, -2.0), scale_map(0.1, -4.0)], R.params(2, 0, min_count=2)))
    C.append(case("mosaic_65_frames", rnd(65, 2, 2, 18), [scale_map(0.05, -0.02 * k) for k in range(65)], R.params(2, 0, first=1, step=3)))
    # first and step skip the only frame with a map: an empty mosaic, and a frame with no overlap with it
    C.append(case("mosaic_skips_the_covering_frame", rnd(3, 4, 4, 19), [scale_map(0.04)] * 3, R.params(2, 0, first=0, step=2), valid=[0, 1, 0]))
    # the mosaic is frame 0 alone; frame 1 is frame 0 plus 5
    base = rnd(1, 5, 7, 20, hi=250)
    C.append(case("residual_constant_offset", np.concatenate([base, base + 5]), [scale_map(0.08)] * 2, R.params(2, 0, first=0, step=2)))
    # ---- boxes: u = X / 2, v = Y / 2 on a 6 x 9 frame; the box 2 .. 4 x 1 .. 3 padded by 0.5 has samples on each edge and half a pixel outside ----
    bx = rnd(2, 6, 9, 21)
    C.append(case("boxes_edges_pad", bx, [scale_map(1)] * 2, R.params(2, 0, mask_boxes=1, box_pad=0.5),
                  boxes=[np.array([[2, 1, 4, 3]], np.float32), np.array([[6, 4, 7, 4.5]], np.float32)]))
    C.append(case("boxes_pad_0", bx, [scale_map(1)] * 2, R.params(2, 0, mask_boxes=1), boxes=[np.array([[2, 1, 4, 3]], np.float32), np.zeros((0, 4), np.float32)]))
    r = np.random.default_rng(22)
    many = np.concatenate([r.uniform(0, 7, (300, 1)), r.uniform(0, 4, (300, 1))], 1)
    many = np.concatenate([many, many + r.uniform(0.1, 0.8, (300, 2))], 1).astype(np.float32)
    C.append(case("boxes_300", bx, [scale_map(1)] * 2, R.params(2, 0, mask_boxes=1, box_pad=0.125), boxes=[many, many[:7]]))
    C.append(case("boxes_whole_frame", bx, [scale_map(1)] * 2, R.params(2, 0, mask_boxes=1), boxes=[np.array([[0, 0, 8, 5]], np.float32)] * 2))
    return C


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(warped frames, mosaic, cnt, res_sum, res_cnt, covered) of a case; computed once, shared, not to be written to"""
    c = BY_NAME[name]
    out = R.topview(c["frames"], c["Hs"], c["valid"], c["boxes"], c["p"])
    for a in out:
        a.setflags(write=False)
    return out


def maps(name):
    c = BY_NAME[name]
    n, h, w, _ = c["frames"].shape
    return [R.frame_map(c["Hs"][i], c["valid"][i], h, w) for i in range(n)]


# (a change of the parameters, what the refusal's message must name)
REFUSALS = [(dict(scale=1), "scale 1"), (dict(scale=3), "scale 3"), (dict(scale=34), "scale 34"), (dict(margin=-2), "margin -2"), (dict(margin=3), "margin 3"),
            (dict(margin=66), "margin 66"), (dict(step=0), "step 0"), (dict(first=-1), "first -1"), (dict(min_count=0), "min_count 0"), (dict(box_pad=-1.0), "box_pad -1"),
            (dict(box_pad=float("nan")), "box_pad nan"), (dict(box_pad=float("inf")), "box_pad inf"), (dict(background=0x1000000), "background 0x1000000"),
            (dict(marking_colour=0x1000000), "marking_colour 0x1000000"), (dict(mask_boxes=1), "mask_boxes needs the records")]


def records_none_own_none_own():
    """four records: no H, an own H, no H, another own H"""
    from eagle_amd import lib
    recs = np.zeros(4, lib.RESULT_DTYPE)
    for i, s in ((1, 2.0), (3, 3.0)):
        recs[i]["H_valid"] = 1
        recs[i]["H"] = np.array([s, 0, 0, 0, -s, 68, 0, 0, 1], F).reshape(recs[i]["H"].shape)
    return recs
