"""Annotated output, the part that needs no GPU: the numpy contract (tests/annot_ref.py) pinned by anchors and properties that hold whatever
OpenCV does, the library's host-side overlay builder against it on hand-built records, the Y4M writer and the ABI surface."""
import math
import os
import re

import numpy as np
import pytest

import annot_ref as A
import yuv_ref as Y
from eagle_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- colour path ---------------------------------------------------------------------------------------------------------
def test_colour_spec_anchors():
    assert (sum(A.CY), sum(A.CU), sum(A.CV)) == (900726, 1, 1)
    v = np.arange(256, dtype=np.int64)
    grey = np.repeat(v[None, None, :, None], 3, -1).repeat(2, 1).astype(np.uint8)          # [1, 2, 256, 3]
    Yp, U, V = A.bgr_to_planes(grey)
    assert np.array_equal(Yp[0, 0], (900726 * v + 17301504) >> 20) and (U == 128).all() and (V == 128).all()
    assert (Yp[0, 0, 0], Yp[0, 0, 255]) == (16, 235)
    for fmt in (A.NV12, A.I420):
        assert A.bgr_to_yuv(fmt, np.zeros((1, 2, 2, 3), np.uint8)).ravel().tolist() == [16] * 4 + [128, 128]
        assert A.bgr_to_yuv(fmt, np.full((1, 2, 2, 3), 255, np.uint8)).ravel().tolist() == [235] * 4 + [128, 128]


def test_nv12_and_i420_carry_the_same_samples_from_the_even_pixel():
    r = np.random.default_rng(3)
    bgr = r.integers(0, 256, (2, 6, 8, 3), dtype=np.uint8)
    n12, i42 = A.bgr_to_yuv(A.NV12, bgr), A.bgr_to_yuv(A.I420, bgr)
    p12, p42 = Y.split(Y.NV12, n12), Y.split(Y.I420, i42)
    assert all(np.array_equal(a, b) for a, b in zip(p12, p42))
    # chroma is the sample of the even-row, even-column pixel alone: changing the other three pixels of every block changes no U / V
    other = bgr.copy()
    other[:, 1::2] = 255 - other[:, 1::2]; other[:, :, 1::2] = 255 - other[:, :, 1::2]
    q = A.bgr_to_planes(other)
    assert np.array_equal(q[1], p12[1]) and np.array_equal(q[2], p12[2])
    # all planes stay inside the byte range without saturation, at the colour cube's corners too
    corners = np.array([[b, g, rr] for b in (0, 255) for g in (0, 255) for rr in (0, 255)], np.uint8).reshape(1, 2, 4, 3).repeat(2, 1).repeat(2, 2)
    for pl in A.bgr_to_planes(corners):
        assert pl.min() >= 0 and pl.max() <= 255


def test_round_trip_through_the_input_side_inverse():
    """BGR -> 4:2:0 (annot_ref) -> BGR (yuv_ref), both numpy specs, frames constant over each 2 x 2 block so that the one chroma sample is the
    block's.  Measured on the CPU when this was written: maximum absolute error 1 level on the grey ramp, 2 levels on random colours (2 is
    also the maximum over all 2^24 colours).  Asserted: the measured maximum plus one level.  A property of two integer formulas, not of
    the kernel."""
    rt = lambda f: Y.planes_to_bgr(*A.bgr_to_planes(f)).astype(np.int64)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, None, :, None], 3, -1).repeat(2, 1).repeat(2, 2)
    e_ramp = int(np.abs(rt(ramp) - ramp).max())
    r = np.random.default_rng(5)
    rnd = r.integers(0, 256, (4, 90, 160, 3), dtype=np.uint8).repeat(2, 1).repeat(2, 2)
    e_rnd = int(np.abs(rt(rnd) - rnd).max())
    print("round trip: grey ramp", e_ramp, "random", e_rnd)
    assert e_ramp <= 1 + 1 and e_rnd <= 2 + 1


# ---- ARC ---------------------------------------------------------------------------------------------------------------
def _arc_masks():
    Yg, Xg = np.mgrid[-30:31, -50:51]
    return Xg, Yg, A.arc_outline(Xg, Yg), A.covers(A.arc(0, 0, A.WHITE), Xg, Yg)


def _dist_to_ellipse(x, y):
    """float64, this test only: distance of (x, y) to the ellipse x = 35 cos t, y = 18 sin t by dense sampling + local refinement"""
    t = np.linspace(0, 2 * math.pi, 20001)
    d = np.hypot(35 * np.cos(t) - x, 18 * np.sin(t) - y)
    k = int(d.argmin())
    tt = np.linspace(t[max(k - 1, 0)], t[min(k + 1, len(t) - 1)], 2001)
    return float(np.hypot(35 * np.cos(tt) - x, 18 * np.sin(tt) - y).min())


def test_arc_counts_and_named_pixels():
    Xg, Yg, outline, drawn = _arc_masks()
    assert (int(outline.sum()), int(drawn.sum())) == (156, 112)
    at = lambda x, y: bool(drawn[y + 30, x + 50])
    assert at(-35, 0) and at(35, 0) and at(0, 18) and not at(0, -18)
    assert not (drawn & ~outline).any()


def test_arc_lies_on_the_ellipse():
    Xg, Yg, _, drawn = _arc_masks()
    worst = max(_dist_to_ellipse(x, y) for x, y in zip(Xg[drawn], Yg[drawn]))
    print("arc: largest distance to the true ellipse", worst)              # 0.9925 for the rule of annot_ref
    assert worst <= 1.0


def test_arc_gap_is_the_angles_235_to_315():
    Xg, Yg, outline, drawn = _arc_masks()
    t = 1.0
    ang = np.degrees(np.arctan2(Yg / 18.0, Xg / 35.0))                       # parametric angle, y down, in (-180, 180]
    ang = np.where(ang < -85, ang + 360, ang)                                # cut in the middle of the gap -> [-85, 275): the arc -45 .. 235 is contiguous
    assert ((ang[drawn] >= -45 - t) & (ang[drawn] <= 235 + t)).all()
    must = outline & (ang >= -45 + t) & (ang <= 235 - t)
    assert not (must & ~drawn).any()
    # the rule of annot_ref needs no tolerance at all
    assert ((ang[drawn] >= -45) & (ang[drawn] <= 235)).all() and not (outline & (ang >= -45) & (ang <= 235) & ~drawn).any()


def test_arc_is_8_connected_between_its_two_ends():
    _, _, _, drawn = _arc_masks()
    pts = {(int(x), int(y)) for y, x in zip(*np.nonzero(drawn))}
    nb = lambda p: [(p[0] + dx, p[1] + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx or dy) and (p[0] + dx, p[1] + dy) in pts]
    seen, todo = set(), [next(iter(pts))]
    while todo:
        p = todo.pop()
        if p not in seen:
            seen.add(p); todo += nb(p)
    assert seen == pts                                                      # one component
    _, _, outline, _ = _arc_masks()
    assert int(outline.sum()) > len(pts)                                    # and open: the closed outline has more pixels


# ---- DISC, TRI, LABEL ------------------------------------------------------------------------------------------------------
def test_disc_r6_is_the_113_lattice_points():
    Yg, Xg = np.mgrid[-10:11, -10:11]
    m = A.covers(A.disc(0, 0, 6, A.BLACK), Xg, Yg)
    assert int(m.sum()) == 113 == sum(1 for x in range(-6, 7) for y in range(-6, 7) if x * x + y * y <= 36)
    assert A.bbox(A.disc(0, 0, 6, A.BLACK)) == (-6, -6, 6, 6)


def test_ball_marker_covers_its_vertices_and_stays_in_its_box():
    f = A.draw(np.zeros((80, 80, 3), np.uint8), [A.ball_marker(40, 60)])
    on = f[..., 1] == 255
    for x, y in ((40, 40), (35, 30), (45, 30)):
        assert on[y, x]
    ys, xs = np.nonzero(on)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (35, 45, 30, 40)
    assert on[30, 35:46].all() and not on[41].any() and not on[29].any()
    # orientation does not matter, and a degenerate triangle stays inside its box
    g = A.draw(np.zeros((80, 80, 3), np.uint8), [A.tri(45, 30, 35, 30, 40, 40, A.GREEN)])
    assert np.array_equal(f, g)


def test_label_glyphs():
    def text(ident):
        f = A.draw(np.zeros((20, 80, 3), np.uint8), [A.label(3, 16, ident, A.WHITE)])
        return f[..., 0] == 255
    glyphs = [text(d) for d in range(10)]
    for d, g in enumerate(glyphs):
        ys, xs = np.nonzero(g)
        assert len(xs) and xs.min() >= 0 and xs.max() <= 9 and ys.min() >= 3 and ys.max() <= 16, d      # 10 x 14, bottom-left pixel at (x - 3, y) = (0, 16)
        blocks = g[3:17, 0:10]
        assert np.array_equal(blocks, blocks[::2, ::2].repeat(2, 0).repeat(2, 1)), d                      # every font pixel is a 2 x 2 block
    for i in range(10):
        for j in range(i):
            assert not np.array_equal(glyphs[i], glyphs[j]), (i, j)
    t10, t01 = text(10), text(1)
    assert not np.array_equal(t10, text(1)) and not np.array_equal(text(10), text(100))
    assert np.array_equal(t10[:, :10], glyphs[1][:, :10]) and np.array_equal(t10[:, 12:22], glyphs[0][:, :10]) and not t10[:, 10:12].any()
    assert not np.array_equal(text(10)[:, :22], np.concatenate([glyphs[0][:, :12], glyphs[1][:, :10]], 1))          # "10" is not "01"
    assert t01.any() and not text(-1).any() and not text(100000).any()
    assert np.array_equal(text(99999)[:, 48:58], glyphs[9][:, :10])


def test_the_library_font_is_the_spec_font():
    txt = open(os.path.join(ROOT, "eagle_amd", "csrc", "annot_font.h")).read()
    rows = [tuple(int(v, 16) for v in re.findall(r"0x[0-9A-Fa-f]{2}", g)) for g in re.findall(r"\{([^{}]*)\}", txt)]
    assert tuple(rows) == A.FONT


# ---- painter's order and clipping ---------------------------------------------------------------------------------------------
def test_painters_order_and_clipping():
    base = np.full((60, 100, 3), 77, np.uint8)
    a, d = A.arc(50, 30, A.RED), A.disc(85, 30, 6, A.BLACK)                   # (85, 30) is the arc's right end
    both = A.draw(base, [a, d])
    only_a, only_d = A.draw(base, [a]), A.draw(base, [d])
    overlap = (only_a != base).any(-1) & (only_d != base).any(-1)
    assert overlap.any() and (both[overlap] == A.BLACK).all()
    assert (A.draw(base, [d, a])[overlap] == A.RED).all()
    untouched = ~((only_a != base).any(-1) | (only_d != base).any(-1))
    assert (both[untouched] == 77).all()
    # primitives centred outside the frame draw their in-frame part only and never wrap
    for prim in (A.disc(-2, -3, 6, A.BLACK), A.disc(101, 30, 6, A.BLACK), A.arc(-20, 65, A.RED), A.label(95, 5, 88, A.WHITE), A.ball_marker(2, 25),
                 A.disc(-500, 30, 6, A.BLACK), A.tri(-50, -50, 20, -50, -50, 20, A.GREEN)):
        big = np.full((60 + 200, 100 + 1200, 3), 77, np.uint8)
        moved = range(6) if prim[0] == A.TRI else range(2)                 # the coordinates among a0 .. a5: x at even positions, y at odd ones
        shifted = (prim[0],) + tuple(v + ((600, 100)[k % 2] if k in moved else 0) for k, v in enumerate(prim[1:7])) + (prim[7],)
        exp = A.draw(big, [shifted])[100:160, 600:700]
        assert np.array_equal(A.draw(base, [prim]), exp), prim
    assert np.array_equal(A.draw(base, [A.disc(-500, 30, 6, A.BLACK)]), base)


# ---- what a record's picture is: the spec and the library's builder, on hand-built records --------------------------------------------
def _rec(dets=(), kps=(), H_valid=False):
    r = np.zeros(1, lib.RESULT_DTYPE)[0]
    r["n_det"], r["n_kp"], r["H_valid"] = len(dets), len(kps), int(H_valid)
    for i, (cls, ident, fx, fy, reported) in enumerate(dets):
        d = r["det"][i]
        d["cls"], d["id"], d["foot_x"], d["foot_y"], d["reported"], d["conf"] = cls, ident, fx, fy, reported, 0.9 - 0.01 * i
    for i, (lab, x, y, on_plane, inlier) in enumerate(kps):
        k = r["kp"][i]
        k["label"], k["x"], k["y"], k["on_plane"], k["inlier"] = lab, x, y, on_plane, inlier
    return r


def _lib_overlay(rec, mapping):
    return [(int(p["kind"]), *map(int, p["a"]), (int(p["b"]), int(p["g"]), int(p["r"]))) for p in lib.overlay_from_record(rec, mapping)]


OVERLAY_CASES = {
    "unreported": (_rec([(0, 4, 100, 200, 0), (0, 5, 300, 400, 1)]), {4: 0, 5: 1}, [A.arc(300, 400, A.BLUE), A.label(300, 400, 5, A.BLUE)]),
    "referee_and_staff": (_rec([(3, -1, 100, 200, 1), (4, -1, 50, 60, 1), (0, 1, 10, 20, 1)]), {1: 0}, [A.arc(10, 20, A.RED), A.label(10, 20, 1, A.RED)]),
    "goalkeeper_needs_no_mapping": (_rec([(1, 7, 640, 360, 1)]), {}, [A.arc(640, 360, A.GREEN), A.label(640, 360, 7, A.GREEN)]),
    "player_missing_from_mapping": (_rec([(0, 2, 10, 10, 1), (0, 3, 20, 20, 1)]), {3: 0}, [A.arc(20, 20, A.RED), A.label(20, 20, 3, A.RED)]),
    "no_mapping_neutral": (_rec([(0, 2, 10, 10, 1), (1, 3, 20, 20, 1)]), None,
                           [A.arc(10, 10, A.WHITE), A.label(10, 10, 2, A.WHITE), A.arc(20, 20, A.GREEN), A.label(20, 20, 3, A.GREEN)]),
    "two_balls_first_wins_and_follows_persons": (_rec([(2, 0, 500, 300, 1), (0, 9, 40, 50, 1), (2, 1, 700, 100, 1)]), {9: 1},
                                                 [A.arc(40, 50, A.BLUE), A.label(40, 50, 9, A.BLUE), A.ball_marker(500, 300)]),
    "unreported_ball_skipped": (_rec([(2, 0, 500, 300, 0), (2, 1, 700, 100, 1)]), None, [A.ball_marker(700, 100)]),
    "H_valid_inliers_only": (_rec([(0, 1, 5, 6, 1)], [(3, 10, 11, 1, 1), (4, 20, 21, 1, 0), (56, 30, 31, 0, 1), (8, 40, 41, 1, 1)], True), {1: 0},
                             [A.arc(5, 6, A.RED), A.label(5, 6, 1, A.RED), A.disc(10, 11, 6, A.BLACK), A.disc(40, 41, 6, A.BLACK)]),
    "no_H_every_keypoint": (_rec([], [(3, 10, 11, 1, 0), (4, 20, 21, 0, 0)], False), None, [A.disc(10, 11, 6, A.BLACK), A.disc(20, 21, 6, A.BLACK)]),
    "empty": (_rec(), {1: 0}, []),
}


@pytest.mark.parametrize("case", sorted(OVERLAY_CASES))
def test_overlay_from_record_spec_and_library(case):
    rec, mapping, exp = OVERLAY_CASES[case]
    assert A.overlay_from_record(rec, mapping) == exp
    assert _lib_overlay(rec, mapping) == exp            # eagle_overlay_from_record: host code of the library, no GPU involved


def test_overlay_matches_the_reference_dict_keypoints():
    from eagle_amd import records
    rec = OVERLAY_CASES["H_valid_inliers_only"][0]
    kp = records.to_reference_dict(rec)["Keypoints"]
    discs = [p for p in A.overlay_from_record(rec, None) if p[0] == A.DISC]
    assert [(p[1], p[2]) for p in discs] == [(int(v[0]), int(v[1])) for v in kp.values()]
    assert lib.MAX_PRIMS == A.MAX_PRIMS == 2 * lib.MAX_DET + lib.MAX_KP + 1
    full = _rec([(0, i, 10 + i, 20, 1) for i in range(lib.MAX_DET)], [(i % 57, i, i, 0, 0) for i in range(lib.MAX_KP)])
    assert len(_lib_overlay(full, None)) == len(A.overlay_from_record(full, None)) == 2 * lib.MAX_DET + 57


# ---- Y4M -----------------------------------------------------------------------------------------------------------------
def test_write_y4m_parses_back(tmp_path):
    from eagle_amd.annotate import write_y4m
    r = np.random.default_rng(2)
    n, h, w = 3, 6, 8
    frames = r.integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)
    path = write_y4m(str(tmp_path / "a.y4m"), frames, 25)
    blob = open(path, "rb").read()
    header, rest = blob.split(b"\n", 1)
    assert header == b"YUV4MPEG2 W8 H6 F25:1 Ip A1:1 C420jpeg"
    assert len(blob) == len(header) + 1 + n * (6 + 3 * h * w // 2)
    fsz = 3 * h * w // 2
    for k in range(n):
        chunk = rest[k * (6 + fsz): (k + 1) * (6 + fsz)]
        assert chunk[:6] == b"FRAME\n" and np.array_equal(np.frombuffer(chunk[6:], np.uint8).reshape(h * 3 // 2, w), frames[k])
    with pytest.raises(ValueError):
        write_y4m(str(tmp_path / "b.y4m"), np.zeros((1, 7, 8), np.uint8), 25)


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_header_and_exports_carry_the_new_entries():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "eagle.h")).read()
    L = lib.load()
    for s in ("eagle_annotate_device_frames", "eagle_annotate_frames", "eagle_overlay_from_record", "eagle_op_annotate"):
        assert re.search(r"^int\s+%s\s*\(" % s, hdr, re.M) and s in lib.EXPORTS and hasattr(L, s), s
    assert re.search(r"#define\s+EAGLE_PIX_BGR\s+0\b", hdr) and lib.OUT_FORMATS == {"bgr": 0, "nv12": 1, "i420": 2}
    for name, v in (("ARC", lib.PRIM_ARC), ("LABEL", lib.PRIM_LABEL), ("DISC", lib.PRIM_DISC), ("TRI", lib.PRIM_TRI)):
        assert re.search(r"#define\s+EAGLE_PRIM_%s\s+%d\b" % (name, v), hdr)
    assert (A.ARC, A.LABEL, A.DISC, A.TRI) == (lib.PRIM_ARC, lib.PRIM_LABEL, lib.PRIM_DISC, lib.PRIM_TRI)
    assert lib.PRIM_DTYPE.itemsize == 32 and C.sizeof(lib.EagleYuvLayout) == 40
    # existing structs keep their sizes
    assert lib.abi_sizes()[1:] == [lib.RESULT_DTYPE.itemsize, lib.DET_DTYPE.itemsize, lib.KP_DTYPE.itemsize]
