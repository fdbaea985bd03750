"""numpy restatement of the library's annotated-output contract (include/eagle.h, eagle_annotate_* / eagle_op_annotate; csrc/annotate.hip):
what is drawn on a frame, pixel by pixel, and how the drawn frame becomes NV12 / I420.  It is the single written definition of every output
byte; the kernel equals it byte for byte, so everything here is integer arithmetic.

PARITY UNPINNED, OWN SPEC.  The overlay follows the reference's main.py:43-81 in intent (a foot ellipse with a gap and the id per player in the
team colour, a triangle above the ball, a disc per pitch key-point), but the rasterisation is this project's own, not OpenCV's: cv2 cannot be
imported where this was written, its Hershey font data is not available, and pixel parity with cv2.ellipse / cv2.putText is worth nothing for
a picture whose purpose is to be looked at.

An overlay is an ordered list of primitives (kind, a0 .. a5, (b, g, r)).  A pixel takes the colour of the LAST primitive of the list that
covers it (painter's order, as sequential cv2 calls give); pixels no primitive covers keep the frame's bytes; primitives are clipped to the
frame.  Coordinates are image pixels (x right, y down), |coordinate| <= COORD_MAX, 0 <= radius <= RADIUS_MAX.

    ARC   (cx, cy)            main.py:72  cv2.ellipse(frame, (x, y), (35, 18), 0, -45, 235, color, 1)
          a = 35, b = 18, F(dx, dy) = b^2 dx^2 + a^2 dy^2 - a^2 b^2.  Outline: F <= 0 and one of the four edge neighbours has F > 0 (the
          one-pixel, 8-connected inner boundary).  Removed: the gap of parametric angles strictly between 235 and 315 degrees (y down: the TOP
          of the ellipse, not symmetric), decided on p = (b dx, a dy) with two integer directions d1 = (-7, -10) (235.008 degrees) and
          d2 = (1, -1) (315 degrees): in the gap iff cross(d1, p) > 0 and cross(p, d2) > 0.  112 of the 156 outline pixels remain.
    LABEL (x, y, id)          main.py:73  cv2.putText(frame, str(id), (x - 3, y), FONT_HERSHEY_SIMPLEX, 0.7, color, 2)
          the decimal digits of id (0 .. 99999; any other id draws nothing) in the 5 x 7 bitmap font FONT, every font pixel a 2 x 2 block:
          10 x 14 glyphs, 2 pixels between glyphs, the text's bottom-left pixel at (x - 3, y) (rows y - 13 .. y).
    DISC  (cx, cy, r)         main.py:77  cv2.circle(frame, (x, y), 6, (0, 0, 0), -1): filled, dx^2 + dy^2 <= r^2
    TRI   (x0, y0, x1, y1, x2, y2)   main.py:58  cv2.drawContours(..., -1): filled by integer edge functions, oriented so that the doubled area
          is >= 0; covered iff all three edge functions are >= 0 (edges inclusive: a marker, not a mesh)

overlay_from_record is what the library draws for one EagleFrameResult (main.py's content taken from the raw record, not from the pandas data
frame, which does not exist here).

BGR -> 4:2:0 is the inverse of tests/yuv_ref.py: OpenCV's integer BT.601 limited-range path of cv2.cvtColor(bgr, COLOR_BGR2YUV_I420)
(modules/imgproc/src/color_yuv.simd.hpp), 20-bit fixed point:
    Y = ( 269484 R + 528482 G + 102760 B + (16  << 20) + (1 << 19)) >> 20
    U = (-155188 R - 305135 G + 460324 B + (128 << 20) + (1 << 19)) >> 20
    V = ( 460324 R - 385875 G -  74448 B + (128 << 20) + (1 << 19)) >> 20
Y per pixel; U and V from the ONE pixel at the even row and even column of each 2 x 2 block (no averaging); NV12 interleaves the same samples.
cv2 cannot be imported where this was written: the constants and the sampling rule are written from memory of the OpenCV source, not taken
from a run of cv2.  Anchors that hold whatever that memory is worth (tests/test_annot_cpu.py): every grey (v, v, v) gives U = V = 128 and
Y = (900726 v + 17301504) >> 20 (16 for 0, 235 for 255); the coefficient rows sum to 900726, 1 and 1.  Chroma is taken from the ANNOTATED pixel.

This is the oracle of tests/test_gpu_annot.py; it writes any layout of include/eagle.h's EagleYuvLayout."""
import numpy as np

import yuv_ref

ARC, LABEL, DISC, TRI = 0, 1, 2, 3
ARC_A, ARC_B = 35, 18
ARC_D1, ARC_D2 = (-7, -10), (1, -1)
COORD_MAX, RADIUS_MAX, MAX_ID = 1 << 20, 1 << 14, 99999
MAX_PRIMS = 2 * 300 + 87 + 1                      # include/eagle.h EAGLE_MAX_PRIMS: two per detection, the key-points, one ball
GLYPH_W, GLYPH_H, GLYPH_ADVANCE = 10, 14, 12
# the test module's own copy of the glyph table (the library's is csrc/annot_font.h): digit -> 7 rows, bit 4 = leftmost column
FONT = ((0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E), (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E), (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F),
        (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E), (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02), (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
        (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E), (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08), (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E),
        (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C))

GREEN, RED, BLUE, WHITE, BLACK = (0, 255, 0), (0, 0, 255), (255, 0, 0), (255, 255, 255), (0, 0, 0)      # BGR
KP_RADIUS = 6
CY = (269484, 528482, 102760)       # R, G, B
CU = (-155188, -305135, 460324)
CV = (460324, -385875, -74448)
SHIFT = 20
BGR, NV12, I420 = "bgr", "nv12", "i420"


def arc(cx, cy, color):
    return (ARC, int(cx), int(cy), 0, 0, 0, 0, tuple(color))


def label(x, y, ident, color):
    return (LABEL, int(x), int(y), int(ident), 0, 0, 0, tuple(color))


def disc(cx, cy, r, color):
    return (DISC, int(cx), int(cy), int(r), 0, 0, 0, tuple(color))


def tri(x0, y0, x1, y1, x2, y2, color):
    return (TRI, int(x0), int(y0), int(x1), int(y1), int(x2), int(y2), tuple(color))


def ball_marker(x, y, color=GREEN):
    return tri(x, y - 20, x - 5, y - 30, x + 5, y - 30, color)


# ---- coverage: boolean masks over pixel grids (X, Y int64 arrays of equal shape) --------------------------------------------------
def _arc_f(dx, dy):
    return ARC_B * ARC_B * dx * dx + ARC_A * ARC_A * dy * dy - ARC_A * ARC_A * ARC_B * ARC_B


def arc_outline(dx, dy):
    """the closed outline before the gap is removed"""
    inside = _arc_f(dx, dy) <= 0
    edge = (_arc_f(dx - 1, dy) > 0) | (_arc_f(dx + 1, dy) > 0) | (_arc_f(dx, dy - 1) > 0) | (_arc_f(dx, dy + 1) > 0)
    return inside & edge


def arc_gap(dx, dy):
    px, py = ARC_B * dx, ARC_A * dy
    c1 = ARC_D1[0] * py - ARC_D1[1] * px
    c2 = px * ARC_D2[1] - py * ARC_D2[0]
    return (c1 > 0) & (c2 > 0)


def label_digits(ident):
    return [int(c) for c in str(int(ident))] if 0 <= int(ident) <= MAX_ID else []


def covers(prim, X, Y):
    kind, a = prim[0], prim[1:7]
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    if kind == ARC:
        dx, dy = X - a[0], Y - a[1]
        return arc_outline(dx, dy) & ~arc_gap(dx, dy)
    if kind == DISC:
        dx, dy = X - a[0], Y - a[1]
        return dx * dx + dy * dy <= a[2] * a[2]
    if kind == TRI:
        x0, y0, x1, y1, x2, y2 = a
        s = -1 if (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) < 0 else 1
        e0 = s * ((x1 - x0) * (Y - y0) - (y1 - y0) * (X - x0))
        e1 = s * ((x2 - x1) * (Y - y1) - (y2 - y1) * (X - x1))
        e2 = s * ((x0 - x2) * (Y - y2) - (y0 - y2) * (X - x2))
        box = (X >= min(x0, x1, x2)) & (X <= max(x0, x1, x2)) & (Y >= min(y0, y1, y2)) & (Y <= max(y0, y1, y2))
        return (e0 >= 0) & (e1 >= 0) & (e2 >= 0) & box
    if kind == LABEL:
        digs = label_digits(a[2])
        m = np.zeros(X.shape, bool)
        ux, uy = X - (a[0] - 3), Y - (a[1] - (GLYPH_H - 1))
        for k, d in enumerate(digs):
            gx = ux - GLYPH_ADVANCE * k
            ok = (gx >= 0) & (gx < GLYPH_W) & (uy >= 0) & (uy < GLYPH_H)
            rows = np.asarray(FONT[d], np.int64)[np.clip(uy // 2, 0, 6)]
            m |= ok & (((rows >> (4 - np.clip(gx // 2, 0, 4))) & 1) == 1)
        return m
    raise ValueError(f"unknown primitive kind {kind}")


def bbox(prim):
    """inclusive (x0, y0, x1, y1) outside of which the primitive covers nothing (None: it covers nothing at all)"""
    kind, a = prim[0], prim[1:7]
    if kind == ARC:
        return a[0] - ARC_A, a[1] - ARC_B, a[0] + ARC_A, a[1] + ARC_B
    if kind == DISC:
        return a[0] - a[2], a[1] - a[2], a[0] + a[2], a[1] + a[2]
    if kind == TRI:
        return min(a[0], a[2], a[4]), min(a[1], a[3], a[5]), max(a[0], a[2], a[4]), max(a[1], a[3], a[5])
    nd = len(label_digits(a[2]))
    if nd == 0:
        return None
    return a[0] - 3, a[1] - (GLYPH_H - 1), a[0] - 3 + GLYPH_ADVANCE * nd - 3, a[1]


def check_prim(prim):
    kind, a = prim[0], prim[1:7]
    coords = a[:2] if kind in (ARC, LABEL, DISC) else a
    assert all(abs(int(c)) <= COORD_MAX for c in coords), prim
    assert kind != DISC or 0 <= a[2] <= RADIUS_MAX, prim


def draw(frame, prims):
    """one BGR frame uint8 [h, w, 3] + its primitive list -> the annotated frame (a copy)"""
    out = np.array(frame, np.uint8, copy=True)
    h, w = out.shape[:2]
    for p in prims:
        check_prim(p)
        bb = bbox(p)
        if bb is None:
            continue
        x0, y0, x1, y1 = max(bb[0], 0), max(bb[1], 0), min(bb[2], w - 1), min(bb[3], h - 1)
        if x0 > x1 or y0 > y1:
            continue
        Y, X = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        out[y0:y1 + 1, x0:x1 + 1][covers(p, X, Y)] = p[7]
    return out


# ---- what the library draws for a record -------------------------------------------------------------------------------------
def _in_domain(*c):
    return all(abs(int(v)) <= COORD_MAX - 64 for v in c)


def overlay_from_record(rec, team_mapping=None):
    """One EagleFrameResult (a lib.RESULT_DTYPE element) -> its primitive list: persons in detection order (ARC + LABEL at the foot point; green
    goalkeepers, team 0 red, any other team blue, players missing from the mapping skipped as main.py:64-65 does; team_mapping None: every player
    white), then the marker of the FIRST reported ball, then a black disc per key-point that records.to_reference_dict(rec) lists under
    "Keypoints" (the RANSAC inliers when the record has a homography, every key-point otherwise; one per label, the last entry of a label
    winning as in a dict).  Entities further than COORD_MAX - 64 from the origin are not drawn."""
    prims = []
    dets = rec["det"][: int(rec["n_det"])]
    for d in dets:
        cls = int(d["cls"])
        if not d["reported"] or cls not in (0, 1):
            continue
        ident, x, y = int(d["id"]), int(d["foot_x"]), int(d["foot_y"])
        if cls == 1:
            color = GREEN
        elif team_mapping is None:
            color = WHITE
        elif ident in team_mapping:
            color = RED if int(team_mapping[ident]) == 0 else BLUE
        else:
            continue
        if _in_domain(x, y):
            prims += [arc(x, y, color), label(x, y, ident, color)]
    for d in dets:
        if d["reported"] and int(d["cls"]) == 2:
            if _in_domain(int(d["foot_x"]), int(d["foot_y"])):
                prims.append(ball_marker(int(d["foot_x"]), int(d["foot_y"])))
            break
    kps = {}
    inliers_only = bool(rec["H_valid"])
    for k in rec["kp"][: int(rec["n_kp"])]:
        if not inliers_only or (k["on_plane"] and k["inlier"]):
            kps[int(k["label"])] = (int(k["x"]), int(k["y"]))
    prims += [disc(x, y, KP_RADIUS, BLACK) for x, y in kps.values() if _in_domain(x, y)]
    return prims


# ---- BGR -> 4:2:0 ---------------------------------------------------------------------------------------------------------------
def bgr_to_planes(bgr):
    """BGR uint8 [n, h, w, 3] (h, w even) -> Y [n, h, w], U, V [n, h/2, w/2] (int64)"""
    a = np.asarray(bgr, np.int64)
    B, G, R = a[..., 0], a[..., 1], a[..., 2]
    half = 1 << (SHIFT - 1)
    Yp = (CY[0] * R + CY[1] * G + CY[2] * B + (16 << SHIFT) + half) >> SHIFT
    Be, Ge, Re = B[:, 0::2, 0::2], G[:, 0::2, 0::2], R[:, 0::2, 0::2]
    U = (CU[0] * Re + CU[1] * Ge + CU[2] * Be + (128 << SHIFT) + half) >> SHIFT
    V = (CV[0] * Re + CV[1] * Ge + CV[2] * Be + (128 << SHIFT) + half) >> SHIFT
    return Yp, U, V


def bgr_to_yuv(fmt, bgr):
    """BGR uint8 [n, h, w, 3] -> dense 4:2:0 frames uint8 [n, 3h/2, w] (cv2 / numpy convention)"""
    n, h, w, _ = np.asarray(bgr).shape
    return yuv_ref.pack(fmt, *bgr_to_planes(bgr), None).reshape(n, h * 3 // 2, w)


def resolve_bgr(h, w, layout=None):
    lay = dict(layout or {})
    pitch = lay.get("y_pitch") or 3 * w
    return {"frame_stride": lay.get("frame_stride") or pitch * h, "y_pitch": pitch}


def span(fmt, h, w, layout, n):
    """bytes n output frames of this layout span"""
    if fmt == BGR:
        L = resolve_bgr(h, w, layout)
        return (n - 1) * L["frame_stride"] + L["y_pitch"] * (h - 1) + 3 * w
    L = yuv_ref.resolve(fmt, h, w, layout)
    ends = [L["y_pitch"] * (h - 1) + w, L["c_offset"] + L["c_pitch"] * (h // 2 - 1) + (w if fmt == NV12 else w // 2)]
    if fmt == I420:
        ends.append(L["v_offset"] + L["c_pitch"] * (h // 2 - 1) + w // 2)
    return (n - 1) * L["frame_stride"] + max(ends)


def annotate(frames, prim_lists, fmt=BGR, layout=None, fill=0):
    """frames uint8 [n, h, w, 3] + one primitive list per frame -> a flat uint8 buffer holding the n annotated frames in the given output format
    and layout (include/eagle.h EagleYuvLayout; BGR: y_pitch = row pitch); bytes between rows / planes / frames = fill."""
    frames = np.asarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    drawn = np.stack([draw(frames[i], prim_lists[i]) for i in range(n)]) if n else frames
    if fmt == BGR:
        L = resolve_bgr(h, w, layout)
        buf = np.full(span(fmt, h, w, layout, n), fill, np.uint8)
        for k in range(n):
            for r in range(h):
                o = k * L["frame_stride"] + r * L["y_pitch"]
                buf[o: o + 3 * w] = drawn[k, r].reshape(-1)
        return buf
    return yuv_ref.pack(fmt, *bgr_to_planes(drawn), layout, fill=fill)


def annotate_dense(frames, prim_lists, fmt=BGR):
    """the dense result in the numpy convention: [n, h, w, 3] (BGR) or [n, 3h/2, w] (4:2:0)"""
    n, h, w, _ = np.asarray(frames).shape
    buf = annotate(frames, prim_lists, fmt)
    return buf.reshape(n, h, w, 3) if fmt == BGR else buf.reshape(n, h * 3 // 2, w)
