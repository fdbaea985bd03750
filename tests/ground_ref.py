"""The written definition of the ground layer (K34; include/eagle.h eagle_ground_*, csrc/ground.hip): every byte of the pictures and every covered
count.  Stated twice: vectorised over the picture (numpy, float64 and int64) and as a plain loop over pixels and sub-samples (Python floats, which are
IEEE doubles, in front of the quantisation and Python ints behind it).  The kernel equals it with no tolerance.

INPUT    n dense BGR frames [h][w][3], Hs [n][9] float64 row-major image -> pitch, valid [n], per frame a list of at most MAX_SHAPES shapes.
MAP      per frame; pixel centres lie at integers.  sb = (h6 (w - 1) / 2 + h7 (h - 1)) + h8, every operation single.  NO MAP when valid == 0, when
         any h_i or sb is not finite, or when sb == 0: the frame is passed through (its source pixels, covered = 0).
SAMPLES  four per pixel (X, Y), the rotated grid OFFSETS: u = X + dx, v = Y + dy; x' = ((h0 u) + (h1 v)) + h2, y' and w' likewise from rows 1 and
         2.  ON THE GROUND iff w' and sb have the same strict sign, and px = x' / w', py = y' / w' are finite with |px|, |py| <= 1024.  Then
         qx = floor(px 1024 + 0.5), qy likewise (int32): the quantisation q of K30 / K33; everything behind it is integers.
SHAPES   dicts (kind, a [6], colour B | G << 8 | R << 16, alpha 0 .. 256, flags).  BAND a = x0, x1, y0, y1: inside iff x0 <= qx < x1 and
         y0 <= qy < y1.  RING a = cx, cy, r0, r1 (0 <= r0 < r1 <= 2^20): inside iff r0^2 <= (qx - cx)^2 + (qy - cy)^2 < r1^2.  KEYED: drawn only
         where the SOURCE pixel is grass, g >= key_min and g - max(r, b) >= key_lead.
BLEND    per pixel over the frame's shapes in list order, from the source pixel: c = its sub-samples on the ground and inside; skipped when c == 0,
         alpha == 0, or KEYED on a pixel that is not grass; else A = alpha c and channel = (channel (1024 - A) + colour A + 512) >> 10.
         covered[f] = the pixels of frame f that at least one shape blended into.
OUTPUT   BGR, NV12 or I420 in a layout, as annot_ref.annotate writes an unannotated picture."""
import numpy as np

import annot_ref as A

F = np.float64
BAND, RING = 0, 1
KEYED = 1
MAX_SHAPES = 16
Q = 1024
LIMIT = 1024.0
ARG_MAX = 1 << 21
R_MAX = 1 << 20
OFFSETS = ((-0.375, -0.125), (0.125, -0.375), (0.375, 0.125), (-0.125, 0.375))
DEFAULT_KEY = dict(key_min=48, key_lead=16)


def band(x0, x1, y0, y1, colour, alpha, keyed=False):
    return dict(kind=BAND, a=(int(x0), int(x1), int(y0), int(y1), 0, 0), colour=int(colour), alpha=int(alpha), flags=KEYED if keyed else 0)


def ring(cx, cy, r0, r1, colour, alpha, keyed=False):
    return dict(kind=RING, a=(int(cx), int(cy), int(r0), int(r1), 0, 0), colour=int(colour), alpha=int(alpha), flags=KEYED if keyed else 0)


def check_shape(s):
    a = s["a"]
    assert s["kind"] in (BAND, RING) and s["flags"] in (0, KEYED) and 0 <= s["alpha"] <= 256 and 0 <= s["colour"] <= 0xFFFFFF and a[4] == 0 and a[5] == 0
    if s["kind"] == BAND:
        assert a[0] < a[1] and a[2] < a[3] and all(abs(t) <= ARG_MAX for t in a[:4])
    else:
        assert abs(a[0]) <= ARG_MAX and abs(a[1]) <= ARG_MAX and 0 <= a[2] < a[3] <= R_MAX


def frame_sb(H, valid, h, w):
    """-> sb (float64), or None when the frame has no map"""
    if not valid:
        return None
    Hm = np.asarray(H, F).reshape(9)
    with np.errstate(all="ignore"):
        sb = (Hm[6] * (F(w - 1) / F(2)) + Hm[7] * F(h - 1)) + Hm[8]
    if not (np.isfinite(Hm).all() and np.isfinite(sb)) or sb == 0:
        return None
    return sb


def grass(frame, key):
    f = np.asarray(frame, np.int64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    return (g >= key["key_min"]) & (g - np.maximum(r, b) >= key["key_lead"])


# ---- vectorised ---------------------------------------------------------------------------------------------------------------
def samples(H, sb, h, w):
    """-> on bool [4, h, w], qx, qy int64 [4, h, w] (0 where not on the ground), w' float64 [4, h, w]"""
    Hm = np.asarray(H, F).reshape(9)
    X, Y = np.arange(w, dtype=F)[None, :], np.arange(h, dtype=F)[:, None]
    on, qx, qy, ws = [], [], [], []
    with np.errstate(all="ignore"):
        for dx, dy in OFFSETS:
            u, v = X + F(dx), Y + F(dy)
            xp, yp, wp = (((Hm[3 * r] * u) + (Hm[3 * r + 1] * v)) + Hm[3 * r + 2] for r in range(3))
            px, py = xp / wp, yp / wp
            ok = ((wp > 0) if sb > 0 else (wp < 0)) & np.isfinite(px) & np.isfinite(py) & (np.abs(px) <= LIMIT) & (np.abs(py) <= LIMIT)
            on.append(ok)
            qx.append(np.floor(np.where(ok, px, 0) * F(Q) + F(0.5)).astype(np.int64))
            qy.append(np.floor(np.where(ok, py, 0) * F(Q) + F(0.5)).astype(np.int64))
            ws.append(np.broadcast_to(wp, (h, w)))
    return np.stack(on), np.stack(qx), np.stack(qy), np.stack(ws)


def inside(s, qx, qy):
    a = s["a"]
    if s["kind"] == BAND:
        return (a[0] <= qx) & (qx < a[1]) & (a[2] <= qy) & (qy < a[3])
    d2 = (qx - a[0]) ** 2 + (qy - a[1]) ** 2
    return (a[2] ** 2 <= d2) & (d2 < a[3] ** 2)


def coverage(s, on, qx, qy):
    """c int64 [h, w]: the sub-samples on the ground and inside the shape"""
    return (on & inside(s, qx, qy)).sum(0)


def frame_bgr(frame, H, valid, shapes, key=DEFAULT_KEY):
    """one frame -> (picture uint8 [h, w, 3], covered int)"""
    frame = np.asarray(frame, np.uint8)
    h, w, _ = frame.shape
    assert len(shapes) <= MAX_SHAPES
    for s in shapes:
        check_shape(s)
    sb = frame_sb(H, valid, h, w)
    if sb is None or not shapes:
        return frame.copy(), 0
    on, qx, qy, _ = samples(H, sb, h, w)
    gr = grass(frame, key)
    px = frame.astype(np.int64)
    hit = np.zeros((h, w), bool)
    for s in shapes:
        c = coverage(s, on, qx, qy)
        take = (c > 0) & (s["alpha"] > 0)
        if s["flags"] & KEYED:
            take &= gr
        Aw = (s["alpha"] * c)[..., None]
        col = np.array([s["colour"] & 255, (s["colour"] >> 8) & 255, (s["colour"] >> 16) & 255], np.int64)
        px = np.where(take[..., None], (px * (1024 - Aw) + col * Aw + 512) >> 10, px)
        hit |= take
    return px.astype(np.uint8), int(hit.sum())


def frames_bgr(frames, Hs, valid, shape_lists, key=DEFAULT_KEY):
    """-> (pictures uint8 [n, h, w, 3], covered uint32 [n])"""
    frames = np.asarray(frames, np.uint8)
    out, cov = np.zeros_like(frames), np.zeros(len(frames), np.uint32)
    Hs = np.asarray(Hs, F).reshape(-1, 9)
    for i in range(len(frames)):
        out[i], cov[i] = frame_bgr(frames[i], Hs[i], np.asarray(valid).reshape(-1)[i], shape_lists[i], key)
    return out, cov


def ground(frames, Hs, valid, shape_lists, key=DEFAULT_KEY, fmt=A.BGR, layout=None, fill=0):
    """-> (the flat buffer of the pictures in an output format and layout (annot_ref.annotate's), covered)"""
    pics, cov = frames_bgr(frames, Hs, valid, shape_lists, key)
    return A.annotate(pics, [[] for _ in pics], fmt, layout, fill), cov


# ---- scalar: a loop over pixels and sub-samples, Python floats in front of q and Python ints behind it ------------------------------
def sample_scalar(H, sb, X, Y, dx, dy):
    """-> (on, qx, qy, w'); Python's floats are IEEE doubles and its operators single operations"""
    u, v = X + dx, Y + dy
    xp = ((H[0] * u) + (H[1] * v)) + H[2]
    yp = ((H[3] * u) + (H[4] * v)) + H[5]
    wp = ((H[6] * u) + (H[7] * v)) + H[8]
    if not ((wp > 0 and sb > 0) or (wp < 0 and sb < 0)):        # (also w' = 0, which Python will not divide by, and NaN)
        return False, 0, 0, wp
    px, py = xp / wp, yp / wp
    if not (abs(px) <= LIMIT and abs(py) <= LIMIT):            # (NaN and inf fail)
        return False, 0, 0, wp
    return True, int((px * 1024.0 + 0.5) // 1), int((py * 1024.0 + 0.5) // 1), wp


def inside_scalar(s, qx, qy):
    a = s["a"]
    if s["kind"] == BAND:
        return a[0] <= qx < a[1] and a[2] <= qy < a[3]
    return a[2] * a[2] <= (qx - a[0]) * (qx - a[0]) + (qy - a[1]) * (qy - a[1]) < a[3] * a[3]


def frames_bgr_scalar(frames, Hs, valid, shape_lists, key=DEFAULT_KEY, window=None):
    """frames_bgr(), pixel by pixel; window (a slice of rows, a slice of columns): only those pixels are walked, the others keep the source's bytes
    and do not count in covered"""
    frames = np.asarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    out, cov = frames.copy(), np.zeros(n, np.uint32)
    for i in range(n):
        sb = frame_sb(np.asarray(Hs, F).reshape(-1, 9)[i], np.asarray(valid).reshape(-1)[i], h, w)
        if sb is None:
            continue
        H, sb = [float(t) for t in np.asarray(Hs, F).reshape(-1, 9)[i]], float(sb)
        src = frames[i].tolist()
        ys, xs = (range(h), range(w)) if window is None else (range(*window[0].indices(h)), range(*window[1].indices(w)))
        for Y in ys:
            for X in xs:
                sub = [sample_scalar(H, sb, X, Y, dx, dy) for dx, dy in OFFSETS]
                b, g, r = src[Y][X]
                is_grass = g >= key["key_min"] and g - max(r, b) >= key["key_lead"]
                px, hit = [b, g, r], False
                for s in shape_lists[i]:
                    c = sum(1 for on, qx, qy, _ in sub if on and inside_scalar(s, qx, qy))
                    if c == 0 or s["alpha"] == 0 or (s["flags"] & KEYED and not is_grass):
                        continue
                    Aw = s["alpha"] * c
                    px = [(ch * (1024 - Aw) + ((s["colour"] >> (8 * k)) & 255) * Aw + 512) >> 10 for k, ch in enumerate(px)]
                    hit = True
                out[i, Y, X] = px
                cov[i] += hit
    return out, cov
