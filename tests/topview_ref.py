"""The written definition of the top view (K32; include/eagle.h eagle_topview_*, csrc/topview.hip): every byte of the warped frames, the mosaic, its
count map and the per-frame residual triples.  Stated twice: vectorised over the canvas (numpy, float64 and int64) and as a scalar loop over pixels
(Python floats, which are IEEE doubles, for the projective map and Python ints behind it).  The kernels equal it with no tolerance.

CANVAS   the minimap's: S even in 2 .. 32, M even in 0 .. 64, W = 105 S + 2 M, Hc = 68 S + 2 M.  Pixel (X, Y) stands for the pitch point
         x = (X - M) / S, y = 68 - (Y - M) / S (float64, one operation each).
MAP      per frame, float64, every product and sum a single rounded operation: A = adj(H) (COFACTORS below: two products and one difference each),
         det = (h0 A0 + h1 A3) + h2 A6, sb = (h6 (w - 1) / 2 + h7 (h - 1)) + h8.  No map when valid == 0, when any of H, A, det, sb is not finite,
         when det == 0 or sb == 0.  G = A when det and sb have the same sign, else -A.
SAMPLE   u' = ((G0 x) + (G1 y)) + G2, v' and w' from rows 1 and 2; u = u' / w', v = v' / w'; tu = u 256 + 0.5, tv = v 256 + 0.5.  Covered iff
         w' > 0, 0 <= tu < 256 (w - 1) + 1 and 0 <= tv < 256 (h - 1) + 1 (NaN fails).  U = floor(tu): x0 = U >> 8, fx = U & 255, x1 = min(x0 + 1,
         w - 1), likewise in y; channel = ((256 - fx)(256 - fy) p00 + fx (256 - fy) p10 + (256 - fx) fy p01 + fx fy p11 + 32768) >> 16.
VIDEO    covered pixels the sample, the others `background`; with `markings` the minimap's marking mask in `marking_colour` on top.
MOSAIC   over the frames first, first + step, ...: a frame adds its sample to sumB, sumG, sumR and 1 to cnt where the pixel is covered and, with
         mask_boxes, (u, v) lies in no box of the frame: x1 - pad <= u <= x2 + pad and y1 - pad <= v <= y2 + pad, the float32 boxes widened
         exactly.  Picture: (2 sum + cnt) // (2 cnt) where cnt >= min_count, else background; markings on request.
RESIDUAL for every frame f: over the pixels f would add (covered, not masked) where cnt >= min_count, res_sum = sum |sample - mosaic| over B, G, R,
         res_cnt their number; covered = the covered pixels with M <= X < M + 105 S and M <= Y < M + 68 S."""
import numpy as np

import annot_ref as A
import minimap_ref as MR

F = np.float64
MAX_DET = 300
MAX_FRAMES = 1 << 23
BLACK, RED = 0x000000, 0xFF0000                                # B | G << 8 | R << 16
DEFAULTS = dict(background=BLACK, markings=0, marking_colour=RED, mask_boxes=0, box_pad=0.0, first=0, step=1, min_count=1)
# cofactor k = h[a] h[b] - h[c] h[d]
COFACTORS = ((4, 8, 5, 7), (2, 7, 1, 8), (1, 5, 2, 4), (5, 6, 3, 8), (0, 8, 2, 6), (2, 3, 0, 5), (3, 7, 4, 6), (1, 6, 0, 7), (0, 4, 1, 3))


def params(S, M, **kw):
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, scale=S, margin=M, **kw)


def size(S, M):
    return MR.size(S, M)


def colour(c):
    return np.array([c & 255, (c >> 8) & 255, (c >> 16) & 255], np.uint8)


def frame_map(H, valid, h, w):
    """-> G, float64 [9], or None when the frame has no map"""
    if not valid:
        return None
    with np.errstate(all="ignore"):
        Hm = np.asarray(H, F).reshape(9)
        Aj = np.array([Hm[a] * Hm[b] - Hm[c] * Hm[d] for a, b, c, d in COFACTORS], F)
        det = (Hm[0] * Aj[0] + Hm[1] * Aj[3]) + Hm[2] * Aj[6]
        sb = (Hm[6] * (F(w - 1) / F(2)) + Hm[7] * F(h - 1)) + Hm[8]
    if not (np.isfinite(Hm).all() and np.isfinite(Aj).all() and np.isfinite(det) and np.isfinite(sb)) or det == 0 or sb == 0:
        return None
    return Aj if (det > 0) == (sb > 0) else -Aj


def pitch_axes(S, M):
    W, Hc = size(S, M)
    x = (np.arange(W, dtype=np.int64) - M).astype(F) / F(S)
    y = F(68) - (np.arange(Hc, dtype=np.int64) - M).astype(F) / F(S)
    return x, y


# ---- vectorised ---------------------------------------------------------------------------------------------------------------
def project(G, S, M):
    """-> u', v', w' float64 [Hc, W]"""
    x, y = pitch_axes(S, M)
    x, y = x[None, :], y[:, None]
    with np.errstate(all="ignore"):
        return tuple(((G[3 * r] * x) + (G[3 * r + 1] * y)) + G[3 * r + 2] for r in range(3))


def sample_points(G, S, M, h, w):
    """-> u, v, w', tu, tv float64 [Hc, W] and covered bool [Hc, W]"""
    up, vp, wp = project(G, S, M)
    with np.errstate(all="ignore"):
        u, v = up / wp, vp / wp
        tu, tv = u * F(256) + F(0.5), v * F(256) + F(0.5)
        cov = (wp > 0) & (tu >= 0) & (tu < F(256 * (w - 1) + 1)) & (tv >= 0) & (tv < F(256 * (h - 1) + 1))
    return u, v, wp, tu, tv, cov


def numerators(frame, G, S, M):
    """-> (covered, the sums in front of + 32768 and >> 16 int64 [Hc, W, 3], fx, fy int64 [Hc, W], u, v)"""
    h, w, _ = frame.shape
    u, v, _, tu, tv, cov = sample_points(G, S, M, h, w)
    U = np.floor(np.where(cov, tu, 0)).astype(np.int64)
    V = np.floor(np.where(cov, tv, 0)).astype(np.int64)
    x0, fx, y0, fy = U >> 8, U & 255, V >> 8, V & 255
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    f = frame.astype(np.int64)
    ax, ay = fx[..., None], fy[..., None]
    num = (256 - ax) * (256 - ay) * f[y0, x0] + ax * (256 - ay) * f[y0, x1] + (256 - ax) * ay * f[y1, x0] + ax * ay * f[y1, x1]
    return cov, num, fx, fy, u, v


def sample(frame, G, S, M):
    """one frame -> (covered bool [Hc, W], sample uint8 [Hc, W, 3] (0 where not covered), u, v float64 [Hc, W])"""
    W, Hc = size(S, M)
    if G is None:
        nan = np.full((Hc, W), np.nan)
        return np.zeros((Hc, W), bool), np.zeros((Hc, W, 3), np.uint8), nan, nan
    cov, num, _, _, u, v = numerators(frame, G, S, M)
    return cov, np.where(cov[..., None], (num + 32768) >> 16, 0).astype(np.uint8), u, v


def in_boxes(u, v, boxes, pad):
    """float64 [Hc, W] sample points, float32 [k, 4] boxes -> bool [Hc, W]"""
    hit = np.zeros(u.shape, bool)
    pad = F(pad)
    with np.errstate(all="ignore"):
        for x1, y1, x2, y2 in np.asarray(boxes, np.float32).reshape(-1, 4).astype(F):
            hit |= (x1 - pad <= u) & (u <= x2 + pad) & (y1 - pad <= v) & (v <= y2 + pad)
    return hit


def _paint(pic, p):
    if p["markings"]:
        pic[MR.markings(p["scale"], p["margin"])] = colour(p["marking_colour"])
    return pic


def _maps(frames, Hs, valid):
    n, h, w, _ = frames.shape
    return [frame_map(np.asarray(Hs, F).reshape(-1, 9)[i], np.asarray(valid).reshape(-1)[i], h, w) for i in range(n)]


def frames_bgr(frames, Hs, valid, p):
    """uint8 [n, h, w, 3] -> the warped frames, uint8 [n, Hc, W, 3]"""
    frames = np.asarray(frames, np.uint8)
    S, M = p["scale"], p["margin"]
    W, Hc = size(S, M)
    out = np.zeros((len(frames), Hc, W, 3), np.uint8)
    for i, G in enumerate(_maps(frames, Hs, valid)):
        cov, s, _, _ = sample(frames[i], G, S, M)
        out[i] = _paint(np.where(cov[..., None], s, colour(p["background"])), p)
    return out


def video(frames, Hs, valid, p, fmt=A.BGR, layout=None, fill=0):
    """the flat buffer of the warped frames in an output format and layout (annot_ref.annotate's)"""
    pics = frames_bgr(frames, Hs, valid, p)
    return A.annotate(pics, [[] for _ in pics], fmt, layout, fill)


def _adds(frame, G, boxes, p):
    """what a frame would add to the mosaic: (adds bool, sample, covered bool)"""
    cov, s, u, v = sample(frame, G, p["scale"], p["margin"])
    adds = cov & ~in_boxes(u, v, boxes, p["box_pad"]) if p["mask_boxes"] else cov
    return adds, s, cov


def _no_boxes(n):
    return [np.zeros((0, 4), np.float32)] * n


def accumulate(frames, Hs, valid, boxes, p):
    """-> acc uint32 [Hc, W, 4]: sumB, sumG, sumR, cnt"""
    frames = np.asarray(frames, np.uint8)
    W, Hc = size(p["scale"], p["margin"])
    assert len(frames) <= MAX_FRAMES
    acc = np.zeros((Hc, W, 4), np.int64)
    boxes = _no_boxes(len(frames)) if boxes is None else boxes
    maps = _maps(frames, Hs, valid) if len(frames) else []
    for i in range(p["first"], len(frames), p["step"]):
        adds, s, _ = _adds(frames[i], maps[i], boxes[i], p)
        acc[..., :3] += np.where(adds[..., None], s, 0)
        acc[..., 3] += adds
    return acc.astype(np.uint32)


def finish(acc, p):
    """acc -> (picture uint8 [Hc, W, 3], cnt uint32 [Hc, W], the unpainted means int64 [Hc, W, 3], where they count bool [Hc, W])"""
    acc = acc.astype(np.int64)
    cnt = acc[..., 3]
    ok = cnt >= p["min_count"]
    c = np.where(ok, cnt, 1)[..., None]
    mean = (2 * acc[..., :3] + c) // (2 * c)
    pic = np.where(ok[..., None], mean, colour(p["background"]).astype(np.int64)).astype(np.uint8)
    return _paint(pic, p), cnt.astype(np.uint32), mean, ok


def residuals(frames, Hs, valid, boxes, p, acc):
    """-> res_sum uint64 [n], res_cnt uint32 [n], covered uint32 [n]"""
    frames = np.asarray(frames, np.uint8)
    S, M = p["scale"], p["margin"]
    n = len(frames)
    _, _, mean, ok = finish(acc, dict(p, markings=0))
    rs, rc, cv = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    boxes = _no_boxes(n) if boxes is None else boxes
    maps = _maps(frames, Hs, valid) if n else []
    for i in range(n):
        adds, s, cov = _adds(frames[i], maps[i], boxes[i], p)
        take = adds & ok
        rs[i] = int(np.abs(s.astype(np.int64) - mean)[take].sum())
        rc[i] = int(take.sum())
        cv[i] = int(cov[M:M + 68 * S, M:M + 105 * S].sum())
    return rs, rc, cv


def topview(frames, Hs, valid, boxes, p):
    """everything of a clip: (warped frames, mosaic picture, cnt, res_sum, res_cnt, covered)"""
    acc = accumulate(frames, Hs, valid, boxes, p)
    pic, cnt, _, _ = finish(acc, p)
    return (frames_bgr(frames, Hs, valid, p), pic, cnt) + residuals(frames, Hs, valid, boxes, p, acc)


# ---- scalar: a loop over pixels, Python floats in the map and Python ints behind it -------------------------------------------
def sample_scalar(frame, G, S, M, X, Y):
    """frame as nested lists, G as Python floats -> (covered, (b, g, r), u, v); Python's floats are IEEE doubles and its operators single operations"""
    h, w = len(frame), len(frame[0])
    x = (X - M) / S
    y = 68.0 - (Y - M) / S
    up = ((G[0] * x) + (G[1] * y)) + G[2]
    vp = ((G[3] * x) + (G[4] * y)) + G[5]
    wp = ((G[6] * x) + (G[7] * y)) + G[8]
    if not wp > 0:                                              # (also w' = 0, which Python will not divide by, and NaN)
        return False, (0, 0, 0), 0.0, 0.0
    u, v = up / wp, vp / wp
    tu, tv = u * 256.0 + 0.5, v * 256.0 + 0.5
    if not (tu >= 0 and tu < float(256 * (w - 1) + 1) and tv >= 0 and tv < float(256 * (h - 1) + 1)):
        return False, (0, 0, 0), u, v
    U, V = int(tu // 1), int(tv // 1)
    x0, fx, y0, fy = U >> 8, U & 255, V >> 8, V & 255
    x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
    px = []
    for c in range(3):
        p00, p10, p01, p11 = frame[y0][x0][c], frame[y0][x1][c], frame[y1][x0][c], frame[y1][x1][c]
        px.append(((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p10 + (256 - fx) * fy * p01 + fx * fy * p11 + 32768) >> 16)
    return True, tuple(px), u, v


def in_boxes_scalar(u, v, boxes, pad):
    pad = float(pad)
    for x1, y1, x2, y2 in boxes:
        if x1 - pad <= u and u <= x2 + pad and y1 - pad <= v and v <= y2 + pad:
            return True
    return False


def topview_scalar(frames, Hs, valid, boxes, p):
    """topview(), pixel by pixel"""
    frames = np.asarray(frames, np.uint8)
    S, M = p["scale"], p["margin"]
    W, Hc = size(S, M)
    n = len(frames)
    boxes = _no_boxes(n) if boxes is None else boxes
    maps = [None if G is None else [float(g) for g in G] for G in _maps(frames, Hs, valid)] if n else []
    boxes = [[tuple(float(t) for t in b) for b in np.asarray(bx, np.float32).reshape(-1, 4)] for bx in boxes]
    frames = [f.tolist() for f in frames]
    bg, mc = [int(t) for t in colour(p["background"])], [int(t) for t in colour(p["marking_colour"])]
    mark = (MR.markings(S, M) if p["markings"] else np.zeros((Hc, W), bool)).tolist()
    vid, pic, cnt = np.zeros((n, Hc, W, 3), np.uint8), np.zeros((Hc, W, 3), np.uint8), np.zeros((Hc, W), np.uint32)
    vid[:], pic[:] = bg, bg
    rs, rc, cv = [0] * n, [0] * n, [0] * n
    mapped = [i for i in range(n) if maps[i] is not None]
    for Y in range(Hc):
        for X in range(W):
            sums, k, mine = [0, 0, 0], 0, []
            for i in mapped:
                cov, px, u, v = sample_scalar(frames[i], maps[i], S, M, X, Y)
                if not cov:
                    continue
                vid[i, Y, X] = px
                cv[i] += int(M <= X < M + 105 * S and M <= Y < M + 68 * S)
                if p["mask_boxes"] and in_boxes_scalar(u, v, boxes[i], p["box_pad"]):
                    continue
                mine.append((i, px))
                if i >= p["first"] and (i - p["first"]) % p["step"] == 0:
                    sums = [a + b for a, b in zip(sums, px)]
                    k += 1
            cnt[Y, X] = k
            if k >= p["min_count"]:
                mean = [(2 * s + k) // (2 * k) for s in sums]
                pic[Y, X] = mean
                for i, px in mine:
                    rs[i] += sum(abs(a - b) for a, b in zip(px, mean))
                    rc[i] += 1
            if mark[Y][X]:
                vid[:, Y, X] = mc
                pic[Y, X] = mc
    return vid, pic, cnt, np.array(rs, np.uint64), np.array(rc, np.uint32), np.array(cv, np.uint32)
