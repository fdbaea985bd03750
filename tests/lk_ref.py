"""A plain second reference for the optical-flow kernels (K11 gray / pyrDown, K12 pyramidal Lucas-Kanade, the filter stage of
calculate_optical_flow), written from OpenCV's definitions and independent of oracle/eo_flow.c and of the HIP kernels:

  cvtColor(BGR2GRAY), 8 bit   (3735 B + 19235 G + 9798 R + 2^14) >> 15
  pyrDown, 8 bit              [1 4 6 4 1] x [1 4 6 4 1], (sum + 128) >> 8, BORDER_REFLECT_101, size (h + 1) / 2 x (w + 1) / 2
  buildOpticalFlowPyramid     a further level is built only while its size exceeds winSize in both directions
  calcOpticalFlowPyrLK        winSize 15 x 15, maxLevel 2, criteria (EPS | COUNT, 10, 0.03), minEigThreshold 1e-4, flags 0, err requested:
                              Scharr derivatives of the WHOLE level (reflected at the image edge, zero outside the image), W_BITS = 14
                              bilinear weights, the I window and its derivatives descaled to 16 bit, the 2 x 2 system per level, at
                              most 10 Newton steps, then the rule that the final window must start inside the frame
  cvtColor(BGR2HSV), 8 bit    hue by the 180-range fixed-point table (hsv_shift 12)

Whole images are padded once per level and windows are cut out with numpy slices; there is no per-pixel reflect function and no per-thread
layout here.  The integer window sums are exact (int64, every term below 2^26, 225 terms) and converted to float32 once, which is this
project's stated deviation from OpenCV's float accumulation (oracle/eo_flow.c header); every float step is np.float32 in cv2's order.
lk() also returns a trace of what it did, from which tests/test_lk_cases_cpu.py proves what each constructed case forces."""
import numpy as np

WIN = 15
W_BITS = 14
MAX_LEVEL = 2
MAX_COUNT = 10
EPSILON = 0.03
MIN_EIG = 1e-4
PAD = WIN + 2                     # window origins lie in [-WIN, size - 1] and a window reads 16 pixels from its origin
F = np.float32


def gray(bgr):
    b = np.asarray(bgr).astype(np.int64)
    return ((3735 * b[..., 0] + 19235 * b[..., 1] + 9798 * b[..., 2] + (1 << 14)) >> 15).astype(np.uint8)


def pyrdown(g):
    g = np.asarray(g)
    h, w = g.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    p = np.pad(g.astype(np.int64), 2, mode="reflect")                 # numpy's "reflect" is BORDER_REFLECT_101
    k = (1, 4, 6, 4, 1)
    rows = sum(k[b] * p[:, b:b + 2 * dw:2][:, :dw] for b in range(5))
    full = sum(k[a] * rows[a:a + 2 * dh:2][:dh] for a in range(5))
    return ((full + 128) >> 8).astype(np.uint8)


def level_sizes(h, w):
    """[(h, w) of level 0, 1, ...] of the levels calcOpticalFlowPyrLK uses."""
    sizes = [(h, w)]
    while len(sizes) <= MAX_LEVEL:
        h, w = (h + 1) // 2, (w + 1) // 2
        if h <= WIN or w <= WIN:
            break
        sizes.append((h, w))
    return sizes


def levels(h, w):
    """Index of the highest pyramid level in use."""
    return len(level_sizes(h, w)) - 1


def _scharr(img):
    """calcScharrDeriv: (dx, dy) of the whole image as int64 (they fit 16 bit: |d| <= 16 * 255), rows and columns reflected at the edges."""
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    smooth_y = 3 * (p[:-2] + p[2:]) + 10 * p[1:-1]                    # [h, w + 2]
    diff_y = p[2:] - p[:-2]
    dx = smooth_y[:, 2:] - smooth_y[:, :-2]
    dy = 3 * (diff_y[:, 2:] + diff_y[:, :-2]) + 10 * diff_y[:, 1:-1]
    return dx, dy


def _weights(a, b):
    one, s = F(1), F(1 << W_BITS)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _interp(buf, oy, ox, wts, shift):
    """The 15 x 15 window with origin (oy, ox) (image coordinates) of a padded plane, bilinear with integer weights, rounded down by `shift` bits."""
    blk = buf[oy + PAD:oy + PAD + WIN + 1, ox + PAD:ox + PAD + WIN + 1]
    v = blk[:-1, :-1] * wts[0] + blk[:-1, 1:] * wts[1] + blk[1:, :-1] * wts[2] + blk[1:, 1:] * wts[3]
    return ((v + (1 << (shift - 1))) >> shift).astype(np.int16).astype(np.int64)


def _outside(x, y, w, h):
    """cv2: floor(x) < -winSize.width || floor(x) >= cols (same for y) of a float32 window origin; a non-finite origin is outside."""
    if not (np.isfinite(x) and np.isfinite(y)):
        return True, 0, 0
    ix, iy = int(np.floor(x)), int(np.floor(y))
    return ix < -WIN or ix >= w or iy < -WIN or iy >= h, ix, iy


def _pyramid(g):
    out = [np.asarray(g, np.uint8)]
    for _ in range(levels(*out[0].shape)):
        out.append(pyrdown(out[-1]))
    return out


def lk(I, J, pts):
    """calcOpticalFlowPyrLK(I, J, pts) on gray u8 images -> (next [n, 2] f32, status [n] u8, trace).

    trace[p][level] = {"origin": (x, y) of the I window, "skipped": why the level ended before its iterations (or None), "lost": at level 0, which of the four
    rules took the status ("I window outside", "minEig / determinant", "J window outside", "final window outside"; else None), "A": (sA11, sA12, sA22) raw
    integer sums, "A_f32": the three float32 matrix entries, "iters": [{"origin": (x, y) of the J window, "sb1", "sb2": raw integer sums, "part1",
    "part2": their partial sums over the window pixels e = 64 k .. 64 k + 63 (e = 15 row + column)}]}."""
    I = np.asarray(I, np.uint8); J = np.asarray(J, np.uint8)
    assert I.shape == J.shape and I.ndim == 2
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    pyr_i, pyr_j = _pyramid(I), _pyramid(J)
    top = len(pyr_i) - 1
    planes = []
    for gi, gj in zip(pyr_i, pyr_j):
        dx, dy = _scharr(gi)
        planes.append((np.pad(gi.astype(np.int64), PAD, mode="reflect"), np.pad(dx, PAD), np.pad(dy, PAD), np.pad(gj.astype(np.int64), PAD, mode="reflect")))
    half = F((WIN - 1) * 0.5)
    flt_scale = F(1.0 / (1 << 20))
    eps2 = EPSILON * EPSILON
    nxt_out = np.zeros((len(pts), 2), np.float32)
    status = np.ones(len(pts), np.uint8)
    trace = []
    for p, (x0, y0) in enumerate(pts):
        tr = {}
        nxt = (F(0), F(0))
        ok = True
        for level in range(top, -1, -1):
            h, w = pyr_i[level].shape
            ibuf, dxbuf, dybuf, jbuf = planes[level]
            scale = F(1.0 / (1 << level))
            prev = (x0 * scale, y0 * scale)
            nxt = prev if level == top else (nxt[0] * F(2), nxt[1] * F(2))
            t = tr[level] = {"origin": None, "skipped": None, "lost": None, "A": None, "A_f32": None, "iters": []}
            wx, wy = prev[0] - half, prev[1] - half
            out, ipx, ipy = _outside(wx, wy, w, h)
            if out:
                t["skipped"] = "I window outside"
                if level == 0:
                    ok = False; t["lost"] = t["skipped"]
                continue
            t["origin"] = (ipx, ipy)
            wts = _weights(wx - F(ipx), wy - F(ipy))
            iwin = _interp(ibuf, ipy, ipx, wts, W_BITS - 5)
            ix = _interp(dxbuf, ipy, ipx, wts, W_BITS)
            iy = _interp(dybuf, ipy, ipx, wts, W_BITS)
            sums = (int((ix * ix).sum()), int((ix * iy).sum()), int((iy * iy).sum()))
            a11, a12, a22 = (F(s) * flt_scale for s in sums)
            t["A"] = sums; t["A_f32"] = (a11, a12, a22)
            det = a11 * a22 - a12 * a12
            min_eig = (a22 + a11 - np.sqrt((a11 - a22) * (a11 - a22) + F(4) * a12 * a12)) / F(2 * WIN * WIN)
            if float(min_eig) < MIN_EIG or det < np.finfo(np.float32).eps:
                t["skipped"] = "minEig / determinant"
                if level == 0:
                    ok = False; t["lost"] = t["skipped"]
                continue
            det = F(1) / det
            cx, cy = nxt[0] - half, nxt[1] - half
            pdx = pdy = F(0)
            for j in range(MAX_COUNT):
                out, inx, iny = _outside(cx, cy, w, h)
                if out:
                    if level == 0:
                        ok = False; t["lost"] = "J window outside"
                    break
                jw = _weights(cx - F(inx), cy - F(iny))
                diff = _interp(jbuf, iny, inx, jw, W_BITS - 5) - iwin
                t1, t2 = (diff * ix).ravel(), (diff * iy).ravel()
                sb1, sb2 = int(t1.sum()), int(t2.sum())
                t["iters"].append({"origin": (inx, iny), "sb1": sb1, "sb2": sb2,
                                   "part1": [int(t1[k:k + 64].sum()) for k in range(0, WIN * WIN, 64)],
                                   "part2": [int(t2[k:k + 64].sum()) for k in range(0, WIN * WIN, 64)]})
                b1, b2 = F(sb1) * flt_scale, F(sb2) * flt_scale
                ddx = (a12 * b2 - a22 * b1) * det
                ddy = (a12 * b1 - a11 * b2) * det
                cx, cy = cx + ddx, cy + ddy
                nxt = (cx + half, cy + half)
                if float(ddx) * float(ddx) + float(ddy) * float(ddy) <= eps2:
                    break
                if j > 0 and abs(float(ddx + pdx)) < 0.01 and abs(float(ddy + pdy)) < 0.01:
                    nxt = (nxt[0] - ddx * F(0.5), nxt[1] - ddy * F(0.5))
                    break
                pdx, pdy = ddx, ddy
            if ok and level == 0:                           # the err output: the final window, rounded, must start inside the frame
                fx, fy = nxt[0] - half, nxt[1] - half
                rx, ry = (int(np.rint(fx)), int(np.rint(fy))) if np.isfinite(fx) and np.isfinite(fy) else (w, h)
                if rx < -WIN or rx >= w or ry < -WIN or ry >= h:
                    ok = False; t["lost"] = "final window outside"
        nxt_out[p] = nxt
        status[p] = 1 if ok else 0
        trace.append(tr)
    return nxt_out, status, trace


def hue180(b, g, r):
    """H of cvtColor(BGR2HSV) for one 8-bit pixel, hue range 180."""
    b, g, r = int(b), int(g), int(r)
    v, d = max(b, g, r), max(b, g, r) - min(b, g, r)
    if d == 0:
        return 0
    sector = (g - b) if v == r else (b - r + 2 * d) if v == g else (r - g + 4 * d)
    hdiv = int(round((180 << 12) / (6.0 * d)))             # saturate_cast<int>(double): round half to even, as Python's round
    hh = (sector * hdiv + (1 << 11)) >> 12
    return hh + 180 if hh < 0 else hh


def _hue_mean(frame, pt):
    h, w = frame.shape[:2]
    x, y = (int(v) for v in np.asarray(pt).astype(int))
    x = min(max(x, 0), w - 1); y = min(max(y, 0), h - 1)
    grid = frame[max(0, y - 1):min(h, y + 2), max(0, x - 1):min(w, x + 2)].reshape(-1, 3)
    return np.mean(np.array([hue180(*px) for px in grid], np.uint8))


def filter(frame, kps, nxt, status):
    """calculate_optical_flow after the cv2 call (cm.py:438-478): kps = [(label, (x, y))] in dict order, nxt / status = lk()'s output for those points, frame =
    the BGR frame the hue windows are read from -> [(label, (x, y))] in dict order.  Row j of the surviving points carries the j-th label of the unfiltered
    list, as the reference's bookkeeping does."""
    prev = np.array([xy for _, xy in kps], np.float32).reshape(-1, 2)
    keep = np.asarray(status).reshape(-1) == 1
    new, old = np.asarray(nxt, np.float32)[keep], prev[keep]
    if len(new) == 0:
        return []
    move = np.linalg.norm(new - old, axis=1)
    mean, std = np.mean(move), np.std(move) + 1e-6
    out = []
    for j, (o, n) in enumerate(zip(old, new)):
        if (move[j] - mean) / std > 2:
            continue
        if abs(_hue_mean(frame, n) - _hue_mean(frame, o)) > 25:
            continue
        out.append((kps[j][0], tuple(int(v) for v in n.astype(int))))
    return out


def flow(frames, src, dst, hue, kps):
    """calculate_optical_flow(frames[hue], gray(frames[src]), kps, gray(frames[dst])) -> (filtered list, next, status, trace)."""
    if len(kps) == 0:
        return [], np.zeros((0, 2), np.float32), np.zeros(0, np.uint8), []
    nxt, st, tr = lk(gray(frames[src]), gray(frames[dst]), np.array([xy for _, xy in kps], np.float32))
    return filter(frames[hue], kps, nxt, st), nxt, st, tr
