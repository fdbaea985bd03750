"""The arithmetic of csrc/ecc.hip (K17) in plain numpy, written from the kernels' own statements: ecc_small_kernel's integer taps, and ecc_kernel
iteration by iteration with its fixed-point warp coordinates, its float32 operation order, its 3 x 3 inverse and the summation order of ecc_reduce
(thread t adds pixels t, t + 512, ... in order; the 64-lane tree 32, 16, ..., 1; the waves 0..7 added to 0.0).  It shares no code with
oracle/ecc.py: gradients are taken on the fly with reflected indices, sums are not numpy's pairwise ones, the warp taps are clamped as the
kernel clamps them.  tests/test_ecc_cases_cpu.py holds the two against each other."""
import numpy as np

F32, F64 = np.float32, np.float64
THREADS, LANES = 512, 64
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


# ---- ecc_small_kernel -------------------------------------------------------------------------------------------------------------------------
def small_size(size, scale):
    return int(np.rint(F64(size) * F64(scale)))


def _taps(dsize, inv_scale, ssize):
    """resize_tap_scaled for d = 0 .. dsize - 1: (s0, s1, a0, a1)"""
    d = np.arange(dsize, dtype=F64)
    f = ((d + 0.5) * F64(inv_scale) - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(F32)
    lo, hi = s < 0, s >= ssize - 1
    s = np.where(lo, 0, np.where(hi, ssize - 1, s))
    f = np.where(lo | hi, F32(0), f).astype(F32)
    a0 = np.rint((F32(1) - f) * F32(2048)).astype(np.int16).astype(np.int64)
    a1 = np.rint(f * F32(2048)).astype(np.int16).astype(np.int64)
    return s, np.minimum(s + 1, ssize - 1), a0, a1


def small(gray, scale=0.15, size_ratio=False):
    """gray u8 [h, w] or [n, h, w] -> the scale-sized image(s) of ecc_small_kernel: dh = lrint(h * scale), taps from 1 / scale.  size_ratio restates a
    deliberate break (taps from ssize / dsize, as cv2.resize with a dsize)."""
    g = np.asarray(gray, np.uint8)
    if g.ndim == 3:
        return np.stack([small(x, scale, size_ratio) for x in g])
    h, w = g.shape
    dh, dw = small_size(h, scale), small_size(w, scale)
    inv = 1.0 / F64(scale)
    x0, x1, ax0, ax1 = _taps(dw, F64(w) / F64(dw) if size_ratio else inv, w)
    y0, y1, ay0, ay1 = _taps(dh, F64(h) / F64(dh) if size_ratio else inv, h)
    s = g.astype(np.int64)
    t0 = s[y0][:, x0] * ax0[None, :] + s[y0][:, x1] * ax1[None, :]
    t1 = s[y1][:, x0] * ax0[None, :] + s[y1][:, x1] * ax1[None, :]
    out = (((ay0[:, None] * (t0 >> 4)) >> 16) + ((ay1[:, None] * (t1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


# ---- ecc_reduce -------------------------------------------------------------------------------------------------------------------------------
def reduce(v, waves_backwards=False):
    """float64 [k, npx] -> [k]: the order of ecc_reduce.  (A pixel a thread does not add is a + 0.0 here: the same bits, the sums start at + 0.0.)"""
    v = np.asarray(v, F64)
    k, npx = v.shape
    rounds = -(-npx // THREADS)
    pad = np.zeros((k, rounds * THREADS), F64)
    pad[:, :npx] = v
    pad = pad.reshape(k, rounds, THREADS)
    acc = np.zeros((k, THREADS), F64)
    for r in range(rounds):                                  # thread t: pixels t, t + 512, ...
        acc = acc + pad[:, r]
    acc = acc.reshape(k, THREADS // LANES, LANES)
    off = LANES // 2
    while off:                                               # v += shfl_down(v, off): lane 0 ends with the tree's sum
        acc = acc[:, :, :off] + acc[:, :, off:2 * off]
        off //= 2
    tot = np.zeros(k, F64)
    order = range(THREADS // LANES)
    for wv in (reversed(order) if waves_backwards else order):
        tot = tot + acc[:, wv, 0]
    return tot


# ---- ecc_sample -------------------------------------------------------------------------------------------------------------------------------
def _tap(img, yy, xx):
    h, w = img.shape
    ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
    return np.where(ok, img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(F32), F32(0))


def _gx(img, yy, xx):
    h, w = img.shape
    ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
    y, x = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
    xm, xp = np.where(x == 0, 1, x - 1), np.where(x == w - 1, w - 2, x + 1)
    return np.where(ok, F32(0.5) * (img[y, xp].astype(F32) - img[y, xm].astype(F32)), F32(0))


def _gy(img, yy, xx):
    h, w = img.shape
    ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
    y, x = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
    ym, yp = np.where(y == 0, 1, y - 1), np.where(y == h - 1, h - 2, y + 1)
    return np.where(ok, F32(0.5) * (img[yp, x].astype(F32) - img[ym, x].astype(F32)), F32(0))


def sample(img, M, round_16=16):
    """every pixel of the template's grid (flat, row-major): (iw, gx, gy float32, inside bool, fixed-point X, Y int64 in 1/32 pixel)"""
    h, w = img.shape
    M = [F64(v) for v in M]
    p = np.arange(h * w)
    y, x = p // w, p % w
    xd, yd = x.astype(F64), y.astype(F64)
    ad = np.rint(M[0] * xd * 1024).astype(np.int64); bd = np.rint(M[3] * xd * 1024).astype(np.int64)
    X0 = np.rint((M[1] * yd + M[2]) * 1024).astype(np.int64); Y0 = np.rint((M[4] * yd + M[5]) * 1024).astype(np.int64)
    nx, ny = (X0 + 512 + ad) >> 10, (Y0 + 512 + bd) >> 10
    inside = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
    X, Y = (X0 + round_16 + ad) >> 5, (Y0 + round_16 + bd) >> 5
    sx, sy = np.clip(X >> 5, -4, w + 4), np.clip(Y >> 5, -4, h + 4)
    fx = (X & 31).astype(F32) * F32(1.0 / 32); fy = (Y & 31).astype(F32) * F32(1.0 / 32)
    wx0, wy0 = F32(1) - fx, F32(1) - fy
    w00, w01, w10, w11 = wy0 * wx0, wy0 * fx, fy * wx0, fy * fx

    def blend(f):
        return ((f(img, sy, sx) * w00 + f(img, sy, sx + 1) * w01) + f(img, sy + 1, sx) * w10) + f(img, sy + 1, sx + 1) * w11

    return blend(_tap), blend(_gx), blend(_gy), inside, X, Y


# ---- ecc_inv3 ---------------------------------------------------------------------------------------------------------------------------------
def inv3(Hf):
    S = [F64(v) for v in Hf]
    d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6])
    if d == 0.0:
        return np.zeros(9, F32), d
    det = d
    d = F64(1.0) / d
    out = [(S[4] * S[8] - S[5] * S[7]) * d, (S[2] * S[7] - S[1] * S[8]) * d, (S[1] * S[5] - S[2] * S[4]) * d,
           (S[5] * S[6] - S[3] * S[8]) * d, (S[0] * S[8] - S[2] * S[6]) * d, (S[2] * S[3] - S[0] * S[5]) * d,
           (S[3] * S[7] - S[4] * S[6]) * d, (S[1] * S[6] - S[0] * S[7]) * d, (S[0] * S[4] - S[1] * S[3]) * d]
    return np.array(out, F64).astype(F32), det


def _row3(H, r, v):
    return F32((F64(H[3 * r]) * F64(v[0]) + F64(H[3 * r + 1]) * F64(v[1])) + F64(H[3 * r + 2]) * F64(v[2]))


def _dot3(a, b):
    return (F64(a[0]) * F64(b[0]) + F64(a[1]) * F64(b[1])) + F64(a[2]) * F64(b[2])


def _spread(v, ulps):
    """v (any shape) -> [2 * ulps + 1, ...]: v moved by -ulps .. ulps float64 ulps"""
    v = np.asarray(v, F64)
    out, up, dn = [v], v, v
    for _ in range(ulps):
        up = np.nextafter(up, F64(np.inf)); dn = np.nextafter(dn, F64(-np.inf))
        out += [up, dn]
    return np.stack(out)


def libm_margin_ok(dp0, m3, ulps=4):
    """True where no float32 stored into M depends on the last `ulps` float64 ulps of asin's result, of theta, or of cos's and sin's results: the
    device's maths library and numpy's are not specified to agree there."""
    theta = F64(dp0) + np.arcsin(F64(m3))
    c, s = F32(np.cos(theta)), F32(np.sin(theta))
    th = _spread(F64(dp0) + _spread(np.arcsin(F64(m3)), ulps), ulps)
    return bool(np.all(_spread(np.cos(th), ulps).astype(F32) == c) and np.all(_spread(np.sin(th), ulps).astype(F32) == s))


# ---- ecc_kernel -------------------------------------------------------------------------------------------------------------------------------
def align(template, image, max_iter=100, eps=1e-5, trace=None, check_libm=False, swap_h=False, round_16=16, waves_backwards=False):
    """-> (ok, iters, rho, M float32 [6]) as ecc_kernel writes them: ok = 0 and iters = the iteration that failed where cv2 raises (the warp is then
    what the failed iteration started from).  trace: a list that receives one dict per iteration.  swap_h, round_16, waves_backwards restate
    deliberate breaks of the kernel (tests/test_ecc_cases_cpu.py shows that the cases tell them apart); leave them alone otherwise."""
    T8, I8 = np.asarray(template, np.uint8), np.asarray(image, np.uint8)
    assert T8.shape == I8.shape and T8.ndim == 2
    h, w = T8.shape
    npx = h * w
    Tf = T8.reshape(-1).astype(F32)
    p = np.arange(npx)
    xf, yf = (p % w).astype(F32), (p // w).astype(F32)
    M = np.array(IDENT, F32)
    rho, last_rho = F64(-1.0), F64(-eps)
    it = 0

    def red(rows):
        return reduce(np.stack(rows), waves_backwards)

    with np.errstate(all="ignore"):
        while it < max_iter and abs(rho - last_rho) >= eps:
            it += 1
            rec = {"M_in": M.copy()}
            if trace is not None:
                trace.append(rec)
            iw, gx, gy, inside, X, Y = sample(I8, M, round_16)
            h0, h1 = (M[3], M[0]) if swap_h else (M[0], M[3])
            rec.update(n=int(inside.sum()), outside_nonzero=int((~inside & (iw != 0)).sum()), negative_coords=int(((X < 0) | (Y < 0)).sum()),
                       clamped=int((((X >> 5) < -4) | ((X >> 5) > w + 4) | ((Y >> 5) < -4) | ((Y >> 5) > h + 4)).sum()))
            # pass A
            a, t = iw.astype(F64), Tf.astype(F64)
            z = F64(0)
            tot = red([np.where(inside, F64(1), z), np.where(inside, a, z), np.where(inside, a * a, z), np.where(inside, t, z), np.where(inside, t * t, z)])
            n = tot[0]
            if n == 0.0:
                rec["exit"] = "empty mask"
                return 0, it, float(rho), M
            im, tm = tot[1] / n, tot[3] / n
            iv, tv = max(tot[2] / n - im * im, F64(0)), max(tot[4] / n - tm * tm, F64(0))
            i_mean, t_mean = F32(im), F32(tm)
            i_norm, t_norm = np.sqrt(n * iv), np.sqrt(n * tv)
            # pass B
            izm = np.where(inside, iw - i_mean, iw).astype(F32)
            tzm = np.where(inside, Tf - t_mean, F32(0)).astype(F32)
            hat_x = -(xf * h1) - (yf * h0); hat_y = (xf * h0) - (yf * h1)
            j0 = (gx * hat_x + gy * hat_y).astype(F64); j1 = gx.astype(F64); j2 = gy.astype(F64)
            di, dt = izm.astype(F64), tzm.astype(F64)
            tot = red([j0 * j0, j0 * j1, j0 * j2, j1 * j1, j1 * j2, j2 * j2, dt * di, j0 * di, j1 * di, j2 * di, j0 * dt, j1 * dt, j2 * dt])
            Hs = np.array([tot[0], tot[1], tot[2], tot[1], tot[3], tot[4], tot[2], tot[4], tot[5]], F64).astype(F32)
            Hinv, det = inv3(Hs)
            rec["det"] = float(det)
            corr = tot[6]
            last_rho = rho
            rho = corr / (i_norm * t_norm)
            rec["rho"] = float(rho)
            if rho != rho:
                rec["exit"] = "nan"
                return 0, it, float(rho), M
            ip, tp = tot[7:10].astype(F32), tot[10:13].astype(F32)
            iph = [_row3(Hinv, r, ip) for r in range(3)]
            lam_n = i_norm * i_norm - _dot3(ip, iph)
            lam_d = corr - _dot3(tp, iph)
            if lam_d <= 0.0:
                rec["exit"] = "lambda"
                return 0, it, float(rho), M
            lam = F32(lam_n / lam_d)
            # pass C
            e = (lam * tzm - izm).astype(F64)
            tot = red([j0 * e, j1 * e, j2 * e])
            ep = tot.astype(F32)
            dp = [_row3(Hinv, r, ep) for r in range(3)]
            theta = F64(dp[0]) + np.arcsin(F64(M[3]))
            if check_libm:
                rec["libm_ok"] = libm_margin_ok(dp[0], M[3])
            M = M.copy()
            M[2] = M[2] + dp[1]; M[5] = M[5] + dp[2]
            M[0] = M[4] = F32(np.cos(theta))
            M[3] = F32(np.sin(theta))
            M[1] = -M[3]
            rec["M"] = M.copy()
    if trace is not None:
        trace.append({"exit": "count" if it >= max_iter and abs(rho - last_rho) >= eps else "eps"})
    return 1, it, float(rho), M
