"""The written definition of the shots stage (K31; include/eagle.h, eagle_op_shots): a clip of dense BGR frames -> per frame a colour signature, per
frame pair a score, and from the scores the flashes, hard cuts, gradual transitions and the list of shots.  Stated twice: `shots` in array operations
(np.bincount), `shots_scalar` as plain loops over pixels, frames and a row-by-row scan.  Everything behind the pixel read is integer arithmetic, so
the two statements, and the library, agree bit for bit.  The thresholds are conventional choices, not fitted to footage.

  signature of a frame [h, w, 3] (h, w >= 4, P = h * w), 1537 u32:
    hist [512]      pixels per bin (b >> 5) * 64 + (g >> 5) * 8 + (r >> 5)
    tile [16][64]   a 4 x 4 grid of tiles of th = h // 4 rows and tw = w // 4 columns over the top-left 4 th x 4 tw pixels; tile ty * 4 + tx counts the
                    bins (b >> 6) * 16 + (g >> 6) * 4 + (r >> 6).  The up to 3 remaining rows and columns count in hist and grass only.  A = th * tw
    grass           pixels with g >= 48 and g - max(r, b) >= 16
  score of a pair (a, b), in 1 / 65536:
    sg = 65536 * sum |hist_a - hist_b| // (2 P)
    st = 65536 * u // (16 A), u the sum of the 8 smallest of the 16 tile distances sum_64 |tile_a[t] - tile_b[t]|
    S  = max(sg, st)
  per frame i: d1 = S(i-1, i), d2 = S(i-2, i), dW = S(i-W, i) (0 where the earlier frame does not exist), sg and st of the d1 pair, grass
  decisions (cut, low, grass_thr in 1 / 65536; window W >= 2; min_len >= 1):
    flash f          f >= 1, d1[f] >= cut, f + 1 < n, d2[f+1] < low
    hard cut i       i >= 1, d1[i] >= cut, neither i nor i - 1 a flash
    eligible i       i >= W, dW[i] >= cut, no hard cut in [i-W+1, i], neither i nor i - W a flash
    gradual end i    eligible, dW[i] > dW[j] for the eligible j of [i-W+1, i-1] and dW[i] >= dW[j] for the eligible j of [i+1, i+W-1]; the frames
                     [i-W+1, i-1] are then IN_TRANSITION
    shots            the runs between boundaries: frame 0, a hard cut, a transition's first frame, a gradual end.  kind: TRANSITION, else
                     AFTER_TRANSITION at a gradual end, else AFTER_CUT, else START.  pitch: kind != TRANSITION and grass_sum * 65536 >= grass_thr * P * count;
                     short: count < min_len; usable: pitch and not short
"""
import numpy as np

SIG = 1537
START, AFTER_CUT, AFTER_TRANSITION, TRANSITION = 0, 1, 2, 3
FLASH, HARD, GRADUAL_END, IN_TRANSITION = 1, 2, 4, 8
PITCH, SHORT, USABLE = 1, 2, 4
FRAME_DTYPE = np.dtype([("d1", "<i4"), ("d2", "<i4"), ("dW", "<i4"), ("sg", "<i4"), ("st", "<i4"), ("grass", "<u4"), ("flags", "<i4"), ("reserved", "<i4")])
SHOT_DTYPE = np.dtype([("first", "<i4"), ("count", "<i4"), ("kind", "<i4"), ("flags", "<i4"), ("grass_sum", "<i8"), ("reserved", "<i4", 2)])
ONE = 65536


def default_params(fps):
    """cut 0.30, low 0.10, grass_thr 0.35 (rounded to 1 / 65536), W = max(2, round(0.4 fps)) with halves up, min_len = fps"""
    fps = int(fps)
    if fps < 1:
        raise ValueError(f"fps {fps} must be at least 1")
    return {"cut": (30 * ONE + 50) // 100, "low": (10 * ONE + 50) // 100, "grass_thr": (35 * ONE + 50) // 100, "window": max(2, (4 * fps + 5) // 10), "min_len": fps}


def check(p, n, h, w):
    for k in ("cut", "low", "grass_thr"):
        if not 0 <= p[k] <= ONE:
            raise ValueError(f"{k} {p[k]} lies outside 0 .. 65536")
    if p["low"] > p["cut"]:
        raise ValueError(f"low {p['low']} is above cut {p['cut']}")
    if p["window"] < 2:
        raise ValueError(f"window {p['window']} must be at least 2")
    if p["min_len"] < 1:
        raise ValueError(f"min_len {p['min_len']} must be at least 1")
    if n < 0:
        raise ValueError(f"n {n} is negative")
    if h < 4 or w < 4:
        raise ValueError(f"frames of {h} x {w} are below 4 x 4")


# ---- in array operations ---------------------------------------------------------------------------------------------------------------------
def signature(frame):
    f = np.asarray(frame)
    h, w = f.shape[:2]
    b, g, r = (f[..., k].astype(np.int64) for k in range(3))
    out = np.zeros(SIG, np.uint32)
    out[:512] = np.bincount(((b >> 5) * 64 + (g >> 5) * 8 + (r >> 5)).ravel(), minlength=512)
    th, tw = h // 4, w // 4
    small = ((b >> 6) * 16 + (g >> 6) * 4 + (r >> 6))[:4 * th, :4 * tw].reshape(4, th, 4, tw).transpose(0, 2, 1, 3).reshape(16, th * tw)
    out[512:1536] = np.bincount((np.arange(16)[:, None] * 64 + small).ravel(), minlength=1024)
    out[1536] = int(((g >= 48) & (g - np.maximum(r, b) >= 16)).sum())
    return out


def signatures(frames):
    return np.stack([signature(f) for f in frames]) if len(frames) else np.zeros((0, SIG), np.uint32)


def pair_scores(sa, sb, P, A):
    """(sg, st) of signature rows [..., 1537] against each other"""
    a, b = sa.astype(np.int64), sb.astype(np.int64)
    sg = ONE * np.abs(a[..., :512] - b[..., :512]).sum(-1) // (2 * P)
    t = np.abs(a[..., 512:1536] - b[..., 512:1536]).reshape(a.shape[:-1] + (16, 64)).sum(-1)
    st = ONE * np.sort(t, -1)[..., :8].sum(-1) // (16 * A)
    return sg, st


def distances(sig, P, A, W):
    n = len(sig)
    out = np.zeros(n, FRAME_DTYPE)
    out["grass"] = sig[:, 1536]
    for name, lag in (("d1", 1), ("d2", 2), ("dW", W)):
        if n > lag:
            sg, st = pair_scores(sig[:-lag], sig[lag:], P, A)
            out[name][lag:] = np.maximum(sg, st)
            if lag == 1:
                out["sg"][1:], out["st"][1:] = sg, st
    return out


def _shift(a, k):
    """a[i - k] at i (False / 0 where it does not exist); k may be negative"""
    out = np.zeros_like(a)
    n = len(a)
    if 0 <= k < n:
        out[k:] = a[:n - k]
    elif -n < k < 0:
        out[:n + k] = a[-k:]
    return out


def decide(rows, P, p):
    """sets rows["flags"] and returns the shots"""
    n = len(rows)
    cut, low, W = p["cut"], p["low"], p["window"]
    d1, d2, dW = (rows[k].astype(np.int64) for k in ("d1", "d2", "dW"))
    idx = np.arange(n)
    flash = (idx >= 1) & (d1 >= cut) & (idx + 1 < n) & (_shift(d2, -1) < low)
    hard = (idx >= 1) & (d1 >= cut) & ~flash & ~_shift(flash, 1)
    csum = np.concatenate([[0], np.cumsum(hard)])
    in_window = csum[idx + 1] - csum[np.maximum(idx - W + 1, 0)]          # hard cuts in [i-W+1, i]
    elig = (idx >= W) & (dW >= cut) & (in_window == 0) & ~flash & ~_shift(flash, W)
    gend = elig.copy()
    for k in range(1, W):
        gend &= ~(_shift(elig, k) & (_shift(dW, k) >= dW))               # an earlier eligible frame at least as great
        gend &= ~(_shift(elig, -k) & (_shift(dW, -k) > dW))              # a later eligible frame greater
    intr = np.zeros(n, bool)
    tstart = np.zeros(n, bool)
    for k in range(1, W):
        intr |= _shift(gend, -k)
    tstart = _shift(gend, -(W - 1))
    rows["flags"] = flash * FLASH + hard * HARD + gend * GRADUAL_END + intr * IN_TRANSITION
    bound = hard | gend | tstart
    if n:
        bound[0] = True
    first = np.flatnonzero(bound)
    shots = np.zeros(len(first), SHOT_DTYPE)
    if not n:
        return shots
    count = np.diff(np.concatenate([first, [n]]))
    kind = np.where(tstart[first], TRANSITION, np.where(gend[first], AFTER_TRANSITION, np.where(hard[first], AFTER_CUT, START)))
    gcum = np.concatenate([[0], np.cumsum(rows["grass"].astype(np.int64))])
    gsum = gcum[first + count] - gcum[first]
    pitch = np.array([k != TRANSITION and int(g) * ONE >= p["grass_thr"] * P * int(c) for k, g, c in zip(kind, gsum, count)], bool)
    short = count < p["min_len"]
    shots["first"], shots["count"], shots["kind"], shots["grass_sum"] = first, count, kind, gsum
    shots["flags"] = pitch * PITCH + short * SHORT + (pitch & ~short) * USABLE
    return shots


def shots(frames, p):
    """frames uint8 [n, h, w, 3] -> (signatures u32 [n, 1537], rows FRAME_DTYPE [n], shots SHOT_DTYPE [m])"""
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    check(p, n, h, w)
    sig = signatures(frames)
    rows = distances(sig, h * w, (h // 4) * (w // 4), p["window"])
    return sig, rows, decide(rows, h * w, p)


# ---- as plain loops ------------------------------------------------------------------------------------------------------------------------------
def signature_scalar(frame):
    h, w = len(frame), len(frame[0])
    th, tw = h // 4, w // 4
    out = [0] * SIG
    for y in range(h):
        row = frame[y]
        for x in range(w):
            b, g, r = row[x]
            out[(b >> 5) * 64 + (g >> 5) * 8 + (r >> 5)] += 1
            if y < 4 * th and x < 4 * tw:
                out[512 + ((y // th) * 4 + x // tw) * 64 + (b >> 6) * 16 + (g >> 6) * 4 + (r >> 6)] += 1
            if g >= 48 and g - max(r, b) >= 16:
                out[1536] += 1
    return out


def score_scalar(a, b, P, A):
    sg = ONE * sum(abs(a[k] - b[k]) for k in range(512)) // (2 * P)
    tiles = sorted(sum(abs(a[512 + t * 64 + k] - b[512 + t * 64 + k]) for k in range(64)) for t in range(16))
    return sg, ONE * sum(tiles[:8]) // (16 * A)


def shots_scalar(frames, p):
    frames = np.asarray(frames)
    n, h, w = frames.shape[:3]
    check(p, n, h, w)
    cut, low, W, P, A = p["cut"], p["low"], p["window"], h * w, (h // 4) * (w // 4)
    sig = [signature_scalar(f.tolist()) for f in frames]
    rec = [dict(d1=0, d2=0, dW=0, sg=0, st=0, grass=sig[i][1536], flags=0) for i in range(n)]
    for i in range(n):
        for name, lag in (("d1", 1), ("d2", 2), ("dW", W)):
            if i - lag >= 0:
                sg, st = score_scalar(sig[i - lag], sig[i], P, A)
                rec[i][name] = max(sg, st)
                if lag == 1:
                    rec[i]["sg"], rec[i]["st"] = sg, st
    flash = [i >= 1 and rec[i]["d1"] >= cut and i + 1 < n and rec[i + 1]["d2"] < low for i in range(n)]
    hard = [i >= 1 and rec[i]["d1"] >= cut and not flash[i] and not flash[i - 1] for i in range(n)]
    elig = [i >= W and rec[i]["dW"] >= cut and not any(hard[i - W + 1:i + 1]) and not flash[i] and not flash[i - W] for i in range(n)]
    kinds = {0: START} if n else {}
    for i in range(n):
        if hard[i]:
            rec[i]["flags"] |= HARD
            kinds[i] = AFTER_CUT
        if flash[i]:
            rec[i]["flags"] |= FLASH
    for i in range(n):                                                   # the scan: a frame is an end when no eligible neighbour beats it
        if not elig[i]:
            continue
        v = rec[i]["dW"]
        if any(elig[j] and rec[j]["dW"] >= v for j in range(max(i - W + 1, 0), i)) or any(elig[j] and rec[j]["dW"] > v for j in range(i + 1, min(i + W, n))):
            continue
        rec[i]["flags"] |= GRADUAL_END
        kinds[i] = AFTER_TRANSITION
        for j in range(i - W + 1, i):
            rec[j]["flags"] |= IN_TRANSITION
        kinds[i - W + 1] = TRANSITION
    firsts = sorted(kinds)
    out = np.zeros(len(firsts), SHOT_DTYPE)
    for s, first in enumerate(firsts):
        count = (firsts[s + 1] if s + 1 < len(firsts) else n) - first
        gsum = sum(rec[i]["grass"] for i in range(first, first + count))
        pitch = kinds[first] != TRANSITION and gsum * ONE >= p["grass_thr"] * P * count
        short = count < p["min_len"]
        out[s] = (first, count, kinds[first], PITCH * pitch + SHORT * short + USABLE * (pitch and not short), gsum, (0, 0))
    rows = np.zeros(n, FRAME_DTYPE)
    for i in range(n):
        rows[i] = tuple(rec[i][k] for k in ("d1", "d2", "dW", "sg", "st", "grass", "flags")) + (0,)
    return np.array(sig, np.uint32).reshape(n, SIG), rows, out
