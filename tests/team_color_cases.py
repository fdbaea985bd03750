"""Constructed crops for the team-colour kernel (csrc/teams.hip, K15), one place where it can go wrong at a time (no GPU;
tests/test_gpu_teams.py runs them on the GPU, tests/test_team_cases_cpu.py checks that every case forces what its ``why`` says).

A case is a dict: name, frame_hw, frames (uint8 [n, h, w, 3] BGR), crops [(frame, x1, y1, x2, y2)], why; optional: tied (the crops have an
exact distance tie on the Lloyd path, the contract is the restatement, not scikit-learn) and refused (indices of crops the kernel must
answer with twelve zeros).  All content comes from np.random.default_rng with fixed seeds.

``replay`` restates oracle/colors.py::kmeans2_labels once more with every assignment decided in exact integer arithmetic (centres kept
as integer sum and count), which is what makes "no tie on the path" a checked condition and not a measurement:
  tie      a pixel exactly equidistant from two DIFFERENT centres at some assignment step.  With coincident centres (a flat crop, a crop
           of one pixel) both energies are the same expression of the same numbers in any arithmetic, and every implementation takes the
           first minimum: that is not a tie in this sense;
  fragile  the float64 energies of the restatement order two centres differently from the exact ones (never seen; asserted false).
Equality of kmeans2_labels with scikit-learn's labels is claimed, and tested, for tie-free crops only.

The 300-iteration cap: no crop of 2 000 pixels or fewer reaching it was found (600 seeded gradient crops of 64 .. 1 800 pixels were searched for the Lloyd
cases below; the longest run took 21 iterations, and the noise crops of the size cases reach 26), so no case claims to hit it."""
import functools
import math

import numpy as np

from oracle import colors
from oracle import prims as P

U0, U1, U2 = colors._U0, colors._U1, colors._U2
THREADS = 256                      # workgroup size of team_color_kernel; thread t owns pixels [t * chunk, (t + 1) * chunk), chunk = ceil(n / 256)
FRAME = (96, 160)
ODD_FRAME = (33, 47)               # odd width: the row stride (141 bytes) is no multiple of 4


# ---- the exact replay ------------------------------------------------------------------------------------------------------------------------
def _energies(Xf, C):
    return (C ** 2).sum(1)[None, :] - 2.0 * (Xf[:, :1] * C[None, :, 0] + Xf[:, 1:2] * C[None, :, 1] + Xf[:, 2:3] * C[None, :, 2])


def _assign(X, Xf, S, N):
    """labels for the centres S[k] / N[k] (Python integers) -> (exact labels, tie, fragile)"""
    C = np.array([[float(s) for s in S[k]] for k in range(2)]) / np.array([[float(N[0])], [float(N[1])]])
    e = _energies(Xf, C)
    lab = np.argmin(e, 1)
    coincide = [s * N[1] for s in S[0]] == [s * N[0] for s in S[1]]
    tie = fragile = False
    near = np.flatnonzero(np.abs(e[:, 1] - e[:, 0]) < 1e-6)      # float64 error of an energy is below 1e-9 (|e| < 6e5, a dozen roundings)
    if len(near):
        s0, s1 = sum(s * s for s in S[0]) * N[1] * N[1], sum(s * s for s in S[1]) * N[0] * N[0]
        seen = {}
        for i in near:
            x = tuple(int(v) for v in X[i])
            if x not in seen:
                a0 = s0 - 2 * sum(a * b for a, b in zip(x, S[0])) * N[0] * N[1] * N[1]       # (|c0|^2 - 2 x.c0) * N0^2 N1^2
                a1 = s1 - 2 * sum(a * b for a, b in zip(x, S[1])) * N[1] * N[0] * N[0]
                seen[x] = (1 if a1 < a0 else 0, a1 == a0)
            l, t = seen[x]
            tie |= t and not coincide
            if l != lab[i]:
                fragile = True
                lab[i] = l
    return lab, tie, fragile


def replay(rgb, side="left"):
    """kmeans2_labels(rgb) step by step -> dict of its intermediate values: n, i0, d0, pot, cum, vals, cands, pots, winner, labels,
    rule ("repeat" | "tol" | "cap"), iters, tied, fragile.  side="right": the seeded mistake in the candidate search (the CPU test shows that
    the case "side_left" tells the two apart; everywhere else they cannot differ)."""
    X = np.asarray(rgb).astype(np.int64).reshape(-1, 3)
    n = len(X)
    i0 = min(int(np.floor(U0 * n)), n - 1)
    d0 = ((X - X[i0]) ** 2).sum(1)
    pot = int(d0.sum())
    cum = np.cumsum(d0)
    vals = [u * pot for u in (U1, U2)]
    cands = [min(int(np.searchsorted(cum, v, side=side)), n - 1) for v in vals]
    pots = [int(np.minimum(d0, ((X - X[c]) ** 2).sum(1)).sum()) for c in cands]
    winner = 1 if pots[1] < pots[0] else 0
    S = [[int(v) for v in X[i0]], [int(v) for v in X[cands[winner]]]]
    N = [1, 1]
    Xf = X.astype(np.float64)
    mean = Xf.sum(0) / n
    tol = float(((Xf ** 2).sum(0) / n - mean * mean).sum() / 3.0 * 1e-4)
    labels, rule, tied, fragile, iters = None, "cap", False, False, 0
    for _ in range(300):
        iters += 1
        new, t, f = _assign(X, Xf, S, N)
        tied |= t; fragile |= f
        C = np.array(S, np.float64) / np.array(N, np.float64)[:, None]
        Sn, Nn = [list(S[0]), list(S[1])], list(N)
        for k in range(2):
            m = new == k
            if m.any():
                Sn[k], Nn[k] = [int(v) for v in X[m].sum(0)], int(m.sum())
        Cn = np.array(Sn, np.float64) / np.array(Nn, np.float64)[:, None]
        same = labels is not None and np.array_equal(new, labels)
        shift = float(((Cn - C) ** 2).sum())
        labels, S, N = new, Sn, Nn
        if same:
            rule = "repeat"
            break
        if shift <= tol:
            rule = "tol"
            break
    if rule != "repeat":
        labels, t, f = _assign(X, Xf, S, N)
        tied |= t; fragile |= f
    return dict(n=n, i0=i0, d0=d0, pot=pot, cum=cum, vals=vals, cands=cands, pots=pots, winner=winner, labels=labels, rule=rule, iters=iters,
                tied=bool(tied), fragile=bool(fragile))


def ties_on_path(rgb):
    return replay(rgb)["tied"]


def stop_rule(rgb):
    r = replay(rgb)
    return r["rule"], r["iters"]


def chunk_of(n):
    return (n + THREADS - 1) // THREADS


# ---- crops, frames, expectations ----------------------------------------------------------------------------------------------------------------
def crop_bgr(case, crop):
    f, x1, y1, x2, y2 = crop
    return case["frames"][f][y1:y2, x1:x2]


def crop_rgb(case, crop):
    return crop_bgr(case, crop)[..., ::-1].reshape(-1, 3)


def valid_crops(case):
    return [(k, c) for k, c in enumerate(case["crops"]) if k not in case.get("refused", ())]


def oracle_row(img, labels=None):
    """the twelve numbers of eagle_team_colors for one BGR crop, from oracle/colors.py: the eleven colours in the kernel's order (red2 merged
    into red), then the size of the player cluster"""
    if labels is None:
        labels = colors.kmeans2_labels(img[..., ::-1].reshape(-1, 3))
    labels = np.asarray(labels).reshape(img.shape[:2])
    corners = [labels[0, 0], labels[0, -1], labels[-1, 0], labels[-1, -1]]
    mask = labels == (1 if max(set(corners), key=corners.count) == 0 else 0)
    cnt = colors.color_counts(P.bgr2hsv(np.ascontiguousarray(img)), mask)
    return [cnt[c] for c in colors.COLOR_ORDER] + [int(mask.sum())]


@functools.lru_cache(maxsize=None)
def expected(name):
    """int32 [crops, 12] of a case, computed once: the oracle's rows, zeros for the refused crops"""
    case = CASES[name]
    out = np.zeros((len(case["crops"]), 12), np.int32)
    for k, c in valid_crops(case):
        out[k] = oracle_row(crop_bgr(case, c))
    out.setflags(write=False)
    return out


def _noise(seed, h, w, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w, 3), dtype=np.uint8)


def _from_rgb(rgb, h, w):
    return np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(h, w, 3)[..., ::-1])


def pack(name, why, images, frame_hw=FRAME, seed=0, **extra):
    """shelf-pack the BGR crop images into as few noise frames of frame_hw as they need, one pixel apart"""
    fh, fw = frame_hw
    frames, crops = [], []
    x = y = shelf = 0
    for img in images:
        h, w = img.shape[:2]
        assert h <= fh and w <= fw, (name, h, w)
        if x + w > fw:
            x, y, shelf = 0, y + shelf + 1, 0
        if y + h > fh or not frames:
            frames.append(_noise(1000 * seed + len(frames), fh, fw))
            x = y = shelf = 0
        frames[-1][y:y + h, x:x + w] = img
        crops.append((len(frames) - 1, x, y, x + w, y + h))
        x, shelf = x + w + 1, max(shelf, h)
    return dict(name=name, frame_hw=frame_hw, frames=np.stack(frames), crops=crops, why=why, **extra)


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------------
TINY = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (3, 5)]                                   # (h, w)
CHUNK_COUNTS = [255, 256, 257, 511, 512, 513, 767, 768, 769]
NEAR_SQUARE = {255: (15, 17), 256: (16, 16), 511: (7, 73), 512: (16, 32), 513: (19, 27), 767: (13, 59), 768: (24, 32)}
LARGE_HW = (200, 300)


def _two_populations(seed, h, w, a, b, sigma, inner=None):
    """BGR crop: colour a with normal noise, the rectangle ``inner`` (y1, y2, x1, x2; default the middle half) colour b"""
    r = np.random.default_rng(seed)
    img = np.zeros((h, w, 3)) + np.array(a, np.float64)
    y1, y2, x1, x2 = inner or (h // 4, h - h // 4, w // 4, w - w // 4)
    img[y1:y2, x1:x2] = b
    return np.clip(np.rint(img + r.normal(0, sigma, img.shape)), 0, 255).astype(np.uint8)


def _size_cases():
    out = [pack("tiny", "fewer pixels than the block has threads, down to one: most threads own nothing, centre 0 is the last pixel at n = 2",
                [_noise(100 + k, h, w) for k, (h, w) in enumerate(TINY)], seed=1)]
    out.append(pack("chunk_rows", "single-row crops of 255 .. 769 pixels: chunk 1 .. 4, with idle threads where the count is no multiple of the chunk (the frame is 800 wide "
                    "because a row of 769 pixels needs it)", [_noise(200 + n, 1, n) for n in CHUNK_COUNTS], frame_hw=(32, 800), seed=2))
    out.append(pack("chunk_blocks", "the same pixel counts as near-square crops (257 and 769 are prime and exist as rows only)",
                    [_noise(300 + n, *hw) for n, hw in NEAR_SQUARE.items()], seed=3))
    out.append(pack("thin", "one pixel wide and one pixel high: the four corners coincide in pairs", [_noise(401, 61, 1), _noise(402, 1, 97)], seed=4))
    h, w = LARGE_HW
    out.append(pack("large", "the one crop over 5 000 pixels: 60 000 pixels, chunk 235, two noisy populations",
                    [_two_populations(5, h, w, (60, 140, 70), (40, 50, 200), 14.0)], frame_hw=(208, 320), seed=5))
    return out


# ---- seeding -----------------------------------------------------------------------------------------------------------------------------------
DARK, RED, GREEN = (40, 40, 40), (200, 40, 40), (40, 200, 40)            # RGB; RED and GREEN are equally far from DARK and farther from each other
ROSE = (200, 60, 60)                                                      # close to RED
SEED_HW = (30, 30)                                                        # 900 pixels: chunk 4, 225 non-empty chunks, centre 0 is pixel 493


def _placed(hw, placed, base=DARK):
    h, w = hw
    rgb = np.zeros((h * w, 3), np.uint8) + np.array(base, np.uint8)
    for i, c in placed:
        rgb[i] = c
    return _from_rgb(rgb, h, w)


def _ten(j2, j1, before, after, major, minor, minor_at):
    """ten odd pixels on a flat crop: six at ``before``, the 7th at j2 (where the quantile u2 lands: candidate 1), the 8th at j1 (u1: candidate 0),
    two at ``after``; all of colour ``major`` except the one at ``minor_at``"""
    idx = list(before) + [j2, j1] + list(after)
    assert len(idx) == 10 and idx == sorted(idx)
    return _placed(SEED_HW, [(i, minor if i == minor_at else major) for i in idx])


def _seed_cases():
    b6, a2 = (10, 101, 202, 303, 404, 550), (880, 890)
    imgs = [
        ("first_of_chunk", _ten(600, 704, b6, a2, RED, ROSE, 600)),                          # 600 % 4 == 704 % 4 == 0
        ("last_of_chunk", _ten(603, 707, b6, a2, RED, ROSE, 707)),                           # % 4 == 3
        ("last_chunk", _placed(SEED_HW, [(20, RED), (897, ROSE), (899, RED)])),              # three nearly equal weights: u2 -> the 2nd, u1 -> the 3rd, chunk 224
        ("cand0_wins", _ten(601, 706, b6, a2, RED, ROSE, 601)),                              # candidate 0 is of the majority colour
        ("cand1_wins", _ten(601, 706, b6, a2, RED, ROSE, 706)),                              # candidate 1 is
        ("equal_pots", _placed(SEED_HW, [(i, RED if k in (0, 2, 4, 7, 9) else GREEN) for k, i in enumerate(b6 + (601, 706) + a2)])),
        ("flat", _placed((9, 7), [])),
        ("odd_before_seed", _placed((9, 7), [(5, RED)])),
        ("odd_at_seed", _placed((9, 7), [(34, RED)])),
        ("odd_after_seed", _placed((9, 7), [(50, RED)])),
        ("odd_after_seed_900", _placed(SEED_HW, [(899, RED)])),
        ("side_left", _side_left_crop()),
    ]
    case = pack("seeding", "the candidate search of the k-means++ seeding: chunk edges, either candidate winning, equal potentials, pot == 0, one odd pixel, and the one crop where searchsorted's side decides",
                [i for _, i in imgs], seed=6)
    case["labels"] = [n for n, _ in imgs]
    return [case]


# the one place where searchsorted's side matters: cum[j] == u1 * pot exactly.  u * pot is a float64 product, so this needs a potential for which the
# product is an integer: 448 315 870 is one of nine such values between 3e8 and 5e8 (none exists below 1e8, where a crop of a few hundred
# pixels lives).  The crop reaches exactly that potential and has cum[j] == u1 * pot at a white pixel j, followed by background and then a grey pixel.
SIDE_POT = 448315870
SIDE_HW = (70, 70)
BLACK, GREY, WHITE = (0, 0, 0), (120, 120, 120), (255, 255, 255)          # seed colour, d0 = 43 200, d0 = 195 075
SIDE_PLATEAU = 5


def _four_squares(r):
    for a in range(math.isqrt(r), -1, -1):
        for b in range(math.isqrt(r - a * a), -1, -1):
            for c in range(math.isqrt(r - a * a - b * b), -1, -1):
                d = math.isqrt(r - a * a - b * b - c * c)
                if a * a + b * b + c * c + d * d == r:
                    return [(a, b, 0), (c, d, 0)]


def _run(total, whites):
    """pixels whose squared distances to black sum to ``total``: two dark ones for the remainder, greys, then ``whites`` white ones"""
    rest = total - 195075 * whites
    greys, r = divmod(rest, 43200)
    return _four_squares(r) + [GREY] * greys + [WHITE] * whites


def _side_left_crop():
    h, w = SIDE_HW
    n = h * w
    k = U1 * SIDE_POT
    assert k == int(k)
    k = int(k)
    whites = round(SIDE_POT / 281475)                                     # twice as many greys as whites
    first = _run(k, round(0.6 * whites))
    second = _run(SIDE_POT - k, whites - round(0.6 * whites))
    i0 = min(int(np.floor(U0 * n)), n - 1)
    rgb, i = np.zeros((n, 3), np.uint8), 0
    for px in first + [BLACK] * SIDE_PLATEAU + second[2:] + second[:2]:    # the grey pixels of the second run follow the plateau
        if i == i0:
            i += 1                                                         # centre 0 stays black
        rgb[i] = px
        i += 1
    return _from_rgb(rgb, h, w)


# ---- Lloyd -------------------------------------------------------------------------------------------------------------------------------------
def _gradient(seed, h, w, frac, sigma):
    """a colour gradient along the pixel index plus normal noise, with a small second population scattered into it"""
    r = np.random.default_rng(seed)
    n = h * w
    a, b = r.integers(0, 256, 3), r.integers(0, 256, 3)
    img = a + (b - a) * np.linspace(0, 1, n)[:, None]
    k = r.random(n) < frac
    img[k] = r.integers(0, 256, 3)
    return _from_rgb(np.clip(np.rint(img + r.normal(0, sigma, (n, 3))), 0, 255), h, w)


LLOYD = [  # (seed, h, w, frac, sigma), found by a seeded search over these parameters -> the stop rule and iteration count the CPU test asserts
    ((93, 18, 40, 0.1, 15.0), ("repeat", 21)), ((158, 23, 18, 0.3, 30.0), ("repeat", 20)), ((501, 14, 23, 0.1, 15.0), ("repeat", 15)),
    ((459, 24, 33, 0.02, 30.0), ("tol", 20)), ((175, 15, 38, 0.02, 30.0), ("tol", 19)), ((262, 23, 25, 0.1, 15.0), ("tol", 12))]


def _lloyd_cases():
    return [pack("lloyd", "Lloyd runs that stop by label repetition and by the tolerance rule, short and of 8 or more iterations",
                 [_gradient(*p) for p, _ in LLOYD], seed=7)]


# ---- corner vote -------------------------------------------------------------------------------------------------------------------------------
VOTES = {"4-0 label 0": "AAAA", "4-0 label 1": "BBBB", "3-1 label 0": "AABA", "3-1 label 1": "BABB", "2-2": "ABBA"}
VOTE_A, VOTE_B = (70, 150, 60), (30, 40, 210)          # BGR: grass-like background, red figure


def _vote_cases():
    """one picture (centre 0, pixel floor(u0 n), lies on the background A: label 0 is the background cluster) with the four corner pixels set
    to A or B"""
    h, w = 24, 18
    base = _two_populations(8, h, w, VOTE_A, VOTE_B, 6.0, inner=(2, 12, 4, 14))
    imgs = []
    for pat in VOTES.values():
        img = base.copy()
        for (y, x), ch in zip(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)), pat):
            img[y, x] = VOTE_A if ch == "A" else VOTE_B
        imgs.append(img)
    case = pack("corner_vote", "the same picture with the corners voting 4-0, 3-1 each way and 2-2 (background 0 wins); with 4-0 for label 1 the player cluster is label 0",
                imgs, seed=8)
    case["labels"] = list(VOTES)
    return [case]


# ---- colour ranges -----------------------------------------------------------------------------------------------------------------------------
HUES = [0, 10, 11, 25, 26, 35, 36, 85, 86, 95, 96, 125, 126, 145, 146, 159, 160, 179]
SATS = [29, 30, 31, 99, 100, 101]
VALS = [49, 50, 51, 99, 100, 101, 199, 200, 201]
_TABLE_V = (255, 230, 201, 200, 199, 150, 120, 101, 100, 99, 51, 50, 49, 20)


@functools.lru_cache(maxsize=None)
def hsv_table():
    """BGR values with their HSV (oracle.prims.bgr2hsv): every (min, mid) under each maximum of _TABLE_V, in all six channel orders"""
    rows = []
    for v in _TABLE_V:
        mn, md = np.meshgrid(np.arange(v + 1), np.arange(v + 1), indexing="ij")
        k = md >= mn
        t = np.stack([np.full(k.sum(), v), md[k], mn[k]], 1)
        rows += [t[:, p] for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))]
    bgr = np.unique(np.concatenate(rows).astype(np.uint8), axis=0)
    return bgr, P.bgr2hsv(bgr.reshape(-1, 1, 3)).reshape(-1, 3)


def hue_before_wrap(bgr):
    """the hue numerator's sign as cv2's integer path has it: negative where the maximum is red and green < blue"""
    b, g, r = (np.asarray(bgr)[..., k].astype(np.int64) for k in range(3))
    v = np.maximum(np.maximum(b, g), r)
    return np.where(v == r, g - b, 1)


def _pick(r, k, h=None, s=None, v=None, extra=None):
    """k table entries with h, s, v inside the given inclusive (lo, hi)"""
    bgr, hsv = hsv_table()
    m = np.ones(len(bgr), bool)
    for ch, rng_ in enumerate((h, s, v)):
        if rng_ is not None:
            m &= (hsv[:, ch] >= rng_[0]) & (hsv[:, ch] <= rng_[1])
    if extra is not None:
        m &= extra(bgr)
    idx = np.flatnonzero(m)
    assert len(idx), (h, s, v)
    return bgr[r.choice(idx, k)]


def _framed(r, interior, border_lo, border_hi, side=8, rim=2):
    """a noisy border of one colour range around an interior of side x side swept values (the list is cycled)"""
    n = side + 2 * rim
    img = r.integers(border_lo, border_hi, (n, n, 3)).astype(np.uint8)
    pix = np.concatenate(interior)
    img[rim:rim + side, rim:rim + side] = pix[np.arange(side * side) % len(pix)].reshape(side, side, 3)
    return img


def _colour_cases():
    r = np.random.default_rng(9)
    bright = dict(s=(160, 255), v=(200, 255))
    dark, light = (0, 31), (215, 256)
    imgs, labels = [], []
    for a, b in ((10, 11), (25, 26), (35, 36), (85, 86), (95, 96), (125, 126), (145, 146), (159, 160), (179, 0)):
        imgs.append(_framed(r, [_pick(r, 8, h=(x, x), **bright) for x in (a, b)] * 4, *dark)); labels.append(f"hue {a}|{b}")
    imgs.append(_framed(r, [_pick(r, 10, h=(100, 120), s=(x, x), v=(200, 255)) for x in (99, 100, 101)], *dark)); labels.append("sat 99..101")
    imgs.append(_framed(r, [_pick(r, 10, s=(x, x), v=(220, 255)) for x in (29, 30, 31)], *dark)); labels.append("sat 29..31 white")
    imgs.append(_framed(r, [_pick(r, 10, s=(x, x), v=(120, 150)) for x in (29, 30, 31)], *dark)); labels.append("sat 29..31 gray")
    imgs.append(_framed(r, [_pick(r, 10, h=(100, 120), s=(200, 255), v=(x, x)) for x in (99, 100, 101)], *light)); labels.append("val 99..101")
    imgs.append(_framed(r, [_pick(r, 10, s=(0, 30), v=(x, x)) for x in (49, 50, 51)], *light)); labels.append("val 49..51 gray|black")
    imgs.append(_framed(r, [_pick(r, 10, s=(120, 255), v=(x, x)) for x in (49, 50, 51)], *light)); labels.append("val 49..51 black only")
    imgs.append(_framed(r, [_pick(r, 10, s=(0, 30), v=(x, x)) for x in (199, 200, 201)], *dark)); labels.append("val 199..201 white|gray")
    grey = lambda lo, hi: np.repeat(r.integers(lo, hi, (40, 1)), 3, 1).astype(np.uint8)
    imgs.append(_framed(r, [grey(0, 56)], *light)); labels.append("pure grey, dark")
    imgs.append(_framed(r, [grey(195, 256)], *dark)); labels.append("pure grey, light")
    for name, ch in (("red = green", (2, 1)), ("green = blue", (1, 0)), ("red = blue", (2, 0))):
        tie = lambda bgr, ch=ch: (bgr[:, ch[0]] == bgr[:, ch[1]]) & (bgr[:, ch[0]] == bgr.max(1))
        imgs.append(_framed(r, [_pick(r, 40, extra=tie, **bright)], *dark)); labels.append("two maxima: " + name)
    case = pack("colour_ranges", "a noisy border around interiors that sweep every hue, S and V bound of the twelve ranges, pure greys, tied maxima, negative hues",
                imgs, seed=9)
    case["labels"] = labels
    return [case]


# ---- placement, refused crops ------------------------------------------------------------------------------------------------------------------
def _figure_frames(seed, n, hw, boxes):
    """noise-textured grass frames with a noisy red or blue figure in the middle of each box (frame, x1, y1, x2, y2)"""
    r = np.random.default_rng(seed)
    fh, fw = hw
    frames = np.clip(np.array((60, 140, 70)) + r.normal(0, 9, (n, fh, fw, 3)), 0, 255).astype(np.uint8)
    for k, (f, x1, y1, x2, y2) in enumerate(boxes):
        w, h = x2 - x1, y2 - y1
        kit = np.array((35, 40, 205) if k % 2 else (200, 60, 30))
        ys, xs = slice(y1 + h // 4, y2 - h // 4), slice(x1 + w // 4, x2 - w // 4)
        frames[f, ys, xs] = np.clip(kit + r.normal(0, 9, frames[f, ys, xs].shape), 0, 255).astype(np.uint8)
    return frames


def _placement_cases():
    fh, fw = FRAME
    boxes = [(0, 0, 0, 14, 22), (0, fw - 15, 30, fw, 55), (0, 40, fh - 21, 53, fh), (1, fw - 13, fh - 19, fw, fh), (1, 0, fh - 9, 11, fh), (1, fw - 9, 0, fw, 10)]
    out = [dict(name="placement", frame_hw=FRAME, frames=_figure_frames(10, 2, FRAME, boxes), crops=boxes,
                why="crops that start at (0, 0), end at x2 == frame_w or y2 == frame_h, and the bottom-right corner of the last frame")]
    oh, ow = ODD_FRAME
    boxes = [(0, 0, 0, 9, 12), (1, ow - 11, oh - 13, ow, oh), (1, 0, 0, ow, oh), (0, ow - 7, 3, ow, 18), (1, 5, oh - 8, 20, oh), (0, 13, 2, 14, 31), (0, 3, 20, 40, 21)]
    out.append(dict(name="odd_frame", frame_hw=ODD_FRAME, frames=_figure_frames(11, 2, ODD_FRAME, boxes), crops=boxes,
                    why="a 33 x 47 frame (row stride 141 bytes): corner crops, the whole last frame, a column and a row"))
    return out


def _refused_case():
    fh, fw = FRAME
    good = [(0, 4, 4, 18, 26), (1, 30, 10, 44, 30), (0, 60, 40, 75, 62), (1, 100, 50, 112, 70), (0, 120, 5, 135, 30)]
    bad = {"x2 <= x1": (0, 30, 10, 30, 30), "x2 < x1": (0, 31, 10, 30, 30), "y2 <= y1": (0, 10, 40, 25, 40), "y2 < y1": (0, 10, 41, 25, 40),
           "x1 < 0": (0, -1, 0, 12, 12), "y1 < 0": (1, 0, -1, 12, 12), "x2 > frame_w": (1, fw - 10, 0, fw + 1, 12), "y2 > frame_h": (0, 0, fh - 10, 12, fh + 1),
           "frame < 0": (-1, 4, 4, 18, 26), "frame >= n_frames": (2, 4, 4, 18, 26)}
    crops, refused, labels = [], [], []
    names = list(bad)
    for k in range(len(bad) + len(good)):                 # refused crops sit between the valid ones: refused ones double up towards the end
        if k % 3 == 0 and k // 3 < len(good):
            crops.append(good[k // 3]); labels.append("valid")
        else:
            refused.append(len(crops)); labels.append(names[0]); crops.append(bad[names.pop(0)])
    return [dict(name="refused", frame_hw=FRAME, frames=_figure_frames(12, 2, FRAME, good), crops=crops, refused=tuple(refused), labels=labels,
                 why="every rectangle the kernel refuses, between valid crops of one call: twelve zeros each, the neighbours' rows undisturbed")]


# ---- tied ----------------------------------------------------------------------------------------------------------------------------------------
def few_levels(seed):
    """the seeded few-level input of the tie search: a crop of 1..20 x 1..20 pixels (2 .. 399 pixels in all), 2..5 levels per channel spread over
    0..255 by a factor drawn per input -> BGR crop"""
    r = np.random.default_rng(seed)
    while True:
        h, w = int(r.integers(1, 21)), int(r.integers(1, 21))
        if 2 <= h * w <= 399:
            break
    levels = r.integers(2, 6, 3)
    spread = float(r.uniform(1.0, 255.0 / 4))
    rgb = np.stack([np.minimum(np.rint(r.integers(0, levels[c], h * w) * spread), 255) for c in range(3)], 1)
    return _from_rgb(rgb, h, w)


TIE_SEARCH = 400                   # seeds 0 .. 399 of few_levels are searched by the CPU test
TIED_SEEDS = [2, 35, 62, 99, 141, 179, 262, 302]                   # among them: ties_on_path and scikit-learn 1.7.2's partition differs from the restatement's


def _tied_case():
    return [pack("tied", "few-level crops with an exact distance tie on the Lloyd path where scikit-learn's labels differ: the contract is the restatement (ties to cluster 0)",
                 [few_levels(s) for s in TIED_SEEDS], seed=13, tied=True)]


# ---- the host mapping (eagle_amd/teams.py::get_team_mapping against oracle/colors.py::get_team_mapping) ------------------------------------------
KIT = {"red": (35, 40, 205), "blue": (200, 60, 30), "yellow": (30, 205, 205), "dull": (120, 120, 160)}       # BGR; dull lies in no colour range (S 64, V 160)
BIG = 1200                                                                   # area of the 30 x 40 boxes of the overlap pairs
UNDER, OVER = (19, 22), (17, 25)                                             # overlaps of 418 / 1200 = 0.3483 (kept) and 425 / 1200 = 0.3542 (dropped)


def _kit_frames(seed, n, hw, items):
    """grass frames with uniform noise of +-4; per item (frame, box, kit) the middle half of the box in the kit colour, noise +-4"""
    r = np.random.default_rng(seed)
    fh, fw = hw
    frames = (np.array((60, 140, 70)) + r.integers(-4, 5, (n, fh, fw, 3))).astype(np.uint8)
    for f, (x1, y1, x2, y2), kit in items:
        w, h = x2 - x1, y2 - y1
        ys, xs = slice(y1 + h // 4, y2 - h // 4), slice(x1 + w // 4, x2 - w // 4)
        frames[f, ys, xs] = (np.array(KIT[kit]) + r.integers(-4, 5, frames[f, ys, xs].shape)).astype(np.uint8)
    return frames


def _coords(n, items):
    coords = {i: {"Coordinates": {"Player": {}, "Goalkeeper": {}}, "Time": "00:00", "Keypoints": {}, "Boundaries": [None] * 4} for i in range(n)}
    for f, pid, box in items:
        coords[f]["Coordinates"]["Player"][pid] = {"BBox": list(box), "Confidence": 0.9, "Transformed_Coordinates": None}
    return coords


def _small(x, y):
    return (x, y, x + 12, y + 20)


def _mapping(name, why, seed, n_frames, n_coords, items, hw=FRAME, **extra):
    """items: (frame, player id, box, kit); frames beyond n_frames exist in coords only"""
    return dict(name=name, why=why, frame_hw=hw, n_frames=n_frames, coords=_coords(n_coords, [(f, p, b) for f, p, b, _ in items]),
                frames=_kit_frames(seed, n_frames, hw, [(f, b, k) for f, _, b, k in items if f < n_frames and k is not None]), **extra)


def _mapping_cases():
    (uw, uh), (ow, oh) = UNDER, OVER
    main = [
        # frame 0: two of each team, the pair that overlaps by just under 35 % (3 and 4, both kept with weight 1 - 418 / 1200), the outlier 7 in yellow
        (0, 1, _small(2, 2), "red"), (0, 2, _small(18, 2), "red"), (0, 11, _small(34, 2), "blue"), (0, 12, _small(50, 2), "blue"),
        (0, 3, (70, 2, 100, 42), "red"), (0, 4, (100 - uw, 42 - uh, 130 - uw, 82 - uh), "red"), (0, 7, _small(140, 2), "yellow"),
        # frame 1: the same players elsewhere; 4 alone and in blue (its weight 1 beats the 0.652 of its red crop); 6 and 8 overlap by just over 35 %: dropped
        (1, 1, _small(20, 60), "red"), (1, 2, _small(2, 60), "red"), (1, 11, _small(50, 60), "blue"), (1, 12, _small(34, 60), "blue"),
        (1, 3, _small(70, 60), "red"), (1, 4, _small(90, 60), "blue"), (1, 7, _small(140, 60), "yellow"),
        (1, 6, (70, 2, 100, 42), "blue"), (1, 8, (100 - ow, 42 - oh, 130 - ow, 82 - oh), "blue"),
        # frame 2: nobody.  frame 3: 6 and 8 apart, the outlier 7 in red
        (3, 6, _small(2, 30), "blue"), (3, 8, _small(30, 30), "blue"), (3, 7, _small(60, 30), "red"),
        # coords entry 4 lies beyond the clip: player 99 must not be mapped
        (4, 99, _small(2, 2), None), (4, 1, _small(30, 2), None),
    ]
    out = [_mapping("two_teams", "overlaps just under and just over 35 %, a fractional weight that decides player 4, the outlier 7 (yellow twice, red once), "
                    "players seen in several frames, a frame without players, coords longer than the clip", 20, 4, 5, main)]
    out.append(_mapping("one_team", "a clip with one team only: everybody is team 0", 21, 2, 2,
                        [(0, 1, _small(2, 2), "red"), (0, 2, _small(30, 2), "red"), (1, 1, _small(40, 50), "red"), (1, 3, _small(90, 50), "red")]))
    pair = [(0, 1, _small(2, 2), "red"), (0, 2, _small(30, 2), "blue"), (0, 5, _small(120, 2), "red")]
    out.append(_mapping("zero_area", "a box of zero area: the reference divides by zero (proc.py:423), the library skips the box", 22, 1, 1,
                        pair + [(0, 3, (60, 10, 60, 30), None), (0, 4, (80, 40, 95, 40), None)], skipped=(3, 4), raises=ZeroDivisionError))
    out.append(_mapping("no_colour", "a player whose crop hits no colour range: the reference takes max() of an empty dict (proc.py:447), the library leaves the player out",
                        23, 1, 1, pair + [(0, 3, _small(60, 2), "dull")], skipped=(3,), raises=ValueError))
    return {c["name"]: c for c in out}


def without(coords, pids):
    """coords without the players ``pids``"""
    return {i: dict(e, Coordinates=dict(e["Coordinates"], Player={p: v for p, v in e["Coordinates"]["Player"].items() if p not in pids})) for i, e in coords.items()}




def _build():
    cases = _size_cases() + _seed_cases() + _lloyd_cases() + _vote_cases() + _colour_cases() + _placement_cases() + _refused_case() + _tied_case()
    return {c["name"]: c for c in cases}


CASES = _build()
MAPPINGS = _mapping_cases()
