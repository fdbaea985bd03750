"""Constructed clips for the shots stage (tests/shots_ref.py), each named after what it forces; `check` asserts it on the reference's result.  Most are
tiny, so the plain-loop statement of the reference stays fast.  A "dissolve" here replaces a growing share of the pixels, k / (L + 1) in mixed frame
k of L, spread evenly over the tiles: both scores are then linear in k.  Its steps score 1 / (L + 1) each, so the dissolves of one and two frames
run with cut = 0.6: at the default 0.30 their steps are hard cuts (back to back, leaving short shots), which is what a cut detector should say of a
change of half the picture from one frame to the next."""
import functools

import numpy as np

import shots_ref as SR

ONE = 65536
GRASS, GRASS2, CROWD, RED, WHITE, BLACK = (40, 140, 50), (0, 255, 0), (60, 60, 200), (0, 0, 255), (255, 255, 255), (0, 0, 0)      # b, g, r
BASE = {"cut": 19661, "low": 6554, "grass_thr": 22938, "window": 4, "min_len": 3}
CASES = []


def P(**kw):
    return dict(BASE, **kw)


def solid(h, w, colour):
    return np.broadcast_to(np.array(colour, np.uint8), (h, w, 3)).copy()


def mix(a, b, k, m):
    """pixel (y, x) comes from b when (x + y) % m < k"""
    y, x = np.mgrid[:a.shape[0], :a.shape[1]]
    return np.where((((x + y) % m) < k)[..., None], b, a).astype(np.uint8)


def first_pixels(frame, c, colour):
    out = frame.copy()
    out.reshape(-1, 3)[:c] = colour
    return out


def case(name, frames, p, check):
    frames = np.ascontiguousarray(np.stack(frames) if len(frames) else np.zeros((0,) + p.pop("_hw") + (3,), np.uint8), np.uint8)
    p.pop("_hw", None)
    CASES.append({"name": name, "frames": frames, "p": p, "check": check})


def flags(rows, bit):
    return np.flatnonzero(rows["flags"] & bit).tolist()


def bounds(shots):
    return [(int(s["first"]), int(s["count"]), int(s["kind"])) for s in shots]


# ---- signatures: sizes, bin edges, seams, grass edges, one colour ----------------------------------------------------------------------------
def _random_size(h, w):
    r = np.random.default_rng(h * 1000 + w)
    frames = [r.integers(0, 256, (h, w, 3), np.uint8) for _ in range(3)]
    th, tw = h // 4, w // 4

    def check(sig, rows, shots):
        return (sig[:, :512].sum(1) == h * w).all() and (sig[:, 512:1536].sum(1) == 16 * th * tw).all() and \
            (sig[:, 512:1536].reshape(3, 16, 64).sum(2) == th * tw).all() and (16 * th * tw < h * w) == (h % 4 > 0 or w % 4 > 0)
    case(f"random_{h}x{w}", frames, P(), check)


for _h, _w in ((4, 4), (5, 7), (8, 16), (17, 33), (64, 48), (256, 256)):
    _random_size(_h, _w)

EDGES = [0, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224, 255]


def _bin_edges():
    v = np.array(EDGES, np.uint8)[np.arange(128) % 16].reshape(8, 16)
    grey = np.stack([v, v, v], -1)
    only_b, only_g, only_r = (np.stack([v if k == c else np.zeros_like(v) for k in range(3)], -1) for c in range(3))

    def check(sig, rows, shots):
        ok = all(sig[0, k * 73] == 16 for k in range(8)) and sig[0, :512].sum() == 128 and all(sig[0, 512:1536].reshape(16, 64)[:, k * 21].sum() == 32 for k in range(4))
        for f, step5, step6 in ((1, 64, 16), (2, 8, 4), (3, 1, 1)):
            ok = ok and all(sig[f, k * step5] == 16 for k in range(8)) and all(sig[f, 512:1536].reshape(16, 64)[:, k * step6].sum() == 32 for k in range(4))
        return ok
    case("bin_edges_8x16", [grey, only_b, only_g, only_r], P(), check)


_bin_edges()


def _tile_seams():
    f = solid(17, 33, BLACK)                                              # th = 4, tw = 8: tiles over 16 x 32, one row and one column outside
    for y, x in ((3, 7), (4, 8), (15, 31), (16, 32), (16, 0), (0, 32)):
        f[y, x] = WHITE

    def check(sig, rows, shots):
        t = sig[0, 512:1536].reshape(16, 64)
        return sig[0, 511] == 6 and t[0, 63] == 1 and t[5, 63] == 1 and t[15, 63] == 1 and t[:, 63].sum() == 3 and t[:, 0].sum() == 16 * 32 - 3
    case("tile_seams_17x33", [f, f], P(), check)


_tile_seams()


def _grass_edges():
    f = solid(4, 4, BLACK)
    f.reshape(-1, 3)[:6] = [(0, 47, 0), (0, 48, 0), (0, 100, 85), (0, 100, 84), (85, 100, 0), (84, 100, 0)]
    case("grass_edges_4x4", [f, f], P(), lambda sig, rows, shots: list(rows["grass"]) == [3, 3])


_grass_edges()


def _one_colour():
    def check(sig, rows, shots):
        k5, k6 = (40 >> 5) * 64 + (140 >> 5) * 8 + (50 >> 5), (40 >> 6) * 16 + (140 >> 6) * 4 + (50 >> 6)
        return (sig[:, k5] == 64 * 48).all() and (sig[:, 512:1536].reshape(3, 16, 64)[:, :, k6] == 16 * 12).all() and (rows["grass"] == 64 * 48).all() and \
            not rows["d1"].any() and bounds(shots) == [(0, 3, SR.START)] and shots[0]["flags"] == SR.PITCH | SR.USABLE
    case("one_colour_64x48", [solid(64, 48, GRASS)] * 3, P(), check)


_one_colour()


# ---- scores exactly at, below and above cut and low: P = 65536, the change confined to the upper eight tiles, so S = sg = the pixels changed -----------
def _thresholds():
    base, other = solid(256, 256, GRASS), solid(256, 256, CROWD)
    for d in (-1, 0, 1):
        c = BASE["cut"] + d
        case(f"score_cut{d:+d}_256x256", [base, first_pixels(base, c, RED)], P(),
             lambda sig, rows, shots, c=c, d=d: rows["d1"][1] == c == rows["sg"][1] and rows["st"][1] == 0 and flags(rows, SR.HARD) == ([1] if d >= 0 else []))
        c = BASE["low"] + d
        case(f"score_low{d:+d}_256x256", [base, other, first_pixels(base, c, RED)], P(),
             lambda sig, rows, shots, c=c, d=d: rows["d2"][2] == c and flags(rows, SR.FLASH) == ([1] if d < 0 else []) and flags(rows, SR.HARD) == ([] if d < 0 else [1, 2]))


_thresholds()


# ---- cuts and flashes ------------------------------------------------------------------------------------------------------------------------
def _cuts():
    A, B, C, W = (solid(8, 16, c) for c in (GRASS, CROWD, RED, WHITE))
    case("cut_at_frame_1", [A, B, B, B], P(), lambda sig, rows, shots: flags(rows, SR.HARD) == [1] and bounds(shots) == [(0, 1, SR.START), (1, 3, SR.AFTER_CUT)])
    case("cut_at_last_frame", [A, A, A, B], P(), lambda sig, rows, shots: flags(rows, SR.HARD) == [3] and bounds(shots) == [(0, 3, SR.START), (3, 1, SR.AFTER_CUT)])
    case("cuts_back_to_back", [A, A, B, C, C], P(),
         lambda sig, rows, shots: flags(rows, SR.HARD) == [2, 3] and not flags(rows, SR.FLASH) and bounds(shots) == [(0, 2, 0), (2, 1, 1), (3, 2, 1)])
    case("flash_one_frame", [A, A, A, W, A, A, A], P(),
         lambda sig, rows, shots: flags(rows, SR.FLASH) == [3] and not flags(rows, SR.HARD) and bounds(shots) == [(0, 7, SR.START)] and rows["d1"][4] >= BASE["cut"])
    case("flash_in_last_frame_is_a_cut", [A, A, A, W], P(), lambda sig, rows, shots: not flags(rows, SR.FLASH) and flags(rows, SR.HARD) == [3])
    case("flash_two_frames", [A, A, W, W, A, A], P(),
         lambda sig, rows, shots: not flags(rows, SR.FLASH) and flags(rows, SR.HARD) == [2, 4] and bounds(shots)[1] == (2, 2, SR.AFTER_CUT) and shots[1]["flags"] & SR.SHORT)


_cuts()


# ---- gradual transitions -----------------------------------------------------------------------------------------------------------------
def _dissolves():
    W = 5
    for L in (1, 2, 3, 4):
        A, B = solid(20, 20, GRASS), solid(20, 20, CROWD)
        frames = [A] * 6 + [mix(A, B, k, L + 1) for k in range(1, L + 1)] + [B] * 6
        end = 6 + L

        def check(sig, rows, shots, end=end, L=L):
            ok = flags(rows, SR.GRADUAL_END) == [end] and flags(rows, SR.IN_TRANSITION) == list(range(end - W + 1, end)) and not flags(rows, SR.HARD)
            ok = ok and bounds(shots) == [(0, end - W + 1, SR.START), (end - W + 1, W - 1, SR.TRANSITION), (end, 6, SR.AFTER_TRANSITION)] and rows["dW"][end] == ONE
            if L == 1:                                                    # the plateau: the first of equal maxima wins
                ok = ok and list(rows["dW"][end:end + 4]) == [ONE] * 4
            return ok
        case(f"dissolve_{L}_of_window_5", frames, P(window=W, cut=39322 if L < 3 else BASE["cut"]), check)
    A, B = solid(24, 24, GRASS), solid(24, 24, CROWD)
    frames = [A] * 6 + [mix(A, B, k, 6) for k in range(1, 6)] + [B] * 6      # as long as the window: dW ties at 5 / 6 on the last mixed and the first new frame
    case("dissolve_of_window_length_ends_on_the_last_mixed_frame", frames, P(window=W),
         lambda sig, rows, shots: rows["dW"][10] == rows["dW"][11] == ONE * 5 // 6 and flags(rows, SR.GRADUAL_END) == [10] and not flags(rows, SR.HARD))
    A, B, C = solid(20, 20, GRASS), solid(20, 20, CROWD), solid(20, 20, RED)
    frames = [A] * 6 + [mix(A, B, 1, 4), mix(A, B, 1, 4)] + [C] * 6            # a dissolve that got a quarter of the way (below cut) when the cut came
    case("hard_cut_inside_the_window", frames, P(window=W),
         lambda sig, rows, shots: flags(rows, SR.HARD) == [8] and not flags(rows, SR.GRADUAL_END) and (rows["dW"][8:13] >= BASE["cut"]).all())
    A, B, C = solid(16, 16, GRASS), solid(16, 16, CROWD), solid(16, 16, RED)
    frames = [A] * 5 + [mix(A, B, k, 4) for k in (1, 2, 3)] + [B] + [mix(B, C, k, 4) for k in (1, 2, 3)] + [C] * 5
    case("two_transitions_a_window_apart", frames, P(window=4),
         lambda sig, rows, shots: flags(rows, SR.GRADUAL_END) == [8, 12] and
         bounds(shots) == [(0, 5, SR.START), (5, 3, SR.TRANSITION), (8, 1, SR.AFTER_TRANSITION), (9, 3, SR.TRANSITION), (12, 5, SR.AFTER_TRANSITION)])


_dissolves()


def _pan_and_captions():
    y, x = np.mgrid[:16, :64]
    frames = [np.where((((x + t) // 16) % 2 == 0)[..., None], np.array(GRASS, np.uint8), np.array(CROWD, np.uint8)).astype(np.uint8) for t in range(12)]
    case("slow_pan_has_no_boundary", frames, P(),
         lambda sig, rows, shots: not rows["flags"].any() and bounds(shots) == [(0, 12, SR.START)] and 0 < rows["dW"].max() < BASE["cut"] and rows["st"][1:].min() > 0)
    A = solid(64, 48, GRASS)
    B, C = A.copy(), A.copy()
    B[48:, :36] = WHITE                                                   # tiles 12, 13, 14
    C[16:, :] = WHITE                                                     # tiles 4 .. 15, twelve of them ...
    C[16:32, :36] = GRASS                                                 # ... less 4, 5, 6: nine
    case("caption_over_3_tiles_is_no_cut", [A, A, B, B], P(),
         lambda sig, rows, shots: not rows["flags"].any() and rows["sg"][2] == ONE * 3 // 16 and rows["st"][2] == 0)
    case("caption_over_9_tiles_is_a_cut", [A, A, C, C], P(),
         lambda sig, rows, shots: flags(rows, SR.HARD) == [2] and rows["sg"][2] == ONE * 9 // 16 and rows["st"][2] == ONE // 8)


_pan_and_captions()


# ---- clip lengths, shot lengths, the grass threshold -----------------------------------------------------------------------------------
def _lengths():
    cols = (GRASS, CROWD, RED, WHITE)
    for n in (0, 1, 2, 4, 5, 63, 64, 65, 257):
        frames = [solid(4, 4, cols[(i // 7) % 4]) for i in range(n)]
        case(f"frames_{n}", frames, P(_hw=(4, 4)),
             lambda sig, rows, shots, n=n: len(rows) == n and flags(rows, SR.HARD) == list(range(7, n, 7)) and len(shots) == (n + 6) // 7 and shots["count"].sum() == n)
    A, B = solid(4, 4, GRASS), solid(4, 4, CROWD)
    case("shot_of_min_len_and_one_shorter", [A, A, A, B, B], P(),
         lambda sig, rows, shots: [int(f) & SR.SHORT for f in shots["flags"]] == [0, SR.SHORT] and shots[0]["flags"] == SR.PITCH | SR.USABLE and shots[1]["flags"] == SR.SHORT)
    a = solid(4, 4, BLACK)
    a.reshape(-1, 3)[:8] = GRASS
    b = solid(4, 4, RED)
    b.reshape(-1, 3)[:8] = GRASS2
    b7 = b.copy()
    b7[0, 0] = RED
    case("grass_sum_at_the_threshold_product", [a, a, b, b7], P(grass_thr=32768, min_len=1),
         lambda sig, rows, shots: list(shots["grass_sum"]) == [16, 15] and list(shots["flags"]) == [SR.PITCH | SR.USABLE, 0] and flags(rows, SR.HARD) == [2])


_lengths()

# every refusal: (what changes, the value the message must name)
REFUSALS = [({"cut": -1}, "-1"), ({"cut": 65537}, "65537"), ({"low": -2}, "-2"), ({"low": 65538, "cut": 65536}, "65538"), ({"grass_thr": -3}, "-3"),
            ({"grass_thr": 65539}, "65539"), ({"low": 20000}, "20000"), ({"window": 1}, "window 1"), ({"window": 0}, "window 0"), ({"window": -7}, "-7"),
            ({"min_len": 0}, "min_len 0"), ({"min_len": -9}, "-9")]
BAD_SIZES = [(3, 8), (8, 3), (0, 8), (-1, 8)]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = BY_NAME[name]
    out = SR.shots(c["frames"], c["p"])
    for a in out:
        a.setflags(write=False)
    return out
