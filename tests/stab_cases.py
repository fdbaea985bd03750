"""Constructed tables for the stabilisation stage (tests/stab_ref.py is the contract): the smallest shapes at which stab.hip can go wrong.  A case is
{"name", "values" float64 [cols][rows][2], "frames" int32 [rows], "columns" [(kind, id, video)], "params" (stab_ref.stabilise's keywords, fps included)};
`reference(name)` computes the contract once (windowed formulation) and every test shares it.  FLAGGED names the cases built to hit the 64-voter cap or
a fall-back; no other case may (tests/test_stab_cpu.py)."""
import functools

import numpy as np

import stab_ref as SB

P, G, BALL, BND = SB.PLAYER, SB.GOALKEEPER, SB.BALL, SB.BOUNDARY
ST_TILE = 256                                   # csrc/stab.hip: rows of a column per workgroup of the predict kernel
NAN, INF = float("nan"), float("inf")
SPOTS = [(-40.0, -20.0), (-25.0, 15.0), (-10.0, -5.0), (0.0, 25.0), (10.0, -25.0), (20.0, 10.0), (35.0, -10.0), (45.0, 20.0), (-30.0, 0.0), (5.0, 5.0), (28.0, 28.0),
         (-15.0, -28.0)]


def spot(i):
    x, y = SPOTS[i % len(SPOTS)]
    k = i // len(SPOTS)
    return x + 1.7 * k, y - 1.3 * k


def common_error(rows, seed, shift=0.4, gain=0.003):
    """per row (tx, ty, gxx, gxy, gyx, gyy): the affine error of the frame's homography about the pitch centre"""
    rng = np.random.default_rng(1000 + seed)
    return np.concatenate([rng.uniform(-shift, shift, (rows, 2)), rng.uniform(-gain, gain, (rows, 4))], 1)


def distort(p, e):
    """[rows][2] true positions, [rows][6] errors -> observed positions"""
    x, y = p[:, 0], p[:, 1]
    return np.stack([x + e[:, 0] + e[:, 2] * x + e[:, 3] * y, y + e[:, 1] + e[:, 4] * x + e[:, 5] * y], 1)


def runner(rows, i, seed, frames, jitter=0.02):
    """person i on a slow curve around its spot, [rows][2] metres"""
    rng = np.random.default_rng(seed * 131 + i)
    t = np.asarray(frames, np.float64)
    x0, y0 = spot(i)
    x = x0 + 0.04 * t * np.cos(i) + 1.5 * np.sin(t / 40.0 + i)
    y = y0 + 0.03 * t * np.sin(i) + 1.0 * np.cos(t / 50.0 + 2 * i)
    return np.stack([x, y], 1) + rng.uniform(-jitter, jitter, (rows, 2))


def table(rows, persons, seed, frames=None, ball=True, video=True, boundary=True, shift=0.4, gain=0.003, jitter=0.02):
    """persons person columns (the second a goalkeeper), a video column after the first, then optionally the ball pair and a boundary column; every pitch
    column carries the rows' common error, the boundary too (it is not moved)"""
    frames = np.arange(rows) + 7 if frames is None else np.asarray(frames)
    e = common_error(rows, seed, shift, gain)
    cols, vals = [], []
    for i in range(persons):
        cols.append((G if i == 1 else P, i + 1, 0))
        vals.append(distort(runner(rows, i, seed, frames, jitter), e))
        if i == 0 and video:
            cols.append((P, 1, 1))
            vals.append(runner(rows, 40, seed, frames, jitter) * 10.0)
    if ball:
        cols += [(BALL, 0, 0), (BALL, 0, 1)]
        vals += [distort(runner(rows, 50, seed, frames, jitter), e), runner(rows, 51, seed, frames, jitter) * 10.0]
    if boundary:
        cols.append((BND, 0, 0))
        vals.append(distort(runner(rows, 60, seed, frames, jitter), e))
    return np.array(vals, np.float64).reshape(len(cols), rows, 2), cols


def static_table(spots_q, rows, ball_q=None):
    """persons standing still at integer quantisation units (so every prediction is exact), optionally a standing ball"""
    cols = [(P, i + 1, 0) for i in range(len(spots_q))]
    vals = [np.tile(np.array(s, np.float64) / 1024.0, (rows, 1)) for s in spots_q]
    if ball_q is not None:
        cols.append((BALL, 0, 0))
        vals.append(np.tile(np.array(ball_q, np.float64) / 1024.0, (rows, 1)))
    return np.array(vals, np.float64).reshape(len(cols), rows, 2), cols


STATIC_Q = [(int(x * 1024), int(y * 1024)) for x, y in SPOTS[:8]]


def _case(name, values, columns, frames=None, **params):
    rows = values.shape[1]
    frames = np.arange(rows, dtype=np.int32) + 7 if frames is None else np.asarray(frames, np.int32)
    params.setdefault("fps", 25)
    return {"name": name, "values": np.ascontiguousarray(values, np.float64), "frames": frames, "columns": list(columns), "params": params}


def _cases():
    out = []
    # rows 0 .. 3: nobody can vote below three rows; with three the middle row does
    for rows in range(4):
        v, c = table(rows, 7, 10 + rows)
        out.append(_case(f"rows_{rows}", v, c, window=2))
    # around the predict kernel's tile: the window crosses the 256-row edge from both sides
    for rows in (ST_TILE - 1, ST_TILE, ST_TILE + 1, ST_TILE + 11):
        v, c = table(rows, 10, 20, boundary=False)
        out.append(_case(f"tile_rows_{rows}", v, c, window=10, iterations=1))
    # frames with holes: rows near in position are far in frames
    frames = np.array([0, 1, 2, 3, 4, 5, 20, 40, 41, 60, 61, 62, 80, 82, 84, 86, 88, 89, 90, 91, 92, 93, 200, 201, 202, 203, 204, 205, 206, 207], np.int32)
    v, c = table(len(frames), 7, 41, frames=frames, boundary=False)
    out.append(_case("frames_with_holes", v, c, frames=frames, window=3))
    # columns that begin or end inside the table: a cell with rows only before or only after it does not vote
    v, c = table(24, 9, 42)
    v[0, :9] = NAN
    v[2, 15:] = NAN
    v[3, :5] = NAN
    v[3, 19:] = NAN
    out.append(_case("one_sided_columns", v, c, window=4))
    # NaN, +-inf and |x| just over 1024 inside a run; exactly 1024 is present
    v, c = table(30, 10, 43)
    v[0, 12] = (NAN, 3.0)
    v[2, 20] = (5.0, INF)
    v[3, 12] = (-INF, 2.0)
    v[4, 18] = (1024.0009765625, 10.0)
    v[5, 10] = (10.0, -1024.0009765625)
    v[6, 22] = (NAN, NAN)
    v[11, 14] = (NAN, NAN)                                   # the ball (column 11: ten persons and the first one's video column come first)
    out.append(_case("nan_inf_limit", v, c, window=4))
    v, c = static_table(STATIC_Q, 7)
    v[3, 3] = (1024.0, -1024.0)
    out.append(_case("exactly_1024", v, c, window=2, iterations=1))
    # one voter below min_voters and exactly min_voters
    for persons in (5, 6):
        v, c = table(12, persons, 44, gain=0.0)                 # a pure shift: nobody is trimmed, the six inliers carry the affine map
        out.append(_case(f"voters_{persons}_of_6", v, c, window=3))
    v, c = table(12, 4, 44)
    out.append(_case("min_voters_3_translation", v, c, window=3, min_voters=3, model=0))
    # 64 and 65 voters
    for persons in (64, 65):
        v, c = table(7, persons, 45, ball=False, boundary=False)
        out.append(_case(f"voters_{persons}", v, c, window=2, iterations=1))
    # 300 columns of which six are present per row (twelve where the two sets overlap, of which six vote: a set's first and last row cannot)
    v, c = table(18, 300, 46, ball=False, video=False, boundary=False, gain=0.0)
    keep_a, keep_b = (12, 25, 39, 100, 150, 295), (24, 61, 75, 136, 186, 283)
    for col in range(300):
        if col in keep_a:
            v[col, 10:] = NAN
        elif col in keep_b:
            v[col, :8] = NAN
        else:
            v[col] = NAN
    out.append(_case("columns_300_six_present", v, c, window=2, iterations=1))
    # all voters on one line along x: the spread fall-back
    v, c = static_table([(x, 5000) for x, _ in STATIC_Q], 7)
    v[:, 3] += (0.25, -0.125)
    out.append(_case("collinear_spread_fallback", v, c, window=2, iterations=1))
    # two tight clusters far apart on a diagonal: the correlation fall-back
    two = [(-30000 + 40 * i, -20000 + 55 * i * (-1) ** i) for i in range(4)] + [(30000 + 35 * i * (-1) ** i, 20000 + 60 * i) for i in range(4)]
    v, c = static_table(two, 7)
    v[:, 3] += (0.25, -0.125)
    out.append(_case("two_clusters_correlation_fallback", v, c, window=2, iterations=1))
    # a pure scale error of 3 % along x in one row (0.03 / 1.03 = 0.029126 of the observed x): just inside and just outside max_gain
    v, c = static_table(STATIC_Q, 7, ball_q=(1024, 2048))
    v[:, 3, 0] += np.rint(0.03 * v[:, 3, 0] * 1024.0) / 1024.0
    out.append(_case("gain_inside", v, c, window=2, iterations=1, max_gain=0.0292, jump=0.001))
    out.append(_case("gain_outside", v, c, window=2, iterations=1, max_gain=0.0290))
    # one row shifted by an integer vector: every vote equal, the medians tie
    v, c = static_table(STATIC_Q, 7, ball_q=(1024, 2048))
    v[:, 3] += (300 / 1024.0, -77 / 1024.0)
    out.append(_case("equal_votes", v, c, window=2, iterations=1))
    out.append(_case("equal_votes_translation", v, c, window=2, iterations=1, model=0))
    # votes 0, 0, 0, 1, -1, 3, 4 along x and the last two along y too, no floor: m = 1, the threshold 3 m is met exactly by 3 and missed by 4
    v, c = static_table(STATIC_Q[:7], 7)
    for col, (dx, dy) in enumerate(((0, 0), (0, 0), (0, 0), (1, 0), (-1, 0), (3, -3), (4, 0))):
        v[col, 3] += (dx / 1024.0, dy / 1024.0)
    out.append(_case("trim_threshold", v, c, window=2, iterations=1, floor=0.0, model=0))
    out.append(_case("trim_k_0", v, c, window=2, iterations=1, floor=0.0, model=0, trim_k=0.0))
    # 40 % of a row's voters displaced by 3 m
    v, c = table(9, 10, 47, ball=False, boundary=False, video=False)
    v[:4, 4] += (3.0, 0.0)
    out.append(_case("displaced_40_percent", v, c, window=3, iterations=1))
    # rounds, half-widths, degrees
    v, c = table(40, 10, 48)
    for it in (1, 2, 4):
        out.append(_case(f"iterations_{it}", v, c, window=5, iterations=it))
    out.append(_case("window_1", v, c, window=1))
    out.append(_case("degree_1", v, c, window=5, degree=1))
    out.append(_case("degree_2_translation", v, c, window=5, degree=2, model=0))
    v, c = table(ST_TILE + 64 + 1, 10, 49, ball=False, boundary=False)
    out.append(_case("window_64", v, c, window=64, iterations=1))
    v, c = table(70, 10, 49, boundary=False)
    out.append(_case("window_64_short", v, c, window=64, degree=1))
    # a table without a voter column
    v, c = table(9, 0, 50)
    c = [(P, 3, 1)] + c
    v = np.concatenate([runner(9, 41, 50, np.arange(9))[None] * 10.0, v])
    out.append(_case("no_voter_column", v, c, window=3))
    return out


FLAGGED = {"voters_65": SB.F_OVER_CAP, "collinear_spread_fallback": SB.F_SPREAD, "two_clusters_correlation_fallback": SB.F_CORR, "gain_outside": SB.F_GAIN}
CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def reference(name, form="window"):
    c = BY_NAME[name]
    return SB.stabilise(c["values"], c["frames"], c["columns"], form=form, **c["params"])
