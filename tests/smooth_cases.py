"""Constructed tables for the track-smoothing stage (tests/smooth_ref.py is the contract): the smallest shapes at which smooth.hip can go wrong.  A case is
{"name", "values" float64 [cols][rows][2], "frames" int32 [rows], "columns" [(kind, id, video)], "params" (smooth_ref.smooth's keywords, fps included)};
`reference(name)` computes the contract once (windowed formulation) and every test shares it."""
import functools

import numpy as np

import smooth_ref as SR

P, G, BALL, BND = SR.PLAYER, SR.GOALKEEPER, SR.BALL, SR.BOUNDARY
SM_TILE = 256                                   # csrc/smooth.hip: rows of a column per workgroup
NAN, INF = float("nan"), float("inf")


def path(rows, seed, jitter=0.05, speed=0.2):
    """a runner on a curve, [rows][2] metres, with uniform jitter"""
    rng = np.random.default_rng(seed)
    t = np.arange(rows, dtype=np.float64)
    x = 20.0 + speed * t + 3.0 * np.sin(t / 17.0 + seed)
    y = 30.0 + 5.0 * np.cos(t / 23.0 + 0.5 * seed)
    return np.stack([x, y], 1) + rng.uniform(-jitter, jitter, (rows, 2))


def table(rows, persons, seed, ball=True, video=True, boundary=True, **kw):
    """persons person columns (the second a goalkeeper), then optionally a video column, the ball pair and a boundary column"""
    cols, vals = [], []
    for i in range(persons):
        cols.append((G if i == 1 else P, i + 1, 0))
        vals.append(path(rows, seed + i, **kw))
    if video:
        cols.append((P, 1, 1))
        vals.append(path(rows, seed + 50, **kw) * 10.0)
    if ball:
        cols += [(BALL, 0, 0), (BALL, 0, 1)]
        vals += [path(rows, seed + 60, **kw), path(rows, seed + 61, **kw) * 10.0]
    if boundary:
        cols.append((BND, 0, 0))
        vals.append(path(rows, seed + 70, **kw))
    return np.array(vals, np.float64).reshape(len(cols), rows, 2), cols


def _case(name, values, columns, frames=None, **params):
    rows = values.shape[1]
    frames = np.arange(rows, dtype=np.int32) * 1 + 7 if frames is None else np.asarray(frames, np.int32)
    params.setdefault("fps", 25)
    return {"name": name, "values": np.ascontiguousarray(values, np.float64), "frames": frames, "columns": list(columns), "params": params}


def _cases():
    out = []
    # rows 0 .. 4 (the degree rule: n = 1, 2, 3, 4), and a table without a person column
    for rows in range(5):
        v, c = table(rows, 2, 10 + rows)
        out.append(_case(f"rows_{rows}", v, c, window=2, ball_window=2))
    v, c = table(5, 0, 3)
    out.append(_case("no_person_column", v, c, window=3))
    # around a tile: an outlier on the last row of a tile, one in each halo
    for rows in (SM_TILE - 1, SM_TILE, SM_TILE + 1, SM_TILE + 10 + 1):
        v, c = table(rows, 2, 20, boundary=False)
        for col, r in ((0, SM_TILE - 1), (0, SM_TILE + 3), (1, SM_TILE - 4), (1, 5)):
            if r < rows:
                v[col, r] += (3.0, -2.0)
        out.append(_case(f"tile_rows_{rows}", v, c, window=10))
    # every half-width and both degrees
    for W, deg, rows in ((1, 1, 40), (1, 2, 40), (2, 1, 60), (2, 2, 60), (10, 1, 90), (10, 2, 90), (64, 1, 140), (64, 2, SM_TILE + 64 + 1)):
        v, c = table(rows, 1, 30 + W + deg, video=False, boundary=False)
        for r in range(7, rows, 29):
            v[0, r] += (-2.5, 3.0)
        v[1, rows // 2] += (4.0, 0.0)
        out.append(_case(f"window_{W}_degree_{deg}", v, c, window=W, degree=deg, ball_window=min(W, 3)))
    # frames with holes: windows of n = 1, 2, 3 and more rows
    frames = np.array([0, 1, 2, 3, 4, 5, 20, 40, 41, 60, 61, 62, 80, 82, 84, 86, 88, 89, 90, 91, 92, 93, 200, 201, 202, 203, 204, 205, 206, 207], np.int32)
    v, c = table(len(frames), 2, 41, boundary=False)
    out.append(_case("frames_with_holes", v, c, frames=frames, window=3))
    out.append(_case("frames_with_holes_degree_1", v, c, frames=frames, window=3, degree=1))
    # columns that begin or end inside the table; NaN, +-inf and |x| just over 1024 inside a run; exactly 1024 is present
    v, c = table(40, 3, 42, ball=False)
    v[0, :9] = NAN
    v[1, 30:] = NAN
    v[2, :4] = NAN
    v[2, 37:] = NAN
    v[0, 15] = (NAN, 3.0)
    v[0, 20] = (5.0, INF)
    v[1, 12] = (-INF, 2.0)
    v[1, 18] = (1024.0009765625, 10.0)
    v[2, 10] = (10.0, -1024.0009765625)
    v[2, 14] = (1024.0, -1024.0)
    v[2, 22] = (NAN, NAN)
    out.append(_case("begin_end_nan_inf_limit", v, c, window=4))
    # x * 1024 exactly on a half: ties to even, both signs
    v, c = table(24, 1, 43, ball=False, video=False, boundary=False)
    k = np.arange(24)
    v[0, :, 0] = (k + 0.5) / 1024.0
    v[0, :, 1] = -(3 * k + 0.5) / 1024.0
    out.append(_case("ties_to_even", v, c, window=2))
    # a constant column: every residual 0, the median ties, the floor (0 here) decides: nothing is rejected
    v, c = table(30, 2, 44, ball=False, video=False, boundary=False)
    v[0] = (12.5, -3.25)
    v[1] = (7.0, 7.0)
    out.append(_case("constant_column", v, c, window=5, outlier_floor=0.0))
    # an exactly quadratic integer column (in quantisation units), with holes in the frames
    frames = np.cumsum(np.array([1, 1, 2, 1, 3, 1, 1, 1, 2, 1] * 6)).astype(np.int32)
    t = frames.astype(np.int64)
    v = np.zeros((2, len(t), 2))
    v[0, :, 0] = (1000 + 37 * t - 2 * t * t) / 1024.0
    v[0, :, 1] = (-50000 + 11 * t + 3 * t * t) / 1024.0
    v[1, :, 0] = (5 * t * t) / 1024.0
    v[1, :, 1] = (123456 - 7 * t) / 1024.0
    out.append(_case("exactly_quadratic", v, [(P, 1, 0), (G, 2, 0)], frames=frames, window=6))
    out.append(_case("exactly_quadratic_window_64", v, [(P, 1, 0), (G, 2, 0)], frames=frames, window=64))
    # a low threshold without a floor: windows whose samples are all rejected but one, or all (the cell keeps its raw value), and cells whose own sample goes
    v, c = table(80, 2, 45, ball=False, video=False, boundary=False, jitter=0.5)
    out.append(_case("nearly_all_rejected", v, c, window=2, outlier_k=0.5, outlier_floor=0.0))
    out.append(_case("nearly_all_rejected_window_1", v, c, window=1, outlier_k=0.25, outlier_floor=0.0, degree=1))
    # the same jumps with trimming off
    v, c = table(60, 2, 46, ball=False, boundary=False)
    v[0, 20] += (3.0, 3.0)
    v[1, 41] -= (3.0, 0.0)
    out.append(_case("outlier_k_0", v, c, window=10, outlier_k=0.0))
    out.append(_case("outlier_k_4", v, c, window=10))
    # a row on which every person jumps (suspect) and one with three persons present, all jumping (below the threshold of 4)
    v, c = table(60, 5, 47)
    v[:5, 20] += (3.0, -1.0)
    v[3:5, 38:43] = NAN
    v[:3, 40] += (-2.0, 3.0)
    v[:2, 50] += (3.0, 0.0)                                  # two of five: fewer than half
    out.append(_case("suspect_rows", v, c, window=6))
    # the ball: left alone, and smoothed with its own half-width
    v, c = table(50, 2, 48)
    v[3, 25] += (5.0, 5.0)
    out.append(_case("ball_window_0", v, c, window=5, ball_window=0))
    out.append(_case("ball_window_3", v, c, window=5, ball_window=3))
    # a speed above the cap: 1 m a frame at 25 fps
    v, c = table(40, 2, 49, ball=False, boundary=False, speed=1.0)
    out.append(_case("speed_above_cap", v, c, window=4, fps=25, speed_cap=12.0, max_gap=2))
    out.append(_case("speed_cap_3_fps_5", v, c, window=2, fps=5, speed_cap=3.0))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def reference(name, form="window"):
    c = BY_NAME[name]
    return SR.smooth(c["values"], c["frames"], c["columns"], form=form, **c["params"])
