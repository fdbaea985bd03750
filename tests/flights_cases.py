"""Constructed tables for the ball-flight contract (tests/flights_ref.py).  A case: name, values float64 [cols][rows][2], frames int32 [rows], columns
[(kind, id, video)], params (keywords of flights_ref.params / lib.flight_params; fps and max_gap always), cuts.  Most have a few dozen rows; `tiles` has
770 (runs of 255, 256 and 257 rows around the cost kernel's tile of 256 rows) and `capped_300` has 300."""
import functools

import numpy as np

import flights_ref as FR

P, G, B, X = FR.PLAYER, FR.GOALKEEPER, FR.BALL, FR.BOUNDARY
NAN, INF = float("nan"), float("inf")
CASES = []


def table(ball, persons=(), frames=None, ball_column=True):
    """ball [rows][2] -> columns Ball, Ball_video, then per person a pitch and a video column"""
    ball = np.asarray(ball, np.float64).reshape(-1, 2)
    rows = len(ball)
    cols, vals = [], []
    if ball_column:
        cols += [(B, 0, 0), (B, 0, 1)]
        vals += [ball, ball * 7.0 + 3.0]
    for k, p in enumerate(persons):
        p = np.broadcast_to(np.asarray(p, np.float64), (rows, 2))
        cols += [(G if k == 0 else P, 10 + k, 0), (G if k == 0 else P, 10 + k, 1)]
        vals += [p, p * 5.0]
    values = np.stack(vals) if vals else np.zeros((0, rows, 2))
    frames = np.arange(rows, dtype=np.int32) if frames is None else np.asarray(frames, np.int32)
    return values, frames, cols


def add(name, values, frames, columns, cuts=None, fps=32.0, max_gap=8, **kw):
    CASES.append(dict(name=name, values=np.ascontiguousarray(values, np.float64), frames=np.asarray(frames, np.int32), columns=list(columns),
                      params=dict(fps=fps, max_gap=max_gap, **kw), cuts=None if cuts is None else np.asarray(cuts, np.int32)))


def line(p0, v, n, t=None):
    """n samples of p0 + v t (metres, metres per row), t = 0 .. n - 1 unless given"""
    t = np.arange(n, dtype=np.float64) if t is None else np.asarray(t, np.float64)
    return np.asarray(p0, np.float64)[None, :] + t[:, None] * np.asarray(v, np.float64)[None, :]


def path(*legs, start=(20.0, 20.0)):
    """legs (v, rows): each leg starts where the one before ended"""
    out, p = [np.asarray(start, np.float64)[None, :]], np.asarray(start, np.float64)
    for v, n in legs:
        seg = line(p, v, n + 1)[1:]
        out.append(seg)
        p = seg[-1]
    return np.concatenate(out)


def _build():
    rng = np.random.default_rng(40)
    far = [(90.0, 60.0), (5.0, 5.0)]
    # ---- empty and degenerate ----
    add("empty", *table(np.zeros((0, 2)), far))
    add("no_ball_column", *table(line((10, 10), (0.5, 0), 6), far, ball_column=False))
    add("ball_all_nan", *table(np.full((7, 2), NAN), far))
    one = np.full((6, 2), NAN); one[3] = (30.0, 30.0)
    add("one_present_row", *table(one, far))
    two = np.full((6, 2), NAN); two[2] = (30.0, 30.0); two[3] = (30.5, 30.25)
    add("two_present_rows", *table(two, far))
    ab = line((10, 10), (0.5, 0.25), 24)
    ab[4] = (NAN, 12.0); ab[9] = (14.0, INF); ab[10] = (-INF, 1.0); ab[15] = (1024.5, 10.0); ab[16] = (10.0, -1025.0); ab[20] = (1024.0, -1024.0)
    add("absent_kinds", *table(ab, far))
    # ---- exact and tied fits ----
    add("all_equal", *table(np.full((12, 2), 33.25), far))
    add("integer_slope", *table(line((10, 20), (0.5, 0.25), 14), far))
    add("right_angle", *table(path(((0.5, 0.0), 12), ((0.0, 0.5), 12)), far))
    add("reversal", *table(path(((0.75, 0.25), 10), ((-0.75, -0.25), 10)), far))
    # ---- spikes ----
    sp = line((10, 10), (0.5, 0.125), 16); sp[1] += (0.0, 3.0); sp[14] += (-3.0, 0.0)
    add("spike_row1_and_last_but_one", *table(sp, far))
    adj = line((40, 30), (0.0, 0.0), 14); adj[6] += (3.0, 0.0); adj[7] += (3.0, 0.0)
    add("two_adjacent_displaced", *table(adj, far))
    zz = line((40, 30), (0.25, 0.0), 13); zz[1::2] += (0.0, 2.0)
    add("equal_A_neighbours", *table(zz, far))
    sk = path(((0.5, 0.0), 10), ((0.0, 0.5), 10)); sk[11] += (2.5, 2.5)
    add("spike_next_to_knot", *table(sk, far))
    sk2 = path(((0.5, 0.0), 10), ((0.0, 0.5), 10)); sk2[9] += (0.0, -3.0)
    add("spike_before_knot", *table(sk2, far))
    # ---- frames, runs and cuts ----
    fr = np.array([0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 20, 21, 22, 23, 24], np.int32)
    add("hole_max_gap_and_one_more", *table(line((10, 10), (0.25, 0.5), 16, fr), far, frames=fr), max_gap=5)
    steps = np.cumsum([0, 1, 2, 3, 1, 1, 4, 2, 1, 3, 3, 1, 2, 2, 1, 4, 1, 1]).astype(np.int32)
    un = np.concatenate([line((10, 10), (0.25, 0.0), 9, steps[:9]), line((10 + 0.25 * steps[8], 10), (0.0, 0.375), 9, steps[9:] - steps[8])])
    add("uneven_steps", *table(un, far, frames=steps), max_gap=4)
    add("cut_inside_run", *table(path(((0.5, 0.0), 19)), far, frames=np.arange(100, 120)), cuts=[90, 110, 300])
    hole = line((10, 10), (0.5, 0.0), 20); hole[8] = NAN
    add("cut_on_run_first_row", *table(hole, far, frames=np.arange(50, 70)), cuts=[50, 59])
    # ---- segment length and tiles ----
    noisy = path(((0.6, 0.1), 14), ((-0.2, 0.5), 9), ((0.0, 0.0), 8), ((0.3, -0.6), 12)) + rng.normal(0.0, 0.1, (44, 2))
    persons = [line((24, 21), (0.3, 0.1), 44), (28.0, 24.0), line((30, 30), (-0.1, -0.2), 44)]
    for L in (2, 3, 64, 128):
        add(f"max_rows_{L}", *table(noisy, persons), max_rows=L)
    long_line = line((5, 5), (0.3, 0.2), 300) + rng.normal(0.0, 0.05, (300, 2))
    add("capped_300", *table(line((5, 5), (0.25, 0.125), 300), far), max_rows=128)       # every cost is 0: the ties give the longest last segments
    add("noisy_300", *table(long_line, far), max_rows=128)
    add("capped_150_L64", *table(long_line[:150], far), max_rows=64)
    legs, v = [], np.array([0.4, 0.1])
    while sum(n for _, n in legs) < 769:
        legs.append((tuple(v), int(rng.integers(9, 40))))
        v = rng.uniform(-0.6, 0.6, 2)
    til = path(*legs, start=(50.0, 34.0))[:770] + rng.normal(0.0, 0.08, (770, 2))
    til = np.clip(til, -900.0, 900.0)
    til[255] = NAN; til[512] = NAN                                 # runs [0, 254], [256, 511], [513, 769]: 255, 256 and 257 rows
    sel = rng.choice(np.setdiff1d(np.arange(3, 767), [254, 255, 256, 511, 512, 513]), 12, replace=False)
    til[sel] += 3.0
    add("tiles", *table(til, [line((50, 34), (0.05, 0.0), 770)]), max_rows=128)
    add("tiles_L33", *table(til, [line((50, 34), (0.05, 0.0), 770)]), max_rows=33)
    # ---- cost and penalty extremes ----
    alt = np.tile(np.array([[1023.0, -1023.0], [-1023.0, 1023.0]]), (10, 1))
    add("cost_above_clamp", *table(alt, far), max_rows=128, spike=1024.0, penalty=2.0 ** 20, noise=1.0)
    add("penalty_zero", *table(noisy, persons), penalty=0.0)
    add("penalty_at_bound", *table(noisy, persons), penalty=2.0 ** 20, noise=1.0)
    add("noise_zero", *table(noisy, persons), noise=0.0)
    # ---- kicks: fps 32, so 96 / 1024 m per row is 3 m/s and 128 / 1024 m per row 4 m/s ----
    corner = path(((96 / 1024, 0.0), 10), ((0.0, 128 / 1024), 10), start=(30.0, 30.0))
    add("dv_exactly_kick_dv", *table(corner, far), kick_dv=5.0)
    add("dv_just_below_kick_dv", *table(corner, far), kick_dv=5.000000000000001)
    kx, ky = corner[10]
    add("kicker_tie", *table(corner, [(kx + 1.0, ky), (kx - 1.0, ky), (kx, ky + 1.0)]), kick_dv=1.0)
    add("kick_nobody_in_radius", *table(corner, [(kx + 2.5, ky), (kx, ky - 2.5)]), kick_dv=1.0)
    add("no_person_columns", *table(corner), kick_dv=1.0)
    add("person_cells_absent", *table(corner, [(NAN, ky), (kx, INF), (kx + 2000.0, ky)]), kick_dv=1.0)
    # ---- flight kind ----
    fast = line((30, 30), (0.5, 0.0), 10)
    walk = np.concatenate([fast[:5] + (0.0, 1.0), np.full((5, 2), 0.0)])
    add("near_exactly_half", *table(fast, [walk]))
    add("near_one_more_than_half", *table(fast, [np.concatenate([fast[:6] + (0.0, 1.0), np.full((4, 2), 0.0)])]))
    add("speed_exactly_still_speed", *table(line((30, 30), (16 / 1024, 0.0), 10), far))
    add("speed_below_still_speed", *table(line((30, 30), (15 / 1024, 0.0), 10), far))
    # ---- shots: 512 / 1024 m per row is 16 m/s.  Runs are separated by an absent row ----
    def runs(*parts):
        out = []
        for p in parts:
            out += [p, np.full((1, 2), NAN)]
        return np.concatenate(out[:-1])
    h = 512 / 1024
    on_post_in, on_post_out = 38563 / 1024, 38564 / 1024           # 34 + 3.66 = 37.66 lies between these neighbours of the grid
    shots = runs(line((80.0, 34.0), (h, 0.0), 6),                  # on target, the right goal
                 line((80.0, on_post_in), (h, 0.0), 6), line((80.0, on_post_out), (h, 0.0), 6),
                 line((80.0, 40.0), (h, 0.0), 6),                  # |y* - 34| = 6 = 3.66 + shot_margin exactly
                 line((80.0, 40.0 + 1 / 1024), (h, 0.0), 6),
                 line((65.0, 34.0), (h, 0.0), 6),                  # reach 40 = shot_range exactly
                 line((65.0 - 1 / 1024, 34.0), (h, 0.0), 6),
                 line((25.0, 35.0), (-h, 1 / 64), 6),              # the left goal
                 line((50.0, 20.0), (0.0, h), 6),                  # vx == 0
                 line((110.0, 34.0), (h, 0.0), 6),                 # behind the goal line, moving away: reach < 0
                 line((10.0, 34.0), (h, 0.0), 6),                  # too far
                 line((90.0, 30.0), (0.25, 0.0), 6))               # too slow
    add("shots", *table(shots, far), shot_margin=6.0 - 3.66)
    add("shots_default_margin", *table(shots, far))
    # ---- a general noisy table with people around ----
    gen = path(((0.55, 0.1), 16), ((0.1, 0.12), 14), ((0.0, 0.0), 9), ((-0.5, 0.3), 15)) + rng.normal(0.0, 0.12, (55, 2))
    gen[7] += (2.0, -2.0); gen[30] = NAN; gen[40] += (0.0, 3.0)
    fr = np.cumsum(rng.integers(1, 3, 55)).astype(np.int32)
    add("general", *table(gen, [gen + rng.normal(0.0, 1.2, (55, 2)), (25.0, 22.0), gen[::-1].copy()], frames=fr), cuts=[int(fr[22])], fps=25.0, max_gap=2)


_build()


def demo(seed, rows=500, fps=25.0):
    """The demonstration clip: the ball alternates passes (8 .. 22 m/s for 12 .. 44 rows), carries (2 .. 6 m/s for 15 .. 49 rows, a player beside it) and
    rests (10 .. 39 rows), reflected at the pitch edge; 0.15 m Gaussian jitter; 2 % of the samples displaced by exactly 3 m in a random direction, no two
    within 3 rows of each other -> dict(values, frames, columns, truth float64 [rows][2] m/s, changes [(row, |dv|)], displaced [rows])."""
    rng = np.random.default_rng(seed)
    pos, vel, changes = np.zeros((rows, 2)), np.zeros((rows, 2)), []
    carried = np.zeros(rows, bool)
    p, v, r, kind = np.array([rng.uniform(20, 85), rng.uniform(15, 53)]), np.zeros(2), 0, 0
    while r < rows:
        if kind % 3 == 0:
            speed, n = rng.uniform(8, 22), int(rng.integers(12, 45))
        elif kind % 3 == 1:
            speed, n = rng.uniform(2, 6), int(rng.integers(15, 50))
        else:
            speed, n = 0.0, int(rng.integers(10, 40))
        ang = rng.uniform(0, 2 * np.pi)
        nv = speed * np.array([np.cos(ang), np.sin(ang)])
        if r:
            changes.append((r - 1, float(np.hypot(*(nv - v)))))   # the sample at row r - 1 is the last on the old line and the first on the new one
        v = nv
        for _ in range(n):
            if r >= rows:
                break
            if r:
                q = p + v / fps
                for k, hi in ((0, 105.0), (1, 68.0)):
                    if q[k] < 0.0 or q[k] > hi:                   # reflected at the pitch edge: a change of velocity too
                        old = v.copy()
                        v = v.copy(); v[k] = -v[k]
                        changes.append((r - 1, float(np.hypot(*(v - old)))))
                        q = p + v / fps
                p = q
            pos[r], vel[r], carried[r] = p, v, kind % 3 == 1
            r += 1
        kind += 1
    noisy = pos + rng.normal(0.0, 0.15, (rows, 2))
    displaced = []
    for r in rng.permutation(np.arange(2, rows - 2)):
        if len(displaced) < round(0.02 * rows) and all(abs(int(r) - d) > 3 for d in displaced):
            displaced.append(int(r))
    for r in displaced:
        a = rng.uniform(0, 2 * np.pi)
        noisy[r] += 3.0 * np.array([np.cos(a), np.sin(a)])
    player = np.where(carried[:, None], pos + (0.6, 0.4), (52.5, 34.0) - 0.2 * (pos - (52.5, 34.0)))
    values, frames, columns = table(noisy, [(1.0, 34.0), player])
    return dict(values=values, frames=frames, columns=columns, truth=vel, changes=changes, displaced=sorted(displaced), fps=fps)


DEMO_SEED = 0
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def params_of(case):
    kw = dict(case["params"])
    return FR.params(kw.pop("fps"), kw.pop("max_gap"), **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the contract's result of a case, computed once and shared"""
    c = BY_NAME[name]
    out = FR.flights(c["values"], c["frames"], c["columns"], params_of(c), c["cuts"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
