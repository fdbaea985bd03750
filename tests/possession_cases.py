"""Constructed tables for the possession entries (include/eagle.h eagle_op_possession / eagle_post_possession; contract: tests/possession_ref.py), each
named after the edge it forces (tests/test_possession_cpu.py asserts through the contract that it does).  A scripted table has a few persons standing
10 m apart (drifting a little, so every row's coordinates differ), the ball per row next to one of them (an int: the person's index), loose (-1: 20 m
from everybody) or absent (None: NaN).  The row counts put run heads, confirmations, owner changes and the event compaction on both sides of the scan
kernel's seams: the wave (64 rows) and the workgroup, which is also the chunk the scan walks (1024 rows).  reference(name) is computed once and shared."""
import functools

import numpy as np

import possession_ref as PR

P, G, BALL, BND = PR.PLAYER, PR.GOALKEEPER, PR.BALL, PR.BOUNDARY
NAN = float("nan")
BOUNDS = [(BND, k, 0) for k in range(4)]
ROWS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097)
GK_ID = 900


def _case(name, values, frames, columns, mapping, fps=5, radius=PR.RADIUS, min_hold=PR.MIN_HOLD, max_gap=None, no_ball=False):
    frames = np.asarray(frames, np.int32)
    assert len(frames) == values.shape[1] and len(columns) == values.shape[0]
    return {"name": name, "values": values, "frames": frames, "columns": columns, "mapping": mapping, "fps": fps, "radius": radius, "min_hold": min_hold,
            "max_gap": fps if max_gap is None else max_gap, "no_ball": no_ball}


def person_columns(n, goalkeeper=True):
    """BOUNDS, then per person the pitch column and its video column, a goalkeeper (the last person, no mapping entry), the ball and its video column"""
    cols = BOUNDS + [c for i in range(n) for c in ((P, i + 1, 0), (P, i + 1, 1))]
    if goalkeeper:
        cols += [(G, GK_ID, 0), (G, GK_ID, 1)]
    return cols + [(BALL, 0, 0), (BALL, 0, 1)]


def col_of(k):
    """table column of scripted person k (the goalkeeper is person n)"""
    return 4 + 2 * k


def scripted(name, script, n=3, frames=None, mapping="teams", goalkeeper=True, **kw):
    rows = len(script)
    cols = person_columns(n, goalkeeper)
    v = np.full((len(cols), rows, 2), NAN, np.float64)
    np_ = n + (1 if goalkeeper else 0)
    row = np.arange(rows, dtype=np.float64)
    for k in range(np_):
        v[col_of(k), :, 0], v[col_of(k), :, 1] = 10.0 * k + 5.0 + 0.0078125 * (row % 64), 20.0 + 0.00390625 * (row % 128)
        v[col_of(k) + 1, :] = v[col_of(k), :] * 12.0                        # a video point: never a candidate
    b = len(cols) - 2
    for r, who in enumerate(script):
        if who is None:
            continue
        v[b, r] = (v[col_of(who), r, 0] + 0.5, v[col_of(who), r, 1] + 0.25) if who >= 0 else (7.0 + 0.015625 * (r % 32), 40.0)
    v[b + 1, :] = (640.0, 360.0)
    if mapping == "teams":
        mapping = {i + 1: i % 2 for i in range(n)}
    return _case(name, v, np.arange(rows) if frames is None else frames, cols, mapping, **kw)


def walkers(name, count, rows, seed, **kw):
    """`count` players on a random walk, the ball hopping between them, loose or absent at random; a few person cells NaN"""
    r = np.random.default_rng(seed)
    cols = BOUNDS + [(P, i + 1, 0) for i in range(count)] + [(G, GK_ID, 0), (BALL, 0, 0), (P, 5000, 1)]
    v = np.full((len(cols), rows, 2), NAN, np.float64)
    pos = np.stack([r.uniform(0, 105, count + 1), r.uniform(0, 68, count + 1)], 1)
    who = 0
    for row in range(rows):
        pos = pos + r.normal(0, 0.2, pos.shape)
        v[4:5 + count, row] = pos
        u = r.random()
        if u < 0.25:
            who = int(r.integers(0, count + 1))
        if u < 0.85:
            v[5 + count, row] = pos[who] + r.normal(0, 0.9, 2)
        elif u < 0.95:
            v[5 + count, row] = (r.uniform(0, 105), r.uniform(0, 68))
        if r.random() < 0.1:
            v[4 + int(r.integers(0, count + 1)), row, int(r.integers(0, 2))] = NAN
    v[-1, :] = (1.0, 1.0)
    return _case(name, v, np.cumsum(r.integers(1, 4, rows)), cols, {i + 1: (0, 1, -1)[i % 3] for i in range(0, count, 1) if i % 7 != 6}, **kw)


def _gap_frames(rows, at, gap):
    f = np.arange(rows)
    f[at:] += gap - 1
    return f


def _cases():
    out = []
    A, B, C, L, X = 0, 1, 2, -1, None
    # ---- who takes part ----
    cols = BOUNDS + [(BALL, 0, 0), (BALL, 0, 1)]
    v = np.full((len(cols), 5, 2), NAN)
    v[4, :], v[5, :] = (50.0, 30.0), (600.0, 300.0)
    out.append(_case("no_person_columns", v, np.arange(5), cols, {1: 0}))
    out.append(scripted("one_person", [A, A, A, L, A, A], n=1, goalkeeper=False))
    out.append(walkers("persons22", 21, 130, 3))
    out.append(walkers("persons257", 256, 70, 4, min_hold=1))
    c = scripted("x", [A, A, B, B], n=2)
    keep = [i for i, k in enumerate(c["columns"]) if k[0] != BALL]
    out.append(_case("no_ball_column", c["values"][keep].copy(), c["frames"], [c["columns"][i] for i in keep], c["mapping"]))
    c = scripted("x", [X, X, X, X], n=2)
    out.append(_case("no_ball_flag", c["values"], c["frames"], c["columns"], c["mapping"], no_ball=True))
    out.append(scripted("ball_absent_first_row", [X, A, A, A, B, B], n=2))
    out.append(scripted("ball_absent_last_row", [A, A, A, B, B, X], n=2))
    out.append(scripted("ball_absent_interior_rows", [A, A, X, A, A, B, B, X, X, B, B, A, A], n=2))
    c = scripted("person_nan_where_they_would_win", [A, A, A, A, B, B], n=2)
    c["values"][col_of(A), 2, 0] = NAN                 # row 2: A's x is missing, B (10 m away) is the nearest and outside the radius
    c["values"][col_of(A), 3, 1] = float("inf")
    out.append(c)
    # ---- ties and the radius ----
    cols = BOUNDS + [(P, 1, 0), (P, 2, 0), (BALL, 0, 0)]
    v = np.full((len(cols), 4, 2), NAN)
    v[6, :] = (30.0, 20.0)
    v[4, :2], v[5, :2] = (31.5, 20.0), (28.5, 20.0)    # rows 0, 1: +1.5 in the earlier column, -1.5 in the later
    v[4, 2:], v[5, 2:] = (28.5, 20.0), (31.5, 20.0)    # rows 2, 3: the other way round: still the earlier column
    out.append(_case("equidistant_earlier_column_wins", v, np.arange(4), cols, {1: 0, 2: 0}))
    cols = BOUNDS + [(P, 1, 0), (BALL, 0, 0)]
    v = np.full((len(cols), 4, 2), NAN)
    v[5, :] = (10.0, 10.0)
    v[4, 0], v[4, 1], v[4, 2], v[4, 3] = (12.0, 10.0), (np.nextafter(12.0, 13.0), 10.0), (10.0, 8.0), (10.0, np.nextafter(8.0, 7.0))
    out.append(_case("distance_at_radius_and_one_ulp_beyond", v, np.arange(4), cols, {1: 0}, radius=2.0, min_hold=1))
    # ---- min_hold ----
    s = [A] * 6 + [B] * 6 + [L] * 2 + [C] * 7 + [A] * 3
    for mh in (1, 2, 5, len(s) + 1):
        out.append(scripted("min_hold_%s" % ("beyond_rows" if mh > len(s) else mh), s, min_hold=mh))
    out.append(scripted("run_broken_one_short", [A] * 5 + [B] * 4 + [A] + [B] * 4 + [L] + [B] * 5, min_hold=5))
    # ---- frame gaps: exactly max_gap and one more, inside a run, inside a flight, at an owner change ----
    for gap, tag in ((5, "exact"), (6, "beyond")):
        out.append(scripted("gap_%s_inside_run" % tag, [A, A, A, A, A, B, B], frames=_gap_frames(7, 3, gap), n=2, max_gap=5))
        out.append(scripted("gap_%s_inside_flight" % tag, [A, A, L, L, B, B, B], frames=_gap_frames(7, 3, gap), n=2, max_gap=5))
        out.append(scripted("gap_%s_at_owner_change" % tag, [A, A, B, B, A], frames=_gap_frames(5, 2, gap), n=2, max_gap=5, min_hold=1))
    # ---- kinds ----
    out.append(scripted("change_within_team", [A, A, C, C, A, A], n=3))                       # teams 0, 1, 0
    out.append(scripted("change_across_teams", [A, A, B, B, C, C], n=3))
    out.append(scripted("change_unknown_team", [A, A, 3, 3, B, B, C, C, A, A], n=3, mapping={1: 0, 2: -1, 3: 0}))      # person 3: the goalkeeper, no entry; id 2: below 0
    out.append(scripted("no_mapping", [A, A, B, B, A, A], n=2, mapping=None))
    out.append(scripted("a_loose_a", [A, A, L, L, L, A, A, L, A], n=2))
    # ---- every seam ----
    for n in ROWS:
        out.append(scripted("alternating_%d" % n, [(A, B)[r % 2] for r in range(n)], n=2, min_hold=1, fps=25))
        out.append(walkers("random_%d" % n, 5, n, 100 + n, min_hold=(1, 2, 3)[n % 3], fps=25, max_gap=2))
    for mh in (2, 3):
        s = [A] * 4200
        for seam, j in ((64, 0), (128, 1), (192, 2), (1024, 0), (2048, 1), (3072, 2), (4096, 1)):
            s[seam - j:seam - j + mh] = [B] * mh       # a run of B whose head (j = 0) or confirmation (j = min_hold - 1) falls on the seam's first row
        out.append(scripted("seams_hold%d" % mh, s, n=2, min_hold=mh, fps=25))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
for _c in CASES:
    _c["values"].setflags(write=False)


def args(c):
    return (c["values"], c["frames"], c["columns"], c["mapping"], c["fps"], c["radius"], c["min_hold"], c["max_gap"])


@functools.lru_cache(maxsize=None)
def reference(name):
    c = BY_NAME[name]
    res = PR.possession(*args(c), no_ball=c["no_ball"])
    for k, a in res.items():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res


# A table whose aggregates are worked out by hand (tests/test_possession_cpu.py): persons 1, 2 (teams 0, 1), 3 (team 0), fps 5, min_hold 2, frames with
# one step of 2.  Rows: A A A L B B C C C A A  ->  owner: - A A A A B B C C C A  (confirmed on the second row of each run)
def hand_table():
    s = [0, 0, 0, -1, 1, 1, 2, 2, 2, 0, 0]
    f = np.array([0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11])
    return scripted("hand", s, n=3, frames=f, goalkeeper=False, fps=5, max_gap=5)
