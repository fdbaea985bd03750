"""Constructed velocity tables for the physical-report entries (include/eagle.h eagle_op_physical / eagle_post_physical; contract:
tests/physical_ref.py), each named after the edge it forces (tests/test_physical_cpu.py asserts through the contract that it does).  A scripted table
gives every person a speed per row (None: the cell is absent, NaN); the velocity is (s, 0), (0, s) or (-s, 0), whose length is s exactly, so a speed can
sit on an edge or one ulp below it.  Between the persons stand a ball column and video columns with velocities of their own, which nothing may read.  The
row counts put run heads, tails and the effort compaction on both sides of the scan kernel's seams: the wave (64 rows) and the workgroup, which is also
the chunk the scan walks (1024 rows).  reference(name) is computed once and shared."""
import functools

import numpy as np

import physical_ref as PR

P, G, BALL, BND = PR.PLAYER, PR.GOALKEEPER, PR.BALL, PR.BOUNDARY
NAN = float("nan")
BOUNDS = [(BND, k, 0) for k in range(4)]
ROWS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
PERSONS = (0, 1, 3)
GK_ID = 900
FPS, MIN_FRAMES = 10, (5, 3)           # the scripted cases' defaults: max_gap = fps


def _case(name, vel, frames, columns, fps=FPS, max_gap=None, zone_edges=PR.ZONE_EDGES, effort_speed=PR.EFFORT_SPEED, accel=PR.ACCEL_EDGE, min_frames=MIN_FRAMES):
    frames = np.asarray(frames, np.int32)
    assert len(frames) == vel.shape[1] and len(columns) == vel.shape[0]
    return {"name": name, "velocities": vel, "frames": frames, "columns": columns, "fps": fps, "max_gap": fps if max_gap is None else max_gap,
            "zone_edges": tuple(zone_edges), "effort_speed": tuple(effort_speed), "accel": accel, "min_frames": tuple(min_frames)}


def person_columns(n):
    """BOUNDS, then per person the pitch column and its video column; the ball and its video column stand behind the first person; the last of three or
    more persons is a goalkeeper"""
    cols = list(BOUNDS)
    for i in range(n):
        kind, cid = (G, GK_ID) if (n >= 3 and i == n - 1) else (P, i + 1)
        cols += [(kind, cid, 0), (kind, cid, 1)]
        if i == 0:
            cols += [(BALL, 0, 0), (BALL, 0, 1)]
    if n == 0:
        cols += [(BALL, 0, 0), (BALL, 0, 1), (P, 7, 1)]
    return cols


def col_of(k):
    """table column of scripted person k"""
    return 4 if k == 0 else 6 + 2 * k


def _fill(cols, rows):
    """every column that is no person carries finite velocities of its own (a ball at 30 m/s, video points at hundreds of px/s)"""
    v = np.full((len(cols), rows, 2), NAN, np.float64)
    row = np.arange(rows, dtype=np.float64)
    for c, (kind, cid, video) in enumerate(cols):
        if video or kind not in (P, G):
            v[c, :, 0], v[c, :, 1] = 30.0 + 0.125 * (row % 16), 200.0 * video - 9.0
    return v


def scripted(name, scripts, frames=None, **kw):
    """scripts: per person a list of speeds (None: absent)"""
    n, rows = len(scripts), len(scripts[0])
    cols = person_columns(n)
    v = _fill(cols, rows)
    for k, sc in enumerate(scripts):
        assert len(sc) == rows
        for r, s in enumerate(sc):
            if s is not None:
                v[col_of(k), r] = ((s, 0.0), (0.0, s), (-s, 0.0))[(r + k) % 3]
    return _case(name, v, np.arange(rows) if frames is None else frames, cols, **kw)


def walkers(name, count, rows, seed, **kw):
    """`count` persons whose speed is a random walk between 0 and 10 m/s with a random heading, absent now and then; frame steps of 1, 2 and, rarely,
    max_gap + 1"""
    r = np.random.default_rng(seed)
    cols = person_columns(count)
    v = _fill(cols, rows)
    for k in range(count):
        s = np.abs(np.cumsum(r.normal(0.0, 0.6, rows)) + r.uniform(0.0, 8.0)) % 10.0
        th = r.uniform(0.0, 2.0 * np.pi, rows)
        v[col_of(k), :, 0], v[col_of(k), :, 1] = s * np.cos(th), s * np.sin(th)
        v[col_of(k), r.random(rows) < 0.03] = NAN
    fps = kw.get("fps", FPS)
    step = r.choice([1, 1, 1, 1, 2, kw.get("max_gap", fps), kw.get("max_gap", fps) + 1], rows, p=[0.3, 0.3, 0.2, 0.1, 0.06, 0.02, 0.02])
    return _case(name, v, np.cumsum(step), cols, **kw)


def _run(rows, spans, hot=8.0, cold=1.0):
    """a script cold everywhere but on the inclusive row spans"""
    sc = [cold] * rows
    for a, b in spans:
        for r in range(a, b + 1):
            sc[r] = hot
    return sc


def _saw(rows, period=4, step=1.0):
    """speed up for `period` rows by `step` per row, down for `period` rows: accelerations and decelerations alternate"""
    return [step * (r % (2 * period) if r % (2 * period) <= period else 2 * period - r % (2 * period)) for r in range(rows)]


def _build():
    cases = []
    for rows in ROWS:
        for n in PERSONS:
            cases.append(walkers("walk_%d_rows_%d_persons" % (rows, n), n, rows, 1000 + 7 * rows + n))
    one_ulp = float(np.nextafter(5.5, 0.0))
    cases += [
        scripted("run_across_lanes_63_64", [_run(130, [(58, 70)])]),
        scripted("run_across_rows_1023_1024", [_run(1100, [(1019, 1030)]), _run(1100, [(1023, 1028)]), _run(1100, [(1024, 1030)])]),
        scripted("run_over_two_chunks", [_run(3200, [(1000, 3100)])]),
        scripted("run_from_row_0", [_run(40, [(0, 9)])]),
        scripted("run_to_the_last_row", [_run(1025, [(1015, 1024)])]),
        scripted("all_rows_hot", [_run(1025, [(0, 1024)])]),
        scripted("no_row_hot", [_run(130, [])]),
        # person 0: 5.5 exactly (a high-speed run, zone 3); person 1: one ulp below (no run, zone 2); person 2: 2.0 and one ulp below it (zones 1 and 0)
        scripted("speed_on_an_edge", [_run(20, [(5, 12)], hot=5.5), _run(20, [(5, 12)], hot=one_ulp), _run(20, [(5, 12)], hot=2.0, cold=float(np.nextafter(2.0, 0.0)))]),
        # min_frames = 5 for the speed kinds: rows 10 .. 15 last exactly 5 frames, rows 30 .. 34 one frame less
        scripted("duration_exactly_min_frames", [_run(50, [(10, 15), (30, 34)])]),
        # frames step by max_gap (10) between rows 12 and 13 (the run goes on) and by max_gap + 1 between rows 32 and 33 (two runs)
        scripted("step_of_max_gap", [_run(50, [(8, 18), (26, 40)])],
                 frames=np.cumsum([1] * 13 + [10] + [1] * 19 + [11] + [1] * 16) - 1),
        scripted("absent_cell_splits_a_run", [[None if r == 20 else s for r, s in enumerate(_run(40, [(10, 30)]))]]),
        scripted("accelerations_alternate", [_saw(1100, 5), _saw(1100, 3, 1.5)], min_frames=(5, 1)),
        # fps 1, steps of one frame, both speeds (k + 0.5) / 2^20: d 2^20 = k + 0.5 exactly, q = k + 1
        scripted("half_quantum", [[(k + 0.5) / PR.Q for k in (0, 0, 1, 1, 2, 2, 7, 7, 1000, 1000)]], fps=1, max_gap=1, min_frames=(1, 1)),
        # 2e7 m/s: 2e6 m in a step, just beyond the clamp; 1e150 m/s: finite, far beyond it
        scripted("distance_clamp", [[1.0, 1.0, 1e150, 1e150, 1.0, 1.0, 2e7, 2e7, 1.0]], min_frames=(1, 1)),
        # pairs of present rows between absent ones, and a pair parted by a hole in the frame numbers
        scripted("one_sided_neighbours", [[1.0, 4.0, None, 6.0, 2.0, None, 3.0, 9.0, 1.0, 5.0, None, None, 7.0]],
                 frames=[0, 1, 2, 3, 4, 5, 6, 7, 30, 31, 32, 33, 34], min_frames=(1, 1)),
    ]
    return cases


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def args(c):
    return (c["velocities"], c["frames"], c["columns"], c["fps"], c["max_gap"], c["zone_edges"], c["effort_speed"], c["accel"], c["min_frames"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """the contract's answer for a case, computed once and never changed by a test"""
    return PR.physical(*args(BY_NAME[name]))
