"""Constructed tables for the minimap's trail, pass-arrow and owner layers and the two stills (include/eagle.h eagle_op_minimap_trails /
eagle_op_trajectory_picture / eagle_op_pass_picture; contract: tests/trails_ref.py), each named after the edge it forces.  S = 2, M = 0 -> 210 x 136 (one
tile column, nine tile rows); S = 4, M = 8 -> 436 x 288 (the x tile seam at 256).  Points are given in sixteenths of a pixel and turned into metres that
quantise back exactly (S is a power of two).  reference(name) is computed once per case and shared by the tests."""
import functools

import numpy as np

import minimap_ref as R
import trails_ref as T

P, G, BALL, BND = R.PLAYER, R.GOALKEEPER, R.BALL, R.BOUNDARY
NAN, INF = float("nan"), float("inf")
EVENT_DTYPE = np.dtype([("row", "<i4"), ("from_col", "<i4"), ("to_col", "<i4"), ("release_row", "<i4"), ("receive_row", "<i4"), ("kind", "<i4"),
                        ("reserved", "<i4", 2), ("x0", "<f8"), ("y0", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("length", "<f8"),
                        ("duration", "<f8")])                   # include/eagle.h EaglePossessionEvent
SMALL, LARGE = (2, 0), (4, 8)
# found by a search over segments right of the canvas (tests/test_trails_cpu.py checks that the wrapped product changes a pixel)
WIDE = ((1006.0, 963.0), (1015.0, -1017.0))
MM_CHUNK = 256                                                  # csrc/minimap.hip: list entries staged per trip


def metres(q, S, M):
    """a point in sixteenths of a pixel -> pitch metres that quantise to it"""
    return (q[0] - 16 * M) / (16.0 * S), (16 * M + 16 * 68 * S - q[1]) / (16.0 * S)


def events(rows):
    """[(release_row, receive_row, kind, (x0, y0), (x1, y1), from_col, to_col)] -> EVENT_DTYPE"""
    ev = np.zeros(len(rows), EVENT_DTYPE)
    for k, (rel, rec, kind, a, b, fc, tc) in enumerate(rows):
        ev[k]["row"], ev[k]["release_row"], ev[k]["receive_row"], ev[k]["kind"], ev[k]["from_col"], ev[k]["to_col"] = rec, rel, rec, kind, fc, tc
        ev[k]["x0"], ev[k]["y0"], ev[k]["x1"], ev[k]["y1"] = a[0], a[1], b[0], b[1]
    return ev


def _case(name, values, columns, mapping, SM, layers=T.TRAILS, p=None, sel=(), owner=None, ev=None, frames=None, row0=None, n=1, **kw):
    rows = values.shape[1]
    return {"name": name, "values": values, "frames": np.arange(rows, dtype=np.int32) if frames is None else np.asarray(frames, np.int32), "columns": columns,
            "mapping": mapping, "S": SM[0], "M": SM[1], "row0": rows - n if row0 is None else row0, "n": n, "layers": layers, "p": T.trail_params(**(p or {})),
            "sel": list(sel), "owner": None if owner is None else np.asarray(owner, np.int32), "events": ev, "kw": kw}


def seg_case(name, SM, a, b, hw, **extra):
    """one mapped player, two rows: the one segment a -> b (sixteenths) on the picture of row 1; seg = its end points for the tests"""
    v = np.full((1, 2, 2), NAN)
    v[0, 0], v[0, 1] = metres(a, *SM), metres(b, *SM)
    c = _case(name, v, [(P, 1, 0)], {1: 0}, SM, p=dict(window=1, half_width=hw, dim_floor=256), sel=[0], footprint=0)
    c.update(seg=(a[0], a[1], b[0], b[1], 16 * hw), **extra)
    return c


def walk(seed, rows, ncols, SM, step=1.5, start=None):
    """random walks on the pitch, float64 [ncols][rows][2]"""
    r = np.random.default_rng(seed)
    v = np.zeros((ncols, rows, 2))
    v[:, 0] = r.uniform((10, 10), (95, 58), (ncols, 2)) if start is None else start
    for j in range(1, rows):
        v[:, j] = np.clip(v[:, j - 1] + r.uniform(-step, step, (ncols, 2)), (1, 1), (104, 67))
    return v


WALK_COLS = [(P, 1, 0), (P, 1, 1), (P, 99, 0), (G, 3, 0), (BALL, 0, 0), (P, 2, 0)]      # (99 has no mapping entry; column 1 is a video column)
WALK_MAP = {1: 0, 2: 1}


def walk_case(name, SM=SMALL, rows=8, sel=(0, 3, 4, 5), mapping=WALK_MAP, edit=None, **kw):
    v = walk(7, rows, len(WALK_COLS), SM)
    if edit:
        edit(v)
    return _case(name, v, WALK_COLS, mapping, SM, sel=sel, **kw)


def count_case(count, W, C):
    rows = W + 1
    cols = [(P, i + 1, 0) for i in range(C)]
    v = walk(100 + count, rows, C, SMALL, step=0.6)
    c = _case("count_%d" % count, v, cols, None if C else {}, SMALL, p=dict(window=W, dim_floor=32, max_gap=2), sel=range(max(C, 1)) if C else [0], footprint=0)
    if not C:                                                   # the one selected player has no mapping entry: a trail layer of no entries
        c["values"], c["columns"], c["frames"] = walk(100, 3, 1, SMALL), [(P, 1, 0)], np.arange(3, dtype=np.int32)
        c["row0"] = 2
    c["count"] = count
    return c


def _ball_table(SM, rows, seed=3):
    cols = [(P, 1, 0), (P, 2, 0), (G, 3, 0), (BALL, 0, 0), (P, 99, 0)]
    return walk(seed, rows, len(cols), SM), cols, {1: 0, 2: 1}


def event_case(name, SM, rows, evs, p=None, row0=None, n=1, layers=T.PASSES, **kw):
    v, cols, mp = _ball_table(SM, rows)
    return _case(name, v, cols, mp, SM, layers=layers, p=dict(dict(pass_hold=3, half_width=2), **(p or {})), ev=events(evs), row0=row0, n=n, **kw)


def _cases():
    out = []
    # ---- geometry ----
    out.append(seg_case("horizontal", SMALL, (320, 800), (1600, 800), 2, at=(50, 48), beyond=(50, 47)))      # (50, 48) lies exactly 32 sixteenths above the line
    out.append(seg_case("beyond_straight", SMALL, (320, 801), (1600, 801), 2, beyond=(50, 48)))             # one sixteenth further
    out.append(seg_case("vertical", SMALL, (1600, 300), (1600, 1700), 1))
    out.append(seg_case("diagonal", SMALL, (300, 300), (2900, 1900), 3))
    out.append(seg_case("zero_length", SMALL, (1600, 1000), (1600, 1000), 4))
    out.append(seg_case("x_seam", LARGE, (3900, 1000), (4300, 1000), 2))
    out.append(seg_case("y_seam", SMALL, (500, 200), (500, 300), 2))
    out.append(seg_case("both_seams", LARGE, (3900, 200), (4300, 300), 2))
    out.append(seg_case("oblique_at", SMALL, (1600, 800), (1696, 928), 5, at=(99, 57)))                     # d = 2 (48, 64); (1584, 912) = A + d / 2 + 80 (-0.8, 0.6)
    out.append(seg_case("oblique_beyond", SMALL, (1601, 800), (1697, 928), 5, beyond=(99, 57)))
    out.append(seg_case("half_width_1", LARGE, (1000, 1000), (5000, 3000), 1))
    out.append(seg_case("half_width_8", LARGE, (1000, 3000), (5000, 1000), 8))
    out.append(seg_case("endpoint_off_canvas", SMALL, (1600, 800), (-500, 2600), 2))
    far = _case("far_line", np.array([[(-1024.0, -1000.0), (1024.0, 1024.0)]]), [(P, 1, 0)], {1: 1}, LARGE, p=dict(window=1, half_width=2, dim_floor=256), sel=[0], footprint=0)
    out.append(far)
    # a segment far to the right of the canvas: for every pixel cross^2 >= 2^64; the true picture has none of it, the 64-bit wrap lights pixels
    wide = _case("wide_product", np.array([[WIDE[0], WIDE[1]]]), [(P, 1, 0)], {1: 0}, LARGE, p=dict(window=1, half_width=8, dim_floor=256), sel=[0], footprint=0)
    out.append(wide)

    # ---- presence and window ----
    def hole(v):
        v[0, 3] = (NAN, 30.0); v[3, 4] = (40.0, INF); v[5, 2] = (1025.0, 10.0)
    out.append(walk_case("nan_inf_beyond_domain", edit=hole, p=dict(window=7), row0=0, n=8))
    out.append(walk_case("gap_at_and_beyond", frames=[0, 1, 2, 5, 6, 10, 11, 12], p=dict(window=8, max_gap=3), row0=5, n=3))
    out.append(walk_case("row_0_and_r_below_W", p=dict(window=5), row0=0, n=4))
    out.append(walk_case("window_1", p=dict(window=1), row0=1, n=3))
    out.append(walk_case("window_beyond_rows", p=dict(window=1000000, dim_floor=0), row0=6, n=2))
    out.append(walk_case("unmapped_player", sel=(2, 0), p=dict(window=4)))
    out.append(walk_case("no_mapping", mapping=None, sel=(0, 2, 5), p=dict(window=4)))
    out.append(walk_case("goalkeeper_and_ball", sel=(4, 3), p=dict(window=6, half_width=2)))

    # ---- W x C entries against the chunk ----
    out += [count_case(0, 2, 0), count_case(1, 1, 1), count_case(255, 51, 5), count_case(256, 64, 4), count_case(257, 257, 1), count_case(769, 769, 1)]

    # ---- order ----
    cols = [(P, 1, 0), (P, 2, 0)]
    v = np.array([[(20.0, 20.0), (60.0, 50.0)], [(20.0, 50.0), (60.0, 20.0)]])
    out.append(_case("two_columns_cross", v, cols, {1: 0, 2: 1}, SMALL, p=dict(window=1, half_width=3), sel=[0, 1]))
    out.append(_case("two_columns_cross_swapped", v, cols, {1: 0, 2: 1}, SMALL, p=dict(window=1, half_width=3), sel=[1, 0]))
    v = np.array([[(20.0, 20.0), (60.0, 50.0), (60.0, 20.0), (20.0, 50.0)]])
    for floor in (0, 64, 256):
        out.append(_case("self_crossing_floor_%d" % floor, v, [(P, 1, 0)], {1: 1}, SMALL, p=dict(window=3, half_width=3, dim_floor=floor), sel=[0]))

    # ---- events ----
    a, b, c, d = (20.0, 20.0), (70.0, 50.0), (80.0, 10.0), (30.0, 60.0)
    out.append(event_case("three_kinds", SMALL, 6, [(1, 2, 0, a, b, 0, 1), (2, 3, 1, b, c, 1, 0), (3, 4, 2, c, d, 0, 4)], row0=3))
    out.append(event_case("zero_length_arrow", SMALL, 4, [(1, 2, 0, b, b, 0, 1)], row0=2))
    out.append(event_case("absent_release_cell", SMALL, 4, [(1, 2, 0, (NAN, 20.0), b, 0, 1), (1, 2, 1, c, (5000.0, 1.0), 1, 0)], row0=2))
    out.append(event_case("arrow_across_both_seams", LARGE, 4, [(1, 2, 0, metres((3700, 150), *LARGE), metres((4500, 420), *LARGE), 0, 1)], row0=2, p=dict(half_width=1)))
    out.append(event_case("hold_1", SMALL, 6, [(1, 3, 0, a, b, 0, 1)], p=dict(pass_hold=1), row0=0, n=6))
    out.append(event_case("two_visible_in_order", SMALL, 6, [(1, 2, 0, a, b, 0, 1), (2, 3, 1, d, c, 1, 0)], row0=3))
    r = np.random.default_rng(5)
    many = [(k, k + 1, k % 3, tuple(r.uniform((0, 0), (105, 68))), tuple(r.uniform((0, 0), (105, 68))), 0, 1) for k in range(257)]
    out.append(event_case("events_257_visible", SMALL, 259, many, p=dict(pass_hold=300, half_width=1), row0=257))
    out.append(event_case("before_and_after_events", SMALL, 9, [(3, 4, 0, a, b, 0, 1)], p=dict(pass_hold=2), row0=0, n=9))

    # ---- owner ----
    v, cols, mp = _ball_table(SMALL, 6)
    v[1, 3] = (NAN, NAN)
    out.append(_case("owner_kinds", v, cols, mp, SMALL, layers=T.OWNER, owner=[-1, 0, 2, 1, 4, 1], row0=0, n=6))      # row 3: the owner's cell is absent; row 4: no mapping entry
    out.append(_case("owner_radius_7", v, cols, mp, LARGE, layers=T.OWNER, owner=[0] * 6, row0=5, player_radius=7))

    # ---- the layers together ----
    bcols = [(BND, k, 0) for k in range(4)] + [(P, 1, 0), (P, 2, 0), (G, 3, 0), (BALL, 0, 0)]
    v = np.concatenate([np.zeros((4, 5, 2)), walk(9, 5, 4, SMALL, step=4.0)])
    for k, (x, y) in enumerate(((20.0, 0.0), (5.0, 68.0), (90.0, 68.0), (75.0, 0.0))):
        v[k, :] = (x, y)
    evs = events([(1, 2, 0, tuple(v[7, 1]), tuple(v[7, 2]), 4, 5), (3, 4, 1, tuple(v[7, 3]), tuple(v[7, 4]), 5, 4)])
    allp = dict(window=3, half_width=2, pass_hold=2)
    own = [4, 4, 5, 5, 6]
    out.append(_case("all_with_voronoi", v, bcols, {1: 0, 2: 1}, SMALL, layers=7, p=allp, sel=[4, 5, 7], owner=own, ev=evs, row0=0, n=5, voronoi=1, footprint=0))
    out.append(_case("all_with_footprint", v, bcols, {1: 0, 2: 1}, LARGE, layers=7, p=allp, sel=[7, 6, 4], owner=own, ev=evs, row0=2, n=3))

    # ---- pictures per call ----
    out.append(walk_case("pictures_3", p=dict(window=4), row0=3, n=3))
    out.append(walk_case("pictures_65", rows=70, p=dict(window=10, half_width=2), row0=5, n=65))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
YUV_CASES = ["all_with_voronoi", "pictures_3", "three_kinds"]
PADDED_CASE = "all_with_voronoi"

# ---- stills ----
TRAJ = [("window_1_row", dict(row0=3, n=1)), ("window_2_rows", dict(row0=2, n=2)), ("window_with_hole", dict(row0=0, n=8))]


def trajectory_case(name):
    kw = dict(TRAJ)[name]

    def hole(v):
        v[0, 3] = (NAN, NAN); v[4, 0] = (NAN, 1.0); v[4, 7] = (INF, 1.0); v[3, :] = NAN
    c = walk_case("trajectory_" + name, SM=SMALL, edit=hole, sel=(0, 2, 3, 4, 5))
    c.update(kw, half_width=2, max_gap=25)
    return c


def pass_case():
    """the passer (column 0) and the receiver (column 2) are the same distance either side of a bystander (column 1): their discs overlap its"""
    cols = [(P, 1, 0), (P, 2, 0), (P, 3, 0), (BALL, 0, 0), (G, 4, 0)]
    v = np.zeros((5, 3, 2))
    v[0, :], v[1, :], v[2, :], v[3, :], v[4, :] = (49.0, 34.0), (50.0, 34.0), (51.0, 34.0), (49.0, 36.0), (5.0, 30.0)
    ev = events([(1, 2, 0, (49.0, 36.0), (80.0, 50.0), 0, 2), (1, 2, 1, (10.0, 10.0), (20.0, 20.0), 2, 0)])
    return {"name": "pass_overlap", "values": v, "frames": np.arange(3, dtype=np.int32), "columns": cols, "mapping": {1: 0, 2: 1, 3: 0}, "S": 4, "M": 8, "events": ev,
            "event": 0, "half_width": 2}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the contract's BGR pictures of a case, uint8 [n, h, w, 3] (read only: shared by the tests)"""
    c = BY_NAME[name]
    fr = T.frames_bgr(c["values"], c["frames"], c["columns"], c["mapping"], c["row0"], c["n"], c["S"], c["M"], layers=c["layers"], p=c["p"], sel=c["sel"],
                      owner=c["owner"], events=c["events"], **c["kw"])
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def trajectory_reference(name):
    c = trajectory_case(name)
    return T.trajectory_picture(c["values"], c["frames"], c["columns"], c["mapping"], c["sel"], c["row0"], c["n"], c["S"], c["M"], c["half_width"], c["max_gap"])


@functools.lru_cache(maxsize=None)
def pass_reference():
    c = pass_case()
    return T.pass_picture(c["values"], c["frames"], c["columns"], c["mapping"], c["events"], c["event"], c["S"], c["M"], c["half_width"])
