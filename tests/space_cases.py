"""Constructed tables for the space stage (include/eagle.h eagle_op_space; contract: tests/space_ref.py), each named after what it forces; "check" says, on
the contract's result (records [rows], sites [rows, 32], totals [members], owner maps [rows, gh, gw] of ALL rows), that it does
(tests/test_space_cpu.py asserts every one).  reference(name) is computed once per case and shared by the tests.  Cases at 4 cells per metre stay at or
below 8 rows; cases with many rows run at 1 cell per metre with few sites.  The sites kernel takes 4 rows per workgroup and 64 member columns per step, the
totals kernel 64 rows per wave (csrc/space.hip): 63, 65 and 257 rows and 70 members cross those boundaries."""
import functools

import numpy as np

import minimap_ref as R_
import space_ref as SR

P, G, BALL, BOUNDARY = R_.PLAYER, R_.GOALKEEPER, R_.BALL, R_.BOUNDARY
NAN, INF = float("nan"), float("inf")
BEYOND = float(np.nextafter(1024.0, INF))


def _case(name, values, columns, mapping, p, check=None):
    return {"name": name, "values": np.asarray(values, np.float64), "columns": columns, "mapping": mapping, "p": p, "check": check or (lambda rec, st, tot, grid: True)}


def still(pts, rows=1):
    """[(x, y)] per column -> values [len(pts)][rows][2], everybody standing"""
    return np.repeat(np.array(pts, np.float64)[:, None, :], rows, 1)


def players(teams, ids0=1):
    """[team per column] -> (columns, mapping)"""
    return [(P, ids0 + i, 0) for i in range(len(teams))], {ids0 + i: t for i, t in enumerate(teams)}


def used(st, r):
    return [s for s in st[r] if s["col"] >= 0]


def walk(seed, n_per_team, rows, holes=0.0, keepers=2):
    """two teams of n_per_team players and `keepers` goalkeepers on a random walk over (and a little beyond) the pitch, the ball and an unmapped player; the
    groups' columns interleave in the table; a share of the cells absent"""
    r = np.random.default_rng(seed)
    k = 2 * n_per_team + keepers + 2
    cols = [(P, 1 + i, 0) for i in range(2 * n_per_team)] + [(G, 900 + i, 0) for i in range(keepers)] + [(BALL, 0, 0), (P, 999, 0)]
    mp = {1 + i: (0 if i % 2 == 0 else 3) for i in range(2 * n_per_team)}
    v = np.stack([r.uniform(-3, 108, k), r.uniform(-3, 71, k)], 1)[:, None, :] + np.cumsum(r.normal(0, 1.5, (k, rows, 2)), 1)
    v[r.uniform(size=(k, rows)) < holes] = NAN
    order = r.permutation(k)
    return v[order], [cols[i] for i in order], mp


def conserves(rec, st, tot, grid):
    """every ACTIVE row: all cells add up to the grid, the map agrees with the counts; every other row: zeros and a map of 255"""
    gh, gw = grid.shape[1:]
    R = gw // 105
    third = np.where(np.arange(gw) < 35 * R, 0, np.where(np.arange(gw) < 70 * R, 1, 2))
    for r in range(len(rec)):
        if rec[r]["status"] != SR.ACTIVE:
            if rec[r]["cells"].any() or (st[r]["col"] != -1).any() or (grid[r] != SR.NO_OWNER).any():
                return False
            continue
        S = int(rec[r]["n_sites"])
        if int(rec[r]["cells"].sum()) != gw * gh or int(st[r]["cells"].sum()) != gw * gh or grid[r].max() >= S or (st[r, S:]["col"] != -1).any():
            return False
        for k in range(S):
            if [int(((grid[r] == k) & (third[None] == t)).sum()) for t in range(3)] != [int(v) for v in st[r, k]["cells"]]:
                return False
        for g in range(3):
            if [int(v) for v in rec[r]["cells"][g]] != [sum(int(s["cells"][t]) for s in st[r, :S] if s["group"] == g) for t in range(3)]:
                return False
    return True


def _cases():
    out = []
    prm = SR.space_params
    # ---- two sites mirrored about a line of cell centres: a whole column of exact ties goes to the earlier table column ----
    for R in (1, 2, 4):
        x0 = 52.0 + 0.5 / R                                     # the centre of cell column 52 R
        for swapped in (False, True):
            pts = [(x0 + 10.0, 30.0), (x0 - 10.0, 30.0)] if swapped else [(x0 - 10.0, 30.0), (x0 + 10.0, 30.0)]
            c, m = players([0, 1])

            def check(rec, st, tot, grid, R=R, swapped=swapped):
                left = (52 * R + (0 if swapped else 1)) * 68 * R          # the cells of the left-hand site, with the tie column when it is column 0
                a, b = (int(st[0, k]["cells"].sum()) for k in (0, 1))
                return (grid[0][:, 52 * R] == 0).all() and (a, b) == ((105 * 68 * R * R - left, left) if swapped else (left, 105 * 68 * R * R - left)) and conserves(rec, st, tot, grid)
            out.append(_case("tie_mirror_column_R%d%s" % (R, "_swapped" if swapped else ""), still(pts, 2), c, m, prm(R), check))
    # ---- coincident sites: the earlier column takes everything ----
    c, m = players([0, 1, 0])
    out.append(_case("coincident_sites", still([(40.0, 30.0), (70.0, 20.0), (40.0, 30.0)], 2), c, m, prm(1),
                     lambda rec, st, tot, grid: int(st[0, 2]["cells"].sum()) == 0 and int(st[0, 0]["cells"].sum()) > 0 and tot[1]["min"] == 0 and tot[1]["rows"] == 2
                     and st[0, 2]["near_col"] == 1 and conserves(rec, st, tot, grid)))
    # ---- one site owns the pitch; one group only: no opponent ----
    c, m = players([1])
    out.append(_case("one_site", still([(10.0, 10.0)], 3), c, m, prm(2),
                     lambda rec, st, tot, grid: [int(v) for v in st[1, 0]["cells"]] == [70 * 136] * 3 and (grid == 0).all() and tot[0]["opp_rows"] == 0
                     and (tot[0]["min"], tot[0]["max"]) == (210 * 136, 210 * 136)))
    c, m = players([0, 0, 0])
    out.append(_case("one_group_only", still([(10.0, 10.0), (50.0, 40.0), (90.0, 60.0)], 2), c, m, prm(1),
                     lambda rec, st, tot, grid: (st[:, :3]["near_col"] == -1).all() and (st[:, :3]["near_d2"] == -1).all() and not st["within"].any()
                     and not tot["opp_rows"].any() and list(rec[0]["n"]) == [3, 0, 0]))
    # ---- an empty row between active ones ----
    c, m = players([0, 1])
    v = still([(30.0, 30.0), (60.0, 40.0)], 3)
    v[:, 1] = NAN
    out.append(_case("empty_row_between", v, c, m, prm(1),
                     lambda rec, st, tot, grid: list(rec["status"]) == [SR.ACTIVE, SR.EMPTY, SR.ACTIVE] and (grid[1] == 255).all() and (tot["rows"] == 2).all()
                     and conserves(rec, st, tot, grid)))
    # ---- 32 sites are ACTIVE, 33 are TOO_MANY ----
    c, m = players([i % 2 for i in range(33)])
    v = still([(3.0 + 3.0 * i, 5.0 + 1.7 * i) for i in range(33)], 3)
    v[32, 0] = NAN; v[5, 2] = NAN
    out.append(_case("sites_32_active_33_too_many", v, c, m, prm(1),
                     lambda rec, st, tot, grid: list(rec["status"]) == [SR.ACTIVE, SR.TOO_MANY, SR.ACTIVE] and list(rec["n_sites"]) == [32, 33, 32]
                     and list(rec[1]["n"]) == [17, 16, 0] and not rec[1]["cells"].any() and (st[1]["col"] == -1).all() and tot[16]["rows"] == 1 and st[2, 5]["col"] == 6
                     and conserves(rec, st, tot, grid)))
    # ---- sites off the pitch and at exactly +-1024 m; one ulp beyond is absent ----
    c, m = players([0, 1, 0, 1, 0])
    v = still([(-20.0, -5.0), (1024.0, 1024.0), (-1024.0, -1024.0), (BEYOND, 30.0), (50.0, 34.0)], 2)
    v[3, 1] = (30.0, -BEYOND)
    out.append(_case("off_pitch_and_domain_edge", v, c, m, prm(1),
                     lambda rec, st, tot, grid: list(rec["n_sites"]) == [4, 4] and [int(s["col"]) for s in used(st, 0)] == [0, 1, 2, 4] and st[0, 0]["cells"].sum() > 0
                     and st[0, 2]["near_d2"] == 2 ** 43 and st[0, 2]["near_col"] == 1 and (st[0, 1]["qx"], st[0, 2]["qy"]) == (2 ** 20, -2 ** 20)
                     and conserves(rec, st, tot, grid)))
    # ---- NaN and infinite cells ----
    c, m = players([0, 1, 0, 1])
    v = still([(20.0, 20.0), (80.0, 50.0), (40.0, 10.0), (60.0, 60.0)], 2)
    v[0, 0] = (NAN, 20.0); v[1, 0] = (80.0, INF); v[2, 1] = (-INF, 1.0); v[3, 1] = (NAN, NAN)
    out.append(_case("nan_and_inf_cells", v, c, m, prm(1),
                     lambda rec, st, tot, grid: [[int(s["col"]) for s in used(st, r)] for r in (0, 1)] == [[2, 3], [0, 1]] and conserves(rec, st, tot, grid)))
    # ---- an opponent exactly at the radius is inside, one q further is outside ----
    c, m = players([0, 1])
    v = still([(50.0, 30.0), (53.0, 30.0)], 3)
    v[1, 1] = (53.0 + 1.0 / 1024.0, 30.0); v[1, 2] = (50.0, 30.0 - 2.5)
    out.append(_case("radius_inclusive", v, c, m, prm(1, 1, 3.0),
                     lambda rec, st, tot, grid: [int(st[r, 0]["within"]) for r in range(3)] == [1, 0, 1] and [int(st[r, 0]["near_d2"]) for r in range(2)] == [3072 ** 2, 3073 ** 2]
                     and tot[0]["within_rows"] == 2 and tot[0]["within_sum"] == 2 and tot[0]["opp_rows"] == 3))
    out.append(_case("radius_2_5", v, c, m, prm(1, 1, 2.5), lambda rec, st, tot, grid: [int(st[r, 1]["within"]) for r in range(3)] == [0, 0, 1]))
    # ---- an equidistant pair of nearest opponents: the earlier column ----
    c, m = players([1, 0, 1, 1])
    out.append(_case("equidistant_nearest_opponents", still([(55.0, 30.0), (50.0, 30.0), (45.0, 30.0), (50.0, 35.0)], 2), c, m, prm(1, 1, 5.0),
                     lambda rec, st, tot, grid: st[0, 1]["near_col"] == 0 and st[0, 1]["near_d2"] == 5120 ** 2 and st[0, 1]["within"] == 3 and st[0, 0]["near_col"] == 1))
    # ---- goalkeepers on and off ----
    c = [(P, 1, 0), (G, 50, 0), (P, 2, 0), (G, 51, 0), (G, 52, 1)]
    m = {1: 0, 2: 1, 50: 0}
    v = still([(30.0, 34.0), (2.0, 34.0), (75.0, 34.0), (103.0, 34.0), (640.0, 360.0)], 2)
    out.append(_case("goalkeepers_on", v, c, m, prm(1, 1),
                     lambda rec, st, tot, grid: list(rec[0]["n"]) == [1, 1, 2] and [int(t["group"]) for t in tot] == [0, 1, 2, 2] and [int(t["col"]) for t in tot] == [0, 2, 1, 3]
                     and st[0, 1]["near_col"] == -1 and st[0, 1]["within"] == 0 and st[0, 0]["near_col"] == 2 and rec[0]["cells"][2].sum() > 0 and conserves(rec, st, tot, grid)))
    out.append(_case("goalkeepers_off", v, c, m, prm(1, 0),
                     lambda rec, st, tot, grid: list(rec[0]["n"]) == [1, 1, 0] and len(tot) == 2 and rec[0]["n_sites"] == 2 and not rec[0]["cells"][2].any()
                     and conserves(rec, st, tot, grid)))
    # ---- the ball, _video columns, boundary columns, unmapped players and negative mapping entries are ignored ----
    c = [(BALL, 0, 0), (P, 1, 1), (P, 1, 0), (BOUNDARY, 2, 0), (P, 7, 0), (P, 8, 0), (P, 2, 0), (G, 3, 1)]
    m = {1: 0, 2: 1, 8: -1, 3: 0}
    out.append(_case("non_members_ignored", still([(52.0, 34.0), (600.0, 300.0), (20.0, 20.0), (0.0, 0.0), (50.0, 50.0), (60.0, 10.0), (80.0, 40.0), (5.0, 5.0)], 2), c, m, prm(1),
                     lambda rec, st, tot, grid: [int(s["col"]) for s in used(st, 0)] == [2, 6] and [int(t["col"]) for t in tot] == [2, 6] and conserves(rec, st, tot, grid)))
    # ---- members of the groups interleaved in column order: the totals go by group, the sites by column ----
    c = [(P, 1, 0), (P, 2, 0), (G, 9, 0), (P, 3, 0), (P, 4, 0)]
    m = {1: 1, 2: 0, 3: 1, 4: 0}
    out.append(_case("groups_interleaved", still([(20.0, 20.0), (30.0, 50.0), (3.0, 34.0), (70.0, 20.0), (80.0, 50.0)], 2), c, m, prm(2),
                     lambda rec, st, tot, grid: [int(t["col"]) for t in tot] == [1, 4, 0, 3, 2] and [int(s["group"]) for s in used(st, 0)] == [1, 0, 2, 1, 0]
                     and conserves(rec, st, tot, grid)))
    # ---- a site moving across a third boundary ----
    c, m = players([0, 1])
    v = still([(33.0, 34.0), (90.0, 34.0)], 6)
    v[0, :, 0] = 33.0 + np.arange(6)
    out.append(_case("crossing_a_third", v, c, m, prm(1),
                     lambda rec, st, tot, grid: (np.diff(st[:, 0]["cells"][:, 0]) == 0).all() and (np.diff(st[:, 0]["cells"][:, 1]) > 0).any()
                     and (st[:, 0]["cells"][:, 0] == 35 * 68).all() and conserves(rec, st, tot, grid)))
    # ---- 70 member columns, five of them present per row: a window that moves by one column per row (the second step of the sites kernel) ----
    c, m = players([i % 2 for i in range(70)])
    v = still([(5.0 + 1.3 * i, 4.0 + 0.9 * ((7 * i) % 70)) for i in range(70)], 20)
    for r in range(20):
        v[[i for i in range(70) if (i - 55 - r) % 70 >= 5], r] = NAN
    out.append(_case("members_70_window", v, c, m, prm(1),
                     lambda rec, st, tot, grid: (rec["n_sites"] == 5).all() and [int(s["col"]) for s in used(st, 12)] == [0, 1, 67, 68, 69] and tot["rows"].sum() == 100
                     and conserves(rec, st, tot, grid)))
    # ---- seeded random walks with holes ----
    for R, rows, n in ((1, 12, 10), (2, 6, 10), (4, 4, 10), (4, 8, 3)):
        out.append(_case("walk_R%d_%d_rows_%d_a_side" % (R, rows, n), *walk(40 + R + rows, n, rows, 0.1), prm(R, 1, 4.0), conserves))
    out.append(_case("walk_goalkeepers_off", *walk(44, 10, 6, 0.1), prm(1, 0, 4.0), conserves))
    for rows in (63, 65, 257):
        out.append(_case("rows_%d" % rows, *walk(rows, 1, rows, 0.5, keepers=1), prm(1, 1, 60.0),
                         lambda rec, st, tot, grid: conserves(rec, st, tot, grid) and {SR.ACTIVE, SR.EMPTY} <= set(rec["status"].tolist()) and tot["within_rows"].any()))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the contract's (records, sites, totals, owner maps of all rows) of a case (read only: shared by the tests)"""
    c = BY_NAME[name]
    out = SR.space(c["values"], c["columns"], c["mapping"], c["p"], 0, c["values"].shape[1])
    for a in out:
        a.setflags(write=False)
    return out
