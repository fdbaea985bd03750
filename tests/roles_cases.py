"""Constructed tables for the role stage (include/eagle.h eagle_op_roles; contract: tests/roles_ref.py), each named after what it forces; "check" says,
on the contract's result (records [rows, 2], member roles [members, rows], model [1]), that it does (tests/test_roles_cpu.py asserts every one).
reference(name) is computed once per case and shared by the tests.  Cases with 10 roles stay at or below 16 rows, cases with many rows at 5 roles or
fewer.  The prepare kernel takes 64 rows per workgroup, the assign kernel 32 (row, group) pairs per workgroup of four waves (csrc/roles.hip): 63, 65 and
257 rows cross both boundaries."""
import functools

import numpy as np

import minimap_ref as R_
import roles_ref as RR

P, G, BALL = R_.PLAYER, R_.GOALKEEPER, R_.BALL
NAN, INF = float("nan"), float("inf")
FORM = {2: [(30.0, 34.0), (62.0, 30.0)],
        3: [(20.0, 20.0), (40.0, 50.0), (90.0, 30.0)],
        5: [(15.0, 14.0), (18.0, 50.0), (45.0, 33.0), (72.0, 12.0), (76.0, 55.0)],
        10: [(20.0, 8.0), (18.0, 26.0), (18.0, 42.0), (20.0, 60.0), (45.0, 10.0), (43.0, 27.0), (43.0, 41.0), (45.0, 58.0), (70.0, 24.0), (70.0, 44.0)]}


def _case(name, values, columns, mapping, p, check=None):
    return {"name": name, "values": np.asarray(values, np.float64), "columns": columns, "mapping": mapping, "p": p, "check": check or (lambda rec, mr, model: True)}


def one_team(pts, ids0=1, team=0):
    """[(x, y)] per column -> (columns, mapping) of one team"""
    return [(P, ids0 + i, 0) for i in range(len(pts))], {ids0 + i: team for i in range(len(pts))}


def still(pts, rows):
    """[(x, y)] -> values [len(pts)][rows][2], everybody standing"""
    return np.repeat(np.array(pts, np.float64)[:, None, :], rows, 1)


def walk(seed, pts, rows, jitter=1.0, drift=3.0):
    """the players round their places, the whole team drifting from row to row (the centre takes the drift out)"""
    r = np.random.default_rng(seed)
    return np.array(pts, np.float64)[:, None, :] + r.normal(0, jitter, (len(pts), rows, 2)) + np.cumsum(r.normal(0, drift, (1, rows, 2)), 1)


def two_teams(name, seed, R, rows, p, extra=1, holes=0.0, check=None, swap_every=0):
    """two groups of R players round FORM[R] (group 1 mirrored) and `extra` more who show up on three rows in ten, a goalkeeper, the ball and an unmapped
    player; a share of the cells absent.  swap_every = k: every k rows two columns of a group exchange places for good, so that a column's mean (a seed)
    lies between the places it stood at and the rounds have something to move"""
    r = np.random.default_rng(seed)
    cols, mp, vals = [], {}, []
    for g in (0, 1):
        pts = FORM[R] + [(52.5, 34.0 + 3.0 * e) for e in range(extra)]
        if g:
            pts = [(105.0 - x, y) for x, y in pts]
        v = walk(seed + 10 * g, pts, rows)
        for s in range(swap_every, rows, max(swap_every, 1)):
            a, b = r.choice(R, 2, replace=False)
            v[[a, b], s:] = v[[b, a], s:]
        v[R:][r.uniform(size=(extra, rows)) >= 0.3] = NAN
        v[:R][r.uniform(size=(R, rows)) < holes] = NAN
        for i in range(len(pts)):
            cols.append((P, 1 + 100 * g + i, 0))
            mp[1 + 100 * g + i] = 0 if g == 0 else 2
        vals.append(v)
    cols += [(G, 900, 0), (BALL, 0, 0), (P, 999, 0)]
    vals.append(walk(seed + 5, [(5.0, 34.0), (50.0, 30.0), (60.0, 40.0)], rows))
    order = r.permutation(len(cols))                            # the groups' columns interleave in the table
    return _case(name, np.concatenate(vals)[order], [cols[i] for i in order], mp, p, check)


def statuses(rec, g=0):
    return [int(s) for s in rec[:, g]["status"]]


def is_assignment(rec, mr, model):
    """every ACTIVE row of a seeded group: n distinct columns in col, cost >= 0"""
    for g in (0, 1):
        if model["group"][0, g]["status"] != RR.MODEL_OK:
            continue
        for o in rec[:, g]:
            held = [c for c in o["col"] if c >= 0]
            if (o["status"] == RR.ACTIVE) != (len(held) > 0) or len(set(held)) != len(held) or (held and len(held) != o["n"]):
                return False
    return True


def _cases():
    out = []
    prm = RR.role_params
    # ---- role counts, everybody present ----
    for R, rows in ((2, 20), (3, 20), (5, 20), (10, 8)):
        c, m = one_team(FORM[R])
        out.append(_case("roles_%d" % R, walk(R, FORM[R], rows), c, m, prm(R, R, 4),
                         lambda rec, mr, model, R=R, rows=rows: statuses(rec) == [RR.ACTIVE] * rows and is_assignment(rec, mr, model) and (rec[:, 0]["n"] == R).all()
                         and model["group"][0, 0]["status"] == RR.MODEL_OK and model["group"][0, 1]["status"] == RR.NO_SEEDS and int(model["group"][0, 0]["count"].sum()) == R * rows))
    # ---- n == R, n == min_present, min_present - 1, R + 1, 0: R = 5, min_present = 3, seven members ----
    pts = FORM[5] + [(50.0, 60.0), (55.0, 5.0)]
    c, m = one_team(pts)
    v = walk(11, pts, 15)
    for r in range(15):
        v[(5, 3, 2, 6, 0)[r % 5]:, r] = NAN
    out.append(_case("present_counts", v, c, m, prm(5, 3, 4),
                     lambda rec, mr, model: statuses(rec) == [RR.ACTIVE, RR.ACTIVE, RR.TOO_FEW, RR.TOO_MANY, RR.EMPTY] * 3 and [int(n) for n in rec[:5, 0]["n"]] == [5, 3, 2, 6, 0]
                     and model["group"][0, 0]["active_rows"] == 6 and (rec[4, 0]["cx"], rec[4, 0]["cy"]) == (0, 0) and is_assignment(rec, mr, model)))
    # ---- a group of R - 1 seed columns beside a healthy one; a group without members is roles_*'s group 1 ----
    c0, m0 = one_team(FORM[5])
    c1, m1 = one_team(FORM[5][:4], 101, 1)
    out.append(_case("no_seeds_beside_healthy", walk(12, FORM[5] + FORM[5][:4], 6), c0 + c1, {**m0, **m1}, prm(5, 4, 3),
                     lambda rec, mr, model: model["group"][0, 1]["status"] == RR.NO_SEEDS and model["group"][0, 1]["active_rows"] == 6 and statuses(rec, 1) == [RR.ACTIVE] * 6
                     and (rec[:, 1]["col"] == -1).all() and (rec[:, 1]["cost"] == 0).all() and (mr[5:] == -1).all() and (rec[:, 1]["cx"] != 0).all()
                     and model["group"][0, 0]["status"] == RR.MODEL_OK and not model["group"][0, 1]["mean"].any()))
    # ---- ties.  Two players mirror-symmetric about two roles: four rows (-10, 0), (10, 0), then (0, 10), (0, -10) and its mirror: the seeds are (-20/3, 0)
    # and (20/3, 0) rounded alike, rows 4 and 5 have all four costs equal, and the lexicographic rule gives player 0 role 0 ----
    c, m = one_team([0, 0])
    v = still([(-10.0, 0.0), (10.0, 0.0)], 6)
    v[:, 4] = [(0.0, 10.0), (0.0, -10.0)]; v[:, 5] = [(0.0, -10.0), (0.0, 10.0)]
    out.append(_case("tie_mirror_every_cost_equal", v, c, m, prm(2, 2, 3),
                     lambda rec, mr, model: [list(o["col"][:2]) for o in rec[:, 0]] == [[0, 1]] * 6 and model["group"][0, 0]["mean"][0, 0] == -model["group"][0, 0]["mean"][1, 0]
                     and rec[4, 0]["cost"] == rec[5, 0]["cost"] == 2 * (model["group"][0, 0]["mean"][1, 0] ** 2 + 10240 ** 2)))
    c, m = one_team(FORM[3])
    v = walk(13, FORM[3], 5)
    v[2, 2] = v[1, 2]; v[0, 4] = v[1, 4]
    out.append(_case("tie_coincident_players", v, c, m, prm(3, 3, 3),
                     lambda rec, mr, model: is_assignment(rec, mr, model) and mr[1, 2] != mr[2, 2] and mr[0, 4] != mr[1, 4]))
    # two fragments of one standing person seed two coincident roles; the later of them never gets a row and keeps its place (cnt == 0)
    pts = FORM[5][:4] + [FORM[5][3]]
    c, m = one_team(pts)
    v = still(pts, 20)
    v[3, 10:] = NAN; v[4, :10] = NAN
    out.append(_case("tie_coincident_roles_and_an_empty_role", v, c, m, prm(5, 4, 3),
                     lambda rec, mr, model: list(model["group"][0, 0]["mean"][3]) == list(model["group"][0, 0]["mean"][4]) and model["group"][0, 0]["count"][4] == 0
                     and model["group"][0, 0]["count"][3] == 20 and (rec[:10, 0]["col"][:, 3] == 3).all() and (rec[10:, 0]["col"][:, 3] == 4).all()))
    # ---- a fragment that ends, a new id two rows later a metre away ----
    pts = FORM[3] + [(91.0, 30.0)]
    c, m = one_team(pts)
    v = still(pts, 20)
    v[2, 10:] = NAN; v[3, :12] = NAN
    out.append(_case("fragment_replaced", v, c, m, prm(3, 2, 4),
                     lambda rec, mr, model: statuses(rec) == [RR.ACTIVE] * 20 and (mr[2, :10] == 2).all() and (mr[3, 12:] == 2).all() and (mr[0] == 0).all() and (mr[1] == 1).all()))
    # ---- two ids exchanging places at row 14 of 20: the roles stay, col[j] changes hands ----
    c, m = one_team(FORM[3])
    v = walk(14, FORM[3], 20, jitter=0.3)
    v[[0, 1], 14:] = v[[1, 0], 14:]
    out.append(_case("exchange", v, c, m, prm(3, 3, 6),
                     lambda rec, mr, model: (rec[:14, 0]["col"][:, :2] == [0, 1]).all() and (rec[14:, 0]["col"][:, :2] == [1, 0]).all() and (mr[2] == 2).all()))
    # ---- T = 1; T beyond the fixed point ----
    out.append(two_teams("iterations_1", 15, 5, 30, prm(5, 4, 1), swap_every=4, check=lambda rec, mr, model: model["changed"][0, 0] > 0 and not model["changed"][0, 1:].any()))
    out.append(two_teams("iterations_12", 15, 5, 30, prm(5, 4, 12), swap_every=4,
                         check=lambda rec, mr, model: model["changed"][0, 11] == 0 and model["changed"][0, 1] > 0))
    # ---- absent cells: NaN, infinity, exactly 1024 m (present) and one ulp beyond (absent) ----
    pts = FORM[3] + [(50.0, 34.0)] * 5
    c, m = one_team(pts)
    v = still(pts, 2)
    v[3:, 0] = [(NAN, 1.0), (1.0, INF), (-INF, 1.0), (np.nextafter(1024.0, INF), 1.0), (1.0, -np.nextafter(1024.0, INF))]
    v[3:, 1] = NAN; v[3, 1] = (1024.0, -1024.0)
    out.append(_case("absent_cells", v, c, m, prm(4, 3, 2),
                     lambda rec, mr, model: [int(n) for n in rec[:, 0]["n"]] == [3, 4] and (mr[3:, 0] == -1).all() and mr[3, 1] >= 0))
    # ---- the domain's corners: three players in one corner, the others in the three left, turning with the row; |u| beyond 2^20, costs beyond 2^41 ----
    cn = [(1024.0, 1024.0), (-1024.0, 1024.0), (-1024.0, -1024.0), (1024.0, -1024.0)]
    c, m = one_team([0] * 6)
    v = np.array([[cn[(min(i, 3) + r) % 4] for r in range(8)] for i in range(6)])
    out.append(_case("domain_corners", v, c, m, prm(6, 6, 4),
                     lambda rec, mr, model: int(rec[:, 0]["cost"].max()) > 2 ** 41 and abs(int(rec[0, 0]["cx"])) == (2 ** 21 + 3) // 6 and is_assignment(rec, mr, model)))
    # ---- centres and centred sums of both signs: the floor-division rule on negative numerators ----
    pts = [(x - 80.0, y - 50.0) for x, y in FORM[3]]
    c, m = one_team(pts)
    out.append(_case("negative_sums", walk(16, pts, 21), c, m, prm(3, 3, 4),
                     lambda rec, mr, model: (rec[:, 0]["cx"] < 0).all() and (model["group"][0, 0]["mean"][:3] < 0).any() and (model["group"][0, 0]["mean"][:3] > 0).any()
                     and (model["group"][0, 0]["sum"][:3] % np.maximum(model["group"][0, 0]["count"][:3, None], 1) != 0).any()))
    # ---- rows across the wave and workgroup boundaries ----
    for rows in (1, 63, 65):
        out.append(two_teams("rows_%d" % rows, 20 + rows, 5, rows, prm(5, 4, 4), holes=0.05, check=is_assignment, swap_every=7))
    out.append(two_teams("rows_257", 257, 5, 257, prm(5, 4, 5), holes=0.08, swap_every=20,
                         check=lambda rec, mr, model: is_assignment(rec, mr, model) and {RR.ACTIVE, RR.TOO_MANY} <= set(statuses(rec))))
    # ---- ACTIVE and inactive rows interleaved one by one ----
    c, m = one_team(FORM[5])
    v = walk(17, FORM[5], 40)
    v[2:, 1::2] = NAN
    out.append(_case("interleaved_active", v, c, m, prm(5, 4, 3), lambda rec, mr, model: statuses(rec) == [RR.ACTIVE, RR.TOO_FEW] * 20 and (mr[:, 1::2] == -1).all()))
    # ---- 23 member columns, five of them present per row: a window that moves by one column every second row ----
    pts = [FORM[5][i % 5] for i in range(23)]
    c, m = one_team(pts)
    v = walk(18, pts, 46, jitter=0.5)
    for r in range(46):
        v[[i for i in range(23) if (i - r // 2) % 23 >= 5], r] = NAN
    out.append(_case("members_23", v, c, m, prm(5, 5, 4), lambda rec, mr, model: (rec[:, 0]["n"] == 5).all() and is_assignment(rec, mr, model) and (mr >= 0).sum() == 5 * 46))
    # ---- ten roles, two teams, holes ----
    out.append(two_teams("ten_roles_two_teams", 19, 10, 12, prm(10, 8, 6), holes=0.06, check=is_assignment, swap_every=3))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the contract's (records, member roles, model) of a case (read only: shared by the tests)"""
    c = BY_NAME[name]
    out = RR.roles(c["values"], c["columns"], c["mapping"], c["p"])
    for a in out:
        a.setflags(write=False)
    return out
