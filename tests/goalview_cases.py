"""Constructed tables for the goal-view stage (include/eagle.h eagle_op_goal_view; contract: tests/goalview_ref.py), each named after what it forces;
"check" says, on the contract's result (goal_view()'s dict), that it does (tests/test_goalview_cpu.py asserts every one).  reference(name) is computed
once per case and shared by the tests.  Tables have 1 to 70 rows and 0 to 33 blockers per group.  Every case carries a grid at R = 1 over its rows (one
over a sub-range of them), one case each at R = 2 and R = 4.  What the kernels' shapes need (csrc/goalview.hip): a row with 0, 1, 32 and 33 blockers; the
range's boundary through a 16 x 16 tile and through a wave's 8 x 8 block (every case: the circle of 40 m, and one of 12.3 m); partial last tiles
(105 R and 68 R are no multiples of 16 for R = 1, 2, 4); 70 rows are three workgroups of the prepare and rows kernels and, with 14 points, four of the
points kernel.  Unless a case says otherwise the direction is RIGHT: group 0 attacks the goal at x = 105."""
import functools

import numpy as np

import goalview_ref as GR
import minimap_ref as R_
import offside_ref as OR
from offside_cases import walk

P, G, BALL, BOUNDARY = R_.PLAYER, R_.GOALKEEPER, R_.BALL, R_.BOUNDARY
NAN = float("nan")
ALL = 2 ** 64 - 1
SPOT = (94.0, 34.0)                                                        # the penalty spot of the goal at x = 105
prm = GR.goal_view_params


def _case(name, values, columns, mapping, check, owner=None, no_ball=False, **kw):
    values = np.asarray(values, np.float64)
    kw.setdefault("grid_rows", values.shape[1])
    return {"name": name, "values": values, "columns": columns, "mapping": mapping, "p": prm(**kw), "check": check,
            "owner": None if owner is None else np.asarray(owner, np.int32), "no_ball": no_ball}


def scene(att=(), dfn=(), keepers=(), ball=None, rows=1):
    """[(x, y)] of group 0, of group 1, of the keepers, the ball -> (values [cols][rows][2], columns, mapping); ids are column + 1"""
    pts = list(att) + list(dfn) + list(keepers) + ([ball] if ball is not None else [])
    kinds = [P] * (len(att) + len(dfn)) + [G] * len(keepers) + ([BALL] if ball is not None else [])
    cols = [(k, c + 1, 0) for c, k in enumerate(kinds)]
    mp = {c + 1: (0 if c < len(att) else 1) for c in range(len(att) + len(dfn))}
    return np.repeat(np.array(pts, np.float64).reshape(-1, 1, 2), rows, 1), cols, mp


def bits(m):
    return [k for k in range(64) if (int(m) >> k) & 1]


def reverse(m):
    return int("{:064b}".format(int(m))[::-1], 2)


def consistent(o):
    """what holds of every result: open within 0 .. full, masks only on OK points, the records' best member, the totals"""
    rec, opn, msk, sts, tot = o["rows"], o["open"].astype(np.int64), o["mask"], o["status"], o["totals"]
    ok = sts == GR.PT_OK
    if ((opn < 0) != ~(ok | (sts == GR.PT_FAR))).any() or (msk[~ok] != 0).any() or (opn[sts == GR.PT_FAR] != 0).any():
        return False
    for g in (0, 1):
        mine = tot["group"] == g
        best = np.where(ok[mine], opn[mine], -1).max(0) if mine.any() else np.full(len(rec), -1)
        if not np.array_equal(best, rec[:, g]["best_open"]):
            return False
        b = rec[:, g]
        bok = b["ball_status"] == GR.PT_OK
        if (b["ball_open"][bok] > b["ball_full"][bok]).any() or (b["ball_mask"][~bok] != 0).any() or (b["ball_full"][~bok] != 0).any():
            return False
        if ((b["status"] == GR.TOO_MANY) != (b["n_blockers"] > GR.BLOCKERS)).any():
            return False
    return (np.array_equal(tot["rows"], ok.sum(1)) and np.array_equal(tot["sum_open"], np.where(ok, opn, 0).sum(1))
            and np.array_equal(tot["max_open"], np.where(ok, opn, -1).max(1) if opn.shape[1] else tot["max_open"]))


def _cases():
    out = []
    RIGHT, LEFT = OR.DIR_RIGHT, OR.DIR_LEFT
    # ---- hand-made scenes with known answers ---------------------------------------------------------------------------------------------
    v, c, m = scene([SPOT], ball=SPOT)
    out.append(_case("empty_goal_from_the_penalty_spot", v, c, m,
                     lambda o: o["mask"][0, 0] == 0 and o["rows"][0, 0]["ball_mask"] == 0 and o["rows"][0, 0]["ball_open"] == o["rows"][0, 0]["ball_full"] == o["open"][0, 0]
                     and o["open"][0, 0] >> 16 == 164 and o["rows"][0, 0]["n_blockers"] == 0 and (o["rows"][0, 0]["best_col"], o["rows"][0, 0]["best_open"]) == (0, o["open"][0, 0])
                     and 155 <= o["grid"][0, 33, 93] <= 160 and 168 <= o["grid"][0, 34, 94] <= 174 and o["grid"][0, 34, 104] == 0 and o["grid"][0, 34, 60] == 0
                     and o["rows"][0, 1]["ball_status"] == GR.PT_FAR and o["rows"][0, 1]["ball_open"] == 0 and consistent(o)))
    v, c, m = scene([SPOT], [(94.25, 34.0)])
    out.append(_case("blocker_standing_on_the_point", v, c, m, lambda o: o["mask"][0, 0] == ALL and o["open"][0, 0] == 0 and o["status"][0, 0] == GR.PT_OK
                     and o["totals"][0]["rows"] == 1 and o["totals"][0]["max_open"] == 0 and consistent(o)))
    v, c, m = scene([SPOT], keepers=[(105.0, 34.0)])
    out.append(_case("keeper_on_the_line_at_the_centre", v, c, m, lambda o: bits(o["mask"][0, 0]) == list(range(23, 41)) and reverse(o["mask"][0, 0]) == o["mask"][0, 0]
                     and list(o["rows"][0]["n_blockers"]) == [1, 1] and consistent(o)))       # (the attacker is in the way of group 1)
    out.append(_case("keeper_with_an_outfield_radius", v, c, m, lambda o: bits(o["mask"][0, 0]) == list(range(29, 35)), keeper_radius=0.4))
    v, c, m = scene([SPOT], [(94.3, 34.5)])
    out.append(_case("lateral_blocker_with_one_tangent_pointing_away", v, c, m,
                     lambda o: bits(o["mask"][0, 0]) == list(range(bits(o["mask"][0, 0])[0], 64)) and 55 <= bits(o["mask"][0, 0])[0] <= 60 and consistent(o)))
    v, c, m = scene([SPOT], [(94.3, 33.5)])
    out.append(_case("lateral_blocker_on_the_other_side", v, c, m, lambda o: o["mask"][0, 0] == reverse(reference("lateral_blocker_with_one_tangent_pointing_away")["mask"][0, 0])))
    v, c, m = scene([SPOT], [(90.0, 34.0), (106.0, 34.0), (94.0, 34.3), (105.0 + 1.0 / 1024, 33.0)])
    out.append(_case("blockers_behind_the_point_beside_it_and_beyond_the_line", v, c, m, lambda o: o["mask"][0, 0] == 0 and o["rows"][0, 0]["n_blockers"] == 4 and consistent(o)))
    v, c, m = scene([SPOT], [(105.0, 34.0)])
    out.append(_case("blocker_exactly_on_the_line_counts", v, c, m, lambda o: bits(o["mask"][0, 0]) == list(range(29, 35))))
    v, c, m = scene([SPOT, (100.0, 34.0), (97.0, 34.0)])
    out.append(_case("teammates_do_not_block", v, c, m, lambda o: (o["mask"] == 0).all() and (o["rows"][0]["n_blockers"] == [0, 3]).all() and o["rows"][0, 0]["best_col"] == 1))
    # the same scene turned towards the other goal
    sv, sc, sm = scene([(88.0, 29.5), (95.5, 40.25), (99.0, 31.0)], [(93.0, 31.5), (97.25, 37.0), (101.0, 33.0), (96.0, 30.0)], [(103.5, 34.75), (2.0, 34.0)], (92.0, 33.0))
    out.append(_case("a_scene_towards_the_right_goal", sv, sc, sm, lambda o: (o["mask"][:3, 0] != 0).all() and (o["status"][:3, 0] == GR.PT_OK).all()
                     and list(o["rows"][0]["n_blockers"]) == [5, 4] and consistent(o)))
    mx = sv.copy(); mx[:, :, 0] = 105.0 - sv[:, :, 0]
    out.append(_case("mirrored_in_x_towards_the_left_goal_is_equal", mx, sc, sm,
                     lambda o: all(o[k].tobytes() == reference("a_scene_towards_the_right_goal")[k].tobytes() for k in ("open", "mask", "status", "rows", "totals"))
                     and np.array_equal(o["grid"], reference("a_scene_towards_the_right_goal")["grid"][:, :, ::-1]), direction=LEFT))
    rot = mx.copy(); rot[:, :, 1] = 68.0 - sv[:, :, 1]
    out.append(_case("turned_half_round_gives_the_bit_reversed_masks", rot, sc, sm,
                     lambda o: [int(x) for x in o["mask"][:, 0]] == [reverse(x) for x in reference("a_scene_towards_the_right_goal")["mask"][:, 0]]
                     and o["rows"][0, 0]["ball_mask"] == reverse(reference("a_scene_towards_the_right_goal")["rows"][0, 0]["ball_mask"])
                     and (np.abs(o["open"].astype(np.int64) - reference("a_scene_towards_the_right_goal")["open"]) <= 64).all(), direction=LEFT))
    # ---- statuses ------------------------------------------------------------------------------------------------------------------------
    v, c, m = scene([(104.5, 34.0), (104.0, 34.0), (50.0, 34.0), (65.0, 34.0), (65.0 - 1.0 / 1024, 34.0), (107.0, 34.0), (NAN, 34.0)], [(104.25, 34.0)], ball=(NAN, NAN))
    out.append(_case("near_the_line_far_and_absent", v, c, m,
                     lambda o: list(o["status"][:7, 0]) == [GR.PT_NEAR_LINE, GR.PT_OK, GR.PT_FAR, GR.PT_OK, GR.PT_FAR, GR.PT_OK, GR.PT_ABSENT]
                     and list(o["open"][[0, 2, 4, 6], 0]) == [-1, 0, 0, -1] and o["mask"][1, 0] == ALL and o["mask"][5, 0] == 0 and o["open"][5, 0] > 0
                     and (o["rows"][0]["ball_status"] == GR.PT_ABSENT).all() and (o["rows"][0]["ball_open"] == -1).all() and o["totals"][2]["rows"] == 0
                     and (o["totals"][2]["max_open"], o["totals"][2]["max_row"]) == (-1, -1) and consistent(o)))
    v, c, m = scene([SPOT], [(100.0, 34.0)])
    out.append(_case("table_without_a_ball_column", v, c, m, lambda o: (o["rows"][0]["ball_status"] == GR.PT_ABSENT).all() and o["status"][0, 0] == GR.PT_OK))
    v, c, m = scene([SPOT], [(100.0, 34.0)], ball=(95.0, 34.0))
    out.append(_case("table_flagged_no_ball", v, c, m, lambda o: o["rows"].tobytes() == reference("table_without_a_ball_column")["rows"].tobytes(), no_ball=True))
    # 33 opponents: row 0 nobody of them, row 1 one, row 2 thirty-two, row 3 all
    v, c, m = scene([SPOT, (20.0, 30.0)], [(96.0 + 0.25 * (k % 8), 28.0 + 1.5 * (k // 8) + 0.125 * (k % 3)) for k in range(33)], [(104.0, 34.5)], (93.0, 35.0), rows=4)
    v[2:35, 0] = NAN; v[3:35, 1] = NAN; v[34, 2] = NAN; v[35, :3] = NAN
    out.append(_case("rows_with_0_1_32_and_33_blockers", v, c, m,
                     lambda o: list(o["rows"][:, 0]["n_blockers"]) == [0, 1, 32, 34] and list(o["rows"][:, 0]["status"]) == [0, 0, 0, GR.TOO_MANY]
                     and list(o["status"][0]) == [0, 0, 0, GR.PT_ROW] and o["rows"][3, 0]["ball_status"] == GR.PT_ROW and o["open"][0, 3] == -1 and o["mask"][0, 0] == 0
                     and o["mask"][0, 2] != 0 and not o["grid"][3].any() and o["grid"][2].any() and o["totals"][0]["rows"] == 3 and o["totals"][0]["max_row"] == 0
                     and (o["rows"][:, 1]["status"] == 0).all() and o["rows"][3, 1]["n_blockers"] == 2 and consistent(o)))
    v2 = v.copy(); v2[35, 3] = NAN
    out.append(_case("exactly_33_blockers_is_too_many", v2, c, m, lambda o: o["rows"][3, 0]["n_blockers"] == 33 and o["rows"][3, 0]["status"] == GR.TOO_MANY
                     and o["rows"][2, 0]["status"] == GR.OK and o["rows"][2, 0]["n_blockers"] == 32))
    # ---- keepers: K33's rule ---------------------------------------------------------------------------------------------------------------
    v, c, m = scene([SPOT], [(11.0, 34.0)], [(20.0, 34.0), (52.5, 34.0), (100.0, 34.0)])
    out.append(_case("a_keeper_blocks_only_in_his_own_half", v, c, m, lambda o: list(o["rows"][0]["n_blockers"]) == [2, 2] and o["mask"][0, 0] != 0 and o["mask"][1, 0] == 0
                     and consistent(o)))
    # ---- the best member, the owner and the totals -----------------------------------------------------------------------------------------
    v, c, m = scene([(80.0, 10.0), (96.0, 36.0), (96.0, 36.0), (70.0, 34.0)], [(99.0, 35.5)], [(104.0, 34.25)], (96.0, 36.0), rows=5)
    # [column, row]: row 1: column 0 joins 1 and 2; row 2: 1 leaves; row 3: 2 is absent; row 4: 1 and 2 stand together nearer the goal
    v[0, 1] = (96.0, 36.0); v[1, 2] = (80.0, 10.0); v[2, 3] = (NAN, NAN); v[1, 4] = (97.0, 33.0); v[2, 4] = (97.0, 33.0)
    own = [1, 2, 4, 5, -1]
    out.append(_case("ties_of_the_best_member_the_owner_and_the_totals", v, c, m,
                     lambda o: list(o["rows"][:, 0]["best_col"]) == [1, 0, 2, 1, 1] and o["open"][1, 0] == o["open"][2, 0] == o["open"][0, 1] == o["rows"][0, 0]["ball_open"]
                     and list(o["rows"][:, 0]["owner_col"]) == [1, 2, -1, -1, -1] and list(o["rows"][:, 1]["owner_col"]) == [-1, -1, 4, -1, -1]
                     and o["rows"][0, 0]["owner_open"] == o["open"][1, 0] and o["rows"][0, 0]["owner_mask"] == o["mask"][1, 0] and o["rows"][2, 1]["owner_open"] == 0
                     and (o["totals"][1]["rows"], o["totals"][1]["max_row"]) == (5, 4) and o["totals"][1]["sum_open"] == int(o["open"][1].astype(np.int64).sum())
                     and o["totals"][1]["chance_rows"] == 4 and o["open"][1, 2] < int(np.rint(0.2 * 2 ** 24)) <= o["open"][1, 0]
                     and (o["totals"][2]["rows"], o["totals"][2]["max_row"]) == (4, 4) and o["totals"][0]["max_row"] == 1 and o["totals"][3]["max_row"] == 0
                     and o["totals"][3]["max_open"] == o["open"][3, 0] == o["open"][3, 4] and o["totals"][4]["rows"] == 0
                     and o["grid"][0].any() and o["grid"][1].any() and o["grid"][2].any() and not o["grid"][3].any() and not o["grid"][4].any() and consistent(o),
                     owner=own, group=-1, chance=0.2))
    # ---- mapping and other columns (K33's membership) --------------------------------------------------------------------------------------
    c2 = [(P, 1, 0), (P, 2, 0), (P, 3, 0), (P, 4, 0), (P, 2, 1), (BOUNDARY, 0, 0), (G, 9, 0), (G, 9, 1), (BALL, 0, 0), (BALL, 0, 1)]
    v = np.array([SPOT, (97.0, 34.0), (98.0, 33.0), (99.0, 35.0), (600.0, 300.0), (0.0, 0.0), (103.0, 34.0), (900.0, 400.0), (95.0, 34.0), (640.0, 360.0)]).reshape(-1, 1, 2)
    out.append(_case("unmapped_players_and_video_columns_are_nobody", v, c2, [(1, 0), (2, 1), (3, 1), (4, -1), (1, 1)],
                     lambda o: list(o["totals"]["col"]) == [0, 1, 2] and list(o["totals"]["group"]) == [0, 1, 1] and o["rows"][0, 0]["n_blockers"] == 3
                     and o["rows"][0, 0]["ball_status"] == GR.PT_OK and consistent(o)))
    # ---- parameters -------------------------------------------------------------------------------------------------------------------------
    out.append(_case("a_short_range_cuts_tiles_and_waves", sv, sc, sm,
                     lambda o: (o["status"][:3, 0] == [GR.PT_FAR, GR.PT_OK, GR.PT_OK]).all() and 0 < np.count_nonzero(o["grid"][0]) < 300 and not o["grid"][0, :, :92].any(),
                     max_range=12.3, min_depth=1.5, radius=0.75, keeper_radius=1.25))
    out.append(_case("group_1_on_the_grid", sv, sc, sm, lambda o: not o["grid"][0, :, 50:].any() and o["grid"][0, :, :40].any(), group=1))
    out.append(_case("two_cells_per_metre", sv, sc, sm,
                     lambda o: o["grid"].shape == (1, 136, 210) and o["grid"][0].any() and not o["grid"][0, :, :128].any(), cells_per_metre=2))
    out.append(_case("four_cells_per_metre", sv, sc, sm, lambda o: o["grid"].shape == (1, 272, 420) and o["grid"][0].any() and not o["grid"][0, :, :256].any(), cells_per_metre=4))
    # ---- many rows ----------------------------------------------------------------------------------------------------------------------------
    wv, wc, wm = walk(41, 6, 70, 0.15)
    wv[:, :, 0] = 52.5 + (wv[:, :, 0] - 52.5) * 1.15                       # (some beyond the goal lines)
    r = np.random.default_rng(5)
    own = r.integers(-1, len(wc), 70)
    out.append(_case("seventy_rows_with_holes_and_an_owner", wv, wc, wm,
                     lambda o: {GR.PT_OK, GR.PT_ABSENT, GR.PT_FAR} <= set(o["status"].ravel().tolist()) and (o["mask"] != 0).any() and (o["rows"]["owner_col"] >= 0).any()
                     and (o["totals"]["rows"] > 0).any() and o["grid"].shape[0] == 9 and o["grid"].any() and consistent(o), owner=own, group=-1, grid_row0=58, grid_rows=9))
    out.append(_case("one_row_of_the_walk", wv[:, 7:8], wc, wm, lambda o: consistent(o), direction=LEFT))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
PARTS = ("rows", "open", "mask", "status", "totals", "grid")


@functools.lru_cache(maxsize=None)
def reference(name):
    """the contract's result of a case (read only: shared by the tests)"""
    c = BY_NAME[name]
    out = GR.goal_view(c["values"], c["columns"], c["mapping"], c["p"], c["owner"], c["no_ball"])
    for a in out.values():
        a.setflags(write=False)
    return out
