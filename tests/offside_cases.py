"""Constructed tables for the offside stage (include/eagle.h eagle_op_offside; contract: tests/offside_ref.py), each named after what it forces; "check"
says, on the contract's result (records [rows, 2], margins [members, rows], totals [members], the clip record [1], event records), that it does
(tests/test_offside_cpu.py asserts every one).  reference(name) is computed once per case and shared by the tests.  Every case stays at or below 300
rows, most at or below 8.  The rows kernel takes 64 listed columns per step of a wave, the vote and events kernels 256 rows / events per workgroup, the
totals kernel 256 rows per step (csrc/offside.hip): 63, 64, 65 and 130 members and 257 and 300 rows cross those boundaries.  Unless a case says
otherwise the direction is forced RIGHT: group 0 attacks towards x = 105, so for a = 0 a depth is qx itself."""
import functools

import numpy as np

import minimap_ref as R_
import offside_ref as OR
import possession_ref as PR

P, G, BALL, BOUNDARY = R_.PLAYER, R_.GOALKEEPER, R_.BALL, R_.BOUNDARY
NAN, INF = float("nan"), float("inf")
Q = 1024
prm = OR.offside_params


def _case(name, values, columns, mapping, p, check, events=None, no_ball=False):
    return {"name": name, "values": np.asarray(values, np.float64), "columns": columns, "mapping": mapping, "p": p, "check": check, "events": events, "no_ball": no_ball}


def still(pts, rows=1):
    """[(x, y)] per column -> values [len(pts)][rows][2], everybody standing"""
    return np.repeat(np.array(pts, np.float64)[:, None, :], rows, 1)


def table(spec, rows=1):
    """[(kind, team or None, x)] -> (values, columns, mapping): ids are column + 1, y = 30 + column"""
    cols = [(k, c + 1, 0) for c, (k, _, _) in enumerate(spec)]
    mp = {c + 1: t for c, (k, t, _) in enumerate(spec) if t is not None}
    return still([(x, 30.0 + c) for c, (_, _, x) in enumerate(spec)], rows), cols, mp


def events(*ev):
    """(kind, from_col, to_col, release_row, receive_row) -> possession's event records"""
    out = np.zeros(len(ev), PR.EVENT_DTYPE)
    for o, (kind, frm, to, rel, rcv) in zip(out, ev):
        o["kind"], o["from_col"], o["to_col"], o["release_row"], o["receive_row"], o["row"] = kind, frm, to, rel, rcv, rcv
    return out


def flags(rec, r, a):
    return int(rec[r, a]["flags"])


def walk(seed, n_per_team, rows, holes=0.0, keepers=2):
    """two teams on a random walk, team 0 on the left; goalkeepers near their lines, the ball and an unmapped player; the groups' columns interleave"""
    r = np.random.default_rng(seed)
    k = 2 * n_per_team + keepers + 2
    cols = [(P, 1 + i, 0) for i in range(2 * n_per_team)] + [(G, 900 + i, 0) for i in range(keepers)] + [(BALL, 0, 0), (P, 999, 0)]
    mp = {1 + i: (0 if i % 2 == 0 else 3) for i in range(2 * n_per_team)}
    x0 = np.array([r.uniform(5, 70) if i % 2 == 0 else r.uniform(35, 100) for i in range(2 * n_per_team)] + [3.0, 102.0][:keepers] + [52.0, 50.0])
    v = np.stack([x0, r.uniform(0, 68, k)], 1)[:, None, :] + np.cumsum(r.normal(0, 1.5, (k, rows, 2)), 1)
    v[r.uniform(size=(k, rows)) < holes] = NAN
    order = r.permutation(k)
    return v[order], [cols[i] for i in order], mp


def consistent(rec, mg, tot, clip, ev):
    """n_off is the count of positive margins, the line is never below the halfway line, margins exist exactly on OK rows"""
    groups = tot["group"]
    for a in (0, 1):
        m = mg[groups == a].astype(np.int64)
        has = m != OR.NONE
        ok = rec[:, a]["status"] == OR.OK
        if (has & ~ok[None]).any() or not np.array_equal(has.sum(0)[ok], rec[:, a]["n_att"][ok]) or not np.array_equal((has & (m > 0)).sum(0), rec[:, a]["n_off"]):
            return False
        right = OR.attacks_right(int(clip[0]["direction"]), a)
        line = rec[:, a]["line_qx"].astype(np.int64) if right else OR.U_MAX - rec[:, a]["line_qx"].astype(np.int64)
        if (line[ok] < OR.U_HALF).any():
            return False
        best = np.where(has, m, OR.NONE).max(0) if len(m) else np.full(len(rec), OR.NONE)
        if not np.array_equal(best, rec[:, a]["max_margin"]):
            return False
    return True


def _members_case(n, seed):
    """five members of group 0, n of group 1, a keeper on each side and the ball; six rows: everybody of group 1 level; depths from a set of three;
    the two deepest in the last two listed columns; the two deepest in listed columns 5 and 69 (one lane, two steps); depths from the set with holes"""
    r = np.random.default_rng(seed)
    spec = [(P, 0, 40.0 + 2 * i) for i in range(5)] + [(P, 1, 80.0) for _ in range(n)] + [(G, None, 2.0), (G, None, 103.0), (BALL, None, 50.0)]
    v, cols, mp = table(spec, 6)
    d = slice(5, 5 + n)
    v[d, 1, 0] = r.choice([80.0, 80.0 + 1.0 / Q, 81.0], n)
    v[d, 2, 0] = r.choice([60.0, 61.0], n); v[5 + n - 2, 2, 0] = 90.0; v[5 + n - 1, 2, 0] = 90.0 + 1.0 / Q
    v[d, 3, 0] = r.choice([60.0, 61.0], n); v[5, 3, 0] = 91.0
    if n > 64:
        v[5 + 64, 3, 0] = 91.0
    v[d, 4, 0] = r.choice([80.0, 80.0 + 1.0 / Q, 81.0], n)
    v[d, 5, 0] = r.choice([70.0, 75.0], n)
    hole = r.uniform(size=n) < 0.4
    v[5:5 + n][hole, 4] = NAN
    v[0:5, :, 0] = 82.0 + np.arange(5)[:, None]                              # the attackers of a = 0 stand beyond most of the lines
    keeper_col = 5 + n + 1

    def check(rec, mg, tot, clip, ev):
        a0 = rec[:, 0]
        return (list(a0["n_def"][:4]) == [n + 1] * 4 and a0[4]["n_def"] == n + 1 - int(hole.sum()) and (a0["keepers_seen"] == 1).all() and (rec[:, 1]["n_att"][:4] == n).all()
                and a0[0]["second_col"] == 5 and a0[0]["line_qx"] == 80 * Q                                          # all level: the earliest of them
                and a0[2]["second_col"] == 5 + n - 1 and a0[2]["line_qx"] == 90 * Q + 1                              # keeper 103, then the last column
                and a0[3]["second_col"] == 5 and a0[3]["line_qx"] == 91 * Q                                          # 103, then 91 twice: the earlier
                and a0[1]["second_col"] == int(np.nonzero(v[d, 1, 0] == 81.0)[0][0]) + 5 and (a0["status"] == OR.OK).all()
                and rec[0, 1]["max_col"] == 5 and rec[0, 1]["n_att"] == n and keeper_col not in tot["col"] and consistent(rec, mg, tot, clip, ev))
    return _case("members_%d" % n, v, cols, mp, prm(OR.DIR_RIGHT), check)


def _cases():
    out = []
    RIGHT, LEFT, AUTO = OR.DIR_RIGHT, OR.DIR_LEFT, OR.DIR_AUTO
    # ---- depth ties and line terms -------------------------------------------------------------------------------------------------------
    # columns: 0, 1 attackers; 2, 3 defenders; 4 keeper; 5 ball
    v, c, m = table([(P, 0, 80.0), (P, 0, 80.0 + 1.0 / Q), (P, 1, 80.0), (P, 1, 70.0), (G, None, 100.0), (BALL, None, 60.0)], 2)
    out.append(_case("level_is_onside_one_q_beyond_is_not", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: list(mg[:2, 0]) == [0, 1] and rec[0, 0]["n_off"] == 1 and flags(rec, 0, 0) == OR.BY_DEFENDER and rec[0, 0]["second_col"] == 2
                     and (rec[0, 0]["max_margin"], rec[0, 0]["max_col"]) == (1, 1) and rec[0, 0]["line_qx"] == 80 * Q and list(tot["off_rows"]) == [0, 2, 0, 0]
                     and flags(rec, 0, 1) == OR.BY_HALF | OR.KEEPER_ASSUMED and rec[0, 1]["line_qx"] == OR.U_HALF and consistent(rec, mg, tot, clip, ev)))
    v, c, m = table([(P, 0, 91.0), (P, 1, 90.0), (P, 1, 90.0), (P, 1, 60.0), (BALL, None, 60.0)])
    out.append(_case("two_defenders_level", v, c, m, prm(RIGHT, 0),
                     lambda rec, mg, tot, clip, ev: rec[0, 0]["line_qx"] == 90 * Q and rec[0, 0]["second_col"] == 1 and mg[0, 0] == Q and flags(rec, 0, 0) == OR.BY_DEFENDER))
    v, c, m = table([(P, 0, 93.0), (P, 0, 90.0), (P, 1, 85.0), (P, 1, 70.0), (G, None, 101.0), (BALL, None, 92.0)])
    out.append(_case("ball_deeper_than_the_second_last_defender", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: flags(rec, 0, 0) == OR.BY_BALL and rec[0, 0]["line_qx"] == 92 * Q and list(mg[:2, 0]) == [Q, -2 * Q] and rec[0, 0]["second_col"] == 2))
    v, c, m = table([(P, 0, 85.0), (P, 1, 85.0), (P, 1, 70.0), (G, None, 101.0), (BALL, None, 85.0)])
    out.append(_case("ball_level_with_the_defender_is_by_defender", v, c, m, prm(RIGHT), lambda rec, mg, tot, clip, ev: flags(rec, 0, 0) == OR.BY_DEFENDER and mg[0, 0] == 0))
    v, c, m = table([(P, 0, 50.0), (P, 0, 52.5), (P, 0, 52.5 + 1.0 / Q), (P, 1, 30.0), (P, 1, 40.0), (G, None, 45.0), (BALL, None, 20.0)])
    out.append(_case("everybody_in_the_attackers_own_half", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: flags(rec, 0, 0) == OR.BY_HALF | OR.KEEPER_ASSUMED and rec[0, 0]["line_qx"] == OR.U_HALF and list(mg[:3, 0]) == [-2560, 0, 1]
                     and rec[0, 0]["n_off"] == 1))
    v, c, m = table([(P, 0, 5.0), (P, 1, 80.0), (P, 1, 90.0), (G, None, 100.0), (BALL, None, 6.0)])
    out.append(_case("attacker_deep_in_his_own_half", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: mg[0, 0] == (5 - 90) * Q and rec[0, 0]["n_off"] == 0 and rec[0, 0]["max_margin"] == -85 * Q and tot[0]["max_margin"] == -85 * Q))
    # ---- keepers -------------------------------------------------------------------------------------------------------------------------
    v, c, m = table([(P, 0, 86.0), (P, 1, 85.0), (P, 1, 70.0), (G, None, 100.0)])
    out.append(_case("keeper_seen", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: rec[0, 0]["keepers_seen"] == 1 and rec[0, 0]["n_def"] == 3 and rec[0, 0]["line_qx"] == 85 * Q
                     and flags(rec, 0, 0) == OR.BY_DEFENDER | OR.NO_BALL and clip[0]["n_keepers"] == 1))
    v, c, m = table([(P, 0, 86.0), (P, 1, 85.0), (P, 1, 70.0)])
    out.append(_case("keeper_unseen_and_assumed", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: rec[0, 0]["line_qx"] == 85 * Q and flags(rec, 0, 0) & OR.KEEPER_ASSUMED and rec[0, 0]["second_col"] == 1 and mg[0, 0] == Q))
    out.append(_case("keeper_unseen_and_not_assumed", v, c, m, prm(RIGHT, 0),
                     lambda rec, mg, tot, clip, ev: rec[0, 0]["line_qx"] == 70 * Q and not flags(rec, 0, 0) & OR.KEEPER_ASSUMED and rec[0, 0]["second_col"] == 2 and mg[0, 0] == 16 * Q))
    v, c, m = table([(P, 0, 86.0), (P, 1, 85.0), (P, 1, 70.0), (G, None, 52.5)])
    out.append(_case("keeper_exactly_on_the_halfway_line", v, c, m, prm(RIGHT, 0),
                     lambda rec, mg, tot, clip, ev: not rec[0]["keepers_seen"].any() and list(rec[0]["n_def"]) == [2, 1] and rec[0, 1]["status"] == OR.TOO_FEW
                     and rec[0, 0]["line_qx"] == 70 * Q))
    v, c, m = table([(P, 0, 86.0), (P, 1, 85.0), (P, 1, 70.0), (G, None, 20.0)])
    out.append(_case("keeper_in_the_wrong_half", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: list(rec[0]["keepers_seen"]) == [0, 1] and flags(rec, 0, 0) & OR.KEEPER_ASSUMED and rec[0, 0]["line_qx"] == 85 * Q
                     and rec[0, 1]["second_col"] == 0 and not flags(rec, 0, 1) & OR.KEEPER_ASSUMED))
    v, c, m = table([(P, 0, 99.0), (P, 1, 85.0), (G, None, 100.0), (G, None, 98.0)])
    out.append(_case("two_keepers_in_one_half", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: rec[0, 0]["keepers_seen"] == 2 and rec[0, 0]["n_def"] == 3 and rec[0, 0]["second_col"] == 3 and rec[0, 0]["line_qx"] == 98 * Q
                     and mg[0, 0] == Q))
    v, c, m = table([(P, 0, 86.0), (P, 1, 85.0)])
    out.append(_case("one_defender_no_keeper_not_assumed_is_too_few", v, c, m, prm(RIGHT, 0),
                     lambda rec, mg, tot, clip, ev: (rec[0]["status"] == OR.TOO_FEW).all() and (mg == OR.NONE).all() and list(rec[0]["n_att"]) == [1, 1] and not rec[0]["flags"].any()
                     and (rec[0]["second_col"] == -1).all() and (tot["rows"] == 0).all() and (tot["max_margin"] == OR.NONE).all()))
    out.append(_case("one_defender_no_keeper_assumed_is_ok", v, c, m, prm(RIGHT, 1),
                     lambda rec, mg, tot, clip, ev: (rec[0]["status"] == OR.OK).all() and mg[0, 0] == Q and rec[0, 0]["second_col"] == 1 and (tot["rows"] == 1).all()))
    # ---- direction -----------------------------------------------------------------------------------------------------------------------
    wv, wc, wm = walk(7, 4, 6, 0.1)
    wq = np.floor(wv * Q + 0.5) / Q                                            # (on the grid of q: 105 - x is exact)
    mirrored = wq.copy(); mirrored[:, :, 0] = 105.0 - wq[:, :, 0]
    out.append(_case("forced_right", wq, wc, wm, prm(RIGHT), lambda rec, mg, tot, clip, ev: clip[0]["direction"] == RIGHT and (rec["status"] != OR.NO_DIRECTION).all()
                     and clip[0]["neg"] > clip[0]["pos"] and consistent(rec, mg, tot, clip, ev)))
    out.append(_case("forced_left_on_the_mirrored_table", mirrored, wc, wm, prm(LEFT),
                     lambda rec, mg, tot, clip, ev: clip[0]["direction"] == LEFT and mg.tobytes() == reference("forced_right")[1].tobytes()
                     and tot.tobytes() == reference("forced_right")[2].tobytes() and consistent(rec, mg, tot, clip, ev)))
    out.append(_case("auto_resolved_right", wq, wc, wm, prm(AUTO), lambda rec, mg, tot, clip, ev: clip[0]["direction"] == RIGHT and clip[0]["requested"] == AUTO
                     and rec.tobytes() == reference("forced_right")[0].tobytes()))
    out.append(_case("auto_resolved_left", mirrored, wc, wm, prm(AUTO), lambda rec, mg, tot, clip, ev: clip[0]["direction"] == LEFT and clip[0]["pos"] > clip[0]["neg"]
                     and rec.tobytes() == reference("forced_left_on_the_mirrored_table")[0].tobytes()))
    v, c, m = table([(P, 0, 30.0), (P, 1, 70.0), (P, 1, 60.0), (BALL, None, 50.0)], 3)
    v[0, 1, 0] = 90.0; v[0, 2, 0] = 65.0                                       # row 0 votes neg, row 1 pos, row 2 zero
    no_direction = lambda rec, mg, tot, clip, ev: ((rec["status"] == OR.NO_DIRECTION).all() and (mg == OR.NONE).all() and not rec["n_att"].any() and not rec["flags"].any()
                                                   and clip[0]["direction"] == 0 and (tot["rows"] == 0).all() and (tot["max_margin"] == OR.NONE).all())
    out.append(_case("auto_tied", v, c, m, prm(AUTO),
                     lambda rec, mg, tot, clip, ev: (clip[0]["neg"], clip[0]["pos"], clip[0]["zero"]) == (1, 1, 1) and no_direction(rec, mg, tot, clip, ev)))
    v = v.copy(); v[0, 1:] = NAN; v[1:, 0] = NAN
    out.append(_case("auto_with_no_row_holding_both_groups", v, c, m, prm(AUTO),
                     lambda rec, mg, tot, clip, ev: (clip[0]["neg"], clip[0]["pos"], clip[0]["zero"]) == (0, 0, 0) and no_direction(rec, mg, tot, clip, ev)))
    # ---- presence and mapping ------------------------------------------------------------------------------------------------------------
    v, c, m = table([(P, 0, 90.0)] * 6 + [(P, 1, 85.0), (P, 1, 70.0), (G, None, 100.0), (BALL, None, 50.0)])
    v[0, 0] = (NAN, 30.0); v[1, 0] = (90.0, NAN); v[2, 0] = (INF, 30.0); v[3, 0] = (90.0, -INF); v[4, 0] = (1024.5, 30.0); v[5, 0] = (90.0, -1024.5)
    out.append(_case("absent_cells_nan_inf_and_beyond_1024", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: (mg[:6] == OR.NONE).all() and rec[0, 0]["n_att"] == 0 and (rec[0, 0]["max_margin"], rec[0, 0]["max_col"]) == (OR.NONE, -1)
                     and rec[0, 0]["status"] == OR.OK and rec[0, 1]["status"] == OR.TOO_FEW and (tot[:6]["rows"] == 0).all()))
    v, c, m = table([(P, 0, 1024.0), (P, 0, 90.0), (P, 1, 85.0), (P, 1, -1024.0), (G, None, 100.0), (BALL, None, 50.0)])
    v[1, 0, 1] = -1024.0
    out.append(_case("present_at_exactly_1024", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: list(mg[:2, 0]) == [2 ** 20 - 85 * Q, 5 * Q] and rec[0, 0]["n_att"] == 2 and rec[0, 0]["max_col"] == 0
                     and rec[0, 1]["n_att"] == 2 and mg[3, 0] == OR.U_MAX + 2 ** 20 - 55 * Q and flags(rec, 0, 1) == OR.BY_BALL | OR.KEEPER_ASSUMED and consistent(rec, mg, tot, clip, ev)))
    v, c, m = table([(P, 0, 86.0), (P, 1, 85.0), (P, 1, 70.0), (G, None, 100.0)], 2)
    out.append(_case("table_without_a_ball_column", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: all(flags(rec, r, a) & OR.NO_BALL for r in (0, 1) for a in (0, 1)) and rec[0, 0]["line_qx"] == 85 * Q))
    v, c, m = table([(P, 0, 86.0), (P, 1, 85.0), (P, 1, 70.0), (G, None, 100.0), (BALL, None, NAN)], 2)
    out.append(_case("table_flagged_no_ball", v, c, m, prm(RIGHT), lambda rec, mg, tot, clip, ev: all(flags(rec, r, a) & OR.NO_BALL for r in (0, 1) for a in (0, 1))
                     and rec.tobytes() == reference("table_without_a_ball_column")[0].tobytes(), events(), True))
    v, c, m = table([(P, 0, 86.0), (P, 1, 85.0), (P, 1, 70.0), (G, None, 100.0), (BALL, None, 50.0)])
    out.append(_case("first_mapping_entry_counts", v, c, [(1, 0), (2, 1), (3, 1), (1, 1), (2, 0), (3, -1)], prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: list(tot["group"]) == [0, 1, 1] and list(clip[0]["n_members"]) == [1, 2] and mg[0, 0] == Q))
    c2 = [(P, 1, 0), (P, 2, 0), (P, 3, 0), (P, 4, 0), (P, 5, 0), (P, 2, 1), (BOUNDARY, 0, 0), (G, 9, 0), (G, 9, 1), (BALL, 0, 0), (BALL, 0, 1)]
    v = still([(86.0, 30.0), (85.0, 31.0), (70.0, 32.0), (99.0, 33.0), (99.5, 34.0), (600.0, 300.0), (0.0, 0.0), (100.0, 35.0), (900.0, 400.0), (50.0, 36.0), (640.0, 360.0)])
    out.append(_case("negative_and_missing_mapping_entries_and_other_columns", v, c2, {1: 0, 2: 1, 3: 1, 4: -1, 9: 0}, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: list(tot["col"]) == [0, 1, 2] and rec[0, 0]["n_def"] == 3 and rec[0, 0]["line_qx"] == 85 * Q and clip[0]["n_keepers"] == 1
                     and rec[0, 0]["n_att"] == 1))
    v, c, m = table([(P, 0, 86.0), (P, 0, 60.0), (G, None, 100.0), (G, None, 3.0), (BALL, None, 50.0)])
    out.append(_case("group_with_no_members", v, c, m, prm(RIGHT),
                     lambda rec, mg, tot, clip, ev: rec[0, 0]["status"] == OR.TOO_FEW and (rec[0, 0]["n_def"], rec[0, 0]["keepers_seen"]) == (1, 1) and rec[0, 1]["status"] == OR.OK
                     and (rec[0, 1]["n_att"], rec[0, 1]["max_col"], rec[0, 1]["max_margin"], rec[0, 1]["n_def"]) == (0, -1, OR.NONE, 3) and list(clip[0]["n_members"]) == [2, 0]
                     and len(tot) == 2 and (mg == OR.NONE).all()))
    # ---- wave and block edges ------------------------------------------------------------------------------------------------------------
    for n in (63, 64, 65, 130):
        out.append(_members_case(n, n))
    for rows in (1, 5, 257, 300):
        out.append(_case("rows_%d" % rows, *walk(rows, 3, rows, 0.35 if rows > 1 else 0.0, keepers=1), prm(AUTO if rows > 1 else RIGHT),
                         lambda rec, mg, tot, clip, ev, rows=rows: consistent(rec, mg, tot, clip, ev) and clip[0]["direction"] == RIGHT
                         and (rows < 100 or ({OR.OK, OR.TOO_FEW} <= set(rec["status"].ravel().tolist()) and tot["off_rows"].any() and clip[0]["neg"] > 200))))
    BY_NAME_ = {c["name"]: c for c in out}
    # ---- events --------------------------------------------------------------------------------------------------------------------------
    # columns: 0 passer, 1 and 2 receivers (group 0); 3, 4, 5 defenders (group 1); 6 keeper; 7 ball.  Row 0: the release; row 1: the reception; row 2: the
    # defenders 3 .. 5 absent (TOO_FEW for a = 0: the keeper alone); row 3: receiver 1 and the ball absent.  Defender 5 stands in front of the ball at the release and
    # behind it at the reception: the pass does not take him out
    v, c, m = table([(P, 0, 60.0), (P, 0, 80.0 + 307.0 / Q), (P, 0, 80.0 - 307.0 / Q), (P, 1, 80.0), (P, 1, 70.0), (P, 1, 65.0), (G, None, 100.0), (BALL, None, 60.0)], 4)
    v[7, 1, 0] = 85.0; v[5, 1, 0] = 88.0; v[3:6, 2] = NAN; v[1, 3] = NAN; v[7, 3] = NAN
    PASS, TURN, UNK = PR.PASS, PR.TURNOVER, PR.UNKNOWN
    ev = events((PASS, 0, 1, 0, 1), (PASS, 0, 2, 0, 1), (TURN, 0, 3, 0, 1), (UNK, 0, 1, 0, 1), (7, 0, 1, 0, 1), (PASS, 0, 6, 0, 1), (PASS, 0, 1, 2, 3), (PASS, 0, 2, 3, 3),
                (PASS, 0, 1, 3, 3), (PASS, 0, 1, 0, 2), (PASS, 0, 1, 0, 3), (PASS, 3, 4, 0, 1))
    for tol, verdicts in ((0.0, (OR.OFFSIDE, OR.ONSIDE)), (0.25, (OR.OFFSIDE, OR.ONSIDE)), (0.5, (OR.CLOSE, OR.CLOSE))):
        def check(rec, mg, tot, clip, e, verdicts=verdicts):
            return (list(e["status"]) == [0, 0, 1, 1, 1, 2, 3, 0, 3, 0, 0, 0] and tuple(e["verdict"][:2]) == verdicts and list(e["margin"][:2]) == [307, -307]
                    and list(e["bypassed"]) == [2, 2, -1, -1, -1, -1, -1, -1, -1, 0, -1, 0] and list(e["group"]) == [0, 0, -1, -1, -1, -1, 0, 0, 0, 0, 0, 1]
                    and e[0]["line_qx"] == 80 * Q and e[0]["n_off"] == 1 and rec[2, 0]["status"] == OR.TOO_FEW and e[7]["margin"] == -307
                    and not e["verdict"][[2, 3, 4, 5, 6, 8]].any() and (e["margin"][[2, 3, 4, 5, 6, 8]] == OR.NONE).all())
        out.append(_case("passes_at_tolerance_%g" % tol, v, c, m, prm(RIGHT, 1, tol), check, ev))
    v2 = v.copy(); v2[1, 0, 0] = 80.0
    out.append(_case("level_pass_at_tolerance_0_is_onside", v2, c, m, prm(RIGHT, 1, 0.0), lambda rec, mg, tot, clip, e: (e[0]["margin"], e[0]["verdict"]) == (0, OR.ONSIDE),
                     events((PASS, 0, 1, 0, 1))))
    out.append(_case("zero_events", v, c, m, prm(RIGHT), lambda rec, mg, tot, clip, e: len(e) == 0 and rec[0, 0]["status"] == OR.OK, events()))
    out.append(_case("events_with_the_direction_voted", v, c, m, prm(AUTO),
                     lambda rec, mg, tot, clip, e: clip[0]["direction"] == RIGHT and e[0]["status"] == OR.EV_OK and e[0]["margin"] == 307, events((PASS, 0, 1, 0, 1))))
    tied = BY_NAME_["auto_tied"]
    out.append(_case("events_without_a_direction_have_no_line", tied["values"], tied["columns"], tied["mapping"], prm(AUTO),
                     lambda rec, mg, tot, clip, e: clip[0]["direction"] == 0 and list(e["status"]) == [OR.EV_NO_LINE, OR.EV_NOT_PASS] and list(e["group"]) == [1, -1],
                     events((PASS, 0, 1, 0, 1), (TURN, 1, 0, 1, 2))))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
PARTS = ("rows", "margins", "totals", "clip", "events")


@functools.lru_cache(maxsize=None)
def reference(name):
    """the contract's (records, margins, totals, clip record, event records) of a case (read only: shared by the tests)"""
    c = BY_NAME[name]
    out = OR.offside(c["values"], c["columns"], c["mapping"], c["p"], c["events"], c["no_ball"])
    for a in out:
        a.setflags(write=False)
    return out
