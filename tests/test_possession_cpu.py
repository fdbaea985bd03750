"""The possession contract without a GPU (tests/possession_ref.py; the kernels of csrc/possession.hip are held against it in tests/test_gpu_possession.py):
its two formulations (max-scans; a row-by-row state machine) agree bit for bit on every constructed table of tests/possession_cases.py and on seeded
random tables; every named case forces the edge it is named after; the invariants of the event fields hold; the aggregates eagle_amd/possession.py sums
on the host equal the contract's and a table worked out by hand."""
import numpy as np
import pytest

import possession_cases as PC
import possession_ref as PR

NAMES = [c["name"] for c in PC.CASES]
A, B, C = PC.col_of(0), PC.col_of(1), PC.col_of(2)


def _same(a, b):
    return (np.array_equal(a["cand"], b["cand"]) and np.array_equal(a["owner"], b["owner"]) and np.array_equal(np.isnan(a["dist"]), np.isnan(b["dist"]))
            and np.array_equal(a["dist"], b["dist"], equal_nan=True) and a["events"].dtype == b["events"].dtype and a["events"].tobytes() == b["events"].tobytes())


def _invariants(res, c):
    ev, rows = res["events"], len(res["owner"])
    assert np.all(np.diff(ev["row"]) > 0)                                               # ascending rows
    for e in ev:
        r = int(e["row"])
        assert 1 <= r < rows and not res["seg"][r]
        assert e["receive_row"] == r - c["min_hold"] + 1 and e["release_row"] < e["receive_row"]
        assert e["from_col"] == res["owner"][r - 1] >= 0 and e["to_col"] == res["owner"][r] >= 0 and e["from_col"] != e["to_col"]
        assert res["conf"][r] and res["conf"][e["release_row"]] and res["cand"][e["release_row"]] == e["from_col"] and res["cand"][e["receive_row"]] == e["to_col"]
        assert e["duration"] > 0 and np.isfinite(e["length"]) and (e["reserved"] == 0).all()
    own = res["owner"]
    assert np.all((own == -1) | np.isin(own, res["persons"])) and np.all(own[~res["ball"]] == -1)
    assert np.array_equal(np.isnan(res["dist"]), ~res["ball"] | (np.isnan(res["dist"]) & (res["cand"] < 0)))


@pytest.mark.parametrize("name", NAMES)
def test_formulations_agree_and_invariants_hold(name):
    c = PC.BY_NAME[name]
    res = PC.reference(name)
    assert _same(res, PR.state_machine(*PC.args(c), no_ball=c["no_ball"]))
    _invariants(res, c)


def _random_table(seed):
    r = np.random.default_rng(seed)
    rows, n = int(r.integers(0, 48)), int(r.integers(0, 5))
    cols = PC.BOUNDS[: int(r.integers(0, 5))] + [((PC.P, PC.G)[int(r.integers(0, 2))], i + 1, 0) for i in range(n)]
    if r.random() < 0.9:
        cols.insert(int(r.integers(0, len(cols) + 1)), (PC.BALL, 0, 0))
    cols.append((PC.P, 1, 1))
    v = r.uniform(0, 6, (len(cols), rows, 2)).round(int(r.integers(0, 3)))               # coarse coordinates: ties and exact radii happen
    v[r.random(v.shape) < 0.08] = np.nan
    v[r.random(v.shape) < 0.01] = np.inf
    frames = np.cumsum(r.integers(1, 5, rows)).astype(np.int32)
    mapping = None if r.random() < 0.2 else {i + 1: int(r.integers(-1, 3)) for i in range(n) if r.random() < 0.8}
    return {"values": v, "frames": frames, "columns": cols, "mapping": mapping, "fps": int(r.integers(1, 30)), "radius": float(r.choice([0.5, 1.0, 2.0, 3.0, 1024.0])),
            "min_hold": int(r.integers(1, 5)), "max_gap": int(r.integers(1, 5)), "no_ball": bool(r.random() < 0.05)}


def test_formulations_agree_on_random_tables():
    events = owned = 0
    for seed in range(300):
        c = _random_table(seed)
        res = PR.possession(*PC.args(c), no_ball=c["no_ball"])
        assert _same(res, PR.state_machine(*PC.args(c), no_ball=c["no_ball"])), seed
        _invariants(res, c)
        events += len(res["events"])
        owned += int((res["owner"] >= 0).sum())
    assert events > 100 and owned > 500                                                # the tables are not trivially empty


# ---- every named case forces its edge ------------------------------------------------------------------------------------------------------
def _ref(name):
    return PC.reference(name), PC.BY_NAME[name]


def test_cases_who_takes_part():
    res, c = _ref("no_person_columns")
    assert res["persons"] == [] and res["ball"].all() and np.isnan(res["dist"]).all() and (res["cand"] == -1).all() and not len(res["events"])
    res, c = _ref("one_person")
    assert len(res["persons"]) == 1 and (res["owner"][1:] == A).all() and res["cand"][3] == -1 and not len(res["events"])
    assert len(_ref("persons22")[0]["persons"]) == 22 and len(_ref("persons257")[0]["persons"]) == 257
    for name in ("persons22", "persons257"):
        res, c = _ref(name)
        assert len(res["events"]) > 3 and len(set(res["cand"].tolist())) > 4 and (~res["ball"]).any() and max(res["persons"]) == len(c["columns"]) - 3
    res, c = _ref("no_ball_column")
    assert res["ball_col"] == -1 and not res["ball"].any() and (res["owner"] == -1).all() and np.isnan(res["dist"]).all()
    res, c = _ref("no_ball_flag")
    assert c["no_ball"] and res["ball_col"] == -1 and (res["owner"] == -1).all()
    assert _same(res, PR.possession(*PC.args(c), no_ball=False))                        # the flag says the ball column is all NaN: the same answer without it


def test_cases_ball_absent():
    res, c = _ref("ball_absent_first_row")
    assert not res["ball"][0] and res["seg"][:2].tolist() == [True, False] and res["owner"].tolist() == [-1, -1, A, A, A, B] and len(res["events"]) == 1
    res, c = _ref("ball_absent_last_row")
    assert not res["ball"][-1] and res["owner"].tolist() == [-1, A, A, A, B, -1] and np.isnan(res["dist"][-1])
    res, c = _ref("ball_absent_interior_rows")
    assert res["owner"].tolist() == [-1, A, -1, -1, A, A, B, -1, -1, -1, B, B, A] and res["events"]["row"].tolist() == [6, 12]
    res, c = _ref("person_nan_where_they_would_win")
    assert res["cand"].tolist() == [A, A, -1, -1, B, B] and res["dist"][2] > 9.0 and res["dist"][3] > 9.0      # the nearest PRESENT person is 10 m away
    assert res["owner"].tolist() == [-1, A, A, A, A, B]


def test_cases_ties_and_radius():
    res, c = _ref("equidistant_earlier_column_wins")
    assert res["cand"].tolist() == [4, 4, 4, 4] and (res["dist"] == 1.5).all()
    res, c = _ref("distance_at_radius_and_one_ulp_beyond")
    assert res["cand"].tolist() == [4, -1, 4, -1] and res["dist"][0] == 2.0 == res["dist"][2] and res["dist"][1] > 2.0 and res["dist"][3] > 2.0
    assert res["dist"][1] - 2.0 < 4e-15 and res["owner"].tolist() == [4, 4, 4, 4]


def test_cases_min_hold():
    rows = {1: [6, 14, 21], 2: [7, 15, 22], 5: [10, 18]}
    for mh, ev in rows.items():
        res, c = _ref("min_hold_%d" % mh)
        assert c["min_hold"] == mh and res["events"]["row"].tolist() == ev and res["owner"][mh - 1] == A and (res["owner"][: mh - 1] == -1).all()
    res, c = _ref("min_hold_5")
    assert res["owner"][-1] == C and res["run"][-1] == 3                                 # the last run of A is too short: C keeps the ball
    res, c = _ref("min_hold_beyond_rows")
    assert c["min_hold"] > len(res["owner"]) and (res["cand"] >= 0).sum() == 22 and (res["owner"] == -1).all() and not res["conf"].any()
    res, c = _ref("run_broken_one_short")
    assert res["run"][5:9].tolist() == [1, 2, 3, 4] and res["run"][10:14].tolist() == [1, 2, 3, 4] and res["events"]["row"].tolist() == [19]
    assert (res["owner"][4:19] == A).all() and res["events"]["release_row"][0] == 4 and res["events"]["receive_row"][0] == 15


def test_cases_frame_gaps():
    res, c = _ref("gap_exact_inside_run")
    assert c["frames"][3] - c["frames"][2] == c["max_gap"] and not res["seg"][3] and res["owner"].tolist() == [-1, A, A, A, A, A, B]
    res, c = _ref("gap_beyond_inside_run")
    assert c["frames"][3] - c["frames"][2] == c["max_gap"] + 1 and res["seg"][3] and res["owner"].tolist() == [-1, A, A, -1, A, A, B] and res["run"][3] == 1
    res, c = _ref("gap_exact_inside_flight")
    assert res["cand"][2:4].tolist() == [-1, -1] and res["owner"].tolist() == [-1, A, A, A, A, B, B] and res["events"]["row"].tolist() == [5]
    assert res["events"]["release_row"][0] == 1 and res["events"]["duration"][0] == (c["frames"][4] - c["frames"][1]) / 5.0
    res, c = _ref("gap_beyond_inside_flight")
    assert res["seg"][3] and res["owner"].tolist() == [-1, A, A, -1, -1, B, B] and not len(res["events"])
    res, c = _ref("gap_exact_at_owner_change")
    assert res["owner"].tolist() == [A, A, B, B, A] and res["events"]["row"].tolist() == [2, 4]
    res, c = _ref("gap_beyond_at_owner_change")
    assert res["owner"].tolist() == [A, A, B, B, A] and res["seg"][2] and res["events"]["row"].tolist() == [4]      # the change at row 2 is no event


def test_cases_kinds():
    assert _ref("change_within_team")[0]["events"]["kind"].tolist() == [PR.PASS, PR.PASS]
    assert _ref("change_across_teams")[0]["events"]["kind"].tolist() == [PR.TURNOVER, PR.TURNOVER]
    res, c = _ref("change_unknown_team")
    gk = PC.col_of(3)
    assert c["columns"][gk][0] == PC.G and PC.GK_ID not in c["mapping"] and c["mapping"][2] < 0
    assert res["events"]["to_col"].tolist() == [gk, B, C, A] and res["events"]["kind"].tolist() == [PR.UNKNOWN, PR.UNKNOWN, PR.UNKNOWN, PR.PASS]
    res, c = _ref("no_mapping")
    assert c["mapping"] is None and res["events"]["kind"].tolist() == [PR.UNKNOWN, PR.UNKNOWN]
    res, c = _ref("a_loose_a")
    assert (res["cand"] == -1).sum() == 4 and (res["owner"][1:] == A).all() and not len(res["events"])


@pytest.mark.parametrize("n", PC.ROWS)
def test_cases_seams(n):
    res, c = _ref("alternating_%d" % n)
    assert len(res["owner"]) == n and res["events"]["row"].tolist() == list(range(1, n))          # an event at every row but the first
    res, c = _ref("random_%d" % n)
    assert len(res["owner"]) == n and res["seg"][1:].sum() >= (n > 60) and (n < 60 or len(set(res["owner"].tolist())) > 2)


def test_cases_seams_hold():
    for mh in (2, 3):
        res, c = _ref("seams_hold%d" % mh)
        ev = set(res["events"]["row"].tolist())
        heads = set(np.flatnonzero(res["head"]).tolist())
        for seam, j in ((64, 0), (128, 1), (192, 2), (1024, 0), (2048, 1), (3072, 2), (4096, 1)):
            assert seam - j in heads and seam - j + mh - 1 in ev and seam - j + 2 * mh - 1 in ev
        assert {64, 1024}.issubset(heads) and (4096 in ev if mh == 2 else 3072 in ev)               # a head and a confirmation exactly on a chunk's first row


# ---- the aggregates ------------------------------------------------------------------------------------------------------------------------
def test_aggregates_of_the_module_equal_the_contract_and_the_hand_table():
    from eagle_amd import lib, possession as po
    c = PC.hand_table()
    res = PR.possession(*PC.args(c))
    assert res["owner"].tolist() == [-1, A, A, A, A, B, B, C, C, C, A]
    ev = res["events"]
    assert ev["row"].tolist() == [5, 7, 10] and ev["kind"].tolist() == [PR.TURNOVER, PR.TURNOVER, PR.PASS]
    assert ev["release_row"].tolist() == [2, 5, 8] and ev["receive_row"].tolist() == [4, 6, 9] and ev["duration"].tolist() == [2 / 5.0, 1 / 5.0, 1 / 5.0]
    players, teams, matrix = PR.aggregates(res, c["frames"], c["columns"], c["fps"])
    d = 1 / 5.0
    hand = [{"id": 1, "type": "Player", "rows": 5, "seconds": d + d + d, "passes_made": 0, "passes_received": 1, "turnovers_lost": 1, "turnovers_won": 0},
            {"id": 2, "type": "Player", "rows": 2, "seconds": d, "passes_made": 0, "passes_received": 0, "turnovers_lost": 1, "turnovers_won": 1},
            {"id": 3, "type": "Player", "rows": 3, "seconds": d + d, "passes_made": 1, "passes_received": 0, "turnovers_lost": 0, "turnovers_won": 1}]
    t0 = d + d + d + d + d
    assert players == hand and matrix == {(3, 1): 1} and teams == {0: t0 / (t0 + d), 1: d / (t0 + d)}
    assert teams[0] == pytest.approx(5 / 6)
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    assert lib.EVENT_DTYPE == PR.EVENT_DTYPE and lib.EVENT_DTYPE.itemsize == 80
    got = po.summarise(res["owner"], ev, c["frames"], cols, c["mapping"], c["fps"], c["max_gap"])
    assert got["players"] == hand and got["teams"] == teams and got["pass_matrix"] == matrix
    assert [o["id"] for o in got["owner"]] == [None, 1, 1, 1, 1, 2, 2, 3, 3, 3, 1] and got["owner"][7] == {"frame": 8, "id": 3, "type": "Player"}
    assert [(e["frame"], e["kind"], e["from_id"], e["to_id"], e["release_frame"], e["receive_frame"]) for e in got["events"]] == \
        [(5, "turnover", 1, 2, 2, 4), (8, "turnover", 2, 3, 5, 6), (11, "pass", 3, 1, 9, 10)]
    assert got["events"][0]["length"] == float(ev["length"][0]) and po.from_json(__import__("json").loads(__import__("json").dumps(po.to_json(got)))) == got
    # every case: the module's sums are the contract's (goalkeepers, unknown teams, segments without a ball, min_hold 1 across a gap)
    for case in PC.CASES:
        res = PC.reference(case["name"])
        cols = np.array([(k, i, v, 0) for k, i, v in case["columns"]], lib.POSTCOL_DTYPE)
        got = po.summarise(res["owner"], res["events"], case["frames"], cols, case["mapping"], case["fps"], case["max_gap"])
        players, teams, matrix = PR.aggregates(res, case["frames"], case["columns"], case["fps"])
        assert got["players"] == players and got["teams"] == teams and got["pass_matrix"] == matrix, case["name"]
