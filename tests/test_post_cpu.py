"""tests/post_ref.py, the numpy restatement of the reference's clip post-processor, against tests/golden/post_golden.json (what the reference
itself returns under pandas; written by tests/golden/make_post_golden.py): column order, kept rows, every double by bit pattern, NaN positions and
the rows of format_data, for every constructed clip and both ``smooth`` values — and, per clip, the edge it is named after."""
import json
import os

import numpy as np
import pytest

import post_cases
import post_ref

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_golden.json")))["cases"]
# where the reference raises, the restatement is the definition (post_ref's docstring) and there is nothing to compare
DIVERGES = {"empty": "all", "single_frame": "all", "ball_none": "all", "ball_one_sighting": "all"}
NAMES = [c["name"] for c in post_cases.CASES]


def golden_values(g):
    """The golden's cells -> float64 [columns][rows][2], NaN = null."""
    v = np.full((len(g["columns"]), len(g["rows"]), 2), np.nan)
    for c, col in enumerate(g["values"]):
        for r, cell in enumerate(col):
            if cell is not None:
                v[c, r] = [np.nan if e is None else e for e in cell]
    return v


def golden_cell(cell):
    return None if cell is None or (cell[0] is None and cell[1] is None) else tuple(np.nan if e is None else e for e in cell)


def golden_format(g):
    """The golden's format_data rows: stored as references into the table (the generator checked that every value IS its table cell)."""
    v = golden_values(g)

    def cell(c, r):
        return golden_cell([None if np.isnan(e) else float(e) for e in v[c, r]])

    def item(it, r):
        d = {"ID": it[0], "Coordinates": cell(it[2], r)}
        return d if it[1] is None else dict(d, Type=it[1])

    return [{"Boundaries": [cell(c, r) for c in row[0]], "Coordinates": [item(it, r) for it in row[1]], "Coordinates_video": [item(it, r) for it in row[2]]}
            for r, row in enumerate(row for count, row in g["format"] for _ in range(count))]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def table_of(name, smooth):
    case = post_cases.BY_NAME[name]
    return post_ref.process_data(post_cases.coords_of(case), case["team_mapping"], smooth=smooth)


def column(t, name):
    return t["values"][t["columns"].index(name)]


def test_golden_is_of_these_cases():
    assert list(GOLDEN) == NAMES
    for case in post_cases.CASES:
        clip = GOLDEN[case["name"]]["clip"]
        assert clip["frames"] == json.loads(json.dumps(case["frames"])) and clip["fps"] == case["fps"]
        assert clip["team_mapping"] == {str(k): v for k, v in case["team_mapping"].items()}


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_ref_equals_golden(name, smooth):
    g = GOLDEN[name][f"smooth{int(smooth)}"]
    t = table_of(name, smooth)
    if DIVERGES.get(name) == "all":
        assert "raises" in g, "the reference no longer raises here: compare it"
        return
    assert t["rows"] == g["rows"] and t["columns"] == g["columns"]
    assert t["team_mapping"] == {int(k): v for k, v in g["team_mapping"].items()}
    assert same_bits(t["values"], golden_values(g))
    fmt, gf = post_ref.format_data(t), golden_format(g)
    assert len(fmt) == len(gf)
    for a, b in zip(fmt, gf):
        assert json.dumps(a, sort_keys=False) == json.dumps(b, sort_keys=False)      # (NaN == NaN as text; key and item order included)
    rows = post_ref.raw_data_rows(t)
    assert [list(r) for r in rows] == [g["columns"]] * len(g["rows"])


# ---- the edge each clip is named after ---------------------------------------------------------------------------------------------------
def test_empty_and_degenerate():
    for name in ("empty", "no_persons"):
        for smooth in (False, True):
            t = table_of(name, smooth)
            assert t["rows"] == [] and t["columns"] == [] and t["values"].shape == (0, 0, 2) and t["team_mapping"] == {}
            assert post_ref.format_data(t) == [] and post_ref.raw_data_rows(t) == []
    t = table_of("single_frame", False)
    assert t["rows"] == [0] and t["columns"] == list(post_ref.BOUNDARIES) + ["Player_1", "Player_1_video", "Ball", "Ball_video"]
    assert t["flags"] & post_ref.FLAG_NO_BALL and np.isnan(column(t, "Ball")).all() and tuple(column(t, "Player_1_video")[0]) == (110.0, 300.0)
    assert np.isnan(table_of("single_frame", True)["values"]).all()           # smoothing forgets row 0 and has nothing to bring it back from


def test_ids_and_gaps():
    t = table_of("appear_vanish_return", False)
    assert not np.isnan(column(t, "Player_5_video")).any() and not np.isnan(column(t, "Player_5")).any()
    v = column(t, "Player_5_video")
    assert v[6, 0] == (v[9, 0] - v[4, 0]) / 5.0 * 2.0 + v[4, 0]
    t = table_of("gap_at_both_ends", False)
    p = np.isnan(column(t, "Player_5_video")[:, 0])
    assert p[:3].all() and p[17:].all() and not p[3:17].any()                   # "inside" leaves both ends, fills rows 9 and 10
    b = np.isnan(column(t, "Bottom_Left")[:, 0])
    assert b[:2].all() and b[19] and not b[2:19].any()
    assert not np.isnan(column(t, "Ball")).any()                                # the ball is filled to both ends
    t = table_of("rare_id_dropped", False)
    assert len(t["rows"]) == 101 and "Player_77" not in t["columns"] and "Player_77_video" not in t["columns"] and "Player_78_video" in t["columns"]


def test_goalkeeper_fold():
    for name in ("goalkeeper_fold", "goalkeeper_fold_overlap"):
        t = table_of(name, False)
        assert "Player_9" not in t["columns"] and "Player_9_video" not in t["columns"] and "Goalkeeper_9_video" in t["columns"]
    v = column(table_of("goalkeeper_fold", False), "Goalkeeper_9_video")
    assert tuple(v[0]) == (710.0, 500.0) and tuple(v[4]) == (724.0, 505.0) and not np.isnan(v).any()       # a Player row, a Goalkeeper row, row 3 filled
    v = column(table_of("goalkeeper_fold_overlap", False), "Goalkeeper_9_video")
    assert tuple(v[5]) == (725.0, 505.0) and tuple(v[9]) == (797.0, 529.0)       # both present: the Player's value wins


def test_person_coordinates():
    t = table_of("no_transformed_coordinates", False)
    raw = post_ref.create_dataframe(post_cases.coords_of(post_cases.BY_NAME["no_transformed_coordinates"]))[1]
    assert np.isnan(raw["Player_5"][[2, 3, 7]]).all() and not np.isnan(raw["Player_5_video"]).any()
    assert not np.isnan(column(t, "Player_5")).any()                              # ... and the pitch gaps are interpolated afterwards
    t = table_of("frames_dropped", False)
    assert t["rows"] == [0, 1, 2, 3, 4, 5, 11, 12, 14, 15, 16, 17, 18, 19]
    v = column(t, "Player_5_video")[:, 0]                                         # missing on rows 4, 5, 6 (frames 4, 5, 11): thirds between rows 3 and 7, whatever the frame numbers
    assert v[5] == (v[7] - v[3]) / 4.0 * 2.0 + v[3]


def test_ball():
    for name in ("ball_none", "ball_one_sighting"):
        t = table_of(name, False)
        assert t["flags"] & post_ref.FLAG_NO_BALL and np.isnan(column(t, "Ball")).all() and np.isnan(column(t, "Ball_video")).all()
        assert t["columns"][-2:] == ["Ball", "Ball_video"]
    t = table_of("ball_two_sightings", False)
    v = column(t, "Ball_video")
    assert t["flags"] == 0 and tuple(v[0]) == tuple(v[2]) == (317.0, 206.0) and tuple(v[9]) == tuple(v[7]) and v[4, 0] == (v[7, 0] - v[2, 0]) / 5.0 * 2.0 + v[2, 0]
    t = table_of("ball_candidates_tie", False)
    v, w = column(t, "Ball_video"), column(t, "Ball")
    assert tuple(v[2]) == (303.0, 400.0) and tuple(w[2]) == (30.0, 40.0)           # tie: the first minimum in confidence order
    assert tuple(v[4]) == (303.0, 400.0) and tuple(w[4]) == (30.0, 40.0)           # ... which is the other box's list position here
    assert tuple(v[6]) == (123.0, 80.0) and tuple(w[6]) == (12.0, 8.0)             # nearest to the prediction (the origin), not the most confident
    t = table_of("ball_no_homography", False)
    assert tuple(column(t, "Ball")[2]) == tuple(column(t, "Ball_video")[2])         # no homography: the image point on the pitch too
    assert tuple(column(t, "Ball")[6]) == (94.0, 31.0)                              # 2 candidates: (313, 220) without a pitch point is farther than (200 % 106, 100 % 69)
    det = [None] * 4 + [[(1.0, 1.0)], None, [(2.0, 2.0)]] + [None] * 3
    assert post_ref.parse_ball_detections(det)[1] and not post_ref.parse_ball_detections(det[:6])[1]
    assert table_of("ball_long_init_window", False)["flags"] == 0


def test_smoothing():
    for name, n in (("smooth_odd_rows", 15), ("smooth_even_rows", 16)):
        plain, t = table_of(name, False), table_of(name, True)
        for c in range(len(t["columns"])):
            a, b = plain["values"][c], t["values"][c]
            assert same_bits(a[1::2], b[1::2])                                    # odd rows are kept
            assert np.isnan(b[0]).all() and (n % 2 == 0 or np.isnan(b[n - 1]).all())        # the first row, and an even last row, have one neighbour only
        a, b = column(plain, "Player_3_video")[:, 0], column(t, "Player_3_video")[:, 0]
        assert b[2] == (a[3] - a[1]) / 2.0 * 1.0 + a[1]


def test_would_merge_clips_stay_unmerged():
    for name in ("would_merge_same_team", "would_merge_unknown_team"):
        t = table_of(name, False)
        assert {"Player_3", "Player_3_video", "Player_4", "Player_4_video"} <= set(t["columns"])
        a, b = np.isnan(column(t, "Player_3_video")[:, 0]), np.isnan(column(t, "Player_4_video")[:, 0])
        assert not a[:5].any() and a[5:].all() and b[:9].all() and not b[9:].any()
        last, first = column(t, "Player_3_video")[4], column(t, "Player_4_video")[9]
        assert np.hypot(*(last - first)) <= 10 * 5 and 9 - 4 <= int(5 * 1.1)        # the intended rule (proc.py:268-276) would have merged them


def test_filter_ball_is_refused():
    with pytest.raises(NotImplementedError):
        post_ref.process_data(post_cases.coords_of(post_cases.BY_NAME["ball_two_sightings"]), {}, filter_ball_detections=True)
    from eagle_amd import postprocess
    with pytest.raises(NotImplementedError):
        postprocess.process_data(None, post_cases.records_of(post_cases.BY_NAME["ball_two_sightings"]), 25, 1280, {}, filter_ball_detections=True)


def test_no_pandas_under_the_package():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eagle_amd")
    for fn in os.listdir(root):
        if fn.endswith(".py"):
            assert "import pandas" not in open(os.path.join(root, fn)).read(), fn
