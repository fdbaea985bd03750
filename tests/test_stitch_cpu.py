"""The contract of the post-processor's id merge (tests/stitch_ref.py) on the constructed clips of tests/stitch_cases.py, without a GPU: every case
forces the edge it is named after (the link list is asserted, not only the table); with the switch off the contract is tests/post_ref.py bit for
bit; the invariants of the rule on randomly fragmented clips; and the strong check: a fragmented clip, stitched, is bit-equal to the same clip under
its original ids."""
import numpy as np
import pytest

import post_cases
import post_ref
import stitch_cases
import stitch_ref


def run(case, smooth=False, merge_ids=True, recs=None):
    return stitch_ref.process_data(post_cases.coords_of(case, recs), case["team_mapping"], smooth=smooth, fps=case["fps"], merge_ids=merge_ids)


def same_tables(a, b):
    assert a["rows"] == b["rows"] and a["columns"] == b["columns"] and a["flags"] == b["flags"]
    assert a["values"].shape == b["values"].shape and np.array_equal(np.isnan(a["values"]), np.isnan(b["values"]))
    ok = ~np.isnan(a["values"])
    assert np.array_equal(a["values"].view(np.uint64)[ok], b["values"].view(np.uint64)[ok])


def heads_of(table):
    return [int(n.split("_")[1]) for n in table["columns"] if n.endswith("_video") and n.split("_")[0] in ("Player", "Goalkeeper")]


@pytest.mark.parametrize("name", [c["name"] for c in stitch_cases.CASES])
def test_case_forces_its_edge(name):
    case = stitch_cases.BY_NAME[name]
    t = run(case)
    assert [(m["from_id"], m["to_id"]) for m in t["merges"]] == case["links"]
    assert heads_of(t) == case["heads"] and t["team_mapping"] == case["teams"]
    off = run(case, merge_ids=False)
    assert len(heads_of(off)) == len(case["heads"]) + len(case["links"]) and off["merges"] == []
    for m in t["merges"]:
        assert m["gap_frames"] <= int(case["fps"] * 1.1) and m["dist"] <= 10.0 * m["gap_frames"]


def test_the_order_of_the_key_matters():
    """Each part of the key (d, g, column of a, column of b) decides one constructed case: the case comes out otherwise under a key without it."""
    pos = lambda tr, l, k: tr[l[k]]["pos"]                # noqa: E731
    mutants = {"tie_on_distance_by_gap": lambda tr: lambda l: (l[0], pos(tr, l, 2), pos(tr, l, 3)),                 # g dropped
               "distance_before_gap": lambda tr: lambda l: (l[1], l[0], pos(tr, l, 2), pos(tr, l, 3)),              # g in front of d
               "tie_on_both_crossed": lambda tr: lambda l: (l[0], l[1]),                                            # no column tie-break (stable sort)
               "tie_on_both_by_column": lambda tr: lambda l: (l[0], l[1], tr[l[2]]["id"], tr[l[3]]["id"])}          # ids for columns
    for name, key in mutants.items():
        case = stitch_cases.BY_NAME[name]
        coords = post_cases.coords_of(case)
        assert stitch_ref.accepted_ids(coords, case["team_mapping"], case["fps"]) == case["links"]
        assert stitch_ref.accepted_ids(coords, case["team_mapping"], case["fps"], key) != case["links"], name


def _col(t, name):
    return t["values"][t["columns"].index(name)]


def test_hand_over_interpolates_the_gap():
    t = run(stitch_cases.BY_NAME["hand_over"])
    v = _col(t, "Player_5_video")
    assert "Player_9_video" not in t["columns"] and "Player_9" not in t["columns"] and not np.isnan(v).any()
    assert v[9].tolist() == [118.0, 400.0] and v[12].tolist() == [126.0, 402.0]
    assert v[10].tolist() == [(126.0 - 118.0) / 3.0 * 1.0 + 118.0, (402.0 - 400.0) / 3.0 * 1.0 + 400.0]
    assert t["merges"] == [{"kind": 0, "from_id": 5, "to_id": 9, "head_id": 5, "gap_frames": 3, "team": -1, "dist": float(np.sqrt(np.float64(68.0)))}]


def test_thresholds_are_met_exactly():
    for name, g, d in (("temporal_fps25_gap27", 27, 0.0), ("temporal_fps24_gap26", 26, 0.0), ("temporal_fps30_gap33", 33, 0.0), ("distance_g3_at", 3, 30.0),
                       ("distance_g1_at", 1, 10.0), ("distance_g2_half", 2, 20.0), ("frame_gap_within", 5, 40.0)):
        (m,) = run(stitch_cases.BY_NAME[name])["merges"]
        assert (m["gap_frames"], m["dist"]) == (g, d)
    t = run(stitch_cases.BY_NAME["frame_gap_over"])                   # the rows are neighbours, the frames are not
    assert t["rows"] == [0, 1, 2, 9, 10, 11] and t["merges"] == []


def test_report_carries_the_finished_chain():
    t = run(stitch_cases.BY_NAME["goalkeeper_chain_with_fold"])
    assert [(m["kind"], m["from_id"], m["to_id"], m["head_id"]) for m in t["merges"]] == [(1, 7, 8, 6), (1, 6, 7, 6)]
    assert "Goalkeeper_6_video" in t["columns"] and not any(n.startswith(("Player_7", "Goalkeeper_7", "Goalkeeper_8")) for n in t["columns"])
    assert _col(t, "Goalkeeper_6_video")[6].tolist() == [312.0, 400.0]                    # the Player cell wins the shared row inside the member
    t = run(stitch_cases.BY_NAME["teams_chain_second_link_wins"])
    assert [(m["head_id"], m["team"]) for m in t["merges"]] == [(7, 1)]
    t = run(stitch_cases.BY_NAME["chain_100"])
    assert len(t["columns"]) == 8 and len(t["rows"]) == 100 and len(t["merges"]) == 99 and {m["head_id"] for m in t["merges"]} == {200}


def test_pitch_over_the_chain():
    t = run(stitch_cases.BY_NAME["pitch_missing_at_ends"])
    pit, off = _col(t, "Player_5"), run(stitch_cases.BY_NAME["pitch_missing_at_ends"], merge_ids=False)
    assert not np.isnan(pit).any() and np.isnan(_col(off, "Player_5")[5:]).all() and np.isnan(_col(off, "Player_9")[:10]).all()
    a, z = pit[4], pit[10]                                            # the cells on either side of the missing run 5 .. 9
    assert pit[7].tolist() == [(z[k] - a[k]) / 6.0 * 3.0 + a[k] for k in (0, 1)]
    t = run(stitch_cases.BY_NAME["pitch_column_from_member"])         # Player_5 has no pitch column of its own: the chain's sits in front of its video column
    off = run(stitch_cases.BY_NAME["pitch_column_from_member"], merge_ids=False)
    assert "Player_5" not in off["columns"] and t["columns"].index("Player_5") + 1 == t["columns"].index("Player_5_video")
    assert np.isnan(_col(t, "Player_5")[:8]).all() and not np.isnan(_col(t, "Player_5")[8:]).any()


@pytest.mark.parametrize("smooth", [False, True])
def test_switch_off_is_post_ref(smooth):
    for case in post_cases.CASES + stitch_cases.CASES[:12]:
        exp = post_ref.process_data(post_cases.coords_of(case), case["team_mapping"], smooth=smooth)
        got = run(case, smooth=smooth, merge_ids=False)
        same_tables(got, exp)
        assert got["team_mapping"] == exp["team_mapping"] and got["merges"] == [] and set(got) == set(exp) | {"merges"}


def test_would_merge_clips_merge_with_the_switch():
    for name, teams in (("would_merge_same_team", {3: 0, 4: 0, 8: 1}), ("would_merge_unknown_team", {8: 1})):
        t = run(post_cases.BY_NAME[name])
        assert [(m["from_id"], m["to_id"], m["gap_frames"]) for m in t["merges"]] == [(3, 4, 5)] and heads_of(t) == [8, 3] and t["team_mapping"] == teams


@pytest.fixture(scope="module", params=stitch_cases.FRAGMENTED, ids=lambda p: "x".join(map(str, p[1:])))
def fragmented(request):
    case, restored, head_of = stitch_cases.fragmented(*request.param)
    return case, restored, head_of, request.param


def test_fragmented_invariants(fragmented):
    case, _, head_of, (seed, rows, players, fragments) = fragmented
    coords = post_cases.coords_of(case)
    kept, table, _ = post_ref.create_dataframe(coords)
    table = post_ref.merge_data(table)
    tracks = stitch_ref.tracks_of(table, case["team_mapping"])
    assert len(kept) == rows and len(tracks) == players * fragments + 1
    accepted, succ, pred, head, team = stitch_ref.select_links(tracks, kept, case["fps"])
    assert len(accepted) == players * (fragments - 1)
    for d, g, a, b in accepted:                                       # the four conditions
        A, B = tracks[a], tracks[b]
        assert A["kind"] == B["kind"] and A["last"] < B["first"] and g == kept[B["first"]] - kept[A["last"]] <= int(case["fps"] * 1.1)
        dx, dy = B["p_first"] - A["p_last"]
        assert d == float(np.sqrt(dx * dx + dy * dy)) and d <= 10.0 * g
        assert not (A["team"] >= 0 and B["team"] >= 0 and A["team"] != B["team"])
        assert head_of[A["id"]] == head_of[B["id"]] == tracks[head[a]]["id"]
    assert len({a for _, _, a, _ in accepted}) == len(accepted) == len({b for _, _, _, b in accepted})      # one successor, one predecessor
    present = {}
    for i, T in enumerate(tracks):                                    # no chain has two members in one row
        ok = post_ref._present(table[T["name"]])
        present[head[i]] = present.get(head[i], 0) + ok.astype(int)
    assert all(v.max() == 1 for v in present.values())


@pytest.mark.parametrize("smooth", [False, True])
def test_fragmented_equals_the_clip_under_its_original_ids(fragmented, smooth):
    case, restored, head_of, _ = fragmented
    got = run(case, smooth=smooth)
    exp = post_ref.process_data(post_cases.coords_of(restored), restored["team_mapping"], smooth=smooth)
    same_tables({k: got[k] for k in ("rows", "columns", "values", "flags")}, exp)
    for pid, team in case["team_mapping"].items():                    # every head carries its trajectory's team when any fragment had one
        assert got["team_mapping"][head_of[pid]] == team
