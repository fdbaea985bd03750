"""The constructed team-colour cases of tests/team_color_cases.py are themselves checked (no GPU):
(1) every case forces what its ``why`` says, asserted from the intermediate values of the restatement (``replay``), not assumed;
(2) no crop of a case that is not marked ``tied`` has an exact distance tie on its Lloyd path, and on all of them with two or more pixels
    scikit-learn's own KMeans(n_clusters=2, random_state=0) gives the labels of oracle/colors.py::kmeans2_labels; on every crop of the tied case the
    two differ (if a later scikit-learn makes them agree this fails, and the case is searched anew);
(3) colors.detect_color equals a second, direct statement of proc.py:466-503 written here;
(4) the host mapping scenarios take the branches they are built for, on the CPU oracle."""
import warnings

import numpy as np
import pytest

import team_color_cases as T
from oracle import colors
from oracle import prims as P


def _sk_labels(rgb):
    from sklearn.cluster import KMeans
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                # ConvergenceWarning: fewer distinct points than clusters (flat crops)
        return KMeans(n_clusters=2, random_state=0).fit(rgb).labels_


@pytest.fixture(scope="module")
def replays():
    return {name: {k: T.replay(T.crop_rgb(c, crop)) for k, crop in T.valid_crops(c)} for name, c in T.CASES.items()}


def test_case_table(replays):
    """per crop: pixels, stop rule, iterations, ties_on_path (printed with -s); the replay in exact integers gives the restatement's labels"""
    for name, c in T.CASES.items():
        assert set(c) >= {"name", "frame_hw", "frames", "crops", "why"} and c["frames"].dtype == np.uint8 and c["frames"].shape[1:] == (*c["frame_hw"], 3)
        for k, crop in T.valid_crops(c):
            r = replays[name][k]
            print(f"{name}[{k}] {c.get('labels', {k: ''})[k] if 'labels' in c else ''}: {r['n']} pixels, {r['rule']}, {r['iters']} iterations, ties_on_path {r['tied']}")
            assert not r["fragile"]
            if not r["tied"]:
                assert np.array_equal(r["labels"], colors.kmeans2_labels(T.crop_rgb(c, crop))), (name, k)
            assert T.stop_rule(T.crop_rgb(c, crop)) == (r["rule"], r["iters"]) and T.ties_on_path(T.crop_rgb(c, crop)) == r["tied"]


def test_only_the_tied_case_has_ties_and_sklearn_agrees_everywhere_else(replays):
    skipped, compared = [], 0
    for name, c in T.CASES.items():
        for k, crop in T.valid_crops(c):
            rgb = T.crop_rgb(c, crop)
            if c.get("tied"):
                assert replays[name][k]["tied"], (name, k)
                assert not np.array_equal(_sk_labels(rgb), colors.kmeans2_labels(rgb)), ("scikit-learn now agrees on this tied crop: search the tied cases anew", k)
                continue
            assert not replays[name][k]["tied"], (name, k)
            if len(rgb) < 2:                            # scikit-learn refuses n_samples < n_clusters
                skipped.append((name, k))
                continue
            assert np.array_equal(_sk_labels(rgb), colors.kmeans2_labels(rgb)), (name, k)
            compared += 1
    one_pixel = [(name, k) for name, c in T.CASES.items() for k, (f, x1, y1, x2, y2) in T.valid_crops(c) if (x2 - x1, y2 - y1) == (1, 1)]
    assert skipped == one_pixel == [("tiny", 0)] and compared >= 80
    assert len(T.CASES["tied"]["crops"]) >= 5


def test_tie_search_counts():
    """the seeded search behind the tied case: scikit-learn equals the restatement on EVERY tie-free input, and differs on some tied ones (the
    counts printed here are the ones quoted in teams.hip, oracle/colors.py and include/eagle.h)"""
    tied = differ = free = 0
    found = []
    for s in range(T.TIE_SEARCH):
        rgb = T.few_levels(s)[..., ::-1].reshape(-1, 3)
        same = np.array_equal(_sk_labels(rgb), colors.kmeans2_labels(rgb))
        if T.ties_on_path(rgb):
            tied += 1
            if not same:
                differ += 1; found.append(s)
        else:
            free += 1
            assert same, ("a tie-free input on which scikit-learn differs", s)
    print(f"{T.TIE_SEARCH} few-level inputs: {tied} with a tie on the path, of which {differ} differ from scikit-learn; {free} tie-free, all identical")
    assert tied + free == T.TIE_SEARCH and free > 200 and set(T.TIED_SEEDS) <= set(found)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------
def _hw(crop):
    return crop[4] - crop[2], crop[3] - crop[1]


def test_sizes(replays):
    C = T.CASES
    assert [_hw(c) for c in C["tiny"]["crops"]] == T.TINY == [(1, 1), (1, 2), (2, 1), (2, 2), (1, 7), (3, 5)]
    assert all(h * w < T.THREADS for h, w in T.TINY)
    assert replays["tiny"][1]["n"] == 2 and replays["tiny"][1]["i0"] == 1 and replays["tiny"][2]["i0"] == 1          # floor(U0 * 2): centre 0 is the last pixel
    want = [255, 256, 257, 511, 512, 513, 767, 768, 769]
    assert [_hw(c) for c in C["chunk_rows"]["crops"]] == [(1, n) for n in want]
    assert [h * w for h, w in map(_hw, C["chunk_blocks"]["crops"])] == [n for n in want if n not in (257, 769)] and all(min(_hw(c)) > 1 for c in C["chunk_blocks"]["crops"])
    assert all(any(n % d == 0 for d in range(2, n)) is False for n in (257, 769))                                    # prime: no near-square crop exists
    assert [T.chunk_of(n) for n in want] == [1, 1, 2, 2, 2, 3, 3, 3, 4]
    assert [-(-n // T.chunk_of(n)) for n in want] == [255, 256, 129, 256, 256, 171, 256, 256, 193]                  # threads that own a pixel; the last may own fewer
    assert [_hw(c) for c in C["thin"]["crops"]] == [(61, 1), (1, 97)]
    (big,) = C["large"]["crops"]
    assert _hw(big) == T.LARGE_HW and T.LARGE_HW[0] * T.LARGE_HW[1] == 60000
    over = [(name, k) for name, c in C.items() for k, crop in T.valid_crops(c) if _hw(crop)[0] * _hw(crop)[1] > 5000]
    assert over == [("large", 0)]
    row = T.expected("large")[0]
    assert 0 < row[11] < 60000 and row[:11].sum() > 0


# ---- seeding -------------------------------------------------------------------------------------------------------------------------------------
def test_seeding(replays):
    case, R = T.CASES["seeding"], replays["seeding"]
    lab = {n: k for k, n in enumerate(case["labels"])}
    n, chunk = 900, T.chunk_of(900)
    assert chunk == 4 and (n - 1) // chunk == 224
    for name in ("first_of_chunk", "last_of_chunk", "last_chunk", "cand0_wins", "cand1_wins", "equal_pots"):
        r = R[lab[name]]
        assert r["n"] == n and r["pot"] > 0 and r["cands"][0] != r["cands"][1]
        for u, cand in zip((T.U1, T.U2), r["cands"]):     # the candidate is the first index whose cumulative distance reaches u * pot
            assert r["cum"][cand] >= u * r["pot"] and (cand == 0 or r["cum"][cand - 1] < u * r["pot"])
            assert r["cum"][cand] != u * r["pot"]         # never equal: side = left and side = right agree wherever pot > 0
    assert all(c % chunk == 0 for c in R[lab["first_of_chunk"]]["cands"])
    assert all(c % chunk == chunk - 1 for c in R[lab["last_of_chunk"]]["cands"])
    assert all(c // chunk == 224 for c in R[lab["last_chunk"]]["cands"]) and R[lab["last_chunk"]]["cands"][0] == n - 1
    p = R[lab["cand0_wins"]]["pots"]; assert p[0] < p[1] and R[lab["cand0_wins"]]["winner"] == 0
    p = R[lab["cand1_wins"]]["pots"]; assert p[1] < p[0] and R[lab["cand1_wins"]]["winner"] == 1
    r = R[lab["equal_pots"]]
    rgb = T.crop_rgb(case, case["crops"][lab["equal_pots"]])
    assert r["pots"][0] == r["pots"][1] > 0 and r["winner"] == 0 and tuple(rgb[r["cands"][0]]) == T.RED and tuple(rgb[r["cands"][1]]) == T.GREEN
    # ... and the loser would have given another answer: the row counts the five red pixels, not the five green ones
    assert T.expected("seeding")[lab["equal_pots"]].tolist() == [5] + [0] * 10 + [5]
    # the winning candidate of each 900-pixel case has neighbours of the background colour: a search that is off by one pixel changes the row
    for name in ("first_of_chunk", "last_of_chunk", "cand0_wins", "cand1_wins"):
        r = R[lab[name]]
        w = r["cands"][r["winner"]]
        x = T.crop_rgb(case, case["crops"][lab[name]])
        assert tuple(x[w - 1]) == tuple(x[w + 1]) == T.DARK != tuple(x[w])
    # side = left: the one crop where the cumulative distance EQUALS u1 * pot at the candidate; side = right would skip the background that follows,
    # take the grey pixel behind it, and give another row
    k = lab["side_left"]
    r, x = R[k], T.crop_rgb(case, case["crops"][k])
    j = r["cands"][0]
    assert r["pot"] == T.SIDE_POT and r["vals"][0] == float(int(r["vals"][0])) == r["cum"][j] and r["cum"][j - 1] < r["vals"][0] and r["n"] <= 5000
    assert tuple(x[j]) == T.WHITE and all(tuple(x[j + 1 + i]) == T.BLACK for i in range(T.SIDE_PLATEAU)) and tuple(x[j + 1 + T.SIDE_PLATEAU]) == T.GREY
    wrong = T.replay(x, side="right")
    assert wrong["cands"] == [j + 1 + T.SIDE_PLATEAU, r["cands"][1]] and wrong["winner"] == 0 and r["winner"] == 0
    assert T.oracle_row(T.crop_bgr(case, case["crops"][k]), wrong["labels"]) != T.expected("seeding")[k].tolist()
    for other in range(len(case["crops"])):               # ... and nowhere else can the side matter
        if other != k:
            assert all(R[other]["pot"] == 0 or R[other]["cum"][c] != v for c, v in zip(R[other]["cands"], R[other]["vals"]))
    flat = R[lab["flat"]]
    assert flat["pot"] == 0 and flat["cands"] == [0, 0] and not flat["labels"].any() and not T.expected("seeding")[lab["flat"]].any()
    i0 = R[lab["odd_at_seed"]]["i0"]
    assert i0 == 34 and R[lab["odd_before_seed"]]["cands"] == [5, 5] and R[lab["odd_after_seed"]]["cands"] == [50, 50] and R[lab["odd_after_seed_900"]]["cands"] == [899, 899]
    for name, odd in (("odd_before_seed", 5), ("odd_at_seed", 34), ("odd_after_seed", 50), ("odd_after_seed_900", 899)):
        x = T.crop_rgb(case, case["crops"][lab[name]])
        assert [i for i in range(len(x)) if tuple(x[i]) != T.DARK] == [odd]
        assert T.expected("seeding")[lab[name]].tolist() == [1] + [0] * 10 + [1]


# ---- Lloyd ---------------------------------------------------------------------------------------------------------------------------------------
def test_lloyd_stop_rules(replays):
    got = [(replays["lloyd"][k]["rule"], replays["lloyd"][k]["iters"]) for k in range(len(T.LLOYD))]
    assert got == [want for _, want in T.LLOYD]
    for rule in ("repeat", "tol"):
        its = [i for r, i in got if r == rule]
        assert max(its) >= 8 and len(its) >= 2
    assert all(r["n"] <= 2000 for r in replays["lloyd"].values())
    rules = {(r["rule"]) for per in replays.values() for r in per.values()}
    assert rules == {"repeat", "tol"}                  # no case reaches the 300-iteration cap (team_color_cases' docstring)
    assert any(r["rule"] == "tol" and r["iters"] <= 2 for per in replays.values() for r in per.values())
    assert any(r["rule"] == "repeat" and r["iters"] <= 2 for per in replays.values() for r in per.values())


# ---- corner vote ---------------------------------------------------------------------------------------------------------------------------------
def test_corner_votes(replays):
    case = T.CASES["corner_vote"]
    rows = T.expected("corner_vote")
    want = {"4-0 label 0": ([0, 0, 0, 0], 0), "4-0 label 1": ([1, 1, 1, 1], 1), "3-1 label 0": ([0, 0, 1, 0], 0), "3-1 label 1": ([1, 0, 1, 1], 1), "2-2": ([0, 1, 1, 0], 0)}
    pictures = []
    for k, name in enumerate(case["labels"]):
        h, w = _hw(case["crops"][k])
        lab = replays["corner_vote"][k]["labels"].reshape(h, w)
        corners = [int(lab[0, 0]), int(lab[0, -1]), int(lab[-1, 0]), int(lab[-1, -1])]
        assert corners == want[name][0], name
        background = want[name][1]
        assert rows[k, 11] == int((lab != background).sum()) and 0 < rows[k, 11] < h * w
        inner = T.crop_bgr(case, case["crops"][k]).copy()
        for y, x in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            inner[y, x] = 0
        pictures.append(inner)
    assert all(np.array_equal(pictures[0], p) for p in pictures)                  # the same picture but for the corner pixels
    # label 0 is the background population (centre 0 lies on it): where label 1 wins the vote the player cluster is label 0, the larger one
    assert rows[1, 11] > 300 and rows[3, 11] > 300 and rows[0, 11] < 110 and rows[2, 11] < 110 and rows[4, 11] < 110
    assert rows[1, 3] == rows[1, 11] and rows[0, 0] == rows[0, 11]              # green grass against a red figure


# ---- colour ranges ---------------------------------------------------------------------------------------------------------------------------------
def _player_pixels():
    """BGR pixels of the player cluster of every valid crop of every case"""
    out = []
    for name, c in T.CASES.items():
        for k, crop in T.valid_crops(c):
            img = T.crop_bgr(c, crop)
            lab = colors.kmeans2_labels(img[..., ::-1].reshape(-1, 3)).reshape(img.shape[:2])
            corners = [lab[0, 0], lab[0, -1], lab[-1, 0], lab[-1, -1]]
            bg = max(set(corners), key=corners.count)
            out.append(img[lab != bg])
    return np.concatenate(out)


def test_colour_ranges_are_hit_on_both_sides_of_every_bound():
    bgr = _player_pixels()
    hsv = P.bgr2hsv(bgr.reshape(-1, 1, 3)).reshape(-1, 3).astype(int)
    h, s, v = hsv.T
    for color, (lo, hi) in colors.COLOR_RANGES.items():            # red2 separately
        inside = np.all((hsv >= lo) & (hsv <= hi), axis=1)
        assert inside.any(), color
    coloured = (s >= 100) & (v >= 100)
    for x in T.HUES:
        assert (coloured & (h == x)).any(), ("hue", x)
    for x in (29, 30, 31):
        assert ((s == x) & (v >= 200)).any() and ((s == x) & (v >= 50) & (v <= 200)).any(), ("saturation", x)
    for x in (99, 100, 101):
        assert ((s == x) & (v >= 100)).any(), ("saturation", x)
        assert ((v == x) & (s >= 100)).any(), ("value", x)
    for x in (49, 50, 51):
        assert ((v == x) & (s <= 30)).any() and ((v == x) & (s > 30)).any(), ("value", x)
    for x in (199, 200, 201):
        assert ((v == x) & (s <= 30)).any(), ("value", x)
    assert set(T.HUES) | set(T.SATS) | set(T.VALS) == set(T.HUES + [29, 30, 31, 99, 100, 101, 49, 50, 51, 199, 200, 201])
    b, g, r = bgr.T.astype(int)
    mx = bgr.max(1)
    assert ((b == g) & (g == r)).any()                                                             # diff == 0
    for p, q, o in ((r, g, b), (g, b, r), (r, b, g)):
        assert ((p == q) & (p == mx) & (o < mx)).any()                                             # two channels tie for the maximum
    neg = T.hue_before_wrap(bgr) < 0
    assert neg.any() and ((h[neg] >= 150) | (h[neg] == 0)).all() and (coloured & neg & (h >= 160)).any()            # negative before the + 180


def test_detect_color_against_a_direct_statement():
    """proc.py:466-503 once more: labels, the corner vote by max(set(c), key=c.count), the inclusive range comparisons on bgr2hsv, red2 added to
    red, the list sorted by count (stable) — independent of colors.color_counts / colors.detect_color / team_color_cases.oracle_row"""
    for name, c in T.CASES.items():
        rows = T.expected(name)
        for k, crop in T.valid_crops(c):
            img = T.crop_bgr(c, crop)
            hh, ww = img.shape[:2]
            lab = [int(v) for v in colors.kmeans2_labels(img[..., ::-1].reshape(-1, 3))]
            cn = [lab[0], lab[ww - 1], lab[(hh - 1) * ww], lab[hh * ww - 1]]
            background = max(set(cn), key=cn.count)
            hsv = P.bgr2hsv(np.ascontiguousarray(img)).reshape(-1, 3)
            cnt = dict.fromkeys(colors.COLOR_RANGES, 0)
            players = 0
            for i, (h, s, v) in enumerate(hsv.tolist()):
                if lab[i] == background:
                    continue
                players += 1
                for color, ((h0, s0, v0), (h1, s1, v1)) in colors.COLOR_RANGES.items():
                    if h0 <= h <= h1 and s0 <= s <= s1 and v0 <= v <= v1:
                        cnt[color] += 1
            cnt["red"] += cnt.pop("red2")
            want = sorted([(c_, n) for c_, n in cnt.items() if n > 0], key=lambda x: x[1], reverse=True)
            assert colors.detect_color(img) == want, (name, k)
            assert rows[k].tolist() == [cnt[c_] for c_ in colors.COLOR_ORDER] + [players], (name, k)
        for k in c.get("refused", ()):
            assert not rows[k].any()


# ---- placement, refused crops ----------------------------------------------------------------------------------------------------------------------
def test_placement_and_refused_rectangles():
    c = T.CASES["placement"]
    fh, fw = c["frame_hw"]
    last = len(c["frames"]) - 1
    cr = c["crops"]
    assert any(x[1:3] == (0, 0) for x in cr) and any(x[3] == fw and x[4] < fh for x in cr) and any(x[4] == fh and x[3] < fw for x in cr)
    assert any(x[0] == last and x[3] == fw and x[4] == fh for x in cr)
    o = T.CASES["odd_frame"]
    oh, ow = o["frame_hw"]
    assert (oh, ow) == (33, 47) and (ow * 3) % 4 and any(x == (1, 0, 0, ow, oh) for x in o["crops"]) and any(x[0] == 1 and x[3:] == (ow, oh) and x[1] > 0 for x in o["crops"])
    r = T.CASES["refused"]
    fh, fw = r["frame_hw"]
    n = len(r["frames"])

    def refused(f, x1, y1, x2, y2):                    # csrc/teams.hip: the row of such a crop is twelve zeros
        return x2 <= x1 or y2 <= y1 or f < 0 or f >= n or x1 < 0 or y1 < 0 or x2 > fw or y2 > fh

    assert [k for k, x in enumerate(r["crops"]) if refused(*x)] == list(r["refused"])
    why = {r["labels"][k] for k in r["refused"]}
    assert why >= {"x2 <= x1", "y2 <= y1", "x1 < 0", "y1 < 0", "x2 > frame_w", "y2 > frame_h", "frame < 0", "frame >= n_frames"}
    valid = [k for k, _ in T.valid_crops(r)]
    assert all(any(k - 1 == j or k + 1 == j for j in valid) for k in r["refused"] if k < max(valid))      # refused crops sit between valid ones
    assert all(T.expected("refused")[k, 11] > 0 for k in valid)
    for name, case in T.CASES.items():                  # nothing but the refused crops leaves its frame
        H, W = case["frame_hw"]
        for k, (f, x1, y1, x2, y2) in T.valid_crops(case):
            assert 0 <= f < len(case["frames"]) and 0 <= x1 < x2 <= W and 0 <= y1 < y2 <= H, (name, k)


# ---- the host mapping ------------------------------------------------------------------------------------------------------------------------------
def _votes(m):
    """per player {colour: weighted votes} and the per-crop records (frame, player, overlap, colours), as proc.py:405-447 collects them"""
    votes, seen = {}, []
    for i, (frame, key) in enumerate(zip(m["frames"], m["coords"])):
        players = m["coords"][key]["Coordinates"]["Player"]
        boxes = [p["BBox"] for p in players.values()]
        for pid, it in players.items():
            x1, y1, x2, y2 = it["BBox"]
            if pid in m.get("skipped", ()) and (x2 - x1) * (y2 - y1) <= 0:
                continue
            prop = colors.overlap_weight(it["BBox"], boxes)
            if prop > 0.35:
                seen.append((i, pid, prop, None))
                continue
            crop = frame[y1:y2, x1:x2]
            assert not T.ties_on_path(crop[..., ::-1].reshape(-1, 3)), (m["name"], i, pid)
            found = [c for c, _ in colors.detect_color(crop)]
            seen.append((i, pid, prop, found))
            for c in found:
                votes.setdefault(pid, {}); votes[pid][c] = votes[pid].get(c, 0) + 1 - prop
    return votes, seen


def test_mapping_scenarios_take_their_branches():
    m = T.MAPPINGS["two_teams"]
    votes, seen = _votes(m)
    props = {(i, pid): prop for i, pid, prop, _ in seen}
    assert props[(0, 3)] == props[(0, 4)] == 418 / T.BIG < 0.35 < 425 / T.BIG == props[(1, 6)] == props[(1, 8)]
    assert [(i, pid) for i, pid, _, found in seen if found is None] == [(1, 6), (1, 8)]
    assert votes[4] == {"red": 1 - 418 / T.BIG, "blue": 1.0} and list(votes[4]) == ["red", "blue"]      # unweighted: a 1-1 draw that red, seen first, would win
    assert votes[7] == {"yellow": 2.0, "red": 1.0}
    assert len(m["coords"]) == 5 > m["n_frames"] == len(m["frames"]) == 4 and not m["coords"][2]["Coordinates"]["Player"]
    assert sum(1 for i, pid, _, _ in seen if pid == 1) == 2 and 99 in m["coords"][4]["Coordinates"]["Player"]
    got = colors.get_team_mapping(list(m["frames"]), m["coords"])
    assert got == {1: 1, 2: 1, 3: 1, 7: 1, 4: 0, 6: 0, 8: 0, 11: 0, 12: 0}
    one = T.MAPPINGS["one_team"]
    assert colors.get_team_mapping(list(one["frames"]), one["coords"]) == {1: 0, 2: 0, 3: 0}


@pytest.mark.parametrize("name", ["zero_area", "no_colour"])
def test_where_the_reference_raises(name):
    """the two deviations of eagle_amd/teams.py: the reference raises, the library skips (test_gpu_teams.py states what it gives instead)"""
    m = T.MAPPINGS[name]
    with pytest.raises(m["raises"]):
        colors.get_team_mapping(list(m["frames"]), m["coords"])
    assert colors.get_team_mapping(list(m["frames"]), T.without(m["coords"], m["skipped"])) == {1: 0, 2: 1, 5: 0}
    if name == "no_colour":
        votes, seen = _votes(m)
        assert [found for _, pid, _, found in seen if pid == 3] == [[]]
