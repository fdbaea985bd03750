"""The constructed optical-flow cases (tests/lk_cases.py) force what they are named after, shown with the references alone (no GPU):
tests/lk_ref.py (written from OpenCV's definitions) against oracle/eo_flow.c + oracle/flow.py bit for bit, and lk_ref's trace for the
branches and magnitudes the HIP kernels must get through.  Every assertion here is a condition on the case list."""
import os
import re

import numpy as np
import pytest

import lk_cases
import lk_ref
from lk_cases import CASES, SHIFTS, expected, key_points
from oracle import flow
from oracle import prims as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(CASES)
TEXTURED = [n for n in NAMES if n in SHIFTS]


def test_case_list_covers_the_sizes_and_point_counts():
    assert {CASES[n][0].shape[1:3] for n in NAMES} == set(lk_cases.SIZES)
    assert {len(CASES[n][3]) for n in NAMES} >= {0, 1, 4, 57}
    assert any(CASES[n][0].shape[0] == 3 and CASES[n][0].size // 3 % 4 == 1 for n in NAMES)
    for n in NAMES:                                            # the three frames of the odd clip differ: a wrong frame offset cannot hide
        f = CASES[n][0]
        if f.shape[0] == 3:
            assert not np.array_equal(f[0], f[1]) and not np.array_equal(f[1], f[2]) and not np.array_equal(f[0], f[2])
        pts = CASES[n][3]
        assert all(isinstance(x, int) and isinstance(y, int) for x, y in pts) and len(pts) <= 57
    big = CASES["translate_243x321_0"][3]
    assert len(set(big)) < len(big), "duplicates"
    h, w = 243, 321
    assert {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)} <= set(big)
    assert {x for x, _ in big} >= set(lk_cases.boundary_values(w)) and {y for _, y in big} >= set(lk_cases.boundary_values(h))
    assert any(abs(x) > 10 * w or abs(y) > 10 * h for x, y in big), "far outside"


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_oracle_bit_for_bit(name):
    frames, src, dst, pts = CASES[name]
    for f in frames:
        g = lk_ref.gray(f)
        assert np.array_equal(g, P.bgr2gray(f))
        g1 = lk_ref.pyrdown(g)
        assert np.array_equal(g1, P.pyrdown(g)) and np.array_equal(lk_ref.pyrdown(g1), P.pyrdown(P.pyrdown(g)))
    got, nxt, st, _ = expected(name)
    kps = dict(key_points(pts))
    gs, gd = P.bgr2gray(frames[src]), P.bgr2gray(frames[dst])
    if pts:
        enxt, est = P.calc_optical_flow_pyr_lk(gs, gd, np.array(pts, np.float32))
        assert np.array_equal(st, est[:, 0]), np.nonzero(st != est[:, 0])
        assert np.array_equal(nxt.view(np.uint32), enxt.view(np.uint32)), np.nonzero((nxt.view(np.uint32) != enxt.view(np.uint32)).any(1))
    exp = flow.calculate_optical_flow(frames[dst], gs, kps, gd)
    assert got == [(k, (int(v[0]), int(v[1]))) for k, v in exp.items()]


def test_pyramid_depth():
    assert [lk_ref.levels(s, s) for s in (32, 60, 61)] == [1, 1, 2]
    assert lk_ref.level_sizes(61, 61) == [(61, 61), (31, 31), (16, 16)] and lk_ref.level_sizes(60, 60) == [(60, 60), (30, 30)]
    assert lk_ref.levels(64, 61) == 2 and lk_ref.levels(33, 95) == 1 and lk_ref.levels(243, 321) == 2 and lk_ref.levels(720, 1280) == 2
    for n in NAMES:                                            # the trace has exactly the levels in use
        h, w = CASES[n][0].shape[1:3]
        for tr in expected(n)[3]:
            assert sorted(tr) == list(range(lk_ref.levels(h, w) + 1))


@pytest.mark.parametrize("hw", lk_cases.SIZES)
def test_pyrdown_matches_float_gaussian(hw):
    h, w = hw
    g = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w), dtype=np.uint8)
    d = lk_ref.pyrdown(g)
    assert d.shape == ((h + 1) // 2, (w + 1) // 2)
    k = np.array([1, 4, 6, 4, 1], float) / 16
    pad = np.pad(g.astype(float), 2, mode="reflect")
    full = sum(k[a] * k[b] * pad[a:a + h, b:b + w] for a in range(5) for b in range(5))
    assert np.abs(d - full[::2, ::2]).max() <= 0.5 + 1e-9


def test_gray_known_answers():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [10, 200, 100], [128, 128, 128], [1, 2, 3]]], np.uint8)
    assert lk_ref.gray(px).tolist() == [[29, 150, 76, 255, 0, 148, 128, 2]]
    assert [lk_ref.hue180(*p) for p in px[0][:5]] == [120, 60, 0, 0, 0]


@pytest.mark.parametrize("name", TEXTURED)
def test_translation_is_recovered(name):
    frames, src, dst, pts = CASES[name]
    h, w = frames.shape[1:3]
    _, nxt, st, _ = expected(name)
    inner = [k for k, p in enumerate(pts) if lk_cases.is_interior(p, h, w)]
    if min(h, w) > 24:
        assert len(inner) >= 10
    prev = np.array(pts, np.float32)
    if SHIFTS[name] == (0.0, 0.0):
        assert src == dst and st[inner].all() and np.array_equal(nxt[st == 1], prev[st == 1])      # identical frames: next == prev exactly
        return
    assert st[inner].all(), [pts[k] for k in inner if not st[k]]
    err = np.abs((nxt[inner] - prev[inner]) - np.array(SHIFTS[name]))
    assert err.max() < 0.1, (err.max(), SHIFTS[name])


def test_interior_points_of_the_textured_cases_mostly_keep_their_status():
    total = kept = 0
    for name in TEXTURED:
        frames, _, _, pts = CASES[name]
        h, w = frames.shape[1:3]
        st = expected(name)[2]
        inner = [k for k, p in enumerate(pts) if lk_cases.is_interior(p, h, w)]
        total += len(inner); kept += int(st[inner].sum())
    assert total > 300 and kept * 2 >= total


def _uncached(tr):
    """Iterations of one point whose J window lies more than 8 pixels (in x or in y) from the window the level started with: the kernel's global-load branch."""
    n = 0
    for lv in tr.values():
        if lv["iters"]:
            x0, y0 = lv["iters"][0]["origin"]
            n += sum(abs(it["origin"][0] - x0) > 8 or abs(it["origin"][1] - y0) > 8 for it in lv["iters"])
    return n


def test_windows_leave_the_cached_neighbourhood():
    names = ["uncorrelated_243x321", "far_shift_243x321", "odd3_33x95_uncorrelated", "odd3_33x95_backwards"]
    pts = sum(sum(_uncached(tr) > 0 for tr in expected(n)[3]) for n in names)
    its = sum(sum(_uncached(tr) for tr in expected(n)[3]) for n in names)
    print(f"uncached branch: {pts} points, {its} iterations")
    assert pts >= 5
    # ... and the small-shift cases never do: both branches of the kernel are exercised
    assert sum(_uncached(tr) for tr in expected("translate_243x321_0")[3]) == 0


def _partials(name, key):
    return [p for tr in expected(name)[3] for it in tr[0]["iters"] for p in it[key]]


@pytest.mark.parametrize("axis,key,reached", [("x", "part1", (1131955200, -1131955200)), ("y", "part2", (1082016000, -1044561600))])
def test_extreme_cases_reach_the_32_bit_range_of_a_wave_partial(axis, key, reached):
    pos, neg = _partials(f"extreme_pos_{axis}_60x60", key), _partials(f"extreme_neg_{axis}_60x60", key)
    print(f"largest 64-pixel partial ({key}): {max(pos)}, {min(neg)}")
    assert 2 ** 29 <= max(pos) < 2 ** 31 and 2 ** 29 <= -min(neg) < 2 ** 31
    assert (max(pos), min(neg)) == reached                           # the figures in lk_cases.extreme_pair's docstring
    for name in (f"extreme_pos_{axis}_60x60", f"extreme_neg_{axis}_60x60"):
        # reached at level 0, iteration 0, at integral positions: the upper levels reject every point, so level 0 starts at the point itself
        frames, _, _, pts = CASES[name]
        for p, tr in list(zip(pts, expected(name)[3]))[:25]:             # (the last four points lie at the frame's edge, where the reflection breaks the period)
            assert tr[1]["skipped"] == "minEig / determinant" and tr[0]["iters"][0]["origin"] == (p[0] - 7, p[1] - 7)
        first = [abs(v) for tr in expected(name)[3][:25] for v in tr[0]["iters"][0][key]]
        assert max(first) >= 2 ** 29
        assert all(abs(v) < 2 ** 31 for tr in expected(name)[3] for lv in tr.values() for it in lv["iters"] for k in ("part1", "part2") for v in it[k])


@pytest.mark.parametrize("name", ["flat_black_60x60", "flat_white_61x61", "edge_64x61"])
def test_flat_cases_track_nothing(name):
    got, _, st, tr = expected(name)
    assert not st.any() and got == []
    assert all(t[0]["skipped"] is not None for t in tr)


def test_status_boundaries_have_both_outcomes():
    """The window origin of an integer point is the point - 7, and the status survives for origins in [-15, size - 1] only: -9, size + 7 and size + 8 lose it
    to that rule whatever the picture shows.  -8 (no window pixel inside the frame) and -7 / size + 6 (only the frame's edge line, across which the reflected
    Scharr derivative is 0) pass that rule and always fail the determinant test: no picture gives them status 1.  -6 and size + 5 are the outermost points
    that can be tracked, and they are the ones that must show both outcomes.  Every coordinate is checked with the rule that decided it."""
    seen = {}
    for name in TEXTURED:
        frames, _, _, pts = CASES[name]
        h, w = frames.shape[1:3]
        _, _, st, trace = expected(name)
        for (x, y), s, tr in zip(pts, st, trace):
            for side, v, size, other, mid in (("x", x, w, y, h // 2), ("y", y, h, x, w // 2)):
                if other == mid and v in lk_cases.boundary_values(size):
                    seen.setdefault((side, v - size if v > 0 else v), set()).add((int(s), tr[0]["lost"]))
    for side in "xy":
        for v in (-9, 7, 8):
            assert seen[(side, v)] == {(0, "I window outside")}
        for v in (-8, -7, 6):
            assert seen[(side, v)] == {(0, "minEig / determinant")}
        for v in (-6, 5):
            assert {s for s, _ in seen[(side, v)]} == {0, 1}, seen[(side, v)]
            assert (0, "J window outside") in seen[(side, v)]           # the same bound inside the iteration loop


def test_every_status_rule_decides_some_point():
    lost = {}
    for name in NAMES:
        for tr in expected(name)[3]:
            lost[tr[0]["lost"]] = lost.get(tr[0]["lost"], 0) + 1
    print("status rules:", lost)
    assert set(lost) == {None, "I window outside", "minEig / determinant", "J window outside", "final window outside"}
    for name in ("final_window_x_64x61", "final_window_y_61x61"):
        _, nxt, st, trace = expected(name)
        h, w = CASES[name][0].shape[1:3]
        hit = [k for k, tr in enumerate(trace) if tr[0]["lost"] == "final window outside"]
        assert hit and st.any() and not st[hit].any()
        o = nxt[hit] - 7                                            # a final origin in the half pixel where floor() is inside the frame and rint() outside
        assert np.any((np.floor(o[:, 0]) < w) & (np.floor(o[:, 1]) < h) & ((np.rint(o[:, 0]) >= w) | (np.rint(o[:, 1]) >= h)))


def _moves(name):
    frames, src, dst, pts = CASES[name]
    got, nxt, st, _ = expected(name)
    prev = np.array(pts, np.float32).reshape(-1, 2)
    return got, np.linalg.norm(nxt[st == 1] - prev[st == 1], axis=1), st


def test_filter_cases_force_their_rule():
    got, move, st = _moves("filter_one_survivor_60x60")
    assert st.sum() == 1 and len(got) == 1 and got[0][0] == 0          # the survivor is row 0: it carries the FIRST label (the reference's bookkeeping)
    got, move, st = _moves("filter_identical_moves_61x61")
    assert st.sum() >= 10 and np.all(move == move[0]) and len(got) == st.sum()
    got, move, st = _moves("filter_outlier_243x321")
    z = (move - move.mean()) / (move.std() + 1e-6)
    assert st.all() and (z > 2).sum() == 1 and len(got) <= 9 and 4 not in [k for k, _ in got]
    # hue: some survivors are dropped by the hue rule alone, some are kept
    frames, src, dst, pts = CASES["filter_hue_change_64x61"]
    got, move, st = _moves("filter_hue_change_64x61")
    z = (move - move.mean()) / (move.std() + 1e-6)
    assert st.sum() >= 12 and len(got) >= 3 and (z <= 2).sum() - len(got) >= 3
    # corners of the smallest frame: survivors whose hue windows are clipped to 2 x 2 and 2 x 3 pixels
    frames, src, dst, pts = CASES["filter_corner_32x32"]
    _, nxt, st, _ = expected("filter_corner_32x32")
    corners = [k for k, p in enumerate(pts) if p in ((0, 0), (31, 0), (0, 31), (31, 31))]
    edges = [k for k, p in enumerate(pts) if (p[0] in (0, 31)) != (p[1] in (0, 31))]
    assert st[corners].sum() >= 2 and st[edges].sum() >= 2


def test_counts():
    assert expected("count_0_32x32")[0] == [] and len(expected("count_0_32x32")[2]) == 0
    assert len(expected("count_1_32x32")[2]) == 1 and len(expected("count_4_61x61")[2]) == 4


def test_a_dropped_gray_tail_or_a_truncated_pyramid_size_would_show():
    """The two K11 mutations of the pull request's check list, applied to the reference: without the scalar tail the last pixel of the odd clip stays what the
    zeroed buffer held, and with dh = h / 2 the flat output of an odd-height level is another picture."""
    frames = CASES["odd3_33x95_translate"][0]
    g = np.stack([lk_ref.gray(f) for f in frames])
    assert g.size % 4 == 1 and g.reshape(-1)[-1] != 0
    for name in ("odd3_33x95_translate", "translate_61x61", "translate_243x321_0"):
        frames = CASES[name][0]
        g = np.stack([lk_ref.gray(f) for f in frames])
        n, h, w = g.shape
        good = np.stack([lk_ref.pyrdown(x) for x in g]).reshape(-1)
        dh, dw = h // 2, (w + 1) // 2                           # the mutated kernel: same flat indexing, one row short per frame
        bad = np.zeros_like(good)
        bad[:n * dh * dw] = np.stack([lk_ref.pyrdown(x)[:dh] for x in g]).reshape(-1)
        assert h % 2 == 1 and not np.array_equal(good, bad)


def test_operator_entry_points_are_declared():
    from eagle_amd import lib
    head = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name in ("eagle_op_gray_pyramid", "eagle_op_flow"):
        assert re.search(r"^int %s\(" % name, head, re.M) and name in lib.EXPORTS
    assert callable(lib.op_gray_pyramid) and callable(lib.op_flow)
