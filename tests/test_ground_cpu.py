"""The ground layer without a GPU: the two formulations of tests/ground_ref.py agree on every constructed case, each case of tests/ground_cases.py
forces what it is named after, eagle_amd/ground.py's offside_shapes gives the stated bands and rings on constructed offside rows, and the command line
refuses the new flags without what they need."""
import types

import numpy as np
import pytest

import ground_cases as GC
import ground_ref as R
from eagle_amd import ground, lib


@pytest.mark.parametrize("name", [c["name"] for c in GC.CASES])
def test_the_two_formulations_agree(name):
    c = GC.BY_NAME[name]
    pics, cov = GC.reference(name)
    win = GC.SCALAR_WINDOW.get(name)
    got, got_cov = R.frames_bgr_scalar(c["frames"], c["Hs"], c["valid"], c["shapes"], c["key"], win)
    if win is None:
        assert np.array_equal(got, pics) and np.array_equal(got_cov, cov)
    else:                                                   # the large case: the scalar loop walks a window that the line, the zone and a ring cross
        assert np.array_equal(got[:, win[0], win[1]], pics[:, win[0], win[1]]) and got_cov[0] > 1000
        assert len({tuple(p) for p in (pics[0, win[0], win[1]].astype(int) - c["frames"][0, win[0], win[1]]).reshape(-1, 3)}) > 50        # line, zone and ring blend there


def _samples(name, i=0):
    c = GC.BY_NAME[name]
    n, h, w, _ = c["frames"].shape
    return c, R.samples(c["Hs"][i], R.frame_sb(c["Hs"][i], c["valid"][i], h, w), h, w)


def test_the_horizon_case_has_sub_samples_on_both_sides_and_beyond_the_limit():
    c, (on, qx, qy, wp) = _samples("horizon_264x34")
    assert (wp > 0).any() and (wp < 0).any() and not (wp == 0).any()
    # above the horizon nothing; in row 10 two sub-samples lie above it, one maps to py = 1600 m (beyond the limit) and one to 533 m; further down the
    # columns far from the centre map beyond 1024 m in x
    assert not on[:, :10].any() and not on[:2, 10].any() and not on[2, 10].any() and on[3, 10, 132] and on[:, 20].all() and on[0, 11, 132] and not on[0, 11, 263]
    c3, (on3, qx3, qy3, wp3) = _samples("horizon_times_minus_3")
    assert R.frame_sb(c3["Hs"][0], 1, 34, 264) < 0 < R.frame_sb(c["Hs"][0], 1, 34, 264)
    assert np.array_equal(on, on3) and np.array_equal(qx, qx3) and np.array_equal(qy, qy3)
    assert np.array_equal(GC.reference("horizon_times_minus_3")[0], GC.reference("horizon_264x34")[0])
    assert GC.reference("horizon_264x34")[1][0] > 0


def test_no_map_frames_are_passed_through():
    c = GC.BY_NAME["no_map"]
    pics, cov = GC.reference("no_map")
    maps = [R.frame_sb(c["Hs"][i], c["valid"][i], 34, 264) for i in range(5)]
    assert [m is None for m in maps] == [True, True, True, True, False]
    assert np.array_equal(pics[:4], c["frames"][:4]) and list(cov[:4]) == [0] * 4 and cov[4] > 0
    assert not np.isfinite(c["Hs"][1]).all() and c["valid"][2] == 1 and np.isfinite(c["Hs"][2]).all()      # frame 2: sb == 0 alone


def test_the_edge_case_has_every_coverage_count_and_edges_on_q():
    c, (on, qx, qy, _) = _samples("band_edges_on_q")
    assert on.all()
    counts = set()
    for s in c["shapes"][0]:
        cv = R.coverage(s, on, qx, qy)
        counts |= set(np.unique(cv).tolist())
    assert counts == {0, 1, 2, 3, 4}
    e = [s["a"] for s in c["shapes"][0]]                       # these edges lie on a sub-sample's q: both sides of the half-open interval, in x and in y
    assert (qx == e[0][0]).any() and (qx == e[0][1]).any() and (qx == e[1][1]).any() and (qy == e[2][2]).any() and (qy == e[2][3]).any() and (qy == e[3][3]).any()
    first = R.coverage(c["shapes"][0][0], on, qx, qy)
    assert first[0, 5] == 3 and first[0, 9] == 2 and first[0, 4] == 0 and first[0, 10] == 0 and first[0, 7] == 4
    assert R.coverage(c["shapes"][0][1], on, qx, qy)[8, 20] == 1


def test_the_keyed_case_has_pixels_on_both_sides_of_both_thresholds():
    c = GC.BY_NAME["keyed_thresholds_38x18"]
    f = c["frames"][0].astype(int)
    g, lead = f[..., 1], f[..., 1] - np.maximum(f[..., 0], f[..., 2])
    gr = R.grass(c["frames"][0], c["key"])
    for want_g, want_lead, is_grass in ((47, 47, False), (48, 48, True), (48, 15, False), (48, 16, True)):
        m = (g == want_g) & (lead == want_lead)
        assert m.any() and (gr[m] == is_grass).all()
    pics, cov = GC.reference("keyed_thresholds_38x18")
    _, (on, qx, qy, _) = _samples("keyed_thresholds_38x18")
    inside = R.coverage(c["shapes"][0][0], on, qx, qy) == 4
    changed = (pics[0] != c["frames"][0]).any(-1)
    assert (inside & gr & changed).any() and not (inside & ~gr & changed & (R.coverage(c["shapes"][0][2], on, qx, qy) == 0)).any() and (inside & ~gr).any()


def test_alpha_and_order():
    pics, cov = GC.reference("alpha_0_and_256")
    c = GC.BY_NAME["alpha_0_and_256"]
    assert np.array_equal(pics[0], c["frames"][0]) and cov[0] == 0 and cov[1] > 0
    _, (on, qx, qy, _) = _samples("alpha_0_and_256", 1)
    full = R.coverage(c["shapes"][1][1], on, qx, qy) == 4
    assert (pics[1][full] == 255).all()                      # alpha 256 on four sub-samples replaces the pixel
    both, cov = GC.reference("overlap_both_orders")
    assert cov[0] == cov[1] and not np.array_equal(both[0], both[1])
    pics, cov = GC.reference("shapes_16_then_0")
    c = GC.BY_NAME["shapes_16_then_0"]
    assert len(c["shapes"][0]) == R.MAX_SHAPES and c["shapes"][1] == [] and cov[0] > 0 and cov[1] == 0 and np.array_equal(pics[1], c["frames"][1])


def test_the_one_corner_case_covers_one_pixel_of_the_first_tile():
    c, (on, qx, qy, _) = _samples("one_corner_sub_sample")
    cv = R.coverage(c["shapes"][0][0], on, qx, qy)
    tile = cv[:GC.TILE_H, :GC.TILE_W]
    assert (tile > 0).sum() == 1 and tile[15, 255] == 1 and (cv[GC.TILE_H:] > 0).any() and (cv[:, GC.TILE_W:] > 0).any()
    assert on[2, 15, 255] and (qx[2, 15, 255], qy[2, 15, 255]) == (c["shapes"][0][0]["a"][0], c["shapes"][0][0]["a"][2])


def test_the_large_case_and_the_sizes():
    sizes = {c["frames"].shape[1:3] for c in GC.CASES}
    assert {(34, 264), (18, 38), (19, 37), (1, 1), (2, 8), (720, 1280)} <= sizes
    assert all(c["formats"] == GC.BGR for c in GC.CASES if c["frames"].shape[1] % 2 or c["frames"].shape[2] % 2)
    c, (on, qx, qy, wp) = _samples("pinhole_1280x720")
    assert on.any() and GC.reference("pinhole_1280x720")[1][0] > 10000
    for name, fmt, layout in GC.PADDED:
        assert fmt in GC.BY_NAME[name]["formats"]


# ---- offside_shapes on constructed offside rows -------------------------------------------------------------------------------------------------------
def _rows():
    """three rows, two members per group (columns 0, 1: group 0; 2, 3: group 1) and a ball column 4; group 0 attacks right.  Row 0: both records OK;
    row 1: group 0 TOO_FEW, group 1 OK; row 2: nothing OK"""
    rec = np.zeros((3, 2), lib.OFFSIDE_ROW_DTYPE)
    rec["status"] = [[lib.OFFSIDE_OK, lib.OFFSIDE_OK], [lib.OFFSIDE_TOO_FEW, lib.OFFSIDE_OK], [lib.OFFSIDE_TOO_FEW, lib.OFFSIDE_NO_DIRECTION]]
    rec["line_qx"] = [[80 * 1024, 30 * 1024 + 7], [0, 25 * 1024], [0, 0]]
    rec["second_col"] = [[2, 0], [-1, 1], [-1, -1]]
    totals = np.zeros(4, lib.OFFSIDE_TOTALS_DTYPE)
    totals["col"], totals["group"] = [0, 1, 2, 3], [0, 0, 1, 1]
    margins = np.full((4, 3), lib.OFFSIDE_NONE, np.int32)
    margins[:, 0] = [5, -100, 0, 2048]                          # member 0 (group 0) and member 3 (group 1) are beyond their lines on row 0
    margins[2:, 1] = [-1, -2]
    clip = np.zeros(1, lib.OFFSIDE_CLIP_DTYPE)
    clip["direction"] = lib.OFFSIDE_DIR_RIGHT
    values = np.full((5, 3, 2), np.nan)
    values[:4, :, 0] = np.array([81.0, 60.5, 80.0, 28.25])[:, None]
    values[:4, :, 1] = np.array([10.0, 20.0, 30.125, 40.0])[:, None]
    return types.SimpleNamespace(values=values, rows=np.arange(3)), (rec, margins, totals, clip)


def _as_tuples(shapes, off):
    return [[(int(s["kind"]), tuple(int(t) for t in s["a"][:4]), int(s["colour"]), int(s["alpha"]), int(s["flags"])) for s in shapes[off[i]: off[i + 1]]] for i in range(len(off) - 1)]


def test_offside_shapes_gives_the_stated_bands_and_rings():
    table, res = _rows()
    wq = 256
    r0, r1 = 614, 922
    red, blue = ground.GROUP_COLOURS
    assert (red, blue) == (0xFF0000, 0x0000FF) and ground.q(0.25) == wq and (ground.q(0.6), ground.q(0.9)) == (r0, r1)
    K = lib.GROUND_KEYED
    g0 = [(lib.GROUND_BAND, (80 * 1024, 107520, 0, 69632), red, 48, K), (lib.GROUND_BAND, (80 * 1024 - 128, 80 * 1024 + 128, 0, 69632), red, 208, K),
          (lib.GROUND_RING, (80 * 1024, 30 * 1024 + 128, r0, r1), ground.SECOND, 160, K), (lib.GROUND_RING, (81 * 1024, 10 * 1024, r0, r1), ground.WARNING, 160, K)]
    L1 = 30 * 1024 + 7                                         # group 1 attacks left: its zone runs from the goal line x = 0 to the line
    g1 = [(lib.GROUND_BAND, (0, L1, 0, 69632), blue, 48, K), (lib.GROUND_BAND, (L1 - 128, L1 + 128, 0, 69632), blue, 208, K),
          (lib.GROUND_RING, (81 * 1024, 10 * 1024, r0, r1), ground.SECOND, 160, K), (lib.GROUND_RING, (28 * 1024 + 256, 40 * 1024, r0, r1), ground.WARNING, 160, K)]
    row1 = [(lib.GROUND_BAND, (0, 25 * 1024, 0, 69632), blue, 48, K), (lib.GROUND_BAND, (25 * 1024 - 128, 25 * 1024 + 128, 0, 69632), blue, 208, K),
            (lib.GROUND_RING, (60 * 1024 + 512, 20 * 1024, r0, r1), ground.SECOND, 160, K)]
    assert _as_tuples(*ground.offside_shapes(table, res, 0)) == [g0, [], []]
    assert _as_tuples(*ground.offside_shapes(table, res, 1)) == [g1, row1, []]
    assert _as_tuples(*ground.offside_shapes(table, res, "both")) == [g0 + g1, row1, []]
    # "possession" follows the owner's group; no owner, or an owner that is no member (the ball's column), draws nothing
    assert _as_tuples(*ground.offside_shapes(table, res, "possession", owner=[3, 0, 2])) == [g1, [], []]
    assert _as_tuples(*ground.offside_shapes(table, res, "possession", owner=[1, 2, -1])) == [g0, row1, []]
    assert _as_tuples(*ground.offside_shapes(table, res, "possession", owner=[-1, 4, 0])) == [[], [], []]
    # the switches: no zone, no rings, not keyed; the line is exactly wq wide for an odd wq too
    plain = _as_tuples(*ground.offside_shapes(table, res, 0, width=0.2, zone=False, rings=False, keyed=False))
    wq = ground.q(0.2)
    assert wq == 205 and plain == [[(lib.GROUND_BAND, (80 * 1024 - 102, 80 * 1024 - 102 + 205, 0, 69632), red, 208, 0)], [], []]
    shapes, off = ground.offside_shapes(table, res, "both")
    assert shapes.dtype == lib.GROUND_SHAPE_DTYPE and off.dtype == np.int32 and list(off) == [0, 8, 11, 11]
    for s in R_lists(shapes):
        R.check_shape(s)
    with pytest.raises(lib.EagleError, match="team"):
        ground.offside_shapes(table, res, "home")
    with pytest.raises(lib.EagleError, match="owners"):
        ground.offside_shapes(table, res, "possession", owner=[0])
    with pytest.raises(lib.EagleError, match="width"):
        ground.offside_shapes(table, res, 0, width=0.0001)


def R_lists(shapes):
    return [dict(kind=int(s["kind"]), a=tuple(int(t) for t in s["a"]), colour=int(s["colour"]), alpha=int(s["alpha"]), flags=int(s["flags"])) for s in shapes]


def test_offside_shapes_keeps_to_16_per_row_and_skips_an_unresolved_clip():
    table, (rec, margins, totals, clip) = _rows()
    n = 20
    totals = np.zeros(n, lib.OFFSIDE_TOTALS_DTYPE)
    totals["col"], totals["group"] = np.arange(n), 0
    margins = np.full((n, 3), 1, np.int32)
    table.values = np.full((n, 3, 2), 50.0)
    rec["second_col"][0, 0] = 0
    shapes, off = ground.offside_shapes(table, (rec, margins, totals, clip), 0)
    assert off[1] == lib.GROUND_MAX_SHAPES and (shapes["kind"][:2] == lib.GROUND_BAND).all() and (shapes["kind"][2:16] == lib.GROUND_RING).all()
    clip["direction"] = 0
    assert list(ground.offside_shapes(table, (rec, margins, totals, clip), "both")[1]) == [0, 0, 0, 0]


def test_a_line_on_the_goal_line_has_no_zone():
    assert [int(s["a"][0]) for s in ground.line_shapes(107520, 0, True)] == [107520 - 128]
    assert [int(s["a"][1]) for s in ground.line_shapes(0, 1, False)] == [128]
    assert len(ground.line_shapes(53760, 0, True)) == 2 and len(ground.line_shapes(53760, 1, False, zone=False)) == 1


# ---- the command line refuses the new flags without what they need ----------------------------------------------------------------------------------
@pytest.mark.parametrize("args, text", [
    (["--offside-view"], "--processed --offside"), (["--processed", "--offside-view"], "--processed --offside"), (["--processed", "--offside-stills"], "--processed --offside"),
    (["--processed", "--offside", "--offside-stills"], "--possession"), (["--processed", "--offside", "--offside-view-team", "both"], "--offside-view"),
    (["--processed", "--offside", "--offside-view-width", "0.5"], "--offside-view or --offside-stills"), (["--processed", "--offside", "--offside-view-no-zone"], "--offside-view or"),
    (["--processed", "--offside", "--offside-view-no-key"], "--offside-view or"), (["--processed", "--offside", "--offside-view", "--offside-view-team", "possession"], "--possession"),
    (["--processed", "--offside", "--offside-view", "--offside-view-width", "0"], "> 0"), (["--processed", "--offside", "--offside-view", "--offside-view-width", "11"], "<= 10"),
    (["--processed", "--offside", "--offside-view", "--offside-view-team", "home"], "invalid choice")])
def test_cli_refuses_the_flags_without_their_prerequisites(args, text, capsys, tmp_path):
    from eagle_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--frames", "2", "--fps", "5", "--synthetic-weights", "--out", str(tmp_path / "out")] + args)
    assert e.value.code == 2 and text in capsys.readouterr().err
