"""The occupancy contract without a GPU (tests/occupancy_ref.py; the kernels of csrc/occupancy.hip are held against it in tests/test_gpu_occupancy.py):
every constructed table of tests/occupancy_cases.py forces the edge it is named after; sigma = 0 returns the counts; a single interior point gives a
map symmetric in both axes whose sum is w (sum of the taps)^2; total + outside is the weight of the present cells; a radius beyond the grid clips on
both sides (not reachable through the library, whose sigma ends at 10 m: rad <= 30 R < 68 R); the module's selections, thirds and channels; the JSON
round trip; the CLI's flag errors."""
import json

import numpy as np
import pytest

import occupancy_cases as OC
import occupancy_ref as OR

F = np.float32
NAMES = [c["name"] for c in OC.CASES]


def _ref(name):
    return OC.reference(name), OC.BY_NAME[name]


@pytest.mark.parametrize("name", NAMES)
def test_total_plus_outside_is_the_weight_of_the_present_cells(name):
    res, c = _ref(name)
    w = OR.weights(c["frames"], c["max_gap"])
    present = np.isfinite(c["values"]).all(2)
    for s in range(len(c["sel_off"]) - 1):
        mem = c["sel_cols"][c["sel_off"][s]:c["sel_off"][s + 1]]
        assert res["total"][s] + res["outside"][s] == sum(int(w[present[m]].sum()) for m in mem)
        assert res["counts"][s].sum() == res["total"][s] and res["counts"][s].min() >= 0
    assert res["grids"].dtype == F and res["bytes"].dtype == np.uint8 and np.isfinite(res["grids"]).all()
    assert len(c["frames"]) * c["max_gap"] * max(np.diff(c["sel_off"]), default=0) < 2 ** 31           # the library's 32-bit bound holds for every case


@pytest.mark.parametrize("R", OR.RS)
def test_cases_edges(R):
    res, c = _ref("edges_R%d" % R)
    gw, gh = OR.size(R)
    cnt = res["counts"][0]
    pts = OC.EDGE_POINTS
    inside = [(0.0, 0.0), (0.0, 5.5), (5.5, 0.0), (OC.BELOW_105, OC.BELOW_68), (OC.BELOW_105, 5.5), (5.5, OC.BELOW_68), (-0.0, -0.0), (-0.0, 7.25), (52.5, 34.0)]
    absent = 6                                                                 # a NaN or an infinity in either coordinate
    assert res["total"][0] == len(inside) and res["outside"][0] == len(pts) - len(inside) - absent
    assert cnt[0, 0] == 2 and cnt[gh - 1, gw - 1] == 1 and cnt[int(5.5 * R), gw - 1] == 1 and cnt[gh - 1, int(5.5 * R)] == 1      # (0, 0) and (-0, -0)
    assert cnt[int(5.5 * R), 0] == 1 and cnt[int(7.25 * R), 0] == 1 and cnt[0, int(5.5 * R)] == 1 and cnt[34 * R, int(52.5 * R)] == 1
    assert OC.BELOW_105 * R < gw and np.floor(OC.BELOW_105 * R) == gw - 1 and 105.0 * R == gw


@pytest.mark.parametrize("R", OR.RS)
def test_cases_corners_and_centre(R):
    res, c = _ref("corners_centre_R%d" % R)
    gw, gh = OR.size(R)
    cnt, v = res["counts"][0], res["grids"][0]
    assert [cnt[0, 0], cnt[0, gw - 1], cnt[gh - 1, 0], cnt[gh - 1, gw - 1], cnt[34 * R, int(52.5 * R)]] == [1] * 5 and cnt.sum() == 5
    rad, t = OR.taps(c["sigma"], R)
    assert rad == 6 * R
    # a corner keeps a quarter of its kernel (border clipping, no renormalisation), the centre all of it
    full = float(np.sum(np.concatenate([t[:0:-1], t]), dtype=np.float64)) ** 2
    centre = float(v[34 * R - rad:34 * R + rad + 1, int(52.5 * R) - rad:int(52.5 * R) + rad + 1].sum(dtype=np.float64))
    corner = float(v[:rad + 1, :rad + 1].sum(dtype=np.float64))
    quarter = float(np.sum(t, dtype=np.float64)) ** 2
    assert centre == pytest.approx(full, rel=1e-5) and corner == pytest.approx(quarter, rel=1e-5)
    assert v[0, 0] == v[0, gw - 1] == v[gh - 1, 0] == v[gh - 1, gw - 1] == F(1.0)


def test_cases_radii():
    for key, (sigma, R, rad) in OC.RADII.items():
        res, c = _ref(key)
        got, t = OR.taps(c["sigma"], c["R"])
        assert got == rad and len(t) == rad + 1 and t[0] == 1 and np.isfinite(t).all() and (t > 0).all(), key
        assert rad <= 30 * R < 68 * R
    r = {k: v[2] for k, v in OC.RADII.items()}
    assert r["rad0"] == 0 and r["rad1"] == 1 and 1 < r["rad_below_tile"] < OC.BLUR_TILE == r["rad_is_tile"] < r["rad_beyond_tile"] < r["rad_max"] == 120
    with np.errstate(all="ignore"):
        s = F(1e-30) * F(2)
        assert not np.isfinite(F(1.0) / (F(2.0) * s * s))                       # rad1_inv_inf: the formula's t[0] would be -0 x inf
    assert np.array_equal(_ref("rad0")[0]["grids"], _ref("rad0")[0]["counts"].astype(F))


def test_cases_contention():
    res, c = _ref("one_cell_4096")
    assert len(c["frames"]) == 4096 and np.count_nonzero(res["counts"]) == 1 and res["counts"].max() == 4096 == res["total"][0]
    res, c = _ref("one_cell_two_columns_4096")
    assert list(c["sel_off"]) == [0, 2] and np.count_nonzero(res["counts"]) == 1 and res["counts"].max() == 8192


def test_cases_frame_steps():
    res, c = _ref("frame_steps")
    assert np.diff(c["frames"]).tolist() == [1, 1, 3, 7, 8, 1] and c["max_gap"] == 7
    assert OR.weights(c["frames"], 7).tolist() == [1, 1, 3, 7, 1, 1, 1]         # steps of 1, k, exactly max_gap, max_gap + 1 (one frame), the last row
    assert res["counts"][0][10, [2, 5, 8, 11, 14, 17, 20]].tolist() == [1, 1, 3, 7, 1, 1, 1]


def test_cases_selections():
    res, c = _ref("selections")
    assert np.diff(c["sel_off"]).tolist() == [0, 2, 1, 4, 1, 0]
    assert not res["counts"][0].any() and not res["grids"][5].any() and not res["bytes"][0].any() and res["total"][0] == res["outside"][5] == 0
    assert np.array_equal(res["counts"][1], res["counts"][2] + OR.histogram(c["values"], c["frames"], c["columns"], [0, 1], [6], c["R"], c["max_gap"])[0][0])
    assert c["columns"][12][0] == OC.BALL and res["total"][4] > 0 and res["total"][3] > res["total"][1] > res["total"][2] > 0
    res, c = _ref("ball_only_table")
    assert [k for k, _, v in c["columns"] if not v and k != OC.BND] == [OC.BALL] and list(c["sel_off"]) == [0, 1] and res["total"][0] > 0
    res, c = _ref("no_person_no_ball")
    assert list(c["sel_off"]) == [0, 0] and c["sel_cols"] == [] and not res["grids"].any()            # the ball's selection, empty
    res, c = _ref("everyone_R2")
    assert len(c["sel_off"]) - 1 == 23 + 2 + 1 and res["outside"].sum() > 0


def test_cases_count_beyond_2p24_rounds():
    res, c = _ref("count_above_2p24")
    n = int(res["counts"].max())
    assert n == res["total"][0] >= 2 ** 24 and n == 131073 * 128 + 1 and int(F(n)) != n
    assert np.count_nonzero(res["counts"]) == 1


@pytest.mark.parametrize("n", OC.ROWS)
def test_cases_rows(n):
    res, c = _ref("rows_%d" % n)
    assert len(c["frames"]) == n and res["total"].sum() + res["outside"].sum() > 0


# ---- properties of the contract ------------------------------------------------------------------------------------------------------------
def test_single_interior_point_is_symmetric_and_sums_to_w_times_taps_squared():
    for R, sigma, w in ((1, 2.0, 3), (2, 1.5, 1), (4, 0.8, 5)):
        gw, gh = OR.size(R)
        cnt = np.zeros((1, gh, gw), np.int64)
        j, i = gh // 2 - 1, gw // 2
        cnt[0, j, i] = w
        v = OR.smooth(cnt, sigma, R)[0]
        rad, t = OR.taps(sigma, R)
        win = v[j - rad:j + rad + 1, i - rad:i + rad + 1]
        assert np.array_equal(win, win[::-1]) and np.array_equal(win, win[:, ::-1])          # (not its transpose: (w t_i) t_j rounds differently from (w t_j) t_i)
        assert not v[:j - rad].any() and not v[:, i + rad + 1:].any()
        full = float(np.sum(np.concatenate([t[:0:-1], t]), dtype=np.float64))
        assert float(v.sum(dtype=np.float64)) == pytest.approx(w * full * full, rel=2e-6)
        assert OR.to_bytes(v[None])[0, j, i] == 255 and OR.to_bytes(v[None]).max() == 255


def test_a_radius_beyond_the_grid_clips_on_both_sides():
    R, sigma = 1, 25.0
    rad, t = OR.taps(sigma, R)
    assert rad == 75 > 68
    cnt = np.zeros((1, 68, 105), np.int64)
    cnt[0, 10, 50] = 2
    cnt[0, 60, 3] = 1
    v = OR.smooth(cnt, sigma, R)[0]
    exp = np.zeros((68, 105), np.float64)
    for (j0, i0), w in (((10, 50), 2), ((60, 3), 1)):
        ty = np.array([t[abs(j - j0)] if abs(j - j0) <= rad else 0.0 for j in range(68)], np.float64)
        tx = np.array([t[abs(i - i0)] if abs(i - i0) <= rad else 0.0 for i in range(105)], np.float64)
        exp += w * ty[:, None] * tx[None, :]
    assert np.allclose(v, exp, rtol=1e-5, atol=0) and v.min() > 0              # every cell is within reach: taps dropped at both ends of every column


def test_module_selections_and_shares():
    from eagle_amd import lib, occupancy as oc
    c = OC.BY_NAME["everyone_R2"]
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    off, sc, names = oc.default_selections(cols, c["mapping"])
    assert (off, sc, names) == OR.default_selections(c["columns"], c["mapping"]) and (off, sc) == (c["sel_off"], c["sel_cols"])
    kinds = [n["kind"] for n in names]
    assert kinds == ["player"] * 22 + ["goalkeeper", "team", "team", "ball"] and [n["team"] for n in names if n["kind"] == "team"] == [0, 1]
    mapped = [4 + 2 * i for i in range(22) if i % 5 != 4]
    assert sorted(sc[off[23]:off[25]]) == mapped and 4 + 2 * 22 not in sc[off[23]:off[25]]               # no goalkeeper, no unmapped player in a team
    assert oc.default_selections(cols, None)[2][-2]["kind"] == "goalkeeper"                             # no mapping: no team maps
    res = OC.reference("everyone_R2")
    d = oc.summarise(res["grids"], res["counts"], res["total"], res["outside"], names, c["fps"], c["R"], c["sigma"])
    assert d["grids"].dtype == np.float64 and np.array_equal(d["grids"], res["grids"].astype(np.float64) / 5.0)
    for s, sel in enumerate(d["selections"]):
        assert sel["seconds"] == res["total"][s] / 5.0 and sel["outside_seconds"] == res["outside"][s] / 5.0
        assert (sel["thirds"], sel["channels"]) == OR.shares(res["counts"][s], c["R"])
        if res["total"][s]:
            assert sum(sel["thirds"]) == pytest.approx(1.0, abs=1e-12) and sum(sel["channels"]) == pytest.approx(1.0, abs=1e-12)
        else:
            assert sel["thirds"] == [0.0] * 3 == sel["channels"]
    # a hand table at one cell per metre: the x thirds fall on cell edges (35, 70), the y thirds (22.67, 45.33) do not: a cell counts by its centre
    cnt = np.zeros((68, 105), np.int64)
    cnt[0, 34], cnt[0, 35], cnt[22, 69], cnt[23, 70], cnt[45, 104], cnt[67, 0] = 1, 2, 3, 4, 5, 6
    thirds, chans = oc.shares(cnt, 1)
    assert thirds == [7 / 21, 5 / 21, 9 / 21] and chans == [6 / 21, 4 / 21, 11 / 21]
    j = json.loads(json.dumps(oc.to_json(d)))
    back = oc.from_json(j, d["grids"])
    assert back["selections"] == d["selections"] and np.array_equal(back["grids"], d["grids"]) and set(back) == set(d) and "grids" not in j


def test_picture_of_the_contract():
    res, c = _ref("corners_centre_R2")
    img = OR.picture(res["bytes"][0], 2, 4, 8, (0, 0, 255))
    import minimap_ref as MR
    w, h = MR.size(4, 8)
    assert img.shape == (h, w, 3) and (img[MR.markings(4, 8)] == 255).all()
    rest = ~MR.markings(4, 8)
    assert not img[..., :2][rest].any() and img[..., 2][rest].max() > 0 and not img[:8][rest[:8]].any()      # red only, the margin black


def test_cli_flag_errors():
    from eagle_amd import cli
    for argv in (["--occupancy"], ["--processed", "--occupancy-pictures"], ["--processed", "--occupancy", "--occupancy-grid", "3"]):
        with pytest.raises(SystemExit) as e:
            cli.main(["--frames", "2", "--synthetic-weights"] + argv)
        assert e.value.code == 2
