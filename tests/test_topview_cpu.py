"""The top view's written definition (tests/topview_ref.py) without a GPU: its two statements agree on every constructed case of topview_cases.py, each
case forces what it is named after, the exact-copy cases return the frame, and the Python side around the library (homographies, to_json, the command
line's argument errors) does what eagle_amd/topview.py says."""
import json

import numpy as np
import pytest

import minimap_ref as MR
import topview_cases as TC
import topview_ref as R
from eagle_amd import topview

NAMES = [c["name"] for c in TC.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_the_two_statements_agree(name):
    c = TC.BY_NAME[name]
    got = R.topview_scalar(c["frames"], c["Hs"], c["valid"], c["boxes"], c["p"])
    for a, b, part in zip(got, TC.reference(name), ("video", "mosaic", "cnt", "res_sum", "res_cnt", "covered")):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (name, part)


def _points(name, i):
    c = TC.BY_NAME[name]
    _, h, w, _ = c["frames"].shape
    return R.sample_points(TC.maps(name)[i], c["p"]["scale"], c["p"]["margin"], h, w)


@pytest.mark.parametrize("S", (2, 4))
def test_exact_copy_returns_the_frame(S):
    c = TC.BY_NAME[f"exact_copy_S{S}"]
    vid, pic, cnt, rs, rc, cv = TC.reference(c["name"])
    assert np.array_equal(vid[0], c["frames"][0, :68 * S, :105 * S]) and np.array_equal(pic, vid[0]) and (cnt == 1).all()
    assert rs[0] == 0 and rc[0] == cv[0] == 105 * S * 68 * S


def test_det_negative_case():
    c = TC.BY_NAME["mirrored_det_negative"]
    assert np.linalg.det(c["Hs"][0].reshape(3, 3)) < 0
    vid = TC.reference(c["name"])[0]
    assert np.array_equal(vid[0, ::-1][:, :], c["frames"][0, 1:137, :210])      # v = 2 y = 136 - Y: the frame upside down


def test_tie_cases_contain_ties():
    c = TC.BY_NAME["half_pixel_ties"]
    G = TC.maps(c["name"])[0]
    cov, num, fx, fy, _, _ = R.numerators(c["frames"][0], G, 2, 0)
    tie = cov[..., None] & ((num & 65535) == 32768)
    for sel in ((fx == 128) & (fy == 0), (fx == 0) & (fy == 128), (fx == 128) & (fy == 128)):
        assert (tie & sel[..., None]).any()
    f = c["frames"][0].astype(int)
    assert (f[0, 0, 0] < f[0, 1, 0]) and (f[0, 1, 0] > f[0, 2, 0])              # both orders along a row
    acc = R.accumulate(TC.BY_NAME["mosaic_2_frames_mean_tie"]["frames"], TC.BY_NAME["mosaic_2_frames_mean_tie"]["Hs"], [1, 1], None, R.params(2, 0)).astype(np.int64)
    full = acc[..., 3] == 2
    assert full.any() and ((2 * acc[..., 0][full]) % 4 == 2).all() and (TC.reference("mosaic_2_frames_mean_tie")[1][full] == 11).all()


def test_edge_cases_sit_on_the_edges():
    u, v, wp, tu, tv, cov = _points("edges", 0)                                  # 4 x 4 frame: the last column is u = 3
    assert tu[0, 10] == 256 * 3 + 0.5 and cov[0, 10] and tu[0, 11] == 256 * 3 + 1.5 and not cov[0, 11] and tu[0, 9] == 256 * 3 - 0.5 and cov[0, 9]
    assert tv[7, 0] == 256 * 3 + 0.5 and cov[7, 0] and not cov[8, 0] and cov[6, 0] and cov[7, 10] and not cov[8, 11]
    u, v, wp, tu, tv, cov = _points("edges", 1)
    assert tu[3, 5] == 0.0 and cov[3, 5] and tu[3, 4] == -0.5 and not cov[3, 4] and tv[3, 5] == 0.0 and tv[2, 5] == -0.5 and not cov[2, 5]
    _, _, _, _, _, cov = _points("frame_1x1", 0)
    assert cov.sum() == 4 and cov[4:6, 9:11].all()


def test_pinhole_coverage_is_a_trapezoid_inside_the_canvas():
    _, _, _, _, _, cov = _points("pinhole_trapezoid", 0)
    ys, xs = np.nonzero(cov)
    assert ys.min() > 2 and xs.min() > 2 and ys.max() < cov.shape[0] - 3 and xs.max() < cov.shape[1] - 3
    widths = cov[ys.min():ys.max() + 1].sum(1)
    assert widths[0] > widths[len(widths) // 2] > widths[-1] > 0                 # the far edge (top of the canvas) is the wide one
    vid = TC.reference("pinhole_trapezoid")[0]
    mark = MR.markings(2, 2)
    assert (vid[0][mark] == R.colour(R.RED)).all() and (vid[0][~mark & ~cov] == 0).all()


def test_behind_the_camera_and_scaled_H():
    u, v, wp, tu, tv, cov = _points("behind_camera_and_scaled_H", 0)
    inside = (tu >= 0) & (tu < 256 * 63 + 1) & (tv >= 0) & (tv < 256 * 47 + 1)
    assert (inside & (wp < 0)).any() and not cov[wp <= 0].any() and cov.any()
    row = 2 * (68 - 20)
    assert (wp[row] == 0).all() and not cov[row].any() and (wp[row - 1] < 0).all() and (wp[row + 1] > 0).all()
    vid, _, _, rs, rc, cv = TC.reference("behind_camera_and_scaled_H")
    assert np.array_equal(vid[0], vid[1]) and np.array_equal(vid[0], vid[2]) and vid[0].any() and rc[0] == rc[1] == rc[2] > 0 and not rs.any()
    Hs = TC.BY_NAME["behind_camera_and_scaled_H"]["Hs"]
    assert np.array_equal(Hs[1], -Hs[0]) and np.array_equal(Hs[2], 3 * Hs[0])


def test_frames_without_a_map():
    c = TC.BY_NAME["no_map"]
    maps = TC.maps("no_map")
    assert [m is not None for m in maps] == [True, False, False, False, False, False, False, True, True]
    with np.errstate(all="ignore"):
        assert not np.isfinite(TC.adj(c["Hs"][4])).any() and np.isfinite(c["Hs"][4]).all()           # 1e200: the products of A overflow
    H = c["Hs"][5]
    assert H[6] * 1.5 + H[7] * 3 + H[8] == 0 and np.linalg.det(H.reshape(3, 3)) != 0                # sb == 0
    assert np.linalg.det(c["Hs"][1].reshape(3, 3)) == 0
    vid = TC.reference("no_map")[0]
    bg = R.colour(c["p"]["background"])
    for i in (1, 2, 3, 4, 5, 6, 7):
        assert (vid[i] == bg).all(), i
    assert (vid[0] != bg).any() and (vid[8] != bg).any()
    u, v, wp, tu, tv, cov = _points("no_map", 7)
    assert np.isinf(tu).any() and not cov.any()


def test_marking_colour_equal_to_a_picture_colour():
    vid, pic, _, _, _, _ = TC.reference("markings_in_a_picture_colour")
    mark = MR.markings(2, 2)
    red = R.colour(R.RED)
    assert (vid[0][mark] == red).all() and (vid[0][~mark] == red).all(1).any() and (vid[0][~mark] == R.colour(0x00ff00)).all(1).any() and (pic[mark] == red).all()


def test_mosaic_cases():
    vid, pic, cnt, rs, rc, cv = TC.reference("mosaic_0_frames")
    assert len(vid) == 0 and not cnt.any() and (pic[~MR.markings(2, 0)] == R.colour(0x010203)).all() and (pic[MR.markings(2, 0)] == R.colour(R.RED)).all()
    _, pic, cnt, rs, rc, _ = TC.reference("mosaic_1_frame_residual_0")
    assert rs[0] == 0 and rc[0] > 0 and cnt.max() == 1
    _, pic, cnt, rs, rc, _ = TC.reference("mosaic_3_frames_min_count")
    assert (cnt == 2).any() and (cnt == 1).any() and (pic[cnt == 1] == 0).all() and pic[cnt == 2].any() and cnt.max() == 2
    _, _, cnt, _, rc, _ = TC.reference("mosaic_65_frames")
    assert cnt.max() > 3 and len(rc) == 65 and (rc > 0).all()
    _, pic, cnt, rs, rc, cv = TC.reference("mosaic_skips_the_covering_frame")
    assert not cnt.any() and not pic.any() and cv[1] > 0 and rc[1] == 0 and rs[1] == 0           # a frame with no overlap with the mosaic
    _, _, _, rs, rc, _ = TC.reference("residual_constant_offset")
    assert rs[0] == 0 and rc[1] == rc[0] > 0 and rs[1] == 15 * rc[1]


def test_box_cases():
    c = TC.BY_NAME["boxes_edges_pad"]
    u, v, _, _, _, cov = _points(c["name"], 0)
    hit = R.in_boxes(u, v, c["boxes"][0], 0.5)
    # u = X / 2, v = Y / 2: the padded box is 1.5 .. 4.5 x 0.5 .. 3.5
    assert hit[1, 3] and hit[1, 9] and hit[7, 3] and hit[7, 9] and not hit[1, 2] and not hit[1, 10] and not hit[0, 3] and not hit[8, 9]
    assert u[1, 3] == 1.5 and u[1, 9] == 4.5 and v[1, 3] == 0.5 and v[7, 3] == 3.5
    cnt = TC.reference(c["name"])[2]
    assert cnt[1, 3] == 1 and cnt[1, 2] == 2 and cnt[8, 9] == 2 and cnt[7, 9] == 1
    cnt0 = TC.reference("boxes_pad_0")[2]
    assert cnt0[2, 4] == 1 and cnt0[1, 4] == 2 and cnt0[2, 3] == 2 and cnt0[6, 8] == 1 and cnt0[7, 8] == 2      # n_det = 0 in frame 1: it adds everywhere
    assert len(TC.BY_NAME["boxes_300"]["boxes"][0]) == R.MAX_DET and 0 < (TC.reference("boxes_300")[2] == 2).sum() < cov.sum()
    _, pic, cnt, rs, rc, cv = TC.reference("boxes_whole_frame")
    assert not cnt.any() and not rc.any() and (cv == cov.sum()).all() and not pic.any()


def test_homographies_carry():
    recs = TC.records_none_own_none_own()
    Hs, valid, kind = topview.homographies(recs)
    assert list(valid) == [0, 1, 0, 1] and list(kind) == [0, 1, 0, 1] and np.array_equal(Hs[1], recs[1]["H"].reshape(9)) and not Hs[0].any() and not Hs[2].any()
    Hs, valid, kind = topview.homographies(recs, carry=True)
    assert list(valid) == [0, 1, 1, 1] and list(kind) == [0, 1, 2, 1] and np.array_equal(Hs[2], Hs[1]) and np.array_equal(Hs[3], recs[3]["H"].reshape(9))


def test_to_json():
    p = dict(scale=2, margin=0, background=0, markings=0, marking_colour=255, mask_boxes=0, box_pad=0.0, first=0, step=1, min_count=1)
    res = topview.Result(None, None, np.array([30, 0, 300, 60], np.uint64), np.array([10, 0, 10, 10], np.uint32), np.array([28560, 0, 14280, 7140], np.uint32),
                         np.array([1, 0, 2, 1], np.uint8), p)
    d = json.loads(json.dumps(topview.to_json(res, carry=True)))
    assert [f["residual"] for f in d["frames"]] == [1.0, None, 10.0, 2.0] and [f["kind"] for f in d["frames"]] == [1, 0, 2, 1]
    assert [f["coverage"] for f in d["frames"]] == [1.0, 0.0, 0.5, 0.25] and d["median_residual"] == 2.0 and d["suspect_frames"] == [2]
    assert d["params"]["suspect"] == 2.0 and d["params"]["carry"] is True and d["params"]["scale"] == 2 and d["params"]["min_count"] == 1
    assert topview.to_json(res, suspect=0.4)["suspect_frames"] == [0, 2, 3]
    empty = topview.to_json(topview.Result(None, None, np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint8), p))
    assert empty["median_residual"] is None and empty["suspect_frames"] == [] and empty["frames"][0]["residual"] is None


@pytest.mark.parametrize("argv, text", [
    (["--topview-scale", "4"], "need --topview"), (["--topview-margin", "4"], "need --topview"), (["--topview-markings"], "need --topview"),
    (["--topview-carry"], "need --topview"), (["--topview-mosaic"], "need --topview"), (["--topview-mask-boxes", "2"], "need --topview"),
    (["--topview-step", "2"], "need --topview"), (["--topview-min-count", "2"], "need --topview"), (["--topview-suspect", "3"], "need --topview"),
    (["--topview", "--topview-scale", "3"], "--topview-scale"), (["--topview", "--topview-margin", "66"], "--topview-margin"),
    (["--topview", "--topview-step", "2"], "--topview-mosaic"), (["--topview", "--topview-mosaic", "--topview-step", "0"], "--topview-step"),
    (["--topview", "--topview-mosaic", "--topview-min-count", "0"], "--topview-min-count"), (["--topview", "--topview-mosaic", "--topview-mask-boxes", "-1"], "--topview-mask-boxes"),
    (["--topview", "--topview-mosaic", "--topview-suspect", "nan"], "--topview-suspect")])
def test_cli_argument_errors(argv, text, capsys):
    from eagle_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--clip", "none.npy", "--out", "none"] + argv)
    assert e.value.code == 2 and text in capsys.readouterr().err
