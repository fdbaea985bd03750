"""Every constructed case of tests/tail_cases.py is what its name says (no GPU): the oracle's plain functions are run on each case and the tie or edge the
case exists for is asserted, so a case that stops exercising its edge fails here instead of passing silently on the GPU.  Also the configuration check
that refuses a detector geometry with more anchors than the NMS kernel sorts."""
import numpy as np
import pytest

import tail_cases as T


def _sorted_conf(case, f):
    rows = T.detector_rows(case, f)
    order = T.sorted_candidates(rows, case["conf_floor"])
    return rows, order, rows[:, 4:].max(1)[order]


def _full_nms(case, f):
    """survivors without the 300-box cap, as sorted positions"""
    from oracle import host
    rows, order, conf = _sorted_conf(case, f)
    dets = host.nms_and_scale(rows, *case["frame_hw"], *case["in_hw"], conf_thres=case["conf_floor"], iou_thres=case["nms_iou"], max_det=10 ** 6)
    assert len(np.unique(conf)) == len(conf), "positions are recovered from distinct confidences"
    return np.searchsorted(-conf, -dets[:, 4]), len(conf)


def test_detector_cases_are_finite_and_decode_exactly():
    for name, case in T.detector_cases().items():
        for b, c, _ in case["levels"]:
            assert np.isfinite(b).all() and np.isfinite(c).all(), name
    # the constructed boxes are the integers they were meant to be: frame 0 of the threshold case
    case = T.case_iou_threshold()
    boxes, conf, cls = T.decode_scratch(T.detector_rows(case, 0))
    assert np.array_equal(boxes[1], np.float32([0.5, 0.5, 3.5, 2.5]) * 8) and np.array_equal(boxes[2], np.float32([1.5, 0.5, 4.5, 2.5]) * 8)


def test_counts_case_has_the_sort_edges():
    case = T.case_counts()
    got = [T.detector_expected(case, f)[2] for f in range(8)]
    assert got == [0, 1, 2, 63, 64, 65, 1024, 1025]


def test_all_candidates_case_fills_the_largest_geometry():
    case = T.case_all_candidates()
    for f in range(2):
        dets, _, cnt = T.detector_expected(case, f)
        assert cnt == 10710 == sum(b.shape[1] * b.shape[2] for b, _, _ in case["levels"]) and len(dets) == 300


def test_cap_case_stops_where_it_says():
    case = T.case_cap()
    for f, want in enumerate((300, 319, 320)):
        pos, n = _full_nms(case, f)
        assert len(pos) > 300, "more than 300 survivors before the cap"
        assert pos[300] == want, (f, pos[300])           # the 301st alive candidate: mid-block, a block's last lane, the next block's first lane
        assert len(T.detector_expected(case, f)[0]) == 300
    assert 300 % 64 not in (0, 63) and 319 % 64 == 63 and 320 % 64 == 0


def test_cross_block_case_suppresses_far_behind_and_keeps_the_chain_end():
    case, abc = T.case_cross_block()
    rows, order, conf = _sorted_conf(case, 0)
    pos, n = _full_nms(case, 0)
    assert n > 1024 + 64 and len(pos) == 16 < 300
    boxes, _, _ = T.decode_scratch(rows)
    sb = boxes[order]
    # every kept block box has identical copies (victims) at least 128 sorted positions behind it, and beyond position 64 + 1024 of its own 64-block
    far = 0
    for p in pos:
        same = np.nonzero((sb == sb[p]).all(1))[0]
        if len(same) > 1:
            assert same.min() == p
            assert same.max() - p >= 128
            far += int((same >= (p // 64) * 64 + 64 + 1024).any())
    assert far >= 14
    pa, pb, pc = (int(np.nonzero(order == a)[0][0]) for a in abc)
    assert (pa, pb, pc) == (5, 130, 1300)
    assert pa in pos and pb not in pos and pc in pos, "A kills B, C survives"


def test_ties_case_has_equal_confidences_among_the_kept_boxes():
    case = T.case_ties()
    d0 = T.detector_expected(case, 0)[0]
    d1 = T.detector_expected(case, 1)[0]
    assert len(d0) == 300 and len(np.unique(d0[:, 4])) <= 6 and len(np.unique(d1[:, 4])) == 1 and len(d1) == 200
    rows, order, conf = _sorted_conf(case, 0)
    runs = np.diff(np.nonzero(np.diff(conf) != 0)[0])
    assert 64 in runs and 130 in runs                      # tied runs as long as a block and longer than two
    assert conf[299] == conf[300], "the cap falls inside a run of equal confidences"
    assert (np.diff(order[conf == conf[10]]) > 0).all(), "ties are walked in anchor order"
    assert list(order[:2]) == [10, 11] and conf[0] == conf[1], "the two tied copies of one box lead the order"
    assert d0[0, 4] == conf[0] and d0[1, 4] < conf[0], "only one of them is kept"


def test_iou_threshold_case():
    case = T.case_iou_threshold()
    rows = T.detector_rows(case, 0)
    b, conf, _ = T.decode_scratch(rows)

    def iou(i, j):
        iw = max(np.float32(0), min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0])); ih = max(np.float32(0), min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]))
        ai = (b[i, 2] - b[i, 0]) * (b[i, 3] - b[i, 1]); aj = (b[j, 2] - b[j, 0]) * (b[j, 3] - b[j, 1])
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.float32(iw * ih) / np.float32(ai + aj - iw * ih)
    assert iou(1, 2) == np.float32(0.5) == case["nms_iou"]
    assert iou(81, 82) == np.float32(0.6)
    assert np.isnan(iou(165, 166)) and iou(169, 189) == 0
    dets = T.detector_expected(case, 0)[0]
    kept = set(np.float32(dets[:, 4]).tolist())
    assert {float(conf[1]), float(conf[2]), float(conf[81]), float(conf[165]), float(conf[166]), float(conf[169]), float(conf[189])} <= kept
    assert float(conf[82]) not in kept


def test_classes_case():
    case = T.case_classes()
    dets, objects, cnt = T.detector_expected(case, 0)
    cls = dets[:, 5].astype(int)
    assert set(cls) == {0, 1, 2, 3, 4}
    same = [(i, j) for i in range(len(dets)) for j in range(i + 1, len(dets)) if np.array_equal(dets[i, :4], dets[j, :4])]
    assert any(cls[i] != cls[j] for i, j in same), "one box kept once per class"
    assert cnt == len(dets) + 1, "the third copy (same class) is suppressed"
    assert (cls == 2).sum() == 9 and sorted(objects["Ball"]) == list(range(7)), "ball ids count earlier kept balls; two balls are below detector_conf"
    assert 0.5 in dets[:, 4] and (dets[:, 4] < 0.5).sum() == 3
    assert len(objects["Player"]) + len(objects["Goalkeeper"]) == ((cls <= 1) & (dets[:, 4] >= 0.5)).sum()
    fh, fw = case["frame_hw"]
    assert any(o["BBox"][2] == fw - 1 for o in objects["Player"].values()) and any(o["BBox"][2] == fw for o in objects["Ball"].values())
    assert any(o["BBox"][3] == fh - 1 for o in objects["Goalkeeper"].values()) and any(o["BBox"][3] == fh for o in objects["Ball"].values())
    assert (dets[:, 0] == 0).any() and (dets[:, 1] == 0).any()


def test_random_cases_have_every_class_and_thousands_of_candidates():
    for which, lo in (("384x640", 1089), ("544x960", 1089), ("1x1", 0)):
        case = T.case_random(which)
        dets, _, cnt = T.detector_expected(case, 0)
        assert cnt > lo and len(dets) >= 1
        if lo:
            assert set(dets[:, 5].astype(int)) == {0, 1, 2, 3, 4} and len(dets) == 300


# ---- heat maps ------------------------------------------------------------------------------------------------------
def test_heat_patterns_tie_where_they_say():
    from oracle import prims as P
    h, w = T.HEAT_SIZES["135x240"]
    lg = T.heat_logits(h, w)
    assert np.isfinite(lg).all()
    sig = P.sigmoid(lg[0]).reshape(-1, 64)
    assert P.sigmoid(np.float32([T.HI]))[0] == np.float32(1.0)
    per = (h * w + 63) // 64
    pat = T.heat_patterns(h, w)
    for c, (name, pix) in pat.items():
        ones = np.nonzero(sig[:, c] == np.float32(1.0))[0]
        assert sorted(set(pix)) == list(ones), name
    two = pat[0][1]
    assert two[0] // per == 0 and two[1] // per == 1 and (two[0] + 1) % per == 0          # spans two chunks; its first pixel is the last of chunk 0
    wave = [(p - p // per * per) & 3 for p in pat[1][1]]                                  # the wave of heat_argmax_kernel that reads the pixel
    assert sorted(wave) == [0, 1, 2, 3] and wave[0] != 0
    assert len(pat[2][1]) == h * w and not pat[3][1]
    assert pat[4][1][0] & 3 == 3 and pat[4][1][1] & 3 == 0
    for c in (5, 6, 9):
        (y0, x0), (y1, x1) = (divmod(p, w) for p in pat[c][1])
        assert (y0 // 8, x0 // 32) != (y1 // 8, x1 // 32), pat[c][0]
    (y0, x0), (y1, x1) = (divmod(p, w) for p in pat[9][1])
    assert y0 < y1 and x0 // 32 > x1 // 32, "the first maximum lies in the LATER tile of its tile row order"
    assert pat[8][1][0] // per != pat[8][1][1] // per
    idx, score = P.heatmap_argmax(lg[0], 57)
    assert idx[2] == 0 and idx[3] == 0 and idx[0] == per - 1 and idx[4] == 7 and idx[7] == h * w - 1
    assert (score[11:] == 1.0).all() and len({int(i) for i in idx[11:]}) > 40
    assert (lg[1, ..., 11:57].reshape(-1, 46).max(0) < T.HI).all(), "frame 1: unique maxima"
    assert 5 * 9 < 64, "a map with fewer pixels than chunks"


def test_fused_cases_are_exact_and_saturate():
    from oracle import prims as P
    from eagle_amd import lib
    for hw in ((135, 240), (7, 65)):
        x, w, b, logits = T.fused_case_1x1(*hw)
        assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 128, "small integers: exact in fp16 and in the split format"
        assert set(np.unique(w)) <= {0.0, 0.5, 1.0}
        ref = P.conv2d(x, w, b)
        assert np.array_equal(ref, logits)
        sig = P.sigmoid(logits[0]).reshape(-1, 57)
        assert ((sig == 1.0).sum(0)[[0, 1, 16, 17, 32, 33]] >= 2).all(), "plateaus of exactly 1.0 in every weight / bias group"
        for prec in (lib.PREC_F16, lib.PREC_F32S):
            tiles, th, tw = lib.conv2d_argmax_tiles(hw, 16, 57, 1, 1, prec)
            assert (th, tw) == (8, 32), "heat_patterns places its tile-spanning plateaus for this tile"
            assert tiles == -(-hw[0] // th) * -(-hw[1] // tw)
    assert 135 % 8 and 240 % 32 and 65 % 32, "partial tiles in y and in x"


# ---- post stage -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def post():
    cases = T.post_cases()
    return cases, {k: T.post_expected(c) for k, c in cases.items()}


def test_post_cases_use_ransac_alone(post):
    cases, exp = post
    for k, e in exp.items():
        assert np.isfinite(cases[k]["score"]).all()
        assert e["n_plane"] < 4 or e["H"] is not None, f"{k}: cv2.RANSAC's restatement fails: the reference would fall back to RHO / LMEDS, which the GPU does not run"


def test_dedup_and_threshold_cases(post):
    from eagle_amd.pitch import INTERSECTION_TO_PITCH_POINTS as NAME
    cases, exp = post
    d = exp["dedup_different_scores"]["detected"]
    assert NAME[42] in d and NAME[14] not in d and NAME[15] in d and NAME[43] not in d
    assert cases["dedup_different_scores"]["idx"][42] == cases["dedup_different_scores"]["idx"][14], "two channels on one pixel"
    d = exp["dedup_equal_scores"]["detected"]
    keys = list(d)
    assert NAME[42] in d and NAME[14] not in d and NAME[40] in d and NAME[4] not in d
    assert keys.index(NAME[40]) == 0 and keys.index(NAME[42]) < keys.index(NAME[15]), "the later label sits in the earlier label's slot"
    d = exp["score_at_keypoint_conf"]["detected"]
    assert NAME[38] in d and NAME[39] not in d and cases["score_at_keypoint_conf"]["score"][38] == 0.5 > cases["score_at_keypoint_conf"]["score"][39]
    d = exp["score_just_above_0_01"]["detected"]
    c = cases["score_just_above_0_01"]
    assert NAME[38] in d and NAME[39] not in d and float(c["score"][39]) < 0.01 < float(c["score"][38]) and c["score"][39] == np.float32(0.01)
    d = exp["last_row_and_column"]["detected"]
    assert d[NAME[42]] == (1280, 720) and d[NAME[43]] == (0, 720) and d[NAME[48]] == (1280, 0)


def test_synthesis_cases(post):
    cases, exp = post
    # The 30-addition cap cannot be reached with this pitch table: a candidate needs two OTHER detected points in its x-group and in its y-group, and only
    # 21 of the 53 on-plane landmarks lie in two groups of three or more.  The cap's branch is therefore dead code for any input; the case below adds as
    # many points as one dict can (every group line that can exist from 14 detections).
    assert T.synthesis_candidate_bound() == 21 < 30
    e = exp["synth_most_candidates"]
    added = [k for k in e["synth"] if k not in e["detected"]]
    assert len(added) == 7 and list(e["synth"])[:14] == list(e["detected"])
    assert exp["synth_one_keypoint"]["synth"] == exp["synth_one_keypoint"]["detected"] and len(exp["synth_one_keypoint"]["detected"]) == 1
    assert not exp["synth_no_keypoint"]["detected"]
    e = exp["synth_two_point_line"]
    assert len(e["detected"]) == 3 and e["synth"] == e["detected"] and e["H"] is None
    from oracle import host
    e = exp["synth_parallel_lines"]
    from eagle_amd.pitch import INTERSECTION_TO_PITCH_POINTS as NAME
    l1 = host.fit_line(np.float32([e["detected"][NAME[38]], e["detected"][NAME[39]]]))
    l2 = host.fit_line(np.float32([e["detected"][NAME[40]], e["detected"][NAME[41]]]))
    assert host.intersect_lines(l1, l2) is None and NAME[42] not in e["synth"], "parallel lines: no centre mark"
    assert len(e["synth"]) > len(e["detected"])


def test_bounds_and_projection_cases(post):
    cases, exp = post
    e = exp["bounds_none_axis_camera"]
    assert e["H"] is not None and e["bounds"] == [None] * 4, "the exception path: no bounds"
    e = exp["bounds_and_pitch_limits"]
    assert e["H"] is not None and None not in e["bounds"]
    p = e["pitch"]
    assert any(tx == 105 and inb for _, _, tx, ty, inb in p) and any(tx == 106 and not inb for _, _, tx, ty, inb in p)
    assert any(ty == 68 and inb for _, _, tx, ty, inb in p) and any(ty == 69 and not inb for _, _, tx, ty, inb in p)
    assert any(-1 < xf < 0 and tx == 0 and inb for xf, _, tx, ty, inb in p) and any(-1 < yf < 0 and ty == 0 and inb for _, yf, tx, ty, inb in p)
    assert any(xf <= -1 and not inb for xf, _, tx, ty, inb in p)


# ---- the anchor limit ---------------------------------------------------------------------------------------------------
def test_resolve_config_refuses_more_anchors_than_nms_sorts():
    from eagle_amd import lib
    with pytest.raises(lib.EagleError, match=r"18900.*16384"):
        lib.resolve_config(lib.default_config(letterbox="square", det_imgsz=960, frame_h=1080, frame_w=1920))
    with pytest.raises(lib.EagleError, match=r"18900.*16384"):
        lib.resolve_config(lib.default_config(letterbox="square", det_imgsz=960))
    for kw in (dict(letterbox="rect", det_imgsz=960), dict(letterbox="square", det_imgsz=640), dict(letterbox="rect", det_imgsz=960, frame_h=1080, frame_w=1920)):
        cfg = lib.resolve_config(lib.default_config(**kw))
        assert cfg.det_precision == lib.PREC_F32 + 1
