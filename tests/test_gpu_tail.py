"""The kernels behind the two networks on constructed inputs (tests/tail_cases.py; what each case forces is asserted in tests/test_tail_cases_cpu.py):
yolo_decode_kernel + nms_kernel (csrc/detect.hip), heat_argmax_kernel (csrc/elementwise.hip), the fused arg-max epilogue of the head convolution
(csrc/conv_kernels.inc) and the reduction, decode, dedup, synthesis, bounds and projection of post_kernel (csrc/geom.hip), through the operator entries
eagle_op_detect_tail / eagle_op_post / eagle_op_conv2d_argmax.  The oracle's plain functions are the reference and EVERY comparison is exact: integers and
flags with array_equal, floats bit for bit.  Each case runs once."""
import numpy as np
import pytest

import tail_cases as T

pytestmark = pytest.mark.gpu

DET_CASES = T.detector_cases()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_f32(a, b):
    return np.array_equal(bits(a), bits(b))


def expected_det_fields(dets, frame_h, frame_w, detector_conf):
    """id / reported / integer box / foot point of every kept detection (cm.py:598-627 as include/eagle.h records it)"""
    out = []
    balls = 0
    for k in range(len(dets)):
        c = int(dets[k, 5])
        x1, y1, x2, y2 = (int(v) for v in dets[k, :4].astype(int))
        ok = not (float(dets[k, 4]) < detector_conf)
        ident, rep = -1, 0
        if c in (0, 1):
            x1 = min(max(x1, 0), frame_w - 1); x2 = min(max(x2, 0), frame_w - 1)
            y1 = min(max(y1, 0), frame_h - 1); y2 = min(max(y2, 0), frame_h - 1)
            ident, rep = k, int(ok)
        elif c == 2:
            ident, rep = balls, int(ok)
            balls += 1
        out.append((ident, rep, x1, y1, x2, y2, int((x1 + x2) / 2), y2))
    return np.array(out, np.int64).reshape(-1, 8)


@pytest.mark.parametrize("name", list(DET_CASES))
def test_detector_tail(name):
    from eagle_amd import lib, records
    from oracle import host
    case = DET_CASES[name]
    recs, boxes, conf, cls = lib.op_detect_tail(case["levels"], case["nc"], case["in_hw"], case["frame_hw"], conf_floor=float(case["conf_floor"]),
                                                nms_iou=float(case["nms_iou"]), detector_conf=case["detector_conf"])
    fh, fw = case["frame_hw"]
    for f in range(len(recs)):
        rows = T.detector_rows(case, f)
        eb, ec, ek = T.decode_scratch(rows)
        assert same_f32(boxes[f], eb), f"{name} frame {f}: decoded boxes"
        assert same_f32(conf[f], ec) and np.array_equal(cls[f], ek), f"{name} frame {f}: decoded confidence / class"
        dets, objects, cnt = T.detector_expected(case, f)
        rec = recs[f]
        K = int(rec["n_det"])
        print(f"{name} frame {f}: {int(rec['n_candidates'])} candidates (oracle {cnt}), {K} kept (oracle {len(dets)})")
        assert int(rec["n_candidates"]) == cnt and K == len(dets), f"{name} frame {f}"
        d = rec["det"][:K]
        assert same_f32(np.stack([d[k] for k in ("x1", "y1", "x2", "y2", "conf")], 1), dets[:, :5]), f"{name} frame {f}: kept boxes / order"
        assert np.array_equal(d["cls"], dets[:, 5].astype(np.int32))
        want = expected_det_fields(dets, fh, fw, case["detector_conf"])
        got = np.stack([d[k].astype(np.int64) for k in ("id", "reported", "bx1", "by1", "bx2", "by2", "foot_x", "foot_y")], 1).reshape(-1, 8)
        assert np.array_equal(got, want), f"{name} frame {f}: id / reported / integer box / foot point"
        # ... and as the reference dict: what objects_from_detections reports, keyed as it keys it
        ref = records.to_reference_dict(rec)["Coordinates"]
        exp = host.project_objects(objects, None)
        assert {k: v for k, v in ref.items()} == {k: v for k, v in exp.items() if v}, f"{name} frame {f}: object dict"


HEAT = [(s, c) for s in T.HEAT_SIZES for c in T.HEAT_CHUNKS]


@pytest.mark.parametrize("size,chunks", HEAT)
def test_heat_argmax_kernel_and_its_reduction(size, chunks):
    from eagle_amd import lib
    from oracle import prims as P
    h, w = T.HEAT_SIZES[size]
    lg = T.heat_logits(h, w, 2, chunks)
    recs, parts = lib.op_post((h, w), T.FRAME, logits=lg, chunks=chunks)
    for f in range(2):
        es, ei = T.chunk_first_max(P.sigmoid(lg[f]).reshape(-1, 64), chunks)
        assert np.array_equal(parts[f]["idx"], ei), f"frame {f}: partial indices"
        assert same_f32(parts[f]["score"], es), f"frame {f}: partial scores"
        idx, score = P.heatmap_argmax(lg[f], 57)
        assert np.array_equal(recs[f]["hm_idx"], idx) and same_f32(recs[f]["hm_score"], score), f"frame {f}: reduced maxima"


FUSED = [("1x1_135x240", "f16"), ("1x1_135x240", "f32s"), ("1x1_7x65", "f16"), ("1x1_7x65", "f32s"), ("3x3_20x33", "f16"), ("3x3_20x33", "f32s")]


@pytest.mark.parametrize("which,prec", FUSED)
def test_fused_argmax_epilogue(which, prec):
    from eagle_amd import lib
    from oracle import prims as P
    exact = None
    if which.startswith("1x1"):
        hw = tuple(int(v) for v in which[4:].split("x"))
        x, w, b, exact = T.fused_case_1x1(*hw)
    else:
        x, w, b = T.fused_case_3x3()
    logits, parts, (th, tw) = lib.op_conv2d_argmax(x, w, b, precision=lib.PRECISIONS[prec])
    n, h, wd, cout = logits.shape
    if exact is not None:
        assert same_f32(logits, exact), "power-of-two weights on small integers: the logits are exact in this family"
    lg64 = np.full((n, h, wd, 64), -30.0, np.float32)
    lg64[..., :cout] = logits
    assert parts.shape == (n, -(-h // th) * -(-wd // tw), 64)
    for f in range(n):
        es, ei = T.tile_first_max(P.sigmoid(logits[f]), th, tw)
        assert np.array_equal(parts[f]["idx"][:, :cout], ei), f"frame {f}: tile partial indices"
        assert same_f32(parts[f]["score"][:, :cout], es), f"frame {f}: tile partial scores"
    idx_score = [P.heatmap_argmax(lg64[f], 57) for f in range(n)]
    recs, _ = lib.op_post((h, wd), T.FRAME, parts=parts)                      # post_kernel's reduction of the tile partials
    recs2, _ = lib.op_post((h, wd), T.FRAME, logits=lg64, chunks=64)          # heat_argmax_kernel on the same logits
    for f in range(n):
        for r, what in ((recs, "tile partials"), (recs2, "unfused")):
            assert np.array_equal(r[f]["hm_idx"], idx_score[f][0]) and same_f32(r[f]["hm_score"], idx_score[f][1]), f"frame {f}: {what}"


def test_post_stage_cases_side_by_side():
    from eagle_amd import lib
    from eagle_amd.pitch import PITCH_POINTS_TO_INTERSECTION as IDX
    cases = T.post_cases()
    names = list(cases)
    n = len(names)
    parts = np.zeros((n, 1, 64), lib.PART_DTYPE)
    parts["score"] = -1.0; parts["idx"] = 0x7fffffff
    recs = np.zeros(n, lib.RESULT_DTYPE)
    for f, k in enumerate(names):
        c = cases[k]
        parts["score"][f, 0, :57] = c["score"]; parts["idx"][f, 0, :57] = c["idx"]
        m = len(c["feet"])
        recs["n_det"][f] = m
        recs["det"]["foot_x"][f, :m] = c["feet"][:, 0]; recs["det"]["foot_y"][f, :m] = c["feet"][:, 1]
    conf = {cases[k]["keypoint_conf"] for k in names}
    out = {}
    for kc in sorted(conf):                                                   # keypoint_conf is a launch parameter: one launch per value, all frames each
        out[kc], _ = lib.op_post(T.HM, T.FRAME, parts=parts, recs=recs, keypoint_conf=kc)
    for f, k in enumerate(names):
        c, e, rec = cases[k], T.post_expected(cases[k]), out[cases[k]["keypoint_conf"]][f]
        assert np.array_equal(rec["hm_idx"], c["idx"]) and same_f32(rec["hm_score"], c["score"]), k
        nk = int(rec["n_kp"])
        kp = rec["kp"][:nk]
        labels = [IDX[lab] for lab in e["synth"]]
        print(f"{k}: {nk} key-points ({len(e['detected'])} detected), H_valid {bool(rec['H_valid'])}, bounds_valid {bool(rec['bounds_valid'])}")
        assert list(kp["label"]) == labels, f"{k}: key-point list / dict order"
        assert [(int(p["x"]), int(p["y"])) for p in kp] == [tuple(v) for v in e["synth"].values()], f"{k}: key-point pixels"
        assert list(kp["synthesized"]) == [int(lab not in e["detected"]) for lab in e["synth"]], f"{k}: synthesised flags"
        assert same_f32(kp["score"], [0.0 if lab not in e["detected"] else c["score"][IDX[lab]] for lab in e["synth"]])
        assert list(kp["on_plane"]) == [int(lab in e["used"]) for lab in e["synth"]], f"{k}: on-plane flags"
        if e["H"] is None:
            assert not rec["H_valid"] and not rec["H"].any(), k
        else:
            assert rec["H_valid"] and np.array_equal(rec["H"].reshape(3, 3), e["H"]), f"{k}: H"
            inl = dict(zip(e["used"], e["mask"].tolist()))
            assert [int(p["inlier"]) for p in kp if p["on_plane"]] == [int(inl[lab]) for lab in e["synth"] if lab in e["used"]], f"{k}: inlier flags"
        if None in e["bounds"]:
            assert not rec["bounds_valid"], k
        else:
            assert rec["bounds_valid"] and np.array_equal(rec["bounds"], np.float64([b[0] for b in e["bounds"]])), f"{k}: bounds"
        m = len(c["feet"])
        d = rec["det"][:m]
        assert int(rec["n_det"]) == m and np.array_equal(d["foot_x"], c["feet"][:, 0]) and np.array_equal(d["foot_y"], c["feet"][:, 1])
        if e["H"] is not None and m:
            p = e["pitch"]
            assert same_f32(d["pitch_xf"], [v[0] for v in p]) and same_f32(d["pitch_yf"], [v[1] for v in p]), f"{k}: projected foot points"
            assert list(d["pitch_x"]) == [v[2] for v in p] and list(d["pitch_y"]) == [v[3] for v in p] and list(d["in_bounds"]) == [int(v[4]) for v in p], f"{k}: pitch limits"
        else:
            assert not d["in_bounds"].any() and not d["pitch_xf"].any()


def test_rect_960_handle_sorts_its_10710_anchors(state_dicts):
    """the largest supported geometry end to end (rect letterbox, det_imgsz 960: 10710 anchors, the NMS sorts 16384 keys): class biases that make EVERY anchor a
    candidate; detections bit-equal to the oracle's.  The square letterbox at 960 (18900 anchors) is refused when the handle is created, not by its first step."""
    from eagle_amd import lib, synth
    from eagle_amd.coordinate_model import CoordinateModel
    from oracle import pipeline
    hs, ys = state_dicts
    ys = dict(ys)
    for l in range(3):
        ys[f"model.22.cv3.{l}.2.bias"] = np.full_like(ys[f"model.22.cv3.{l}.2.bias"], 8.0)
    with pytest.raises(lib.EagleError, match=r"18900.*16384"):
        CoordinateModel(precision="f32", batch=1, det_imgsz=960, letterbox="square", hrnet_state_dict=hs, detector_state_dict=ys)
    frame = synth.frame(0, 3)
    cm = CoordinateModel(precision="f32", batch=1, det_imgsz=960, hrnet_state_dict=hs, detector_state_dict=ys)
    rec = cm.process_records(frame[None])[0]
    cm.handle.close()
    ora = pipeline.OracleModel(hs, ys, imgsz=960, backend="c")
    objects, dets, rows = ora.detect_objects(frame)
    cnt = int((rows[:, 4:].max(1) > np.float32(0.15)).sum())
    print(f"rect/960: {len(rows)} anchors, {cnt} candidates, {len(dets)} kept")
    assert len(rows) == 10710 == cnt, "every anchor is a candidate"
    n = int(rec["n_det"])
    assert int(rec["n_candidates"]) == cnt and n == len(dets)
    assert same_f32(np.stack([rec["det"][k][:n] for k in ("x1", "y1", "x2", "y2", "conf")], 1), dets[:, :5])
    assert np.array_equal(rec["det"]["cls"][:n], dets[:, 5].astype(np.int32))
