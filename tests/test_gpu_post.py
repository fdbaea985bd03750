"""The library's clip post-processor (include/eagle.h eagle_postprocess; csrc/post.hip) against tests/post_ref.py, bit for bit: the constructed
clips of tests/post_cases.py (whose reference results are tests/golden/post_golden.json), seeded random tables at the wave and block seams of the
scans, both ``smooth`` values; the JSON products, the overlay of a processed row and the picture drawn from it; the refusals; no side effect on
the handle; the command line."""
import json
import os

import numpy as np
import pytest

import annot_ref as A
import post_cases
import post_ref
from eagle_amd import lib, postprocess, synth, weights
from test_post_cpu import GOLDEN, DIVERGES, golden_format, golden_values, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _ref(case, recs, smooth):
    return post_ref.process_data(post_cases.coords_of(case, recs), case["team_mapping"], smooth=smooth)


def _check(handle, case, smooth, recs=None):
    recs = post_cases.records_of(case) if recs is None else recs
    exp = _ref(case, recs, smooth)
    t = postprocess.process_data(handle, recs, case["fps"], case["frame_w"], case["team_mapping"], smooth=smooth)
    try:
        assert list(t.rows) == exp["rows"] and t.names == exp["columns"] and t.flags == exp["flags"]
        got = np.ascontiguousarray(t.values)
        assert got.shape == exp["values"].shape
        assert np.array_equal(np.isnan(got), np.isnan(exp["values"]))
        ok = ~np.isnan(got)
        assert np.array_equal(got.view(np.uint64)[ok], exp["values"].view(np.uint64)[ok])
        return t, exp
    except BaseException:
        t.close()
        raise


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("name", [c["name"] for c in post_cases.CASES])
def test_golden_cases(handle, name, smooth):
    case = post_cases.BY_NAME[name]
    t, exp = _check(handle, case, smooth)
    try:
        rows, fmt = postprocess.raw_data_rows(t), postprocess.format_data(t)
        assert json.dumps(rows) == json.dumps(post_ref.raw_data_rows(exp)) and json.dumps(fmt) == json.dumps(post_ref.format_data(exp))
        g = GOLDEN[name][f"smooth{int(smooth)}"]
        if name not in DIVERGES:                        # ... and directly against what the reference returned
            assert t.names == g["columns"] and list(t.rows) == g["rows"] and same_bits(t.values, golden_values(g))
            assert [json.dumps(r) for r in fmt] == [json.dumps(r) for r in golden_format(g)]
            assert [list(r) for r in rows] == [g["columns"]] * len(g["rows"])
        json.dumps(postprocess.json_rows(fmt), allow_nan=False)
    finally:
        t.close()


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("rows,cols,occ", [(1, 1, 1.0), (2, 3, 0.5), (63, 7, 0.3), (64, 12, 0.6), (65, 40, 0.2), (255, 5, 0.5), (256, 9, 0.0), (257, 17, 1.0),
                                           (1025, 11, 0.35)])
def test_random_tables(handle, rows, cols, occ, smooth):
    case = post_cases.random_records(rows * 1000 + cols, rows, cols, occ)
    t, exp = _check(handle, case, smooth)
    t.close()
    assert len(exp["rows"]) == rows and len(exp["columns"]) >= 8


def test_overlay_and_annotate_from_table(handle, state_dicts):
    from eagle_amd.processor import Processor
    p = Processor(batch=2, hrnet_state_dict=state_dicts[0], detector_state_dict=state_dicts[1])
    try:
        P, G, person, ball = post_cases.P, post_cases.G, post_cases.person, post_cases.ball
        fr = [post_cases.frame([person(P, 3, 100 + 9 * t, 400 + t), person(P, 7, 900 - 5 * t, 300)] + ([person(P if t < 3 else G, 9, 600 + 4 * t, 650 - t)] if t != 4 else []),
                               [ball(640 + 11 * t, 200 + 7 * t)] if t in (0, 1, 5) else []) for t in range(6)]
        fr[1]["persons"] = []                           # frame 1 keeps its ball only: not a kept row
        case = post_cases._case("overlay", fr, team_mapping={3: 1, 9: 0})      # (id 7 has no team: not drawn)
        recs, tm = post_cases.records_of(case), case["team_mapping"]
        frames = synth.clip(0, 4)
        real = p.model.process_records(frames[:1])[0]   # the key-points of a real record on every frame
        for r in recs:
            r["n_kp"], r["kp"] = real["n_kp"], real["kp"]
            r["kp"]["on_plane"], r["kp"]["inlier"] = 1, 1
        frames6 = np.concatenate([frames, frames[:2]])
        t = postprocess.process_data(p.model.handle, recs, 25, 1280, tm)
        exp = post_ref.process_data(post_cases.coords_of(case, recs), tm)
        assert list(t.rows) == exp["rows"] == [0, 2, 3, 4, 5] and t.names == exp["columns"]
        lists = []
        for r, f in enumerate(t.rows):
            want = post_ref.overlay_of_row(exp, r, recs[f])
            got = [(int(q["kind"]), *map(int, q["a"]), (int(q["b"]), int(q["g"]), int(q["r"]))) for q in t.overlay(r, recs[f])]
            assert got == want and any(q[0] == A.TRI for q in got) and any(q[0] == A.DISC for q in got) == (int(real["n_kp"]) > 0)
            lists.append(want)
        assert any(q[0] == A.LABEL and q[3] == 9 and q[7] == (0, 255, 0) for q in lists[0])        # Player_9 of frame 0 is drawn as goalkeeper 9
        assert not any(q[0] == A.LABEL and q[3] == 7 for lst in lists for q in lst) and any(q[0] == A.LABEL and q[3] == 9 for q in lists[3])      # row 3 = frame 4: interpolated
        for fmt in ("bgr", "i420"):
            out = p.annotate(frames6, recs, out_format=fmt, table=t)
            assert np.array_equal(out, A.annotate_dense(frames6[np.asarray(t.rows)], lists, fmt))
        t.close()
    finally:
        p.model.handle.close()


def test_refusals(handle):
    case = post_cases.BY_NAME["ball_two_sightings"]
    recs = post_cases.records_of(case)
    L, h = handle.L, handle._h
    import ctypes as C

    def call(recs_p, n, params, out=True):
        t = C.c_void_p()
        rc = L.eagle_postprocess(h, recs_p, n, None if params is None else C.byref(params), C.byref(t) if out else None)
        assert not t.value
        return rc, L.eagle_last_error(h).decode()

    rp = recs.ctypes.data_as(C.c_void_p)
    good = dict(fps=25, frame_w=1280, smooth=0, filter_ball=0, team_ids=None, team_vals=None, n_team=0, reserved=0, max_bytes=0)
    rc, msg = call(rp, len(recs), lib.EaglePostParams(**dict(good, filter_ball=1)))
    assert rc == lib.E_INVALID and "filter_ball" in msg
    for bad in (dict(fps=0), dict(frame_w=0), dict(n_team=-1), dict(max_bytes=-1)):
        assert call(rp, len(recs), lib.EaglePostParams(**dict(good, **bad)))[0] == lib.E_INVALID
    assert call(rp, -1, lib.EaglePostParams(**good))[0] == lib.E_INVALID
    assert call(None, 3, lib.EaglePostParams(**good))[0] == lib.E_INVALID
    assert call(rp, len(recs), None)[0] == lib.E_INVALID
    assert call(rp, len(recs), lib.EaglePostParams(**good), out=False)[0] == lib.E_INVALID
    rc, msg = call(rp, len(recs), lib.EaglePostParams(**dict(good, max_bytes=1024)))      # 10 rows x 10 raw columns x 16 bytes do not fit 1 KiB
    assert rc == lib.E_INVALID and "10 rows" in msg and "1024" in msg
    with pytest.raises(NotImplementedError):
        postprocess.process_data(handle, recs, 25, 1280, {}, filter_ball_detections=True)
    t = postprocess.process_data(handle, recs, 25, 1280, {})                               # the handle still works
    assert len(t.rows) == 10
    with pytest.raises(lib.EagleError):
        t.overlay(10)
    t.close()


def test_no_side_effect_on_the_handle(handle):
    frames = synth.clip(0, 2)
    before = handle.process(frames).copy()
    captures = handle.timings().graph_captures
    for smooth in (False, True):
        postprocess.process_data(handle, post_cases.records_of(post_cases.BY_NAME["appear_vanish_return"]), 25, 1280, {3: 0}, smooth=smooth).close()
    postprocess.process_data(handle, before, 25, 1280, None).close()                       # the handle's own records as input: read only
    after = handle.process(frames)
    assert all(np.array_equal(before[k], after[k]) for k in lib.RESULT_DTYPE.names)        # (field by field: the struct's tail padding is not data)
    assert handle.timings().graph_captures == captures


def test_cli_processed(tmp_path):
    from eagle_amd import cli
    out_a, out_b = str(tmp_path / "with"), str(tmp_path / "without")
    common = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3"]
    assert cli.main(common + ["--out", out_a, "--processed", "--annotated"]) == 0
    assert cli.main(common + ["--out", out_b]) == 0
    assert sorted(os.listdir(out_a)) == ["annotated.y4m", "metadata.json", "processed_data.json", "raw_coordinates.json", "raw_data.json"]
    assert sorted(os.listdir(out_b)) == ["metadata.json", "raw_coordinates.json"]
    meta_a, meta_b = json.load(open(os.path.join(out_a, "metadata.json"))), json.load(open(os.path.join(out_b, "metadata.json")))
    assert isinstance(meta_a["team_mapping"], dict) and meta_a["fps"] == 5
    assert sorted(meta_b) == ["fps", "frames", "note", "seconds"] and meta_b["note"] == "team_mapping needs the post-processor (out of scope)"
    raw, proc = json.load(open(os.path.join(out_a, "raw_data.json"))), json.load(open(os.path.join(out_a, "processed_data.json")))
    assert isinstance(raw, list) and len(raw) == len(proc)
    for r, q in zip(raw, proc):
        assert list(r)[:4] == list(post_ref.BOUNDARIES) and list(r)[-2:] == ["Ball", "Ball_video"]
        assert list(q) == ["Boundaries", "Coordinates", "Coordinates_video"] and len(q["Boundaries"]) == 4
        assert q["Coordinates"][-1]["ID"] == "Ball" and q["Coordinates_video"][-1]["ID"] == "Ball"
        assert all(sorted(it) == ["Coordinates", "ID", "Type"] for it in q["Coordinates"][:-1] + q["Coordinates_video"][:-1])
