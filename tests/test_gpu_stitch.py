"""The library's id merge (include/eagle.h, EaglePostParams.merge_ids; csrc/post.hip) against tests/stitch_ref.py, bit for bit, on the constructed
clips of tests/stitch_cases.py and the randomly fragmented ones, both ``smooth`` values: rows, column names and order, the NaN pattern and the
values' bits; the merge report; the inherited teams; the overlay and the velocities of a merged column; the refusal of other switch values; the
switch off; the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import control_ref
import post_cases
import post_ref
import stitch_cases
import stitch_ref
from eagle_amd import lib, postprocess, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _same(t, exp):
    assert list(t.rows) == exp["rows"] and t.names == exp["columns"] and t.flags == exp["flags"]
    got = np.ascontiguousarray(t.values)
    assert got.shape == exp["values"].shape and np.array_equal(np.isnan(got), np.isnan(exp["values"]))
    ok = ~np.isnan(got)
    assert np.array_equal(got.view(np.uint64)[ok], exp["values"].view(np.uint64)[ok])


def _same_merges(got, exp):
    assert [{k: v for k, v in m.items() if k != "dist"} for m in got] == [{k: v for k, v in m.items() if k != "dist"} for m in exp]
    assert np.array_equal(np.array([m["dist"] for m in got], np.float64).view(np.uint64), np.array([m["dist"] for m in exp], np.float64).view(np.uint64))


def _check(handle, case, smooth):
    recs = post_cases.records_of(case)
    exp = stitch_ref.process_data(post_cases.coords_of(case, recs), case["team_mapping"], smooth=smooth, fps=case["fps"], merge_ids=True)
    t = postprocess.process_data(handle, recs, case["fps"], case["frame_w"], case["team_mapping"], smooth=smooth, merge_ids=True)
    try:
        _same(t, exp)
        _same_merges(t.merges, exp["merges"])
        assert t.team_mapping == exp["team_mapping"]
    finally:
        t.close()
    return exp


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("name", [c["name"] for c in stitch_cases.CASES])
def test_constructed_cases(handle, name, smooth):
    case = stitch_cases.BY_NAME[name]
    exp = _check(handle, case, smooth)
    assert [(m["from_id"], m["to_id"]) for m in exp["merges"]] == case["links"]


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("name", ["would_merge_same_team", "would_merge_unknown_team", "goalkeeper_fold", "goalkeeper_fold_overlap", "frames_dropped", "rare_id_dropped"])
def test_post_cases_with_the_switch(handle, name, smooth):
    _check(handle, post_cases.BY_NAME[name], smooth)


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("param", stitch_cases.FRAGMENTED, ids=lambda p: "x".join(map(str, p[1:])))
def test_fragmented_clips(handle, param, smooth):
    case, _, _ = stitch_cases.fragmented(*param)
    exp = _check(handle, case, smooth)
    assert len(exp["merges"]) == param[2] * (param[3] - 1) and len(exp["columns"]) == 6 + 2 * (param[2] + 1)


def test_overlay_of_a_merged_row_carries_the_head(handle):
    case = stitch_cases.BY_NAME["teams_head_inherits"]                # 5 (no team) -> 9 (team 1): Player_5 is drawn, in team 1's blue, on 9's rows too
    recs = post_cases.records_of(case)
    exp = stitch_ref.process_data(post_cases.coords_of(case, recs), case["team_mapping"], fps=case["fps"], merge_ids=True)
    with_switch = postprocess.process_data(handle, recs, case["fps"], case["frame_w"], case["team_mapping"], merge_ids=True)
    without = postprocess.process_data(handle, recs, case["fps"], case["frame_w"], case["team_mapping"])
    try:
        for r in range(len(exp["rows"])):
            got = [(int(q["kind"]), *map(int, q["a"]), (int(q["b"]), int(q["g"]), int(q["r"]))) for q in with_switch.overlay(r)]
            assert got == post_ref.overlay_of_row(exp, r)
            labels = [(q[3], q[7]) for q in got if q[0] == lib.PRIM_LABEL]
            assert labels == [(5, (255, 0, 0))]                       # (the anchor has no team: skipped)
            plain = [int(q["a"][2]) for q in without.overlay(r) if q["kind"] == lib.PRIM_LABEL]
            assert plain == ([9] if r >= 5 else [])                   # without the switch id 5 has no team and is not drawn at all
    finally:
        with_switch.close()
        without.close()


def test_velocities_run_across_the_seam(handle):
    case = stitch_cases.BY_NAME["seam_64_256"]                        # steady (2, 1) px per frame under three ids
    recs = post_cases.records_of(case)
    t = postprocess.process_data(handle, recs, case["fps"], case["frame_w"], None, merge_ids=True)
    off = postprocess.process_data(handle, recs, case["fps"], case["frame_w"], None)
    try:
        v = handle.velocities(t, case["fps"])
        exp = control_ref.velocities(np.ascontiguousarray(t.values), np.asarray(t.rows), case["fps"])
        assert np.array_equal(np.isnan(v), np.isnan(exp)) and np.array_equal(v[~np.isnan(v)], exp[~np.isnan(exp)])
        c = t.names.index("Player_300_video")
        assert not np.isnan(v[c]).any() and np.all(v[c] == v[c][100])                       # one speed over all 300 rows, the seams included
        vo = handle.velocities(off, case["fps"])
        co = off.names.index("Player_301_video")
        assert np.isnan(vo[co][63]).all() and not np.isnan(vo[co][64]).any() and len(off.names) == len(t.names) + 4
    finally:
        t.close()
        off.close()


def test_other_switch_values_are_refused(handle):
    case = stitch_cases.BY_NAME["hand_over"]
    recs = post_cases.records_of(case)
    for bad in (2, -1):
        with pytest.raises(lib.EagleError, match="merge_ids"):
            handle.postprocess(recs, 25, 1280, {}, merge_ids=bad)
    p = lib.EaglePostParams(fps=25, frame_w=1280, smooth=0, filter_ball=0, team_ids=None, team_vals=None, n_team=0, reserved=2, max_bytes=0)
    out = C.c_void_p()
    assert handle.L.eagle_postprocess(handle._h, recs.ctypes.data_as(C.c_void_p), len(recs), C.byref(p), C.byref(out)) == lib.E_INVALID and not out.value
    assert "merge_ids = 2" in handle.L.eagle_last_error(handle._h).decode()
    t = postprocess.process_data(handle, recs, 25, 1280, {}, merge_ids=True)                # the handle still works
    assert [(m["from_id"], m["to_id"]) for m in t.merges] == [(5, 9)]
    t.close()


@pytest.mark.parametrize("smooth", [False, True])
def test_switch_off(handle, smooth):
    for case in post_cases.CASES + [stitch_cases.BY_NAME[n] for n in ("hand_over", "chain_65", "goalkeeper_chain_with_fold", "seam_257")]:
        recs = post_cases.records_of(case)
        exp = post_ref.process_data(post_cases.coords_of(case, recs), case["team_mapping"], smooth=smooth)
        a = postprocess.process_data(handle, recs, case["fps"], case["frame_w"], case["team_mapping"], smooth=smooth, merge_ids=False)
        b = handle.postprocess(recs, case["fps"], case["frame_w"], case["team_mapping"], smooth=smooth)       # a call without the keyword
        try:
            _same(a, exp)
            _same(b, exp)
            assert a.merges == [] and b.merges == [] and a.team_mapping == case["team_mapping"]
            n = C.c_int(-1)
            assert handle.L.eagle_post_merges(a._t, None, 0, C.byref(n)) == 0 and n.value == 0
        finally:
            a.close()
            b.close()


def test_cli_merge_ids(tmp_path, monkeypatch):
    """--processed --merge-ids on a synthetic clip writes "merges"; with the detections of a constructed clip in place of the random networks' (the
    model's records and the team mapping are substituted, everything behind them is the command line's own path) the joins reach metadata.json."""
    from eagle_amd import cli, records
    from eagle_amd.coordinate_model import CoordinateModel
    from eagle_amd.processor import Processor
    out = str(tmp_path / "merged")
    common = ["--fps", "25", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out]
    assert cli.main(common + ["--frames", "6", "--processed", "--merge-ids"]) == 0
    meta = json.load(open(os.path.join(out, "metadata.json")))
    assert isinstance(meta["merges"], list) and isinstance(meta["team_mapping"], dict)
    with pytest.raises(SystemExit):
        cli.main(common + ["--frames", "6", "--merge-ids"])           # only with --processed

    case = stitch_cases.BY_NAME["chain_3"]                            # one person under the ids 200, 237, 274 on 9 frames, inside the picture
    recs = post_cases.records_of(case)

    def get_coordinates(self, frames, fps, **kw):
        coords = {i: records.to_reference_dict(r, i, fps) for i, r in enumerate(recs)}
        self._last = (coords, recs, np.ones(len(recs), bool))
        return coords

    monkeypatch.setattr(CoordinateModel, "get_coordinates", get_coordinates)
    monkeypatch.setattr(Processor, "get_team_mapping", lambda self, frames, coords, pixel_format="bgr": {237: 1})
    assert cli.main(common + ["--frames", "9", "--processed", "--merge-ids", "--kinematics"]) == 0
    meta = json.load(open(os.path.join(out, "metadata.json")))
    assert [(m["kind"], m["from_id"], m["to_id"], m["head_id"], m["gap_frames"], m["team"]) for m in meta["merges"]] == [(0, 200, 237, 200, 1, 1), (0, 237, 274, 200, 1, 1)]
    assert all(sorted(m) == sorted(lib.POSTMERGE_DTYPE.names) and m["dist"] == float(np.sqrt(np.float64(10.0))) for m in meta["merges"])
    assert meta["team_mapping"] == {"237": 1, "200": 1}                # the head inherited its chain's team
    proc = json.load(open(os.path.join(out, "processed_data.json")))
    assert len(proc) == 9 and all([it["ID"] for it in row["Coordinates_video"]] == [200, "Ball"] for row in proc)
    kin = json.load(open(os.path.join(out, "kinematics.json")))["players"]
    assert [(p["id"], p["type"]) for p in kin] == [(200, "Player")] and kin[0]["distance"] > 0       # one person, followed over all three ids
