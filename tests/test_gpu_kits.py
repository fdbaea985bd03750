"""The team clustering on the GPU (include/eagle.h, eagle_op_team_cluster / eagle_op_team_cluster_ids / eagle_team_cluster; csrc/kits.hip): every field of
every output equals the contract of tests/kits_ref.py — tobytes(), no tolerance — for the constructed cases of tests/kits_cases.py; two runs give
identical bytes; NULL outputs in every combination; every refusal leaves poisoned outputs alone; through a handle on an uploaded clip eagle_team_cluster
equals the operator entry; Processor.get_team_mapping(method="colours") is today's result on the golden team clip and method="cluster" splits the clip of
two blues that the colours method puts into one team; Processor.process_data(team_method="cluster"); the command line's teams.json equals kits.to_json
of the contract, and without the flag it writes what it wrote before."""
import ctypes as C
import itertools
import json
import os
import types

import numpy as np
import pytest

import kits_cases as KC
import kits_ref as KR
import team_cases
from eagle_amd import kits, lib, teams

pytestmark = pytest.mark.gpu

vp = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def _equal(got, exp, what):
    assert len(got) == len(exp)
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, a.shape, b.shape)
        for k in a.dtype.names:
            assert np.array_equal(a[k], b[k]), (what, k)
        assert a.tobytes() == b.tobytes(), what


def _op(c):
    if c["kind"] == "ids":
        return lib.op_team_cluster_ids(c["sums"], c["used"], lib.kit_params(**c["p"]))
    return lib.op_team_cluster(c["frames"], c["crops"], c["slots"], c["n_ids"], lib.kit_params(**c["p"]))


@pytest.mark.parametrize("name", [c["name"] for c in KC.CASES])
def test_op_team_cluster_equals_contract(name):
    _equal(_op(KC.BY_NAME[name]), KC.reference(name), name)


def test_two_runs_give_identical_bytes():
    for name in ("crops_1000", "two_blues_and_a_yellow_referee", "ids_257", "two_pairs_of_equal_cost"):
        _equal(_op(KC.BY_NAME[name]), _op(KC.BY_NAME[name]), "second run of " + name)


def _poisoned(n_crops, n_ids):
    cr, ids, model = np.zeros(max(n_crops, 1), lib.KIT_CROP_DTYPE), np.zeros(max(n_ids, 1), lib.KIT_ID_DTYPE), np.zeros(1, lib.KIT_MODEL_DTYPE)
    cr["n"], ids["skipped"], model["reserved"] = 77, 66, 55
    return cr, ids, model


UNTOUCHED = (lambda cr: (cr["n"] == 77).all() and not cr["units"].any() and not cr["flags"].any(), lambda ids: (ids["skipped"] == 66).all() and not ids["p"].any() and not ids["team"].any(),
             lambda m: (m["reserved"] == 55).all() and not m["voters"].any() and not m["a"].any() and not m["flags"].any())


def test_null_outputs_in_every_combination():
    L = lib.load()
    c = KC.BY_NAME["two_blues_with_weak_ids"]
    exp = KC.reference(c["name"])
    p = lib.kit_params(**c["p"])
    n, fh, fw = c["frames"].shape[:3]
    for want in itertools.product((False, True), repeat=3):
        out = _poisoned(len(c["crops"]), c["n_ids"])
        ptr = [vp(a) if w else None for a, w in zip(out, want)]
        assert L.eagle_op_team_cluster(0, vp(c["frames"]), n, fh, fw, vp(c["crops"]), vp(c["slots"]), len(c["crops"]), c["n_ids"], C.byref(p), *ptr, None) == 0, want
        for a, b, w, alone in zip(out, exp, want, UNTOUCHED):
            assert a.tobytes() == b.tobytes() if w else alone(a), want
    c = KC.BY_NAME["ids_65"]
    exp = KC.reference(c["name"])
    p = lib.kit_params(**c["p"])
    for want in itertools.product((False, True), repeat=2):
        out = _poisoned(0, len(c["used"]))[1:]
        ptr = [vp(a) if w else None for a, w in zip(out, want)]
        assert L.eagle_op_team_cluster_ids(0, vp(c["sums"]), vp(c["used"]), len(c["used"]), C.byref(p), *ptr, None) == 0, want
        for a, b, w, alone in zip(out, exp, want, UNTOUCHED[1:]):
            assert a.tobytes() == b.tobytes() if w else alone(a), want
    ids, model, ms = lib.op_team_cluster_ids(c["sums"], c["used"], p, times=True)
    assert ms[0] == 0 and ms[1] > 0
    cr, ids, model, ms = lib.op_team_cluster(KC.BY_NAME["crops_5"]["frames"], KC.BY_NAME["crops_5"]["crops"], KC.BY_NAME["crops_5"]["slots"], 3, times=True)
    assert (ms > 0).all()


@pytest.mark.parametrize("what,change", KC.ID_REFUSALS, ids=[w for w, _ in KC.ID_REFUSALS])
def test_refusals_of_the_ids_entry_leave_the_outputs_alone(what, change):
    L = lib.load()
    c = KC.BY_NAME["clusters_of_equal_weight"]
    a = dict(sums=c["sums"].copy(), used=c["used"].copy(), n_ids=2, par=True)
    change = dict(change)
    p = lib.kit_params(**change.pop("p", {}))
    if "reserved" in change:
        p.reserved[change.pop("reserved")] = 1
    if "used0" in change:
        a["used"][0] = min(change["used0"], 2 ** 31 - 1); change.pop("used0")
    if "sum0" in change:
        a["sums"][0, 2] = change.pop("sum0")
    if "used_all" in change:                                                    # each within its bound, their sum one beyond
        a["used"][:] = change.pop("used_all")
    if "zero_row" in change:
        a["sums"][change.pop("zero_row")] = 0
    a.update(change)
    if a["n_ids"] > 2:                                                          # (the arrays hold what the count says)
        a["sums"], a["used"] = np.ones((a["n_ids"], KR.BINS), np.int64), np.full(a["n_ids"], 3, np.int32)
    out = _poisoned(0, 1025)[1:]
    rc = L.eagle_op_team_cluster_ids(0, vp(a["sums"]), vp(a["used"]), a["n_ids"], C.byref(p) if a["par"] else None, vp(out[0]), vp(out[1]), None)
    assert rc == lib.E_INVALID and L.eagle_last_error(None).decode() and all(f(x) for f, x in zip(UNTOUCHED[1:], out)), what
    if what == "crops_in_all_above":
        assert str((1 << 22) + 2) in L.eagle_last_error(None).decode() and str(1 << 22) in L.eagle_last_error(None).decode()
        with pytest.raises(ValueError):
            KR.cluster_ids(a["sums"], a["used"])


@pytest.mark.parametrize("what,change", KC.PIXEL_REFUSALS, ids=[w for w, _ in KC.PIXEL_REFUSALS])
def test_refusals_of_the_pixel_entry_leave_the_outputs_alone(what, change):
    L = lib.load()
    c = KC.BY_NAME["window_all_grass"]
    n, fh, fw = c["frames"].shape[:3]
    a = dict(frames=c["frames"], crops=c["crops"].copy(), slots=c["slots"].copy(), n_crops=2, n_ids=2, par=True, h=fh)
    change = dict(change)
    p = lib.kit_params(**change.pop("p", {}))
    if "slot0" in change:
        a["slots"][0] = change.pop("slot0")
    a.update(change)
    out = _poisoned(2, 1025)
    # (a count of crops beyond the cap is refused before the two crops behind the pointer are looked at)
    rc = L.eagle_op_team_cluster(0, vp(a["frames"]), n, a["h"], fw, vp(a["crops"]), vp(a["slots"]), a["n_crops"], a["n_ids"], C.byref(p) if a["par"] else None,
                                 vp(out[0]), vp(out[1]), vp(out[2]), None)
    assert rc == lib.E_INVALID and L.eagle_last_error(None).decode() and all(f(x) for f, x in zip(UNTOUCHED, out)), what
    if what in ("ids_1025", "crops_above"):
        assert ("1024" if what == "ids_1025" else str(1 << 22)) in L.eagle_last_error(None).decode()


def test_the_unchanged_calls_of_the_refusals_succeed():
    for name in ("clusters_of_equal_weight", "window_all_grass"):
        _equal(_op(KC.BY_NAME[name]), KC.reference(name), name)


# ---- through a handle -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle():
    hd = lib.Handle(batch=1, frame_h=KC.FH, frame_w=KC.FW)
    yield hd
    hd.close()


def _stub_model(hd, recs=None):
    return types.SimpleNamespace(handle=hd, _upload=lambda frames, pixel_format: hd.upload(np.ascontiguousarray(frames)), _records_of=lambda c: recs)


@pytest.mark.parametrize("name", ["two_blues_and_a_yellow_referee", "crops_1000", "crops_leaving_the_frame_or_the_clip", "crops_0", "ids_0_and_no_crops"])
def test_handle_team_cluster_equals_the_operator_entry(handle, name):
    c = KC.BY_NAME[name]
    d = handle.upload(c["frames"])
    try:
        got = handle.team_cluster(d, len(c["frames"]), c["crops"], c["slots"], c["n_ids"], lib.kit_params(**c["p"]))
        _equal(got, _op(c), name)
        _equal(got, KC.reference(name), name)
        out = _poisoned(len(c["crops"]), c["n_ids"])
        p = lib.kit_params(min_crops=0)
        rc = handle.L.eagle_team_cluster(handle._h, d, len(c["frames"]), vp(c["crops"]), vp(c["slots"]), len(c["crops"]), c["n_ids"], C.byref(p), vp(out[0]), vp(out[1]), vp(out[2]))
        assert rc == lib.E_INVALID and b"min_crops" in handle.L.eagle_last_error(handle._h) and all(f(x) for f, x in zip(UNTOUCHED, out))
    finally:
        handle.free(d)


def test_get_team_mapping_colours_is_today_s_and_cluster_splits_the_two_blues(handle):
    from eagle_amd.processor import Processor
    frames, coords = team_cases.make_case()
    big = lib.Handle(batch=1)
    try:
        d = big.upload(np.stack(frames))
        try:
            today = teams.get_team_mapping(big, d, coords, n_frames=len(frames))
        finally:
            big.free(d)
        pr = Processor(_stub_model(big))
        assert pr.get_team_mapping(np.stack(frames), coords) == today == pr.get_team_mapping(np.stack(frames), coords, method="colours") and len(today) >= 2
        with pytest.raises(ValueError):
            pr.get_team_mapping(np.stack(frames), coords, method="colours", outlier=0.5)
        with pytest.raises(ValueError):
            pr.get_team_mapping(np.stack(frames), coords, method="kmeans")
    finally:
        big.close()
    frames, coords, truth = KC.two_blues()
    pr = Processor(_stub_model(handle))
    by_names = pr.get_team_mapping(frames, coords)
    assert set(by_names) == set(truth) and set(by_names.values()) == {0}                     # the reference's rule: both kits are "blue"
    ours = pr.get_team_mapping(frames, coords, method="cluster")
    assert set(ours) == set(truth) and len({(truth[p], ours[p]) for p in truth}) == 2       # the clustering: the two kits, no error
    c = KC.BY_NAME["two_blues"]
    assert ours == KR.mapping_of(KC.reference("two_blues")[1], c["slot_ids"]) and pr.team_report["slot_ids"] == c["slot_ids"]
    _equal((pr.team_report["crops"], pr.team_report["ids"], pr.team_report["model"]), KC.reference("two_blues"), "the report")
    frames, coords, truth = KC.two_blues(True)
    ours = pr.get_team_mapping(frames, coords, method="cluster")
    assert 21 not in ours and len(ours) == 20
    assert pr.get_team_mapping(frames, coords, method="cluster", outlier=0)[21] in (0, 1)


def _records(coords, n, scale=(1, 1)):
    """records whose reported detections are the boxes of ``coords`` (class 0, the id as the tracker's); pitch = picture / scale"""
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["H_valid"], recs["bounds_valid"] = 1, 1
    recs["bounds"] = (0.0, 0.0, 105.0, 105.0)
    for i in range(n):
        players = coords[i]["Coordinates"]["Player"]
        recs[i]["n_det"] = len(players)
        d = recs[i]["det"]
        for j, (pid, it) in enumerate(players.items()):
            x1, y1, x2, y2 = it["BBox"]
            d["reported"][j], d["in_bounds"][j], d["conf"][j], d["cls"][j], d["id"][j] = 1, 1, 0.9, 0, pid
            d["bx1"][j], d["by1"][j], d["bx2"][j], d["by2"][j] = x1, y1, x2, y2
            d["pitch_x"][j], d["pitch_y"][j] = x1 // scale[0], y2 // scale[1]
    return recs


def test_processor_process_data_with_the_cluster_method(handle):
    from eagle_amd.processor import Processor
    frames, coords, truth = KC.two_blues(True)
    recs = _records(coords, len(frames))
    pr = Processor(_stub_model(handle, recs))
    table, tm = pr.process_data(frames, coords, 25, team_method="cluster")
    plain, tm0 = pr.process_data(frames, coords, 25)
    loose, tm1 = pr.process_data(frames, coords, 25, team_method="cluster", team_params=dict(outlier=0, min_crops=2))
    try:
        c = KC.BY_NAME["two_blues_and_a_yellow_referee"]
        assert tm == KR.mapping_of(KC.reference(c["name"])[1], c["slot_ids"]) and 21 not in tm and tm == table.team_mapping
        _equal((table.team_report["crops"], table.team_report["ids"], table.team_report["model"]), KC.reference(c["name"]), "table.team_report")
        assert plain.team_report is None and set(tm0.values()) <= {0, 1} and tm0 != tm
        assert 21 in tm1 and loose.team_report["params"] == {"min_pixels": 32, "min_crops": 2, "outlier": 0}
        with pytest.raises(ValueError):
            pr.process_data(frames, coords, 25, team_params=dict(outlier=0))
        # with merge_ids the heads inherit teams as they do from the colours' mapping: the table is the post-processor's own on the cluster mapping
        merged, tm2 = pr.process_data(frames, coords, 25, team_method="cluster", merge_ids=True)
        direct = handle.postprocess(recs, 25, KC.FW, dict(tm), merge_ids=True)
        try:
            assert tm2 == direct.team_mapping == merged.team_mapping and all(tm2[k] == v for k, v in tm.items()) and 21 not in tm2
            assert merged.merges == direct.merges and np.array(merged.values).tobytes() == np.array(direct.values).tobytes()
            _equal((merged.team_report["ids"], merged.team_report["model"]), KC.reference(c["name"])[1:], "merge_ids: the report")
        finally:
            merged.close(); direct.close()
    finally:
        for t in (table, plain, loose):
            t.close()


def _cli_clip(monkeypatch, n=12):
    """the boxes of the constructed clip stand in for the random networks' (the model's records are substituted, as in test_gpu_balltrack); the frames
    are the command line's own synthetic ones, so the expectation is the contract on those frames.  -> (records, coords, what get_coordinates saw)"""
    from eagle_amd import records
    from eagle_amd.coordinate_model import CoordinateModel
    _, coords, _ = KC.two_blues(True)
    box = {}
    for i in range(n):                                                          # the 64 x 96 layout scaled to the 720p frames of the command line
        box[i] = {"Coordinates": {"Player": {pid: {"BBox": [13 * it["BBox"][0], 11 * it["BBox"][1], 13 * it["BBox"][2], 11 * it["BBox"][3]]}
                                             for pid, it in coords[i]["Coordinates"]["Player"].items()}}}
    recs = _records(box, n, (13, 11))
    seen = {}

    def get_coordinates(self, frames, fps, **kw):
        seen["frames"] = np.ascontiguousarray(frames)
        out = {i: records.to_reference_dict(r, i, fps) for i, r in enumerate(recs)}
        self._last = (out, recs, np.ones(len(recs), bool))
        return out

    monkeypatch.setattr(CoordinateModel, "get_coordinates", get_coordinates)
    return recs, {i: records.to_reference_dict(r, i, 25) for i, r in enumerate(recs)}, seen


CLI_VALUES = ["--team-method", "cluster", "--team-min-pixels", "40", "--team-min-crops", "2", "--team-outlier", "0.75"]


def _cli_contract(coords_cli, frames, n):
    crops, slots, slot_ids = kits.crop_list(coords_cli, n)
    assert len(crops) >= 30 and len(slot_ids) >= 10
    exp = KR.team_cluster(frames, crops, slots, len(slot_ids), 40, 2, 768)
    report = {"params": {"min_pixels": 40, "min_crops": 2, "outlier": 768}, "crops": exp[0], "ids": exp[1], "model": exp[2], "slot_ids": slot_ids}
    return json.loads(json.dumps(kits.to_json(report))), {str(k): v for k, v in KR.mapping_of(exp[1], slot_ids).items()}


def test_cli_team_method(tmp_path, monkeypatch):
    from eagle_amd import cli
    n = 12
    recs, coords_cli, seen = _cli_clip(monkeypatch, n)
    out = str(tmp_path / "out")
    common = ["--frames", str(n), "--fps", "25", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed"]
    assert cli.main(common) == 0
    meta0 = json.load(open(os.path.join(out, "metadata.json")))
    assert "teams" not in meta0 and not os.path.exists(os.path.join(out, "teams.json"))                     # without the flag: the reference's rule, as before
    big = lib.Handle(batch=1)
    try:
        d = big.upload(seen["frames"])
        assert meta0["team_mapping"] == {str(k): v for k, v in teams.get_team_mapping(big, d, coords_cli, n_frames=n).items()}
    finally:
        big.close()
    assert cli.main(common + CLI_VALUES) == 0
    teams_json, mapping = _cli_contract(coords_cli, seen["frames"], n)
    assert json.load(open(os.path.join(out, "teams.json"))) == teams_json and len(teams_json["ids"]) >= 10
    meta = json.load(open(os.path.join(out, "metadata.json")))
    assert meta["teams"] == "cluster" and meta["team_mapping"] == mapping


def test_cli_team_method_with_annotated_alone(tmp_path, monkeypatch):
    """--annotated without --processed finds the mapping on a path of its own"""
    from eagle_amd import cli
    n = 12
    recs, coords_cli, seen = _cli_clip(monkeypatch, n)
    out = str(tmp_path / "annotated")
    assert cli.main(["--frames", str(n), "--fps", "25", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--annotated"] + CLI_VALUES) == 0
    teams_json, mapping = _cli_contract(coords_cli, seen["frames"], n)
    assert json.load(open(os.path.join(out, "teams.json"))) == teams_json and os.path.getsize(os.path.join(out, "annotated.y4m")) > n * 720 * 1280
    meta = json.load(open(os.path.join(out, "metadata.json")))
    assert meta["teams"] == "cluster" and meta["team_mapping"] == mapping
