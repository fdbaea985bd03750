"""The ball track on the GPU (include/eagle.h, eagle_op_ball_track / eagle_ball_track / eagle_postprocess_ball; csrc/balltrack.hip): every field of every
output equals the contract of tests/balltrack_ref.py — tobytes(), no tolerance — for the constructed clips of tests/balltrack_cases.py, with either way
of recovering the chosen nodes; two runs give identical bytes; NULL outputs in every combination; every refusal leaves poisoned outputs alone; through
a handle on constructed records: eagle_postprocess_ball(NULL) is eagle_postprocess byte for byte, with a ball_det it is eagle_postprocess on the pruned
records; the point of the feature: a clip whose ball hops between team mates, with a distractor near the image origin in every frame, gives the clean
clip's possession events from the tracked table and other events from the plain one; Processor.process_data(ball_track=True); the command line's
ball_track.json equals balltrack.to_json of the contract."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import balltrack_cases as BC
import balltrack_ref as BR
import post_cases
from eagle_amd import balltrack, lib, weights

pytestmark = pytest.mark.gpu

vp = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def _equal(got, exp, what):
    for a, b, part in zip(got, exp, BC.PARTS):
        assert a.shape == b.shape, (what, part, a.shape, b.shape)
        for k in a.dtype.names:
            assert np.array_equal(a[k], b[k]), (what, part, k)
        assert a.tobytes() == b.tobytes(), (what, part)


def _op(c, recover=lib.BALL_RECOVER_DEFAULT):
    return lib.op_ball_track(c["counts"], c["pos"], c["cq"], lib.ball_track_params(**c["p"]), c["cuts"], det=c["det"], recover=recover)


@pytest.mark.parametrize("name", [c["name"] for c in BC.CASES])
def test_op_ball_track_equals_contract(name):
    got = _op(BC.BY_NAME[name])
    if len(BC.BY_NAME[name]["counts"]) == 0:                                    # n == 0 succeeds and writes nothing: the wrapper's zeros
        assert got[0].shape == (0,) and got[1].shape == (0,) and got[2].tobytes() == bytes(64)
    else:
        _equal(got, BC.reference(name), name)


@pytest.mark.parametrize("name", ["one_segment_of_5000_random_frames", "segments_300", "cuts_back_to_back", "mirror_images_crossing_gaps", "n_1", "candidates_0"])
def test_both_recoveries_equal_contract(name):
    for recover in (lib.BALL_RECOVER_DOUBLING, lib.BALL_RECOVER_CHASE):
        _equal(_op(BC.BY_NAME[name], recover), BC.reference(name), (name, recover))


def test_two_runs_give_identical_bytes():
    for name in ("one_segment_of_5000_random_frames", "ring_wrap_G_64_two_candidates", "segments_300"):
        _equal(_op(BC.BY_NAME[name]), _op(BC.BY_NAME[name]), "second run of " + name)


def test_conf_and_det_inputs():
    """conf instead of cq (cq = floor(conf * 1024)), and det carried into the frame records"""
    c = BC.BY_NAME["distractor_in_every_frame"]
    conf = (c["cq"] / 1024.0 + 0.0004).astype(np.float32)
    conf[c["cq"] == 1024] = 1.0
    det = (np.arange(len(c["cq"])) * 3 % 300).astype(np.int32)
    got = lib.op_ball_track(c["counts"], c["pos"], None, lib.ball_track_params(**c["p"]), c["cuts"], conf=conf, det=det)
    exp = BR.track_window(c["counts"], c["pos"], BR.cq_of_conf(conf), *BC.resolved(c), cuts=c["cuts"], det=det)
    assert np.array_equal(BR.cq_of_conf(conf), c["cq"]) and (got[0]["det"] >= 0).all()
    _equal(got, exp, "conf and det")


def _poisoned(n):
    fr, tr, clip, ms = np.zeros(n, lib.BALL_FRAME_DTYPE), np.zeros(max(n, 1), lib.BALL_TRACKLET_DTYPE), np.zeros(1, lib.BALL_CLIP_DTYPE), np.full(4, -7.0, np.float32)
    fr["qx"] = 77; tr["shot"] = 66; clip["reserved"] = 55
    return fr, tr, clip, ms


UNTOUCHED = (lambda fr: (fr["qx"] == 77).all() and not fr["cand"].any() and not fr["f"].any(), lambda tr: (tr["shot"] == 66).all() and not tr["sightings"].any(),
             lambda clip: (clip["reserved"] == 55).all() and not clip["V"].any() and not clip["shots"].any(), lambda ms: (ms == -7.0).all())


def test_null_outputs_in_every_combination_and_no_frames():
    L = lib.load()
    c = BC.BY_NAME["cuts_back_to_back"]
    n, exp = len(c["counts"]), BC.reference(c["name"])
    p = lib.ball_track_params(**c["p"])
    cuts = np.array(c["cuts"], np.int32)
    head = (0, vp(c["counts"]), n, vp(c["pos"]), vp(c["cq"]), None, None, vp(cuts), len(cuts), C.byref(p), 0)
    for want in itertools.product((False, True), repeat=4):
        fr, tr, clip, ms = _poisoned(n)
        ptr = [vp(a) if w else None for a, w in zip((fr, tr, clip, ms), want)]
        assert L.eagle_op_ball_track(*head, ptr[0], ptr[1], n, ptr[2], ptr[3]) == 0, want
        for a, b, w, alone in zip((fr, tr[:len(exp[1])], clip), exp, want, UNTOUCHED):
            assert a.tobytes() == b.tobytes() if w else alone(a), want
        assert (ms >= 0).all() and ms[3] > 0 if want[3] else UNTOUCHED[3](ms)
    fr, tr, clip, ms = _poisoned(n)
    assert L.eagle_op_ball_track(*head, vp(fr), vp(tr), 1, vp(clip), None) == 0                     # a small cap: the first tracklet only
    assert tr[:1].tobytes() == exp[1][:1].tobytes() and UNTOUCHED[1](tr[1:]) and clip[0]["tracklets"] == 2
    out = _poisoned(n)
    assert L.eagle_op_ball_track(0, None, 0, None, None, None, None, None, 0, C.byref(p), 0, vp(out[0]), vp(out[1]), n, vp(out[2]), vp(out[3])) == 0      # n == 0 writes nothing
    assert all(f(a) for f, a in zip(UNTOUCHED, out))
    fr, tr, clip = lib.op_ball_track(np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.int32), p)
    assert fr.shape == (0,) and tr.shape == (0,) and not clip[0]["shots"]


@pytest.mark.parametrize("what,change", BC.REFUSALS, ids=[w for w, _ in BC.REFUSALS])
def test_refusals_leave_the_outputs_alone(what, change):
    L = lib.load()
    c = BC.BY_NAME["candidates_2"]
    n = len(c["counts"])
    a = dict(counts=c["counts"].copy(), pos=c["pos"].copy(), cq=c["cq"].copy(), conf=None, cuts=[2], n=n, n_cuts=None, par=True, recover=0)
    par = dict(c["p"], max_bytes=0)
    change = dict(change)
    par.update(change.pop("p", {}))
    p = lib.ball_track_params(**par)
    if "reserved" in change:
        p.reserved[change.pop("reserved")] = 1
    if "count0" in change:
        a["counts"][0] = change.pop("count0")
    if "pos0" in change:
        a["pos"][0] = change.pop("pos0")
    if "cq0" in change:
        a["cq"][0] = change.pop("cq0")
    if "conf0" in change:
        a["conf"] = (c["cq"] / 1024.0).astype(np.float32)
        a["conf"][0], a["cq"] = change.pop("conf0"), None
    a.update(change)
    if a["counts"] is not None and a["counts"][0] == 301:                       # (the arrays hold what the counts say)
        a["pos"], a["cq"] = np.zeros((int(a["counts"].sum()), 2), np.int32), np.zeros(int(a["counts"].sum()), np.int32)
    cuts = None if a["cuts"] is None else np.array([n if v == "n" else v for v in a["cuts"]], np.int32)
    n_cuts = a["n_cuts"] if a["n_cuts"] is not None else 0 if cuts is None else len(cuts)
    out = _poisoned(n)
    rc = L.eagle_op_ball_track(0, vp(a["counts"]), a["n"], vp(a["pos"]), vp(a["cq"]), vp(a["conf"]), None, vp(cuts), n_cuts, C.byref(p) if a["par"] else None, a["recover"],
                               vp(out[0]), vp(out[1]), n, vp(out[2]), vp(out[3]))
    assert rc == lib.E_INVALID and L.eagle_last_error(None).decode() and all(f(x) for f, x in zip(UNTOUCHED, out)), what


def test_the_unchanged_call_of_the_refusals_succeeds():
    c = BC.BY_NAME["candidates_2"]
    got = lib.op_ball_track(c["counts"], c["pos"], c["cq"], lib.ball_track_params(**c["p"]), [2])
    _equal(got, BR.track_window(c["counts"], c["pos"], c["cq"], *BC.resolved(c), cuts=[2]), "candidates_2 with a cut")


# ---- through a handle -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


PLAYERS = 8
HOP_MAPPING = {i + 1: i % 2 for i in range(PLAYERS)}
HOP = dict(speed=1300.0)                                                        # every pass is admissible, however far it goes between two frames


def _hop_records(n, distractor, seed=5):
    """n records of eight players on a slow random walk, picture = pitch x 10; the ball sits on a player for three frames and hops to another (ids are
    detection index + 1).  distractor: a second ball detection near the image origin in every frame, of low confidence, listed first"""
    r = np.random.default_rng(seed)
    k = PLAYERS + 1 + (1 if distractor else 0)
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = k, 1, 1
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    pos = np.stack([r.uniform(10, 95, PLAYERS), r.uniform(5, 63, PLAYERS)], 1)[None] + np.cumsum(r.normal(0, 0.7, (n, PLAYERS, 2)), 0)
    pos = np.clip(pos, 1, [104, 67]).astype(np.int32)
    holder = np.repeat(r.integers(0, PLAYERS, n // 3 + 1), 3)[:n]
    d = recs["det"]

    def put(j, cls, ident, conf, px, py):
        d["reported"][:, j], d["in_bounds"][:, j], d["conf"][:, j], d["cls"][:, j], d["id"][:, j] = 1, 1, conf, cls, ident
        d["pitch_x"][:, j], d["pitch_y"][:, j] = px, py
        d["bx1"][:, j], d["bx2"][:, j], d["by1"][:, j], d["by2"][:, j] = 10 * px - 3, 10 * px + 3, 10 * py - 6, 10 * py

    j0 = 1 if distractor else 0
    if distractor:
        put(0, 2, 7, 0.5, 1 + np.arange(n) % 2, 1 + (np.arange(n) // 2) % 2)
    for j in range(PLAYERS):
        put(j0 + j, 0, j + 1, 0.9, pos[:, j, 0], pos[:, j, 1])
    put(j0 + PLAYERS, 2, 0, 0.9, pos[np.arange(n), holder, 0], pos[np.arange(n), holder, 1])
    return recs


def _contract(recs, fps=25, frame_w=1280, cuts=(), **kw):
    counts, pos, cq, det = BR.candidates_of_records(recs)
    return BR.track_window(counts, pos, cq, *BR.resolve(fps, frame_w, **kw), cuts=cuts, det=det)


def _pruned(recs, ball_det):
    out = recs.copy()
    for i, r in enumerate(out):
        for k in range(int(r["n_det"])):
            if r["det"][k]["cls"] == 2 and k != ball_det[i]:
                r["det"][k]["reported"] = 0
    return out


def _same_table(a, b, what):
    assert a.flags == b.flags and np.array_equal(a.rows, b.rows) and a.columns.tobytes() == b.columns.tobytes(), what
    assert np.array(a.values).tobytes() == np.array(b.values).tobytes(), what


def test_handle_ball_track_equals_contract(handle):
    for name, cuts in (("goalkeeper_fold", ()), ("appear_vanish_return", (5,)), ("empty", ()), ("ball_none", ())):
        case = post_cases.BY_NAME[name]
        recs = post_cases.records_of(case)
        got = handle.ball_track(recs, lib.ball_track_params(case["fps"], case["frame_w"]), cuts)
        if len(recs):
            _equal(got, _contract(recs, case["fps"], case["frame_w"], cuts), name)
        else:
            assert got[0].shape == (0,) and got[1].shape == (0,)
    recs = _hop_records(40, True)
    got = handle.ball_track(recs, lib.ball_track_params(25, 1280, **HOP), [13, 14])
    _equal(got, _contract(recs, cuts=[13, 14], **HOP), "hop with cuts")
    assert got[2][0]["shots"] == 3 and got[2][0]["frames_multi"] == 40
    bad = recs.copy()
    bad[3]["det"][0]["conf"] = np.nan
    p = lib.ball_track_params(25, 1280)
    t = C.c_void_p()
    assert handle.L.eagle_ball_track(handle._h, vp(bad), len(bad), None, 0, C.byref(p), C.byref(t)) == lib.E_INVALID and b"conf" in handle.L.eagle_last_error(handle._h) and not t.value
    bad = recs.copy()
    bad[3]["n_det"] = 301
    assert handle.L.eagle_ball_track(handle._h, vp(bad), len(bad), None, 0, C.byref(p), C.byref(t)) == lib.E_INVALID and b"n_det" in handle.L.eagle_last_error(handle._h)
    assert handle.L.eagle_ball_track(handle._h, vp(recs), len(recs), None, 0, C.byref(p), None) == lib.E_INVALID
    small = lib.ball_track_params(25, 1280, max_bytes=64)
    assert handle.L.eagle_ball_track(handle._h, vp(recs), len(recs), None, 0, C.byref(small), C.byref(t)) == lib.E_INVALID and b"budget" in handle.L.eagle_last_error(handle._h)


def test_postprocess_ball_null_is_postprocess_and_a_ball_det_is_the_pruned_records(handle):
    recs = _hop_records(40, True)
    tm = HOP_MAPPING
    plain = handle.postprocess(recs, 25, 1280, tm)
    ids, vals, nt = lib._team_arrays(tm)
    p = lib.EaglePostParams(25, 1280, 0, 0, ids.ctypes.data, vals.ctypes.data, nt, 0, 0)
    t = C.c_void_p()
    assert handle.L.eagle_postprocess_ball(handle._h, vp(recs), len(recs), C.byref(p), None, C.byref(t)) == 0
    null = lib.PostTable(handle, t, tm)
    fr, tr, clip = handle.ball_track(recs, lib.ball_track_params(25, 1280, **HOP))
    tracked = handle.postprocess(recs, 25, 1280, tm, ball_det=fr["det"])
    pruned = handle.postprocess(_pruned(recs, fr["det"]), 25, 1280, tm)
    none = handle.postprocess(recs, 25, 1280, tm, ball_det=np.full(len(recs), -1, np.int32))
    one = np.full(len(recs), -1, np.int32); one[4] = fr["det"][4]
    single = handle.postprocess(recs, 25, 1280, tm, ball_det=one)
    try:
        _same_table(null, plain, "ball_det NULL")
        _same_table(tracked, pruned, "ball_det of the track")
        assert np.array(tracked.values).tobytes() != np.array(plain.values).tobytes()
        assert none.flags & lib.POST_NO_BALL and single.flags & lib.POST_NO_BALL and not tracked.flags & lib.POST_NO_BALL          # fewer than two sightings
        for bad in (1, -2, 10, 300):                                                                                              # a player, below -1, n_det, beyond the record
            wrong = fr["det"].copy(); wrong[7] = bad
            t2 = C.c_void_p()
            assert handle.L.eagle_postprocess_ball(handle._h, vp(recs), len(recs), C.byref(p), vp(wrong), C.byref(t2)) == lib.E_INVALID and not t2.value
            assert b"ball_det[7]" in handle.L.eagle_last_error(handle._h)
    finally:
        for x in (plain, null, tracked, pruned, none, single):
            x.close()


def test_the_tracked_table_gives_the_clean_clip_s_events(handle):
    """the point of the feature"""
    clean, noisy = _hop_records(60, False), _hop_records(60, True)
    pp = lib.possession_params(25, 1024.0, 1, 1000)
    fr, tr, clip = handle.ball_track(noisy, lib.ball_track_params(25, 1280, **HOP))
    tables = [handle.postprocess(clean, 25, 1280, HOP_MAPPING), handle.postprocess(noisy, 25, 1280, HOP_MAPPING), handle.postprocess(noisy, 25, 1280, HOP_MAPPING, ball_det=fr["det"])]
    try:
        ev = [handle.possession(t, pp)[3] for t in tables]
        print("events: clean", len(ev[0]), "plain", len(ev[1]), "tracked", len(ev[2]), "tracklets", len(tr), "chosen", clip[0]["frames_chosen"], "rejected", clip[0]["rejected"])
        assert (fr["cand"] == 0).all() and (fr["det"] == PLAYERS + 1).all() and clip[0]["rejected"] == 60                    # the distractor, detection 0, is never chosen
        assert (ev[0]["kind"] == lib.EVENT_PASS).sum() >= 3
        assert ev[1].tobytes() != ev[0].tobytes() and ev[2].tobytes() == ev[0].tobytes()
        ball = [k for k, c in enumerate(tables[0].columns) if int(c["kind"]) == lib.POST_BALL]
        assert np.array(tables[2].values)[ball].tobytes() == np.array(tables[0].values)[ball].tobytes()
    finally:
        for t in tables:
            t.close()


def _stub_model(handle, recs):
    import types
    return types.SimpleNamespace(handle=handle, _records_of=lambda c: recs)


def test_processor_process_data_with_ball_track(handle, monkeypatch):
    from eagle_amd.processor import Processor
    recs = _hop_records(40, True)
    pr = Processor(_stub_model(handle, recs))
    monkeypatch.setattr(Processor, "get_team_mapping", lambda self, frames, coords, pixel_format="bgr": dict(HOP_MAPPING))
    table, tm = pr.process_data(None, recs, 25, ball_track=dict(HOP), cuts=[20])
    plain, _ = pr.process_data(None, recs, 25)
    exp = _contract(recs, cuts=[20], **HOP)
    pruned = handle.postprocess(_pruned(recs, exp[0]["det"]), 25, 1280, HOP_MAPPING)
    try:
        _equal(table.ball_track, exp, "Processor.process_data")
        _equal(pr.ball_track(recs, 25, [20], **HOP), exp, "Processor.ball_track")
        _same_table(table, pruned, "the tracked table")
        assert plain.ball_track is None and np.array(plain.values).tobytes() != np.array(table.values).tobytes()
    finally:
        for t in (table, plain, pruned):
            t.close()


def test_cli_ball_track(tmp_path, monkeypatch):
    """the detections of the constructed clip stand in for the random networks' (the model's records and the team mapping are substituted, as in
    test_gpu_offside); everything behind them is the command line's own path"""
    from eagle_amd import cli, records
    from eagle_amd.coordinate_model import CoordinateModel
    from eagle_amd.processor import Processor
    recs = _hop_records(30, True)

    def get_coordinates(self, frames, fps, **kw):
        coords = {i: records.to_reference_dict(r, i, fps) for i, r in enumerate(recs)}
        self._last = (coords, recs, np.ones(len(recs), bool))
        return coords

    monkeypatch.setattr(CoordinateModel, "get_coordinates", get_coordinates)
    monkeypatch.setattr(Processor, "get_team_mapping", lambda self, frames, coords, pixel_format="bgr": dict(HOP_MAPPING))
    out = str(tmp_path / "out")
    common = ["--frames", "30", "--fps", "25", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed", "--ball-track"]
    assert cli.main(common + ["--ball-track-speed", "1300", "--ball-track-gap", "5", "--ball-track-rows"]) == 0
    exp = _contract(recs, speed=1300.0, gap=5)
    j = json.load(open(os.path.join(out, "ball_track.json")))
    assert j == json.loads(json.dumps(balltrack.to_json(*exp, rows=True))) and len(j["frames"]) == 30 and j["totals"]["frames_chosen"] == 30
    assert json.load(open(os.path.join(out, "metadata.json")))["ball"] == "ball_track"
    rows = json.load(open(os.path.join(out, "processed_data.json")))
    assert cli.main(common + ["--ball-track-speed", "1300", "--ball-track-reward", "350", "--ball-track-break", "900"]) == 0
    j = json.load(open(os.path.join(out, "ball_track.json")))
    assert j == json.loads(json.dumps(balltrack.to_json(*_contract(recs, speed=1300.0, reward=350.0, brk=900.0)))) and "frames" not in j
    assert cli.main(common[:-1]) == 0 and "ball" not in json.load(open(os.path.join(out, "metadata.json")))
    assert json.load(open(os.path.join(out, "processed_data.json"))) != rows                                             # without the flag: the reference's ball
