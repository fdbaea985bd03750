"""The ball track's contract (tests/balltrack_ref.py) against itself, without a GPU: its two definitions agree on every constructed clip of
tests/balltrack_cases.py; every clip of at most 6 frames and 3 candidates is also enumerated, choice by choice, and the chosen path's score is the
maximum; each clip forces what its name says; cutting a shot at its runs of at least G candidate-free frames changes nothing (the argument the forward
kernel's segments rest on); the sum of the tracklets' gains is the clip's score; the records have the sizes include/eagle.h states; the command line
refuses the value flags without --ball-track."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import balltrack_cases as BC
import balltrack_ref as BR

NAMES = [c["name"] for c in BC.CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, what):
    for x, y, part in zip(a, b, BC.PARTS):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, part)
        for k in x.dtype.names:
            assert np.array_equal(x[k], y[k]), (what, part, k)
        assert x.tobytes() == y.tobytes(), (what, part)


@pytest.mark.parametrize("name", NAMES)
def test_the_two_definitions_agree(name):
    c = BC.BY_NAME[name]
    loop = BR.track_loop(c["counts"], c["pos"], c["cq"], *BC.resolved(c), cuts=c["cuts"], det=c["det"])
    _same(loop, BC.reference(name), name)


def test_small_clips_are_enumerated():
    assert len(BC.SMALL) >= 20
    positive = 0
    for name in BC.SMALL:
        c = BC.BY_NAME[name]
        best = BR.enumerate_best(c["counts"], c["pos"], c["cq"], *BC.resolved(c), cuts=c["cuts"])
        assert BC.reference(name)[2][0]["score"] == best, name
        positive += best > 0
    assert positive >= 10


@pytest.mark.parametrize("name", sorted(BC.FORCES))
def test_each_case_forces_its_name(name):
    BC.FORCES[name](*BC.reference(name))


def test_every_constructed_case_has_its_property():
    assert not [n for n in NAMES if n not in BC.FORCES and not n.startswith("small_random_")]


@pytest.mark.parametrize("name", NAMES)
def test_splitting_at_empty_runs_changes_nothing(name):
    c = BC.BY_NAME[name]
    _same(BR.track_window(c["counts"], c["pos"], c["cq"], *BC.resolved(c), cuts=c["cuts"], det=c["det"], split=True), BC.reference(name), name)


def test_the_split_cases_do_split():
    c = BC.BY_NAME["segments_300"]
    m = np.minimum(c["counts"], BR.MAX_CAND)
    assert len(BR.split_at_empty_runs(m, 0, len(m), BC.resolved(c)[1])) == 300
    for name, pieces in (("empty_run_of_G_minus_1", 1), ("empty_run_of_G", 2), ("gap_of_G", 1), ("gap_of_G_plus_1", 2)):
        c = BC.BY_NAME[name]
        m = np.minimum(c["counts"], BR.MAX_CAND)
        assert len(BR.split_at_empty_runs(m, 0, len(m), BC.resolved(c)[1])) == pieces, name


@pytest.mark.parametrize("name", NAMES)
def test_gains_add_up_to_the_score(name):
    fr, tr, clip = BC.reference(name)
    assert int(tr["gain"].sum()) == int(clip[0]["score"]) and int(tr["sightings"].sum()) == int(clip[0]["frames_chosen"])
    assert clip[0]["rejected"] + clip[0]["frames_chosen"] + clip[0]["ignored"] == BC.BY_NAME[name]["counts"].sum()


def test_defaults_at_1280():
    assert BR.resolve(25, 1280) == (256, 25, 256, 640) and BR.resolve(120, 1280)[1] == 64 and BR.resolve(25, 1280, 10.25, 3, 7.5, 1.0) == (21, 3, 15, 2)
    two = BC._case("two", [[(600, 400, 1024)], [(610, 400, 1024)]])
    assert BR.track_window(two["counts"], two["pos"], two["cq"], *BC.resolved(two))[2][0]["tracklets"] == 0        # two perfect sightings 5 px apart give nothing
    assert BC.reference("n_3")[2][0]["tracklets"] == 1                                                              # three give a track


def test_isqrt_array_at_the_boundaries():
    ks = np.array([1, 2, 255, 256, 65535, 185361], np.int64)
    for d in (-1, 0, 1):
        v = ks * ks + d
        assert [int(x) for x in BR.isqrt_array(v)] == [BR.isqrt(int(x)) for x in v]


def test_struct_sizes():
    from eagle_amd import lib
    assert (BR.FRAME_DTYPE.itemsize, BR.TRACKLET_DTYPE.itemsize, BR.CLIP_DTYPE.itemsize) == (32, 48, 64)
    assert (lib.BALL_FRAME_DTYPE, lib.BALL_TRACKLET_DTYPE, lib.BALL_CLIP_DTYPE) == (BR.FRAME_DTYPE, BR.TRACKLET_DTYPE, BR.CLIP_DTYPE)
    assert C.sizeof(lib.EagleBallTrackParams) == 64 and lib.BALL_MAX_CAND == BR.MAX_CAND
    header = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name, size in (("EagleBallTrackParams", 64), ("EagleBallFrame", 32), ("EagleBallTracklet", 48), ("EagleBallClip", 64)):
        assert re.search(r"\} %s;\s*/\* %d bytes" % (name, size), header), name
    for name in ("eagle_ball_track", "eagle_ball_track_values", "eagle_ball_track_tracklets", "eagle_op_ball_track", "eagle_postprocess_ball"):
        assert re.search(r"^int %s\(" % name, header, re.M) and name in lib.EXPORTS, name


@pytest.mark.parametrize("argv", [["--ball-track"], ["--processed", "--ball-track-speed", "100"], ["--processed", "--ball-track-gap", "5"],
                                  ["--processed", "--ball-track-reward", "50"], ["--processed", "--ball-track-break", "50"], ["--processed", "--ball-track-rows"],
                                  ["--processed", "--ball-track", "--ball-track-gap", "65"], ["--processed", "--ball-track", "--ball-track-speed", "-1"]])
def test_cli_argument_errors(argv, capsys):
    from eagle_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--frames", "4", "--synthetic-weights"] + argv)
    assert e.value.code == 2 and "ball-track" in capsys.readouterr().err


def test_cuts_of_shots_and_to_json():
    from eagle_amd import balltrack
    shots = [{"first": 0}, {"first": 10}, {"first": 25}, {"first": 40}]
    assert balltrack.cuts_of_shots(shots, 0, 40) == [10, 25] and balltrack.cuts_of_shots(shots, 10, 15) == [] and balltrack.cuts_of_shots(shots, 5, 30) == [5, 20]
    fr, tr, clip = BC.reference("cuts_back_to_back")
    j = balltrack.to_json(fr, tr, clip, rows=True)
    assert j["parameters"] == {"speed_half_px": 256, "gap_frames": 25, "reward_half_px": 256, "break_half_px": 640, "speed_px": 128.0, "reward_px": 128.0, "break_px": 320.0,
                               "max_candidates": 8}
    assert j["totals"]["shots"] == 3 and len(j["tracklets"]) == 2 and [r["shot_start"] for r in j["frames"]].count(True) == 3 and j["frames"][4]["candidate"] == -1
    assert "frames" not in balltrack.to_json(fr, tr, clip)
