"""The contract of the shots stage (tests/shots_ref.py), its cases (tests/shots_cases.py) and the host module eagle_amd/shots.py, without a GPU: every
case forces what it is named after; the two statements of the rule (array operations; plain loops) agree on every case and on 200 random small
clips; the refusals; the ABI; default_params; split, longest_usable and to_json on a hand-made result; the command line's refusals."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import shots_cases as SC
import shots_ref as SR
from eagle_amd import lib, shots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in SC.CASES]


def _same(a, b, what):
    for x, y, part in zip(a, b, ("signatures", "frames", "shots")):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, part)


@pytest.mark.parametrize("name", NAMES)
def test_case_forces_what_it_is_named_after(name):
    assert SC.BY_NAME[name]["check"](*SC.reference(name)), name


@pytest.mark.parametrize("name", NAMES)
def test_the_two_statements_agree(name):
    c = SC.BY_NAME[name]
    _same(SC.reference(name), SR.shots_scalar(c["frames"], c["p"]), name)


def test_the_two_statements_agree_on_random_small_clips():
    """200 clips of 4 x 4 .. 9 x 11 pixels and up to 24 frames: runs of a few palette colours with noise, cut, flashed and dissolved at random, with
    random parameters, so that every flag and kind occurs"""
    r = np.random.default_rng(31)
    seen_flags, seen_kinds = 0, set()
    for k in range(200):
        h, w, n = int(r.integers(4, 10)), int(r.integers(4, 12)), int(r.integers(0, 25))
        palette = r.integers(0, 256, (4, 3), np.uint8)
        frames = np.zeros((n, h, w, 3), np.uint8)
        cur = 0
        for i in range(n):
            if r.random() < 0.2:
                cur = int(r.integers(0, 4))
            frames[i] = palette[cur]
            if r.random() < 0.5:                                          # part of the picture from another colour: small and middling scores
                frames[i].reshape(-1, 3)[:int(r.integers(0, h * w))] = palette[int(r.integers(0, 4))]
            if r.random() < 0.1:
                frames[i] = 255
        cut = int(r.integers(0, SR.ONE + 1))
        p = {"cut": cut, "low": int(r.integers(0, cut + 1)), "grass_thr": int(r.integers(0, SR.ONE + 1)), "window": int(r.integers(2, 7)), "min_len": int(r.integers(1, 6))}
        a, b = SR.shots(frames, p), SR.shots_scalar(frames, p)
        _same(a, b, (k, p))
        seen_flags |= int(np.bitwise_or.reduce(a[1]["flags"])) if n else 0
        seen_kinds |= set(a[2]["kind"].tolist())
    assert seen_flags == 15 and seen_kinds == {0, 1, 2, 3}


def test_refusals():
    frames = SC.BY_NAME["cut_at_frame_1"]["frames"]
    for change, _ in SC.REFUSALS:
        for fn in (SR.shots, SR.shots_scalar):
            with pytest.raises(ValueError):
                fn(frames, dict(SC.BASE, **change))
    for h, w in SC.BAD_SIZES:
        with pytest.raises(ValueError):
            SR.check(SC.BASE, 1, h, w)
    with pytest.raises(ValueError):
        SR.check(SC.BASE, -1, 8, 8)
    for ok in ({"cut": 0, "low": 0}, {"cut": 65536, "low": 65536}, {"grass_thr": 0}, {"grass_thr": 65536}, {"window": 2}, {"min_len": 1}):
        SR.shots(frames, dict(SC.BASE, **ok))


def test_dtypes_constants_and_exports_are_the_library_s():
    assert (SR.FRAME_DTYPE, SR.SHOT_DTYPE, SR.SIG) == (lib.SHOT_FRAME_DTYPE, lib.SHOT_DTYPE, lib.SHOT_SIGNATURE)
    assert (SR.START, SR.AFTER_CUT, SR.AFTER_TRANSITION, SR.TRANSITION) == (lib.SHOT_START, lib.SHOT_AFTER_CUT, lib.SHOT_AFTER_TRANSITION, lib.SHOT_TRANSITION)
    assert (SR.FLASH, SR.HARD, SR.GRADUAL_END, SR.IN_TRANSITION) == (lib.SHOT_FRAME_FLASH, lib.SHOT_FRAME_HARD, lib.SHOT_FRAME_GRADUAL_END, lib.SHOT_FRAME_IN_TRANSITION)
    assert (SR.PITCH, SR.SHORT, SR.USABLE) == (lib.SHOT_PITCH, lib.SHOT_SHORT, lib.SHOT_USABLE)
    assert [SR.FRAME_DTYPE.fields[k][1] for k in ("d1", "d2", "dW", "sg", "st", "grass", "flags", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28] and SR.FRAME_DTYPE.itemsize == 32
    assert [SR.SHOT_DTYPE.fields[k][1] for k in ("first", "count", "kind", "flags", "grass_sum", "reserved")] == [0, 4, 8, 12, 16, 24] and SR.SHOT_DTYPE.itemsize == 32
    assert [getattr(lib.EagleShotParams, k).offset for k in ("cut", "low", "grass_thr", "window", "min_len", "reserved")] == [0, 4, 8, 12, 16, 20]
    assert C.sizeof(lib.EagleShotParams) == 32
    head = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name, v in (("EAGLE_SHOT_SIGNATURE", 1537), ("EAGLE_SHOT_START", 0), ("EAGLE_SHOT_AFTER_CUT", 1), ("EAGLE_SHOT_AFTER_TRANSITION", 2), ("EAGLE_SHOT_TRANSITION", 3),
                    ("EAGLE_SHOT_FRAME_FLASH", 1), ("EAGLE_SHOT_FRAME_HARD", 2), ("EAGLE_SHOT_FRAME_GRADUAL_END", 4), ("EAGLE_SHOT_FRAME_IN_TRANSITION", 8),
                    ("EAGLE_SHOT_PITCH", 1), ("EAGLE_SHOT_SHORT", 2), ("EAGLE_SHOT_USABLE", 4)):
        assert re.search(r"#define %s %d\b" % (name, v), head), name
    for name in ("eagle_shots_device_frames", "eagle_shots_frames", "eagle_op_shots"):
        assert re.search(r"^int %s\(" % name, head, re.M) and name in lib.EXPORTS, name
    for text in ("EagleShotParams", "EagleShotFrame", "EagleShot"):
        assert re.search(r"\} %s;\s+/\* 32 bytes \*/" % text, head), text
    declared = set(re.findall(r"^\s*(?:int|void|const char\*)\s+(eagle_\w+)\s*\(", head, re.M))
    assert declared == set(lib.EXPORTS)
    L = lib.load()
    assert all(hasattr(L, n) for n in lib.EXPORTS)


def test_default_params():
    assert shots.default_params(5) == {"cut": 19661, "low": 6554, "grass_thr": 22938, "window": 2, "min_len": 5} == SR.default_params(5)
    assert shots.default_params(24) == dict(shots.default_params(5), window=10, min_len=24) == SR.default_params(24)
    assert shots.default_params(25) == dict(shots.default_params(5), window=10, min_len=25) == SR.default_params(25)
    assert shots.default_params(1)["window"] == 2 and shots.default_params(30)["window"] == 12 and shots.default_params(60)["window"] == 24
    with pytest.raises(ValueError):
        shots.default_params(0)
    p = lib.shot_params(fps=24, cut=100, min_len=7)
    assert (p.cut, p.low, p.grass_thr, p.window, p.min_len, list(p.reserved)) == (100, 6554, 22938, 10, 7, [0, 0, 0])


def _hand_made():
    """six shots over 40 frames of 10 pixels: usable 8, short pitch 2, transition 3, usable 12 (the longest), usable 12 (a tie), not pitch 3"""
    sh = np.zeros(6, lib.SHOT_DTYPE)
    sh["first"], sh["count"] = [0, 8, 10, 13, 25, 37], [8, 2, 3, 12, 12, 3]
    sh["kind"] = [lib.SHOT_START, lib.SHOT_AFTER_CUT, lib.SHOT_TRANSITION, lib.SHOT_AFTER_TRANSITION, lib.SHOT_AFTER_CUT, lib.SHOT_AFTER_CUT]
    sh["flags"] = [5, 3, 2, 5, 5, 2]
    sh["grass_sum"] = [80, 10, 15, 60, 120, 0]
    fr = np.zeros(40, lib.SHOT_FRAME_DTYPE)
    fr["flags"][[4, 30]] = lib.SHOT_FRAME_FLASH
    fr["flags"][[8, 25, 37]] = lib.SHOT_FRAME_HARD
    return shots.Result(fr, sh, dict(shots.default_params(4), min_len=4, fps=4, pixels=10))


def test_split_longest_usable_and_to_json_on_a_hand_made_result():
    res = _hand_made()
    assert shots.usable(res) == [0, 3, 4] and shots.longest_usable(res) == 3
    frames = np.arange(40)
    got = list(shots.split(frames, res))
    assert [(a, b) for a, b, _ in got] == [(0, 8), (13, 12), (25, 12)] and all(np.array_equal(f, frames[a:a + b]) for a, b, f in got)
    assert [(a, b) for a, b, _ in shots.split(frames, res, usable_only=False)] == [(0, 8), (8, 2), (10, 3), (13, 12), (25, 12), (37, 3)]
    none = shots.Result(res.frames, res.shots[[1, 2, 5]], res.params)
    assert shots.usable(none) == [] and shots.longest_usable(none) is None and list(shots.split(frames, none)) == []
    j = shots.to_json(res)
    assert json.loads(json.dumps(j)) == j
    assert j["params"] == {"cut": 19661, "low": 6554, "grass_thr": 22938, "window": 2, "min_len": 4, "fps": 4} and j["frames"] == 40 and j["flashes"] == [4, 30]
    assert j["shots"][0] == {"first": 0, "count": 8, "seconds": 2.0, "kind": "start", "pitch": True, "short": False, "usable": True, "grass_share": 1.0}
    assert j["shots"][2] == {"first": 10, "count": 3, "seconds": 0.75, "kind": "transition", "pitch": False, "short": True, "usable": False, "grass_share": 0.5}
    assert [s["kind"] for s in j["shots"]] == ["start", "after_cut", "transition", "after_transition", "after_cut", "after_cut"]
    empty = shots.Result(np.zeros(0, lib.SHOT_FRAME_DTYPE), np.zeros(0, lib.SHOT_DTYPE), res.params)
    assert shots.to_json(empty)["shots"] == [] and shots.longest_usable(empty) is None


def test_cli_refusals(capsys):
    from eagle_amd import cli
    for argv in (["--shots-cut", "0.5"], ["--shots-low", "0.1"], ["--shots-grass", "0.2"], ["--shots-window", "4"], ["--shots-min-len", "3"],
                 ["--shots", "--shots-cut", "1.5"], ["--shots", "--shots-cut", "-0.1"], ["--shots", "--shots-cut", "nan"], ["--shots", "--shots-low", "0.5"],
                 ["--shots", "--shots-low", "2"], ["--shots", "--shots-grass", "1.01"], ["--shots", "--shots-window", "1"], ["--shots", "--shots-min-len", "0"],
                 ["--trim-to-shot", "first"], ["--trim-to-shot", "-1"], ["--trim-to-shot", "1.5"], ["--shots", "--fps", "0"], ["--trim-to-shot"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
