"""The team clustering's contract (tests/kits_ref.py) against itself, without a GPU: its two definitions agree on every constructed case of
tests/kits_cases.py; each case forces what its name says; the records have the sizes include/eagle.h states; the command line refuses the value flags
without --team-method cluster; kits.to_json; permuting the slots of a tie-free case leaves the partition alone; and the point of the feature: on the
seeded clip of a navy and a sky-blue kit the reference's rule (the oracle's colour counts under the vote of eagle_amd/teams.py) puts every id into one
team, while the contract splits the kits with no error."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import kits_cases as KC
import kits_ref as KR

NAMES = [c["name"] for c in KC.CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, what
        for k in x.dtype.names:
            assert np.array_equal(x[k], y[k]), (what, k)
        assert x.tobytes() == y.tobytes(), what


@pytest.mark.parametrize("name", NAMES)
def test_the_two_definitions_agree(name):
    _same(KC.reference(name, True), KC.reference(name), name)


@pytest.mark.parametrize("name", NAMES)
def test_each_case_forces_its_name(name):
    KC.FORCES[name](*KC.reference(name))


def test_the_cases_the_issue_lists_are_there():
    assert set(KC.FORCES) == set(NAMES) and len(KC.PIXEL_CASES) >= 15 and len(KC.ID_CASES) >= 15
    assert {len(KC.BY_NAME[f"crops_{n}"]["crops"]) for n in (0, 1, 4, 5, 1000)} == {0, 1, 4, 5, 1000}
    assert {len(KC.BY_NAME[f"ids_{n}"]["used"]) for n in (0, 1, 2, 3, 63, 64, 65, 257, 1024)} == {0, 1, 2, 3, 63, 64, 65, 257, 1024}


def test_the_hues_the_edge_case_leaves_out_of_the_upper_band_do_not_exist_there():
    assert set(KC.HUES) - KC.hues_of_the_upper_band() == set(KC.LOWER_BAND_ONLY)


def test_the_hsv_of_the_contract_is_the_oracle_s():
    from oracle import prims
    px = np.random.default_rng(3).integers(0, 256, (4000, 3), dtype=np.uint8)
    px[:256] = np.arange(256, dtype=np.uint8)[:, None]
    h, s, v = KR.hsv_array(px)
    assert np.array_equal(np.stack([h, s, v], 1), prims.bgr2hsv(px[None])[0].astype(np.int64))
    assert all(KR.hsv_px(*(int(c) for c in p)) == (a, b, c) for p, a, b, c in zip(px[:500], h, s, v))


def test_struct_sizes():
    from eagle_amd import lib
    assert (KR.CROP_DTYPE.itemsize, KR.ID_DTYPE.itemsize, KR.MODEL_DTYPE.itemsize) == (144, 160, 64)
    assert (lib.KIT_CROP_DTYPE, lib.KIT_ID_DTYPE, lib.KIT_MODEL_DTYPE) == (KR.CROP_DTYPE, KR.ID_DTYPE, KR.MODEL_DTYPE)
    assert C.sizeof(lib.EagleKitParams) == 32 and (lib.KIT_BINS, lib.KIT_MAX_IDS) == (KR.BINS, KR.MAX_IDS)
    assert (lib.KIT_CROP_OUTSIDE, lib.KIT_CROP_EMPTY, lib.KIT_CROP_FEW, lib.KIT_ID_WEAK, lib.KIT_ID_NEITHER, lib.KIT_ID_SINGLE, lib.KIT_MODEL_SINGLE, lib.KIT_MODEL_SWAPPED) == \
        (KR.CROP_OUTSIDE, KR.CROP_EMPTY, KR.CROP_FEW, KR.ID_WEAK, KR.ID_NEITHER, KR.ID_SINGLE, KR.MODEL_SINGLE, KR.MODEL_SWAPPED)
    header = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name, size in (("EagleKitParams", 32), ("EagleKitCrop", 144), ("EagleKitId", 160), ("EagleKitModel", 64)):
        assert re.search(r"\} %s;\s*/\* %d bytes" % (name, size), header), name
    for name in ("eagle_kit_params_default", "eagle_team_cluster", "eagle_op_team_cluster", "eagle_op_team_cluster_ids"):
        assert re.search(r"^int %s\(" % name, header, re.M) and name in lib.EXPORTS, name
    p = lib.kit_params()
    assert (p.min_pixels, p.min_crops, p.outlier) == KR.resolve() == (32, 3, 512) and lib.kit_params(5, 7, 0).outlier == 0


def test_the_caps_and_ranges_of_the_contract():
    for bad in (dict(min_pixels=0), dict(min_pixels=(1 << 20) + 1), dict(min_crops=0), dict(min_crops=(1 << 16) + 1), dict(outlier=-1), dict(outlier=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            KR.resolve(**bad)
    assert KR.resolve(1 << 20, 1 << 16, 1 << 20) == (1 << 20, 1 << 16, 1 << 20)
    with pytest.raises(ValueError):
        KR.cluster_ids(np.ones((1025, KR.BINS), np.int64), np.ones(1025, np.int64))
    with pytest.raises(ValueError):
        KR.cluster_ids(np.zeros((1, KR.BINS), np.int64), [1])
    c = KC.BY_NAME["window_all_grass"]
    with pytest.raises(ValueError):
        KR.team_cluster(c["frames"], c["crops"], [0, 2], 2)
    # the packed key: the greatest cost and the greatest pair rank share 64 bits
    assert (1 << 22) * 131072 < 1 << 44 and KR.MAX_IDS * (KR.MAX_IDS - 1) // 2 < 1 << 20


@pytest.mark.parametrize("argv", [["--processed", "--team-min-pixels", "10"], ["--processed", "--team-min-crops", "2"], ["--processed", "--team-outlier", "0.5"],
                                  ["--processed", "--team-method", "colours", "--team-outlier", "0"], ["--team-method", "cluster"],
                                  ["--processed", "--team-method", "cluster", "--team-min-pixels", "0"], ["--processed", "--team-method", "cluster", "--team-min-crops", "65537"],
                                  ["--processed", "--team-method", "cluster", "--team-outlier", "-0.1"], ["--processed", "--team-method", "cluster", "--team-outlier", "1025"],
                                  ["--processed", "--team-method", "cluster", "--team-outlier", "nan"], ["--processed", "--team-method", "kmeans"]])
def test_cli_argument_errors(argv, capsys):
    from eagle_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--frames", "4", "--synthetic-weights"] + argv)
    assert e.value.code == 2 and "team-" in capsys.readouterr().err


def _report(name):
    c = KC.BY_NAME[name]
    crops, ids, model = KC.reference(name)
    return {"params": dict(zip(("min_pixels", "min_crops", "outlier"), KR.resolve(**c["p"]))), "crops": crops, "ids": ids, "model": model, "slot_ids": c["slot_ids"]}


def test_to_json():
    from eagle_amd import kits
    j = kits.to_json(_report("two_blues_and_a_yellow_referee"))
    assert json.loads(json.dumps(j)) == j
    assert j["parameters"] == {"min_pixels": 32, "min_crops": 3, "outlier_1024": 512, "outlier": 0.5}
    assert j["model"]["voters"] == 21 and j["model"]["neither"] == 1 and not j["model"]["single"] and len(j["ids"]) == 21
    ref = [r for r in j["ids"] if r["id"] == 21][0]
    assert ref["team"] == "neither" and ref["crops_used"] == 6 and not ref["weak"]
    assert [t["ids"] for t in j["teams"]] == [10, 10] and [t["weight"] for t in j["teams"]] == [60, 60] and j["model"]["medoids"] == [t["medoid"] for t in j["teams"]]
    names = [[c["name"] for c in t["colours"]] for t in j["teams"]]
    truth = KC.two_blues(True)[2]
    navy = 0 if truth[j["teams"][0]["medoid"]] == 0 else 1
    assert names[navy][0].startswith("dark ") and not names[1 - navy][0].startswith("dark ") and all(len(c["bgr"]) == 3 for t in j["teams"] for c in t["colours"])
    for b in range(KR.BINS):                                                   # a bin's representative colour falls into that bin
        got = dict(KR.pixel_units(*kits.bin_bgr(b)))
        if not got:                                                            # a bright, saturated green keys away as grass
            assert b < 30 and b % 15 in (3, 4, 5, 6), b
            continue
        assert max(got, key=got.get) == b and got[b] == 12, b
    one = kits.to_json({"params": dict(min_pixels=32, min_crops=3, outlier=512), "ids": KC.reference("exactly_one_voter")[0], "model": KC.reference("exactly_one_voter")[1],
                        "slot_ids": [7, 8, 9, 10]})
    assert one["model"]["single"] and one["model"]["medoids"] == [None, None] and "colours" not in one["teams"][0] and one["ids"][2]["team"] is None


def test_a_permutation_of_the_slots_leaves_the_partition_alone():
    c = KC.BY_NAME["two_blues_with_weak_ids"]
    base = KR.mapping_of(KC.reference(c["name"])[1], c["slot_ids"])
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(c["n_ids"])
        ids = KR.team_cluster(c["frames"], c["crops"], perm[c["slots"]], c["n_ids"], **c["p"])[1]
        slot_ids = [None] * c["n_ids"]
        for k, pid in enumerate(c["slot_ids"]):
            slot_ids[perm[k]] = pid
        got = KR.mapping_of(ids, slot_ids)
        assert set(got) == set(base) and len({(base[p], got[p]) for p in base}) == 2


def test_crop_list_is_the_reference_s_bookkeeping():
    from eagle_amd import kits
    coords = {0: {"Coordinates": {"Player": {5: {"BBox": [10.7, 10.2, 22.9, 40.0]}, 3: {"BBox": [12, 12, 24, 42]}, 9: {"BBox": [50, 5, 50, 30]}}}},
              1: {"Coordinates": {"Player": {}}}, 2: {"Coordinates": {"Player": {3: {"BBox": [60, 10, 72, 40]}, 4: {"BBox": [30, 10, 42, 40]}}}},
              3: {"Coordinates": {"Player": {8: {"BBox": [0, 0, 12, 30]}}}}}
    crops, slots, ids = kits.crop_list(coords, 3)
    assert crops.tolist() == [[2, 60, 10, 72, 40], [2, 30, 10, 42, 40]] and slots.tolist() == [0, 1] and ids == [3, 4]          # frame 0: both overlap by more than 35 %; 9 is empty
    crops, slots, ids = kits.crop_list(coords)
    assert len(crops) == 3 and ids == [3, 4, 8]


def test_crop_list_holds_the_crops_teams_get_team_mapping_counts():
    """one walk serves both methods: what teams.get_team_mapping hands to eagle_team_colors is crop_list's list"""
    from eagle_amd import kits, teams
    seen = {}

    class Recorder:
        def team_colors(self, dptr, n_frames, crops):
            seen["crops"], seen["n_frames"] = np.asarray(crops, np.int32).reshape(-1, 5), n_frames
            return np.zeros((len(crops), 12), np.int32)

    for frames, coords, _ in (KC.two_blues(True), KC.kit_clip([KC.NAVY, KC.SKY], 4, [6, 6, 1, 2, 6, 6, 2, 1], 13)):
        for n in (len(frames), 3, None, len(frames) + 5):
            seen["n_frames"] = None
            teams.get_team_mapping(Recorder(), None, coords, n_frames=n)
            assert seen["n_frames"] == min(len(frames) if n is None else n, len(coords))          # what the kernel is told is resident
            crops, slots, ids = kits.crop_list(coords, n)
            assert np.array_equal(seen["crops"], crops) and len(crops) and [ids[s] for s in slots] == [pid for _, pid, _, _ in teams.eligible_crops(coords, n)]


class _OracleHandle:
    """eagle_team_colors' twelve counts per crop from the oracle's restatement of the reference's detect_color"""

    def __init__(self, frames):
        self.frames = frames

    def team_colors(self, dptr, n_frames, crops):
        from oracle import colors
        out = np.zeros((len(crops), 12), np.int32)
        for row, (f, x1, y1, x2, y2) in zip(out, crops):
            for colour, n in colors.detect_color(self.frames[f][y1:y2, x1:x2]):
                row[colors.COLOR_ORDER.index(colour)] = n
        return out


def test_the_reference_s_rule_puts_two_blues_in_one_team_and_the_contract_splits_them():
    from eagle_amd import teams
    from oracle import colors
    assert colors.COLOR_ORDER == teams.COLORS
    frames, coords, truth = KC.two_blues()
    by_names = teams.get_team_mapping(_OracleHandle(frames), None, coords, n_frames=len(frames))
    assert set(by_names) == set(truth) and set(by_names.values()) == {0}
    c = KC.BY_NAME["two_blues"]
    ours = KR.mapping_of(KC.reference("two_blues")[1], c["slot_ids"])
    assert set(ours) == set(truth) and len({(truth[p], ours[p]) for p in truth}) == 2
