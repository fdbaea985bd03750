"""-m gpu: team colours through the C ABI (eagle_team_colors, K15) on a clip resident in HBM
 - against the reference's own outputs (tests/golden/team_golden.json: eagle/processor.py's get_team_mapping / detect_color run over
   scikit-learn's KMeans), and
 - team_color_kernel alone on the constructed crops of tests/team_color_cases.py (tests/test_team_cases_cpu.py shows what each forces): the twelve
   counts of every crop equal to oracle/colors.py exactly (integers, no tolerance), whatever the shape of the call, the handle or the frame size;
   the argument refusals of eagle_team_colors; the host mapping of eagle_amd/teams.py against the oracle's on constructed clips."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import team_cases
import team_color_cases as T
from eagle_amd import lib, teams

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "team_golden.json")))


def test_crop_colours_and_team_mapping_equal_reference():
    frames, coords = team_cases.make_case()
    h = lib.Handle(batch=1)
    d = h.upload(np.stack(frames))
    try:
        crops = [(c["frame"], *c["bbox"]) for c in GOLD["crops"]]
        got = teams.crop_colors(h, d, len(frames), crops)
        same = sum([[k, n] for k, n in g] == c["colors"] for g, c in zip(got, GOLD["crops"]))
        top = sum((g[0][0] if g else None) == (c["colors"][0][0] if c["colors"] else None) for g, c in zip(got, GOLD["crops"]))
        print(f"crops with identical colour counts: {same} of {len(crops)}; identical dominant colour: {top}")
        # the kernel runs scikit-learn's 2-means step by step (seeding from RandomState(0)'s first doubles, tolerance rule): every crop equal
        assert same == len(crops) and top == len(crops)
        # ... and equal to the oracle on crops of another clip and of random noise (Lloyd stops by the tolerance rule there)
        from oracle import colors
        frames2, coords2 = team_cases.make_case(seed=1, ts=(3, 12))
        rng = np.random.default_rng(5)
        noise = rng.integers(0, 256, (1, 720, 1280, 3), dtype=np.uint8)
        d2 = h.upload(np.concatenate([np.stack(frames2), noise]))
        try:
            cr = [(i, *p["BBox"]) for i in range(2) for p in coords2[i]["Coordinates"]["Player"].values()]
            cr += [(2, int(x), int(y), int(x) + int(w), int(y) + int(hh)) for x, y, w, hh in zip(rng.integers(0, 1200, 40), rng.integers(0, 640, 40), rng.integers(8, 60, 40), rng.integers(8, 70, 40))]
            got2 = teams.crop_colors(h, d2, 3, cr)
            src = frames2 + [noise[0]]
            bad = [c for c, g in zip(cr, got2) if [(k, n) for k, n in g] != colors.detect_color(src[c[0]][c[2]:c[4], c[1]:c[3]])]
            assert not bad, bad
        finally:
            h.free(d2)
        m = teams.get_team_mapping(h, d, coords)
        assert {str(k): v for k, v in m.items()} == GOLD["team_mapping"]
        # degenerate crops do not break the kernel: empty, out of frame, single colour
        z = h.team_colors(d, len(frames), [(0, 10, 10, 10, 40), (0, -5, 0, 20, 20), (9, 0, 0, 8, 8), (0, 0, 0, 16, 16)])
        assert z.shape == (4, 12) and not z[:3].any()
        crop = frames[0][0:16, 0:16]
        assert z[3].tolist() == T.oracle_row(crop)
        assert sorted([(c, int(n)) for c, n in zip(teams.COLORS, z[3, :11]) if n > 0], key=lambda x: x[1], reverse=True) == colors.detect_color(crop)
    finally:
        h.free(d); h.close()


# ---- the kernel alone on constructed crops (tests/team_color_cases.py) ---------------------------------------------------------------------------
class _Handles:
    """one handle per frame size, made when first asked for"""

    def __init__(self):
        self.made = {}

    def __call__(self, hw):
        if hw not in self.made:
            self.made[hw] = lib.Handle(batch=1, frame_h=hw[0], frame_w=hw[1])
        return self.made[hw]

    def close(self):
        for h in self.made.values():
            h.close()


@pytest.fixture(scope="module")
def handles():
    hs = _Handles()
    yield hs
    hs.close()


def _rows(h, frames, crops):
    d = h.upload(frames)
    try:
        return h.team_colors(d, len(frames), crops)
    finally:
        h.free(d)


@pytest.mark.parametrize("name", list(T.CASES))
def test_counts_equal_the_oracle(handles, name):
    case = T.CASES[name]
    got = _rows(handles(case["frame_hw"]), case["frames"], case["crops"])
    want = T.expected(name)
    bad = [(k, case["crops"][k], got[k].tolist(), want[k].tolist()) for k in range(len(want)) if not np.array_equal(got[k], want[k])]
    assert got.shape == want.shape and not bad, (name, bad[:4])
    for k in case.get("refused", ()):                    # twelve zeros, between neighbours whose rows are the oracle's
        assert not got[k].any()


@pytest.mark.parametrize("name", list(T.CASES))
def test_rows_do_not_depend_on_the_shape_of_the_call(handles, name):
    case = T.CASES[name]
    h = handles(case["frame_hw"])
    crops = case["crops"]
    d = h.upload(case["frames"])
    try:
        n = len(case["frames"])
        whole = h.team_colors(d, n, crops)
        single = np.concatenate([h.team_colors(d, n, [c]) for c in crops])
        rev = h.team_colors(d, n, crops[::-1])[::-1]
    finally:
        h.free(d)
    assert np.array_equal(whole, single) and np.array_equal(whole, rev) and np.array_equal(whole, T.expected(name))


@pytest.mark.parametrize("name", list(T.CASES))
def test_rows_repeat_on_the_same_and_on_another_handle(handles, name):
    """twice on one handle; once more on a handle of another frame size, the frames laid into its top-left corner (another row stride)"""
    case = T.CASES[name]
    fh, fw = case["frame_hw"]
    h = handles((fh, fw))
    d = h.upload(case["frames"])
    try:
        first = h.team_colors(d, len(case["frames"]), case["crops"])
        second = h.team_colors(d, len(case["frames"]), case["crops"])
    finally:
        h.free(d)
    wide = np.random.default_rng(77).integers(0, 256, (len(case["frames"]), fh + 5, fw + 3, 3), dtype=np.uint8)
    wide[:, :fh, :fw] = case["frames"]
    crops = [c for k, c in enumerate(case["crops"]) if k not in case.get("refused", ())]       # what one frame size refuses the other need not
    keep = [k for k in range(len(case["crops"])) if k not in case.get("refused", ())]
    third = _rows(handles((fh + 5, fw + 3)), wide, crops)
    assert np.array_equal(first, second) and np.array_equal(first, T.expected(name)) and np.array_equal(first[keep], third)


POISON = 0x5A5A5A5A


def test_eagle_team_colors_refuses_bad_arguments(handles):
    """argument checks only: every refused call returns before anything is launched, so none reads the clip"""
    case = T.CASES["placement"]
    h = handles(case["frame_hw"])
    d = h.upload(case["frames"])
    try:
        n, k = len(case["frames"]), len(case["crops"])
        crops = np.ascontiguousarray(case["crops"], np.int32)
        counts = np.full((k, 12), POISON, np.int32)
        cp, op = crops.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)
        call = h.L.eagle_team_colors
        for what, args in (("d_bgr == NULL", (None, n, cp, k, op)), ("n_frames < 0", (d, -1, cp, k, op)), ("n_crops < 0", (d, n, cp, -1, op)),
                           ("crops == NULL", (d, n, None, k, op)), ("counts == NULL", (d, n, cp, k, None)), ("handle == NULL", None)):
            rc = call(None, d, n, cp, k, op) if args is None else call(h._h, *args)
            assert rc == lib.E_INVALID, what
            assert (counts == POISON).all(), what
        for args in ((d, n, cp, 0, op), (d, n, None, 0, None), (d, 0, None, 0, op)):
            assert call(h._h, *args) == 0 and (counts == POISON).all()
        assert call(h._h, d, n, cp, k, op) == 0 and np.array_equal(counts, T.expected("placement"))       # the handle still works
    finally:
        h.free(d)


# ---- the host mapping ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_teams", "one_team"])
def test_team_mapping_equals_the_oracle_on_constructed_clips(handles, name):
    from oracle import colors
    m = T.MAPPINGS[name]
    h = handles(m["frame_hw"])
    d = h.upload(m["frames"])
    try:
        got = teams.get_team_mapping(h, d, m["coords"], n_frames=m["n_frames"])
    finally:
        h.free(d)
    want = colors.get_team_mapping(list(m["frames"]), m["coords"])
    assert got == want and list(got) == list(want) and len(want) >= 3, (got, want)


@pytest.mark.parametrize("name", ["zero_area", "no_colour"])
def test_team_mapping_skips_what_the_reference_raises_on(handles, name):
    """a deviation, not a comparison: on a box of zero area the reference divides by zero, on a player whose crops hit no colour range it takes
    max() of an empty dict (tests/test_team_cases_cpu.py shows both).  The library leaves such a box / such a player out and maps the others as if
    it were not there."""
    m = T.MAPPINGS[name]
    h = handles(m["frame_hw"])
    d = h.upload(m["frames"])
    try:
        got = teams.get_team_mapping(h, d, m["coords"], n_frames=m["n_frames"])
        rest = teams.get_team_mapping(h, d, T.without(m["coords"], m["skipped"]), n_frames=m["n_frames"])
    finally:
        h.free(d)
    assert got == rest == {1: 0, 2: 1, 5: 0} and not set(m["skipped"]) & set(got)
