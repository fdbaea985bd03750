"""The contract of the space stage (tests/space_ref.py), its cases (tests/space_cases.py) and the host module eagle_amd/space.py, without a GPU: every
case forces what it is named after; the two definitions (vectorised int64; a plain loop in Python integers) agree on rows of every case at one cell per
metre; ACTIVE rows conserve the grid and the owner map agrees with the counts; the refusals; space.py's figures on constructed results with and without
a possession result; JSON; the command line's refusals; the ABI."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import space_cases as SC
import space_ref as SR
from eagle_amd import lib, space

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in SC.CASES]


def test_dtypes_and_constants_are_the_library_s():
    assert (SR.ROW_DTYPE, SR.SITE_DTYPE, SR.TOTALS_DTYPE) == (lib.SPACE_ROW_DTYPE, lib.SPACE_SITE_DTYPE, lib.SPACE_TOTALS_DTYPE)
    assert (SR.SITE_CAP, SR.EMPTY, SR.ACTIVE, SR.TOO_MANY, SR.NO_OWNER) == (lib.SPACE_SITE_CAP, lib.SPACE_EMPTY, lib.SPACE_ACTIVE, lib.SPACE_TOO_MANY, lib.SPACE_NO_OWNER)
    assert [SR.ROW_DTYPE.fields[k][1] for k in ("status", "n_sites", "n", "cells", "reserved")] == [0, 4, 8, 20, 56]
    assert [SR.SITE_DTYPE.fields[k][1] for k in ("near_d2", "col", "group", "near_col", "within", "cells", "qx", "qy", "reserved")] == [0, 8, 12, 16, 20, 24, 36, 40, 44]
    assert [SR.TOTALS_DTYPE.fields[k][1] for k in ("cells", "within_sum", "col", "group", "rows", "min", "max", "opp_rows", "within_rows", "reserved")] == \
        [0, 24, 32, 36, 40, 44, 48, 52, 56, 60]
    assert [getattr(lib.EagleSpaceParams, k).offset for k in ("cells_per_metre", "goalkeepers", "radius", "reserved")] == [0, 4, 8, 16]
    head = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name, v in (("EAGLE_SPACE_SITE_CAP", 32), ("EAGLE_SPACE_EMPTY", 0), ("EAGLE_SPACE_ACTIVE", 1), ("EAGLE_SPACE_TOO_MANY", 2), ("EAGLE_SPACE_NO_OWNER", 255)):
        assert re.search(r"#define %s %d\b" % (name, v), head), name
    for name in ("eagle_post_space", "eagle_post_space_values", "eagle_post_device_space", "eagle_space_device_grids", "eagle_space_grids", "eagle_op_space"):
        assert re.search(r"\bint %s\(" % name, head) and name in lib.EXPORTS
    for text, size in (("EagleSpaceParams", 32), ("EagleSpaceRow", 64), ("EagleSpaceSite", 48), ("EagleSpaceTotals", 64)):
        assert re.search(r"\} %s;\s+/\* %d bytes \*/" % (text, size), head), text
    p = lib.space_params()
    assert C.sizeof(p) == 32 and (p.cells_per_metre, p.goalkeepers, p.radius, list(p.reserved)) == (1, 1, 3.0, [0] * 4)
    assert SR.space_params() == {"cells_per_metre": 1, "goalkeepers": 1, "radius": 3.0}


@pytest.mark.parametrize("name", NAMES)
def test_case_forces_what_it_is_named_after(name):
    assert SC.BY_NAME[name]["check"](*SC.reference(name)), name
    c = SC.BY_NAME[name]
    assert c["p"]["cells_per_metre"] < 4 or c["values"].shape[1] <= 8
    assert c["values"].shape[1] <= 20 or (c["p"]["cells_per_metre"] == 1 and SC.reference(name)[0]["n_sites"].max() <= 4)


@pytest.mark.parametrize("name", NAMES)
def test_active_rows_conserve_the_grid_and_the_map_agrees_with_the_counts(name):
    assert SC.conserves(*SC.reference(name)), name


@pytest.mark.parametrize("name", NAMES)
def test_the_two_definitions_agree(name):
    """the plain loop runs at one cell per metre on three rows of the case (the first, the middle, the last): every byte of the four outputs"""
    c = SC.BY_NAME[name]
    rows = c["values"].shape[1]
    pick = sorted({0, rows // 2, rows - 1})
    p = dict(c["p"], cells_per_metre=1)
    a = SR.space(c["values"][:, pick], c["columns"], c["mapping"], p, 0, len(pick))
    b = SR.space_scalar(c["values"][:, pick], c["columns"], c["mapping"], p, 0, len(pick))
    for x, y, what in zip(a, b, ("rows", "sites", "totals", "maps")):
        assert x.tobytes() == y.tobytes(), (name, what)
    if c["p"]["cells_per_metre"] == 1:
        ref = SC.reference(name)
        assert a[0].tobytes() == ref[0][pick].tobytes() and a[1].tobytes() == ref[1][pick].tobytes() and a[3].tobytes() == ref[3][pick].tobytes()


def test_a_window_is_a_slice_of_the_whole():
    c = SC.BY_NAME["walk_R1_12_rows_10_a_side"]
    ref = SC.reference(c["name"])
    for row0, n in ((0, 0), (3, 4), (11, 1), (12, 0)):
        out = SR.space(c["values"], c["columns"], c["mapping"], c["p"], row0, n)
        assert out[3].shape == (n, 68, 105) and out[3].tobytes() == ref[3][row0:row0 + n].tobytes() and out[0].tobytes() == ref[0].tobytes()


def test_parameters_members_and_windows_are_refused():
    c = SC.BY_NAME["goalkeepers_on"]
    for bad in (dict(cells_per_metre=0), dict(cells_per_metre=3), dict(cells_per_metre=8), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")),
                dict(radius=float("inf")), dict(radius=1024.5)):
        for fn in (SR.space, SR.space_scalar):
            with pytest.raises(ValueError):
                fn(c["values"], c["columns"], c["mapping"], dict(c["p"], **bad))
    SR.space(c["values"], c["columns"], c["mapping"], dict(c["p"], radius=1024.0))
    with pytest.raises(ValueError):
        SR.space(c["values"], c["columns"], None, c["p"])
    with pytest.raises(ValueError):
        SR.space(c["values"], [(9, 1, 0)] + c["columns"][1:], c["mapping"], c["p"])
    for row0, n in ((-1, 1), (0, 3), (2, 1), (3, 0), (0, -1)):
        with pytest.raises(ValueError):
            SR.space(c["values"], c["columns"], c["mapping"], c["p"], row0, n)
    cols = [(SC.P, 1 + i, 0) for i in range(4096)] + [(SC.G, 5000, 0)]
    mp = {1 + i: 0 for i in range(4096)}
    with pytest.raises(ValueError):
        SR.groups_of(cols, mp, 1)
    assert [len(g) for g in SR.groups_of(cols, mp, 0)] == [4096, 0, 0]


# ---- eagle_amd/space.py ------------------------------------------------------------------------------------------------------------------
def _derive(name, **kw):
    c = SC.BY_NAME[name]
    rec, st, tot, _ = SC.reference(name)
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    p = lib.space_params(**c["p"])
    return space.derive(rec, st, tot, cols, p, 100 + 2 * np.arange(c["values"].shape[1]), **kw)


def test_derived_figures_are_single_roundings_of_the_integers():
    from fractions import Fraction
    rec, st, tot, _ = SC.reference("walk_R2_6_rows_10_a_side")
    d = _derive("walk_R2_6_rows_10_a_side", per_row=True)
    assert d["params"] == {"cells_per_metre": 2, "goalkeepers": 1, "radius": 4.0} and d["rows"] == 6 and d["active_rows"] == int((rec["status"] == SR.ACTIVE).sum())
    assert len(d["ids"]) == len(tot) == 22 and [e["group"] for e in d["ids"]] == [int(t["group"]) for t in tot]
    cols = SC.BY_NAME["walk_R2_6_rows_10_a_side"]["columns"]
    for e, t in zip(d["ids"], tot):
        n, cells = int(t["rows"]), [int(v) for v in t["cells"]]
        assert e["id"] == cols[int(t["col"])][1] and e["rows"] == n and e["goalkeeper"] == (t["group"] == 2)
        if not n:
            assert e["mean_area"] is None and e["marker"] is None
            continue
        assert e["mean_area"] == float(Fraction(sum(cells), 4 * n)) and e["min_area"] == int(t["min"]) / 4 and e["max_area"] == int(t["max"]) / 4
        assert e["min_area"] <= e["mean_area"] <= e["max_area"] and e["pressed_share"] == float(Fraction(int(t["within_rows"]), n))
        assert e["thirds"] is None or e["thirds"] == [float(Fraction(v, sum(cells))) for v in cells]
        mine = (st["col"] == t["col"]) & (st["near_col"] >= 0)
        assert e["opponent_rows"] == int(mine.sum()) == int(t["opp_rows"])
        if mine.any():
            assert e["mean_nearest"] == math.fsum(math.sqrt(int(v)) / 1024 for v in st["near_d2"][mine]) / int(mine.sum())
            hist = {}
            for v in st["near_col"][mine]:
                hist[int(v)] = hist.get(int(v), 0) + 1
            assert e["marker"] == cols[min(hist, key=lambda k: (-hist[k], k))][1]
        else:
            assert e["mean_nearest"] is None and e["marker"] is None
    act = rec["status"] == SR.ACTIVE
    assert [t["group"] for t in d["teams"]] == [0, 1, 2]
    assert abs(sum(t["mean_share"] for t in d["teams"]) - 1.0) < 1e-12
    assert d["teams"][0]["mean_share"] == float(Fraction(int(rec["cells"][act, 0].sum()), int(act.sum()) * 7140 * 4))
    assert len(d["per_row"]) == 6 and d["per_row"][2]["frame"] == 104 and len(d["per_row"][0]["sites"]) == int(rec[0]["n_sites"])
    assert "possession" not in d and "passes" not in d
    assert json.loads(json.dumps(space.to_json(d))) == d


def test_possession_rows_and_passes_on_a_constructed_result():
    """radius_inclusive: column 0 owns the ball on rows 0 and 1, nobody on row 2; a pass from column 0 (release row 0) to column 1 (reception row 2)"""
    rec, st, tot, _ = SC.reference("radius_inclusive")
    owner = np.array([0, 0, -1], np.int32)
    ev = np.zeros(2, lib.EVENT_DTYPE)
    ev[0]["row"], ev[0]["from_col"], ev[0]["to_col"], ev[0]["release_row"], ev[0]["receive_row"], ev[0]["kind"] = 2, 0, 1, 0, 2, lib.EVENT_PASS
    ev[1]["kind"], ev[1]["from_col"], ev[1]["to_col"] = lib.EVENT_TURNOVER, 1, 0
    d = _derive("radius_inclusive", owner=owner, events=ev)
    assert d["possession"] == [{"row": 0, "frame": 100, "id": 1, "area": float(st[0, 0]["cells"].sum()), "within": 1},
                               {"row": 1, "frame": 102, "id": 1, "area": float(st[1, 0]["cells"].sum()), "within": 0}]
    assert d["passes"] == [{"row": 2, "release_row": 0, "receive_row": 2, "from": 1, "to": 2, "passer_within": 1, "receiver_area_release": float(st[0, 1]["cells"].sum()),
                            "receiver_area_receive": float(st[2, 1]["cells"].sum())}]
    assert d["ids"][0]["pressed_share"] == 2 / 3 and d["ids"][0]["marker"] == 2 and d["ids"][0]["mean_within"] == 2 / 3
    # an owner who is no site (the empty row) is left out; a receiver absent at the reception has no area there
    rec, st, tot, _ = SC.reference("empty_row_between")
    ev[0]["receive_row"] = 1
    d = _derive("empty_row_between", owner=np.array([1, 1, -1], np.int32), events=ev[:1])
    assert [e["row"] for e in d["possession"]] == [0] and d["passes"][0]["receiver_area_receive"] is None and d["passes"][0]["receiver_area_release"] is not None
    assert json.loads(json.dumps(space.to_json(d))) == d


def test_skipped_rows_are_reported():
    d = _derive("sites_32_active_33_too_many")
    assert d["skipped_rows"] == 1 and d["active_rows"] == 2 and d["teams"][2]["mean_share"] == 0.0 and d["teams"][2]["thirds"] is None


def test_cli_refusals(capsys):
    from eagle_amd import cli
    for argv in (["--space"], ["--processed", "--space-rows"], ["--processed", "--space-map"], ["--processed", "--space-grid", "2"], ["--processed", "--space-radius", "2"],
                 ["--processed", "--space", "--space-grid", "3"], ["--processed", "--space", "--space-radius", "0"], ["--processed", "--space", "--space-radius", "-1"],
                 ["--processed", "--space", "--space-radius", "1025"], ["--processed", "--space", "--space-radius", "nan"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
