"""The contract of the offside stage (tests/offside_ref.py), its cases (tests/offside_cases.py) and the host module eagle_amd/offside.py, without a GPU:
every case forces what it is named after; the two definitions (vectorised int64; a plain loop in Python integers) agree on every byte of every output of
every case; n_off is the count of positive margins and the line is never below the halfway line; mirroring the table and the direction mirrors nothing but
line_qx (and swaps the vote); the refusals; offside.py's figures on constructed results; JSON; the command line's refusals; the ABI."""
import ctypes as C
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import offside_cases as OC
import offside_ref as OR
import possession_ref as PR
from eagle_amd import lib, offside

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in OC.CASES]


def test_dtypes_and_constants_are_the_library_s():
    assert (OR.ROW_DTYPE, OR.TOTALS_DTYPE, OR.EVENT_DTYPE, OR.CLIP_DTYPE) == (lib.OFFSIDE_ROW_DTYPE, lib.OFFSIDE_TOTALS_DTYPE, lib.OFFSIDE_EVENT_DTYPE, lib.OFFSIDE_CLIP_DTYPE)
    assert PR.EVENT_DTYPE == lib.EVENT_DTYPE and OR.EVENT_PASS == lib.EVENT_PASS == PR.PASS
    assert [OR.ROW_DTYPE.fields[k][1] for k in ("status", "flags", "line_qx", "second_col", "n_att", "n_def", "keepers_seen", "n_off", "max_margin", "max_col", "reserved")] == \
        [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40]
    assert [OR.TOTALS_DTYPE.fields[k][1] for k in ("col", "group", "rows", "off_rows", "max_margin", "reserved")] == [0, 4, 8, 12, 16, 20]
    assert [OR.EVENT_DTYPE.fields[k][1] for k in ("status", "verdict", "margin", "line_qx", "n_off", "bypassed", "group", "reserved")] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert [OR.CLIP_DTYPE.fields[k][1] for k in ("direction", "requested", "neg", "pos", "zero", "n_members", "n_keepers")] == [0, 4, 8, 12, 16, 20, 28]
    assert [getattr(lib.EagleOffsideParams, k).offset for k in ("direction", "assume_keeper", "tolerance", "reserved")] == [0, 4, 8, 16]
    head = open(os.path.join(ROOT, "include", "eagle.h")).read()
    values = {"DIR_AUTO": 0, "DIR_RIGHT": 1, "DIR_LEFT": 2, "OK": 0, "NO_DIRECTION": 1, "TOO_FEW": 2, "KEEPER_ASSUMED": 1, "BY_DEFENDER": 2, "BY_BALL": 4, "BY_HALF": 8,
              "NO_BALL": 16, "EV_OK": 0, "EV_NOT_PASS": 1, "EV_NO_RECEIVER": 2, "EV_NO_LINE": 3, "ONSIDE": 1, "CLOSE": 2, "OFFSIDE": 3, "U_MAX": 107520, "U_HALF": 53760}
    for name, v in values.items():
        assert re.search(r"#define EAGLE_OFFSIDE_%s %d\b" % (name, v), head), name
        assert getattr(OR, name) == v == getattr(lib, "OFFSIDE_" + name), name
    assert re.search(r"#define EAGLE_OFFSIDE_NONE \(-2147483647 - 1\)", head) and OR.NONE == lib.OFFSIDE_NONE == np.iinfo(np.int32).min
    assert OR.U_MAX == 105 * 1024 == 2 * OR.U_HALF
    for name in ("eagle_post_offside", "eagle_post_offside_values", "eagle_post_offside_events", "eagle_post_device_offside", "eagle_op_offside"):
        assert re.search(r"\bint %s\(" % name, head) and name in lib.EXPORTS
    for text, size in (("EagleOffsideParams", 32), ("EagleOffsideRow", 48), ("EagleOffsideTotals", 32), ("EagleOffsideEvent", 32), ("EagleOffsideClip", 32)):
        assert re.search(r"\} %s;\s+/\* %d bytes \*/" % (text, size), head), text
    p = lib.offside_params()
    assert C.sizeof(p) == 32 and (p.direction, p.assume_keeper, p.tolerance, list(p.reserved)) == (0, 1, 0.5, [0] * 4)
    assert OR.offside_params() == {"direction": 0, "assume_keeper": 1, "tolerance": 0.5}


@pytest.mark.parametrize("name", NAMES)
def test_case_forces_what_it_is_named_after(name):
    assert OC.BY_NAME[name]["check"](*OC.reference(name)), name
    assert OC.BY_NAME[name]["values"].shape[1] <= 300


def test_most_cases_are_small_and_the_edges_are_there():
    assert sum(c["values"].shape[1] <= 8 for c in OC.CASES) >= len(OC.CASES) - 3
    assert {"members_63", "members_64", "members_65", "members_130", "rows_1", "rows_5", "rows_257", "rows_300"} <= set(NAMES)
    seen = set()
    for name in NAMES:
        rec, _, _, _, ev = OC.reference(name)
        seen |= {("row", int(s)) for s in np.unique(rec["status"])} | {("flag", b) for b in (1, 2, 4, 8, 16) if (rec["flags"] & b).any()}
        seen |= {("event", int(s)) for s in np.unique(ev["status"])} | {("verdict", int(s)) for s in np.unique(ev["verdict"])}
    assert seen == {("row", s) for s in range(3)} | {("flag", b) for b in (1, 2, 4, 8, 16)} | {("event", s) for s in range(4)} | {("verdict", s) for s in range(4)}


@pytest.mark.parametrize("name", NAMES)
def test_the_two_definitions_agree(name):
    c = OC.BY_NAME[name]
    b = OR.offside_scalar(c["values"], c["columns"], c["mapping"], c["p"], c["events"], c["no_ball"])
    for x, y, what in zip(OC.reference(name), b, OC.PARTS):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, what)


@pytest.mark.parametrize("name", NAMES)
def test_n_off_counts_the_positive_margins_and_the_line_stays_in_the_defenders_half(name):
    rec, mg, tot, clip, ev = OC.reference(name)
    assert OC.consistent(rec, mg, tot, clip, ev), name
    ok = rec["status"] == OR.OK
    assert not rec["flags"][~ok].any() and (rec["second_col"][~ok] == -1).all() and (rec["max_margin"][~ok] == OR.NONE).all() and not rec["n_off"][~ok].any()
    by = rec["flags"][ok] & (OR.BY_DEFENDER | OR.BY_BALL | OR.BY_HALF)
    assert np.isin(by, (OR.BY_DEFENDER, OR.BY_BALL, OR.BY_HALF)).all()                      # exactly one term names the line
    assert not rec["reserved"].any() and not tot["reserved"].any() and not ev["reserved"].any()
    for t, row in zip(tot, mg):
        has = row != OR.NONE
        assert (t["rows"], t["off_rows"]) == (has.sum(), (has & (row > 0)).sum()) and t["max_margin"] == (row[has].max() if has.any() else OR.NONE)


def _mirror(c):
    """the table mirrored about the halfway line on the grid of q (an absent cell stays as it is), the direction with it"""
    v = c["values"].copy()
    x, y = v[:, :, 0], v[:, :, 1]
    present = np.isfinite(x) & np.isfinite(y) & (np.abs(np.where(np.isfinite(x), x, 0)) <= 1024.0) & (np.abs(np.where(np.isfinite(y), y, 0)) <= 1024.0)
    q = np.floor(np.where(present, x, 0.0) * 1024.0 + 0.5)
    v[:, :, 0] = np.where(present, (OR.U_MAX - q) / 1024.0, x)
    d = c["p"]["direction"]
    return v, dict(c["p"], direction={OR.DIR_RIGHT: OR.DIR_LEFT, OR.DIR_LEFT: OR.DIR_RIGHT}.get(d, d)), float(np.abs(np.where(present, x, 0.0)).max())


MIRRORABLE = [n for n in NAMES if _mirror(OC.BY_NAME[n])[2] <= 900.0]      # (further out a mirrored cell would leave the domain of present cells)


@pytest.mark.parametrize("name", MIRRORABLE)
def test_mirroring_the_table_and_the_direction_mirrors_nothing_but_the_line(name):
    assert len(MIRRORABLE) >= len(NAMES) - 2
    c = OC.BY_NAME[name]
    v, p, _ = _mirror(c)
    rec, mg, tot, clip, ev = OC.reference(name)
    rec2, mg2, tot2, clip2, ev2 = OR.offside(v, c["columns"], c["mapping"], p, c["events"], c["no_ball"])
    assert mg2.tobytes() == mg.tobytes() and tot2.tobytes() == tot.tobytes()
    back, ok = rec2.copy(), rec2["status"] == OR.OK
    back["line_qx"] = np.where(ok, OR.U_MAX - rec2["line_qx"], rec2["line_qx"])
    assert back.tobytes() == rec.tobytes()
    eb, eok = ev2.copy(), ev2["status"] == OR.EV_OK
    eb["line_qx"] = np.where(eok, OR.U_MAX - ev2["line_qx"], ev2["line_qx"])
    assert eb.tobytes() == ev.tobytes()
    a, b = clip[0], clip2[0]
    swap = {0: 0, OR.DIR_RIGHT: OR.DIR_LEFT, OR.DIR_LEFT: OR.DIR_RIGHT}
    assert (b["neg"], b["pos"], b["zero"], b["direction"]) == (a["pos"], a["neg"], a["zero"], swap[int(a["direction"])]) and list(b["n_members"]) == list(a["n_members"])


def test_parameters_columns_and_events_are_refused():
    c = OC.BY_NAME["passes_at_tolerance_0.5"]
    for fn in (OR.offside, OR.offside_scalar):
        for bad in (dict(direction=3), dict(direction=-1), dict(tolerance=-0.5), dict(tolerance=float("nan")), dict(tolerance=float("inf")), dict(tolerance=1024.5)):
            with pytest.raises(ValueError):
                fn(c["values"], c["columns"], c["mapping"], dict(c["p"], **bad), c["events"])
        fn(c["values"], c["columns"], c["mapping"], dict(c["p"], tolerance=1024.0), c["events"])
        with pytest.raises(ValueError):
            fn(c["values"], c["columns"], None, c["p"])
        with pytest.raises(ValueError):
            fn(c["values"], [(9, 1, 0)] + c["columns"][1:], c["mapping"], c["p"])
        with pytest.raises(ValueError):
            fn(c["values"], c["columns"][:-1] + [(OC.P, 99, 0), (OC.BALL, 0, 0), (OC.BALL, 1, 0)], c["mapping"], c["p"])
        for field, v in (("release_row", -1), ("release_row", 4), ("receive_row", 4), ("to_col", 8), ("to_col", -1)):
            ev = c["events"].copy()
            ev[0][field] = v
            with pytest.raises(ValueError):
                fn(c["values"], c["columns"], c["mapping"], c["p"], ev)
        ev = c["events"].copy()
        ev[2]["release_row"] = 99                                                            # (an event that is no pass is not read)
        assert fn(c["values"], c["columns"], c["mapping"], c["p"], ev)[4].tobytes() == OC.reference(c["name"])[4].tobytes()
    cols = [(OC.P, 1 + i, 0) for i in range(4096)] + [(OC.G, 5000, 0)]
    with pytest.raises(ValueError):
        OR.columns_of(cols, {1 + i: 0 for i in range(4096)})
    assert [len(g) for g in OR.columns_of(cols[:-1], {1 + i: i % 2 for i in range(4096)})[:3]] == [2048, 2048, 0]
    rec, mg, tot, clip, ev = OR.offside(c["values"][:, :0], c["columns"], c["mapping"], c["p"])
    assert rec.shape == (0, 2) and mg.shape == (6, 0) and len(tot) == 6 and len(ev) == 0


# ---- eagle_amd/offside.py ----------------------------------------------------------------------------------------------------------------
def _derive(name, **kw):
    c = OC.BY_NAME[name]
    rec, mg, tot, clip, ev = OC.reference(name)
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    p = lib.offside_params(**c["p"])
    return offside.derive(rec, mg, tot, clip, cols, p, 100 + 2 * np.arange(c["values"].shape[1]), **kw)


def test_derived_figures_are_single_roundings_of_the_integers():
    name = "rows_257"
    rec, mg, tot, clip, _ = OC.reference(name)
    cols = OC.BY_NAME[name]["columns"]
    d = _derive(name, per_row=True)
    assert d["params"] == {"direction": "auto", "assume_keeper": 1, "tolerance": 0.5} and d["rows"] == 257
    assert d["clip"] == {"direction": "right", "votes": {k: int(clip[0][k]) for k in ("neg", "pos", "zero")}, "members": [3, 3], "keepers": 1}
    for a, t in enumerate(d["teams"]):
        ok = rec[:, a]["status"] == OR.OK
        assert t["group"] == a and t["ok_rows"] == int(ok.sum()) > 0 and t["too_few_rows"] == int((rec[:, a]["status"] == OR.TOO_FEW).sum())
        assert t["mean_line"] == float(Fraction(int(rec[:, a]["line_qx"][ok].astype(np.int64).sum()), int(ok.sum()) * 1024))
        assert t["offside_positions"] == int((mg[tot["group"] == a].astype(np.int64) > 0).sum()) and sum(t["line_by"].values()) == t["ok_rows"]
    for e, t in zip(d["ids"], tot):
        n = int(t["rows"])
        assert e["id"] == cols[int(t["col"])][1] and e["rows"] == n and e["offside_rows"] == int(t["off_rows"])
        assert e["offside_share"] == (float(Fraction(int(t["off_rows"]), n)) if n else None) and e["max_margin"] == (int(t["max_margin"]) / 1024 if n else None)
    assert len(d["per_row"]) == 257 and d["per_row"][3]["frame"] == 106 and "passes" not in d
    for r in (0, 100, 256):
        for a in (0, 1):
            t, o = d["per_row"][r]["teams"][a], rec[r, a]
            mine = {cols[int(tt["col"])][1]: int(mg[m, r]) for m, tt in enumerate(tot) if tt["group"] == a and mg[m, r] != OR.NONE}
            assert t["status"] == lib.OFFSIDE_STATUS_NAMES[int(o["status"])] and t["attackers"] == int(o["n_att"]) and t["defenders"] == int(o["n_def"])
            assert t["beyond"] == [{"id": i, "margin": v / 1024} for i, v in mine.items() if v > 0] and t["on_the_line"] == [i for i, v in mine.items() if v == 0]
            if o["status"] == OR.OK:
                assert t["line"] == int(o["line_qx"]) / 1024 and t["second_last"] == cols[int(o["second_col"])][1] and t["line_by"] in ("defender", "ball", "half")
            else:
                assert t["line"] is None and t["second_last"] is None and t["beyond"] == []
    assert offside.from_json(json.dumps(offside.to_json(d))) == d and offside.from_json(d) == d


def test_passes_on_a_constructed_result():
    c = OC.BY_NAME["passes_at_tolerance_0.5"]
    ev = OC.reference(c["name"])[4]
    d = _derive(c["name"], events=c["events"], offside_events=ev)
    passes = d["passes"]
    assert len(passes) == int((c["events"]["kind"] == PR.PASS).sum()) == 9 and "per_row" not in d
    assert passes[0] == {"row": 1, "release_row": 0, "receive_row": 1, "release_frame": 100, "from": 1, "to": 2, "status": "ok", "verdict": "close", "margin": 307 / 1024,
                         "line": 80.0, "teammates_offside": 1, "bypassed": 2}
    assert (passes[1]["verdict"], passes[1]["margin"]) == ("close", -307 / 1024)
    assert passes[2] == dict(passes[2], status="no_receiver", verdict=None, margin=None, line=None, teammates_offside=None, bypassed=None, to=7)
    assert [p["status"] for p in passes] == ["ok", "ok", "no_receiver", "no_line", "ok", "no_line", "ok", "ok", "ok"] and passes[7]["bypassed"] is None
    assert [p["verdict"] for p in _derive("passes_at_tolerance_0", events=c["events"], offside_events=OC.reference("passes_at_tolerance_0")[4])["passes"][:2]] == ["offside", "onside"]
    assert offside.from_json(json.dumps(offside.to_json(d))) == d
    assert "right" == _derive("forced_right")["params"]["direction"] and _derive("auto_tied")["clip"]["direction"] == "unresolved"
    assert [offside.direction_value(k) for k in ("auto", "RIGHT", "left", 2)] == [0, 1, 2, 2]
    with pytest.raises(lib.EagleError):
        offside.direction_value("up")


def test_cli_refusals(capsys):
    from eagle_amd import cli
    for argv in (["--offside"], ["--processed", "--offside-rows"], ["--processed", "--offside-direction", "left"], ["--processed", "--offside-tolerance", "1"],
                 ["--processed", "--offside-no-assumed-keeper"], ["--processed", "--offside", "--offside-direction", "up"], ["--processed", "--offside", "--offside-tolerance", "-1"],
                 ["--processed", "--offside", "--offside-tolerance", "1025"], ["--processed", "--offside", "--offside-tolerance", "nan"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
