"""The contract of the role stage (tests/roles_ref.py), its cases (tests/roles_cases.py) and the host module eagle_amd/roles.py, without a GPU: every
case forces what it is named after; the two definitions (subset layers in int64; permutations in Python integers) agree on every case; the subset
recurrence against itertools.permutations on 300 small problems with heavy ties and against scipy's cost at ten roles; stopping at the fixed point gives
what all the rounds give; roles.py's lines, labels, swaps and stints; JSON; the command line's refusals; the ABI."""
import ctypes as C
import itertools
import json
import os
import re

import numpy as np
import pytest

import roles_cases as RC
import roles_ref as RR
from eagle_amd import lib, roles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in RC.CASES]


def test_dtypes_and_constants_are_the_library_s():
    assert (RR.ROW_DTYPE, RR.GROUP_DTYPE, RR.MODEL_DTYPE) == (lib.ROLE_ROW_DTYPE, lib.ROLE_GROUP_DTYPE, lib.ROLE_MODEL_DTYPE)
    assert (RR.ROLE_CAP, RR.EMPTY, RR.TOO_FEW, RR.ACTIVE, RR.TOO_MANY, RR.MODEL_OK, RR.NO_SEEDS) == (lib.ROLE_CAP, lib.ROLE_EMPTY, lib.ROLE_TOO_FEW, lib.ROLE_ACTIVE,
                                                                                                       lib.ROLE_TOO_MANY, lib.ROLE_MODEL_OK, lib.ROLE_NO_SEEDS)
    head = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name, v in (("EAGLE_ROLE_CAP", 10), ("EAGLE_ROLE_EMPTY", 0), ("EAGLE_ROLE_TOO_FEW", 1), ("EAGLE_ROLE_ACTIVE", 2), ("EAGLE_ROLE_TOO_MANY", 3),
                    ("EAGLE_ROLE_MODEL_OK", 0), ("EAGLE_ROLE_NO_SEEDS", 1)):
        assert re.search(r"#define %s %d\b" % (name, v), head), name
    for name in ("eagle_post_roles", "eagle_post_roles_values", "eagle_post_device_roles", "eagle_op_roles"):
        assert re.search(r"\bint %s\(" % name, head) and name in lib.EXPORTS
    for text, size in (("EagleRoleParams", 32), ("EagleRoleRow", 64), ("EagleRoleGroup", 448), ("EagleRoleModel", 1024)):
        assert re.search(r"\} %s;\s+/\* %d bytes \*/" % (text, size), head), text
    p = lib.role_params()
    assert C.sizeof(p) == 32 and (p.roles, p.min_present, p.iterations) == (10, 8, 8) and RR.role_params() == {"roles": 10, "min_present": 8, "iterations": 8}


@pytest.mark.parametrize("name", NAMES)
def test_case_forces_what_it_is_named_after(name):
    assert RC.BY_NAME[name]["check"](*RC.reference(name)), name
    c = RC.BY_NAME[name]
    assert c["p"]["roles"] < 10 or c["values"].shape[1] <= 16
    assert c["values"].shape[1] <= 64 or c["p"]["roles"] <= 5


@pytest.mark.parametrize("name", NAMES)
def test_the_two_definitions_agree(name):
    """int64 and subset layers against Python integers and permutations, the domain's corners among the cases"""
    c = RC.BY_NAME[name]
    got = RR.roles_scalar(c["values"], c["columns"], c["mapping"], c["p"])
    for a, b, what in zip(got, RC.reference(name), ("rows", "member roles", "model")):
        assert a.tobytes() == b.tobytes(), (name, what)


def test_subset_recurrence_is_the_first_least_permutation():
    """300 seeded problems, costs drawn from {0 .. 3}: ties everywhere"""
    r = np.random.default_rng(29)
    for _ in range(300):
        R = int(r.integers(2, 7))
        n = int(r.integers(1, R + 1))
        c = r.integers(0, 4, (n, R))
        cost, best = min((sum(int(c[i, s[i]]) for i in range(n)), s) for s in itertools.permutations(range(R), n))
        sig, h0 = RR.assign_costs(c[None].astype(np.int64), R)
        assert (tuple(sig[0]), int(h0[0])) == (best, cost)
        assert RR.assign_permutations([[int(v) for v in row] for row in c], R) == (best, cost)


def test_assign_layers_on_points_is_the_first_least_permutation():
    """the vectorised definition itself, on points of a coarse lattice (equal distances abound), against itertools.permutations"""
    r = np.random.default_rng(30)
    for _ in range(60):
        R = int(r.integers(2, 6))
        n = int(r.integers(1, R + 1))
        u, M = r.integers(-2, 3, (4, n, 2)), r.integers(-2, 3, (R, 2))
        sig, cost = RR.assign_layers(u[:, :, 0].astype(np.int64), u[:, :, 1].astype(np.int64), M.astype(np.int64), R)
        for row in range(4):
            c = ((u[row][:, None, :] - M[None]) ** 2).sum(2)
            exp = min((sum(int(c[i, s[i]]) for i in range(n)), s) for s in itertools.permutations(range(R), n))
            assert (int(cost[row]), tuple(sig[row])) == exp


def test_cost_is_scipy_s_at_ten_roles():
    from scipy.optimize import linear_sum_assignment
    r = np.random.default_rng(31)
    for k in range(20):
        n = 10 if k % 2 else 8
        u, M = r.integers(-2 ** 21, 2 ** 21, (1, n, 2)), r.integers(-2 ** 21, 2 ** 21, (10, 2))
        sig, cost = RR.assign_layers(u[:, :, 0], u[:, :, 1], M, 10)
        c = ((u[0][:, None, :] - M[None]) ** 2).sum(2)
        ri, ci = linear_sum_assignment(c)
        assert int(cost[0]) == int(c[ri, ci].sum()) == sum(int(c[i, sig[0, i]]) for i in range(n)) and len(set(sig[0])) == n
        assert int(c.max()) > 2 ** 42


def test_stopping_at_the_fixed_point_gives_what_all_rounds_give():
    c = RC.BY_NAME["iterations_12"]
    full = RC.reference("iterations_12")
    changed = full[2]["changed"][0]
    k0 = int(np.nonzero(changed[:12] == 0)[0][0])
    assert 1 <= k0 < 11 and not changed[k0:].any()
    for T in (k0 + 1, k0 + 2):
        part = RR.roles(c["values"], c["columns"], c["mapping"], dict(c["p"], iterations=T))
        assert part[0].tobytes() == full[0].tobytes() and part[1].tobytes() == full[1].tobytes()
        assert part[2]["group"].tobytes() == full[2]["group"].tobytes() and list(part[2]["changed"][0]) == list(changed)
    early = RR.roles(c["values"], c["columns"], c["mapping"], dict(c["p"], iterations=k0))     # one round short of seeing the 0: still moving
    assert early[2]["changed"][0, k0 - 1] > 0
    one = RC.reference("iterations_1")
    assert one[2]["changed"][0, 0] == changed[0] and one[0].tobytes() != full[0].tobytes()


def test_parameters_and_members_are_refused():
    c = RC.BY_NAME["roles_3"]
    for bad in (dict(roles=1), dict(roles=11), dict(min_present=1), dict(min_present=4), dict(iterations=0), dict(iterations=33)):
        with pytest.raises(ValueError):
            RR.roles(c["values"], c["columns"], c["mapping"], dict(c["p"], **bad))
    with pytest.raises(ValueError):
        RR.roles(c["values"], c["columns"], None, c["p"])
    with pytest.raises(ValueError):
        RR.roles(c["values"], [(9, 1, 0)] + c["columns"][1:], c["mapping"], c["p"])


# ---- eagle_amd/roles.py -----------------------------------------------------------------------------------------------------------------
def test_lines_and_labels_on_hand_built_means():
    f442 = [10, 11, 9, 10, 30, 31, 29, 30, 50, 52]
    assert roles.label_of(roles.split_lines(f442)[1]) == "4-4-2"
    f433 = [10, 30, 50, 11, 31, 51, 9, 29, 49, 10]
    order, lines = roles.split_lines(f433)
    assert roles.label_of(lines) == "4-3-3" and sorted(lines[0]) == [0, 3, 6, 9] and order[0] == 6
    assert roles.label_of(roles.split_lines([5, 6, 7, 25, 26, 27, 28, 29, 50, 51])[1]) == "3-5-2"
    assert roles.label_of(roles.split_lines([5, 6, 7, 25, 26, 27, 28, 29, 50, 51], 2)[1]) == "8-2"                  # (the one largest gap: 21 against 18)
    assert roles.label_of(roles.split_lines([0, 10, 20, 21, 40, 41, 42, 60, 61, 62], 4)[1]) == "1-3-3-3"     # gaps 10, 10, 19, 18: the three largest, the tie to the back
    # equal gaps: the cut nearer the own goal.  depths 0, 10, 20, 30: three gaps of 10, two cuts -> after the first and the second role
    assert roles.split_lines([0, 10, 20, 30])[1] == [[0], [1], [2, 3]]
    assert roles.split_lines([30, 20, 10, 0], 2)[1] == [[3], [2, 1, 0]]
    assert roles.split_lines([7, 7, 7], 2) == ([0, 1, 2], [[0], [1, 2]])                                     # equal depths: by role
    for bad in (1, 5):
        with pytest.raises(ValueError):
            roles.split_lines(f442, bad)
    with pytest.raises(ValueError):
        roles.split_lines([1, 2], 3)


def _derive(name, defends_left=(True, False), **kw):
    c = RC.BY_NAME[name]
    rec, mr, model = RC.reference(name)
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    import shape_ref as SR
    p = lib.role_params(**c["p"])
    frames = 100 + 2 * np.arange(c["values"].shape[1])
    return roles.derive(rec, mr, model, cols, SR.members(c["columns"], c["mapping"]), p, frames, defends_left, **kw)


def test_exchange_is_two_swaps_and_fragment_is_a_stint_boundary():
    d = _derive("exchange")
    assert d["swaps"] == [{"row": 14, "frame": 128, "id": 1, "from": 0, "to": 1}, {"row": 14, "frame": 128, "id": 2, "from": 1, "to": 0}]
    assert d["stints"][0][0] == [[0, 13, 1], [14, 19, 2]] and d["stints"][0][1] == [[0, 13, 2], [14, 19, 1]] and d["stints"][0][2] == [[0, 19, 3]]
    assert [e["rows"] for e in d["ids"]] == [[14, 6, 0], [6, 14, 0], [0, 0, 20]]
    d = _derive("fragment_replaced")
    assert d["swaps"] == [] and d["stints"][0][2] == [[0, 9, 3], [12, 19, 4]] and d["stints"][0][0] == [[0, 19, 1]]
    assert d["groups"][0]["active_share"] == 1.0 and d["groups"][1]["status"] == "no_seeds" and d["groups"][1]["label"] is None and d["groups"][1]["roles"] == []


def test_derived_floats_orientation_and_json():
    from fractions import Fraction
    import math
    rec, mr, model = RC.reference("ten_roles_two_teams")
    d = _derive("ten_roles_two_teams", per_row=True)
    for g in (0, 1):
        mg, dg = model["group"][0, g], d["groups"][g]
        assert dg["label"] == "4-4-2" and dg["oriented"] and sorted(dg["order"]) == list(range(10))
        for j, e in enumerate(dg["roles"]):
            n, sx, sy, sxx, syy = (int(v) for v in (mg["count"][j], mg["sum"][j][0], mg["sum"][j][1], mg["sum2"][j][0], mg["sum2"][j][1]))
            assert e["mean"] == [float(Fraction(int(mg["mean"][j][0]), 1024)), float(Fraction(int(mg["mean"][j][1]), 1024))] and e["count"] == n > 0
            assert e["depth"] == (e["mean"][0] if g == 0 else -e["mean"][0])                                     # group 1 defends the right: mirrored
            assert e["spread"] == math.sqrt(float(Fraction(n * (sxx + syy) - sx * sx - sy * sy, n * n * 1024 * 1024)))
            assert e["played"] == [float(Fraction(sx, n * 1024)), float(Fraction(sy, n * 1024))]
    assert len(d["rows"]) == 12 and d["rows"][3]["frame"] == 106 and d["rows"][0]["groups"][0]["status"] in lib.ROLE_STATUS_NAMES
    assert d["changed"] == [int(v) for v in model["changed"][0][:6]]
    assert sum(sum(e["rows"]) for e in d["ids"]) == int((mr >= 0).sum())
    j = json.loads(json.dumps(roles.to_json(d)))
    assert roles.from_json(j) == d
    unknown = _derive("ten_roles_two_teams", defends_left=None)
    assert [g["label"] for g in unknown["groups"]] == [None, None] and not unknown["groups"][0]["oriented"] and unknown["groups"][0]["lines"] == d["groups"][0]["lines"]
    assert unknown["swaps"] == d["swaps"] and unknown["stints"] == d["stints"]
    flipped = _derive("ten_roles_two_teams", defends_left=(False, True))
    assert flipped["groups"][0]["label"] == "2-4-4"


def test_cli_refusals(capsys):
    from eagle_amd import cli
    for argv in (["--roles"], ["--processed", "--roles-rows"], ["--processed", "--roles-count", "5"], ["--processed", "--roles", "--roles-count", "11"],
                 ["--processed", "--roles", "--roles-count", "5", "--roles-min-present", "6"], ["--processed", "--roles", "--roles-iterations", "0"],
                 ["--processed", "--roles", "--roles-lines", "5"], ["--processed", "--roles", "--roles-count", "2", "--roles-lines", "3"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
