"""The role stage on the GPU (include/eagle.h, eagle_op_roles / eagle_post_roles; csrc/roles.hip): every field of every output equals the contract of
tests/roles_ref.py — tobytes(), no tolerance — for the constructed tables of tests/roles_cases.py; NULL outputs in every combination and rows == 0; every
refusal leaves poisoned outputs alone; through a handle on tables eagle_postprocess built (a refused call after a good one leaves the good result in
place); Processor.roles and the command line."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import post_cases
import roles_cases as RC
import roles_ref as RR
from eagle_amd import lib, postprocess, roles, shape, weights

pytestmark = pytest.mark.gpu

vp = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def _equal(got, exp, what):
    for a, b, part in zip(got, exp, ("rows", "member roles", "model")):
        if a.dtype.names:
            for k in a.dtype.names:
                assert np.array_equal(a[k], b[k]), (what, part, k)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, part)


@pytest.mark.parametrize("name", [c["name"] for c in RC.CASES])
def test_op_roles_equals_contract(name):
    c = RC.BY_NAME[name]
    _equal(lib.op_roles(c["values"], c["columns"], c["mapping"], lib.role_params(**c["p"])), RC.reference(name), name)


def test_stopping_early_reports_what_all_rounds_give():
    """the launches stop at the first round that moves nothing: 12 rounds asked for, the contract runs them all"""
    c = RC.BY_NAME["iterations_12"]
    exp = RC.reference("iterations_12")
    k0 = int(np.nonzero(exp[2]["changed"][0] == 0)[0][0])
    for T in (k0, k0 + 1, 32):
        p = dict(c["p"], iterations=T)
        _equal(lib.op_roles(c["values"], c["columns"], c["mapping"], lib.role_params(**p)), RR.roles(c["values"], c["columns"], c["mapping"], p), T)


def _raw(c, mapping=True):
    values = np.ascontiguousarray(c["values"], np.float64)
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    ids = np.array(list(c["mapping"]), np.int32)
    vals = np.array(list(c["mapping"].values()), np.int32)
    return values, cols, ids, vals


def _poisoned(rows, nmem):
    rec, mr, model = np.zeros((rows, 2), lib.ROLE_ROW_DTYPE), np.full((nmem, rows), 0x5A, np.int8), np.zeros(1, lib.ROLE_MODEL_DTYPE)
    rec["n"] = 77; rec["col"] = 55; model["changed"] = 66
    return rec, mr, model


UNTOUCHED = (lambda rec: (rec["n"] == 77).all() and (rec["col"] == 55).all() and not rec["cost"].any(), lambda mr: (mr == 0x5A).all(),
             lambda model: (model["changed"] == 66).all() and not model["group"]["count"].any())


def _untouched(*out):
    return all(f(a) for f, a in zip(UNTOUCHED, out))


def test_null_outputs_in_every_combination_and_no_rows():
    L = lib.load()
    c = RC.BY_NAME["rows_65"]
    values, cols, ids, vals = _raw(c)
    rows, exp = values.shape[1], RC.reference("rows_65")
    p = lib.role_params(**c["p"])
    args = (0, vp(values), vp(cols), rows, len(cols), vp(ids), vp(vals), len(ids), C.byref(p))
    for want in itertools.product((False, True), repeat=3):
        out = _poisoned(rows, exp[1].shape[0])
        assert L.eagle_op_roles(*args, *[vp(a) if w else None for a, w in zip(out, want)]) == 0, want
        for a, b, w, alone in zip(out, exp, want, UNTOUCHED):
            assert a.tobytes() == b.tobytes() if w else alone(a), want
    out = _poisoned(rows, exp[1].shape[0])
    assert L.eagle_op_roles(0, vp(values), vp(cols), 0, len(cols), vp(ids), vp(vals), len(ids), C.byref(p), *map(vp, out)) == 0      # rows == 0: nothing written
    assert _untouched(*out)
    rec, mr, model = lib.op_roles(values[:, :0], c["columns"], c["mapping"], p)
    assert rec.shape == (0, 2) and mr.shape == (exp[1].shape[0], 0) and not model["changed"].any()


def test_first_mapping_entry_counts():
    L = lib.load()
    c = RC.BY_NAME["rows_63"]
    values, cols, ids, vals = _raw(c)
    ids2, vals2 = np.concatenate([ids, ids]).astype(np.int32), np.concatenate([vals, 2 - vals]).astype(np.int32)      # later, contradicting entries
    exp = RC.reference("rows_63")
    out = _poisoned(values.shape[1], exp[1].shape[0])
    p = lib.role_params(**c["p"])
    assert L.eagle_op_roles(0, vp(values), vp(cols), values.shape[1], len(cols), vp(ids2), vp(vals2), len(ids2), C.byref(p), *map(vp, out)) == 0
    _equal(out, exp, "first entry")
    _equal(lib.op_roles(c["values"], c["columns"], dict(zip(ids2.tolist()[::-1], vals2.tolist()[::-1])), p), exp, "the wrapper's member count")


def test_refusals_leave_the_outputs_alone():
    L = lib.load()
    c = RC.BY_NAME["roles_5"]
    values, cols, ids, vals = _raw(c)
    rows = values.shape[1]
    out = _poisoned(rows, 5)

    def op(p=lib.role_params(5, 5, 4), values_a=values, cols_a=cols, ids_a=ids, ncols=None, par=True):
        rc = L.eagle_op_roles(0, vp(values_a), vp(cols_a), rows, len(cols) if ncols is None else ncols, vp(ids_a), vp(vals), len(ids), C.byref(p) if par else None,
                              *map(vp, out))
        return rc, L.eagle_last_error(None).decode()

    unknown = cols.copy(); unknown[2]["kind"] = 9
    reserved = lib.role_params(5, 5, 4); reserved.reserved[3] = 1
    for kw in (dict(par=False), dict(ids_a=None), dict(values_a=None), dict(cols_a=None), dict(cols_a=unknown), dict(p=reserved), dict(p=lib.role_params(1, 1, 4)),
               dict(p=lib.role_params(11, 8, 4)), dict(p=lib.role_params(5, 1, 4)), dict(p=lib.role_params(5, 6, 4)), dict(p=lib.role_params(5, 5, 0)),
               dict(p=lib.role_params(5, 5, 33)), dict(ncols=-1)):
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and msg and _untouched(*out), kw
    # 4097 members (4096 pass)
    bc = np.array([(lib.POST_PLAYER, 1 + i, 0, 0) for i in range(4097)], lib.POSTCOL_DTYPE)
    bi, bv, bvals = np.arange(1, 4098, dtype=np.int32), np.zeros(4097, np.int32), np.zeros((4097, 1, 2))
    big = _poisoned(1, 4097)
    p = lib.role_params(5, 5, 2)
    assert L.eagle_op_roles(0, vp(bvals), vp(bc), 1, 4097, vp(bi), vp(bv), 4097, C.byref(p), *map(vp, big)) == lib.E_INVALID and _untouched(*big)
    assert L.eagle_op_roles(0, vp(bvals), vp(bc), 1, 4096, vp(bi), vp(bv), 4096, C.byref(p), *map(vp, big)) == 0
    assert big[0][0, 0]["n"] == 4096 and big[0][0, 0]["status"] == lib.ROLE_TOO_MANY and big[2]["group"][0, 0]["status"] == lib.ROLE_NO_SEEDS and (big[1][:4096] == -1).all()
    assert op()[0] == 0 and out[0].tobytes() == RC.reference("roles_5")[0].tobytes()


# ---- through a handle -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


def _walk_records(n, players, keepers, seed=3):
    """n records of `players` players, `keepers` goalkeepers and the ball on a random walk (ids are detection index + 1)"""
    r = np.random.default_rng(seed)
    k = players + keepers + 1
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = k, 1, 1
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    pos = np.clip(np.stack([r.uniform(5, 100, k), r.uniform(5, 63, k)], 1)[None] + np.cumsum(r.normal(0, 1.0, (n, k, 2)), 0), 0, [105, 68])
    d, j = recs["det"], np.arange(k)
    d["reported"][:, :k], d["in_bounds"][:, :k], d["conf"][:, :k] = 1, 1, 0.9
    d["cls"][:, :k] = np.where(j == k - 1, 2, np.where(j >= players, 1, 0))[None]
    d["id"][:, :k] = (j + 1)[None]
    d["bx1"][:, :k], d["bx2"][:, :k], d["by1"][:, :k], d["by2"][:, :k] = (4 * j)[None], (4 * j + 3)[None], 300, 340
    d["pitch_x"][:, :k], d["pitch_y"][:, :k] = pos[:, :, 0].astype(np.int32), pos[:, :, 1].astype(np.int32)
    return recs


def test_handle_on_a_walk_of_two_teams(handle):
    """a table eagle_postprocess builds from 12 players: six roles per team through the handle entries; a second call replaces the result, a refused one
    leaves it in place"""
    t = handle.postprocess(_walk_records(9, 12, 2), 25, 1280, {i + 1: i % 2 for i in range(12)})
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        assert handle.roles_device(t) == (None, None, None, 0)
        assert handle.L.eagle_post_roles_values(t._t, None, None, None) == lib.E_INVALID                       # no result yet
        p6 = RR.role_params(6, 5, 5)
        got = handle.roles(t, lib.role_params(**p6))
        exp = RR.roles(values, cols, t.team_mapping, p6)
        print("rows", rows, "members", got[1].shape[0], "active", exp[2]["group"][0]["active_rows"], "changed", exp[2]["changed"][0][:5])
        assert rows >= 3 and exp[2]["group"][0]["active_rows"].min() >= 3 and (exp[2]["group"][0]["status"] == RR.MODEL_OK).all()
        _equal(got, exp, "handle")
        _equal(got, lib.op_roles(values, cols, t.team_mapping, lib.role_params(**p6)), "handle against the operator entry")
        a, b, c, n = handle.roles_device(t)
        assert a and b and c and n == 12
        p3 = RR.role_params(3, 2, 2)
        second = handle.roles(t, lib.role_params(**p3))                                                       # (all rows TOO_MANY: another result altogether)
        _equal(second, RR.roles(values, cols, t.team_mapping, p3), "second call")
        assert second[0].tobytes() != got[0].tobytes()
        bad = lib.role_params(3, 4, 2)
        assert handle.L.eagle_post_roles(handle._h, t._t, C.byref(bad)) == lib.E_INVALID and "min_present" in handle.L.eagle_last_error(handle._h).decode()
        assert handle.L.eagle_post_roles(handle._h, t._t, None) == lib.E_INVALID
        kept = _poisoned(rows, 12)
        assert handle.L.eagle_post_roles_values(t._t, *map(vp, kept)) == 0                                    # the refused calls left the good result in place
        _equal(kept, second, "kept")
        assert handle.roles_device(t) == (a, b, c, n)
        assert np.array_equal(np.array(t.values), values, equal_nan=True)
    finally:
        t.close()


def test_handle_on_a_post_case_equals_the_operator_entry(handle):
    case = post_cases.BY_NAME["would_merge_same_team"]
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], case["team_mapping"])
    bare = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], None)
    try:
        values, cols = np.array(t.values), _columns(t)
        p = RR.role_params(2, 2, 3)
        got = handle.roles(t, lib.role_params(**p))
        print("rows", len(t.rows), "members", got[1].shape[0], "status", got[0]["status"].T.tolist())
        _equal(got, lib.op_roles(values, cols, t.team_mapping, lib.role_params(**p)), "operator entry")
        _equal(got, RR.roles(values, cols, t.team_mapping, p), "contract")
        pr = lib.role_params(2, 2, 3)
        assert handle.L.eagle_post_roles(handle._h, bare._t, C.byref(pr)) == lib.E_INVALID and "mapping" in handle.L.eagle_last_error(handle._h).decode()
        assert handle.roles_device(bare) == (None, None, None, 0)
        assert handle.L.eagle_post_roles(handle._h, None, C.byref(pr)) == lib.E_INVALID and handle.L.eagle_post_roles(None, t._t, C.byref(pr)) == lib.E_INVALID
    finally:
        t.close(); bare.close()


def test_processor_roles(handle):
    import types

    from eagle_amd.processor import Processor
    pr = Processor(types.SimpleNamespace(handle=handle))
    t = handle.postprocess(_walk_records(9, 12, 2), 25, 1280, {i + 1: i % 2 for i in range(12)})
    try:
        d = pr.roles(t, roles=6, min_present=5, iterations=5, lines=3, per_row=True)
        values, cols = np.array(t.values), _columns(t)
        rec, mr, model = RR.roles(values, cols, t.team_mapping, RR.role_params(6, 5, 5))
        assert handle.team_shape_device(t)[0]                                                                # (the shape was computed for the orientation)
        left = shape.shape(handle, t)["clip"]["defends_left"]
        exp = roles.derive(rec, mr, model, t.columns, shape.member_columns(t.columns, t.team_mapping), lib.role_params(6, 5, 5), t.rows, left, 3, True)
        assert d == exp and len(d["rows"]) == len(t.rows) and [len(g["roles"]) for g in d["groups"]] == [6, 6]
        assert pr.roles(t, roles=6, min_present=5, iterations=5) == {k: v for k, v in exp.items() if k != "rows"}     # (with the shape already there)
    finally:
        t.close()


def test_cli_roles(tmp_path):
    from eagle_amd import cli
    out = str(tmp_path / "out")
    common = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed"]
    assert cli.main(common + ["--roles", "--roles-count", "2", "--roles-min-present", "2", "--roles-iterations", "3", "--roles-lines", "2", "--roles-rows"]) == 0
    rows = len(json.load(open(os.path.join(out, "processed_data.json"))))
    j = json.load(open(os.path.join(out, "roles.json")))
    d = roles.from_json(j)
    assert d == j and roles.to_json(d) == j and len(d["rows"]) == rows and len(d["groups"]) == 2
    assert d["params"] == {"roles": 2, "min_present": 2, "iterations": 3, "lines": 2} and len(d["changed"]) == 3
    assert cli.main(common + ["--roles"]) == 0 and "rows" not in json.load(open(os.path.join(out, "roles.json")))
