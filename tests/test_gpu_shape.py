"""The team-shape stage and the minimap's hull layer on the GPU (include/eagle.h, eagle_op_team_shape / eagle_op_minimap_hulls / eagle_post_team_shape /
eagle_minimap_set_hulls; csrc/shape.hip, csrc/minimap.hip): every record, every hull vertex and every picture byte equals the contract of
tests/shape_ref.py — no tolerances — for the constructed tables of tests/shape_cases.py; NULL outputs and rows == 0; through a handle on a table
eagle_postprocess built; layers = 7 through the new entry is eagle_op_minimap_trails; every refusal leaves the output alone; the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import annot_ref as A
import minimap_ref as R
import post_cases
import shape_cases as SC
import shape_ref as SR
from eagle_amd import lib, postprocess, shape, weights

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in SC.CASES])
def test_op_team_shape_equals_contract(name):
    c = SC.BY_NAME[name]
    rec, hl = lib.op_team_shape(c["values"], c["columns"], c["mapping"])
    exp_rec, exp_hl = SC.reference(name)
    for k in SR.SHAPE_DTYPE.names:
        assert np.array_equal(rec[k], exp_rec[k]), (name, k)
    assert rec.tobytes() == exp_rec.tobytes() and np.array_equal(hl, exp_hl)


def _raw(c):
    values = np.ascontiguousarray(c["values"], np.float64)
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    ids = np.array(list(c["mapping"]), np.int32)
    vals = np.array(list(c["mapping"].values()), np.int32)
    return values, cols, ids, vals


vp = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def test_null_outputs_and_no_rows():
    L = lib.load()
    c = SC.BY_NAME["rows_63"]
    values, cols, ids, vals = _raw(c)
    rows = values.shape[1]
    exp_rec, exp_hl = SC.reference("rows_63")
    rec, hl = np.zeros((rows, 2), lib.SHAPE_DTYPE), np.zeros((rows, 2, 32), np.int32)
    args = (0, vp(values), vp(cols), rows, len(cols), vp(ids), vp(vals), len(ids))
    assert L.eagle_op_team_shape(*args, vp(rec), None) == 0 and rec.tobytes() == exp_rec.tobytes()
    assert L.eagle_op_team_shape(*args, None, vp(hl)) == 0 and np.array_equal(hl, exp_hl)
    assert L.eagle_op_team_shape(*args, None, None) == 0
    rec[:] = 0; rec["n"] = 77; hl[:] = 55
    assert L.eagle_op_team_shape(0, vp(values), vp(cols), 0, len(cols), vp(ids), vp(vals), len(ids), vp(rec), vp(hl)) == 0      # rows == 0: nothing written
    assert (rec["n"] == 77).all() and (hl == 55).all()


def test_first_mapping_entry_counts():
    L = lib.load()
    c = SC.BY_NAME["team_values"]
    values, cols, ids, vals = _raw(c)
    ids2, vals2 = np.concatenate([ids, ids]).astype(np.int32), np.concatenate([vals, 1 - np.abs(vals)]).astype(np.int32)      # later, contradicting entries
    rec, hl = np.zeros((1, 2), lib.SHAPE_DTYPE), np.zeros((1, 2, 32), np.int32)
    assert L.eagle_op_team_shape(0, vp(values), vp(cols), 1, len(cols), vp(ids2), vp(vals2), len(ids2), vp(rec), vp(hl)) == 0
    assert rec.tobytes() == SC.reference("team_values")[0].tobytes() and np.array_equal(hl, SC.reference("team_values")[1])


# ---- the picture ------------------------------------------------------------------------------------------------------------------
def _hulls(c, layers, fmt="bgr", layout=None, out=None):
    par = lib.minimap_params(c["S"], c["M"], layers=layers)
    p = c["p"]
    trail = lib.trail_params(p["window"], p["max_gap"], p["half_width"], p["pass_hold"], p["dim_floor"]) if layers & 7 else None
    return lib.op_minimap_hulls(c["values"], c["frames"], c["columns"], c["mapping"], par, lib.hull_params(c["hull_hw"]) if layers & 8 else None, trail, c["sel"], c["owner"],
                                c["events"], c["row0"], c["n"], fmt, layout, out)


@pytest.mark.parametrize("layers", [8, 9, 12, 15])
def test_op_minimap_hulls_equals_contract(layers):
    got = _hulls(SC.picture_case(), layers)
    exp = SC.picture_reference(layers)
    assert got.shape == exp.shape == (3, 136, 210, 3) and np.array_equal(got, exp)
    assert not np.array_equal(exp, SC.picture_reference(layers & 7))          # the hulls show


@pytest.mark.parametrize("fmt", ["bgr", "i420"])
def test_op_minimap_hulls_large_and_yuv(fmt):
    c = SC.picture_case((4, 2))
    fr = SC.picture_reference(15, True)
    assert np.array_equal(_hulls(c, 15, fmt).reshape(-1), A.annotate(fr, [[] for _ in fr], fmt))


def test_layers_7_is_eagle_op_minimap_trails():
    c = SC.picture_case()
    p = c["p"]
    trail = lib.trail_params(p["window"], p["max_gap"], p["half_width"], p["pass_hold"], p["dim_floor"])
    old = lib.op_minimap_trails(c["values"], c["frames"], c["columns"], c["mapping"], lib.minimap_params(c["S"], c["M"], layers=7), trail, c["sel"], c["owner"], c["events"],
                                c["row0"], c["n"])
    assert np.array_equal(_hulls(c, 7), old) and np.array_equal(old, SC.picture_reference(7))
    assert np.array_equal(_hulls(c, 0), lib.op_minimap(c["values"], c["columns"], c["mapping"], lib.minimap_params(c["S"], c["M"]), c["row0"], c["n"]))


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
    """a table eagle_postprocess builds from 12 players: real polygons through the handle entries and the hull layer"""
    t = handle.postprocess(_walk_records(9, 12, 2), 25, 1280, {i + 1: i % 2 for i in range(12)})
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        rec, hl = handle.team_shape(t)
        exp_rec, exp_hl = SR.shape(values, cols, t.team_mapping)
        print("rows", rows, "members", [len(g) for g in SR.members(cols, t.team_mapping)], "hull_n", exp_rec["hull_n"].min(), exp_rec["hull_n"].max())
        assert rows >= 3 and exp_rec["hull_n"].min() >= 3
        assert rec.tobytes() == exp_rec.tobytes() and np.array_equal(hl, exp_hl)
        handle.set_hulls(t, 1)
        ref = SR.frames_bgr(values, np.asarray(t.rows, np.int32), cols, t.team_mapping, 0, rows, 2, 2, layers=8, hull_hw=1)
        assert np.array_equal(handle.minimap(t, lib.minimap_params(2, 2, layers=8)), ref)
        assert not np.array_equal(ref, handle.minimap(t, lib.minimap_params(2, 2)))
    finally:
        t.close()


def test_handle_equals_contract(handle):
    case = post_cases.BY_NAME["goalkeeper_fold"]
    tm = case["team_mapping"]
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], tm)
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        assert handle.team_shape_device(t) == (None, None)
        rec, hl = handle.team_shape(t)
        exp_rec, exp_hl = SR.shape(values, cols, t.team_mapping)
        print("rows", rows, "members", [len(g) for g in SR.members(cols, t.team_mapping)], "present", exp_rec["n"].sum(0), "hull_n max", exp_rec["hull_n"].max())
        assert exp_rec["n"].sum() > 0
        assert rec.tobytes() == exp_rec.tobytes() and np.array_equal(hl, exp_hl)
        a, b = handle.team_shape_device(t)
        assert a and b
        d = shape.shape(handle, t)                              # (a second call replaces the first)
        assert len(d["rows"]) == rows and d["rows"][0]["groups"][0]["n"] == int(exp_rec[0, 0]["n"])
        # the hull layer: alone, and over the trails
        S, M = 2, 2
        fr = np.asarray(t.rows, np.int32)
        plain = handle.minimap(t, lib.minimap_params(S, M))
        handle.set_hulls(t, 2)
        ref = SR.frames_bgr(values, fr, cols, t.team_mapping, 0, rows, S, M, layers=8, hull_hw=2)
        assert np.array_equal(handle.minimap(t, lib.minimap_params(S, M, layers=8)), ref)
        sel = [c for c, (k, _, v) in enumerate(cols) if not v and k in (R.PLAYER, R.GOALKEEPER, R.BALL)]
        import trails_ref as T
        p = T.trail_params(window=4, max_gap=case["fps"], half_width=1)
        handle.minimap_set_trails(t, lib.trail_params(p["window"], p["max_gap"], p["half_width"], p["pass_hold"], p["dim_floor"]), sel)
        ref9 = SR.frames_bgr(values, fr, cols, t.team_mapping, 0, rows, S, M, layers=9, p=p, sel=sel, hull_hw=2)
        assert np.array_equal(handle.minimap(t, lib.minimap_params(S, M, layers=9), 2, 3, "i420").reshape(-1), A.annotate(ref9[2:5], [[]] * 3, "i420"))
        from eagle_amd import minimap as mm
        assert np.array_equal(mm.minimap(handle, t, S, M, hulls=2, rows=(1, 2)), ref[1:3])
        assert np.array_equal(handle.minimap(t, lib.minimap_params(S, M)), plain) and np.array_equal(np.array(t.values), values, equal_nan=True)
    finally:
        t.close()


def test_refusals(handle):
    L = handle.L
    c = SC.picture_case()
    values, cols, ids, vals = _raw(c)
    rows = values.shape[1]
    w, h = R.size(2, 0)
    out = np.full(w * h * 3, 0x5A, np.uint8)
    frames = np.arange(rows, dtype=np.int32)

    def op(layers=8, hw=1, hp=True, ids_a=ids, frames_a=frames, cols_a=cols, values_a=values, out_a=out, par=True):
        p = lib.minimap_params(2, 0, layers=layers)
        hpar = lib.hull_params(hw)
        rc = L.eagle_op_minimap_hulls(0, vp(values_a), vp(frames_a), vp(cols_a), rows, len(cols_a), vp(ids_a), vp(vals), len(ids), C.byref(p) if par else None,
                                      C.byref(hpar) if hp else None, None, None, 0, None, None, 0, 0, 1, 0, None, vp(out_a))
        msg = L.eagle_last_error(None).decode()
        assert (out == 0x5A).all() or rc == 0
        return rc, msg

    unknown = cols.copy(); unknown[5]["kind"] = 9
    for kw in (dict(hw=0), dict(hw=9), dict(hp=False), dict(ids_a=None), dict(frames_a=frames[::-1]), dict(cols_a=unknown), dict(values_a=None), dict(out_a=None),
               dict(par=False), dict(layers=16), dict(layers=9)):      # (9: trails without trail parameters)
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and msg, kw
    # 4097 members (4096 pass)
    big_cols, big_map = SC.team(4097)
    bc = np.array([(k, i, v, 0) for k, i, v in big_cols], lib.POSTCOL_DTYPE)
    bi, bv = np.array(list(big_map), np.int32), np.zeros(4097, np.int32)
    bvals = np.zeros((4097, 1, 2))
    rec, hl = np.zeros((1, 2), lib.SHAPE_DTYPE), np.full((1, 2, 32), 55, np.int32)
    rec["n"] = 77
    assert L.eagle_op_team_shape(0, vp(bvals), vp(bc), 1, 4097, vp(bi), vp(bv), 4097, vp(rec), vp(hl)) == lib.E_INVALID and L.eagle_last_error(None)
    assert (rec["n"] == 77).all() and (hl == 55).all()
    p8, hp1 = lib.minimap_params(2, 0, layers=8), lib.hull_params(1)
    assert L.eagle_op_minimap_hulls(0, vp(bvals), None, vp(bc), 1, 4097, vp(bi), vp(bv), 4097, C.byref(p8), C.byref(hp1), None, None, 0, None, None, 0, 0, 1, 0, None,
                                    vp(out)) == lib.E_INVALID and (out == 0x5A).all()
    assert L.eagle_op_team_shape(0, vp(bvals), vp(bc), 1, 4096, vp(bi), vp(bv), 4096, vp(rec), vp(hl)) == 0 and rec[0, 0]["n"] == 4096 and rec[0, 0]["hull_n"] == 1
    for args in ((None, vp(cols)), (vp(values), None)):
        assert L.eagle_op_team_shape(0, args[0], args[1], rows, len(cols), vp(ids), vp(vals), len(ids), None, None) == lib.E_INVALID
    assert L.eagle_op_team_shape(0, vp(values), vp(cols), rows, len(cols), None, None, 0, None, None) == lib.E_INVALID                  # no mapping
    assert L.eagle_op_team_shape(0, vp(values), vp(unknown), rows, len(cols), vp(ids), vp(vals), len(ids), None, None) == lib.E_INVALID
    assert op()[0] == 0 and not (out == 0x5A).all()
    out[:] = 0x5A
    # the handle entries
    case = post_cases.BY_NAME["goalkeeper_fold"]
    t = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, case["team_mapping"])
    bare = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, None)
    try:
        big = np.full(w * h * 3, 0x5A, np.uint8)

        def draw(layers):
            par = lib.minimap_params(2, 0, layers=layers)
            rc = L.eagle_minimap_frames(handle._h, t._t, 0, 1, C.byref(par), 0, None, vp(big))
            assert (big == 0x5A).all() or rc == 0
            return rc, L.eagle_last_error(handle._h).decode()

        rc, msg = draw(8)
        assert rc == lib.E_INVALID and "eagle_post_team_shape" in msg                                   # bit 8 without a result
        assert L.eagle_post_team_shape_values(t._t, None, None) == lib.E_INVALID
        handle.team_shape(t)
        rc, msg = draw(8)
        assert rc == lib.E_INVALID and "eagle_minimap_set_hulls" in msg                                 # ... without parameters
        for hw in (0, 9):
            assert L.eagle_minimap_set_hulls(t._t, C.byref(lib.hull_params(hw))) == lib.E_INVALID
        assert draw(8)[0] == lib.E_INVALID                                                              # (a refused set_hulls set nothing)
        handle.set_hulls(t, 1)
        assert draw(16)[0] == lib.E_INVALID and draw(9)[0] == lib.E_INVALID                             # an unknown bit; trails without their parameters
        assert (big == 0x5A).all()
        assert draw(8)[0] == 0
        handle.set_hulls(t, None)
        big[:] = 0x5A
        assert draw(8)[0] == lib.E_INVALID
        assert L.eagle_post_team_shape(handle._h, bare._t) == lib.E_INVALID and "mapping" in L.eagle_last_error(handle._h).decode()
        assert L.eagle_post_team_shape(handle._h, None) == lib.E_INVALID and L.eagle_post_team_shape(None, t._t) == lib.E_INVALID
    finally:
        t.close(); bare.close()


def test_cli_shape_and_hulls(tmp_path):
    from eagle_amd import cli
    out = str(tmp_path / "out")
    common = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed", "--minimap-scale", "2"]
    assert cli.main(common + ["--shape", "--minimap", "--minimap-hulls", "2"]) == 0
    rows = len(json.load(open(os.path.join(out, "processed_data.json"))))
    d = shape.from_json(json.load(open(os.path.join(out, "shape.json"))))
    assert len(d["rows"]) == rows and len(d["clip"]["groups"]) == 2
    w, h = R.size(2, 4)
    blob = open(os.path.join(out, "minimap.y4m"), "rb").read()
    assert len(blob.split(b"\n", 1)[1]) == rows * (6 + w * h * 3 // 2)
    assert cli.main(common + ["--minimap", "--minimap-hulls"]) == 0                                     # computes the shape itself
