"""The space stage on the GPU (include/eagle.h, eagle_op_space / eagle_post_space / eagle_space_grids; csrc/space.hip): every field of every output
equals the contract of tests/space_ref.py — tobytes(), no tolerance — for the constructed tables of tests/space_cases.py, owner maps included; NULL
outputs and rows == 0; the first mapping entry counts; more rows than one launch of the cells kernel takes; every refusal leaves poisoned outputs alone;
through a handle on tables eagle_postprocess built (the result is kept, a second call replaces it, a refused call leaves it; windows of the owner maps
equal the whole, also over more than one staging pass, in host and in device memory; a result, a window beyond the table's memory budget is refused);
two runs give identical bytes; Processor.space; the command line's space.json and space.npy equal the contract computed on the table the run built."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

import possession_ref as PR
import space_cases as SC
import space_ref as SR
from eagle_amd import lib, space, weights

pytestmark = pytest.mark.gpu

vp = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
PARTS = ("rows", "sites", "totals", "maps")


def _equal(got, exp, what):
    for a, b, part in zip(got, exp, PARTS):
        if a.dtype.names:
            for k in a.dtype.names:
                assert np.array_equal(a[k], b[k]), (what, part, k)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, part)


@pytest.mark.parametrize("name", [c["name"] for c in SC.CASES])
def test_op_space_equals_contract(name):
    c = SC.BY_NAME[name]
    _equal(lib.op_space(c["values"], c["columns"], c["mapping"], lib.space_params(**c["p"]), 0, c["values"].shape[1]), SC.reference(name), name)


def test_two_runs_give_identical_bytes():
    c = SC.BY_NAME["walk_R4_4_rows_10_a_side"]
    a = lib.op_space(c["values"], c["columns"], c["mapping"], lib.space_params(**c["p"]), 0, 4)
    b = lib.op_space(c["values"], c["columns"], c["mapping"], lib.space_params(**c["p"]), 0, 4)
    _equal(a, b, "second run")


def _raw(c):
    values = np.ascontiguousarray(c["values"], np.float64)
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    ids = np.array(list(c["mapping"]), np.int32)
    vals = np.array(list(c["mapping"].values()), np.int32)
    return values, cols, ids, vals


def _poisoned(rows, nm, n=0, R=1):
    rec, st, tot = np.zeros(rows, lib.SPACE_ROW_DTYPE), np.zeros((rows, 32), lib.SPACE_SITE_DTYPE), np.zeros(nm, lib.SPACE_TOTALS_DTYPE)
    rec["n_sites"] = 77; st["col"] = 55; tot["rows"] = 66
    return rec, st, tot, np.full((n, 68 * R, 105 * R), 0x5A, np.uint8)


UNTOUCHED = (lambda rec: (rec["n_sites"] == 77).all() and not rec["cells"].any(), lambda st: (st["col"] == 55).all() and not st["cells"].any(),
             lambda tot: (tot["rows"] == 66).all() and not tot["cells"].any(), lambda grid: (grid == 0x5A).all())


def _untouched(*out):
    return all(f(a) for f, a in zip(UNTOUCHED, out))


def test_null_outputs_in_every_combination_windows_and_no_rows():
    L = lib.load()
    c = SC.BY_NAME["rows_65"]
    values, cols, ids, vals = _raw(c)
    rows, exp = values.shape[1], SC.reference("rows_65")
    p = lib.space_params(**c["p"])
    head = (0, vp(values), vp(cols), rows, len(cols), vp(ids), vp(vals), len(ids), C.byref(p))
    for want in itertools.product((False, True), repeat=4):
        out = _poisoned(rows, len(exp[2]), 5)
        assert L.eagle_op_space(*head, 60, 5, *[vp(a) if w else None for a, w in zip(out, want)]) == 0, want
        for a, b, w, alone in zip(out, exp[:3] + (exp[3][60:65],), want, UNTOUCHED):
            assert a.tobytes() == b.tobytes() if w else alone(a), want
    out = _poisoned(rows, len(exp[2]), 5)
    assert L.eagle_op_space(*head, 65, 0, *map(vp, out)) == 0 and UNTOUCHED[3](out[3]) and out[0].tobytes() == exp[0].tobytes()      # n == 0: no map is written
    out = _poisoned(rows, len(exp[2]), 5)
    assert L.eagle_op_space(0, vp(values), vp(cols), 0, len(cols), vp(ids), vp(vals), len(ids), C.byref(p), 0, 0, *map(vp, out)) == 0      # rows == 0: nothing written
    assert _untouched(*out)
    rec, st, tot, grid = lib.op_space(values[:, :0], c["columns"], c["mapping"], p)
    assert rec.shape == (0,) and st.shape == (0, 32) and tot.shape == (3,) and grid.shape == (0, 68, 105)


def test_first_mapping_entry_counts():
    L = lib.load()
    c = SC.BY_NAME["rows_63"]
    values, cols, ids, vals = _raw(c)
    ids2, vals2 = np.concatenate([ids, ids]).astype(np.int32), np.concatenate([vals, 3 - vals]).astype(np.int32)      # later, contradicting entries
    exp = SC.reference("rows_63")
    out = _poisoned(values.shape[1], len(exp[2]), 63)
    p = lib.space_params(**c["p"])
    assert L.eagle_op_space(0, vp(values), vp(cols), values.shape[1], len(cols), vp(ids2), vp(vals2), len(ids2), C.byref(p), 0, 63, *map(vp, out)) == 0
    _equal(out, exp, "first entry")
    _equal(lib.op_space(c["values"], c["columns"], dict(zip(ids2.tolist()[::-1], vals2.tolist()[::-1])), p, 0, 63), exp, "the wrapper's member count")


def test_more_rows_than_one_launch_of_the_cells_kernel():
    """65 537 rows: the cells kernel takes 65 535 per launch.  Three distinct rows repeat, so the contract is computed on three and tiled; the totals are
    the sums, minima and maxima of the tiled records"""
    c = SC.BY_NAME["radius_inclusive"]
    n = 65537
    idx = np.arange(n) % 3
    rec3, st3, _, _ = SC.reference("radius_inclusive")
    rec, st, tot, grid = lib.op_space(c["values"][:, idx], c["columns"], c["mapping"], lib.space_params(**c["p"]), 65534, 3)
    assert rec.tobytes() == rec3[idx].tobytes() and st.tobytes() == st3[idx].tobytes()
    assert grid.tobytes() == SC.reference("radius_inclusive")[3][idx[65534:]].tobytes()
    for m in (0, 1):
        s = st3[idx, m]
        total = s["cells"].sum(1)
        assert (tot[m]["col"], tot[m]["group"], tot[m]["rows"]) == (m, m, n) and [int(v) for v in tot[m]["cells"]] == [int(v) for v in s["cells"].astype(np.int64).sum(0)]
        assert (tot[m]["min"], tot[m]["max"], tot[m]["opp_rows"]) == (total.min(), total.max(), n)
        assert (tot[m]["within_rows"], tot[m]["within_sum"]) == ((s["within"] > 0).sum(), s["within"].sum())


def test_refusals_leave_the_outputs_alone():
    L = lib.load()
    c = SC.BY_NAME["goalkeepers_on"]
    values, cols, ids, vals = _raw(c)
    rows = values.shape[1]
    out = _poisoned(rows, 4, rows)

    def op(p=lib.space_params(), values_a=values, cols_a=cols, ids_a=ids, ncols=None, par=True, row0=0, n=rows):
        rc = L.eagle_op_space(0, vp(values_a), vp(cols_a), rows, len(cols) if ncols is None else ncols, vp(ids_a), vp(vals), len(ids), C.byref(p) if par else None, row0, n,
                              *map(vp, out))
        return rc, L.eagle_last_error(None).decode()

    unknown = cols.copy(); unknown[2]["kind"] = 9
    reserved = lib.space_params(); reserved.reserved[2] = 1
    for kw in (dict(par=False), dict(ids_a=None), dict(values_a=None), dict(cols_a=None), dict(cols_a=unknown), dict(p=reserved), dict(p=lib.space_params(0)),
               dict(p=lib.space_params(3)), dict(p=lib.space_params(8)), dict(p=lib.space_params(1, 1, 0.0)), dict(p=lib.space_params(1, 1, -2.0)),
               dict(p=lib.space_params(1, 1, float("nan"))), dict(p=lib.space_params(1, 1, float("inf"))), dict(p=lib.space_params(1, 1, 1024.5)), dict(ncols=-1),
               dict(row0=-1, n=1), dict(row0=0, n=rows + 1), dict(row0=rows, n=1), dict(row0=rows + 1, n=0), dict(n=-1)):
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and msg and _untouched(*out), kw
    # 4096 players and a goalkeeper are 4097 members; without the goalkeepers 4096 pass
    bc = np.array([(lib.POST_PLAYER, 1 + i, 0, 0) for i in range(4096)] + [(lib.POST_GOALKEEPER, 5000, 0, 0)], lib.POSTCOL_DTYPE)
    bi, bv, bvals = np.arange(1, 4097, dtype=np.int32), np.zeros(4096, np.int32), np.zeros((4097, 1, 2))
    big = _poisoned(1, 4097)
    p = lib.space_params()
    assert L.eagle_op_space(0, vp(bvals), vp(bc), 1, 4097, vp(bi), vp(bv), 4096, C.byref(p), 0, 0, *map(vp, big)) == lib.E_INVALID and _untouched(*big)
    p0 = lib.space_params(1, 0)
    assert L.eagle_op_space(0, vp(bvals), vp(bc), 1, 4097, vp(bi), vp(bv), 4096, C.byref(p0), 0, 0, *map(vp, big)) == 0
    assert big[0][0]["n_sites"] == 4096 and big[0][0]["status"] == lib.SPACE_TOO_MANY and list(big[0][0]["n"]) == [4096, 0, 0] and (big[1]["col"] == -1).all()
    assert (big[2][:4096]["rows"] == 0).all() and (big[2][:4096]["min"] == 0).all() and big[2][4095]["col"] == 4095
    assert op(p=lib.space_params(**c["p"]))[0] == 0
    _equal(out, SC.reference("goalkeepers_on"), "after the refusals")


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


def test_handle_keeps_replaces_and_leaves_the_result(handle):
    t = handle.postprocess(_walk_records(9, 12, 2), 25, 1280, {i + 1: i % 2 for i in range(12)})
    bare = handle.postprocess(_walk_records(9, 12, 2), 25, 1280, None)
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        assert handle.space_device(t) == (None, None, None, 0)
        assert handle.L.eagle_post_space_values(t._t, None, None, None) == lib.E_INVALID                       # no result yet
        p2 = SR.space_params(2, 1, 6.0)
        got = handle.space(t, lib.space_params(**p2))
        exp = SR.space(values, cols, t.team_mapping, p2, 0, rows)
        print("rows", rows, "members", len(got[2]), "sites", exp[0]["n_sites"].tolist(), "within rows", exp[2]["within_rows"].tolist())
        assert rows >= 3 and (exp[0]["status"] == SR.ACTIVE).sum() >= 3 and len(exp[2]) == 14 and exp[0]["n"][:, 2].max() == 2
        _equal(got, exp[:3], "handle")
        _equal(got, lib.op_space(values, cols, t.team_mapping, lib.space_params(**p2))[:3], "handle against the operator entry")
        maps = handle.space_grids(t, lib.space_params(**p2))
        assert maps.tobytes() == exp[3].tobytes()
        for row0, n in ((0, 1), (2, 3), (rows - 1, 1), (rows, 0)):
            assert handle.space_grids(t, lib.space_params(**p2), row0, n).tobytes() == exp[3][row0:row0 + n].tobytes(), (row0, n)
        a, b, c, n = handle.space_device(t)
        assert a and b and c and n == 14
        p1 = SR.space_params(1, 0, 3.0)
        second = handle.space(t, lib.space_params(**p1))                                                      # (no goalkeepers: other members, another result)
        _equal(second, SR.space(values, cols, t.team_mapping, p1)[:3], "second call")
        assert handle.space_device(t)[3] == 12 and second[0].tobytes() != got[0].tobytes()
        kept_at = handle.space_device(t)
        bad = lib.space_params(3)
        assert handle.L.eagle_post_space(handle._h, t._t, C.byref(bad)) == lib.E_INVALID and "cells_per_metre" in handle.L.eagle_last_error(handle._h).decode()
        bad = lib.space_params(1, 1, 0.0)
        assert handle.L.eagle_post_space(handle._h, t._t, C.byref(bad)) == lib.E_INVALID and "radius" in handle.L.eagle_last_error(handle._h).decode()
        assert handle.L.eagle_post_space(handle._h, t._t, None) == lib.E_INVALID
        g = np.full((1, 68, 105), 0x5A, np.uint8)
        ok = lib.space_params()
        for row0, n in ((-1, 1), (rows, 1), (0, rows + 1), (0, -1)):
            assert handle.L.eagle_space_grids(handle._h, t._t, row0, n, C.byref(ok), vp(g)) == lib.E_INVALID and (g == 0x5A).all(), (row0, n)
        assert handle.L.eagle_space_grids(handle._h, t._t, 0, 1, C.byref(bad), vp(g)) == lib.E_INVALID and (g == 0x5A).all()
        kept = _poisoned(rows, 12)[:3]
        assert handle.L.eagle_post_space_values(t._t, *map(vp, kept)) == 0                                    # the refused calls left the good result in place
        _equal(kept, second, "kept")
        assert handle.space_device(t) == kept_at
        assert np.array_equal(np.array(t.values), values, equal_nan=True)
        pr = lib.space_params()
        assert handle.L.eagle_post_space(handle._h, bare._t, C.byref(pr)) == lib.E_INVALID and "mapping" in handle.L.eagle_last_error(handle._h).decode()
        assert handle.space_device(bare) == (None, None, None, 0)
        assert handle.L.eagle_post_space(handle._h, None, C.byref(pr)) == lib.E_INVALID and handle.L.eagle_post_space(None, t._t, C.byref(pr)) == lib.E_INVALID
    finally:
        t.close(); bare.close()


def test_owner_maps_over_more_than_one_staging_pass(handle):
    """at 4 cells per metre a row's map and records take 115 840 bytes, so 32 MB of staging hold 289 rows: 300 rows are two passes.  The contract is
    computed for the rows round the seam and the ends; a window inside the second pass must equal the slice of the whole"""
    t = handle.postprocess(_walk_records(300, 3, 1), 25, 1280, {1: 0, 2: 1, 3: 0})
    try:
        rows = len(t.rows)
        assert rows >= 295
        values, cols = np.array(t.values), _columns(t)
        p4 = SR.space_params(4, 1, 3.0)
        maps = handle.space_grids(t, lib.space_params(**p4))
        assert maps.shape == (rows, 272, 420)
        for r in (0, 288, 289, 290, rows - 1):
            assert maps[r].tobytes() == SR.space(values[:, r:r + 1], cols, t.team_mapping, p4, 0, 1)[3].tobytes(), r
        assert handle.space_grids(t, lib.space_params(**p4), 285, 10).tobytes() == maps[285:295].tobytes()
    finally:
        t.close()


def _fetch(d, nbytes):
    out = np.zeros(nbytes, np.uint8)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d, nbytes, 2) == 0                       # hipMemcpyDeviceToHost
    return out


def test_what_is_beyond_the_table_s_budget_is_refused(handle):
    """a table of about 300 rows built with max_bytes = 400 000: the table itself needs (raw + kept columns) x rows x 16 bytes, well below that; a space
    result needs 1600 bytes per row (472 000 at 295 rows), the owner maps of all rows at one cell per metre 8740 per row in host form and the 1600 of the
    records in device form: all three are refused with the budget named, no result appears and the destinations keep their bytes.  Windows of 20 rows
    fit and equal the contract, in host and in device memory"""
    L = handle.L
    t = handle.postprocess(_walk_records(300, 3, 1), 25, 1280, {1: 0, 2: 1, 3: 0}, max_bytes=400_000)
    try:
        rows = len(t.rows)
        assert rows >= 295
        values, cols = np.array(t.values), _columns(t)
        p = lib.space_params()
        assert L.eagle_post_space(handle._h, t._t, C.byref(p)) == lib.E_INVALID and b"budget" in L.eagle_last_error(handle._h)
        assert handle.space_device(t) == (None, None, None, 0) and L.eagle_post_space_values(t._t, None, None, None) == lib.E_INVALID
        g = np.full((rows, 68, 105), 0x5A, np.uint8)
        assert L.eagle_space_grids(handle._h, t._t, 0, rows, C.byref(p), vp(g)) == lib.E_INVALID and b"budget" in L.eagle_last_error(handle._h) and (g == 0x5A).all()
        d = handle.upload(np.full(rows * 7140, 0xA5, np.uint8))
        try:
            assert L.eagle_space_device_grids(handle._h, t._t, 0, rows, C.byref(p), d) == lib.E_INVALID and b"budget" in L.eagle_last_error(handle._h)
            assert (_fetch(d, rows * 7140) == 0xA5).all()
            exp = SR.space(values[:, 100:120], cols, t.team_mapping, SR.space_params(), 0, 20)[3]
            assert handle.space_grids(t, p, 100, 20).tobytes() == exp.tobytes()
            handle.space_device_grids(t, p, C.c_void_p(d.value + 5 * 7140), 100, 20)
            raw = _fetch(d, rows * 7140)
            assert raw[5 * 7140:25 * 7140].tobytes() == exp.tobytes() and (raw[:5 * 7140] == 0xA5).all() and (raw[25 * 7140:] == 0xA5).all()
            assert L.eagle_space_device_grids(handle._h, t._t, 0, 1, C.byref(p), None) == lib.E_INVALID             # a NULL destination
        finally:
            handle.free(d)
        assert handle.space_device(t) == (None, None, None, 0)                                                 # the windows keep no result
    finally:
        t.close()


def test_processor_space_with_and_without_possession(handle):
    import types

    from eagle_amd.processor import Processor
    pr = Processor(types.SimpleNamespace(handle=handle))
    t = handle.postprocess(_walk_records(9, 12, 2), 25, 1280, {i + 1: i % 2 for i in range(12)})
    try:
        values, cols = np.array(t.values), _columns(t)
        p = SR.space_params(1, 1, 5.0)
        rec, st, tot, _ = SR.space(values, cols, t.team_mapping, p)
        d = pr.space(t, radius=5.0, per_row=True)
        assert d == space.derive(rec, st, tot, t.columns, lib.space_params(**p), t.rows, per_row=True) and "possession" not in d and len(d["ids"]) == 14
        cand, owner, dist, ev = handle.possession(t, lib.possession_params(25))
        d = pr.space(t, radius=5.0)
        assert d == space.derive(rec, st, tot, t.columns, lib.space_params(**p), t.rows, owner, ev) and "possession" in d and "passes" in d and "per_row" not in d
    finally:
        t.close()


def test_cli_space(tmp_path, monkeypatch):
    """the detections of a constructed walk of 12 players and 2 goalkeepers stand in for the random networks' (the model's records and the team mapping are
    substituted, as in test_gpu_stitch); the table each run builds is taken where Processor.process_data hands it to the command line; everything behind
    it is the command line's own path.
    space.json must be the contract's result on that table put through space.derive, space.npy the contract's owner maps"""
    from eagle_amd import cli, records
    from eagle_amd.coordinate_model import CoordinateModel
    from eagle_amd.processor import Processor
    recs = _walk_records(9, 12, 2)                                     # (the random networks see nobody: their rows would all be EMPTY)

    def get_coordinates(self, frames, fps, **kw):
        coords = {i: records.to_reference_dict(r, i, fps) for i, r in enumerate(recs)}
        self._last = (coords, recs, np.ones(len(recs), bool))
        return coords

    monkeypatch.setattr(CoordinateModel, "get_coordinates", get_coordinates)
    monkeypatch.setattr(Processor, "get_team_mapping", lambda self, frames, coords, pixel_format="bgr": {i + 1: i % 2 for i in range(12)})
    seen = []
    build = Processor.process_data

    def spy(self, *a, **kw):
        t, tm = build(self, *a, **kw)
        seen.append({"values": np.array(t.values), "cols": _columns(t), "columns": t.columns.copy(), "frames": t.rows.copy(), "mapping": t.team_mapping,
                     "no_ball": bool(t.flags & lib.POST_NO_BALL)})
        return t, tm

    monkeypatch.setattr(Processor, "process_data", spy)
    out = str(tmp_path / "out")
    common = ["--frames", "9", "--fps", "25", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed"]
    assert cli.main(common + ["--space", "--space-grid", "2", "--space-radius", "4.5", "--space-rows", "--space-map"]) == 0
    T = seen[-1]
    rows = len(json.load(open(os.path.join(out, "processed_data.json"))))
    p = SR.space_params(2, 1, 4.5)
    rec, st, tot, grid = SR.space(T["values"], T["cols"], T["mapping"], p, 0, rows)
    j = json.load(open(os.path.join(out, "space.json")))
    print("rows", rows, "sites", rec["n_sites"].tolist(), "members", len(tot))
    assert rows == len(T["frames"]) >= 3 and (rec["status"] == SR.ACTIVE).sum() >= 3 and len(tot) == 14
    assert j == space.to_json(space.derive(rec, st, tot, T["columns"], lib.space_params(**p), T["frames"], per_row=True))
    maps = np.load(os.path.join(out, "space.npy"))
    assert maps.dtype == np.uint8 and maps.shape == grid.shape and maps.tobytes() == grid.tobytes()
    assert cli.main(common + ["--space", "--possession"]) == 0
    T = seen[-1]
    p = SR.space_params()
    rec, st, tot, _ = SR.space(T["values"], T["cols"], T["mapping"], p)
    poss = PR.possession(T["values"], T["frames"], T["cols"], T["mapping"], 25, no_ball=T["no_ball"])
    j = json.load(open(os.path.join(out, "space.json")))
    assert j == space.to_json(space.derive(rec, st, tot, T["columns"], lib.space_params(**p), T["frames"], poss["owner"], poss["events"]))
    assert "per_row" not in j and "possession" in j and "passes" in j
