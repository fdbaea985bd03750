"""Pass options on the GPU (include/eagle.h, eagle_pass_options_* / eagle_op_pass_options; csrc/options.hip): every output bit equals the numpy contract
of tests/options_ref.py — no tolerances — for the constructed tables of tests/options_cases.py (grids, options, every field of the row record, the sums
as exact int64); NULL grids and options; through a handle on a table eagle_postprocess built (host and device entries, merge_ids on and off); every
refusal; the CLI's three files; and the minimap, control and possession outputs of a table are the same before and after a pass-options call."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import options_cases as OC
import options_ref as OR
import post_cases
import stitch_cases
from eagle_amd import lib, postprocess, weights

pytestmark = pytest.mark.gpu


def _params(p):
    return lib.pass_option_params(p["R"], p["K"], p["t_react"], p["v_max"], p["beta"], p["v_ball"])


def _op(c, p, **kw):
    return lib.op_pass_options(c["values"], c["vel"], c["columns"], c["mapping"], c["cand"], c["owner"], _params(p), c["row0"], c["n"], **kw)


def _same_records(got, exp, what):
    assert got.dtype == OR.ROW_DTYPE and got.shape == exp.shape
    for k in OR.ROW_DTYPE.names:
        bad = np.flatnonzero(got[k] != exp[k])
        assert not len(bad), (what, k, bad[:5], got[k][bad[:5]], exp[k][bad[:5]])


@pytest.mark.parametrize("run", OC.RUNS, ids=OC.run_id)
def test_op_pass_options_equals_contract(run):
    c, p = OC.BY_NAME[run[0]], OC.BY_NAME[run[0]]["variants"][run[1]]
    exp_g, exp_r, exp_o = OC.reference(*run)
    g, recs, opt = _op(c, p)
    bad = np.argwhere(g != exp_g)
    assert g.shape == exp_g.shape and g.dtype == np.uint8 and not len(bad), (len(bad), bad[:5], g[tuple(bad[0])], exp_g[tuple(bad[0])])
    bad = np.argwhere(opt != exp_o)
    assert opt.shape == exp_o.shape and opt.dtype == np.int16 and not len(bad), (len(bad), bad[:5], opt[tuple(bad[0])], exp_o[tuple(bad[0])])
    _same_records(recs, exp_r, run)
    assert recs["sum"].dtype == np.int64 and np.array_equal(recs["sum"], exp_g.reshape(len(exp_g), -1).astype(np.int64).sum(1))


@pytest.mark.parametrize("name", ["sites22", "statuses", "rows65_window"])
def test_null_grid_and_null_options_leave_the_other_outputs(name):
    c, p = OC.BY_NAME[name], OC.BY_NAME[name]["variants"][0]
    exp_g, exp_r, exp_o = OC.reference(name, 0)
    no_sum = exp_r.copy()
    no_sum["sum"] = 0
    g, recs, opt = _op(c, p, grids=False)
    assert g is None and np.array_equal(opt, exp_o)
    _same_records(recs, no_sum, "no grid")
    g, recs, opt = _op(c, p, options=False)
    assert opt is None and np.array_equal(g, exp_g)
    _same_records(recs, exp_r, "no options")
    g, recs, opt = _op(c, p, grids=False, options=False)
    assert g is None and opt is None
    _same_records(recs, no_sum, "records only")


# ---- through a handle ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


def _fetch(d, nbytes):
    out = np.zeros(nbytes, np.uint8)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), d, nbytes, 2) == 0                       # hipMemcpyDeviceToHost
    return out


def _case(name):
    return post_cases.BY_NAME[name] if name in post_cases.BY_NAME else stitch_cases.BY_NAME[name]


SQUAD_MAPPING = {1: 0, 2: 1, 3: 0, 4: 1, 5: 0, 6: 1, 7: 0}


def _squad_records(n=20, seed=3):
    """n records (tools/control_rate.py's construction): seven players on a slow walk, a goalkeeper and a ball that follows player 1 and then player 3;
    the fifth player's track id changes from 5 to 15 half way (15 has no mapping entry: a site column only once merge_ids has stitched it to 5)"""
    r = np.random.default_rng(seed)
    players, k = 7, 9
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = k, 1, 1
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    pos = np.stack([r.uniform(25, 80, k), r.uniform(15, 55, k)], 1)[None] + np.cumsum(r.normal(0, 0.4, (n, k, 2)), 0)
    pos[:, k - 1] = np.where((np.arange(n) < n // 2)[:, None], pos[:, 0], pos[:, 2]) + 1.0
    d = recs["det"]
    j = np.arange(k)
    d["reported"][:, :k], d["in_bounds"][:, :k], d["conf"][:, :k] = 1, 1, 0.9
    d["cls"][:, :k] = np.where(j == k - 1, 2, np.where(j >= players, 1, 0))[None]
    d["id"][:, :k] = (j + 1)[None]
    d["id"][n // 2:, 4] = 15
    d["bx1"][:, :k], d["bx2"][:, :k], d["by1"][:, :k], d["by2"][:, :k] = (40 * j)[None], (40 * j + 30)[None], 300, 340
    d["pitch_x"][:, :k], d["pitch_y"][:, :k] = pos[..., 0].astype(np.int32), pos[..., 1].astype(np.int32)
    return recs


def _table(handle, name, merge=False):
    if name == "squad":
        return postprocess.process_data(handle, _squad_records(), 25, 1280, dict(SQUAD_MAPPING), merge_ids=merge), 25
    case = _case(name)
    return postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], case["team_mapping"], merge_ids=merge), case["fps"]


@pytest.mark.parametrize("name,merge", [("squad", True), ("squad", False), ("goalkeeper_fold", False), ("teams_head_inherits", True)], ids=lambda v: str(v))
def test_handle_pass_options_equals_contract(handle, name, merge):
    t, fps = _table(handle, name, merge)
    d_all = None
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        vel = handle.velocities(t, fps)
        active = 0
        for radius, min_hold, p in ((1024.0, 1, OR.params(1)), (40.0, 2, OR.params(2, 3, v_ball=20.0))):
            cand, owner, _, _ = handle.possession(t, lib.possession_params(fps, radius, min_hold, 1000))
            exp_g, exp_r, exp_o = OR.rows(values, vel, cols, t.team_mapping, cand, owner, 0, rows, p)
            site_cols = handle.pass_options_layout(t)
            assert site_cols.tolist() == [s[0] for s in OR.site_columns(cols, t.team_mapping)] == lib.pass_site_columns(t.columns, t.team_mapping).tolist()
            g, recs, opt = handle.pass_options(t, _params(p))
            assert np.array_equal(g, exp_g) and np.array_equal(opt, exp_o)
            _same_records(recs, exp_r, (name, radius))
            active += int(((exp_r["status"] == OR.ACTIVE) & (exp_r["n_mates"] > 0) & (exp_r["n_defenders"] > 0)).sum())
            assert exp_g.any() == bool(((exp_r["status"] == OR.ACTIVE) & (exp_r["n_mates"] > 0)).any())
            # a window, n == 0, and without grids
            g, recs, opt = handle.pass_options(t, _params(p), 2, rows - 3)
            assert np.array_equal(g, exp_g[2:rows - 1]) and np.array_equal(opt, exp_o[2:rows - 1])
            _same_records(recs, exp_r[2:rows - 1], "window")
            g, recs, opt = handle.pass_options(t, _params(p), rows, 0)
            assert g.shape[0] == 0 and len(recs) == 0 and opt.shape == (0, len(site_cols))
            g, recs, opt = handle.pass_options(t, _params(p), grids=False, options=False)
            assert g is None and opt is None and np.array_equal(recs["best_byte"], exp_r["best_byte"]) and not recs["sum"].any()
            # the device entry equals the host entry: the three outputs behind each other in one allocation, sentinels between and behind them
            gw, gh = lib.pass_options_size(_params(p))
            nb_g, nb_r, nb_o = rows * gw * gh, rows * 40, rows * len(site_cols) * 2
            off_r, off_o = (nb_g + 255) & ~255, ((nb_g + 255) & ~255) + ((nb_r + 255) & ~255)
            total = off_o + ((nb_o + 255) & ~255) + 256
            d_all = handle.upload(np.full(total, 0xA5, np.uint8))
            handle.pass_options_device(t, _params(p), C.c_void_p(d_all.value + off_r), 0, rows, d_all, C.c_void_p(d_all.value + off_o))
            raw = _fetch(d_all, total)
            assert np.array_equal(raw[:nb_g].reshape(rows, gh, gw), exp_g) and (raw[nb_g:off_r] == 0xA5).all()
            _same_records(raw[off_r:off_r + nb_r].view(OR.ROW_DTYPE), exp_r, "device")
            assert (raw[off_r + nb_r:off_o] == 0xA5).all() and (raw[off_o + nb_o:] == 0xA5).all()
            assert np.array_equal(raw[off_o:off_o + nb_o].view(np.int16).reshape(rows, -1), exp_o)
            handle.free(d_all)
            d_all = handle.upload(np.full(total, 0xA5, np.uint8))                                 # records only: nothing else is written
            handle.pass_options_device(t, _params(p), C.c_void_p(d_all.value + off_r), 1, rows - 1)
            raw = _fetch(d_all, total)
            no_sum = exp_r[1:].copy()
            no_sum["sum"] = 0
            _same_records(raw[off_r:off_r + nb_r - 40].view(OR.ROW_DTYPE), no_sum, "device, records only")
            assert (raw[:off_r] == 0xA5).all() and (raw[off_r + nb_r - 40:] == 0xA5).all()
            handle.free(d_all)
            d_all = None
            # the module: the event figures are the contract's
            from eagle_amd import options as op
            res = op.pass_options(handle, t, p["R"], p["K"], v_ball=p["v_ball"], rows=(1, rows - 1))
            assert np.array_equal(res["grids"], exp_g[1:]) and res["site_ids"] == [cols[c][1] for c in site_cols]
            ev = handle.events(t)
            passes = [k for k, e in enumerate(ev) if int(e["kind"]) == lib.EVENT_PASS]
            assert [f["event"] for f in res["events"]] == passes
            for f in res["events"]:
                e = OR.event_figures(ev[f["event"]], site_cols, exp_r[1:], exp_o[1:], 1)
                assert (f["chosen"], f["best_byte"], f["best_col"], f["rank"]) == (e if e[0] >= 0 else (-1, -1, None, None))
            json.dumps(op.to_json(res, t))
        print(name, merge, "columns", len(cols), "sites", len(site_cols), "merges", len(t.merges), "active rows with both sides over the two possession settings:", active)
        assert active > 0 or name != "squad", "no active row with attackers and defenders: the case does not exercise the kernels"
    finally:
        if d_all is not None:
            handle.free(d_all)
        t.close()


def test_other_outputs_of_the_table_are_unchanged_by_a_pass_options_call(handle):
    t, fps = _table(handle, "squad")
    try:
        handle.velocities(t, fps)
        pp = lib.possession_params(fps, 1024.0, 1, 1000)

        def outputs():
            mm = handle.minimap(t, lib.minimap_params(2, 2, voronoi=True))
            ct = handle.control(t, lib.control_params(1))
            po = handle.possession(t, pp)
            return [mm, ct[0], ct[1], np.array(t.values)] + list(po)

        before = outputs()
        g, recs, opt = handle.pass_options(t, lib.pass_option_params(2))
        assert (recs["status"] == OR.ACTIVE).any() and g.any()
        after = outputs()
        for a, b in zip(before, after):
            assert a.tobytes() == b.tobytes()
    finally:
        t.close()


def test_refusals(handle):
    L = handle.L
    c = OC.BY_NAME["statuses"]
    values, vel = np.ascontiguousarray(c["values"]), np.ascontiguousarray(c["vel"])
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    ids = np.array(list(c["mapping"]), np.int32)
    vals = np.array(list(c["mapping"].values()), np.int32)
    cand, owner = np.ascontiguousarray(c["cand"]), np.ascontiguousarray(c["owner"])
    rows, ncols = values.shape[1], len(cols)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    grid = np.full(rows * 7140, 0x5A, np.uint8)
    recs = np.full(rows * 40, 0x5A, np.uint8)
    opt = np.full(rows * 4, 0x5A5A, np.int16)
    good = lib.pass_option_params

    def op(params=good(), values_p=vp(values), vel_p=vp(vel), cols_p=vp(cols), ids_p=vp(ids), cand_p=vp(cand), owner_p=vp(owner), row0=0, n=1, recs_p=vp(recs), ncols=ncols):
        rc = L.eagle_op_pass_options(0, values_p, vel_p, cols_p, rows, ncols, ids_p, vp(vals), len(ids), cand_p, owner_p, None if params is None else C.byref(params),
                                     row0, n, vp(grid), recs_p, vp(opt))
        assert (grid == 0x5A).all() and (recs == 0x5A).all() and (opt == 0x5A5A).all()
        return rc, L.eagle_last_error(None).decode()

    bad_cand, bad_owner, low = cand.copy(), owner.copy(), owner.copy()
    bad_cand[3], bad_owner[5], low[0] = ncols, ncols + 7, -2
    two_balls = cols.copy()
    two_balls[4] = (lib.POST_BALL, 0, 0, 0)
    odd_kind = cols.copy()
    odd_kind[5]["kind"] = 9
    bad = [dict(params=None), dict(params=good(3)), dict(params=good(0)), dict(params=good(1, 0)), dict(params=good(1, 65)), dict(params=good(1, -1)),
           dict(params=good(t_react=-0.5)), dict(params=good(t_react=1001.0)), dict(params=good(v_max=0.0)), dict(params=good(v_max=2e6)), dict(params=good(beta=0.0)),
           dict(params=good(beta=-1.0)), dict(params=good(v_ball=0.0)), dict(params=good(v_ball=2e6)), dict(params=good(v_ball=float("nan"))),
           dict(values_p=None), dict(vel_p=None), dict(cols_p=None), dict(ids_p=None), dict(cand_p=None), dict(owner_p=None), dict(recs_p=None),
           dict(row0=rows, n=1), dict(row0=-1), dict(n=rows + 1), dict(n=-1), dict(row0=rows - 1, n=2),
           dict(cand_p=vp(bad_cand)), dict(owner_p=vp(bad_owner)), dict(owner_p=vp(low)), dict(cols_p=vp(two_balls)), dict(cols_p=vp(odd_kind))]
    for kw in bad:
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and msg, kw
    assert op(n=0)[0] == 0 and op(row0=rows, n=0)[0] == 0
    gw, gh = C.c_int(0), C.c_int(0)
    assert L.eagle_pass_options_size(C.byref(good(4)), C.byref(gw), C.byref(gh)) == 0 and (gw.value, gh.value) == (420, 272)
    assert L.eagle_pass_options_size(C.byref(good(3)), C.byref(gw), C.byref(gh)) == lib.E_INVALID
    assert L.eagle_pass_options_size(C.byref(good(1)), None, C.byref(gh)) == lib.E_INVALID and L.eagle_pass_options_size(None, C.byref(gw), C.byref(gh)) == lib.E_INVALID

    # 1025 site columns
    big = OC.BY_NAME["sites1025"]
    with pytest.raises(lib.EagleError, match="1025 site columns"):
        lib.op_pass_options(big["values"], big["vel"], big["columns"], big["mapping"], big["cand"], big["owner"], good(1, 2), options=False)

    # the handle entries: no mapping, no velocities, no possession, another handle's table, windows, parameters, NULL pointers
    case = post_cases.BY_NAME["goalkeeper_fold"]
    t = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, case["team_mapping"])
    bare = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, None)
    other = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    try:
        n_rows = len(t.rows)
        big_g = np.full(n_rows * 7140, 0x5A, np.uint8)
        big_r = np.full(n_rows * 40, 0x5A, np.uint8)
        big_o = np.full(n_rows * 64, 0x5A5A, np.int16)

        def hc(entry, h, table, params, row0, n, recs_p=vp(big_r)):
            rc = entry(h._h, table, row0, n, None if params is None else C.byref(params), vp(big_g), recs_p, vp(big_o))
            assert (big_g == 0x5A).all() and (big_r == 0x5A).all() and (big_o == 0x5A5A).all()
            return rc, L.eagle_last_error(h._h).decode()

        entries = (L.eagle_pass_options, L.eagle_pass_options_device)
        for entry in entries:
            rc, msg = hc(entry, handle, t._t, good(), 0, 1)
            assert rc == lib.E_INVALID and "velocities" in msg
        handle.velocities(t, 25); handle.velocities(bare, 25)
        for entry in entries:
            rc, msg = hc(entry, handle, t._t, good(), 0, 1)
            assert rc == lib.E_INVALID and "possession" in msg
        handle.possession(t, lib.possession_params(25)); handle.possession(bare, lib.possession_params(25))
        ns = C.c_int(-1)
        assert L.eagle_pass_options_layout(bare._t, None, 0, C.byref(ns)) == lib.E_INVALID and L.eagle_pass_options_layout(None, None, 0, C.byref(ns)) == lib.E_INVALID
        assert L.eagle_pass_options_layout(t._t, None, 0, None) == lib.E_INVALID and L.eagle_pass_options_layout(t._t, None, 3, C.byref(ns)) == lib.E_INVALID
        for entry in entries:
            rc, msg = hc(entry, handle, bare._t, good(), 0, 1)
            assert rc == lib.E_INVALID and "mapping" in msg
            rc, msg = hc(entry, other, t._t, good(), 0, 1)
            assert rc == lib.E_INVALID and "another handle" in msg
            for args in ((None, good(), 0, 1), (t._t, None, 0, 1), (t._t, good(3), 0, 1), (t._t, good(1, 0), 0, 1), (t._t, good(1, 65), 0, 1), (t._t, good(v_max=0.0), 0, 1),
                         (t._t, good(beta=0.0), 0, 1), (t._t, good(t_react=-1.0), 0, 1), (t._t, good(v_ball=0.0), 0, 1), (t._t, good(), 0, n_rows + 1),
                         (t._t, good(), n_rows, 1), (t._t, good(), -1, 1), (t._t, good(), 0, -1)):
                rc, msg = hc(entry, handle, *args)
                assert rc == lib.E_INVALID and msg, args
            assert hc(entry, handle, t._t, good(), 0, 1, recs_p=None)[0] == lib.E_INVALID
            assert hc(entry, handle, t._t, good(), n_rows, 0)[0] == 0 and hc(entry, handle, t._t, good(), 3, 0)[0] == 0
        g, recs, opt = handle.pass_options(t, good(), 0, 2)                          # the table and the handle still work
        assert g.shape == (2, 68, 105) and len(recs) == 2
    finally:
        t.close(); bare.close(); other.close()


def test_cli_pass_options(tmp_path, monkeypatch):
    """one CLI run; what it wrote is what the Python API returned inside it (the result is caught on its way through eagle_amd/options.py)"""
    from eagle_amd import cli, options as op
    seen = {}
    api, api_pictures = op.pass_options, op.pictures

    def caught(handle, table, *a, **kw):
        seen["result"] = api(handle, table, *a, **kw)
        seen["json"] = op.to_json(seen["result"], table)
        return seen["result"]

    def caught_pictures(*a, **kw):
        seen["pictures"] = api_pictures(*a, **kw)
        return seen["pictures"]

    monkeypatch.setattr(op, "pass_options", caught)
    monkeypatch.setattr(op, "pictures", caught_pictures)
    out = str(tmp_path / "out")
    common = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed"]
    assert cli.main(common + ["--pass-options", "--pass-options-grid", "2", "--pass-options-pictures", "--minimap-scale", "2"]) == 0
    rows = len(json.load(open(os.path.join(out, "processed_data.json"))))
    d = json.load(open(os.path.join(out, "pass_options.json")))
    g = np.load(os.path.join(out, "pass_options.npy"))
    res = seen["result"]
    assert d == json.loads(json.dumps(seen["json"])) and np.array_equal(g, res["grids"])
    assert g.shape == (rows, 136, 210) and g.dtype == np.uint8 and d["cells_per_metre"] == 2 and len(d["rows"]) == rows
    assert [r["status"] for r in d["rows"]] == [lib.PASS_STATUS_NAMES[s] for s in res["rows"]["status"]]
    assert all(set(r) == {"frame", "status", "owner_id", "best_id", "best_byte", "options"} for r in d["rows"])
    assert all(set(e) == {"event", "frame", "from_id", "to_id", "chosen", "best_byte", "best_id", "rank"} for e in d["events"])
    for r, row in enumerate(d["rows"]):
        assert row["options"] == {str(i): int(v) for i, v in zip(res["site_ids"], res["options"][r]) if v >= 0} and row["best_byte"] == res["rows"]["best_byte"][r]
        if row["status"] != "active":
            assert not g[r].any() and row["options"] == {} and row["best_id"] is None and row["best_byte"] == -1
    pics = sorted(f for f in os.listdir(out) if f.startswith("pass_options_") and f.endswith(".ppm"))
    assert pics == sorted("pass_options_%d.ppm" % k for k, _ in seen["pictures"]) and len(pics) == len(d["events"])
    for k, img in seen["pictures"]:
        blob = open(os.path.join(out, "pass_options_%d.ppm" % k), "rb").read()
        head = b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0])
        assert blob.startswith(head) and blob[len(head):] == np.ascontiguousarray(img[:, :, ::-1]).tobytes()
    with pytest.raises(SystemExit):
        cli.main(["--frames", "6", "--synthetic-weights", "--out", out, "--pass-options"])
    with pytest.raises(SystemExit):
        cli.main(common + ["--pass-options-grid", "2"])
